// Host program over csrc/ode_select.h (tests/test_ode_select_cpu.py): launch descriptions in, one line each out -- no device, no HIP call.
// A request is 23 integers:
//   S H T C L likelihood method B grid backward grad_mode with_ll force_loop force_generic alg pack enc_fuse x_ext particles Hc family zg head0
// family 0: no prior groups, no label heads; 1: the cvs split (two groups and two sigmoid heads of zg latent dims each); 2: the proc split (one
// group of 4 zg dims, four label heads of zg dims each, scored in the main loss); head0 > 0: label head 0 reads head0 latent dims instead.
// The answer is
//   S H BWD T_ C_ L_ Q_ M_ RA ONE ALG PK ENCF SOFTB grid nthreads lds | carved bound | the fourteen arguments ode_dispatch names for it
// or `refused: <text>`.  `carved` restates how ode_elbo_kernel lays out its dynamic LDS (its LdsMap from its own template arguments, the tanh
// rows of ENCF and the arrival counters of SOFTB behind the PK trajectories); `bound` is the block size the instantiation declares.
// The request `mapped` answers how many instantiations ode_dispatch names in all.
#include "../../structured_latent_odes_amd/csrc/ode_select.h"

#include <stdio.h>
#include <string.h>

alignas(64) static float g_mem[64];   // stands for every device buffer: non-NULL, never read or written

static int g_mapped = 0;
template <int S, int H, bool BWD, int T_, int C_, int L_, int Q_, int M_, bool RA, bool ONE, int ALG, int PK, bool ENCF, bool SOFTB>
struct Show {
  static inline const int id = ++g_mapped;   // one per instantiation of this template = per instantiation ode_dispatch names
  static OdeVariant run() {
    OdeVariant v{};
    v.shape = id;
    v.S = S; v.H = H; v.BWD = BWD; v.T_ = T_; v.C_ = C_; v.L_ = L_; v.Q_ = Q_; v.M_ = M_; v.RA = RA; v.ONE = ONE; v.ALG = ALG; v.PK = PK;
    v.ENCF = ENCF; v.SOFTB = SOFTB;
    return v;
  }
};

static void args14(const OdeVariant& v) {
  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", v.S, v.H, (int)v.BWD, v.T_, v.C_, v.L_, v.Q_, v.M_, (int)v.RA, (int)v.ONE, v.ALG, v.PK, (int)v.ENCF,
         (int)v.SOFTB);
}

// the dynamic LDS an instantiation lays out, in bytes: ode_elbo_kernel's `const LdsMap m = lds_map(...)` with its T, C, L, Q, n_stage_t, NT and
// COLDG, then s_ehid (ENCF: 64 floats per trajectory behind the PK maps) and s_sbar (SOFTB: behind those; the launch reserves 16 slots)
static size_t carved(const OdeVariant& v, const slode_shape& s, int npar, int n_aux_lds) {
  const int T = v.T_ ? v.T_ : s.T, C = v.C_ ? v.C_ : s.C, L = v.L_ ? v.L_ : s.L, Q = v.Q_ ? v.Q_ : (s.likelihood == SLODE_GAUSS ? 1 : 3);
  const int R = v.M_ >= 0 ? fixed_step_times(v.M_) : fixed_step_times(s.method);
  const int n_stage_t = (v.M_ >= 0 && v.T_) ? R * (T - 1) + 1 : fixed_step_times(s.method) * (s.T - 1) + 1;
  const int NT = v.T_ ? ode_threads_for(v.T_, v.Q_, v.C_, v.S) : v.nthreads;
  const bool COLDG = ode_cold_global(v.L_);
  const LdsMap m = lds_map(T, v.S, v.H, C, L, Q, n_stage_t, COLDG ? ode_hot_floats(v.S, v.H) : npar, NT, n_aux_lds, v.ONE, v.ALG == 3);
  size_t floats = (size_t)v.PK * m.total;
  if (v.ENCF) floats += (size_t)v.PK * 64;
  if (v.SOFTB) floats += 16;
  return floats * sizeof(float);
}

int main() {
  char line[512], err[512];
  while (fgets(line, sizeof(line), stdin)) {
    if (strncmp(line, "mapped", 6) == 0) { printf("%d\n", g_mapped); continue; }
    int f[23];
    int n = 0, used = 0;
    for (const char* p = line; n < 23 && sscanf(p, "%d%n", &f[n], &used) == 1; p += used) ++n;
    if (n != 23) { printf("bad request\n"); continue; }
    slode_shape s;
    memset(&s, 0, sizeof(s));
    s.S = f[0]; s.H = f[1]; s.T = f[2]; s.C = f[3]; s.L = f[4]; s.likelihood = f[5]; s.method = f[6]; s.B = f[7];
    s.grad_mode = f[10]; s.particles = f[18]; s.Hc = f[19];
    s.F = 10; s.K = 10; s.P = 5; s.quantile_diff = 0.475f; s.rtol = 1e-7f; s.atol = 1e-9f;
    const int family = f[20], zg = f[21], head0 = f[22];
    if (family == 1) {
      s.n_u = 2; s.n_groups = 2; s.groups[0] = slode_group{0, zg, 0, 1}; s.groups[1] = slode_group{zg, zg, 1, 1};
      s.n_aux = 2; s.U = 25; s.aux_mult = 1.f;
      s.aux[0] = slode_aux{SLODE_AUX_SIGMOID, 0, zg, 0, 1}; s.aux[1] = slode_aux{SLODE_AUX_SIGMOID, zg, zg, 1, 1};
    } else if (family == 2) {
      s.n_u = 9; s.n_groups = 1; s.groups[0] = slode_group{0, 4 * zg, 0, 9};
      s.n_aux = 4; s.U = 25; s.aux_mult = 1.f; s.aux_in_main = 1;
      s.aux[0] = slode_aux{SLODE_AUX_SOFTMAX, 0, zg, 0, 3}; s.aux[1] = slode_aux{SLODE_AUX_SOFTMAX, zg, zg, 3, 4};
      s.aux[2] = slode_aux{SLODE_AUX_EXPEXP, 2 * zg, zg, 7, 1}; s.aux[3] = slode_aux{SLODE_AUX_EXPEXP, 3 * zg, zg, 8, 1};
    }
    if (head0 > 0 && s.n_aux > 0) s.aux[0].z_dim = head0;
    OdeLaunch a{};
    a.s = s;
    if (slode_layout_init(&s, &a.lay) != SLODE_OK) { printf("bad shape\n"); continue; }
    a.params = g_mem; a.times = g_mem; a.stage_t = g_mem; a.loc = g_mem; a.scale = g_mem; a.eps = g_mem;
    a.grid = f[8]; a.backward = f[9]; a.with_ll = f[11]; a.force_loop = f[12]; a.force_generic = f[13]; a.alg = f[14]; a.pack = f[15];
    a.enc_fuse = f[16]; a.x_ext = f[17] ? g_mem : nullptr; a.particles = f[18];
    const int npar = a.lay.cstd - a.lay.ode_begin, n_aux_lds = s.aux_in_main ? s.n_aux : 0;
    err[0] = 0;
    const OdeVariant v = ode_select(a, npar, n_aux_lds, err, sizeof(err));
    if (!v.ok) { printf("refused: %s\n", err); continue; }
    args14(v);
    printf(" %d %d %zu | %zu %d | ", v.grid, v.nthreads, v.lds, carved(v, s, npar, n_aux_lds), ode_block_bound(v.S, v.T_, v.C_, v.Q_, v.ONE, v.BWD, v.PK));
    args14(ode_dispatch<Show>(v));
    printf("\n");
  }
  return 0;
}
