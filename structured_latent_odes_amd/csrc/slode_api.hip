// C ABI of libslode.so (include/slode.h): validation, parameter layout, workspace carving, launch orchestration.
#include "slode_common.h"
#include "fixed_step.h"
#include "ode_select.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

static thread_local char g_err[512] = "";
thread_local ClockTable* g_slode_clock = nullptr;

// scope of one profiled entry point: the kernels launched inside it fill the handle's clock table from slot 0
struct ClockScope {
  explicit ClockScope(slode_handle h, bool on) {
    if (on && h->profile && h->ev_ready) { h->clk.n = 0; g_slode_clock = &h->clk; }
  }
  ~ClockScope() { g_slode_clock = nullptr; }
};

static int fail(slode_handle h, int code, const char* fmt, ...) {
  char* dst = h ? h->err : g_err;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(dst, 512, fmt, ap);
  va_end(ap);
  if (h) snprintf(g_err, sizeof(g_err), "%s", h->err);
  return code;
}
#define HIP_TRY(h, expr)                                                                             \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return fail(h, SLODE_EHIP, "%s: %s", #expr, hipGetErrorString(e_));        \
  } while (0)

// Lanes per trajectory of the forward adaptive solve: sixteen while that leaves every wave a SIMD of its own (B / 4 waves <= 4 SIMDs per CU;
// the two lane groups of a trajectory share the stage evaluations: DESIGN 3.3, 94 against 101 us at B = 4096), eight beyond (the groups
// repeat the Runge-Kutta combination: more instructions in total, which is what counts once the SIMDs hold several waves).
static int dp5_lanes(const slode_ctx* h, int B) {
  if (h->dp5_w64) return h->dp5_w64;
  return (B + 3) / 4 <= 4 * h->num_cu ? 16 : 8;
}

static const char* method_name(int method) {
  static const char* const names[] = {"euler", "midpoint", "rk4", "dopri5", "bosh3", "fehlberg2", "adaptive_heun"};
  return method >= SLODE_EULER && method <= SLODE_ADAPTIVE_HEUN ? names[method] : "?";
}
// the adaptive methods: dopri5 and torchdiffeq's other RKAdaptiveStepsizeODESolver pairs (dopri5_kernel.hip)
static bool is_adaptive(int method) { return slode_is_adaptive(method); }

// particles of a step (slode_shape::particles; 0 and 1 both mean one)
static int particles_of(const slode_shape& s) { return s.particles > 1 ? s.particles : 1; }


static const char* check_shape(const slode_shape* s) {
  if (!s) return "shape is NULL";
  if (s->B < 1) return "B < 1";
  if (s->T < 2 || s->T > SLODE_MAX_T) return "T out of range [2, 1024]";
  if (s->C < 1 || s->C > SLODE_MAX_C) return "C (obs_dim) out of range [1, 4]";
  if (s->L < 1 || s->L > SLODE_MAX_L) return "L (latent dim) out of range [1, 64]";
  if (s->S < 1 || s->S > SLODE_MAX_S) return "S (ode_state_dim) out of range [1, 8]";
  if (s->H < 1 || s->H > SLODE_MAX_H) return "H (ode_hidden_dim) out of range [1, 32]";
  if (s->F < 1 || s->F > SLODE_MAX_F) return "F (n_filters) out of range [1, 16]";
  if (s->K < 1 || s->K > SLODE_MAX_K) return "K (filter_size) out of range [1, 16]";
  if (s->P < 1 || s->P > SLODE_MAX_P) return "P (pool_size) out of range [1, 8]";
  if (s->Hc < 1 || s->Hc > SLODE_MAX_HC) return "Hc (cnn_hidden_dim) out of range [1, 64]";
  if (s->T - s->K + 1 - s->P + 1 < 1) return "T too short for the conv/pool stack";
  if (s->n_u < 0 || s->n_u > SLODE_MAX_NU) return "n_u out of range [0, 16]";
  if (s->n_groups < 0 || s->n_groups > SLODE_MAX_GROUPS) return "n_groups out of range [0, 4]";
  for (int g = 0; g < s->n_groups; ++g) {
    const slode_group& gr = s->groups[g];
    if (gr.z_off < 0 || gr.z_dim < 1 || gr.z_off + gr.z_dim > s->L) return "prior group latent range outside [0, L)";
    if (gr.u_off < 0 || gr.u_dim < 1 || gr.u_off + gr.u_dim > s->n_u) return "prior group label range outside [0, n_u)";
    for (int g2 = 0; g2 < g; ++g2) {
      const slode_group& o = s->groups[g2];
      if (gr.z_off < o.z_off + o.z_dim && o.z_off < gr.z_off + gr.z_dim) return "prior groups overlap";
    }
  }
  if (s->method < SLODE_EULER || s->method > SLODE_ADAPTIVE_HEUN) return "unknown method (slode_method: 0 .. 6)";
  if (s->likelihood != SLODE_ALD && s->likelihood != SLODE_GAUSS) return "likelihood must be ALD or GAUSS";
  if (s->n_aux < 0 || s->n_aux > SLODE_MAX_AUX) return "n_aux out of range [0, 4]";
  if (s->n_aux > 0 && (s->U < 1 || s->U > 32)) return "U (u_hidden_dim) out of range [1, 32]";
  for (int a = 0; a < s->n_aux; ++a) {
    const slode_aux& x = s->aux[a];
    if (x.kind < SLODE_AUX_SIGMOID || x.kind > SLODE_AUX_EXPEXP) return "unknown aux head kind";
    if (x.z_off < 0 || x.z_dim < 1 || x.z_off + x.z_dim > s->L) return "aux head latent range outside [0, L)";
    if (x.u_off < 0 || x.u_dim < 1 || x.u_dim > 8 || x.u_off + x.u_dim > s->n_u) return "aux head label range outside [0, n_u) or wider than 8";
  }
  if (s->grad_mode != SLODE_GRAD_EXACT && s->grad_mode != SLODE_GRAD_REFERENCE_ADJOINT) return "grad_mode must be SLODE_GRAD_EXACT or SLODE_GRAD_REFERENCE_ADJOINT";
  if (s->particles < 0 || s->particles > SLODE_MAX_PARTICLES) return "particles out of range [0, 1024] (0 and 1: one particle)";
  if ((long long)s->B * (s->particles > 1 ? s->particles : 1) > 0x3fffffff) return "B x particles exceeds 2^30 - 1 trajectories";
  return nullptr;
}

extern "C" {

int slode_version(void) { return SLODE_VERSION; }

const char* slode_last_error(slode_handle h) { return h ? h->err : g_err; }

int slode_create(slode_handle* out, int device_id) {
  if (!out) return fail(nullptr, SLODE_EINVAL, "handle pointer is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return fail(nullptr, SLODE_EHIP, "no HIP device visible (%s); libslode has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (device_id < 0 || device_id >= n) return fail(nullptr, SLODE_EINVAL, "device_id %d outside [0, %d)", device_id, n);
  hipDeviceProp_t prop;
  HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, SLODE_EHIP, "device %d is %s; libslode is built for gfx950 only", device_id, prop.gcnArchName);
  slode_ctx* c = new slode_ctx();
  c->device = device_id;
  c->num_cu = prop.multiProcessorCount;
  c->err[0] = 0;
  c->profile = 0; c->ev_ready = 0; c->clk.n = 0;
  c->adam_lo2 = c->adam_hi2 = 0; c->adam_delta2 = 0;
  c->rng_seed = 0; c->rng_counter = 0; c->rng_b0 = 0;
  // the in-launch fold is a measured arm, off by default: it removes the 5.5 us fold launch and adds 6.0 us to the chain launch
  // (profiles/r04_c_ab*_fold_next_*.log)
  c->fold_on = getenv("SLODE_FOLD_NEXT") ? atoi(getenv("SLODE_FOLD_NEXT")) : 0;
  c->fold_valid = 0; c->fold_tmajor = 0; c->fold_ws = nullptr; c->fold_params = nullptr; c->fold_gen = 0;
  // (measured arms: 16 / 32 / 64 lanes per trajectory give the same bits and the same time, profiles/r04_f_ab11_*)
  c->dp5_w64 = getenv("SLODE_DP5_LPT") ? atoi(getenv("SLODE_DP5_LPT")) : 0;   // 0: by batch size (dp5_lanes: 16 while B / 4 <= 4 x CUs, else 8)
  c->chain_resident = 0; memset(c->chain_resident_sig, 0, sizeof(c->chain_resident_sig));
  // diagnostics and test hooks: the environment is read here, once per handle, never at launch time
  c->no_fold = getenv("SLODE_NO_FOLD") != nullptr;   // force the layer-by-layer encoder kernels
  c->ode_loop = getenv("SLODE_ODE_LOOP") != nullptr;
  c->ode_generic = getenv("SLODE_ODE_GENERIC") != nullptr;
  c->ode_alg = getenv("SLODE_ODE_ALG") ? atoi(getenv("SLODE_ODE_ALG")) : 0;
  c->enc_fuse = getenv("SLODE_ENC_FUSE") ? atoi(getenv("SLODE_ENC_FUSE")) : 1;
  c->ode_pack = getenv("SLODE_ODE_PACK") ? atoi(getenv("SLODE_ODE_PACK")) : 0;
  c->ode_grid_cap = getenv("SLODE_ODE_GRID") ? atoi(getenv("SLODE_ODE_GRID")) : 0;
  *out = c;
  return SLODE_OK;
}

int slode_destroy(slode_handle h) {
  if (h && h->ev_ready)
    for (int i = 0; i < SLODE_CLOCK_MAX; ++i) { (void)hipEventDestroy(h->clk.ev[i][0]); (void)hipEventDestroy(h->clk.ev[i][1]); }
  delete h;
  return SLODE_OK;
}

int slode_layout_init(const slode_shape* s, slode_layout* lay) {
  const char* why = check_shape(s);
  if (why) return fail(nullptr, SLODE_EINVAL, "%s", why);
  if (!lay) return fail(nullptr, SLODE_EINVAL, "layout pointer is NULL");
  memset(lay, 0, sizeof(*lay));
  const int n_conv = s->T - s->K + 1, FQ = s->F * (n_conv - s->P + 1);
  const int Q = s->likelihood == SLODE_GAUSS ? 1 : 3;
  int o = 0;
  lay->conv_w = o; o += s->F * s->C * s->K;
  lay->conv_b = o; o += s->F;
  lay->lin_w = o; o += s->Hc * FQ;
  lay->lin_b = o; o += s->Hc;
  lay->zloc_w = o; o += s->L * s->Hc;
  lay->zloc_b = o; o += s->L;
  lay->zls_w = o; o += s->L * s->Hc;
  lay->zls_b = o; o += s->L;
  lay->ode_begin = o;
  for (int g = 0; g < s->n_groups; ++g) {
    const slode_group& gr = s->groups[g];
    lay->ploc_w[g] = o; o += gr.z_dim * gr.u_dim;
    lay->ploc_b[g] = o; o += gr.z_dim;
    lay->pls_w[g] = o; o += gr.z_dim * gr.u_dim;
    lay->pls_b[g] = o; o += gr.z_dim;
  }
  lay->init_w1 = o; o += s->H * s->L;
  lay->init_b1 = o; o += s->H;
  lay->init_w2 = o; o += s->S * s->H;
  lay->init_b2 = o; o += s->S;
  lay->dyn_wh = o; o += s->H * (1 + s->L);
  lay->dyn_bh = o; o += s->H;
  lay->dyn_wg = o; o += s->S * s->H;
  lay->dyn_bg = o; o += s->S;
  lay->dyn_wd = o; o += s->S * s->H;
  lay->dyn_bd = o; o += s->S;
  for (int q = 0; q < SLODE_MAX_HEADS; ++q) {
    lay->head_w[q] = o;
    if (q < Q) o += s->C * s->S;
  }
  for (int a = 0; a < s->n_aux; ++a) {
    const slode_aux& x = s->aux[a];
    lay->aux_w1[a] = o; o += s->U * x.z_dim;
    lay->aux_b1[a] = o; o += s->U;
    lay->aux_w2[a] = o; o += x.u_dim * s->U;
    lay->aux_b2[a] = o; o += x.u_dim;
    if (x.kind == SLODE_AUX_EXPEXP) {
      lay->aux_w3[a] = o; o += x.u_dim * s->U;
      lay->aux_b3[a] = o; o += x.u_dim;
      lay->aux_c[a] = o; o += 1;
    }
  }
  lay->cstd = o; o += s->C * s->T;
  lay->ode_end = o;
  lay->n_params = o;
  return SLODE_OK;
}

int slode_num_stage_times(const slode_shape* s) {
  if (!s || s->T < 2) return SLODE_EINVAL;
  if (is_adaptive(s->method)) return 1;  // adaptive: no table (a 1-element dummy keeps callers uniform)
  return fixed_step_times(s->method) * (s->T - 1) + 1;
}

}  // extern "C"

// ---- workspace carving -------------------------------------------------------------------------------------
struct Workspace {
  float *loc, *scale, *pooled, *hid, *g_loc, *g_scale, *g_pre, *ode_slabs, *ode_part, *small_slabs, *small_part, *lin_slabs;
  float *weff, *rowsum, *wprime, *beff, *gslabs, *conv_slabs, *glat, *gslabs2, *gslabs3;  // folded encoder path
  unsigned int* counter;
  // dopri5 training: solution, dLoss/dx, external latent gradient, latent sample, step records
  float *dp_x, *dp_gx, *dp_gz, *dp_z, *dp_rec, *dp_snap, *dp_eps, *dp_tabs;
  float* sigtab;   // [4][C*T] likelihood-scale table of the step (OdeLaunch::sigtab)
  int* dp_nrec;
  int dp_kmax, dp_rows;
  int gsplit;
  int ode_grid, ode_stride, small_grid, small_stride, lin_splitk;
  size_t bytes;
};

static int ode_grid_for(slode_handle h, const slode_shape& s) {
  const int nthreads = slode_ode_threads(s);
  const size_t lds = slode_ode_lds_bytes(s, nthreads);
  int occ = lds ? (int)((160 * 1024) / lds) : 1;
  const int by_waves = 32 / (nthreads / 64);
  if (occ > by_waves) occ = by_waves;
  if (occ > 8) occ = 8;
  if (occ < 1) occ = 1;
  const int cus = h ? h->num_cu : 256;
  long long g = (long long)cus * occ;
  // One workgroup per trajectory up to 65,536 trajectories (the hardware queues the workgroups; one slab per trajectory);
  // beyond that (and under the SLODE_ODE_LOOP handle flag, which the persistent-loop tests set) a resident grid loops over them.
  // With K particles the grid is (g, K): g workgroups per particle over the B data rows, the same rule applied to the B * K virtual trajectories.
  const int K = particles_of(s);
  if ((long long)s.B * K <= 65536 && !(h && h->ode_loop)) g = s.B;
  else {
    if (K > 1) g = g / K > 0 ? g / K : 1;
    if (h && h->ode_grid_cap > 0 && g > h->ode_grid_cap) g = h->ode_grid_cap;
  }
  if (g > s.B) g = s.B;
  return (int)g;
}

// the Philox key / counter words of drawing call n on this handle (slode_common.h: RngK)
static RngK rng_of(const slode_ctx* h, uint64_t n) {
  RngK r{};
  r.k0 = (unsigned int)h->rng_seed; r.k1 = (unsigned int)(h->rng_seed >> 32);
  r.c2 = (unsigned int)n; r.c3 = (unsigned int)(n >> 32);
  r.b0 = h->rng_b0; r.on = 1;
  return r;
}

static size_t align_up(size_t v) { return (v + 63) & ~(size_t)63; }  // in floats: 256-byte alignment

// dopri5 training runs the fixed-grid ELBO kernel as the scorer of the adaptive solution (explicit Euler on the data grid as its
// placeholder solver: nothing flows through it) -- the shape that kernel, the grid and the workspace are sized for
static slode_shape scorer_shape(const slode_shape& s) {
  slode_shape e = s;
  if (is_adaptive(s.method)) { e.method = SLODE_EULER; e.grad_mode = SLODE_GRAD_EXACT; }
  return e;
}

static Workspace carve(slode_handle h, const slode_shape& s_in, const slode_layout& lay, void* base) {
  Workspace w{};
  const slode_shape s = scorer_shape(s_in);
  const bool dp5 = is_adaptive(s_in.method);
  // particles: K * B virtual trajectories (slode_common.h).  Per DATA row: loc, scale, pooled, hid.  Per VIRTUAL row: the latent and
  // pre-activation gradients (folded over the particles into rows [0, B) before the encoder backward), the slab rows (K grids) and
  // everything of the adaptive solve (sv: the shape its kernels see, B = K * B).
  const int K = particles_of(s);
  const size_t BK = (size_t)s.B * K;
  slode_shape sv = s; sv.B = (int)BK; sv.particles = 0;
  w.dp_rows = dp5 ? slode_dopri5_rows(sv) : 0;
  const int n_conv = s.T - s.K + 1, FQ = s.F * (n_conv - s.P + 1);
  w.ode_grid = ode_grid_for(h, s);
  w.ode_stride = (int)align_up((size_t)(lay.ode_end - lay.ode_begin) + 1);
  w.small_grid = slode_enc_bwd_grid(s);
  w.small_stride = (int)align_up((size_t)slode_enc_small_count(s));
  w.lin_splitk = slode_enc_lin_splitk(s);
  size_t o = 0;
  float* b = (float*)base;
  auto take = [&](size_t n) { float* p = b ? b + o : nullptr; o += align_up(n); return p; };
  w.loc = take((size_t)s.B * s.L);
  w.scale = take((size_t)s.B * s.L);
  w.pooled = take((size_t)s.B * FQ);
  w.hid = take((size_t)s.B * s.Hc);
  w.g_loc = take(BK * s.L);
  w.g_scale = take(BK * s.L);
  w.g_pre = take(BK * 64);
  w.ode_slabs = take(((size_t)w.ode_grid * K + w.dp_rows) * w.ode_stride);   // dopri5: its backward kernel's rows follow the scorer's
  w.ode_part = take((size_t)SLODE_REDUCE_GROUPS * w.ode_stride);
  w.small_slabs = take((size_t)w.small_grid * w.small_stride);
  w.small_part = take((size_t)SLODE_REDUCE_GROUPS * w.small_stride);
  w.lin_slabs = take((size_t)w.lin_splitk * s.Hc * FQ);
  w.gsplit = w.lin_splitk;
  w.weff = take((size_t)s.Hc * s.C * s.T);
  w.rowsum = take((size_t)s.Hc * s.F);
  w.wprime = take((size_t)s.F * s.C * (s.K + s.P));
  w.beff = take(64);
  w.gslabs = take((size_t)w.gsplit * s.Hc * (s.C * s.T + 1));
  w.conv_slabs = take((size_t)s.Hc * (s.F * s.C * s.K + s.F));
  w.glat = take(BK * 128);
  w.gslabs2 = take((size_t)w.gsplit * s.L * (s.Hc + 1));
  w.gslabs3 = take((size_t)w.gsplit * s.L * (s.Hc + 1));
  w.counter = reinterpret_cast<unsigned int*>(take(32 * (16 + SLODE_MAX_HC)));   // arrival counters 128 B apart: one per conv-filter pair (0..7), the in-launch fold's (8, 9, 16 + m)
  w.sigtab = take(4 * (size_t)s.C * s.T);
  if (dp5) {
    w.dp_kmax = slode_dopri5_kmax(sv);
    w.dp_x = take(BK * s.T * s.S);
    w.dp_gx = take(BK * s.T * s.S);
    w.dp_gz = take(BK * s.L);
    w.dp_z = take(BK * s.L);
    w.dp_nrec = reinterpret_cast<int*>(take(BK));
    w.dp_rec = take((size_t)w.dp_kmax * BK * (s.S + 2));
    w.dp_tabs = take((size_t)slode_dopri5_rows(sv) * slode_dopri5_tab_floats(s));   // the forward kernel's set-up tables, handed to the reverse sweep
    w.dp_snap = take(BK * 2 * s.H * 4 * s.S);   // running sums parked at the hidden units' switching times, per lane group (dopri5_kernel.hip)
    w.dp_eps = take(BK * s.L);              // the noise the forward kernel drew (eps == NULL), for the scorer and the reverse sweep
  }
  w.bytes = o * sizeof(float);
  return w;
}

// Data-parallel payload (slode_grad_partial -> all-reduce -> slode_grad_apply): everything the chain rule + tail need of the batch,
// [G = g_pre^T [X | 1]: Hc x (CT + 1)] [glat_loc^T [hid | 1]: L x (Hc + 1)] [glat_ls^T [hid | 1]: L x (Hc + 1)] [loss | ODE-half row],
// each piece starting on a 16-byte boundary.  The chain rule is linear in G, so reducing G over the ranks and chain-ruling once gives the
// gradient of the global batch: 34 k floats instead of the 96 k of the flat gradient at the metric shape.
struct PayloadMap { int g_loc, g_ls, ode, total; };
static PayloadMap payload_map(const slode_shape& s, int part_floats) {
  auto a4 = [](int v) { return (v + 3) & ~3; };
  PayloadMap m;
  m.g_loc = a4(s.Hc * (s.C * s.T + 1));
  m.g_ls = m.g_loc + a4(s.L * (s.Hc + 1));
  m.ode = m.g_ls + a4(s.L * (s.Hc + 1));
  m.total = m.ode + a4(part_floats + 1);
  return m;
}

static int batch_labels(slode_handle h, const slode_shape* s, const slode_batch* batch, LabelSrc* lab) {
  if (batch->n_labels < 0 || batch->n_labels > SLODE_MAX_LABELS) return fail(h, SLODE_EINVAL, "n_labels out of range [0, %d]", SLODE_MAX_LABELS);
  lab->n = batch->n_labels;
  int cols = 0;
  for (int i = 0; i < batch->n_labels; ++i) {
    if (!batch->labels[i] || batch->label_width[i] < 1) return fail(h, SLODE_EINVAL, "label tensor %d is NULL or has width < 1", i);
    lab->p[i] = batch->labels[i]; lab->off[i] = cols; cols += batch->label_width[i];
  }
  for (int i = batch->n_labels; i <= SLODE_MAX_LABELS; ++i) lab->off[i] = cols;
  if (batch->n_labels > 0 && cols != s->n_u)
    return fail(h, SLODE_EINVAL, "the label tensors have %d columns in all, the shape's n_u is %d", cols, s->n_u);
  return SLODE_OK;
}

static const char* check_common(slode_handle h, const slode_shape* s, const slode_layout* lay, const void* params) {
  if (!h) return "handle is NULL";
  const char* why = check_shape(s);
  if (why) return why;
  if (!lay) return "layout is NULL";
  if (!params) return "params is NULL";
  return nullptr;
}

extern "C" {

size_t slode_workspace_bytes(slode_handle h, const slode_shape* s) {
  slode_layout lay;
  if (slode_layout_init(s, &lay) != SLODE_OK) return 0;
  return carve(h, *s, lay, nullptr).bytes;
}

int slode_stage_times(slode_handle h, const slode_shape* s, const float* times, float* stage_t, void* stream) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  const char* why = check_shape(s);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!times || !stage_t) return fail(h, SLODE_EINVAL, "times / stage_t is NULL");
  HIP_TRY(h, slode_launch_stage_times(*s, times, stage_t, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_encoder_conv_fwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                           const float* obs, const int64_t obs_strides[3], float* loc, float* scale, float* pooled,
                           float* hid, void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!obs || !obs_strides || !loc || !scale) return fail(h, SLODE_EINVAL, "obs / obs_strides / loc / scale is NULL");
  EncLaunch a{*s, *lay, params, obs, obs_strides[0], obs_strides[1], obs_strides[2], loc, scale, pooled, hid};
  hipError_t e = slode_launch_enc_fwd(a, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(h, SLODE_EINVAL, "encoder kernels are instantiated for (obs_dim, filter_size) in {(3,10),(4,10)} and need "
                                 "the tile to fit 160 KiB of LDS; got C=%d K=%d T=%d", s->C, s->K, s->T);
  HIP_TRY(h, e);
  return SLODE_OK;
}

int slode_encoder_conv_bwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                           const float* obs, const int64_t obs_strides[3], const float* scale, const float* pooled,
                           const float* hid, const float* g_loc, const float* g_scale, float* grads, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!obs || !obs_strides || !scale || !pooled || !hid || !g_loc || !g_scale || !grads || !workspace)
    return fail(h, SLODE_EINVAL, "a required pointer is NULL");
  Workspace w = carve(h, *s, *lay, workspace);
  if (workspace_bytes < w.bytes) return fail(h, SLODE_ENOSPC, "workspace %zu B < required %zu B", workspace_bytes, w.bytes);
  EncBwdLaunch a{*s, *lay, params, obs, obs_strides[0], obs_strides[1], obs_strides[2], scale, pooled, hid, g_loc, g_scale,
                 w.g_pre, w.small_slabs, w.small_stride, w.small_grid, w.lin_slabs, w.lin_splitk};
  hipError_t e = slode_launch_enc_bwd(a, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(h, SLODE_EINVAL, "unsupported encoder shape C=%d K=%d T=%d", s->C, s->K, s->T);
  HIP_TRY(h, e);
  ReduceLaunch r{};
  r.s = *s; r.lay = *lay; r.small_slabs = w.small_slabs; r.small_stride = w.small_stride; r.small_n = w.small_grid; r.small_part = w.small_part;
  r.lin_slabs = w.lin_slabs; r.lin_n = w.lin_splitk; r.grads = grads;
  HIP_TRY(h, slode_launch_reduce(r, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_ode_solve_fwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                        const float* times, const float* stage_t, const float* z, float* x, void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!times || !z || !x) return fail(h, SLODE_EINVAL, "times / z / x is NULL");
  if (is_adaptive(s->method)) {  // adaptive solve: per-trajectory controller, no stage-time table
    DopriRec plain{};   // (no guide sample, no records: a bare solve) -- carries the handle's choice of forward kernel
    plain.w64 = dp5_lanes(h, s->B);
    if (!slode_dp5_lanes_ok(s->method, plain.w64))
      return fail(h, SLODE_EINVAL, "%s: SLODE_DP5_LPT=%d is not instantiated (8 or 16; 32 / 64 are dopri5 only)", method_name(s->method), plain.w64);
    hipError_t e5 = slode_launch_dopri5(*s, *lay, params, times, z, x, (hipStream_t)stream, &plain);
    if (e5 == hipErrorInvalidValue) return fail(h, SLODE_EINVAL, "%s kernel is instantiated for (S,H) in {(5,25),(8,25)}", method_name(s->method));
    HIP_TRY(h, e5);
    return SLODE_OK;
  }
  if (!stage_t) return fail(h, SLODE_EINVAL, "stage_t is NULL");
  const int grid = ode_grid_for(h, *s);
  OdeLaunch a{};
  a.s = *s; a.lay = *lay; a.params = params; a.times = times; a.stage_t = stage_t; a.z_in = z; a.x_out = x;
  a.slabs = nullptr; a.slab_stride = 0; a.grid = grid; a.backward = 0; a.with_ll = 0;   // pure solve: no loss slot, nothing allocated
  a.force_loop = h->ode_loop; a.force_generic = h->ode_generic;
  hipError_t e = slode_launch_ode(a, (hipStream_t)stream, h->err, sizeof(h->err));
  if (e == hipErrorInvalidValue) return SLODE_EINVAL;
  HIP_TRY(h, e);
  return SLODE_OK;
}

int slode_ode_solve_bwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                        const float* times, const float* stage_t, const float* z, const float* g_x, float* g_z,
                        float* grads, void* workspace, size_t workspace_bytes, void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!times || !stage_t || !z || !g_x || !g_z || !grads || !workspace) return fail(h, SLODE_EINVAL, "a required pointer is NULL");
  if (is_adaptive(s->method))
    return fail(h, SLODE_EINVAL, "%s is forward-only (slode_ode_solve_fwd); gradients need a fixed-grid method", method_name(s->method));
  Workspace w = carve(h, *s, *lay, workspace);
  if (workspace_bytes < w.bytes) return fail(h, SLODE_ENOSPC, "workspace %zu B < required %zu B", workspace_bytes, w.bytes);
  OdeLaunch a{};
  a.s = *s; a.lay = *lay; a.params = params; a.times = times; a.stage_t = stage_t; a.z_in = z; a.gx_in = g_x;
  a.g_loc = g_z; a.slabs = w.ode_slabs; a.slab_stride = w.ode_stride; a.grid = w.ode_grid; a.backward = 1; a.with_ll = 0;
  a.force_loop = h->ode_loop; a.force_generic = h->ode_generic;
  hipError_t e = slode_launch_ode(a, (hipStream_t)stream, h->err, sizeof(h->err));
  if (e == hipErrorInvalidValue) return SLODE_EINVAL;
  HIP_TRY(h, e);
  ReduceLaunch r{};
  r.s = *s; r.lay = *lay; r.ode_slabs = w.ode_slabs; r.ode_stride = w.ode_stride; r.ode_n = w.ode_grid; r.ode_part = w.ode_part; r.grads = grads;
  HIP_TRY(h, slode_launch_reduce(r, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_decode_heads(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* x,
                       float* mu, float* std_ct, void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!x || !mu) return fail(h, SLODE_EINVAL, "x / mu is NULL");
  HIP_TRY(h, slode_launch_decode_heads(*s, *lay, params, x, mu, std_ct, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_decode_heads_bwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* x,
                           const float* g_mu, const float* g_std, float* g_x, float* g_heads, float* g_cstd, void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!x || !g_mu || !g_x || !g_heads) return fail(h, SLODE_EINVAL, "x / g_mu / g_x / g_heads is NULL");
  HIP_TRY(h, slode_launch_decode_heads_bwd(*s, *lay, params, x, g_mu, g_std, g_x, g_heads, g_cstd, (hipStream_t)stream));
  return SLODE_OK;
}

}  // extern "C"

// ---- the ELBO step: one call description, four stages.  Data parallel (slode_grad_partial / slode_grad_apply): STEP_PARTIAL = up to the
// split-K products, packed into `payload` = [G | G_loc | G_ls | loss | ODE-half row]; STEP_APPLY = chain rule + tail (+ Adam) from it.
enum StepPhase { STEP_WHOLE = 0, STEP_PARTIAL = 1, STEP_APPLY = 2 };
struct StepCall {
  int kind = SLODE_SVI_MAIN, phase = STEP_WHOLE;   // kind SLODE_SVI_MAIN: the ELBO; SLODE_SVI_AUX: the auxiliary label-head loss
  const float *params = nullptr, *times = nullptr, *stage_t = nullptr, *obs = nullptr, *u = nullptr, *eps = nullptr;
  const int64_t* obs_strides = nullptr; void* workspace = nullptr; size_t workspace_bytes = 0; hipStream_t stream = nullptr;
  float *loss_out = nullptr, *grads = nullptr, *x_out = nullptr, *z_out = nullptr, *payload = nullptr;
  int no_loss = 0;   // 1: a forward-only set-up that writes no loss (slode_recon_moments): loss_out may be NULL
  AdamHost adam{}; LabelSrc lab{};   // fused Adam (adam_args; adam.p == nullptr: none); label tensors one by one (batch_labels; n == 0: u)
};
struct Step {   // what the stages share, worked out once by step_setup
  slode_handle h; const slode_shape& s; const slode_layout& lay; const StepCall& c;
  bool aux = false, dp5 = false, bwd = false, folded = false, t_major = false;
  int K = 1;   // particles (slode_shape::particles): K * B virtual trajectories, particle-major (slode_common.h)
  RngK rng{}; const float* u = nullptr; Workspace w{};
};
// the slab rows the tail reduces: n rows of [loss | flat elements [part_lo, part_hi)]; rows [0, zr_rows) carry nothing in slab columns
// [zr_lo, zr_hi) (the dopri5 scorer's rows: Stage1::zr_*)
struct SlabRows { int n, part_lo, part_hi, zr_rows = 0, zr_lo = 0, zr_hi = 0; };

// The optional Adam arguments of a step entry point: checked (the message names `who`) and converted once, with the handle's Adam region.
static int adam_args(slode_handle h, const char* who, const char* moments, const slode_layout* lay, float* params, const slode_adam* a, StepCall* c) {
  if (!a) return SLODE_OK;
  if (!c->grads || !a->exp_avg || !a->exp_avg_sq || a->step < 1 || !lay || a->n_total < lay->n_params)
    return fail(h, SLODE_EINVAL, "%s needs grads, %s moments, step >= 1 and n_total >= layout n_params", who, moments);
  c->adam = AdamHost{params, a->exp_avg, a->exp_avg_sq, a->lr, a->beta1, a->beta2, a->eps, a->step, a->n_total};
  if (h) { c->adam.lo2 = h->adam_lo2; c->adam.hi2 = h->adam_hi2; c->adam.delta2 = h->adam_delta2; }   // (no handle: the step refuses the call)
  return SLODE_OK;
}

// handle, kind and batch of slode_svi_step / slode_grad_partial checked; the batch (observations, label tensors, noise) into the call
static int batch_call(slode_handle h, const slode_shape* s, int kind, const slode_batch* batch, StepCall* c) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (!s || !batch) return fail(h, SLODE_EINVAL, "shape / batch is NULL");
  if (kind != SLODE_SVI_MAIN && kind != SLODE_SVI_AUX) return fail(h, SLODE_EINVAL, "kind must be SLODE_SVI_MAIN or SLODE_SVI_AUX");
  c->kind = kind; c->obs = batch->obs; c->obs_strides = batch->obs_strides; c->eps = batch->eps;
  return batch_labels(h, s, batch, &c->lab);
}

// ext_skip assumes slode_layout_init's order: the ten solver-side tensors tile [init_w1, dyn_bd + S) exactly and nothing else (prior
// nets, decoder heads, label heads, constant_std) lies inside; a caller-made layout that does not keeps the zeros written and read
static bool solver_contig(const slode_shape& s, const slode_layout& lay) {
  bool ok = lay.init_b1 == lay.init_w1 + s.H * s.L && lay.init_w2 == lay.init_b1 + s.H && lay.init_b2 == lay.init_w2 + s.S * s.H &&
            lay.dyn_wh == lay.init_b2 + s.S && lay.dyn_bh == lay.dyn_wh + s.H * (1 + s.L) && lay.dyn_wg == lay.dyn_bh + s.H &&
            lay.dyn_bg == lay.dyn_wg + s.S * s.H && lay.dyn_wd == lay.dyn_bg + s.S && lay.dyn_bd == lay.dyn_wd + s.S * s.H;
  const int lo = lay.init_w1, hi = lay.dyn_bd + s.S;
  auto inside = [&](int off) { return off >= lo && off < hi; };
  for (int g = 0; g < s.n_groups; ++g)
    ok = ok && !inside(lay.ploc_w[g]) && !inside(lay.ploc_b[g]) && !inside(lay.pls_w[g]) && !inside(lay.pls_b[g]);
  for (int q = 0; q < (s.likelihood == SLODE_GAUSS ? 1 : 3); ++q) ok = ok && !inside(lay.head_w[q]);
  for (int a = 0; a < s.n_aux; ++a)
    ok = ok && !inside(lay.aux_w1[a]) && !inside(lay.aux_b1[a]) && !inside(lay.aux_w2[a]) && !inside(lay.aux_b2[a]) &&
         (s.aux[a].kind != SLODE_AUX_EXPEXP || (!inside(lay.aux_w3[a]) && !inside(lay.aux_b3[a]) && !inside(lay.aux_c[a])));
  return ok && !inside(lay.cstd);
}

// ---- in-launch fold (SLODE_FOLD_NEXT, a measured arm, off by default: DESIGN 5) ----------------------------------------------------
// The fold launch.  The previous weight-updating step on this (workspace, params) left W_eff / b_eff / rowsum / w' / the likelihood-scale
// table of the CURRENT weights behind (enc_chain_kernel, FOLD-NEXT): then the encoder forward alone, or nothing when the ODE kernel runs it.
// Anything else -- first step, another workspace, weights changed outside this handle (slode_fold_invalidate) -- folds here, which also
// zeroes the in-launch fold's arrival counter.
static int fold_fwd(slode_handle h, const StepCall& c, FoldLaunch& fl, bool enc_fused) {
  const bool have_fold = h->fold_on && h->fold_valid && h->fold_ws == c.workspace && h->fold_params == (const void*)c.params && h->fold_tmajor == fl.t_major;
  if (have_fold && enc_fused) return SLODE_OK;
  fl.fold_skip = have_fold ? 1 : 0;
  HIP_TRY(h, slode_launch_fold_fwd(fl, c.stream));
  if (!have_fold) { h->fold_gen = 0; h->fold_valid = 1; h->fold_ws = c.workspace; h->fold_params = c.params; h->fold_tmajor = fl.t_major; }
  return SLODE_OK;
}
// The chain launch updates the weights (Adam inside) => it also folds them for the next step, provided every block of the launch is resident
// at once (the blocks wait for each other) and the handle's W_eff bookkeeping covers this workspace: tl.fold_next / n_riders / done_target.
static void fold_next_plan(slode_ctx* h, const slode_shape& s, const slode_layout& lay, const StepCall& c, TailK& tl) {
  int n_chain = 0, resident = 0, nblk = slode_chain_blocks(s, tl.n_total, lay.lin_b, &n_chain);
  if (h->fold_on && c.adam.p) {   // (the occupancy query is asked once per shape and handle)
    const int sig[8] = {s.T, s.C, s.F, s.K, s.P, s.Hc, s.L, lay.n_params};
    if (memcmp(sig, h->chain_resident_sig, sizeof(sig)) != 0) {
      h->chain_resident = slode_chain_resident_blocks(s, h->num_cu);
      memcpy(h->chain_resident_sig, sig, sizeof(sig));
    }
    resident = h->chain_resident;
  }
  if (nblk > resident && resident > n_chain && nblk - n_chain <= 4 * (resident - n_chain)) nblk = resident;   // fewer, looping riders: the grid fits
  const bool fold_next = h->fold_on && c.adam.p && c.adam.p == c.params && nblk <= resident && h->fold_valid && h->fold_ws == c.workspace &&
                         h->fold_params == (const void*)c.params;
  tl.fold_next = fold_next ? 1 : 0;
  tl.n_riders = fold_next ? nblk - n_chain : 0;
  tl.done_target = fold_next ? ++h->fold_gen : 0;   // (the generation: every counter's target is gen x its number of arrivals per launch)
  if (c.adam.p) h->fold_valid = fold_next ? 1 : 0;
}

// ---- stage 0: the checks, the call's noise draw, the workspace.  rng_counter is consumed between the pointer checks and the rest: a call
// that a later check refuses still uses up its draw.
static int step_setup(Step& p) {
  slode_handle h = p.h; const slode_shape& s = p.s; const StepCall& c = p.c;
  p.aux = c.kind == SLODE_SVI_AUX;
  const bool missing = c.phase == STEP_APPLY ? !c.payload || !c.grads
                                             : (!p.aux && (!c.times || !c.stage_t)) || !c.obs || (c.phase == STEP_WHOLE ? (!c.loss_out && !c.no_loss) : !c.payload);
  if (missing || !c.obs_strides || !c.workspace) return fail(h, SLODE_EINVAL, "a required pointer is NULL");
  p.K = particles_of(s);
  // eps == NULL: this call draws the guide's noise inside its kernels -- call number rng_counter of the handle's Philox stream; K particles
  // are the K drawing calls rng_counter .. rng_counter + K - 1 (particle k: call rng_counter + k, same trajectory index)
  if (!c.eps && c.phase != STEP_APPLY) { p.rng = rng_of(h, h->rng_counter); h->rng_counter += (uint64_t)p.K; }
  if (p.K > 1) {
    if (c.x_out || c.z_out) return fail(h, SLODE_EINVAL, "x_out / z_out take one particle: the shape has particles = %d", p.K);
    if (h->fold_on || h->ode_pack || h->ode_alg)
      return fail(h, SLODE_EINVAL, "particles = %d cannot be combined with the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG", p.K);
  }
  p.u = c.lab.n > 0 && !c.u ? c.lab.p[0] : c.u;   // (non-null = "labels present"; the kernels read through the accessor)
  if (p.aux && (s.n_aux < 1 || (!p.u && c.phase != STEP_APPLY)))
    return fail(h, SLODE_EINVAL, "the auxiliary loss needs label heads (n_aux >= 1) and labels u");
  // aux_kernel only: every head owns the latent-gradient slots of the dims it reads (one writer per slot).  The reference's heads read disjoint
  // groups (z_iext / z_rtpr, z_aR / z_aS / z_C12 / z_C6, ...).  Heads wider than 16 dims take the kernel's wide instantiation.
  for (int a = 0; p.aux && a < s.n_aux; ++a)
    for (int a2 = 0; a2 < a; ++a2)
      if (s.aux[a].z_off < s.aux[a2].z_off + s.aux[a2].z_dim && s.aux[a2].z_off < s.aux[a].z_off + s.aux[a].z_dim)
        return fail(h, SLODE_EINVAL, "slode_aux_step: label heads %d and %d read overlapping latent ranges", a2, a);
  if (s.n_groups > 0 && !p.u && c.phase != STEP_APPLY) return fail(h, SLODE_EINVAL, "u is NULL but the shape has conditional prior groups");
  p.dp5 = !p.aux && is_adaptive(s.method);
  const char* m = method_name(s.method);
  if (p.dp5 && !(s.H == 25 && (s.S == 5 || s.S == 8))) return fail(h, SLODE_EINVAL, "%s kernels are instantiated for (S,H) in {(5,25),(8,25)}", m);
  if (p.dp5 && ((long long)s.B * p.K > 65536 || h->ode_loop))
    return fail(h, SLODE_EINVAL, "the %s ELBO step takes at most 65,536 trajectories per call (B x particles = %lld)", m, (long long)s.B * p.K);
  if (p.dp5 && !slode_dp5_lanes_ok(s.method, dp5_lanes(h, s.B * p.K)))
    return fail(h, SLODE_EINVAL, "%s: SLODE_DP5_LPT=%d is not instantiated (8 or 16; 32 / 64 are dopri5 only)", m, dp5_lanes(h, s.B * p.K));
  p.w = carve(h, s, p.lay, c.workspace);
  if (c.workspace_bytes < p.w.bytes) return fail(h, SLODE_ENOSPC, "workspace %zu B < required %zu B", c.workspace_bytes, p.w.bytes);
  p.bwd = c.grads != nullptr || c.phase == STEP_PARTIAL;
  // Folded encoder (encoder_fused.hip) when every trajectory's C*T observations are one dense block; else layer by layer.
  const int64_t* os = c.obs_strides;
  p.t_major = os[1] == 1 && os[2] == s.C;            // [B,T,C] contiguous (cvs / challenge batches)
  const bool c_major = os[2] == 1 && os[1] == s.T;   // [B,C,T] contiguous (proc batches)
  p.folded = !h->no_fold && os[0] == (long long)s.C * s.T && (p.t_major || c_major) && (s.C == 3 || s.C == 4);
  return SLODE_OK;
}

// ---- stage 1: the encoder forward -- the fold launch (or its encoder half, when the workspace holds a current fold; or nothing, when the ODE
// kernel runs the encoder forward itself: *enc_fused), layer by layer, or nothing at all (STEP_APPLY).  Fills the fused tail's FoldLaunch.
static int step_encode(Step& p, FoldLaunch& fl, bool* enc_fused) {
  slode_handle h = p.h; const slode_shape& s = p.s; const slode_layout& lay = p.lay; const StepCall& c = p.c; const Workspace& w = p.w;
  if (c.phase != STEP_WHOLE && !p.folded)
    return fail(h, SLODE_EINVAL, "slode_grad_partial / slode_grad_apply need the folded encoder path (dense [B,T,C] or [B,C,T] observations, C in {3,4})");
  if (!p.folded) {
    EncLaunch ef{s, lay, c.params, c.obs, c.obs_strides[0], c.obs_strides[1], c.obs_strides[2], w.loc, w.scale, w.pooled, w.hid};
    hipError_t e = slode_launch_enc_fwd(ef, c.stream);
    if (e == hipErrorInvalidValue) return fail(h, SLODE_EINVAL, "unsupported encoder shape C=%d K=%d T=%d", s.C, s.K, s.T);
    HIP_TRY(h, e);
    return SLODE_OK;
  }
  fl.s = s; fl.lay = lay; fl.params = c.params; fl.x = c.obs; fl.t_major = p.t_major ? 1 : 0;
  fl.weff = w.weff; fl.rowsum = w.rowsum; fl.wprime = w.wprime; fl.beff = w.beff; fl.loc = w.loc; fl.scale = w.scale; fl.hid = w.hid;
  fl.g_loc = w.g_loc; fl.g_scale = w.g_scale; fl.g_pre = w.g_pre; fl.small_slabs = w.small_slabs; fl.small_stride = w.small_stride;
  fl.g_lin_w = c.grads ? c.grads + lay.lin_w : nullptr; fl.conv_slabs = w.conv_slabs; fl.counter = w.counter;
  // STEP_APPLY: no forward work (STEP_PARTIAL's fold launch left w' / rowsum / the zeroed arrival counters); the payload is ONE split
  if (c.phase == STEP_APPLY) { fl.gslabs = c.payload; fl.n_gslabs = 1; return SLODE_OK; }
  fl.gslabs = w.gslabs; fl.n_gslabs = w.gsplit; fl.sigtab = w.sigtab;   // (the aux step does not read the table; the next main step may)
  // the loop-free ODE kernel of the metric shape runs the encoder forward of its own trajectories (ode_kernel.hip, ENCF): fold only
  *enc_fused = !p.aux && h->enc_fuse && !c.x_out &&
               ode_takes_encf(s, p.bwd, w.ode_grid, p.dp5, h->ode_loop, h->ode_generic, h->ode_alg, h->ode_pack);   // (dp5: score_ode's launch has x_ext)
  fl.skip_enc = *enc_fused ? 1 : 0;
  return fold_fwd(h, c, fl, *enc_fused);
}

// ---- stage 2: the loss terms into the slab rows.  Aux: one workgroup per trajectory up to 2,048 of them, then a loop; on the folded path
// the kernel also runs the encoder-head backward and its slab rows carry only the label-head range (the fused tail reduces exactly that).
static int score_aux(Step& p, SlabRows* rows) {
  slode_handle h = p.h; const slode_shape& s = p.s; const slode_layout& lay = p.lay; const Workspace& w = p.w;
  AuxLaunch al{s, lay, p.c.params, w.loc, w.scale, p.c.eps, p.u, w.g_loc, w.g_scale, w.ode_slabs, w.ode_stride,
               w.ode_grid < 2048 ? w.ode_grid : 2048, p.bwd ? 1 : 0};
  al.rng = p.rng; al.lab = p.c.lab; al.particles = p.K;
  // compact rows carry the flat range [aux_w1[0], cstd): every label-head tensor must lie inside it (a caller-made layout may not)
  bool aux_contig = lay.aux_w1[0] <= lay.cstd;
  for (int a = 0; a < s.n_aux; ++a) {
    const int hi = s.aux[a].kind == SLODE_AUX_EXPEXP ? lay.aux_c[a] + 1 : lay.aux_b2[a] + s.aux[a].u_dim;
    aux_contig = aux_contig && lay.aux_w1[a] >= lay.aux_w1[0] && hi <= lay.cstd;
  }
  if (p.bwd && p.folded && !aux_contig) return fail(h, SLODE_EINVAL, "slode_aux_step: the label heads must lie in [aux_w1[0], cstd) of the layout (slode_layout_init's order)");
  if (p.bwd && p.folded) { al.compact = 1; al.enc_hid = w.hid; al.g_pre = w.g_pre; al.glat = w.glat; al.g_loc = nullptr; al.g_scale = nullptr; }
  rows->n = al.grid * p.K;
  HIP_TRY(h, slode_launch_aux(al, p.c.stream));
  return SLODE_OK;
}

static int score_ode(Step& p, bool enc_fused, SlabRows* rows) {
  slode_handle h = p.h; const slode_shape& s = p.s; const slode_layout& lay = p.lay; const StepCall& c = p.c; const Workspace& w = p.w;
  OdeLaunch a{};
  a.s = scorer_shape(s); a.lay = lay; a.params = c.params; a.times = c.times; a.stage_t = p.dp5 ? c.times : c.stage_t;
  a.obs = c.obs; a.sb = c.obs_strides[0]; a.sc = c.obs_strides[1]; a.st = c.obs_strides[2];
  a.u = p.u; a.eps = c.eps; a.loc = w.loc; a.scale = w.scale; a.x_out = c.x_out; a.z_out = c.z_out;
  a.g_loc = w.g_loc; a.g_scale = w.g_scale; a.slabs = w.ode_slabs; a.slab_stride = w.ode_stride; a.grid = w.ode_grid;
  a.backward = p.bwd ? 1 : 0; a.with_ll = 1; a.rng = p.rng; a.lab = c.lab; a.particles = p.K;
  a.sigtab = p.folded ? w.sigtab : nullptr;   // written by the fold launch
  a.force_loop = h->ode_loop; a.force_generic = h->ode_generic; a.alg = h->ode_alg; a.pack = h->ode_pack;
  if (p.bwd && p.folded && !p.dp5) { a.enc_hid = w.hid; a.g_pre = w.g_pre; a.glat = w.glat; a.g_loc = nullptr; a.g_scale = nullptr; }
  if (enc_fused) { a.enc_fuse = 1; a.enc_weff = w.weff; a.enc_beff = w.beff; a.enc_hid_out = w.hid; }
  const int n_scorer = w.ode_grid * p.K;   // the scorer's slab rows: one grid per particle
  slode_shape sv = s; sv.B = s.B * p.K; sv.particles = 0;   // what the adaptive solver's kernels see: every virtual trajectory
  if (p.dp5 && p.bwd && p.folded && solver_contig(s, lay) && n_scorer + w.dp_rows > 2 * SLODE_REDUCE_GROUPS) {
    // the scorer's rows carry nothing in the solver-side range [init net | dynamics] (the reverse sweep's rows do): the scorer does not
    // write those zeros and stage 1 of the fused tail (the only reader of the rows) does not read them
    a.ext_skip = 1;
    rows->zr_rows = n_scorer; rows->zr_lo = 1 + (lay.init_w1 - lay.ode_begin); rows->zr_hi = 1 + (lay.dyn_bd + s.S - lay.ode_begin);
  }
  // adaptive solve (accepted steps recorded) -> ONE scorer pass (loss terms, dLoss/dx, the gradients that do not flow through the solver)
  // -> reverse sweep over the records (solver-side gradients as extra slab rows, the latent gradient through the solver added to g_loc /
  // g_scale, the encoder-head backward).  Forward workgroups of 16 trajectories (8 or 16 lanes), as the sweep's, hand it their tables.
  DopriRec rc{w.loc, w.scale, c.eps, w.dp_z, p.bwd ? w.dp_rec : nullptr, w.dp_nrec, w.dp_kmax};
  rc.data_rows = s.B;
  if (p.dp5) {
    rc.w64 = dp5_lanes(h, sv.B);
    rc.tabs = p.bwd && (rc.w64 == 8 || rc.w64 == 16) ? w.dp_tabs : nullptr;
    // in-kernel noise: the forward kernel draws it once and materialises it, the scorer and the reverse sweep read the same values
    if (p.rng.on) { rc.rng = p.rng; rc.eps_out = w.dp_eps; a.rng = RngK{}; a.eps = w.dp_eps; }
    HIP_TRY(h, slode_launch_dopri5(sv, lay, c.params, c.times, nullptr, w.dp_x, c.stream, &rc));
    a.x_ext = w.dp_x;
    if (p.bwd) { a.gx_out = w.dp_gx; rows->n = n_scorer + w.dp_rows; }
  }
  hipError_t e = slode_launch_ode(a, c.stream, h->err, sizeof(h->err));
  if (e == hipErrorInvalidValue) return SLODE_EINVAL;
  HIP_TRY(h, e);
  rc.eps = a.eps;   // (the noise the forward kernel drew, when it drew it)
  if (p.dp5 && p.bwd)
    HIP_TRY(h, slode_launch_dopri5_bwd(sv, lay, c.params, c.times, rc, w.dp_gx, w.g_loc, w.g_scale, w.ode_slabs + (size_t)n_scorer * w.ode_stride,
                                       w.ode_stride, s.grad_mode == SLODE_GRAD_REFERENCE_ADJOINT ? 1 : 0, w.dp_snap, c.stream,
                                       p.folded ? w.hid : nullptr, p.folded ? w.g_pre : nullptr, p.folded ? w.glat : nullptr));
  return SLODE_OK;
}

// ---- between stages 2 and 3, K > 1 particles only: the particle fold.  The encoder-head backward and the tanh backward are linear in the
// latent gradient and their coefficients (head weights, scale, hid) do not depend on the particle, so the K rows of a data row are averaged
// BEFORE the encoder backward: g_pre / glat on the folded path, g_loc / g_scale on the layer-by-layer one.  Stage 3 then runs on B rows,
// once, whatever K is; only the slab reduction sees K times the rows.  A separate launch behind the scorers: no cross-workgroup wait.
static int particle_fold(Step& p) {
  const slode_shape& s = p.s; const Workspace& w = p.w;
  if (p.K < 2 || !p.bwd || p.c.phase == STEP_APPLY) return SLODE_OK;
  if (p.folded) HIP_TRY(p.h, slode_launch_particle_fold(w.g_pre, (long long)s.B * 64, w.glat, (long long)s.B * 128, p.K, p.c.stream));
  else HIP_TRY(p.h, slode_launch_particle_fold(w.g_loc, (long long)s.B * s.L, w.g_scale, (long long)s.B * s.L, p.K, p.c.stream));
  return SLODE_OK;
}

// ---- stage 3, folded backward: the fused tail.  Stage 2 ran the encoder heads + tanh backward (g_pre, glat): two launches remain -- split-K
// MFMA GEMMs (+ rider blocks: stage 1 of the ODE-slab reduction), chain rule + final reduction (+ Adam).  STEP_PARTIAL: the payload instead.
static int tail_fused(Step& p, FoldLaunch& fl, const SlabRows& rows) {
  slode_handle h = p.h; const slode_shape& s = p.s; const slode_layout& lay = p.lay; const StepCall& c = p.c; const Workspace& w = p.w;
  const int CT = s.C * s.T, count = (rows.part_hi - rows.part_lo) + 1;
  const PayloadMap pm = payload_map(s, rows.part_hi - rows.part_lo);
  const float* ode_part = nullptr; int ode_pn = 0;
  if (c.phase != STEP_APPLY)
    HIP_TRY(h, slode_launch_gemm_tail(w.g_pre, c.obs, w.gslabs, s.Hc, CT, w.glat, w.hid, w.gslabs2, w.gslabs3, s.L, s.B, w.gsplit,
                                      w.ode_slabs, w.ode_stride, rows.n, count, w.ode_part, &ode_part, &ode_pn, c.stream,
                                      rows.zr_rows, rows.zr_lo, rows.zr_hi));
  if (c.phase == STEP_PARTIAL) {   // split-K partials and partial slab rows, summed in fixed order, into the contiguous payload
    HIP_TRY(h, slode_launch_pack_payload(w.gslabs, w.gslabs2, w.gslabs3, w.gsplit, s.Hc, CT, s.L, ode_part, w.ode_stride, ode_pn,
                                         count, c.payload, pm.g_loc, pm.g_ls, pm.ode, pm.total, c.stream));
    return SLODE_OK;
  }
  TailK tl{};
  if (c.phase == STEP_APPLY) {   // the (reduced) payload stands for ONE split / ONE partial row
    tl.gslabs = c.payload; tl.gslabs_loc = c.payload + pm.g_loc; tl.gslabs_ls = c.payload + pm.g_ls;
    tl.ode_part = c.payload + pm.ode; tl.ode_stride = 0; tl.ode_n = 1; tl.gsplit = 1;
  } else {
    tl.gslabs = w.gslabs; tl.gslabs_loc = w.gslabs2; tl.gslabs_ls = w.gslabs3;
    tl.ode_part = ode_part; tl.ode_stride = w.ode_stride; tl.ode_n = ode_pn; tl.gsplit = w.gsplit;
  }
  tl.conv_slabs = w.conv_slabs; tl.loss_out = c.loss_out; tl.part_lo = rows.part_lo; tl.part_hi = rows.part_hi; tl.grads = c.grads;
  tl.Hc = s.Hc; tl.L = s.L; tl.CT = CT; tl.n_cv = s.F * s.C * s.K + s.F; tl.ode_begin = lay.ode_begin; tl.n_params = lay.n_params;
  tl.conv_w = lay.conv_w; tl.lin_w = lay.lin_w; tl.lin_b = lay.lin_b; tl.zloc_w = lay.zloc_w; tl.zloc_b = lay.zloc_b; tl.zls_w = lay.zls_w;
  tl.zls_b = lay.zls_b; tl.n_total = (c.adam.p && c.adam.n > lay.n_params) ? (int)c.adam.n : lay.n_params; tl.ad = make_adamk(&c.adam);
  tl.particles = p.K; tl.inv_k = 1.0f / (float)p.K;   // the slab rows sum over the particles: mean of the loss and of the ODE-half gradient
  tl.counter = tl.done = w.counter; tl.cstd_off = lay.cstd; tl.gauss = s.likelihood == SLODE_GAUSS ? 1 : 0; tl.sigtab = w.sigtab;
  fold_next_plan(h, s, lay, c, tl);
  fl.tail = &tl;
  HIP_TRY(h, slode_launch_fold_chain(fl, c.stream));   // + rider blocks and the last-block conv reduction: the flat gradient is complete
  return SLODE_OK;
}

// ---- stage 3, otherwise: the layer-by-layer encoder backward + the slab reduction (+ Adam), or the forward-only loss reduction
static int tail_reduce(Step& p, const SlabRows& rows) {
  slode_handle h = p.h; const StepCall& c = p.c; const Workspace& w = p.w;
  ReduceLaunch r{};
  r.s = p.s; r.lay = p.lay; r.ode_slabs = w.ode_slabs; r.ode_stride = w.ode_stride; r.ode_n = rows.n; r.ode_part = w.ode_part; r.loss_out = c.loss_out;
  r.particles = p.K;
  if (p.bwd) {
    if (c.adam.p) h->fold_valid = 0;
    EncBwdLaunch eb{p.s, p.lay, c.params, c.obs, c.obs_strides[0], c.obs_strides[1], c.obs_strides[2], w.scale, w.pooled, w.hid,
                    w.g_loc, w.g_scale, w.g_pre, w.small_slabs, w.small_stride, w.small_grid, w.lin_slabs, w.lin_splitk};
    HIP_TRY(h, slode_launch_enc_bwd(eb, c.stream));
    r.small_slabs = w.small_slabs; r.small_stride = w.small_stride; r.small_n = w.small_grid; r.small_part = w.small_part;
    r.lin_slabs = w.lin_slabs; r.lin_n = w.lin_splitk; r.grads = c.grads; r.zero_rest = 1; r.adam = c.adam;
  }
  HIP_TRY(h, slode_launch_reduce(r, c.stream));
  return SLODE_OK;
}

static int elbo_step_impl(slode_handle h, const slode_shape* s, const slode_layout* lay, const StepCall& call) {
  const char* why = check_common(h, s, lay, call.params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  Step p{h, *s, *lay, call};
  int rc = step_setup(p);
  if (rc != SLODE_OK) return rc;
  ClockScope clock_scope(h, true);
  FoldLaunch fl{}; bool enc_fused = false;
  SlabRows rows{p.w.ode_grid * p.K, lay->ode_begin, lay->n_params};
  if (p.aux && p.bwd && p.folded) { rows.part_lo = lay->aux_w1[0]; rows.part_hi = lay->cstd; }   // compact aux rows
  if ((rc = step_encode(p, fl, &enc_fused)) != SLODE_OK) return rc;
  if (call.phase != STEP_APPLY && (rc = p.aux ? score_aux(p, &rows) : score_ode(p, enc_fused, &rows)) != SLODE_OK) return rc;
  if ((rc = particle_fold(p)) != SLODE_OK) return rc;
  return p.bwd && p.folded ? tail_fused(p, fl, rows) : tail_reduce(p, rows);
}

extern "C" {

int slode_elbo_step(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                    const float* stage_t, const float* obs, const int64_t obs_strides[3], const float* u, const float* eps,
                    float* loss_out, float* grads, float* x_out, float* z_out, void* workspace, size_t workspace_bytes,
                    void* stream) {
  StepCall c;
  c.params = params; c.times = times; c.stage_t = stage_t; c.obs = obs; c.obs_strides = obs_strides; c.u = u; c.eps = eps; c.loss_out = loss_out;
  c.grads = grads; c.x_out = x_out; c.z_out = z_out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  return elbo_step_impl(h, s, lay, c);
}

int slode_elbo_adam_step(slode_handle h, const slode_shape* s, const slode_layout* lay, float* params, const float* times,
                         const float* stage_t, const float* obs, const int64_t obs_strides[3], const float* u, const float* eps,
                         float* loss_out, float* grads, void* workspace, size_t workspace_bytes, int64_t n_total, float* exp_avg,
                         float* exp_avg_sq, float lr, float beta1, float beta2, float adam_eps, int64_t step, void* stream) {
  StepCall c;
  c.params = params; c.times = times; c.stage_t = stage_t; c.obs = obs; c.obs_strides = obs_strides; c.u = u; c.eps = eps; c.loss_out = loss_out;
  c.grads = grads; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  const slode_adam a{n_total, exp_avg, exp_avg_sq, lr, beta1, beta2, adam_eps, step};
  const int rc = adam_args(h, "slode_elbo_adam_step", "Adam", lay, params, &a, &c);
  return rc != SLODE_OK ? rc : elbo_step_impl(h, s, lay, c);
}

int slode_aux_step(slode_handle h, const slode_shape* s, const slode_layout* lay, float* params, const float* obs,
                   const int64_t obs_strides[3], const float* u, const float* eps, float* loss_out, float* grads, void* workspace,
                   size_t workspace_bytes, int64_t n_total, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                   float adam_eps, int64_t step, void* stream) {
  StepCall c;
  c.kind = SLODE_SVI_AUX; c.params = params; c.obs = obs; c.obs_strides = obs_strides; c.u = u; c.eps = eps; c.loss_out = loss_out;
  c.grads = grads; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  const slode_adam a{n_total, exp_avg, exp_avg_sq, lr, beta1, beta2, adam_eps, step};
  const int rc = adam_args(h, "slode_aux_step with Adam", "both", lay, params, exp_avg ? &a : nullptr, &c);
  return rc != SLODE_OK ? rc : elbo_step_impl(h, s, lay, c);
}

int slode_svi_step(slode_handle h, const slode_shape* s, const slode_layout* lay, int kind, float* params, const float* times,
                   const float* stage_t, const slode_batch* batch, float* loss_out, float* grads, void* workspace, size_t workspace_bytes,
                   const slode_adam* adam, void* stream) {
  StepCall c;
  c.params = params; c.times = times; c.stage_t = stage_t; c.loss_out = loss_out; c.grads = grads;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  int rc = batch_call(h, s, kind, batch, &c);
  if (rc != SLODE_OK || (rc = adam_args(h, "slode_svi_step with Adam", "both", lay, params, adam, &c)) != SLODE_OK) return rc;
  return elbo_step_impl(h, s, lay, c);
}

// ---- what the eval-side calls share: eval_stats; the moment family (recon_moments, intervene_moments, forecast_moments, cohort_moments,
// calibration); the scored-draw family (traj_bounds, label_evidence, posterior_refine, pointwise_density) ----
// one workgroup per trajectory up to 65,536 of them, then (and under SLODE_ODE_LOOP) a resident grid that loops
static int eval_grid_for(const slode_ctx* h, int B) {
  long long g = B;
  if (B > 65536 || h->ode_loop) {
    g = (long long)h->num_cu * 4;
    if (h->ode_grid_cap > 0 && g > h->ode_grid_cap) g = h->ode_grid_cap;
    if (g > B) g = B;
  }
  return (int)g;
}
// dense [B,T,C] or [B,C,T] observation strides; *t_major: the former (and not also the latter)
static bool obs_dense(const slode_shape* s, const int64_t* os, bool* t_major) {
  const bool tm = os[1] == 1 && os[2] == s->C, cm = os[2] == 1 && os[1] == s->T;
  *t_major = tm && !cm;
  return os[0] == (long long)s->C * s->T && (tm || cm);
}
// The opening of a plan entry point (host arithmetic only; no handle): the shape, then the outputs as the caller's message lists them
static int plan_open(const char* who, const slode_shape* s, bool missing, const char* outputs) {
  const char* bad = check_shape(s);
  if (bad) return fail(nullptr, SLODE_EINVAL, "%s: %s", who, bad);
  if (missing) return fail(nullptr, SLODE_EINVAL, "%s: %s is NULL", who, outputs);
  return SLODE_OK;
}
// One of these calls as data: its name and the per-call pieces of the refusal texts they share.  A nullptr text: the
// call does not make that check.
struct EvalCall {
  const char* name;                      // "slode_traj_bounds"
  const char* pointers; bool missing;    // the pointers the call cannot do without, as its message lists them; whether one of them is NULL
  const char* draws_noun; int draws;     // "num_samples" / "num_draws" and its value (nullptr: eval_stats, whose four draws are fixed)
  const char* adaptive_tail;             // after "... (fixed-grid methods only)" of the adaptive solvers' refusal
  const char* one_particle;              // after "... particles = %d is not taken "
  const char* obs_null;                  // the refusal of batch->obs == NULL (nullptr: the prior; eval_stats, where step_setup finds it)
  const char* strides_tail;              // after "... observations with C in {3, 4}" (nullptr: the prior, which reads no observations)
  const char* lds_tables = nullptr;      // what the LDS figure counts, and the advice that ends that refusal (eval_lds)
  const char* lds_advice = nullptr;
  bool lds_per_draw = false;             // the LDS figure grows with the draw count: the refusal names it
  const char* lds_extra = nullptr;       // another size the LDS figure grows with, as the refusal names it (", n_arms = 6")
};
// The shared refusal ladder, in this order.  First: handle, shape, layout, params; the call's own pointers ...
static int eval_args(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const EvalCall& d) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (d.missing) return fail(h, SLODE_EINVAL, "%s: %s is NULL", d.name, d.pointers);
  return SLODE_OK;
}
// ... then the draw count; what the fused kernels do not take (adaptive solvers, particles, the measured arms); the observations
static int eval_refuse(slode_handle h, const slode_shape* s, const slode_batch* batch, const EvalCall& d) {
  if (d.draws_noun && d.draws < 1) return fail(h, SLODE_EINVAL, "%s: %s = %d < 1", d.name, d.draws_noun, d.draws);
  if (d.draws_noun && (long long)s->B * d.draws > 0x3fffffff)
    return fail(h, SLODE_EINVAL, "%s: B x %s = %lld exceeds 2^30 - 1 noise rows", d.name, d.draws_noun, (long long)s->B * d.draws);
  if (is_adaptive(s->method))
    return fail(h, SLODE_EINVAL, "%s: adaptive solver %s is not taken (fixed-grid methods only)%s", d.name, method_name(s->method), d.adaptive_tail);
  if (particles_of(*s) > 1) return fail(h, SLODE_EINVAL, "%s: particles = %d is not taken %s", d.name, s->particles, d.one_particle);
  if (h->fold_on || h->ode_pack || h->ode_alg)
    return fail(h, SLODE_EINVAL, "%s cannot be combined with the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG", d.name);
  if (d.obs_null && !batch->obs) return fail(h, SLODE_EINVAL, "%s: %s", d.name, d.obs_null);
  const int64_t* os = batch->obs_strides;
  bool t_major;
  if (d.strides_tail && (h->no_fold || !obs_dense(s, os, &t_major) || !(s->C == 3 || s->C == 4)))
    return fail(h, SLODE_EINVAL, "%s: observation strides (%lld, %lld, %lld) are not taken: the folded encoder path needs dense "
                                 "[B,T,C] or [B,C,T] observations with C in {3, 4}%s",
                d.name, (long long)os[0], (long long)os[1], (long long)os[2], d.strides_tail);
  return SLODE_OK;
}
// both, for the calls with no rung of their own between them (slode_traj_bounds: an alignment; slode_joint_band: its draw count)
static int eval_open(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const slode_batch* batch, const EvalCall& d) {
  const int rc = eval_args(h, s, lay, params, d);
  return rc != SLODE_OK ? rc : eval_refuse(h, s, batch, d);
}
// ... then the LDS budget of a kernel that walks the draws of its trajectories (slode_*_lds_bytes against SLODE_*_LDS_MAX); the label
// tensors (batch_labels) follow it, and step_setup's checks and workspace (forward_setup) come last
static int eval_lds(slode_handle h, const slode_shape* s, const EvalCall& d, size_t lds, int budget) {
  if (lds <= (size_t)budget) return SLODE_OK;
  char per_draw[48] = "";
  if (d.lds_per_draw) snprintf(per_draw, sizeof(per_draw), ", %s = %d", d.draws_noun, d.draws);
  else if (d.lds_extra) snprintf(per_draw, sizeof(per_draw), "%s", d.lds_extra);
  return fail(h, SLODE_EINVAL, "%s: the LDS tables of T = %d, S = %d, C = %d%s (%zu B: %s) exceed the budget of %d B; %s", d.name, s->T, s->S,
              s->C, per_draw, lds, d.lds_tables, budget, d.lds_advice);
}

// The shared tail.  The forward-only step on the batch (labels: batch_labels; loss_out == NULL: a set-up that writes no loss) ...
static StepCall forward_call(const float* params, const float* times, const float* stage_t, const slode_batch* batch, const LabelSrc& lab,
                             float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
  StepCall c;
  c.params = params; c.times = times; c.stage_t = stage_t; c.loss_out = loss_out; c.no_loss = loss_out ? 0 : 1;
  c.obs = batch->obs; c.obs_strides = batch->obs_strides; c.eps = batch->eps; c.lab = lab;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  return c;
}
// ... step_setup's checks and workspace without its draw (step_setup counts one draw; the call counts its own once nothing can refuse it
// any more), on the folded encoder path alone ...
static int forward_setup(Step& p, const char* who) {
  const uint64_t n0 = p.h->rng_counter;
  const int rc = step_setup(p);
  p.h->rng_counter = n0;
  if (rc != SLODE_OK) return rc;
  if (!p.folded) return fail(p.h, SLODE_EINVAL, "%s: the folded encoder path does not take these observations", who);
  return SLODE_OK;
}
// the drawing calls of a call that takes `draws` of them (the batch carries no eps), counted once nothing can refuse the call any more
static RngK take_draws(slode_handle h, const float* eps, int draws) {
  if (eps) return RngK{};
  const RngK r = rng_of(h, h->rng_counter);
  h->rng_counter += (uint64_t)draws;
  return r;
}
// ... and, inside the caller's ClockScope, the call's draws counted and the fold + encoder launches, which leave loc / scale (and the
// likelihood scale table) in the workspace for the call's own kernel
static int forward_encode(Step& p, int draws, RngK* rng) {
  *rng = take_draws(p.h, p.c.eps, draws);
  FoldLaunch fl{}; bool enc_fused = false;
  return step_encode(p, fl, &enc_fused);
}

// ---- the calls that walk num_samples draws per trajectory from one source (recon, forecast, cohort; intervene: the posterior alone) ----
// Their EvalCall: the refusal texts differ by the call's name, its advice ("reduce recon_samples instead") and what its LDS figure counts
// (nullptr: the call has an LDS rung of its own); the observation rungs exist for the posterior alone.
struct DrawsCall : EvalCall {
  char adaptive[80], strides[112];
  DrawsCall(const char* name_, const char* pointers_, bool missing_, int num_samples, int is_post, const char* advice, const char* tables) : EvalCall{} {
    snprintf(adaptive, sizeof(adaptive), "; %s", advice);
    snprintf(strides, sizeof(strides), " (and no SLODE_NO_FOLD); %s", advice);
    name = name_; pointers = pointers_; missing = missing_; draws_noun = "num_samples"; draws = num_samples;
    adaptive_tail = adaptive; one_particle = "(one particle only)";
    obs_null = is_post ? "the posterior needs observations (batch->obs is NULL)" : nullptr;
    strides_tail = is_post ? strides : nullptr;
    lds_tables = tables; lds_advice = tables ? advice : nullptr;
  }
  DrawsCall(const DrawsCall&) = delete;
};
// the label tensors of the batch; the prior reads them through the conditional prior nets
static int draws_labels(slode_handle h, const slode_shape* s, const slode_batch* batch, const EvalCall& d, int is_post, LabelSrc* lab) {
  const int rc = batch_labels(h, s, batch, lab);
  if (rc != SLODE_OK) return rc;
  if (!is_post && s->n_groups > 0 && lab->n == 0) return fail(h, SLODE_EINVAL, "%s: the prior needs the label tensors of the conditional prior groups", d.name);
  return SLODE_OK;
}
// everything of DrawsLaunch but lab (draws_labels) and loc / scale / rng (draws_run); items: what the persistent grid walks
static void draws_fill(DrawsLaunch& a, slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                       const float* stage_t, const slode_batch* batch, int is_post, int num_samples, int items) {
  a.s = *s; a.lay = *lay; a.params = params; a.times = times; a.stage_t = stage_t; a.eps = batch->eps;
  a.num_samples = num_samples; a.is_post = is_post ? 1 : 0; a.force_generic = h->ode_generic;
  a.grid = eval_grid_for(h, items);
}
// The tail: launch(stream) runs the call's own kernel(s) on a.  The prior: no observations, no encoder launches, nothing of the workspace but
// its size.  The posterior: the fold + encoder launches of a forward-only step on the training grid times / stage_t, which leave loc /
// scale in the workspace.  Either way the call's drawing calls (a.rng_calls: one; latent_attribution: two) are counted once nothing can refuse
// the call any more.
extern "C++" template <class Launch>
static int draws_run(slode_handle h, const slode_shape* s, const slode_layout* lay, const EvalCall& d, DrawsLaunch& a, const float* times,
                     const float* stage_t, const slode_batch* batch, void* workspace, size_t workspace_bytes, void* stream, Launch&& launch) {
  auto run = [&](hipStream_t st) {
    const hipError_t e = launch(st);
    return e == hipSuccess ? SLODE_OK : fail(h, SLODE_EHIP, "%s: launch: %s", d.name, hipGetErrorString(e));
  };
  if (!a.is_post) {
    if (workspace_bytes < slode_workspace_bytes(h, s)) return fail(h, SLODE_ENOSPC, "workspace %zu B < required %zu B", workspace_bytes, slode_workspace_bytes(h, s));
    a.rng = take_draws(h, batch->eps, a.rng_calls);
    ClockScope clock_scope(h, true);
    return run((hipStream_t)stream);
  }
  const StepCall c = forward_call(a.params, times, stage_t, batch, a.lab, nullptr, workspace, workspace_bytes, stream);
  Step p{h, *s, *lay, c};
  int rc = forward_setup(p, d.name);
  if (rc != SLODE_OK) return rc;
  a.loc = p.w.loc; a.scale = p.w.scale;
  ClockScope clock_scope(h, true);
  if ((rc = forward_encode(p, a.rng_calls, &a.rng)) != SLODE_OK) return rc;
  return run(c.stream);
}
// The three together, for any launch struct with a DrawsLaunch member d whose own fields (and d.rng_calls) the caller has set: labels, fill,
// run of launch(a, stream).  grid_times / grid_stage_t: the grid the kernel solves on where it is not the training grid (forecast).
extern "C++" template <class A>
static int draws_close(slode_handle h, const slode_shape* s, const slode_layout* lay, const EvalCall& d, A& a, const float* params, const float* times,
                       const float* stage_t, const slode_batch* batch, int is_post, int num_samples, int items, void* workspace, size_t workspace_bytes,
                       void* stream, hipError_t (*launch)(const A&, hipStream_t), const float* grid_times = nullptr, const float* grid_stage_t = nullptr) {
  const int rc = draws_labels(h, s, batch, d, is_post, &a.d.lab);
  if (rc != SLODE_OK) return rc;
  draws_fill(a.d, h, s, lay, params, grid_times ? grid_times : times, grid_times ? grid_stage_t : stage_t, batch, is_post, num_samples, items);
  return draws_run(h, s, lay, d, a.d, times, stage_t, batch, workspace, workspace_bytes, stream, [&](hipStream_t st) { return launch(a, st); });
}

// ---- the calls that score num_draws posterior draws of every trajectory against its observations (traj_bounds, label_evidence,
// posterior_refine, pointwise_density) ----
// Their EvalCall: the texts differ by the call's name, its pointer list and what its LDS figure counts (nullptr: an LDS rung of its own)
struct ScoredCall : EvalCall {
  ScoredCall(const char* name_, const char* pointers_, bool missing_, int num_draws, const char* tables = nullptr, const char* advice = nullptr,
             bool per_draw = false)
      : EvalCall{name_, pointers_, missing_, "num_draws", num_draws, "", "(the shape has one particle; the draws are num_draws)", "batch->obs is NULL",
                 " (and no SLODE_NO_FOLD)", tables, advice, per_draw} {}
};
// The tail, after the call's own rungs and outputs: the label tensors, step_setup's checks and workspace, everything of ScoredLaunch (loc /
// scale set on entry are kept: pointwise's caller-supplied posterior), the num_draws drawing calls counted once nothing can refuse the call
// any more, the fold + encoder launches of a forward-only step, then launch(stream): the call's own kernel on a (what: its failure's speaker).
extern "C++" template <class Launch>
static int scored_run(slode_handle h, const slode_shape* s, const slode_layout* lay, const EvalCall& d, ScoredLaunch& a, const float* params,
                      const float* times, const float* stage_t, const slode_batch* batch, void* workspace, size_t workspace_bytes, void* stream,
                      const char* what, Launch&& launch) {
  int rc = batch_labels(h, s, batch, &a.lab);
  if (rc != SLODE_OK) return rc;
  const StepCall c = forward_call(params, times, stage_t, batch, a.lab, nullptr, workspace, workspace_bytes, stream);
  Step p{h, *s, *lay, c};
  if ((rc = forward_setup(p, d.name)) != SLODE_OK) return rc;
  a.s = *s; a.lay = *lay; a.params = params; a.times = times; a.stage_t = stage_t; a.obs = c.obs; a.sb = batch->obs_strides[0];
  a.t_major = p.t_major ? 1 : 0;
  if (!a.loc) { a.loc = p.w.loc; a.scale = p.w.scale; }
  a.eps = c.eps; a.u = p.u; a.sigtab = p.w.sigtab; a.num_draws = d.draws; a.force_generic = h->ode_generic;
  a.grid = eval_grid_for(h, s->B);
  ClockScope clock_scope(h, true);
  if ((rc = forward_encode(p, d.draws, &a.rng)) != SLODE_OK) return rc;
  const hipError_t e = launch(c.stream);
  return e == hipSuccess ? SLODE_OK : fail(h, SLODE_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// The statistics row of one batch (include/slode.h): refusals first -- nothing launched, no draw consumed -- then the fold + encoder launches
// of a forward-only step, the fused kernel and the fixed-order reduction of its partial rows.
int slode_eval_stats(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                     const float* stage_t, const slode_batch* batch, int is_post, float* out, void* workspace, size_t workspace_bytes,
                     void* stream) {
  const EvalCall d{"slode_eval_stats", "batch / out", !batch || !out, nullptr, 0, "; run the unfused calls",
                   "(one particle only); run the unfused calls", nullptr, "; run the unfused calls"};
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (slode_eval_lds_bytes(*s) + 4096 > 160 * 1024)
    return fail(h, SLODE_EINVAL, "slode_eval_stats: T x S = %d x %d does not fit the step table into the LDS; run the unfused calls", s->T, s->S);
  EvalLaunch a{};
  if ((rc = batch_labels(h, s, batch, &a.lab)) != SLODE_OK) return rc;
  const StepCall c = forward_call(params, times, stage_t, batch, a.lab, out, workspace, workspace_bytes, stream);
  Step p{h, *s, *lay, c};
  if ((rc = forward_setup(p, d.name)) != SLODE_OK) return rc;
  const int64_t* os = batch->obs_strides;
  a.s = *s; a.lay = *lay; a.params = params; a.times = times; a.stage_t = stage_t; a.obs = c.obs; a.sb = os[0]; a.sc = os[1]; a.st = os[2];
  a.loc = p.w.loc; a.scale = p.w.scale; a.eps = c.eps; a.u = p.u; a.sigtab = p.w.sigtab; a.part = p.w.ode_slabs; a.out = out;
  a.is_post = is_post ? 1 : 0; a.force_generic = h->ode_generic;
  a.grid = eval_grid_for(h, s->B);
  if ((size_t)a.grid * SLODE_EVAL_SLOTS > (size_t)p.w.ode_grid * p.w.ode_stride)
    return fail(h, SLODE_ENOSPC, "slode_eval_stats: %d partial rows do not fit the workspace's slab rows", a.grid);
  ClockScope clock_scope(h, true);
  if ((rc = forward_encode(p, 4, &a.rng)) != SLODE_OK) return rc;
  HIP_TRY(h, slode_launch_eval(a, c.stream));
  return SLODE_OK;
}

// Mean / sd of the decoder head curves over num_samples latent draws (include/slode.h): refusals first -- nothing launched, no draw consumed --
// then, for the posterior, the fold + encoder launches of a forward-only step; then the one kernel that walks the draws of its trajectories.
int slode_recon_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                        const float* stage_t, const slode_batch* batch, int is_post, int num_samples, float* mean, float* sd, void* workspace,
                        size_t workspace_bytes, void* stream) {
  const DrawsCall d("slode_recon_moments", "batch / mean / times / stage_t / workspace", !batch || !mean || !times || !stage_t || !workspace,
                    num_samples, is_post, "reduce recon_samples instead", "step table, moments, staged weights");
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if ((rc = eval_lds(h, s, d, slode_recon_moments_lds_bytes(*s, h->ode_generic), SLODE_RECON_MOMENTS_LDS_MAX)) != SLODE_OK) return rc;
  ReconMomentsLaunch a{};
  a.mean = mean; a.sd = sd;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_recon_moments);
}

// Per-trajectory -ELBO, importance-weighted bound, effective sample size and mean negative log-likelihood from num_draws posterior draws
// (include/slode.h): refusals first -- nothing launched, no draw consumed -- then the fold + encoder launches of a forward-only step and the
// one kernel that walks the draws of its trajectories.  No composed fallback: no other call returns a per-trajectory loss.
int slode_traj_bounds(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                      const float* stage_t, const slode_batch* batch, int num_draws, float* bounds, float* loss_kb, void* workspace,
                      size_t workspace_bytes, void* stream) {
  const ScoredCall d("slode_traj_bounds", "batch / bounds / times / stage_t / workspace", !batch || !bounds || !times || !stage_t || !workspace,
                     num_draws, "step table, observations, staged weights, the per-draw losses", "fewer draws per call fit", true);
  int rc = eval_args(h, s, lay, params, d);
  if (rc != SLODE_OK) return rc;
  if (((uintptr_t)bounds & 15) != 0) return fail(h, SLODE_EINVAL, "slode_traj_bounds: bounds must be 16-byte aligned");
  if ((rc = eval_refuse(h, s, batch, d)) != SLODE_OK) return rc;
  if ((rc = eval_lds(h, s, d, slode_traj_bounds_lds_bytes(*s, num_draws, h->ode_generic), SLODE_TRAJ_BOUNDS_LDS_MAX)) != SLODE_OK) return rc;
  TrajBoundsLaunch a{};
  a.bounds = bounds; a.loss_kb = loss_kb;
  return scored_run(h, s, lay, d, a.d, params, times, stage_t, batch, workspace, workspace_bytes, stream, "slode_launch_traj_bounds(a, c.stream)",
                    [&](hipStream_t st) { return slode_launch_traj_bounds(a, st); });
}

// V label hypotheses scored on the num_draws posterior draws of every trajectory (include/slode.h): slode_traj_bounds' refusals through the
// same ladder, then the call's own -- nothing launched, no draw consumed -- then slode_traj_bounds' launches with the hypothesis kernel in
// place of its own.  No composed fallback: the composed route is V slode_traj_bounds calls, which refuse the same shapes.
int slode_label_evidence(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                         const float* stage_t, const slode_batch* batch, int num_draws, const float* const* hyp_labels, int V,
                         const float* log_prior, float* evidence, int32_t* best, float* loss_vkb, void* workspace, size_t workspace_bytes,
                         void* stream) {
  const ScoredCall d("slode_label_evidence", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_draws);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (!evidence || ((uintptr_t)evidence & 15) != 0) return fail(h, SLODE_EINVAL, "slode_label_evidence: evidence is NULL or not 16-byte aligned");
  if (V < 1 || V > SLODE_EVIDENCE_MAX_V) return fail(h, SLODE_EINVAL, "slode_label_evidence: V = %d out of range [1, %d]", V, SLODE_EVIDENCE_MAX_V);
  if (!hyp_labels) return fail(h, SLODE_EINVAL, "slode_label_evidence: hyp_labels is NULL");
  bool any = false;
  for (int i = 0; i < batch->n_labels && i < SLODE_MAX_LABELS; ++i) any = any || hyp_labels[i] != nullptr;
  if (batch->n_labels == 0) return fail(h, SLODE_EINVAL, "slode_label_evidence: the hypothesis tables take the widths of batch->labels (n_labels is 0)");
  if (!any) return fail(h, SLODE_EINVAL, "slode_label_evidence: every entry of hyp_labels is NULL (no label is hypothesised)");
  const size_t lds = slode_label_evidence_lds_bytes(*s, num_draws, V, h->ode_generic);
  if (lds > SLODE_LABEL_EVIDENCE_LDS_MAX)
    return fail(h, SLODE_EINVAL, "slode_label_evidence: the LDS tables of T = %d, S = %d, C = %d, num_draws = %d, V = %d (%zu B: step table, observations, "
                                 "staged weights, the V prior rows, the num_draws x V losses) exceed the budget of %d B; fewer draws or hypotheses per call fit",
                s->T, s->S, s->C, num_draws, V, lds, SLODE_LABEL_EVIDENCE_LDS_MAX);
  LabelEvidenceLaunch a{};
  a.log_prior = log_prior; a.evidence = evidence; a.best = best; a.loss_vkb = loss_vkb; a.V = V;
  return scored_run(h, s, lay, d, a.d, params, times, stage_t, batch, workspace, workspace_bytes, stream, "slode_launch_label_evidence(a, c.stream)",
                    [&](hipStream_t st) {
                      a.hyp = a.d.lab;   // widths and offsets as the batch's
                      for (int i = 0; i < SLODE_MAX_LABELS; ++i) a.hyp.p[i] = i < a.d.lab.n ? hyp_labels[i] : nullptr;
                      return slode_launch_label_evidence(a, st);
                    });
}

// num_steps Adam steps of every trajectory on its own (loc, log scale) against its num_draws-draw -ELBO (include/slode.h): slode_traj_bounds'
// refusals through the same ladder, then the call's own -- nothing launched, no draw consumed -- then slode_traj_bounds' launches with the
// refinement kernel in place of its own.  The noise rows are counted once: num_draws drawing calls, whatever num_steps.  No composed fallback.
int slode_posterior_refine(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                           const float* stage_t, const slode_batch* batch, int num_draws, int num_steps, float lr, const float* mask,
                           float* loc_out, float* scale_out, float* elbo_out, float* grad0_out, float* trace_out, int32_t* best_step,
                           void* workspace, size_t workspace_bytes, void* stream) {
  const ScoredCall d("slode_posterior_refine", "batch / loc_out / scale_out / elbo_out / times / stage_t / workspace",
                     !batch || !loc_out || !scale_out || !elbo_out || !times || !stage_t || !workspace, num_draws,
                     "step table and its kept copy, lambda, the stage-gradient table, observations, weights, staged weights, the per-draw losses",
                     "a shorter window or fewer draws per call fit", true);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (num_steps < 0) return fail(h, SLODE_EINVAL, "slode_posterior_refine: num_steps = %d < 0", num_steps);
  if (!(lr > 0.f && lr < INFINITY)) return fail(h, SLODE_EINVAL, "slode_posterior_refine: lr = %g is not a finite positive step size", (double)lr);
  if (s->aux_in_main && s->n_aux > 0)
    return fail(h, SLODE_EINVAL, "slode_posterior_refine: the main loss of this shape scores the labels (aux_in_main: the proc family); the backward "
                                 "pass of the label heads is out of scope");
  if ((rc = eval_lds(h, s, d, slode_refine_lds_bytes(*s, num_draws, h->ode_generic), SLODE_REFINE_LDS_MAX)) != SLODE_OK) return rc;
  RefineLaunch a{};
  a.d.mask = mask;
  a.loc_out = loc_out; a.scale_out = scale_out; a.elbo_out = elbo_out; a.grad0_out = grad0_out; a.trace_out = trace_out; a.best_step = best_step;
  a.lr = lr; a.num_steps = num_steps;
  return scored_run(h, s, lay, d, a.d, params, times, stage_t, batch, workspace, workspace_bytes, stream, "slode_launch_refine(a, c.stream)",
                    [&](hipStream_t st) { return slode_launch_refine(a, st); });
}

// The LDS bytes of slode_pointwise_density for a shape, a draw count and a weighting (host arithmetic only; the compiled state dims, no
// SLODE_ODE_GENERIC): SLODE_EINVAL when the call would refuse them at its LDS rung.
int slode_pointwise_plan(const slode_shape* s, int num_draws, int weights, size_t* lds_bytes) {
  if (int rc = plan_open("slode_pointwise_plan", s, !lds_bytes, "lds_bytes")) return rc;
  if (num_draws < 1) return fail(nullptr, SLODE_EINVAL, "slode_pointwise_plan: num_draws = %d < 1", num_draws);
  if (weights != SLODE_PW_POSTERIOR && weights != SLODE_PW_IMPORTANCE)
    return fail(nullptr, SLODE_EINVAL, "slode_pointwise_plan: weights = %d is neither SLODE_PW_POSTERIOR (0) nor SLODE_PW_IMPORTANCE (1)", weights);
  *lds_bytes = slode_pointwise_lds_bytes(*s, num_draws, weights, 0);
  if (*lds_bytes > SLODE_POINTWISE_LDS_MAX)
    return fail(nullptr, SLODE_EINVAL, "slode_pointwise_plan: the LDS tables of T = %d, S = %d, C = %d, num_draws = %d (%zu B) exceed the budget of %d B",
                s->T, s->S, s->C, num_draws, *lds_bytes, SLODE_POINTWISE_LDS_MAX);
  return SLODE_OK;
}

// Per-point lppd, mean and variance of the log-likelihood over num_draws posterior draws, and their per-trajectory sums (include/slode.h):
// slode_traj_bounds' refusals through the same ladder, then the call's own -- nothing launched, no draw consumed -- then slode_traj_bounds'
// launches with the pointwise kernel in place of its own.  loc / scale given: the fold + encoder launches still run (they leave the
// likelihood scale table); the kernel reads the caller's posterior instead of theirs.  No composed fallback.
int slode_pointwise_density(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                            const float* stage_t, const slode_batch* batch, int num_draws, int weights, const float* mask, const float* loc,
                            const float* scale, float* point, float* summary, float* loss_kb, void* workspace, size_t workspace_bytes,
                            void* stream) {
  const bool imp = weights == SLODE_PW_IMPORTANCE;
  const ScoredCall d("slode_pointwise_density", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_draws,
                     "step table, observations, mask, staged weights, the point accumulators, the per-draw losses and weights",
                     "a shorter window or (importance weights) fewer draws per call fit", imp);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (weights != SLODE_PW_POSTERIOR && weights != SLODE_PW_IMPORTANCE)
    return fail(h, SLODE_EINVAL, "slode_pointwise_density: weights = %d is neither SLODE_PW_POSTERIOR (0) nor SLODE_PW_IMPORTANCE (1)", weights);
  if (!point || !summary || ((uintptr_t)summary & 15) != 0)
    return fail(h, SLODE_EINVAL, "slode_pointwise_density: point / summary is NULL, or summary is not 16-byte aligned");
  if ((loc == nullptr) != (scale == nullptr))
    return fail(h, SLODE_EINVAL, "slode_pointwise_density: loc and scale replace the posterior together (%s is NULL)", loc ? "scale" : "loc");
  if (loss_kb && !imp)
    return fail(h, SLODE_EINVAL, "slode_pointwise_density: loss_kb is written in importance mode alone (SLODE_PW_POSTERIOR forms no per-draw loss)");
  if ((rc = eval_lds(h, s, d, slode_pointwise_lds_bytes(*s, num_draws, weights, h->ode_generic), SLODE_POINTWISE_LDS_MAX)) != SLODE_OK) return rc;
  PointwiseLaunch a{};
  a.d.mask = mask; a.d.loc = loc; a.d.scale = scale;   // (both or neither: scored_run keeps them)
  a.point = point; a.summary = summary; a.loss_kb = loss_kb; a.weights = weights;
  return scored_run(h, s, lay, d, a.d, params, times, stage_t, batch, workspace, workspace_bytes, stream, "slode_launch_pointwise(a, c.stream)",
                    [&](hipStream_t st) { return slode_launch_pointwise(a, st); });
}

// ---- PSIS leave-one-out: the draws of slode_pointwise_density in posterior mode, the smoothed leave-one-out estimate per point (include/slode.h) ----
// The tail-length, depth and tile rules as data: what the plan reports and the launch takes.  why: the refusal.
struct LooPlan { int tile, sweeps, depth; size_t lds; };
static int loo_plan(const slode_shape& s, int K, int tile, int force_generic, LooPlan* p, char* why, size_t why_n) {
  if (K < 1) { snprintf(why, why_n, "num_draws = %d < 1", K); return SLODE_EINVAL; }
  if (tile < 0 || tile > s.T) { snprintf(why, why_n, "tile = %d out of range [0, T = %d] (0: the library chooses)", tile, s.T); return SLODE_EINVAL; }
  // M = min(ceil(min(0.2 K, 3 sqrt K)), K - 1) in fp64; the kernel keeps the M + 1 smallest log-densities of every point
  const double mk = std::ceil(std::fmin(0.2 * (double)K, 3.0 * std::sqrt((double)K)));
  const int M = mk < (double)(K - 1) ? (int)mk : K - 1, D = M + 1;
  p->depth = D;
  const size_t budget = SLODE_LOO_LDS_MAX;
  auto bytes = [&](int tl) { return slode_pointwise_loo_lds_bytes(s, D, tl, force_generic); };
  int tl = tile;
  if (tile > 0) {
    if (bytes(tl) > budget) {
      snprintf(why, why_n, "tile = %d does not fit: the LDS tables of T = %d, S = %d, C = %d, num_draws = %d (%zu B: step table, observations, mask, staged "
               "weights, per point of the tile two (max, sum) pairs and the %d smallest log-densities) exceed the budget of %zu B; pass tile = 0 to let the "
               "library choose", tl, s.T, s.S, s.C, K, bytes(tl), D, budget);
      return SLODE_EINVAL;
    }
  } else {
    if (bytes(1) > budget) {
      snprintf(why, why_n, "num_draws = %d keeps the %d smallest log-densities of every point: the tables of one time point [%d][%d] do not fit beside the "
               "step table and the observations of T = %d, S = %d, C = %d (%zu B of a budget of %zu B); fewer draws or a shorter window fit", K, D, D + 4, s.C,
               s.T, s.S, s.C, bytes(1), budget);
      return SLODE_EINVAL;
    }
    for (int sw = 1;; ++sw) {   // the fewest sweeps that fit (sw = T: tile = 1 fits)
      tl = (s.T + sw - 1) / sw;
      if (bytes(tl) <= budget) break;
    }
  }
  p->tile = tl; p->sweeps = (s.T + tl - 1) / tl; p->lds = bytes(tl);
  return SLODE_OK;
}

// The plan of slode_pointwise_loo for a shape and a draw count (host arithmetic only; the compiled state dims, no SLODE_ODE_GENERIC):
// SLODE_EINVAL where the call would refuse them at its own rungs.
int slode_loo_plan(const slode_shape* s, int num_draws, int tile, int* tile_out, int* sweeps, int* depth, size_t* lds_bytes) {
  if (int rc = plan_open("slode_loo_plan", s, !tile_out || !sweeps || !depth || !lds_bytes, "tile_out / sweeps / depth / lds_bytes")) return rc;
  LooPlan p{};
  char why[512];
  if (loo_plan(*s, num_draws, tile, 0, &p, why, sizeof(why)) != SLODE_OK) return fail(nullptr, SLODE_EINVAL, "slode_loo_plan: %s", why);
  *tile_out = p.tile; *sweeps = p.sweeps; *depth = p.depth; *lds_bytes = p.lds;
  return SLODE_OK;
}

// Per-point PSIS leave-one-out elpd, Pareto khat and lppd over num_draws posterior draws, and their per-trajectory sums (include/slode.h):
// slode_pointwise_density's refusals in posterior mode through the same ladder, then the call's own (point / summary, loc / scale, the plan's
// refusal as the LDS rung) -- nothing launched, no draw consumed -- then its launches with the leave-one-out kernel in place of its own.  The
// noise rows are counted once: num_draws drawing calls, whatever the number of sweeps.
int slode_pointwise_loo(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times, const float* stage_t,
                        const slode_batch* batch, int num_draws, const float* mask, const float* loc, const float* scale, int tile, float* point,
                        float* summary, float* tail_out, void* workspace, size_t workspace_bytes, void* stream) {
  const ScoredCall d("slode_pointwise_loo", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_draws);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (!point || !summary || ((uintptr_t)summary & 15) != 0)
    return fail(h, SLODE_EINVAL, "slode_pointwise_loo: point / summary is NULL, or summary is not 16-byte aligned");
  if ((loc == nullptr) != (scale == nullptr))
    return fail(h, SLODE_EINVAL, "slode_pointwise_loo: loc and scale replace the posterior together (%s is NULL)", loc ? "scale" : "loc");
  LooPlan p{};
  char why[512];
  if (loo_plan(*s, num_draws, tile, h->ode_generic, &p, why, sizeof(why)) != SLODE_OK) return fail(h, SLODE_EINVAL, "slode_pointwise_loo: %s", why);
  PointwiseLooLaunch a{};
  a.d.mask = mask; a.d.loc = loc; a.d.scale = scale;   // (both or neither: scored_run keeps them)
  a.point = point; a.summary = summary; a.tail_out = tail_out; a.tile = p.tile; a.depth = p.depth;
  return scored_run(h, s, lay, d, a.d, params, times, stage_t, batch, workspace, workspace_bytes, stream, "slode_launch_pointwise_loo(a, c.stream)",
                    [&](hipStream_t st) { return slode_launch_pointwise_loo(a, st); });
}

// Paired-draw moments of the counterfactual curves and of their difference to the factual ones (include/slode.h): refusals first -- nothing
// launched, no draw consumed -- then the fold + encoder launches of a forward-only step, then the one kernel that walks the draws of its
// trajectories through both arms.
int slode_intervene_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                            const float* stage_t, const slode_batch* batch, const float* const* cf_labels, unsigned int group_mask, int num_samples,
                            float* cf_mean, float* cf_sd, float* eff_mean, float* eff_sd, void* workspace, size_t workspace_bytes, void* stream) {
  const DrawsCall d("slode_intervene_moments", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, 1,
                    "reduce counterfactual samples instead", "step table, moments, factual values, staged weights");
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (s->n_groups < 32 && (group_mask >> s->n_groups) != 0)
    return fail(h, SLODE_EINVAL, "slode_intervene_moments: group_mask = 0x%x has bits at or beyond n_groups = %d", group_mask, s->n_groups);
  if (group_mask != 0 && !cf_labels) return fail(h, SLODE_EINVAL, "slode_intervene_moments: group_mask = 0x%x needs the counterfactual labels (cf_labels is NULL)", group_mask);
  if ((rc = eval_lds(h, s, d, slode_intervene_moments_lds_bytes(*s, h->ode_generic), SLODE_INTERVENE_MOMENTS_LDS_MAX)) != SLODE_OK) return rc;
  InterveneMomentsLaunch a{};
  const LabelSrc& lab = a.d.lab;
  if ((rc = batch_labels(h, s, batch, &a.d.lab)) != SLODE_OK) return rc;
  a.cf = lab;   // widths as the batch's; a counterfactual tensor that no intervened group reads may be NULL (its slot keeps the batch's pointer, unread)
  if (group_mask != 0) {
    if (lab.n == 0) return fail(h, SLODE_EINVAL, "slode_intervene_moments: the counterfactual labels take the widths of batch->labels (n_labels is 0)");
    for (int i = 0; i < lab.n; ++i) {
      bool read = false;
      for (int g = 0; g < s->n_groups; ++g)
        read = read || (((group_mask >> g) & 1) && lab.off[i] < s->groups[g].u_off + s->groups[g].u_dim && lab.off[i + 1] > s->groups[g].u_off);
      if (cf_labels[i]) a.cf.p[i] = cf_labels[i];
      else if (read) return fail(h, SLODE_EINVAL, "slode_intervene_moments: counterfactual label tensor %d is NULL but an intervened group reads its columns", i);
    }
  }
  draws_fill(a.d, h, s, lay, params, times, stage_t, batch, 1, num_samples, s->B);
  a.cf_mean = cf_mean; a.cf_sd = cf_sd; a.eff_mean = eff_mean; a.eff_sd = eff_sd; a.group_mask = group_mask;
  return draws_run(h, s, lay, d, a.d, times, stage_t, batch, workspace, workspace_bytes, stream,
                   [&](hipStream_t st) { return slode_launch_intervene_moments(a, st); });
}

// ---- latent attribution: the draws of slode_recon_moments, every block of the latent redrawn in turn on a second noise row (include/slode.h) ----
// the blocks of a shape: its prior groups, and the rest block (bit n_groups) when some latent dim lies in no group
static bool attribution_has_rest(const slode_shape* s) {
  for (int l = 0; l < s->L; ++l) {
    bool in = false;
    for (int g = 0; g < s->n_groups; ++g) in = in || (l >= s->groups[g].z_off && l < s->groups[g].z_off + s->groups[g].z_dim);
    if (!in) return true;
  }
  return false;
}

// The LDS bytes of slode_latent_attribution for a shape and an arm count (host arithmetic only; the compiled state dims, no
// SLODE_ODE_GENERIC): SLODE_EINVAL when the call would refuse them at its LDS rung.
int slode_attribution_plan(const slode_shape* s, int n_arms, size_t* lds_bytes) {
  if (int rc = plan_open("slode_attribution_plan", s, !lds_bytes, "lds_bytes")) return rc;
  if (n_arms < 1 || n_arms > SLODE_ATTRIBUTION_MAX_ARMS)
    return fail(nullptr, SLODE_EINVAL, "slode_attribution_plan: n_arms = %d out of range [1, %d]", n_arms, SLODE_ATTRIBUTION_MAX_ARMS);
  *lds_bytes = slode_attribution_lds_bytes(*s, n_arms, 0);
  if (*lds_bytes > SLODE_ATTRIBUTION_LDS_MAX)
    return fail(nullptr, SLODE_EINVAL, "slode_attribution_plan: the LDS tables of T = %d, S = %d, C = %d, n_arms = %d (%zu B) exceed the budget of %d B",
                s->T, s->S, s->C, n_arms, *lds_bytes, SLODE_ATTRIBUTION_LDS_MAX);
  return SLODE_OK;
}

// Per-block variance shares of the head curves from pick-freeze draws (include/slode.h): refusals first -- slode_recon_moments' for the same
// is_post without its LDS rung, then the call's own; nothing launched, no draw consumed -- then slode_recon_moments' launches with the
// attribution kernel in place of its own, and two drawing calls (base, fresh) in place of one.
int slode_latent_attribution(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                             const float* stage_t, const slode_batch* batch, int is_post, int num_samples, const unsigned int* arm_masks,
                             int n_arms, float* mean, float* sd, float* msd, void* workspace, size_t workspace_bytes, void* stream) {
  DrawsCall d("slode_latent_attribution", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
              "reduce the attribution samples instead", nullptr);
  char arms[32];
  snprintf(arms, sizeof(arms), ", n_arms = %d", n_arms);
  d.lds_tables = "step table, base moments, base values, arm sums, staged weights"; d.lds_advice = "fewer arms per call fit (slode_attribution_plan)";
  d.lds_extra = arms;
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (n_arms < 1 || n_arms > SLODE_ATTRIBUTION_MAX_ARMS)
    return fail(h, SLODE_EINVAL, "slode_latent_attribution: n_arms = %d out of range [1, %d]", n_arms, SLODE_ATTRIBUTION_MAX_ARMS);
  if (!arm_masks || !msd) return fail(h, SLODE_EINVAL, "slode_latent_attribution: arm_masks / msd is NULL");
  const bool rest = attribution_has_rest(s);
  for (int a = 0; a < n_arms; ++a) {
    if ((arm_masks[a] >> (s->n_groups + 1)) != 0)
      return fail(h, SLODE_EINVAL, "slode_latent_attribution: arm_masks[%d] = 0x%x has bits beyond n_groups = %d (bit n_groups: the rest block)", a,
                  arm_masks[a], s->n_groups);
    if (!rest && ((arm_masks[a] >> s->n_groups) & 1u))
      return fail(h, SLODE_EINVAL, "slode_latent_attribution: arm_masks[%d] = 0x%x names the rest block, but the %d prior groups cover all L = %d latent dims",
                  a, arm_masks[a], s->n_groups, s->L);
  }
  if ((rc = eval_lds(h, s, d, slode_attribution_lds_bytes(*s, n_arms, h->ode_generic), SLODE_ATTRIBUTION_LDS_MAX)) != SLODE_OK) return rc;
  AttributionLaunch a{};
  a.d.rng_calls = 2;
  a.mean = mean; a.sd = sd; a.msd = msd; a.n_arms = n_arms;
  for (int i = 0; i < n_arms; ++i) a.masks[i] = arm_masks[i];
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_attribution);
}

// ---- curve summaries: the draws of slode_recon_moments, eight functionals of every draw's whole curve (include/slode.h) ----
// The LDS bytes of slode_curve_summary for a shape, with or without the p_beyond counters (host arithmetic only; the compiled state dims, no
// SLODE_ODE_GENERIC): SLODE_EINVAL when the call would refuse them at its LDS rung.
int slode_curve_summary_plan(const slode_shape* s, int want_p_beyond, size_t* lds_bytes) {
  if (int rc = plan_open("slode_curve_summary_plan", s, !lds_bytes, "lds_bytes")) return rc;
  *lds_bytes = slode_curve_summary_lds_bytes(*s, want_p_beyond, 0);
  if (*lds_bytes > SLODE_CURVE_SUMMARY_LDS_MAX)
    return fail(nullptr, SLODE_EINVAL, "slode_curve_summary_plan: the LDS tables of T = %d, S = %d, C = %d, %s p_beyond (%zu B) exceed the budget of %d B",
                s->T, s->S, s->C, want_p_beyond ? "with" : "without", *lds_bytes, SLODE_CURVE_SUMMARY_LDS_MAX);
  return SLODE_OK;
}

// Mean / sd over num_samples latent draws of the eight curve functionals (include/slode.h): refusals first -- slode_recon_moments' for the same
// is_post without its LDS rung, then the call's own, then its LDS rung; nothing launched, no draw consumed -- then slode_recon_moments'
// launches with the summary kernel in place of its own.
int slode_curve_summary(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                        const float* stage_t, const slode_batch* batch, int is_post, int num_samples, const float* thr, int sense, float* mean,
                        float* sd, float* p_beyond, void* workspace, size_t workspace_bytes, void* stream) {
  DrawsCall d("slode_curve_summary", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
              "reduce recon_samples instead", nullptr);
  d.lds_tables = "step table, grid and node weights, value table, counts, moment triples, staged weights";
  d.lds_advice = "drop p_beyond (slode_curve_summary_plan) or reduce recon_samples instead";
  d.lds_extra = ", with p_beyond";
  if (!p_beyond) {
    d.lds_tables = "step table, grid and node weights, value table, moment triples, staged weights";
    d.lds_advice = "reduce recon_samples instead"; d.lds_extra = ", without p_beyond";
  }
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (!mean) return fail(h, SLODE_EINVAL, "slode_curve_summary: mean is NULL");
  if (sense != 1 && sense != -1) return fail(h, SLODE_EINVAL, "slode_curve_summary: sense = %d is neither +1 (beyond: above thr) nor -1 (below)", sense);
  if (thr)
    for (int c = 0; c < s->C; ++c)
      if (!std::isfinite(thr[c])) return fail(h, SLODE_EINVAL, "slode_curve_summary: thr[%d] = %g is not finite", c, (double)thr[c]);
  if (p_beyond && !thr) return fail(h, SLODE_EINVAL, "slode_curve_summary: p_beyond needs a threshold (thr is NULL)");
  if ((rc = eval_lds(h, s, d, slode_curve_summary_lds_bytes(*s, p_beyond != nullptr, h->ode_generic), SLODE_CURVE_SUMMARY_LDS_MAX)) != SLODE_OK) return rc;
  CurveSummaryLaunch a{};
  a.mean = mean; a.sd = sd; a.p_beyond = p_beyond; a.has_thr = thr ? 1 : 0; a.sense = sense;
  for (int c = 0; c < SLODE_MAX_C; ++c) a.thr[c] = (thr && c < s->C) ? thr[c] : 0.f;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_curve_summary);
}

// ---- counterfactual summaries: the paired draws of slode_intervene_moments under V hypothesised inputs, the functionals of
// slode_curve_summary on every arm (include/slode.h) ----
// the largest V in [0, SLODE_INTERVENE_SUMMARY_MAX_ARMS] whose tables fit the budget (0: not even one arm does)
static int intervene_summary_fit(const slode_shape* s, int force_generic) {
  int v = SLODE_INTERVENE_SUMMARY_MAX_ARMS;
  while (v > 0 && slode_intervene_summary_lds_bytes(*s, v, force_generic) > SLODE_INTERVENE_SUMMARY_LDS_MAX) --v;
  return v;
}

// The LDS bytes of slode_intervene_summary for a shape and V arms (host arithmetic only; the compiled state dims, no SLODE_ODE_GENERIC):
// SLODE_EINVAL when the call would refuse them at its V or LDS rung.
int slode_intervene_summary_plan(const slode_shape* s, int V, size_t* lds_bytes) {
  if (int rc = plan_open("slode_intervene_summary_plan", s, !lds_bytes, "lds_bytes")) return rc;
  if (V < 1 || V > SLODE_INTERVENE_SUMMARY_MAX_ARMS)
    return fail(nullptr, SLODE_EINVAL, "slode_intervene_summary_plan: V = %d out of range [1, %d]", V, SLODE_INTERVENE_SUMMARY_MAX_ARMS);
  *lds_bytes = slode_intervene_summary_lds_bytes(*s, V, 0);
  if (*lds_bytes > SLODE_INTERVENE_SUMMARY_LDS_MAX)
    return fail(nullptr, SLODE_EINVAL, "slode_intervene_summary_plan: the LDS tables of T = %d, S = %d, C = %d, V = %d (%zu B) exceed the budget of %d B; "
                                       "at most V = %d fits", s->T, s->S, s->C, V, *lds_bytes, SLODE_INTERVENE_SUMMARY_LDS_MAX, intervene_summary_fit(s, 0));
  return SLODE_OK;
}

// Mean / sd over num_samples paired posterior draws of the eight curve functionals of the factual arm, of V counterfactual arms and of
// their paired differences (include/slode.h): refusals first -- slode_recon_moments' for the posterior without its LDS rung, then the call's
// own, then its LDS rung; nothing launched, no draw consumed -- then slode_recon_moments' launches with the summary kernel in place of its own.
int slode_intervene_summary(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                            const float* stage_t, const slode_batch* batch, const float* const* hyp_labels, int V, unsigned int group_mask,
                            int num_samples, const float* thr, int sense, float* f_mean, float* f_sd, float* cf_mean, float* cf_sd, float* eff_mean,
                            float* eff_sd, void* workspace, size_t workspace_bytes, void* stream) {
  static const char* N = "slode_intervene_summary";
  DrawsCall d(N, "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, 1,
              "reduce counterfactual samples instead", nullptr);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (!cf_mean) return fail(h, SLODE_EINVAL, "%s: cf_mean is NULL", N);
  if (V < 1 || V > SLODE_INTERVENE_SUMMARY_MAX_ARMS) return fail(h, SLODE_EINVAL, "%s: V = %d out of range [1, %d]", N, V, SLODE_INTERVENE_SUMMARY_MAX_ARMS);
  if (sense != 1 && sense != -1) return fail(h, SLODE_EINVAL, "%s: sense = %d is neither +1 (beyond: above thr) nor -1 (below)", N, sense);
  if (thr)
    for (int c = 0; c < s->C; ++c)
      if (!std::isfinite(thr[c])) return fail(h, SLODE_EINVAL, "%s: thr[%d] = %g is not finite", N, c, (double)thr[c]);
  if (s->n_groups < 32 && (group_mask >> s->n_groups) != 0)
    return fail(h, SLODE_EINVAL, "%s: group_mask = 0x%x has bits at or beyond n_groups = %d", N, group_mask, s->n_groups);
  InterveneSummaryLaunch a{};
  if (group_mask != 0) {
    const int n = batch->n_labels < 0 ? 0 : (batch->n_labels > SLODE_MAX_LABELS ? SLODE_MAX_LABELS : batch->n_labels);
    bool any = false, read = false;
    int lo = 0;
    for (int i = 0; hyp_labels && i < n; ++i) {
      const int hi = lo + batch->label_width[i];
      if (hyp_labels[i]) {
        any = true;
        for (int g = 0; g < s->n_groups; ++g)
          read = read || (((group_mask >> g) & 1) && lo < s->groups[g].u_off + s->groups[g].u_dim && hi > s->groups[g].u_off);
      }
      lo = hi;
    }
    if (!any)
      return fail(h, SLODE_EINVAL, "%s: group_mask = 0x%x needs the hypothesis tables (%s)", N, group_mask,
                  !hyp_labels ? "hyp_labels is NULL" : (n == 0 ? "they take the widths of batch->labels: n_labels is 0" : "every entry of hyp_labels is NULL"));
    if (!read) return fail(h, SLODE_EINVAL, "%s: no group of group_mask = 0x%x reads a column of a hypothesised label tensor", N, group_mask);
  }
  char arms[24], advice[96];
  snprintf(arms, sizeof(arms), ", V = %d", V);
  snprintf(advice, sizeof(advice), "at most V = %d fits: fewer hypotheses per call (slode_intervene_summary_plan)", intervene_summary_fit(s, h->ode_generic));
  d.lds_tables = "step table, loc | scale of the V arms, grid and node weights, value table, factual functionals, moment triples and counts of 1 + 2 V sets, staged weights";
  d.lds_advice = advice; d.lds_extra = arms;
  if ((rc = eval_lds(h, s, d, slode_intervene_summary_lds_bytes(*s, V, h->ode_generic), SLODE_INTERVENE_SUMMARY_LDS_MAX)) != SLODE_OK) return rc;
  a.f_mean = f_mean; a.f_sd = f_sd; a.cf_mean = cf_mean; a.cf_sd = cf_sd; a.eff_mean = eff_mean; a.eff_sd = eff_sd;
  a.V = V; a.group_mask = group_mask; a.has_thr = thr ? 1 : 0; a.sense = sense;
  for (int c = 0; c < SLODE_MAX_C; ++c) a.thr[c] = (thr && c < s->C) ? thr[c] : 0.f;
  for (int i = 0; i < SLODE_MAX_LABELS; ++i) a.hyp[i] = (group_mask != 0 && hyp_labels && i < batch->n_labels) ? hyp_labels[i] : nullptr;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, 1, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_intervene_summary);
}

// ---- sample quantiles: the draws of slode_recon_moments, order statistics of every value over the draws (include/slode.h) ----
// The rank, depth and tile rules as data: what the plan reports and the launch takes.  why: the refusal.
struct QuantilePlan { int tile, sweeps, depth_lo, depth_hi; size_t lds; int slot_lo[SLODE_QUANTILE_MAX_LEVELS], slot_hi[SLODE_QUANTILE_MAX_LEVELS]; float g[SLODE_QUANTILE_MAX_LEVELS]; };
static int quantile_plan(const slode_shape& s, int K, int n_levels, const double* levels, int tile, int force_generic, QuantilePlan* p, char* why,
                         size_t why_n) {
  if (K < 1) { snprintf(why, why_n, "num_samples = %d < 1", K); return SLODE_EINVAL; }
  if (n_levels < 1 || n_levels > SLODE_QUANTILE_MAX_LEVELS) {
    snprintf(why, why_n, "n_levels = %d out of range [1, %d]", n_levels, SLODE_QUANTILE_MAX_LEVELS);
    return SLODE_EINVAL;
  }
  if (!levels) { snprintf(why, why_n, "levels is NULL"); return SLODE_EINVAL; }
  for (int i = 0; i < n_levels; ++i)
    if (!(levels[i] >= 0.0 && levels[i] <= 1.0)) { snprintf(why, why_n, "levels[%d] = %g is not in [0, 1]", i, levels[i]); return SLODE_EINVAL; }
  if (tile < 0 || tile > s.T) { snprintf(why, why_n, "tile = %d out of range [0, T = %d] (0: the library chooses)", tile, s.T); return SLODE_EINVAL; }
  // ranks: numpy's "linear" definition, fp64; each rank from the side that costs less, the bottom on a tie
  int r_lo[SLODE_QUANTILE_MAX_LEVELS], r_hi[SLODE_QUANTILE_MAX_LEVELS];
  int m_lo = 0, m_hi = 0;
  for (int i = 0; i < n_levels; ++i) {
    const double hq = levels[i] * (double)(K - 1);
    int lo = (int)std::floor(hq);
    lo = lo < 0 ? 0 : (lo > K - 1 ? K - 1 : lo);
    r_lo[i] = lo; r_hi[i] = lo + 1 < K ? lo + 1 : K - 1;
    p->g[i] = (float)(hq - (double)lo);
    if (p->g[i] == 0.f) r_hi[i] = lo;   // the upper rank has no weight: not needed (fma(0, 0, v_lo) = v_lo)
    for (int r : {r_lo[i], r_hi[i]}) {
      if (r + 1 <= K - r) m_lo = r + 1 > m_lo ? r + 1 : m_lo;
      else m_hi = K - r > m_hi ? K - r : m_hi;
    }
  }
  if (m_lo + m_hi >= K) { m_lo = K; m_hi = 0; }   // the buffers would meet: keep every draw, sorted
  for (int i = 0; i < n_levels; ++i) {
    p->slot_lo[i] = r_lo[i] < m_lo ? r_lo[i] : m_lo + (K - 1 - r_lo[i]);
    p->slot_hi[i] = r_hi[i] < m_lo ? r_hi[i] : m_lo + (K - 1 - r_hi[i]);
  }
  for (int i = n_levels; i < SLODE_QUANTILE_MAX_LEVELS; ++i) { p->slot_lo[i] = p->slot_hi[i] = 0; p->g[i] = 0.f; }
  p->depth_lo = m_lo; p->depth_hi = m_hi;
  const int D = m_lo + m_hi, Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  const size_t budget = SLODE_RECON_QUANTILES_LDS_MAX;
  auto bytes = [&](int tl) { return slode_recon_quantiles_lds_bytes(s, D, tl, force_generic); };
  int tl = tile;
  if (tile > 0) {
    if (bytes(tl) > budget) {
      snprintf(why, why_n, "tile = %d does not fit: the LDS tables of T = %d, S = %d, C = %d, depth = %d + %d (%zu B: step table, staged weights, level table, "
               "sorted buffers [depth][%d][tile]) exceed the budget of %zu B; pass tile = 0 to let the library choose", tl, s.T, s.S, s.C, m_lo, m_hi,
               bytes(tl), Q * s.C, budget);
      return SLODE_EINVAL;
    }
  } else {
    if (bytes(1) > budget) {
      snprintf(why, why_n, "depth = %d + %d of num_samples = %d: the sorted buffers of one time point [depth][%d] do not fit beside the step table of T = %d, "
               "S = %d (%zu B of a budget of %zu B); sort recon_samples instead", m_lo, m_hi, K, Q * s.C, s.T, s.S, bytes(1), budget);
      return SLODE_EINVAL;
    }
    for (int sw = 1;; ++sw) {   // the fewest sweeps that fit (sw = T: tile = 1 fits)
      tl = (s.T + sw - 1) / sw;
      if (bytes(tl) <= budget) break;
    }
  }
  p->tile = tl; p->sweeps = (s.T + tl - 1) / tl; p->lds = bytes(tl);
  return SLODE_OK;
}

// The plan of slode_recon_quantiles for a shape, a draw count and a level set (host arithmetic only; the compiled state dims, no SLODE_ODE_GENERIC):
// SLODE_EINVAL where the call would refuse them at its own rungs.
int slode_quantile_plan(const slode_shape* s, int num_samples, int n_levels, const double* levels, int tile, int* tile_out, int* sweeps,
                        int* depth_lo, int* depth_hi, size_t* lds_bytes) {
  if (int rc = plan_open("slode_quantile_plan", s, !tile_out || !sweeps || !depth_lo || !depth_hi || !lds_bytes, "tile_out / sweeps / depth_lo / depth_hi / lds_bytes")) return rc;
  QuantilePlan p{};
  char why[448];
  if (quantile_plan(*s, num_samples, n_levels, levels, tile, 0, &p, why, sizeof(why)) != SLODE_OK) return fail(nullptr, SLODE_EINVAL, "slode_quantile_plan: %s", why);
  *tile_out = p.tile; *sweeps = p.sweeps; *depth_lo = p.depth_lo; *depth_hi = p.depth_hi; *lds_bytes = p.lds;
  return SLODE_OK;
}

// Sample quantiles of the head curves over num_samples latent draws (include/slode.h): refusals first -- slode_recon_moments' for the same
// is_post without its LDS rung, then the call's own (out, the levels, the tile, the plan's refusal as the LDS rung); nothing launched, no draw
// consumed -- then slode_recon_moments' launches with the quantile kernel in place of its own.
int slode_recon_quantiles(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                          const float* stage_t, const slode_batch* batch, int is_post, int num_samples, int n_levels, const double* levels, int tile,
                          float* out, void* workspace, size_t workspace_bytes, void* stream) {
  const DrawsCall d("slode_recon_quantiles", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
                    "sort recon_samples instead", nullptr);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (!out) return fail(h, SLODE_EINVAL, "slode_recon_quantiles: out is NULL");
  ReconQuantilesLaunch a{};
  QuantilePlan p{};
  char why[448];
  if (quantile_plan(*s, num_samples, n_levels, levels, tile, h->ode_generic, &p, why, sizeof(why)) != SLODE_OK)
    return fail(h, SLODE_EINVAL, "slode_recon_quantiles: %s", why);
  a.d.rng_calls = num_samples;   // the counter moves by num_samples whatever the number of sweeps; the noise: rows k * B + b of drawing call n
  a.out = out; a.n_levels = n_levels; a.tile = p.tile; a.depth_lo = p.depth_lo; a.depth_hi = p.depth_hi;
  for (int i = 0; i < SLODE_QUANTILE_MAX_LEVELS; ++i) { a.slot_lo[i] = p.slot_lo[i]; a.slot_hi[i] = p.slot_hi[i]; a.g[i] = p.g[i]; }
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_recon_quantiles);
}

// ---- mechanism curves: the draws of slode_recon_moments, the moments of x, a, d, a / d and a - d x at every grid point (include/slode.h) ----
// The LDS bytes of slode_mechanism_moments for a shape and a slot mask (host arithmetic only; the compiled state dims, no SLODE_ODE_GENERIC):
// SLODE_EINVAL when the call would refuse them at its mask or LDS rung.
int slode_mechanism_plan(const slode_shape* s, unsigned int slots, size_t* lds_bytes) {
  if (int rc = plan_open("slode_mechanism_plan", s, !lds_bytes, "lds_bytes")) return rc;
  const int n_sel = __builtin_popcount(slots & ((1u << SLODE_MECHANISM_SLOTS) - 1));
  *lds_bytes = slode_mechanism_lds_bytes(*s, n_sel, 0);
  if (slots == 0 || (slots >> SLODE_MECHANISM_SLOTS))
    return fail(nullptr, SLODE_EINVAL, "slode_mechanism_plan: slots = 0x%x selects nothing or has bits at or beyond SLODE_MECHANISM_SLOTS = %d", slots,
                SLODE_MECHANISM_SLOTS);
  if (*lds_bytes > SLODE_MECHANISM_LDS_MAX)
    return fail(nullptr, SLODE_EINVAL, "slode_mechanism_plan: the LDS tables of T = %d, S = %d, slots = %d (%zu B) exceed the budget of %d B", s->T, s->S,
                n_sel, *lds_bytes, SLODE_MECHANISM_LDS_MAX);
  return SLODE_OK;
}

// Mean / sd over num_samples latent draws of the selected mechanism slots (include/slode.h): refusals first -- slode_recon_moments' for the same
// is_post without its LDS rung, then the call's own (mean, the mask), then its LDS rung; nothing launched, no draw consumed -- then
// slode_recon_moments' launches with the mechanism kernel in place of its own.
int slode_mechanism_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                            const float* stage_t, const slode_batch* batch, int is_post, int num_samples, unsigned int slots, float* mean, float* sd,
                            void* workspace, size_t workspace_bytes, void* stream) {
  DrawsCall d("slode_mechanism_moments", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
              "compose slode_ode_solve_fwd and the dynamics net instead", nullptr);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (!mean) return fail(h, SLODE_EINVAL, "slode_mechanism_moments: mean is NULL");
  if (slots == 0 || (slots >> SLODE_MECHANISM_SLOTS))
    return fail(h, SLODE_EINVAL, "slode_mechanism_moments: slots = 0x%x selects nothing or has bits at or beyond SLODE_MECHANISM_SLOTS = %d", slots,
                SLODE_MECHANISM_SLOTS);
  const int n_sel = __builtin_popcount(slots);
  char extra[24];
  snprintf(extra, sizeof(extra), ", slots = %d", n_sel);
  d.lds_tables = "step table, moment triples, capture table, staged weights";
  d.lds_advice = "fewer slots per call fit (slode_mechanism_plan)"; d.lds_extra = extra;
  if ((rc = eval_lds(h, s, d, slode_mechanism_lds_bytes(*s, n_sel, h->ode_generic), SLODE_MECHANISM_LDS_MAX)) != SLODE_OK) return rc;
  MechanismLaunch a{};
  a.mean = mean; a.sd = sd; a.slots = slots;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_mechanism_moments);
}

// ---- simultaneous bands: the draws of slode_recon_moments twice, the quantiles of the draws' largest standardised deviation (include/slode.h) ----
// z = Phi^-1((1 + p) / 2) = sqrt(2) erfinv(p) for p in (0, 1) in fp64: Winitzki's closed form as the start, then Halley steps on
// erfc(x) = 1 - p with the C library's erfc (cubic convergence: the third step is already at rounding level)
static double joint_band_z(double p) {
  if (p >= 1.0) return INFINITY;
  const double pi = 3.14159265358979323846, a = 0.147, q = 1.0 - p;
  const double ln1 = std::log1p(-p * p), t = 2.0 / (pi * a) + 0.5 * ln1;
  double x = std::sqrt(std::sqrt(t * t - ln1 / a) - t);
  for (int it = 0; it < 4; ++it) {
    const double u = (std::erfc(x) - q) / (-2.0 / std::sqrt(pi) * std::exp(-x * x));   // f / f'
    x -= u / (1.0 + x * u);                                                            // f'' / f' = -2 x
  }
  return std::sqrt(2.0) * x;
}
// The level rules as data: what slode_joint_band_levels reports and the launch takes.  why: the refusal.
static int joint_band_levels(int K, int n_levels, const double* levels, int* ranks, double* z, char* why, size_t why_n) {
  if (K < 2) { snprintf(why, why_n, "num_samples = %d < 2 (the sd of one draw is 0)", K); return SLODE_EINVAL; }
  if (n_levels < 1 || n_levels > SLODE_JOINT_BAND_MAX_LEVELS) {
    snprintf(why, why_n, "n_levels = %d out of range [1, %d]", n_levels, SLODE_JOINT_BAND_MAX_LEVELS);
    return SLODE_EINVAL;
  }
  if (!levels) { snprintf(why, why_n, "levels is NULL"); return SLODE_EINVAL; }
  for (int i = 0; i < n_levels; ++i) {
    if (!(levels[i] > 0.0 && levels[i] <= 1.0)) { snprintf(why, why_n, "levels[%d] = %g is not in (0, 1]", i, levels[i]); return SLODE_EINVAL; }
    const double r = std::ceil(levels[i] * (double)K - 1e-9);
    ranks[i] = r < 1.0 ? 1 : (r > (double)K ? K : (int)r);
    z[i] = joint_band_z(levels[i]);
  }
  return SLODE_OK;
}

int slode_joint_band_levels(int num_samples, int n_levels, const double* levels, int* ranks, double* z) {
  if (!ranks || !z) return fail(nullptr, SLODE_EINVAL, "slode_joint_band_levels: ranks / z is NULL");
  char why[160];
  int r[SLODE_JOINT_BAND_MAX_LEVELS];
  double zz[SLODE_JOINT_BAND_MAX_LEVELS];
  if (joint_band_levels(num_samples, n_levels, levels, r, zz, why, sizeof(why)) != SLODE_OK) return fail(nullptr, SLODE_EINVAL, "slode_joint_band_levels: %s", why);
  for (int i = 0; i < n_levels; ++i) { ranks[i] = r[i]; z[i] = zz[i]; }
  return SLODE_OK;
}

// The LDS bytes of slode_joint_band for a shape and a draw count (host arithmetic only; the compiled state dims, no SLODE_ODE_GENERIC):
// SLODE_EINVAL where the call would refuse them at its draw-count or LDS rung.
int slode_joint_band_plan(const slode_shape* s, int num_samples, size_t* lds_bytes) {
  if (int rc = plan_open("slode_joint_band_plan", s, !lds_bytes, "lds_bytes")) return rc;
  if (num_samples < 2) return fail(nullptr, SLODE_EINVAL, "slode_joint_band_plan: num_samples = %d < 2 (the sd of one draw is 0)", num_samples);
  *lds_bytes = slode_joint_band_lds_bytes(*s, num_samples, 0);
  if (*lds_bytes > SLODE_JOINT_BAND_LDS_MAX)
    return fail(nullptr, SLODE_EINVAL, "slode_joint_band_plan: the LDS tables of T = %d, S = %d, C = %d, num_samples = %d (%zu B: step table, staged "
                                       "weights, moment / value table, deviations [%d][num_samples]) exceed the budget of %d B", s->T, s->S, s->C,
                num_samples, *lds_bytes, (s->likelihood == SLODE_GAUSS ? 1 : 3) * s->C, SLODE_JOINT_BAND_LDS_MAX);
  return SLODE_OK;
}

// Simultaneous bands over num_samples latent draws (include/slode.h): refusals first -- the draw count, slode_recon_moments' for the same is_post
// without its LDS rung, then the call's own (outputs, levels, floor, the prior's optional observations), then its LDS rung; nothing launched,
// no draw consumed -- then slode_recon_moments' launches with the band kernel in place of its own.
int slode_joint_band(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                     const float* stage_t, const slode_batch* batch, int is_post, int num_samples, int n_levels, const double* levels,
                     float sd_floor, float* mean, float* sd, float* crit, float* joint, float* obs_dev, float* dev_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
  DrawsCall d("slode_joint_band", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
              "reduce recon_samples instead", nullptr);
  int rc = eval_args(h, s, lay, params, d);
  if (rc != SLODE_OK) return rc;
  if (num_samples < 2) return fail(h, SLODE_EINVAL, "slode_joint_band: num_samples = %d < 2 (the sd of one draw is 0)", num_samples);
  if ((rc = eval_refuse(h, s, batch, d)) != SLODE_OK) return rc;
  if (!mean || !sd || !crit) return fail(h, SLODE_EINVAL, "slode_joint_band: mean / sd / crit is NULL");
  JointBandLaunch a{};
  char why[160];
  double z[SLODE_JOINT_BAND_MAX_LEVELS];
  if (joint_band_levels(num_samples, n_levels, levels, a.rank, z, why, sizeof(why)) != SLODE_OK) return fail(h, SLODE_EINVAL, "slode_joint_band: %s", why);
  for (int i = 0; i < n_levels; ++i) a.z[i] = (float)z[i];
  if (!(sd_floor >= 0.f) || std::isinf(sd_floor)) return fail(h, SLODE_EINVAL, "slode_joint_band: sd_floor = %g is negative or not finite", (double)sd_floor);
  const int64_t* os = batch->obs_strides;
  bool t_major;
  if (!obs_dense(s, os, &t_major) && batch->obs)   // (the posterior: eval_refuse has refused these already)
    return fail(h, SLODE_EINVAL, "slode_joint_band: observation strides (%lld, %lld, %lld) are not taken: the observed deviation needs dense "
                                 "[B,T,C] or [B,C,T] observations; reduce recon_samples instead", (long long)os[0], (long long)os[1], (long long)os[2]);
  d.lds_tables = "step table, staged weights, moment / value table, deviations";
  d.lds_advice = "fewer draws fit (slode_joint_band_plan), or reduce recon_samples instead"; d.lds_per_draw = true;
  if ((rc = eval_lds(h, s, d, slode_joint_band_lds_bytes(*s, num_samples, h->ode_generic), SLODE_JOINT_BAND_LDS_MAX)) != SLODE_OK) return rc;
  a.obs = batch->obs; a.t_major = t_major ? 1 : 0; a.n_levels = n_levels; a.sd_floor = sd_floor;
  a.mean = mean; a.sd = sd; a.crit = crit; a.joint = joint; a.obs_dev = obs_dev; a.dev_out = dev_out;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_joint_band);   // (rng_calls stays 1: the counter moves as slode_recon_moments moves it)
}

// ---- forecast: the solve grid is the call's own argument (include/slode.h) ----
int slode_num_stage_times_n(const slode_shape* s, int n_times) {
  if (!s || n_times < 2 || n_times > SLODE_FORECAST_MAX_T) return SLODE_EINVAL;
  if (is_adaptive(s->method)) return 1;
  return fixed_step_times(s->method) * (n_times - 1) + 1;
}

// slode_stage_times for a grid of n_times points: the same launcher on a shape copy with T = n_times (it reads T and method alone)
int slode_stage_times_n(slode_handle h, const slode_shape* s, int n_times, const float* times, float* stage_t, void* stream) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (!s) return fail(h, SLODE_EINVAL, "shape is NULL");
  if (s->method < SLODE_EULER || s->method > SLODE_ADAPTIVE_HEUN) return fail(h, SLODE_EINVAL, "slode_stage_times_n: unknown method %d", s->method);
  if (n_times < 2 || n_times > SLODE_FORECAST_MAX_T)
    return fail(h, SLODE_EINVAL, "slode_stage_times_n: n_times = %d out of range [2, %d]", n_times, SLODE_FORECAST_MAX_T);
  if (!times || !stage_t) return fail(h, SLODE_EINVAL, "times / stage_t is NULL");
  slode_shape sn = *s;
  sn.T = n_times;
  HIP_TRY(h, slode_launch_stage_times(sn, times, stage_t, (hipStream_t)stream));
  return SLODE_OK;
}

// The window rule.  The LDS figure is monotone in the window, so "the largest that fits" is a bisection.  why: the refusal.
static int forecast_plan(const slode_shape& s, int T_out, int ns, int states, int window, int force_generic, int* window_out, size_t* lds_out,
                         char* why, size_t why_n) {
  const size_t budget = SLODE_FORECAST_LDS_MAX;
  const int NS = T_out - 1;
  auto bytes = [&](int W) { return slode_forecast_lds_bytes(s, ns, states, W, force_generic); };
  int W;
  if (window > 0) {
    W = window < NS ? window : NS;
    if (bytes(W) > budget) {
      snprintf(why, why_n, "window = %d does not fit: its LDS tables of S = %d, C = %d, num_samples = %d%s (%zu B: staged weights, carry, step table, "
               "moments) exceed the budget of %zu B; pass window = 0 to let the library choose", W, s.S, s.C, ns, states ? ", states" : "", bytes(W), budget);
      return SLODE_EINVAL;
    }
  } else {
    if (bytes(1) > budget) {
      snprintf(why, why_n, "num_samples = %d: the carry table [num_samples][S = %d] leaves no room for one grid step beside it (%zu B of a budget of "
               "%zu B); fewer draws per call fit", ns, s.S, bytes(1), budget);
      return SLODE_EINVAL;
    }
    int lo = 1, hi = NS;   // bytes(lo) fits
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (bytes(mid) <= budget) lo = mid; else hi = mid - 1;
    }
    W = lo;
    if (W < NS) {   // not the whole grid: full rounds of the 256 threads in M4 where the room allows, else full waves
      if (W >= 256) W -= W % 256;
      else if (W >= 64) W -= W % 64;
    }
  }
  *window_out = W;
  *lds_out = bytes(W);
  return SLODE_OK;
}

int slode_forecast_plan(const slode_shape* s, int T_out, int num_samples, int want_states, int window, int* window_out, size_t* lds_bytes) {
  if (int rc = plan_open("slode_forecast_plan", s, !window_out || !lds_bytes, "window_out / lds_bytes")) return rc;
  if (T_out < 2 || T_out > SLODE_FORECAST_MAX_T) return fail(nullptr, SLODE_EINVAL, "slode_forecast_plan: T_out = %d out of range [2, %d]", T_out, SLODE_FORECAST_MAX_T);
  if (num_samples < 1) return fail(nullptr, SLODE_EINVAL, "slode_forecast_plan: num_samples = %d < 1", num_samples);
  if (window < 0) return fail(nullptr, SLODE_EINVAL, "slode_forecast_plan: window = %d < 0", window);
  char why[384];
  if (forecast_plan(*s, T_out, num_samples, want_states ? 1 : 0, window, 0, window_out, lds_bytes, why, sizeof(why)) != SLODE_OK)
    return fail(nullptr, SLODE_EINVAL, "slode_forecast_plan: %s", why);
  return SLODE_OK;
}

// Mean / sd of the head curves (and of the ODE state) over num_samples latent draws on the caller's output grid (include/slode.h): the
// refusals of slode_recon_moments for the same is_post without its LDS rung, then the call's own rungs, the plan's refusal as its LDS
// rung; then slode_recon_moments' launches with the windowed kernel in place of its own.
int slode_forecast_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                           const float* stage_t, const slode_batch* batch, int is_post, int num_samples, const float* times_out,
                           const float* stage_t_out, int T_out, int window, float* mean, float* sd, float* x_mean, float* x_sd, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const DrawsCall d("slode_forecast_moments", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
                    "reduce forecast_samples instead", nullptr);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (!times_out || !stage_t_out) return fail(h, SLODE_EINVAL, "slode_forecast_moments: times_out / stage_t_out is NULL");
  if (T_out < 2 || T_out > SLODE_FORECAST_MAX_T)
    return fail(h, SLODE_EINVAL, "slode_forecast_moments: T_out = %d out of range [2, %d]", T_out, SLODE_FORECAST_MAX_T);
  if (!mean) return fail(h, SLODE_EINVAL, "slode_forecast_moments: mean is NULL");
  if (window < 0) return fail(h, SLODE_EINVAL, "slode_forecast_moments: window = %d < 0", window);
  ForecastMomentsLaunch a{};
  size_t lds = 0;
  char why[384];
  if (forecast_plan(*s, T_out, num_samples, (x_mean || x_sd) ? 1 : 0, window, h->ode_generic, &a.window, &lds, why, sizeof(why)) != SLODE_OK)
    return fail(h, SLODE_EINVAL, "slode_forecast_moments: %s", why);
  a.T_out = T_out; a.mean = mean; a.sd = sd; a.x_mean = x_mean; a.x_sd = x_sd;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_forecast_moments, times_out, stage_t_out);   // (the kernel solves on the output grid)
}

// ---- forecast summaries: slode_forecast_moments' windowed solve, slode_curve_summary's functionals from first_point on (include/slode.h) ----
// The window rule of forecast_plan on this kernel's carve, which has no num_samples term.  why: the refusal.
static int forecast_summary_plan(const slode_shape& s, int T_out, int window, int force_generic, int* window_out, size_t* lds_out, char* why, size_t why_n) {
  const size_t budget = SLODE_FORECAST_SUMMARY_LDS_MAX;
  const int NS = T_out - 1;
  auto bytes = [&](int W) { return slode_forecast_summary_lds_bytes(s, W, force_generic); };
  int W;
  if (window > 0) {
    W = window < NS ? window : NS;
    if (bytes(W) > budget) {
      snprintf(why, why_n, "window = %d does not fit: its LDS tables of S = %d, C = %d (%zu B: staged weights, carry, step table, grid and node "
               "weights, value table, moment triples) exceed the budget of %zu B; pass window = 0 to let the library choose", W, s.S, s.C, bytes(W), budget);
      return SLODE_EINVAL;
    }
  } else {
    if (bytes(1) > budget) {
      snprintf(why, why_n, "the staged weights of S = %d, C = %d leave no room for one grid step beside them (%zu B of a budget of %zu B)", s.S, s.C,
               bytes(1), budget);
      return SLODE_EINVAL;
    }
    int lo = 1, hi = NS;   // bytes(lo) fits
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (bytes(mid) <= budget) lo = mid; else hi = mid - 1;
    }
    W = lo;
    if (W < NS) {   // not the whole grid: full rounds of the 256 threads in M4 where the room allows, else full waves
      if (W >= 256) W -= W % 256;
      else if (W >= 64) W -= W % 64;
    }
  }
  *window_out = W;
  *lds_out = bytes(W);
  return SLODE_OK;
}

int slode_forecast_summary_plan(const slode_shape* s, int T_out, int window, int* window_out, size_t* lds_bytes) {
  if (int rc = plan_open("slode_forecast_summary_plan", s, !window_out || !lds_bytes, "window_out / lds_bytes")) return rc;
  if (T_out < 2 || T_out > SLODE_FORECAST_MAX_T)
    return fail(nullptr, SLODE_EINVAL, "slode_forecast_summary_plan: T_out = %d out of range [2, %d]", T_out, SLODE_FORECAST_MAX_T);
  if (window < 0) return fail(nullptr, SLODE_EINVAL, "slode_forecast_summary_plan: window = %d < 0", window);
  char why[384];
  if (forecast_summary_plan(*s, T_out, window, 0, window_out, lds_bytes, why, sizeof(why)) != SLODE_OK)
    return fail(nullptr, SLODE_EINVAL, "slode_forecast_summary_plan: %s", why);
  return SLODE_OK;
}

// Mean / sd over num_samples latent draws of the eight curve functionals on times_out[first_point .. T_out) (include/slode.h): the refusals of
// slode_forecast_moments for the same is_post up to its grid rungs, then the call's own, the plan's refusal as its LDS rung; then
// slode_forecast_moments' launches with the summary kernel in place of its own.
int slode_forecast_summary(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                           const float* stage_t, const slode_batch* batch, int is_post, int num_samples, const float* times_out,
                           const float* stage_t_out, int T_out, int first_point, int window, const float* thr, int sense, float* mean, float* sd,
                           void* workspace, size_t workspace_bytes, void* stream) {
  static const char* N = "slode_forecast_summary";
  const DrawsCall d(N, "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
                    "reduce forecast_samples instead", nullptr);
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if (!times_out || !stage_t_out) return fail(h, SLODE_EINVAL, "%s: times_out / stage_t_out is NULL", N);
  if (T_out < 2 || T_out > SLODE_FORECAST_MAX_T) return fail(h, SLODE_EINVAL, "%s: T_out = %d out of range [2, %d]", N, T_out, SLODE_FORECAST_MAX_T);
  if (first_point < 0 || first_point > T_out - 1)
    return fail(h, SLODE_EINVAL, "%s: first_point = %d out of range [0, T_out - 1 = %d]", N, first_point, T_out - 1);
  if (sense != 1 && sense != -1) return fail(h, SLODE_EINVAL, "%s: sense = %d is neither +1 (beyond: above thr) nor -1 (below)", N, sense);
  if (thr)
    for (int c = 0; c < s->C; ++c)
      if (!std::isfinite(thr[c])) return fail(h, SLODE_EINVAL, "%s: thr[%d] = %g is not finite", N, c, (double)thr[c]);
  if (!mean) return fail(h, SLODE_EINVAL, "%s: mean is NULL", N);
  if (window < 0) return fail(h, SLODE_EINVAL, "%s: window = %d < 0", N, window);
  ForecastSummaryLaunch a{};
  size_t lds = 0;
  char why[384];
  if (forecast_summary_plan(*s, T_out, window, h->ode_generic, &a.window, &lds, why, sizeof(why)) != SLODE_OK)
    return fail(h, SLODE_EINVAL, "%s: %s", N, why);
  a.T_out = T_out; a.first_point = first_point; a.mean = mean; a.sd = sd; a.has_thr = thr ? 1 : 0; a.sense = sense;
  for (int c = 0; c < SLODE_MAX_C; ++c) a.thr[c] = (thr && c < s->C) ? thr[c] : 0.f;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, s->B, workspace, workspace_bytes, stream,
                     slode_launch_forecast_summary, times_out, stage_t_out);   // (the kernel solves on the output grid)
}

// ---- cohort curves: the draws of slode_recon_moments reduced by cohort (include/slode.h) ----
// the call's own argument rungs, shared by the plan and the call (who: the speaker)
static const char* cohort_sizes(const slode_shape* s, int M, int G, int chunk, char* why, size_t why_n) {
  if (M < 0 || M > s->B) { snprintf(why, why_n, "M = %d out of range [0, B = %d]", M, s->B); return why; }
  if (G < 1 || G > SLODE_COHORT_MAX_G) { snprintf(why, why_n, "G = %d out of range [1, %d]", G, SLODE_COHORT_MAX_G); return why; }
  if (chunk < 0 || chunk > SLODE_COHORT_MAX_CHUNK) { snprintf(why, why_n, "chunk = %d out of range [0, %d]", chunk, SLODE_COHORT_MAX_CHUNK); return why; }
  return nullptr;
}

// the plan entry points: host arithmetic only (the compiled state dims, no SLODE_ODE_GENERIC)
static int cohort_plan_for(const char* who, size_t (*lds_bytes_of)(const slode_shape&, int), int budget, const char* tables, size_t partial_bytes,
                           const slode_shape* s, int M, int G, int num_samples, int chunk, int* chunk_out, int* n_partials, size_t* lds_bytes,
                           size_t* scratch_bytes) {
  if (int rc = plan_open(who, s, !chunk_out || !n_partials || !lds_bytes || !scratch_bytes, "chunk_out / n_partials / lds_bytes / scratch_bytes")) return rc;
  if (num_samples < 1) return fail(nullptr, SLODE_EINVAL, "%s: num_samples = %d < 1", who, num_samples);
  char why[128];
  if (cohort_sizes(s, M, G, chunk, why, sizeof(why))) return fail(nullptr, SLODE_EINVAL, "%s: %s", who, why);
  const size_t lds = lds_bytes_of(*s, 0);
  if (lds > (size_t)budget)
    return fail(nullptr, SLODE_EINVAL, "%s: the LDS tables of T = %d, S = %d, C = %d (%zu B: %s) exceed the budget of %d B", who, s->T, s->S, s->C,
                lds, tables, budget);
  const int R = chunk > 0 ? chunk : slode_cohort_default_chunk(M);
  const CohortScratch sc = slode_cohort_scratch(M, G, R, partial_bytes);
  *chunk_out = R; *n_partials = sc.n_partials; *lds_bytes = lds; *scratch_bytes = sc.bytes;
  return SLODE_OK;
}
int slode_cohort_plan(const slode_shape* s, int M, int G, int num_samples, int chunk, int* chunk_out, int* n_partials, size_t* lds_bytes,
                      size_t* scratch_bytes) {
  return cohort_plan_for("slode_cohort_plan", slode_cohort_lds_bytes, SLODE_COHORT_LDS_MAX, "step table, six-float table, observation sum, staged weights",
                         s ? slode_cohort_partial_bytes(*s) : 0, s, M, G, num_samples, chunk, chunk_out, n_partials, lds_bytes, scratch_bytes);
}
int slode_calibration_plan(const slode_shape* s, int M, int G, int num_samples, int chunk, int* chunk_out, int* n_partials, size_t* lds_bytes,
                           size_t* scratch_bytes) {
  return cohort_plan_for("slode_calibration_plan", slode_calibration_lds_bytes, SLODE_CALIBRATION_LDS_MAX,
                         "step table, counts, fp64 sums, observations, staged weights", s ? slode_calibration_partial_bytes(*s) : 0, s, M, G,
                         num_samples, chunk, chunk_out, n_partials, lds_bytes, scratch_bytes);
}

// The argument rungs the two calls share, each group where the call's own ladder has it.  First: members / offsets, cohort_sizes ...
static int cohort_index_args(slode_handle h, const char* who, const slode_shape* s, const int32_t* members, const int32_t* offsets, int M, int G, int chunk) {
  if (M > 0 && (!members || !offsets)) return fail(h, SLODE_EINVAL, "%s: members / offsets is NULL with M = %d", who, M);
  char why[128];
  if (cohort_sizes(s, M, G, chunk, why, sizeof(why))) return fail(h, SLODE_EINVAL, "%s: %s", who, why);
  return SLODE_OK;
}
// ... then (need_obs) the dense observation strides -- need: who reads them -- with c.t_major, and the scratch's alignment ...
static int cohort_obs_args(slode_handle h, const char* who, const slode_shape* s, const slode_batch* batch, bool need_obs, const char* need,
                           void* scratch, CohortPart& c) {
  const int64_t* os = batch->obs_strides;
  bool t_major;
  if (!obs_dense(s, os, &t_major) && need_obs)
    return fail(h, SLODE_EINVAL, "%s: observation strides (%lld, %lld, %lld) are not taken: %s need dense [B,T,C] or "
                                 "[B,C,T] observations; reduce recon_samples instead", who, (long long)os[0], (long long)os[1], (long long)os[2], need);
  if (!scratch || ((uintptr_t)scratch & 15)) return fail(h, SLODE_EINVAL, "%s: scratch is NULL or not 16-byte aligned", who);
  c.obs = need_obs ? batch->obs : nullptr; c.sb = os[0]; c.t_major = t_major ? 1 : 0; c.scratch = scratch;
  return SLODE_OK;
}
// ... and, after the LDS rung, the chunk and the scratch's size (plan: the entry point that gives it); n_partials: what the grid walks
static int cohort_scratch_args(slode_handle h, const char* who, const char* plan, const int32_t* members, const int32_t* offsets, int M, int G,
                               int chunk, size_t partial_bytes, size_t scratch_bytes, CohortPart& c, int* n_partials) {
  c.members = members; c.offsets = offsets; c.M = M; c.G = G; c.chunk = chunk > 0 ? chunk : slode_cohort_default_chunk(M);
  const CohortScratch sc = slode_cohort_scratch(M, G, c.chunk, partial_bytes);
  if (scratch_bytes < sc.bytes) return fail(h, SLODE_ENOSPC, "%s: scratch_bytes %zu B < required %zu B (%s)", who, scratch_bytes, sc.bytes, plan);
  *n_partials = sc.n_partials;
  return SLODE_OK;
}

// Refusals first -- slode_recon_moments' for the same is_post, then the call's own; nothing launched, no draw consumed -- then, for the
// posterior, the fold + encoder launches of a forward-only step; then cohort_plan, cohort_moments, cohort_merge.
int slode_cohort_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                         const float* stage_t, const slode_batch* batch, int is_post, int num_samples, const int32_t* members,
                         const int32_t* offsets, int M, int G, int chunk, float clip_min, float* mean, float* sd, float* sd_subjects,
                         float* obs_mean, float* l1, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  const DrawsCall d("slode_cohort_moments", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
                    "reduce recon_samples instead", "step table, six-float table, observation sum, staged weights");
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if ((rc = cohort_index_args(h, d.name, s, members, offsets, M, G, chunk)) != SLODE_OK) return rc;
  if (!mean) return fail(h, SLODE_EINVAL, "slode_cohort_moments: mean is NULL");
  const bool want_obs = obs_mean || l1;
  if (want_obs && !batch->obs) return fail(h, SLODE_EINVAL, "slode_cohort_moments: obs_mean / l1 need observations (batch->obs is NULL)");
  CohortMomentsLaunch a{};
  int n_partials = 0;
  if ((rc = cohort_obs_args(h, d.name, s, batch, want_obs, "obs_mean / l1", scratch, a.c)) != SLODE_OK) return rc;
  if ((rc = eval_lds(h, s, d, slode_cohort_lds_bytes(*s, h->ode_generic), SLODE_COHORT_LDS_MAX)) != SLODE_OK) return rc;
  if ((rc = cohort_scratch_args(h, d.name, "slode_cohort_plan", members, offsets, M, G, chunk, slode_cohort_partial_bytes(*s), scratch_bytes, a.c,
                                &n_partials)) != SLODE_OK) return rc;
  a.clip_min = clip_min; a.mean = mean; a.sd = sd; a.sd_subjects = sd_subjects; a.obs_mean = obs_mean; a.l1 = l1;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, n_partials, workspace, workspace_bytes, stream,
                     slode_launch_cohort_moments);
}

// ---- calibration: the draws of slode_recon_moments compared with the observations, counted by cohort (include/slode.h) ----
// Refusals first -- slode_cohort_moments' for the same is_post, observations required on both sides; nothing launched, no draw consumed --
// then, for the posterior, the fold + encoder launches of a forward-only step; then cohort_plan, calibration, calibration_merge.
int slode_calibration(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                      const float* stage_t, const slode_batch* batch, int is_post, int num_samples, const int32_t* members,
                      const int32_t* offsets, int M, int G, int chunk, int32_t* below, int32_t* inside, int32_t* cross, float* pinball,
                      float* width, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  DrawsCall d("slode_calibration", "batch / times / stage_t / workspace", !batch || !times || !stage_t || !workspace, num_samples, is_post,
              "reduce recon_samples instead", "step table, counts, fp64 sums, observations, staged weights");
  d.obs_null = "the curves are compared with observations (batch->obs is NULL)";
  int rc = eval_open(h, s, lay, params, batch, d);
  if (rc != SLODE_OK) return rc;
  if ((rc = cohort_index_args(h, d.name, s, members, offsets, M, G, chunk)) != SLODE_OK) return rc;
  if (!below) return fail(h, SLODE_EINVAL, "slode_calibration: below is NULL");
  CalibrationLaunch a{};
  int n_partials = 0;
  if ((rc = cohort_obs_args(h, d.name, s, batch, true, "the comparisons", scratch, a.c)) != SLODE_OK) return rc;
  if ((rc = eval_lds(h, s, d, slode_calibration_lds_bytes(*s, h->ode_generic), SLODE_CALIBRATION_LDS_MAX)) != SLODE_OK) return rc;
  if ((rc = cohort_scratch_args(h, d.name, "slode_calibration_plan", members, offsets, M, G, chunk, slode_calibration_partial_bytes(*s),
                                scratch_bytes, a.c, &n_partials)) != SLODE_OK) return rc;
  a.below = below; a.inside = inside; a.cross = cross; a.pinball = pinball; a.width = width;
  return draws_close(h, s, lay, d, a, params, times, stage_t, batch, is_post, num_samples, n_partials, workspace, workspace_bytes, stream,
                     slode_launch_calibration);
}

size_t slode_grad_payload_floats(const slode_shape* s, const slode_layout* lay, int kind) {
  if (check_shape(s) || !lay) return 0;
  const int part = kind == SLODE_SVI_AUX ? lay->cstd - lay->aux_w1[0] : lay->n_params - lay->ode_begin;
  return (size_t)payload_map(*s, part).total;
}

int slode_grad_partial(slode_handle h, const slode_shape* s, const slode_layout* lay, int kind, const float* params, const float* times,
                       const float* stage_t, const slode_batch* batch, float* payload, void* workspace, size_t workspace_bytes, void* stream) {
  StepCall c;
  c.phase = STEP_PARTIAL; c.params = params; c.times = times; c.stage_t = stage_t; c.payload = payload;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  const int rc = batch_call(h, s, kind, batch, &c);
  return rc != SLODE_OK ? rc : elbo_step_impl(h, s, lay, c);
}

int slode_grad_apply(slode_handle h, const slode_shape* s, const slode_layout* lay, int kind, float* params, const int64_t obs_strides[3],
                     const float* payload, float* loss_out, float* grads, void* workspace, size_t workspace_bytes, const slode_adam* adam,
                     void* stream) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (kind != SLODE_SVI_MAIN && kind != SLODE_SVI_AUX) return fail(h, SLODE_EINVAL, "kind must be SLODE_SVI_MAIN or SLODE_SVI_AUX");
  StepCall c;
  c.kind = kind; c.phase = STEP_APPLY; c.params = params; c.obs_strides = obs_strides; c.payload = const_cast<float*>(payload);
  c.loss_out = loss_out; c.grads = grads; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  const int rc = adam_args(h, "slode_grad_apply with Adam", "both", lay, params, adam, &c);
  return rc != SLODE_OK ? rc : elbo_step_impl(h, s, lay, c);
}

int slode_fold_invalidate(slode_handle h) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  h->fold_valid = 0;
  return SLODE_OK;
}

int slode_rng_seed(slode_handle h, uint64_t seed, int64_t first_trajectory) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (first_trajectory < 0) return fail(h, SLODE_EINVAL, "first_trajectory < 0");
  h->rng_seed = seed; h->rng_b0 = first_trajectory; h->rng_counter = 0;
  return SLODE_OK;
}

int slode_rng_set_counter(slode_handle h, uint64_t n) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  h->rng_counter = n;
  return SLODE_OK;
}

int slode_rng_get(slode_handle h, uint64_t* seed, int64_t* first_trajectory, uint64_t* n) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (seed) *seed = h->rng_seed;
  if (first_trajectory) *first_trajectory = h->rng_b0;
  if (n) *n = h->rng_counter;
  return SLODE_OK;
}

int slode_rng_normal(slode_handle h, uint64_t n, int32_t B, int32_t L, float* eps_out, uint32_t* raw_out, void* stream) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (B < 1 || L < 1 || L > SLODE_MAX_L || (!eps_out && !raw_out)) return fail(h, SLODE_EINVAL, "slode_rng_normal: B >= 1, 1 <= L <= 64 and an output required");
  HIP_TRY(h, slode_launch_rng_fill(rng_of(h, n), B, L, eps_out, raw_out, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_sample_normal(slode_handle h, int32_t B, int32_t L, const float* loc, const float* scale, float* z_out, void* stream) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (B < 1 || L < 1 || L > SLODE_MAX_L || !loc || !scale || !z_out) return fail(h, SLODE_EINVAL, "slode_sample_normal: B >= 1, 1 <= L <= 64, loc / scale / z_out required");
  HIP_TRY(h, slode_launch_rng_fill(rng_of(h, h->rng_counter++), B, L, z_out, nullptr, (hipStream_t)stream, loc, scale));
  return SLODE_OK;
}

int slode_dynamics_eval(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, float t,
                        const float* state, const float* z, float* out, void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!state || !z || !out) return fail(h, SLODE_EINVAL, "state / z / out is NULL");
  HIP_TRY(h, slode_launch_dynamics_eval(*s, *lay, params, t, state, z, out, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_initialize_state(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* z, float* x0,
                           void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!z || !x0) return fail(h, SLODE_EINVAL, "z / x0 is NULL");
  HIP_TRY(h, slode_launch_init_state(*s, *lay, params, z, x0, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_prior_nets(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* u, float* loc,
                     float* scale, void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!loc || !scale || (s->n_groups > 0 && !u)) return fail(h, SLODE_EINVAL, "u / loc / scale is NULL");
  HIP_TRY(h, slode_launch_prior_nets(*s, *lay, params, u, loc, scale, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_label_heads(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* z, float* out,
                      void* stream) {
  const char* why = check_common(h, s, lay, params);
  if (why) return fail(h, SLODE_EINVAL, "%s", why);
  if (!z || !out) return fail(h, SLODE_EINVAL, "z / out is NULL");
  if (s->n_aux < 1) return fail(h, SLODE_EINVAL, "the shape has no label heads");
  HIP_TRY(h, slode_launch_label_heads(*s, *lay, params, z, out, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_dopri5_step_counts(slode_handle h, const slode_shape* s, const slode_layout* lay, const void* workspace, size_t workspace_bytes,
                             int* counts, void* stream) {
  if (!h) return SLODE_EINVAL;
  if (!s || !lay || !workspace || !counts || !is_adaptive(s->method))
    return fail(h, SLODE_EINVAL, "slode_dopri5_step_counts: adaptive-method shape, workspace and output required");
  if (check_shape(s)) return fail(h, SLODE_EINVAL, "%s", check_shape(s));
  if (workspace_bytes < slode_workspace_bytes(h, s)) return fail(h, SLODE_EINVAL, "slode_dopri5_step_counts: workspace too small");
  const Workspace w = carve(h, *s, *lay, const_cast<void*>(workspace));
  HIP_TRY(h, hipMemcpyAsync(counts, w.dp_nrec, sizeof(int) * (size_t)s->B * particles_of(*s), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SLODE_OK;
}

int slode_adam_region(slode_handle h, int64_t lo, int64_t hi, int64_t step_delta) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (lo < 0 || hi < lo || hi > 0x7fffffff) return fail(h, SLODE_EINVAL, "bad Adam region [%lld, %lld)", (long long)lo, (long long)hi);
  h->adam_lo2 = (int)lo; h->adam_hi2 = (int)hi; h->adam_delta2 = step_delta;
  return SLODE_OK;
}

int slode_profile_enable(slode_handle h, int on) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (on != 0 && on != 1) return fail(h, SLODE_EINVAL, "profile mode %d: 0 (off) or 1 (per-kernel timestamps)", on);
  if (on && !h->ev_ready) {
    for (int i = 0; i < SLODE_CLOCK_MAX; ++i) {
      HIP_TRY(h, hipEventCreate(&h->clk.ev[i][0]));
      HIP_TRY(h, hipEventCreate(&h->clk.ev[i][1]));
    }
    h->ev_ready = 1;
  }
  h->profile = on;
  h->clk.n = 0;
  return SLODE_OK;
}

int slode_profile_read(slode_handle h, int max_kernels, const char** names, float* us) {
  if (!h || !names || !us || max_kernels < 1) return fail(h, SLODE_EINVAL, "handle / names / us is NULL or max_kernels < 1");
  if (!h->profile) return fail(h, SLODE_EINVAL, "profiling is off");
  if (h->clk.n < 1) return fail(h, SLODE_EINVAL, "no profiled step has been recorded on this handle");
  const int n = h->clk.n < max_kernels ? h->clk.n : max_kernels;
  for (int i = 0; i < n; ++i) {
    float ms = 0.f;
    HIP_TRY(h, hipEventSynchronize(h->clk.ev[i][1]));
    HIP_TRY(h, hipEventElapsedTime(&ms, h->clk.ev[i][0], h->clk.ev[i][1]));
    names[i] = h->clk.name[i];
    us[i] = 1e3f * ms;
  }
  return n;
}

int slode_adam_step(slode_handle h, int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float lr,
                    float beta1, float beta2, float eps, int64_t step, void* stream) {
  if (!h) return fail(nullptr, SLODE_EINVAL, "handle is NULL");
  if (n < 0 || step < 1 || !params || !grads || !exp_avg || !exp_avg_sq) return fail(h, SLODE_EINVAL, "bad Adam arguments");
  if (n == 0) return SLODE_OK;
  AdamHost a{params, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, n};
  a.lo2 = h->adam_lo2; a.hi2 = h->adam_hi2; a.delta2 = h->adam_delta2;
  h->fold_valid = 0;   // the weights change outside a step's chain launch: the next step folds again
  ClockScope clock_scope(h, true);
  HIP_TRY(h, slode_launch_adam_k(n, grads, a, (hipStream_t)stream));
  return SLODE_OK;
}

}  // extern "C"
