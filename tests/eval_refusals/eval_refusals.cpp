// Every refusing configuration of the four eval-side entry points (slode_eval_stats, slode_recon_moments, slode_traj_bounds,
// slode_intervene_moments), on a hand-filled handle: no slode_create, no HIP call, no device.  One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// tests/golden/eval_refusals.txt holds these lines; tests/test_host_cpu.py compares.  No refusal touches HIP and a refused call
// launches nothing, so this program makes NO call that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 eval_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

enum Call { STATS = 0, RECON = 1, BOUNDS = 2, INTERVENE = 3 };
static const char* const CALL_NAME[] = {"eval_stats", "recon_moments", "traj_bounds", "intervene_moments"};

struct Cfg : BaseCfg {
  float *out = DEV, *second = DEV;   // out / mean / bounds / cf_mean, and sd / loss_kb / cf_sd
  unsigned int mask = 0;
  const float* cf[SLODE_MAX_LABELS] = {DEV, DEV, nullptr, nullptr};
  bool no_cf = false;
};
// the proc-like shape whose tables exceed the LDS: T = 1024, S = 8, C = 4, dense [B,C,T] observations
static void big_tables(Cfg& c) {
  c.s.T = 1024; c.s.S = 8; c.s.C = 4;
  c.b.obs_strides[0] = (int64_t)c.s.C * c.s.T; c.b.obs_strides[1] = c.s.T; c.b.obs_strides[2] = 1;
}

static int call(int which, Cfg& c, const Head& a, const char** column) {
  const float* const* cf = c.no_cf ? nullptr : c.cf;
  *column = CALL_NAME[which];
  switch (which) {
    case STATS: return slode_eval_stats(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.out, c.ws, c.ws_bytes, nullptr);
    case RECON: return slode_recon_moments(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.out, c.second, c.ws, c.ws_bytes, nullptr);
    case BOUNDS: return slode_traj_bounds(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.draws, c.out, c.second, c.ws, c.ws_bytes, nullptr);
    default: return slode_intervene_moments(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, cf, c.mask, c.draws, c.out, c.second, DEV, DEV, c.ws, c.ws_bytes, nullptr);
  }
}

#define ALL {STATS, RECON, BOUNDS, INTERVENE}
#define DRAWN {RECON, BOUNDS, INTERVENE}

int main() {
  // ---- NULL pointers, group by group
  each("handle NULL", ALL, [](Cfg& c) { c.no_handle = true; });
  each("shape NULL", ALL, [](Cfg& c) { c.no_shape = true; });
  each("layout NULL", ALL, [](Cfg& c) { c.no_layout = true; });
  each("params NULL", ALL, [](Cfg& c) { c.no_params = true; });
  each("batch NULL", ALL, [](Cfg& c) { c.no_batch = true; });
  each("first output NULL", {STATS, RECON, BOUNDS}, [](Cfg& c) { c.out = nullptr; });
  each("times NULL", DRAWN, [](Cfg& c) { c.times = nullptr; });
  each("stage_t NULL", DRAWN, [](Cfg& c) { c.stage_t = nullptr; });
  each("workspace NULL", DRAWN, [](Cfg& c) { c.ws = nullptr; });
  each("times NULL (found by the step set-up)", {STATS}, [](Cfg& c) { c.times = nullptr; });
  each("workspace NULL (found by the step set-up)", {STATS}, [](Cfg& c) { c.ws = nullptr; });
  each("bad shape", ALL, [](Cfg& c) { c.s.T = 1; });
  // ---- the draw count
  each("draws 0", DRAWN, [](Cfg& c) { c.draws = 0; });
  each("draws 2^30", DRAWN, [](Cfg& c) { c.draws = 1 << 30; });
  // ---- what the fused kernels do not take
  for (int m : {SLODE_DOPRI5, SLODE_BOSH3, SLODE_FEHLBERG2, SLODE_ADAPTIVE_HEUN}) {
    char name[64];
    snprintf(name, sizeof(name), "adaptive method %d", m);
    each(name, ALL, [m](Cfg& c) { c.s.method = m; });
  }
  each("particles 2", ALL, [](Cfg& c) { c.s.particles = 2; });
  each("fold_on", ALL, [](Cfg& c) { c.ctx.fold_on = 1; });
  each("ode_pack", ALL, [](Cfg& c) { c.ctx.ode_pack = 4; });
  each("ode_alg", ALL, [](Cfg& c) { c.ctx.ode_alg = 1; });
  // ---- the observations
  each("obs NULL", ALL, [](Cfg& c) { c.b.obs = nullptr; });
  each("padded strides", ALL, [](Cfg& c) { c.b.obs_strides[0] += 8; });
  each("channel-major strides of another T", ALL, [](Cfg& c) { c.b.obs_strides[1] = c.s.T + 1; c.b.obs_strides[2] = 1; });
  each("no_fold", ALL, [](Cfg& c) { c.ctx.no_fold = 1; });
  each("prior: obs NULL, padded strides, no_fold; workspace too small", {RECON},
       [](Cfg& c) { c.is_post = 0; c.b.obs = nullptr; c.b.obs_strides[0] += 8; c.ctx.no_fold = 1; c.ws_bytes = 64; });
  // ---- the LDS budget (with a workspace too small behind it: the budget is asked first; the tables of eval_stats and traj_bounds fit
  //      the LDS even at the largest shape, so those two name the workspace)
  each("LDS: T 1024, S 8, C 4", ALL, [](Cfg& c) { big_tables(c); c.ws_bytes = 64; });
  each("LDS: T 1024, S 8, C 4, run-time S", ALL, [](Cfg& c) { big_tables(c); c.ctx.ode_generic = 1; c.ws_bytes = 64; });
  each("LDS: num_draws 100000", {BOUNDS}, [](Cfg& c) { c.draws = 100000; c.ws_bytes = 64; });
  // ---- the label tensors
  each("label columns 3, n_u 2", ALL, [](Cfg& c) { c.b.label_width[1] = 2; });
  each("n_labels 5", ALL, [](Cfg& c) { c.b.n_labels = 5; });
  each("label tensor 1 NULL", ALL, [](Cfg& c) { c.b.labels[1] = nullptr; });
  each("no labels, conditional prior groups", ALL, [](Cfg& c) { c.b.n_labels = 0; });
  each("prior without labels", {RECON}, [](Cfg& c) { c.is_post = 0; c.b.n_labels = 0; });
  // ---- slode_intervene_moments alone
  each("mask bit beyond n_groups", {INTERVENE}, [](Cfg& c) { c.mask = 4; });
  each("cf_labels NULL, mask 1", {INTERVENE}, [](Cfg& c) { c.mask = 1; c.no_cf = true; });
  each("read cf tensor NULL", {INTERVENE}, [](Cfg& c) { c.mask = 2; c.cf[1] = nullptr; });
  each("mask 3, no labels", {INTERVENE}, [](Cfg& c) { c.mask = 3; c.b.n_labels = 0; });
  // ---- slode_traj_bounds alone
  each("unaligned bounds", {BOUNDS}, [](Cfg& c) { c.out = DEV + 1; });
  // ---- the workspace
  each("workspace too small", ALL, [](Cfg& c) { c.ws_bytes = 64; });
  each("prior: workspace too small", {RECON}, [](Cfg& c) { c.is_post = 0; c.ws_bytes = 64; });
  each("unread cf tensor NULL; workspace too small", {INTERVENE}, [](Cfg& c) { c.mask = 1; c.cf[1] = nullptr; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier check of the ladder names the reason
  each("params NULL + batch NULL", ALL, [](Cfg& c) { c.no_params = true; c.no_batch = true; });
  each("output NULL + draws 0", {RECON, BOUNDS}, [](Cfg& c) { c.out = nullptr; c.draws = 0; });
  each("unaligned bounds + draws 0", {BOUNDS}, [](Cfg& c) { c.out = DEV + 1; c.draws = 0; });
  each("draws 0 + adaptive", DRAWN, [](Cfg& c) { c.draws = 0; c.s.method = SLODE_DOPRI5; });
  each("draws 2^30 + adaptive", DRAWN, [](Cfg& c) { c.draws = 1 << 30; c.s.method = SLODE_DOPRI5; });
  each("adaptive + particles 2", ALL, [](Cfg& c) { c.s.method = SLODE_BOSH3; c.s.particles = 2; });
  each("particles 2 + fold_on", ALL, [](Cfg& c) { c.s.particles = 2; c.ctx.fold_on = 1; });
  each("ode_alg + obs NULL", ALL, [](Cfg& c) { c.ctx.ode_alg = 2; c.b.obs = nullptr; });
  each("obs NULL + padded strides", ALL, [](Cfg& c) { c.b.obs = nullptr; c.b.obs_strides[0] += 8; });
  each("padded strides + mask bit beyond n_groups", {INTERVENE}, [](Cfg& c) { c.b.obs_strides[0] += 8; c.mask = 4; });
  each("mask bit beyond n_groups + cf_labels NULL", {INTERVENE}, [](Cfg& c) { c.mask = 5; c.no_cf = true; });
  each("cf_labels NULL + LDS", {INTERVENE}, [](Cfg& c) { big_tables(c); c.mask = 1; c.no_cf = true; });
  each("LDS + label columns 3", ALL, [](Cfg& c) { big_tables(c); c.b.label_width[1] = 2; });
  each("label columns 3 + read cf tensor NULL", {INTERVENE}, [](Cfg& c) { c.b.label_width[1] = 2; c.mask = 2; c.cf[1] = nullptr; });
  each("prior: label columns 3 + workspace too small", {RECON}, [](Cfg& c) { c.is_post = 0; c.b.label_width[1] = 2; });
  each("read cf tensor NULL + workspace too small", {INTERVENE}, [](Cfg& c) { c.mask = 2; c.cf[1] = nullptr; c.ws_bytes = 64; });
  each("label columns 3 + workspace too small", ALL, [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  each("no_fold + workspace too small", ALL, [](Cfg& c) { c.ctx.no_fold = 1; c.ws_bytes = 64; });
  return 0;
}
