// Every refusing configuration of slode_pointwise_density on a hand-filled handle: no slode_create, no HIP call, no device.  One line per case:
//   <case> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_traj_bounds (tests/eval_refusals), then the call's own rungs -- weights, point / summary, loc / scale,
// loss_kb in posterior mode, the LDS tables -- then the label tensors and the workspace.  tests/golden/pointwise_refusals.txt holds these
// lines; tests/test_pointwise_cpu.py compares.  No refusal touches HIP and a refused call launches nothing, so this program makes NO call
// that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 pointwise_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

struct Cfg : BaseCfg {
  int weights = SLODE_PW_IMPORTANCE;
  const float *mask = DEV, *loc = nullptr, *scale = nullptr;
  float *point = DEV, *summary = DEV, *loss_kb = DEV;
};

static int call(int, Cfg& c, const Head& a, const char**) {
  return slode_pointwise_density(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.draws, c.weights, c.mask, c.loc, c.scale, c.point, c.summary,
                                 c.loss_kb, c.ws, c.ws_bytes, nullptr);
}

static void posterior(Cfg& c) { c.weights = SLODE_PW_POSTERIOR; c.loss_kb = nullptr; }

int main() {
  // ---- NULL pointers
  one("handle NULL", [](Cfg& c) { c.no_handle = true; });
  one("shape NULL", [](Cfg& c) { c.no_shape = true; });
  one("layout NULL", [](Cfg& c) { c.no_layout = true; });
  one("params NULL", [](Cfg& c) { c.no_params = true; });
  one("batch NULL", [](Cfg& c) { c.no_batch = true; });
  one("times NULL", [](Cfg& c) { c.times = nullptr; });
  one("stage_t NULL", [](Cfg& c) { c.stage_t = nullptr; });
  one("workspace NULL", [](Cfg& c) { c.ws = nullptr; });
  one("bad shape", [](Cfg& c) { c.s.T = 1; });
  // ---- the draw count
  one("draws 0", [](Cfg& c) { c.draws = 0; });
  one("draws 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  one("posterior: draws 0", [](Cfg& c) { posterior(c); c.draws = 0; });
  // ---- what the fused kernels do not take
  for (int m : {SLODE_DOPRI5, SLODE_BOSH3, SLODE_FEHLBERG2, SLODE_ADAPTIVE_HEUN}) {
    char name[64];
    snprintf(name, sizeof(name), "adaptive method %d", m);
    one(name, [m](Cfg& c) { c.s.method = m; });
  }
  one("particles 2", [](Cfg& c) { c.s.particles = 2; });
  one("fold_on", [](Cfg& c) { c.ctx.fold_on = 1; });
  one("ode_pack", [](Cfg& c) { c.ctx.ode_pack = 4; });
  one("ode_alg", [](Cfg& c) { c.ctx.ode_alg = 1; });
  // ---- the observations
  one("obs NULL", [](Cfg& c) { c.b.obs = nullptr; });
  one("padded strides", [](Cfg& c) { c.b.obs_strides[0] += 8; });
  one("channel-major strides of another T", [](Cfg& c) { c.b.obs_strides[1] = c.s.T + 1; c.b.obs_strides[2] = 1; });
  one("no_fold", [](Cfg& c) { c.ctx.no_fold = 1; });
  // ---- the call's own rungs
  one("weights 2", [](Cfg& c) { c.weights = 2; });
  one("weights -1", [](Cfg& c) { c.weights = -1; });
  one("point NULL", [](Cfg& c) { c.point = nullptr; });
  one("summary NULL", [](Cfg& c) { c.summary = nullptr; });
  one("summary 4 bytes off", [](Cfg& c) { c.summary = DEV + 1; });
  one("loc alone", [](Cfg& c) { c.loc = DEV; });
  one("scale alone", [](Cfg& c) { c.scale = DEV; });
  one("posterior: loss_kb", [](Cfg& c) { posterior(c); c.loss_kb = DEV; });
  one("LDS: T 1000", [](Cfg& c) { c.s.T = 1000; c.b.obs_strides[0] = 3000; c.ws_bytes = 64; });
  one("posterior: LDS: T 1000", [](Cfg& c) { posterior(c); c.s.T = 1000; c.b.obs_strides[0] = 3000; c.ws_bytes = 64; });
  one("LDS: num_draws 100000", [](Cfg& c) { c.draws = 100000; c.ws_bytes = 64; });
  one("LDS: num_draws 2^24", [](Cfg& c) { c.draws = 1 << 24; c.ws_bytes = 64; });
  // ---- the label tensors
  one("label columns 3, n_u 2", [](Cfg& c) { c.b.label_width[1] = 2; });
  one("n_labels 5", [](Cfg& c) { c.b.n_labels = 5; });
  one("label tensor 1 NULL", [](Cfg& c) { c.b.labels[1] = nullptr; });
  // ---- the workspace
  one("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  one("posterior, mask NULL, loc and scale, num_draws 100000; workspace too small",
      [](Cfg& c) { posterior(c); c.mask = nullptr; c.loc = DEV; c.scale = DEV; c.draws = 100000; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  one("params NULL + batch NULL", [](Cfg& c) { c.no_params = true; c.no_batch = true; });
  one("times NULL + draws 0", [](Cfg& c) { c.times = nullptr; c.draws = 0; });
  one("draws 0 + adaptive", [](Cfg& c) { c.draws = 0; c.s.method = SLODE_DOPRI5; });
  one("adaptive + particles 2", [](Cfg& c) { c.s.method = SLODE_BOSH3; c.s.particles = 2; });
  one("ode_alg + obs NULL", [](Cfg& c) { c.ctx.ode_alg = 2; c.b.obs = nullptr; });
  one("no_fold + weights 2", [](Cfg& c) { c.ctx.no_fold = 1; c.weights = 2; });
  one("weights 2 + point NULL", [](Cfg& c) { c.weights = 2; c.point = nullptr; });
  one("summary NULL + loc alone", [](Cfg& c) { c.summary = nullptr; c.loc = DEV; });
  one("scale alone + posterior: loss_kb", [](Cfg& c) { c.weights = SLODE_PW_POSTERIOR; c.scale = DEV; });
  one("posterior: loss_kb + LDS", [](Cfg& c) { c.weights = SLODE_PW_POSTERIOR; c.s.T = 1000; c.b.obs_strides[0] = 3000; });
  one("LDS + label columns 3", [](Cfg& c) { c.draws = 100000; c.b.label_width[1] = 2; });
  one("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // the memory that stands for every output: never written
  bool clean = true;
  for (float v : g_mem) clean = clean && v == 0.f;
  printf("memory that stands for the outputs | %s\n", clean ? "untouched" : "WRITTEN");
  return 0;
}
