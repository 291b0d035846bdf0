// Every refusing configuration of slode_pointwise_loo and slode_loo_plan on a hand-filled handle: no slode_create, no HIP call, no device.
// One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_pointwise_density in posterior mode up to the observations (tests/pointwise_refusals), then the call's
// own rungs -- point / summary, loc / scale, the tile, the plan's refusal -- then the label tensors and the workspace; the plan's own lines
// carry "plan" in the <call> column.  tests/golden/loo_refusals.txt holds these lines; tests/test_loo_cpu.py compares.  No refusal touches
// HIP and a refused call launches nothing, so this program makes NO call that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 loo_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

struct Cfg : BaseCfg {
  const float *mask = DEV, *loc = nullptr, *scale = nullptr;
  float *point = DEV, *summary = DEV, *tail = DEV;
  int tile = 0;
  bool no_plan_out = false;
};

static int call(int which, Cfg& c, const Head& a, const char** column) {
  if (which == 1) {
    int tile = 0, sweeps = 0, depth = 0;
    size_t lds = 0;
    *column = "plan";
    return slode_loo_plan(a.s, c.draws, c.tile, c.no_plan_out ? nullptr : &tile, &sweeps, &depth, &lds);
  }
  *column = "loo";
  return slode_pointwise_loo(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.draws, c.mask, c.loc, c.scale, c.tile, c.point, c.summary, c.tail, c.ws,
                             c.ws_bytes, nullptr);
}

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
  one("point NULL", [](Cfg& c) { c.point = nullptr; });
  one("summary NULL", [](Cfg& c) { c.summary = nullptr; });
  one("summary 4 bytes off", [](Cfg& c) { c.summary = DEV + 1; });
  one("loc alone", [](Cfg& c) { c.loc = DEV; });
  one("scale alone", [](Cfg& c) { c.scale = DEV; });
  one("tile -1", [](Cfg& c) { c.tile = -1; });
  plan("tile -1", [](Cfg& c) { c.tile = -1; });
  one("tile T + 1", [](Cfg& c) { c.tile = c.s.T + 1; });
  plan("tile T + 1", [](Cfg& c) { c.tile = c.s.T + 1; });
  one("tile T does not fit at num_draws 4000", [](Cfg& c) { c.draws = 4000; c.tile = c.s.T; c.ws_bytes = 64; });
  plan("tile T does not fit at num_draws 4000", [](Cfg& c) { c.draws = 4000; c.tile = c.s.T; c.ws_bytes = 64; });
  one("num_draws 2^25", [](Cfg& c) { c.draws = 1 << 25; c.ws_bytes = 64; });
  plan("num_draws 2^25", [](Cfg& c) { c.draws = 1 << 25; c.ws_bytes = 64; });
  // ---- the plan's own
  plan("plan: shape NULL", [](Cfg& c) { c.no_shape = true; });
  plan("plan: bad shape", [](Cfg& c) { c.s.T = 1; });
  plan("plan: outputs NULL", [](Cfg& c) { c.no_plan_out = true; });
  plan("plan: draws 0", [](Cfg& c) { c.draws = 0; });
  // ---- the label tensors
  one("label columns 3, n_u 2", [](Cfg& c) { c.b.label_width[1] = 2; });
  one("n_labels 5", [](Cfg& c) { c.b.n_labels = 5; });
  one("label tensor 1 NULL", [](Cfg& c) { c.b.labels[1] = nullptr; });
  // ---- the workspace
  one("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  one("mask NULL, loc and scale, tail NULL, tile 1, num_draws 1024; workspace too small",
      [](Cfg& c) { c.mask = nullptr; c.loc = DEV; c.scale = DEV; c.tail = nullptr; c.tile = 1; c.draws = 1024; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  one("params NULL + batch NULL", [](Cfg& c) { c.no_params = true; c.no_batch = true; });
  one("times NULL + draws 0", [](Cfg& c) { c.times = nullptr; c.draws = 0; });
  one("draws 0 + adaptive", [](Cfg& c) { c.draws = 0; c.s.method = SLODE_DOPRI5; });
  one("adaptive + particles 2", [](Cfg& c) { c.s.method = SLODE_BOSH3; c.s.particles = 2; });
  one("ode_alg + obs NULL", [](Cfg& c) { c.ctx.ode_alg = 2; c.b.obs = nullptr; });
  one("no_fold + point NULL", [](Cfg& c) { c.ctx.no_fold = 1; c.point = nullptr; });
  one("summary NULL + loc alone", [](Cfg& c) { c.summary = nullptr; c.loc = DEV; });
  one("scale alone + tile -1", [](Cfg& c) { c.scale = DEV; c.tile = -1; });
  one("tile -1 + label columns 3", [](Cfg& c) { c.tile = -1; c.b.label_width[1] = 2; });
  one("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  memory_untouched();
  return 0;
}
