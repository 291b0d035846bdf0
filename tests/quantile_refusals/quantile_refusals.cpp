// Every refusing configuration of slode_recon_quantiles and slode_quantile_plan on a hand-filled handle: no slode_create, no HIP call, no
// device.  One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_recon_moments on that side without its LDS rung (tests/eval_refusals), then the call's own rungs -- out,
// the level count, the levels, the tile, the LDS tables of a given tile and of the smallest tile -- then the label tensors and the workspace.
// tests/golden/quantile_refusals.txt holds these lines; tests/test_quantiles_cpu.py compares.  No refusal touches HIP and a refused call
// launches nothing, so this program makes NO call that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 quantile_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

#include <math.h>

struct Cfg : BaseCfg {
  double lv[SLODE_QUANTILE_MAX_LEVELS + 1] = {0.025, 0.975, 0.5, 0.0, 1.0, 0.25, 0.75, 0.1, 0.9};
  const double* levels = lv;
  int n_levels = 2, tile = 0;
  float* out = DEV;
  int tile_out = -1, sweeps = -1, depth_lo = -1, depth_hi = -1;
  size_t plan_bytes = 0;
  bool no_plan_out = false;
};

static int call(int which, Cfg& c, const Head& a, const char** column) {
  if (which == 1) {
    *column = "plan";
    return slode_quantile_plan(a.s, c.draws, c.n_levels, c.levels, c.tile, &c.tile_out, c.no_plan_out ? nullptr : &c.sweeps, &c.depth_lo, &c.depth_hi,
                               &c.plan_bytes);
  }
  *column = c.is_post ? "post" : "prior";
  return slode_recon_quantiles(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.n_levels, c.levels, c.tile, c.out, c.ws,
                               c.ws_bytes, nullptr);
}


// T = 1024, S = 8, C = 4, ALD, a median of 1024 draws: the step table alone is 64 KB and ONE time point of the sorted buffers is 1024 x 12 x 4 B =
// 48 KB -- three points would fit, 1024 sweeps' worth; with num_samples = 4096 not even one
static void big(Cfg& c) { c.s.T = 1024; c.s.S = 8; c.s.C = 4; c.b.obs_strides[0] = 4096; c.b.obs_strides[2] = 4; c.n_levels = 1; c.lv[0] = 0.5; }

int main() {
  ladder_pointers();
  // ---- the draw count
  pair("num_samples 0", [](Cfg& c) { c.draws = 0; });
  pair("num_samples 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  ladder_not_taken();
  ladder_post_obs();
  // ---- the call's own rungs
  pair("out NULL", [](Cfg& c) { c.out = nullptr; });
  pair("n_levels 0", [](Cfg& c) { c.n_levels = 0; });
  pair("n_levels 9", [](Cfg& c) { c.n_levels = 9; });
  pair("levels NULL", [](Cfg& c) { c.levels = nullptr; });
  pair("levels[1] 1.5", [](Cfg& c) { c.lv[1] = 1.5; });
  pair("levels[0] -0.001", [](Cfg& c) { c.lv[0] = -0.001; });
  pair("levels[1] NaN", [](Cfg& c) { c.lv[1] = NAN; });
  pair("levels[2] NaN beyond n_levels = 2: not read; workspace too small", [](Cfg& c) { c.lv[2] = NAN; c.ws_bytes = 64; });
  pair("tile -1", [](Cfg& c) { c.tile = -1; });
  pair("tile T + 1", [](Cfg& c) { c.tile = c.s.T + 1; });
  pair("LDS: T 1024, S 8, C 4, median of 1024, tile 4", [](Cfg& c) { big(c); c.draws = 1024; c.tile = 4; c.ws_bytes = 64; });
  pair("LDS: T 1024, S 8, C 4, median of 4096, tile 0", [](Cfg& c) { big(c); c.draws = 4096; c.ws_bytes = 64; });
  pair("T 1024, S 8, C 4, median of 1024, tile 0: fits; workspace too small", [](Cfg& c) { big(c); c.draws = 1024; c.ws_bytes = 64; });
  pair("unordered and duplicate levels: taken; workspace too small", [](Cfg& c) { c.n_levels = 4; c.lv[0] = 0.9; c.lv[1] = 0.1; c.lv[2] = 0.9; c.lv[3] = 0.0; c.ws_bytes = 64; });
  ladder_labels();
  // ---- the workspace
  pair("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  ladder_two_at_once(0);
  post("no_fold + out NULL", [](Cfg& c) { c.ctx.no_fold = 1; c.out = nullptr; });
  pair("out NULL + n_levels 0", [](Cfg& c) { c.out = nullptr; c.n_levels = 0; });
  pair("n_levels 9 + levels[0] NaN", [](Cfg& c) { c.n_levels = 9; c.lv[0] = NAN; });
  pair("levels[0] NaN + tile -1", [](Cfg& c) { c.lv[0] = NAN; c.tile = -1; });
  pair("tile -1 + LDS", [](Cfg& c) { big(c); c.draws = 4096; c.tile = -1; });
  pair("LDS + label columns 3", [](Cfg& c) { big(c); c.draws = 4096; c.b.label_width[1] = 2; });
  pair("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // ---- the plan: host arithmetic alone
  plan("shape NULL", [](Cfg& c) { c.no_shape = true; });
  plan("bad shape", [](Cfg& c) { c.s.T = 1; });
  plan("sweeps NULL", [](Cfg& c) { c.no_plan_out = true; });
  plan("num_samples 0", [](Cfg& c) { c.draws = 0; });
  plan("n_levels 9", [](Cfg& c) { c.n_levels = 9; });
  plan("levels NULL", [](Cfg& c) { c.levels = nullptr; });
  plan("levels[1] NaN", [](Cfg& c) { c.lv[1] = NAN; });
  plan("tile T + 1", [](Cfg& c) { c.tile = c.s.T + 1; });
  plan("LDS: T 1024, S 8, C 4, median of 1024, tile 4", [](Cfg& c) { big(c); c.draws = 1024; c.tile = 4; });
  plan("LDS: T 1024, S 8, C 4, median of 4096, tile 0", [](Cfg& c) { big(c); c.draws = 4096; });
  memory_untouched();
  return 0;
}
