// Every refusing configuration of slode_forecast_summary and slode_forecast_summary_plan on a hand-filled handle: no slode_create, no HIP
// call, no device.  One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_recon_moments on that side without its LDS rung (tests/eval_refusals), slode_forecast_moments' grid rungs
// (times_out / stage_t_out, T_out), then the call's own -- first_point, sense, a non-finite threshold, mean, window -- the plan's refusal as
// the LDS rung, then the label tensors and the workspace.  tests/golden/forecast_summary_refusals.txt holds these lines;
// tests/test_forecast_summary_cpu.py compares.  No refusal touches HIP and a refused call launches nothing, so this program makes NO call
// that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 forecast_summary_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

#include <math.h>

struct Cfg : BaseCfg {
  float levels[SLODE_MAX_C] = {0.25f, 0.5f, 0.75f, 1.0f};
  const float* thr = levels;
  const float *times_out = DEV, *stage_t_out = DEV;
  int sense = 1, T_out = 95, first_point = 85, window = 0;
  float *mean = DEV, *sd = DEV;
  int plan_window = 0;
  size_t plan_bytes = 0;
  bool no_window_out = false;
};

static int call(int which, Cfg& c, const Head& a, const char** column) {
  if (which == 1) {
    *column = "plan";
    return slode_forecast_summary_plan(a.s, c.T_out, c.window, c.no_window_out ? nullptr : &c.plan_window, c.no_params ? nullptr : &c.plan_bytes);
  }
  *column = c.is_post ? "post" : "prior";
  return slode_forecast_summary(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.times_out, c.stage_t_out, c.T_out, c.first_point,
                                c.window, c.thr, c.sense, c.mean, c.sd, c.ws, c.ws_bytes, nullptr);
}

int main() {
  ladder_pointers();
  // ---- the draw count
  pair("num_samples 0", [](Cfg& c) { c.draws = 0; });
  pair("num_samples 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  ladder_not_taken();
  ladder_post_obs();
  // ---- slode_forecast_moments' grid rungs
  pair("times_out NULL", [](Cfg& c) { c.times_out = nullptr; });
  pair("stage_t_out NULL", [](Cfg& c) { c.stage_t_out = nullptr; });
  pair("T_out 1", [](Cfg& c) { c.T_out = 1; c.first_point = 0; });
  pair("T_out 2^20 + 1", [](Cfg& c) { c.T_out = (1 << 20) + 1; });
  // ---- the call's own rungs
  pair("first_point -1", [](Cfg& c) { c.first_point = -1; });
  pair("first_point T_out", [](Cfg& c) { c.first_point = 95; });
  pair("first_point T_out - 1: taken so far; workspace too small", [](Cfg& c) { c.first_point = 94; c.ws_bytes = 64; });
  pair("sense 0", [](Cfg& c) { c.sense = 0; });
  pair("sense 2", [](Cfg& c) { c.sense = 2; });
  pair("thr[1] NaN", [](Cfg& c) { c.levels[1] = NAN; });
  pair("thr[3] NaN beyond C = 3: not read; workspace too small", [](Cfg& c) { c.levels[3] = NAN; c.ws_bytes = 64; });
  pair("mean NULL", [](Cfg& c) { c.mean = nullptr; });
  pair("window -1", [](Cfg& c) { c.window = -1; });
  // ---- the plan's refusal, as the LDS rung (a workspace too small behind it: the plan is asked first)
  pair("LDS: window 30000 of T_out 2^20", [](Cfg& c) { c.T_out = 1 << 20; c.window = 30000; c.ws_bytes = 64; });
  pair("LDS: window 2^20 clamped to T_out - 1 = 19999", [](Cfg& c) { c.T_out = 20000; c.window = 1 << 20; c.ws_bytes = 64; });
  pair("num_samples 10000, T_out 2^20, window 0: fits; workspace too small", [](Cfg& c) { c.draws = 10000; c.T_out = 1 << 20; c.ws_bytes = 64; });
  ladder_labels();
  // ---- the workspace
  pair("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  pair("sd and thr NULL, sense -1, first_point 0; workspace too small", [](Cfg& c) { c.sd = nullptr; c.thr = nullptr; c.sense = -1; c.first_point = 0; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  ladder_two_at_once(0);
  post("no_fold + times_out NULL", [](Cfg& c) { c.ctx.no_fold = 1; c.times_out = nullptr; });
  pair("times_out NULL + T_out 1", [](Cfg& c) { c.times_out = nullptr; c.T_out = 1; });
  pair("T_out 1 + first_point -1", [](Cfg& c) { c.T_out = 1; c.first_point = -1; });
  pair("first_point -1 + sense 0", [](Cfg& c) { c.first_point = -1; c.sense = 0; });
  pair("sense 0 + thr[0] NaN", [](Cfg& c) { c.sense = 0; c.levels[0] = NAN; });
  pair("thr[0] NaN + mean NULL", [](Cfg& c) { c.levels[0] = NAN; c.mean = nullptr; });
  pair("mean NULL + window -1", [](Cfg& c) { c.mean = nullptr; c.window = -1; });
  pair("window -1 + label columns 3", [](Cfg& c) { c.window = -1; c.b.label_width[1] = 2; });
  pair("unfit window + label columns 3", [](Cfg& c) { c.T_out = 20000; c.window = 19999; c.b.label_width[1] = 2; });
  pair("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // ---- the plan: host arithmetic alone
  plan("shape NULL", [](Cfg& c) { c.no_shape = true; });
  plan("bad shape", [](Cfg& c) { c.s.T = 1; });
  plan("window_out NULL", [](Cfg& c) { c.no_window_out = true; });
  plan("lds_bytes NULL", [](Cfg& c) { c.no_params = true; });
  plan("T_out 1", [](Cfg& c) { c.T_out = 1; });
  plan("T_out 2^20 + 1", [](Cfg& c) { c.T_out = (1 << 20) + 1; });
  plan("window -1", [](Cfg& c) { c.window = -1; });
  plan("LDS: window 30000 of T_out 2^20", [](Cfg& c) { c.T_out = 1 << 20; c.window = 30000; });
  memory_untouched();
  return 0;
}
