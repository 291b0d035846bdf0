// Every refusing configuration of slode_curve_summary and slode_curve_summary_plan on a hand-filled handle: no slode_create, no HIP call, no
// device.  One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_recon_moments on that side without its LDS rung (tests/eval_refusals), then the call's own rungs -- mean,
// sense, a non-finite threshold, p_beyond without a threshold, the LDS tables with and without p_beyond -- then the label tensors and the
// workspace.  tests/golden/summary_refusals.txt holds these lines; tests/test_summary_cpu.py compares.  No refusal touches HIP and a refused
// call launches nothing, so this program makes NO call that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 summary_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

#include <math.h>

struct Cfg : BaseCfg {
  float levels[SLODE_MAX_C] = {0.25f, 0.5f, 0.75f, 1.0f};
  const float* thr = levels;
  int sense = 1, want_p = 1;
  float *mean = DEV, *sd = DEV, *p_beyond = DEV;
  size_t plan_bytes = 0;
};

static int call(int which, Cfg& c, const Head& a, const char** column) {
  if (which == 1) {
    *column = "plan";
    return slode_curve_summary_plan(a.s, c.want_p, c.no_params ? nullptr : &c.plan_bytes);
  }
  *column = c.is_post ? "post" : "prior";
  return slode_curve_summary(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.thr, c.sense, c.mean, c.sd, c.p_beyond, c.ws,
                             c.ws_bytes, nullptr);
}


// T = 1024, S = 8, C = 4, ALD: the step table alone is 64 KB and the two Q C T tables are 48 KB each -- the shape fits only without p_beyond
// (no shape check_shape takes exceeds the budget without the counters: the figure "without p_beyond" can be seen in the plan alone)
static void big(Cfg& c) { c.s.T = 1024; c.s.S = 8; c.s.C = 4; c.b.obs_strides[0] = 4096; c.b.obs_strides[2] = 4; }

int main() {
  ladder_pointers();
  // ---- the draw count
  pair("num_samples 0", [](Cfg& c) { c.draws = 0; });
  pair("num_samples 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  ladder_not_taken();
  ladder_post_obs();
  // ---- the call's own rungs
  pair("mean NULL", [](Cfg& c) { c.mean = nullptr; });
  pair("sense 0", [](Cfg& c) { c.sense = 0; });
  pair("sense 2", [](Cfg& c) { c.sense = 2; });
  pair("thr[1] NaN", [](Cfg& c) { c.levels[1] = NAN; });
  pair("thr[2] inf", [](Cfg& c) { c.levels[2] = INFINITY; });
  pair("thr[3] NaN beyond C = 3: not read; workspace too small", [](Cfg& c) { c.levels[3] = NAN; c.ws_bytes = 64; });
  pair("p_beyond without thr", [](Cfg& c) { c.thr = nullptr; });
  pair("LDS: T 1024, S 8, C 4, with p_beyond", [](Cfg& c) { big(c); c.ws_bytes = 64; });
  pair("T 1024, S 8, C 4, without p_beyond: fits; workspace too small", [](Cfg& c) { big(c); c.p_beyond = nullptr; c.ws_bytes = 64; });
  ladder_labels();
  // ---- the workspace
  pair("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  pair("sd, p_beyond and thr NULL, sense -1; workspace too small", [](Cfg& c) { c.sd = nullptr; c.p_beyond = nullptr; c.thr = nullptr; c.sense = -1; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  ladder_two_at_once(0);
  post("no_fold + mean NULL", [](Cfg& c) { c.ctx.no_fold = 1; c.mean = nullptr; });
  pair("mean NULL + sense 0", [](Cfg& c) { c.mean = nullptr; c.sense = 0; });
  pair("sense 0 + thr[0] NaN", [](Cfg& c) { c.sense = 0; c.levels[0] = NAN; });
  pair("thr[0] NaN + LDS", [](Cfg& c) { c.levels[0] = NAN; big(c); });
  pair("p_beyond without thr + LDS", [](Cfg& c) { c.thr = nullptr; big(c); });
  pair("LDS + label columns 3", [](Cfg& c) { big(c); c.b.label_width[1] = 2; });
  pair("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // ---- the plan: host arithmetic alone
  plan("shape NULL", [](Cfg& c) { c.no_shape = true; });
  plan("bad shape", [](Cfg& c) { c.s.T = 1; });
  plan("lds_bytes NULL", [](Cfg& c) { c.no_params = true; });
  plan("LDS: T 1024, S 8, C 4, with p_beyond", [](Cfg& c) { big(c); });
  memory_untouched();
  return 0;
}
