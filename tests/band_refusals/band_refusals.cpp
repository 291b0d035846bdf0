// Every refusing configuration of slode_joint_band, slode_joint_band_plan and slode_joint_band_levels on a hand-filled handle: no
// slode_create, no HIP call, no device.  One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the pointers, the draw count (num_samples < 2: the call's own), the ladder of slode_recon_moments on that side without its LDS
// rung (tests/eval_refusals), then the call's own rungs -- the outputs, the levels, the floor, the prior's optional observations, the LDS
// tables -- then the label tensors and the workspace.  tests/golden/band_refusals.txt holds these lines; tests/test_band_cpu.py compares.
// No refusal touches HIP and a refused call launches nothing, so this program makes NO call that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 band_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

#include <math.h>

struct Cfg : BaseCfg {
  int n_levels = 2;
  double levels[9] = {0.95, 0.5, 0.9, 1.0, 0.25, 0.75, 0.99, 0.8, 0.7};
  bool no_levels = false;
  float sd_floor = 0.f;
  float *mean = DEV, *sd = DEV, *crit = DEV, *joint = DEV, *obs_dev = DEV, *dev_out = DEV;
  size_t plan_bytes = 0;
  bool plan_out = true;
  int ranks[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool levels_out = true;
};

static int call(int which, Cfg& c, const Head& a, const char** column) {
  if (which == 1) {
    *column = "plan";
    const int rc = slode_joint_band_plan(a.s, c.draws, c.plan_out ? &c.plan_bytes : nullptr);
    c.ctx.rng_counter = c.plan_bytes;   // (the plan has no generator: the column shows the bytes it wrote, refused or not)
    return rc;
  }
  if (which == 2) {
    *column = "levels";
    const int rc = slode_joint_band_levels(c.draws, c.n_levels, c.no_levels ? nullptr : c.levels, c.levels_out ? c.ranks : nullptr, c.z);
    c.ctx.rng_counter = (unsigned long long)c.ranks[0];   // (no generator either: the first rank it wrote, 0 when refused)
    return rc;
  }
  *column = c.is_post ? "post" : "prior";
  return slode_joint_band(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.n_levels, c.no_levels ? nullptr : c.levels,
                          c.sd_floor, c.mean, c.sd, c.crit, c.joint, c.obs_dev, c.dev_out, c.ws, c.ws_bytes, nullptr);
}

// (the level rule takes no handle, as the plan)
static void levels(const char* name, const Edit& edit) { Cfg c; c.no_handle = true; edit(c); run(name, c, 2); }

// T = 1024, S = 5, C = 3: the step table is 40 KB and the moment / value table 108 KB; the deviations take 36 B per draw
static void big(Cfg& c) { c.s.T = 1024; c.b.obs_strides[0] = 3072; }

int main() {
  ladder_pointers();
  // ---- the draw count
  pair("num_samples 0", [](Cfg& c) { c.draws = 0; });
  pair("num_samples 1", [](Cfg& c) { c.draws = 1; });
  pair("num_samples 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  ladder_not_taken();
  ladder_post_obs();   // (the posterior needs the observations ...)
  // ---- the call's own rungs
  pair("mean NULL", [](Cfg& c) { c.mean = nullptr; });
  pair("sd NULL", [](Cfg& c) { c.sd = nullptr; });
  pair("crit NULL", [](Cfg& c) { c.crit = nullptr; });
  pair("n_levels 0", [](Cfg& c) { c.n_levels = 0; });
  pair("n_levels 9", [](Cfg& c) { c.n_levels = 9; });
  pair("levels NULL", [](Cfg& c) { c.no_levels = true; });
  pair("level 0", [](Cfg& c) { c.levels[1] = 0.0; });
  pair("level 1.5", [](Cfg& c) { c.levels[0] = 1.5; });
  pair("level NaN", [](Cfg& c) { c.levels[1] = NAN; });
  pair("sd_floor -1", [](Cfg& c) { c.sd_floor = -1.f; });
  pair("sd_floor NaN", [](Cfg& c) { c.sd_floor = NAN; });
  pair("sd_floor inf", [](Cfg& c) { c.sd_floor = INFINITY; });
  // ... and the prior takes them for the observed deviation, dense
  prior("padded strides", [](Cfg& c) { c.b.obs_strides[0] += 8; });
  prior("channel-major strides of another T", [](Cfg& c) { c.b.obs_strides[1] = c.s.T + 1; c.b.obs_strides[2] = 1; });
  pair("LDS: T 1024, 400 draws", [](Cfg& c) { big(c); c.draws = 400; c.ws_bytes = 64; });
  pair("LDS: T 86, 4100 draws", [](Cfg& c) { c.draws = 4100; c.ws_bytes = 64; });
  pair("LDS: 2^29 draws", [](Cfg& c) { c.s.B = 1; c.b.obs_strides[0] = 258; c.draws = 1 << 29; c.ws_bytes = 64; });
  pair("T 1024, 8 draws, run-time S build: fits; workspace too small", [](Cfg& c) { big(c); c.draws = 8; c.ctx.ode_generic = 1; c.ws_bytes = 64; });
  pair("T 1024, 8 draws: fits; workspace too small", [](Cfg& c) { big(c); c.draws = 8; c.ws_bytes = 64; });
  ladder_labels();
  // ---- the workspace
  pair("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  pair("joint, obs_dev, dev_out NULL; workspace too small", [](Cfg& c) { c.joint = c.obs_dev = c.dev_out = nullptr; c.ws_bytes = 64; });
  prior("obs NULL; workspace too small", [](Cfg& c) { c.b.obs = nullptr; c.ws_bytes = 64; });
  pair("level 1, eight levels; workspace too small", [](Cfg& c) { c.n_levels = 8; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  ladder_two_at_once(1);
  post("no_fold + mean NULL", [](Cfg& c) { c.ctx.no_fold = 1; c.mean = nullptr; });
  pair("crit NULL + n_levels 0", [](Cfg& c) { c.crit = nullptr; c.n_levels = 0; });
  pair("level 0 + sd_floor -1", [](Cfg& c) { c.levels[0] = 0.0; c.sd_floor = -1.f; });
  pair("sd_floor -1 + LDS", [](Cfg& c) { c.sd_floor = -1.f; c.draws = 4100; });
  pair("LDS + label columns 3", [](Cfg& c) { c.draws = 4100; c.b.label_width[1] = 2; });
  pair("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // ---- the plan: host arithmetic alone (the counter column: the bytes written)
  plan("shape NULL", [](Cfg& c) { c.no_shape = true; });
  plan("bad shape", [](Cfg& c) { c.s.T = 1; });
  plan("lds_bytes NULL", [](Cfg& c) { c.plan_out = false; });
  plan("num_samples 1", [](Cfg& c) { c.draws = 1; });
  plan("LDS: T 1024, 400 draws", [](Cfg& c) { big(c); c.draws = 400; });
  plan("LDS: T 86, 4100 draws", [](Cfg& c) { c.draws = 4100; });
  // ---- the level rule (the counter column: the first rank written)
  levels("ranks NULL", [](Cfg& c) { c.levels_out = false; });
  levels("num_samples 1", [](Cfg& c) { c.draws = 1; });
  levels("n_levels 9", [](Cfg& c) { c.n_levels = 9; });
  levels("levels NULL", [](Cfg& c) { c.no_levels = true; });
  levels("level 0", [](Cfg& c) { c.levels[1] = 0.0; });
  levels("level -0.5", [](Cfg& c) { c.levels[0] = -0.5; });
  memory_untouched();
  return 0;
}
