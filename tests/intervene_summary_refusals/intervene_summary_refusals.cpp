// Every refusing configuration of slode_intervene_summary and slode_intervene_summary_plan on a hand-filled handle: no slode_create, no HIP
// call, no device.  One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_recon_moments for the posterior without its LDS rung (tests/eval_refusals; the call has no prior side,
// so every case is one line), then the call's own rungs -- cf_mean, V, sense, a non-finite threshold, the group mask, the hypothesis tables,
// the LDS tables -- then the label tensors and the workspace.  tests/golden/intervene_summary_refusals.txt holds these lines;
// tests/test_intervene_summary_cpu.py compares.  No refusal touches HIP and a refused call launches nothing, so this program makes NO call
// that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 intervene_summary_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

#include <math.h>

struct Cfg : BaseCfg {
  float levels[SLODE_MAX_C] = {0.25f, 0.5f, 0.75f, 1.0f};
  const float* thr = levels;
  const float* tables[SLODE_MAX_LABELS] = {DEV, DEV, nullptr, nullptr};
  bool no_tables = false;
  int sense = 1, V = 3;
  unsigned int mask = 3;
  float *f_mean = DEV, *f_sd = DEV, *cf_mean = DEV, *cf_sd = DEV, *eff_mean = DEV, *eff_sd = DEV;
  size_t plan_bytes = 0;
};

static int call(int which, Cfg& c, const Head& a, const char** column) {
  if (which == 1) {
    *column = "plan";
    return slode_intervene_summary_plan(a.s, c.V, c.no_params ? nullptr : &c.plan_bytes);
  }
  *column = "post";
  return slode_intervene_summary(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.no_tables ? nullptr : c.tables, c.V, c.mask, c.draws, c.thr, c.sense,
                                 c.f_mean, c.f_sd, c.cf_mean, c.cf_sd, c.eff_mean, c.eff_sd, c.ws, c.ws_bytes, nullptr);
}

// T = 1024, S = 8, C = 4, ALD: the step table is 64 KB, the value table 48 KB and every arm adds two sets of triples (2.8 KB): V = 16 does not fit, V = 1 does
static void big(Cfg& c) { c.V = 16; c.s.T = 1024; c.s.S = 8; c.s.C = 4; c.b.obs_strides[0] = 4096; c.b.obs_strides[2] = 4; }

int main() {
  // ---- slode_recon_moments' ladder for the posterior (the sections of refusals_common.h, one line each)
  post("handle NULL", [](Cfg& c) { c.no_handle = true; });
  post("shape NULL", [](Cfg& c) { c.no_shape = true; });
  post("layout NULL", [](Cfg& c) { c.no_layout = true; });
  post("params NULL", [](Cfg& c) { c.no_params = true; });
  post("batch NULL", [](Cfg& c) { c.no_batch = true; });
  post("times NULL", [](Cfg& c) { c.times = nullptr; });
  post("stage_t NULL", [](Cfg& c) { c.stage_t = nullptr; });
  post("workspace NULL", [](Cfg& c) { c.ws = nullptr; });
  post("bad shape", [](Cfg& c) { c.s.T = 1; });
  post("num_samples 0", [](Cfg& c) { c.draws = 0; });
  post("num_samples 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  for (int m : {SLODE_DOPRI5, SLODE_BOSH3, SLODE_FEHLBERG2, SLODE_ADAPTIVE_HEUN}) {
    char name[64];
    snprintf(name, sizeof(name), "adaptive method %d", m);
    post(name, [m](Cfg& c) { c.s.method = m; });
  }
  post("particles 2", [](Cfg& c) { c.s.particles = 2; });
  post("fold_on", [](Cfg& c) { c.ctx.fold_on = 1; });
  post("ode_pack", [](Cfg& c) { c.ctx.ode_pack = 4; });
  post("ode_alg", [](Cfg& c) { c.ctx.ode_alg = 1; });
  ladder_post_obs();
  // ---- the call's own rungs
  post("cf_mean NULL", [](Cfg& c) { c.cf_mean = nullptr; });
  post("V 0", [](Cfg& c) { c.V = 0; });
  post("V 65", [](Cfg& c) { c.V = 65; });
  post("sense 0", [](Cfg& c) { c.sense = 0; });
  post("thr[1] NaN", [](Cfg& c) { c.levels[1] = NAN; });
  post("thr[3] NaN beyond C = 3: not read; workspace too small", [](Cfg& c) { c.levels[3] = NAN; c.ws_bytes = 64; });
  post("group_mask bit 2 of 2 groups", [](Cfg& c) { c.mask = 4; });
  post("mask 3, hyp_labels NULL", [](Cfg& c) { c.no_tables = true; });
  post("mask 3, every table NULL", [](Cfg& c) { c.tables[0] = c.tables[1] = nullptr; });
  post("mask 3, no label tensors", [](Cfg& c) { c.b.n_labels = 0; });
  post("mask 1, only the table of group 1", [](Cfg& c) { c.mask = 1; c.tables[0] = nullptr; });
  post("mask 0, hyp_labels NULL: taken so far; workspace too small", [](Cfg& c) { c.mask = 0; c.no_tables = true; c.ws_bytes = 64; });
  post("LDS: T 1024, S 8, C 4, V 16", [](Cfg& c) { big(c); c.ws_bytes = 64; });
  post("T 1024, S 8, C 4, V 1: fits; workspace too small", [](Cfg& c) { big(c); c.V = 1; c.ws_bytes = 64; });
  // ---- the label tensors, the workspace
  post("label columns 3, n_u 2", [](Cfg& c) { c.b.label_width[1] = 2; });
  post("n_labels 5", [](Cfg& c) { c.b.n_labels = 5; c.mask = 0; });
  post("label tensor 1 NULL", [](Cfg& c) { c.b.labels[1] = nullptr; });
  post("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  post("every optional output and thr NULL, sense -1; workspace too small", [](Cfg& c) {
    c.f_mean = c.f_sd = c.cf_sd = c.eff_mean = c.eff_sd = nullptr; c.thr = nullptr; c.sense = -1; c.ws_bytes = 64;
  });
  // ---- two conditions at once: the earlier rung speaks
  post("params NULL + batch NULL", [](Cfg& c) { c.no_params = true; c.no_batch = true; });
  post("times NULL + num_samples 0", [](Cfg& c) { c.times = nullptr; c.draws = 0; });
  post("num_samples 0 + adaptive", [](Cfg& c) { c.draws = 0; c.s.method = SLODE_DOPRI5; });
  post("adaptive + particles 2", [](Cfg& c) { c.s.method = SLODE_BOSH3; c.s.particles = 2; });
  post("ode_alg + obs NULL", [](Cfg& c) { c.ctx.ode_alg = 2; c.b.obs = nullptr; });
  post("no_fold + cf_mean NULL", [](Cfg& c) { c.ctx.no_fold = 1; c.cf_mean = nullptr; });
  post("cf_mean NULL + V 0", [](Cfg& c) { c.cf_mean = nullptr; c.V = 0; });
  post("V 0 + sense 0", [](Cfg& c) { c.V = 0; c.sense = 0; });
  post("sense 0 + thr[0] NaN", [](Cfg& c) { c.sense = 0; c.levels[0] = NAN; });
  post("thr[0] NaN + mask bit 2", [](Cfg& c) { c.levels[0] = NAN; c.mask = 4; });
  post("mask bit 2 + hyp_labels NULL", [](Cfg& c) { c.mask = 7; c.no_tables = true; });
  post("every table NULL + LDS", [](Cfg& c) { c.tables[0] = c.tables[1] = nullptr; big(c); });
  post("LDS + label columns 3", [](Cfg& c) { big(c); c.b.label_width[1] = 2; });
  post("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // ---- the plan: host arithmetic alone
  plan("shape NULL", [](Cfg& c) { c.no_shape = true; });
  plan("bad shape", [](Cfg& c) { c.s.T = 1; });
  plan("lds_bytes NULL", [](Cfg& c) { c.no_params = true; });
  plan("V 0", [](Cfg& c) { c.V = 0; });
  plan("V 65", [](Cfg& c) { c.V = 65; });
  plan("LDS: T 1024, S 8, C 4, V 16", [](Cfg& c) { big(c); });
  memory_untouched();
  return 0;
}
