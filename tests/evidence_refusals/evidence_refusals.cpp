// Every refusing configuration of slode_label_evidence on a hand-filled handle: no slode_create, no HIP call, no device.  One line per case:
//   <case> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_traj_bounds (tests/eval_refusals), then the call's own rungs -- evidence, V, hyp_labels, n_labels, the
// LDS tables -- then the label tensors and the workspace.  tests/golden/evidence_refusals.txt holds these lines;
// tests/test_label_evidence_cpu.py compares.  No refusal touches HIP and a refused call launches nothing, so this program makes NO call that
// would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 evidence_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

struct Cfg : BaseCfg {
  float *evidence = DEV, *loss = DEV;
  int V = 4;
  const float* hyp[SLODE_MAX_LABELS] = {DEV, DEV, nullptr, nullptr};
  bool no_hyp = false;
};

static int call(int, Cfg& c, const Head& a, const char**) {
  return slode_label_evidence(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.draws, c.no_hyp ? nullptr : c.hyp, c.V, nullptr, c.evidence,
                              reinterpret_cast<int32_t*>(DEV), c.loss, c.ws, c.ws_bytes, nullptr);
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
  one("evidence NULL", [](Cfg& c) { c.evidence = nullptr; });
  one("unaligned evidence", [](Cfg& c) { c.evidence = DEV + 1; });
  one("V 0", [](Cfg& c) { c.V = 0; });
  one("V -1", [](Cfg& c) { c.V = -1; });
  one("V 65", [](Cfg& c) { c.V = 65; });
  one("hyp_labels NULL", [](Cfg& c) { c.no_hyp = true; });
  one("every hyp tensor NULL", [](Cfg& c) { c.hyp[0] = c.hyp[1] = nullptr; });
  one("n_labels 0", [](Cfg& c) { c.b.n_labels = 0; });
  one("LDS: num_draws 2000, V 64", [](Cfg& c) { c.draws = 2000; c.V = 64; c.ws_bytes = 64; });
  one("LDS: num_draws 100000, V 1", [](Cfg& c) { c.draws = 100000; c.V = 1; c.ws_bytes = 64; });
  one("LDS: num_draws 2^24, V 64", [](Cfg& c) { c.draws = 1 << 24; c.V = 64; c.ws_bytes = 64; });
  // ---- the label tensors
  one("label columns 3, n_u 2", [](Cfg& c) { c.b.label_width[1] = 2; });
  one("n_labels 5", [](Cfg& c) { c.b.n_labels = 5; });
  one("label tensor 1 NULL", [](Cfg& c) { c.b.labels[1] = nullptr; });
  // ---- the workspace
  one("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  one("one hyp tensor NULL; workspace too small", [](Cfg& c) { c.hyp[1] = nullptr; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  one("params NULL + batch NULL", [](Cfg& c) { c.no_params = true; c.no_batch = true; });
  one("times NULL + draws 0", [](Cfg& c) { c.times = nullptr; c.draws = 0; });
  one("draws 0 + adaptive", [](Cfg& c) { c.draws = 0; c.s.method = SLODE_DOPRI5; });
  one("draws 2^30 + adaptive", [](Cfg& c) { c.draws = 1 << 30; c.s.method = SLODE_DOPRI5; });
  one("adaptive + particles 2", [](Cfg& c) { c.s.method = SLODE_BOSH3; c.s.particles = 2; });
  one("particles 2 + fold_on", [](Cfg& c) { c.s.particles = 2; c.ctx.fold_on = 1; });
  one("ode_alg + obs NULL", [](Cfg& c) { c.ctx.ode_alg = 2; c.b.obs = nullptr; });
  one("obs NULL + padded strides", [](Cfg& c) { c.b.obs = nullptr; c.b.obs_strides[0] += 8; });
  one("no_fold + evidence NULL", [](Cfg& c) { c.ctx.no_fold = 1; c.evidence = nullptr; });
  one("draws 0 + unaligned evidence", [](Cfg& c) { c.draws = 0; c.evidence = DEV + 1; });
  one("unaligned evidence + V 0", [](Cfg& c) { c.evidence = DEV + 1; c.V = 0; });
  one("V 65 + hyp_labels NULL", [](Cfg& c) { c.V = 65; c.no_hyp = true; });
  one("hyp_labels NULL + n_labels 0", [](Cfg& c) { c.no_hyp = true; c.b.n_labels = 0; });
  one("every hyp tensor NULL + LDS", [](Cfg& c) { c.hyp[0] = c.hyp[1] = nullptr; c.draws = 2000; c.V = 64; });
  one("LDS + label columns 3", [](Cfg& c) { c.draws = 2000; c.V = 64; c.b.label_width[1] = 2; });
  one("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // the memory that stands for every output: never written
  bool clean = true;
  for (float v : g_mem) clean = clean && v == 0.f;
  printf("memory that stands for the outputs | %s\n", clean ? "untouched" : "WRITTEN");
  return 0;
}
