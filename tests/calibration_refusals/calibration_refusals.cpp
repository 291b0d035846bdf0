// Every refusing configuration of slode_calibration, on a hand-filled handle: no slode_create, no HIP call, no device.  One line per case:
//   <case> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order; the last line says whether the memory that stands for every buffer (the outputs among them) is still as it was.
// tests/test_calibration_cpu.py holds the expected status and the words each message must carry.  No refusal touches HIP and a refused
// call launches nothing, so this program makes NO call that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 calibration_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

struct Cfg : BaseCfg {
  const int32_t *members = (const int32_t*)DEV, *offsets = (const int32_t*)DEV;
  int32_t *below = (int32_t*)DEV, *inside = (int32_t*)DEV, *cross = (int32_t*)DEV;
  float *pinball = DEV, *width = DEV;
  void* scratch = DEV;
  size_t scratch_bytes = BIG;   // (the scratch too is "large enough" unless a case says otherwise)
  int M = 3, G = 2, chunk = 0;
};

static int call(int, Cfg& c, const Head& a, const char**) {
  return slode_calibration(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.members, c.offsets, c.M, c.G, c.chunk, c.below,
                           c.inside, c.cross, c.pinball, c.width, c.scratch, c.scratch_bytes, c.ws, c.ws_bytes, nullptr);
}

int main() {
  // ---- what slode_cohort_moments refuses for the same is_post, in its order; observations are required on both sides
  both("handle NULL", [](Cfg& c) { c.no_handle = true; });
  both("shape NULL", [](Cfg& c) { c.no_shape = true; });
  both("layout NULL", [](Cfg& c) { c.no_layout = true; });
  both("params NULL", [](Cfg& c) { c.no_params = true; });
  both("batch NULL", [](Cfg& c) { c.no_batch = true; });
  both("times NULL", [](Cfg& c) { c.times = nullptr; });
  both("stage_t NULL", [](Cfg& c) { c.stage_t = nullptr; });
  both("workspace NULL", [](Cfg& c) { c.ws = nullptr; });
  both("bad shape", [](Cfg& c) { c.s.T = 1; });
  both("draws 0", [](Cfg& c) { c.draws = 0; });
  both("draws 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  for (int m : {SLODE_DOPRI5, SLODE_BOSH3, SLODE_FEHLBERG2, SLODE_ADAPTIVE_HEUN}) {
    char name[64];
    snprintf(name, sizeof(name), "adaptive method %d", m);
    both(name, [m](Cfg& c) { c.s.method = m; });
  }
  both("particles 2", [](Cfg& c) { c.s.particles = 2; });
  both("fold_on", [](Cfg& c) { c.ctx.fold_on = 1; });
  both("ode_pack", [](Cfg& c) { c.ctx.ode_pack = 4; });
  both("ode_alg", [](Cfg& c) { c.ctx.ode_alg = 1; });
  both("obs NULL", [](Cfg& c) { c.b.obs = nullptr; });
  one("post: padded strides", [](Cfg& c) { c.b.obs_strides[0] += 8; });
  one("post: no_fold", [](Cfg& c) { c.ctx.no_fold = 1; });
  // ---- the call's own rungs
  both("members NULL", [](Cfg& c) { c.members = nullptr; });
  both("offsets NULL", [](Cfg& c) { c.offsets = nullptr; });
  both("M -1", [](Cfg& c) { c.M = -1; });
  both("M B + 1", [](Cfg& c) { c.M = 5; });
  both("G 0", [](Cfg& c) { c.G = 0; });
  both("G 1025", [](Cfg& c) { c.G = 1025; });
  both("chunk -1", [](Cfg& c) { c.chunk = -1; });
  both("chunk 65", [](Cfg& c) { c.chunk = 65; });
  both("below NULL", [](Cfg& c) { c.below = nullptr; });
  one("prior: padded strides", [](Cfg& c) { c.is_post = 0; c.b.obs_strides[0] += 8; });
  one("prior: strides of another T", [](Cfg& c) { c.is_post = 0; c.b.obs_strides[1] = c.s.T + 1; c.b.obs_strides[2] = 1; });
  both("scratch NULL", [](Cfg& c) { c.scratch = nullptr; });
  both("scratch misaligned", [](Cfg& c) { c.scratch = (char*)DEV + 4; });
  both("T 1024: the LDS tables", [](Cfg& c) { c.s.T = 1024; c.b.obs_strides[0] = 3 * 1024; c.scratch_bytes = 64; });
  both("scratch too small", [](Cfg& c) { c.scratch_bytes = 64; });
  // ---- the label tensors, the workspace
  both("label columns 3, n_u 2", [](Cfg& c) { c.b.label_width[1] = 2; });
  one("prior without labels", [](Cfg& c) { c.is_post = 0; c.b.n_labels = 0; });
  both("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier check of the ladder names the reason
  both("adaptive + G 0", [](Cfg& c) { c.s.method = SLODE_DOPRI5; c.G = 0; });
  both("draws 0 + below NULL", [](Cfg& c) { c.draws = 0; c.below = nullptr; });
  both("measured arm + obs NULL", [](Cfg& c) { c.ctx.ode_alg = 1; c.b.obs = nullptr; });
  both("obs NULL + members NULL", [](Cfg& c) { c.b.obs = nullptr; c.members = nullptr; });
  both("members NULL + M -1", [](Cfg& c) { c.members = nullptr; c.M = -1; });
  both("M 5 + G 0", [](Cfg& c) { c.M = 5; c.G = 0; });
  both("G 0 + chunk 65", [](Cfg& c) { c.G = 0; c.chunk = 65; });
  both("chunk 65 + below NULL", [](Cfg& c) { c.chunk = 65; c.below = nullptr; });
  one("prior: below NULL + padded strides", [](Cfg& c) { c.is_post = 0; c.below = nullptr; c.b.obs_strides[0] += 8; });
  both("scratch too small + workspace too small", [](Cfg& c) { c.scratch_bytes = 64; c.ws_bytes = 64; });
  // ---- M = 0 with NULL lists is no refusal of the argument rungs: the scratch rung behind them speaks; the optional outputs may be NULL
  both("M 0 with NULL lists and optional outputs, scratch too small", [](Cfg& c) {
    c.M = 0; c.members = nullptr; c.offsets = nullptr; c.inside = c.cross = nullptr; c.pinball = c.width = nullptr; c.scratch_bytes = 0;
  });
  bool clean = true;
  for (float v : g_mem) clean = clean && v == 0.f;
  printf("memory that stands for the outputs | %s\n", clean ? "untouched" : "WRITTEN");
  return 0;
}
