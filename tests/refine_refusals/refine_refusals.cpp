// Every refusing configuration of slode_posterior_refine on a hand-filled handle: no slode_create, no HIP call, no device.  One line per case:
//   <case> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_traj_bounds (tests/eval_refusals), then the call's own rungs -- num_steps, lr, the shapes whose main loss
// scores the labels, the LDS tables -- then the label tensors and the workspace.  tests/golden/refine_refusals.txt holds these lines;
// tests/test_refine_cpu.py compares.  No refusal touches HIP and a refused call launches nothing, so this program makes NO call that would be
// taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 refine_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

#include <limits>

struct Cfg : BaseCfg {
  float *loc_out = DEV, *scale_out = DEV, *elbo_out = DEV;
  const float* mask = DEV;
  int steps = 4;
  float lr = 0.05f;
};

static int call(int, Cfg& c, const Head& a, const char**) {
  return slode_posterior_refine(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.draws, c.steps, c.lr, c.mask, c.loc_out, c.scale_out, c.elbo_out, DEV,
                                DEV, reinterpret_cast<int32_t*>(DEV), c.ws, c.ws_bytes, nullptr);
}

// the proc family's label heads inside the main loss (what the call refuses by name: only the flag and the count matter to that rung)
static void proc_like(Cfg& c) {
  c.s.aux_in_main = 1; c.s.n_aux = 1; c.s.U = 8; c.s.aux_mult = 46.f;
  c.s.aux[0] = slode_aux{SLODE_AUX_SIGMOID, 0, 3, 0, 1};
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  // ---- NULL pointers
  one("handle NULL", [](Cfg& c) { c.no_handle = true; });
  one("shape NULL", [](Cfg& c) { c.no_shape = true; });
  one("layout NULL", [](Cfg& c) { c.no_layout = true; });
  one("params NULL", [](Cfg& c) { c.no_params = true; });
  one("batch NULL", [](Cfg& c) { c.no_batch = true; });
  one("loc_out NULL", [](Cfg& c) { c.loc_out = nullptr; });
  one("scale_out NULL", [](Cfg& c) { c.scale_out = nullptr; });
  one("elbo_out NULL", [](Cfg& c) { c.elbo_out = nullptr; });
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
  one("steps -1", [](Cfg& c) { c.steps = -1; });
  one("lr 0", [](Cfg& c) { c.lr = 0.f; });
  one("lr -0.05", [](Cfg& c) { c.lr = -0.05f; });
  one("lr inf", [inf](Cfg& c) { c.lr = inf; });
  one("lr nan", [nan](Cfg& c) { c.lr = nan; });
  one("labels in the main loss", [](Cfg& c) { proc_like(c); });
  one("LDS: T 1000", [](Cfg& c) { c.s.T = 1000; c.b.obs_strides[0] = 3000; c.ws_bytes = 64; });
  one("LDS: num_draws 100000", [](Cfg& c) { c.draws = 100000; c.ws_bytes = 64; });
  one("LDS: num_draws 2^24", [](Cfg& c) { c.draws = 1 << 24; c.ws_bytes = 64; });
  // ---- the label tensors
  one("label columns 3, n_u 2", [](Cfg& c) { c.b.label_width[1] = 2; });
  one("n_labels 5", [](Cfg& c) { c.b.n_labels = 5; });
  one("label tensor 1 NULL", [](Cfg& c) { c.b.labels[1] = nullptr; });
  // ---- the workspace
  one("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  one("mask NULL, steps 0; workspace too small", [](Cfg& c) { c.mask = nullptr; c.steps = 0; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  one("params NULL + batch NULL", [](Cfg& c) { c.no_params = true; c.no_batch = true; });
  one("times NULL + draws 0", [](Cfg& c) { c.times = nullptr; c.draws = 0; });
  one("draws 0 + adaptive", [](Cfg& c) { c.draws = 0; c.s.method = SLODE_DOPRI5; });
  one("adaptive + particles 2", [](Cfg& c) { c.s.method = SLODE_BOSH3; c.s.particles = 2; });
  one("particles 2 + fold_on", [](Cfg& c) { c.s.particles = 2; c.ctx.fold_on = 1; });
  one("ode_alg + obs NULL", [](Cfg& c) { c.ctx.ode_alg = 2; c.b.obs = nullptr; });
  one("no_fold + steps -1", [](Cfg& c) { c.ctx.no_fold = 1; c.steps = -1; });
  one("steps -1 + lr nan", [nan](Cfg& c) { c.steps = -1; c.lr = nan; });
  one("lr 0 + labels in the main loss", [](Cfg& c) { c.lr = 0.f; proc_like(c); });
  one("labels in the main loss + LDS", [](Cfg& c) { proc_like(c); c.draws = 100000; });
  one("LDS + label columns 3", [](Cfg& c) { c.draws = 100000; c.b.label_width[1] = 2; });
  one("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // the memory that stands for every output: never written
  bool clean = true;
  for (float v : g_mem) clean = clean && v == 0.f;
  printf("memory that stands for the outputs | %s\n", clean ? "untouched" : "WRITTEN");
  return 0;
}
