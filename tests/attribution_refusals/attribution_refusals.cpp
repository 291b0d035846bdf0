// Every refusing configuration of slode_latent_attribution and slode_attribution_plan on a hand-filled handle: no slode_create, no HIP call, no
// device.  One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_recon_moments on that side without its LDS rung (tests/eval_refusals), then the call's own rungs -- n_arms,
// arm_masks / msd, the masks' bits, the rest bit of a shape without rest dims, the LDS tables -- then the label tensors and the workspace.
// tests/golden/attribution_refusals.txt holds these lines; tests/test_attribution_cpu.py compares.  No refusal touches HIP and a refused call
// launches nothing, so this program makes NO call that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 attribution_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

struct Cfg : BaseCfg {
  unsigned int masks[SLODE_ATTRIBUTION_MAX_ARMS + 1] = {1u, 6u, 2u, 5u, 4u, 3u};   // cvs: each single block, each complement
  const unsigned int* arm_masks = masks;
  int n_arms = 6;
  float *mean = DEV, *sd = DEV, *msd = DEV;
  size_t plan_bytes = 0;
};

static int call(int which, Cfg& c, const Head& a, const char** column) {
  if (which == 1) {
    *column = "plan";
    return slode_attribution_plan(a.s, c.n_arms, c.no_params ? nullptr : &c.plan_bytes);
  }
  *column = c.is_post ? "post" : "prior";
  return slode_latent_attribution(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.arm_masks, c.n_arms, c.mean, c.sd, c.msd, c.ws,
                                  c.ws_bytes, nullptr);
}


int main() {
  ladder_pointers();
  // ---- the draw count
  pair("num_samples 0", [](Cfg& c) { c.draws = 0; });
  pair("num_samples 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  ladder_not_taken();
  ladder_post_obs();
  // ---- the call's own rungs
  pair("n_arms 0", [](Cfg& c) { c.n_arms = 0; });
  pair("n_arms -3", [](Cfg& c) { c.n_arms = -3; });
  pair("n_arms 17", [](Cfg& c) { c.n_arms = 17; });
  pair("arm_masks NULL", [](Cfg& c) { c.arm_masks = nullptr; });
  pair("msd NULL", [](Cfg& c) { c.msd = nullptr; });
  pair("mask bit 3, n_groups 2", [](Cfg& c) { c.masks[2] = 8u; });
  pair("mask bit 31", [](Cfg& c) { c.masks[5] = 0x80000001u; });
  pair("rest bit, groups cover all of L", [](Cfg& c) { c.s.L = 6; });
  pair("no groups: the rest block is bit 0, bits beyond it", [](Cfg& c) { c.s.n_groups = 0; c.s.n_u = 0; c.b.n_labels = 0; });
  pair("LDS: T 1024", [](Cfg& c) { c.s.T = 1024; c.b.obs_strides[0] = 3072; c.ws_bytes = 64; });
  pair("LDS: T 500, n_arms 16", [](Cfg& c) { c.s.T = 500; c.b.obs_strides[0] = 1500; c.n_arms = 16; for (int i = 6; i < 16; ++i) c.masks[i] = 7u; c.ws_bytes = 64; });
  ladder_labels();
  // ---- the workspace
  pair("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  pair("mean and sd NULL, mask 0 among the arms; workspace too small", [](Cfg& c) { c.mean = nullptr; c.sd = nullptr; c.masks[0] = 0u; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  ladder_two_at_once(0);
  post("no_fold + n_arms 0", [](Cfg& c) { c.ctx.no_fold = 1; c.n_arms = 0; });
  pair("n_arms 17 + arm_masks NULL", [](Cfg& c) { c.n_arms = 17; c.arm_masks = nullptr; });
  pair("msd NULL + mask bit 3", [](Cfg& c) { c.msd = nullptr; c.masks[0] = 8u; });
  pair("mask bit 3 + LDS", [](Cfg& c) { c.masks[1] = 9u; c.s.T = 1024; c.b.obs_strides[0] = 3072; });
  pair("LDS + label columns 3", [](Cfg& c) { c.s.T = 1024; c.b.obs_strides[0] = 3072; c.b.label_width[1] = 2; });
  pair("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // ---- the plan: host arithmetic alone
  plan("shape NULL", [](Cfg& c) { c.no_shape = true; });
  plan("bad shape", [](Cfg& c) { c.s.T = 1; });
  plan("lds_bytes NULL", [](Cfg& c) { c.no_params = true; });
  plan("n_arms 0", [](Cfg& c) { c.n_arms = 0; });
  plan("n_arms 17", [](Cfg& c) { c.n_arms = 17; });
  plan("LDS: T 1024", [](Cfg& c) { c.s.T = 1024; });
  plan("LDS: T 500, n_arms 16", [](Cfg& c) { c.s.T = 500; c.n_arms = 16; });
  memory_untouched();
  return 0;
}
