// Every refusing configuration of slode_mechanism_moments and slode_mechanism_plan on a hand-filled handle: no slode_create, no HIP call, no
// device.  One line per case:
//   <case> | <call> | <status> | <rng_counter afterwards> | <slode_last_error>
// in rung order: the ladder of slode_recon_moments on that side without its LDS rung (tests/eval_refusals), then the call's own rungs -- mean,
// the slot mask, the LDS tables -- then the label tensors and the workspace.  tests/golden/mechanism_refusals.txt holds these lines;
// tests/test_mechanism_cpu.py compares.  No refusal touches HIP and a refused call launches nothing, so this program makes NO call that would
// be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 mechanism_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

struct Cfg : BaseCfg {
  unsigned int slots = (1u << SLODE_MECHANISM_SLOTS) - 1;
  float *mean = DEV, *sd = DEV;
  size_t plan_bytes = 0;
  bool plan_out = true;
};

static int call(int which, Cfg& c, const Head& a, const char** column) {
  if (which == 1) {
    *column = "plan";
    const int rc = slode_mechanism_plan(a.s, c.slots, c.plan_out ? &c.plan_bytes : nullptr);
    c.ctx.rng_counter = c.plan_bytes;   // (the plan has no generator: the column shows the bytes it wrote, refused or not)
    return rc;
  }
  *column = c.is_post ? "post" : "prior";
  return slode_mechanism_moments(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.slots, c.mean, c.sd, c.ws, c.ws_bytes, nullptr);
}


// T = 1024, S = 5, C = 3: the step table and the capture table are 40 KB each and one slot's moment triples 60 KB -- one slot fits, two do not
static void big(Cfg& c) { c.s.T = 1024; c.b.obs_strides[0] = 3072; }

int main() {
  ladder_pointers();
  // ---- the draw count
  pair("num_samples 0", [](Cfg& c) { c.draws = 0; });
  pair("num_samples 2^30", [](Cfg& c) { c.draws = 1 << 30; });
  ladder_not_taken();
  ladder_post_obs();
  // ---- the call's own rungs
  pair("mean NULL", [](Cfg& c) { c.mean = nullptr; });
  pair("slots 0", [](Cfg& c) { c.slots = 0; });
  pair("slots bit 5", [](Cfg& c) { c.slots = 1u << 5; });
  pair("slots all + bit 31", [](Cfg& c) { c.slots |= 1u << 31; });
  pair("LDS: T 1024, five slots", [](Cfg& c) { big(c); c.ws_bytes = 64; });
  pair("LDS: T 1024, two slots", [](Cfg& c) { big(c); c.slots = 0x12; c.ws_bytes = 64; });
  pair("T 1024, one slot, run-time S build: fits; workspace too small",[](Cfg& c) { big(c); c.slots = 0x8; c.ctx.ode_generic = 1; c.ws_bytes = 64; });
  pair("T 1024, one slot: fits; workspace too small", [](Cfg& c) { big(c); c.slots = 0x8; c.ws_bytes = 64; });
  ladder_labels();
  // ---- the workspace
  pair("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  pair("sd NULL, one slot; workspace too small", [](Cfg& c) { c.sd = nullptr; c.slots = 1; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier rung speaks
  ladder_two_at_once(0);
  post("no_fold + mean NULL", [](Cfg& c) { c.ctx.no_fold = 1; c.mean = nullptr; });
  pair("mean NULL + slots 0", [](Cfg& c) { c.mean = nullptr; c.slots = 0; });
  pair("slots bit 7 + LDS", [](Cfg& c) { c.slots = 0x9f; big(c); });
  pair("LDS + label columns 3", [](Cfg& c) { big(c); c.b.label_width[1] = 2; });
  pair("label columns 3 + workspace too small", [](Cfg& c) { c.b.label_width[1] = 2; c.ws_bytes = 64; });
  // ---- the plan: host arithmetic alone (the counter column: the bytes written)
  plan("shape NULL", [](Cfg& c) { c.no_shape = true; });
  plan("bad shape", [](Cfg& c) { c.s.T = 1; });
  plan("lds_bytes NULL", [](Cfg& c) { c.plan_out = false; });
  plan("slots 0", [](Cfg& c) { c.slots = 0; });
  plan("slots bit 5", [](Cfg& c) { c.slots = 0x21; });
  plan("LDS: T 1024, five slots", [](Cfg& c) { big(c); });
  plan("LDS: T 1024, two slots", [](Cfg& c) { big(c); c.slots = 0x3; });
  memory_untouched();
  return 0;
}
