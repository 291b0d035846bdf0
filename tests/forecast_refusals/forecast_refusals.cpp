// Every refusing configuration of slode_forecast_moments (and of slode_stage_times_n), on a hand-filled handle: no slode_create, no HIP
// call, no device.  One line per case:
//   <case> | <status> | <rng_counter afterwards> | <slode_last_error>
// tests/golden/forecast_refusals.txt holds these lines; tests/test_forecast_cpu.py compares.  No refusal touches HIP and a refused call
// launches nothing, so this program makes NO call that would be taken: a taken call would launch.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 forecast_refusals.cpp -x none <package dir>/libslode.so
#include "../refusals_common.h"

struct Cfg : BaseCfg {
  const float *times_out = DEV, *stage_t_out = DEV;
  float *mean = DEV, *sd = DEV, *x_mean = DEV, *x_sd = DEV;
  int T_out = 95, window = 0;
};

static int call(int, Cfg& c, const Head& a, const char**) {
  return slode_forecast_moments(a.h, a.s, a.l, a.p, c.times, c.stage_t, a.b, c.is_post, c.draws, c.times_out, c.stage_t_out, c.T_out, c.window,
                                c.mean, c.sd, c.x_mean, c.x_sd, c.ws, c.ws_bytes, nullptr);
}

int main() {
  // ---- what slode_recon_moments refuses for the same is_post, in its order
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
  one("post: obs NULL", [](Cfg& c) { c.b.obs = nullptr; });
  one("post: padded strides", [](Cfg& c) { c.b.obs_strides[0] += 8; });
  one("post: channel-major strides of another T", [](Cfg& c) { c.b.obs_strides[1] = c.s.T + 1; c.b.obs_strides[2] = 1; });
  one("post: no_fold", [](Cfg& c) { c.ctx.no_fold = 1; });
  one("prior: obs NULL, padded strides, no_fold; workspace too small", [](Cfg& c) { c.is_post = 0; c.b.obs = nullptr; c.b.obs_strides[0] += 8; c.ctx.no_fold = 1; c.ws_bytes = 64; });
  // ---- the call's own rungs
  both("times_out NULL", [](Cfg& c) { c.times_out = nullptr; });
  both("stage_t_out NULL", [](Cfg& c) { c.stage_t_out = nullptr; });
  both("T_out 1", [](Cfg& c) { c.T_out = 1; });
  both("T_out 2^20 + 1", [](Cfg& c) { c.T_out = (1 << 20) + 1; });
  both("mean NULL", [](Cfg& c) { c.mean = nullptr; });
  both("window -1", [](Cfg& c) { c.window = -1; });
  // ---- the plan's refusal, as the LDS rung (a workspace too small behind it: the plan is asked first)
  both("window 30000 of T_out 2^20", [](Cfg& c) { c.T_out = 1 << 20; c.window = 30000; c.ws_bytes = 64; });
  both("window 4000, states", [](Cfg& c) { c.T_out = 5000; c.window = 4000; c.ws_bytes = 64; });
  both("window 2^20 clamped to T_out - 1 = 4999", [](Cfg& c) { c.T_out = 5000; c.window = 1 << 20; c.x_mean = c.x_sd = nullptr; c.ws_bytes = 64; });
  both("draws 10000: the carry leaves no room", [](Cfg& c) { c.draws = 10000; c.ws_bytes = 64; });
  both("draws 10000, run-time S", [](Cfg& c) { c.draws = 10000; c.ctx.ode_generic = 1; c.ws_bytes = 64; });
  // ---- the label tensors, the workspace
  both("label columns 3, n_u 2", [](Cfg& c) { c.b.label_width[1] = 2; });
  both("label tensor 1 NULL", [](Cfg& c) { c.b.labels[1] = nullptr; });
  one("prior without labels", [](Cfg& c) { c.is_post = 0; c.b.n_labels = 0; });
  both("workspace too small", [](Cfg& c) { c.ws_bytes = 64; });
  both("workspace too small, T_out 2^20, window 0", [](Cfg& c) { c.T_out = 1 << 20; c.ws_bytes = 64; });
  // ---- two conditions at once: the earlier check of the ladder names the reason
  both("params NULL + batch NULL", [](Cfg& c) { c.no_params = true; c.no_batch = true; });
  both("draws 0 + adaptive", [](Cfg& c) { c.draws = 0; c.s.method = SLODE_DOPRI5; });
  both("adaptive + T_out 1", [](Cfg& c) { c.s.method = SLODE_BOSH3; c.T_out = 1; });
  one("post: padded strides + times_out NULL", [](Cfg& c) { c.b.obs_strides[0] += 8; c.times_out = nullptr; });
  both("times_out NULL + T_out 1", [](Cfg& c) { c.times_out = nullptr; c.T_out = 1; });
  both("T_out 1 + mean NULL", [](Cfg& c) { c.T_out = 1; c.mean = nullptr; });
  both("mean NULL + window -1", [](Cfg& c) { c.mean = nullptr; c.window = -1; });
  both("window -1 + draws 10000", [](Cfg& c) { c.window = -1; c.draws = 10000; });
  both("unfit window + label columns 3", [](Cfg& c) { c.T_out = 5000; c.window = 4000; c.b.label_width[1] = 2; });
  // ---- slode_stage_times_n
  {
    Cfg c;
    slode_handle h = &c.ctx;
    c.ctx.rng_counter = 7;
    struct { const char* name; slode_handle h; const slode_shape* s; int n; const float* t; float* st; } cases[] = {
        {"stage_times_n: handle NULL", nullptr, &c.s, 95, DEV, DEV}, {"stage_times_n: shape NULL", h, nullptr, 95, DEV, DEV},
        {"stage_times_n: n_times 1", h, &c.s, 1, DEV, DEV}, {"stage_times_n: n_times 2^20 + 1", h, &c.s, (1 << 20) + 1, DEV, DEV},
        {"stage_times_n: times NULL", h, &c.s, 95, nullptr, DEV}, {"stage_times_n: stage_t NULL", h, &c.s, 95, DEV, nullptr}};
    for (const auto& k : cases) {
      report(k.name, nullptr, slode_stage_times_n(k.h, k.s, k.n, k.t, k.st, nullptr), c, k.h);
    }
  }
  return 0;
}
