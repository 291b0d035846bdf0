// What the twelve refusal programs share: tests/eval_refusals, forecast_refusals, cohort_refusals, calibration_refusals, evidence_refusals,
// refine_refusals, pointwise_refusals, and the five of the whole-curve calls -- attribution_refusals, summary_refusals, quantile_refusals,
// mechanism_refusals, band_refusals -- which also share the ladder of slode_recon_moments as sections (the end of this file).  Each calls
// entry points of libslode.so in every refusing configuration on a hand-filled handle -- no slode_create, no HIP call, no device -- and
// prints one line per case:
//   <case> | [<call> |] <status> | <rng_counter afterwards> | <slode_last_error>
// A program defines `struct Cfg : BaseCfg` (what its call takes besides), `call` (its one call expression) and its case table in main.
#pragma once
#include "../structured_latent_odes_amd/csrc/slode_common.h"

#include <functional>
#include <stdio.h>
#include <string.h>

alignas(64) static float g_mem[64];   // stands for every device buffer: non-NULL, never read or written
static float* const DEV = g_mem;
static const size_t BIG = (size_t)1 << 40;   // a workspace is "large enough" unless a case says otherwise

// What every eval-side call takes.  As constructed: B = 4, T = 86, C = 3 with the cvs prior groups (tests/test_host_cpu.py::_shape), dense
// [B,T,C] observations, two label tensors.
struct BaseCfg {
  slode_ctx ctx;
  slode_shape s;
  slode_batch b;
  bool no_handle = false, no_shape = false, no_layout = false, no_params = false, no_batch = false;
  const float *times = DEV, *stage_t = DEV;
  void* ws = DEV;
  size_t ws_bytes = BIG;
  int draws = 2, is_post = 1;
  BaseCfg() {
    memset(&ctx, 0, sizeof(ctx));
    ctx.num_cu = 256; ctx.enc_fuse = 1; ctx.rng_seed = 3;
    memset(&s, 0, sizeof(s));
    s.B = 4; s.T = 86; s.C = 3; s.L = 8; s.S = 5; s.H = 25; s.F = 10; s.K = 10; s.P = 5; s.Hc = 50;
    s.n_u = 2; s.n_groups = 2; s.groups[0] = slode_group{0, 3, 0, 1}; s.groups[1] = slode_group{3, 3, 1, 1};
    s.method = SLODE_RK4; s.likelihood = SLODE_ALD; s.quantile_diff = 0.475f; s.rtol = 1e-7f; s.atol = 1e-9f;
    memset(&b, 0, sizeof(b));
    b.obs = DEV; b.obs_strides[0] = (int64_t)s.C * s.T; b.obs_strides[1] = 1; b.obs_strides[2] = s.C;
    b.n_labels = 2; b.label_width[0] = b.label_width[1] = 1; b.labels[0] = b.labels[1] = DEV;
  }
};

// The arguments every call begins with, NULL where the case says so; the generator's counter is preset to 7.
struct Head {
  slode_layout lay;
  slode_handle h;
  const slode_shape* s;
  const slode_layout* l;
  const float* p;
  const slode_batch* b;
  explicit Head(BaseCfg& c) {
    slode_shape plain = BaseCfg().s;   // (the layout of the unmodified shape where the case's own shape is not a valid one)
    if (slode_layout_init(&c.s, &lay) != SLODE_OK) slode_layout_init(&plain, &lay);
    c.ctx.rng_counter = 7;
    h = c.no_handle ? nullptr : &c.ctx;
    s = c.no_shape ? nullptr : &c.s;
    l = c.no_layout ? nullptr : &lay;
    p = c.no_params ? nullptr : DEV;
    b = c.no_batch ? nullptr : &c.b;
  }
  Head(const Head&) = delete;
};

static void report(const char* name, const char* column, int rc, const BaseCfg& c, slode_handle h) {
  printf("%s | ", name);
  if (column) printf("%s | ", column);
  printf("%d | %llu | %s\n", rc, (unsigned long long)c.ctx.rng_counter, slode_last_error(h));
}

// ---- the including program's two
struct Cfg;
// Call number `which` of the program in configuration c -> its status; *column: the <call> column of the line, where the program has one.
static int call(int which, Cfg& c, const Head& a, const char** column);

// (The routines below are templates only so that their bodies are compiled where they are used: in main, where Cfg is complete.)
typedef std::function<void(Cfg&)> Edit;
template <class C = Cfg>
static void run(const char* name, C c, int which = 0) {
  Head a(c);
  const char* column = nullptr;
  const int rc = call(which, c, a, &column);
  report(name, column, rc, c, a.h);
}
template <class C = Cfg>
static void one(const char* name, const Edit& edit) { C c; edit(c); run(name, c); }
// posterior and prior
template <class C = Cfg>
static void both(const char* name, const Edit& edit) {
  char n[128];
  for (int post : {1, 0}) {
    snprintf(n, sizeof(n), "%s: %s", post ? "post" : "prior", name);
    C c; c.is_post = post; edit(c); run(n, c);
  }
}
// several calls of the program
template <class C = Cfg>
static void each(const char* name, std::initializer_list<int> calls, const Edit& edit) {
  for (int which : calls) { C c; edit(c); run(name, c, which); }
}

// ---- the five programs of the whole-curve calls: every line carries the <call> column (post / prior / plan) and a case has one name on
// both sides.  call 0: the call itself; call 1: its plan, which takes no handle (its reason is the global text, which a NULL handle reads).
template <class C = Cfg>
static void pair(const char* name, const Edit& edit) {
  for (int post : {1, 0}) { C c; c.is_post = post; edit(c); run(name, c); }
}
template <class C = Cfg>
static void post(const char* name, const Edit& edit) { one(name, edit); }
template <class C = Cfg>
static void prior(const char* name, const Edit& edit) { C c; c.is_post = 0; edit(c); run(name, c); }
template <class C = Cfg>
static void plan(const char* name, const Edit& edit) { C c; c.no_handle = true; edit(c); run(name, c, 1); }

// The ladder of slode_recon_moments without its LDS rung, in sections: a program calls each where its lines stand, its own rungs between them.
template <class C = Cfg>
static void ladder_pointers() {
  pair("handle NULL", [](C& c) { c.no_handle = true; });
  pair("shape NULL", [](C& c) { c.no_shape = true; });
  pair("layout NULL", [](C& c) { c.no_layout = true; });
  pair("params NULL", [](C& c) { c.no_params = true; });
  pair("batch NULL", [](C& c) { c.no_batch = true; });
  pair("times NULL", [](C& c) { c.times = nullptr; });
  pair("stage_t NULL", [](C& c) { c.stage_t = nullptr; });
  pair("workspace NULL", [](C& c) { c.ws = nullptr; });
  pair("bad shape", [](C& c) { c.s.T = 1; });
}
// what the fused kernels do not take
template <class C = Cfg>
static void ladder_not_taken() {
  for (int m : {SLODE_DOPRI5, SLODE_BOSH3, SLODE_FEHLBERG2, SLODE_ADAPTIVE_HEUN}) {
    char name[64];
    snprintf(name, sizeof(name), "adaptive method %d", m);
    pair(name, [m](C& c) { c.s.method = m; });
  }
  pair("particles 2", [](C& c) { c.s.particles = 2; });
  pair("fold_on", [](C& c) { c.ctx.fold_on = 1; });
  pair("ode_pack", [](C& c) { c.ctx.ode_pack = 4; });
  pair("ode_alg", [](C& c) { c.ctx.ode_alg = 1; });
}
// the observations: the posterior reads them
template <class C = Cfg>
static void ladder_post_obs() {
  post("obs NULL", [](C& c) { c.b.obs = nullptr; });
  post("padded strides", [](C& c) { c.b.obs_strides[0] += 8; });
  post("channel-major strides of another T", [](C& c) { c.b.obs_strides[1] = c.s.T + 1; c.b.obs_strides[2] = 1; });
  post("no_fold", [](C& c) { c.ctx.no_fold = 1; });
}
template <class C = Cfg>
static void ladder_labels() {
  pair("label columns 3, n_u 2", [](C& c) { c.b.label_width[1] = 2; });
  pair("n_labels 5", [](C& c) { c.b.n_labels = 5; });
  pair("label tensor 1 NULL", [](C& c) { c.b.labels[1] = nullptr; });
  prior("no label tensors", [](C& c) { c.b.n_labels = 0; });
}
// two conditions at once, up to the observations: the earlier rung speaks.  low: the largest draw count the call refuses as too small
template <class C = Cfg>
static void ladder_two_at_once(int low) {
  char name[64];
  pair("params NULL + batch NULL", [](C& c) { c.no_params = true; c.no_batch = true; });
  snprintf(name, sizeof(name), "times NULL + num_samples %d", low);
  pair(name, [low](C& c) { c.times = nullptr; c.draws = low; });
  snprintf(name, sizeof(name), "num_samples %d + adaptive", low);
  pair(name, [low](C& c) { c.draws = low; c.s.method = SLODE_DOPRI5; });
  pair("adaptive + particles 2", [](C& c) { c.s.method = SLODE_BOSH3; c.s.particles = 2; });
  post("ode_alg + obs NULL", [](C& c) { c.ctx.ode_alg = 2; c.b.obs = nullptr; });
}
// the last line: the memory that stands for every output was never written
static void memory_untouched() {
  bool clean = true;
  for (float v : g_mem) clean = clean && v == 0.f;
  printf("memory that stands for the outputs | %s\n", clean ? "untouched" : "WRITTEN");
}
