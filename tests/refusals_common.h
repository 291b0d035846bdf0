// What the seven refusal programs (tests/eval_refusals, forecast_refusals, cohort_refusals, calibration_refusals, evidence_refusals,
// refine_refusals, pointwise_refusals) share.  Each calls entry points of
// libslode.so in every refusing configuration on a hand-filled handle -- no slode_create, no HIP call, no device -- and prints one line
// per case:
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
