// Every routine of csrc/fixed_step.h -- the arithmetic of one fixed-grid step as ode_kernel.hip, refine_kernel.hip and the eval-side kernels
// execute it -- on the host, for tests/test_fixed_step_cpu.py to compare with tests/kernel_math.py and the oracle.  Reads one request per line
// from standard input and prints one line of results for each (%.9g: every float32 exactly):
//   counts method                                    -> stage times and evaluations of one step
//   fwd    method h  a0 a1 a2 a3 d0 d1 d2 d3         -> A b                                          (step_fwd)
//   bwd    method h  a0 a1 a2 a3 d0 d1 d2 d3 gA gb   -> ga0 ga1 ga2 ga3 gd0 gd1 gd2 gd3              (step_bwd)
//   radj   method hb A0 A1 A2 A3 D0 D1 D2 D3 lam y   -> M gaq0 gaq1 gaq2 gaq3 gdq0 gdq1 gdq2 gdq3    (radj_M, radj_stage_grads)
//   coeffs SM method h, then a0 .. a3 d0 .. d3 of each of the SM components (SM = 5 or 8)
//                                                    -> the bit patterns of A, b per component: fwd_step_coeffs<SM>, then step_fwd
// In coeffs the stage "times" are the stage indices 0 .. 3 and the evaluator looks the request's stage values up by them.
// No device, no HIP call.  Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 fixed_step.cpp
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "../../structured_latent_odes_amd/csrc/fixed_step.h"

static bool read_floats(float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%f", &v[i]) != 1) return false;
  return true;
}

static unsigned bits(float x) {
  unsigned u;
  memcpy(&u, &x, sizeof u);
  return u;
}

template <int SM>
static bool coeffs(int method, float h) {
  float ta[SM][4], td[SM][4];
  for (int s = 0; s < SM; ++s)
    if (!read_floats(ta[s], 4) || !read_floats(td[s], 4)) return false;
  const float st[4] = {0.f, 1.f, 2.f, 3.f};
  float A[SM], bb[SM];
  fwd_step_coeffs<SM>(method, h, st, [&](float t, float (&a)[SM], float (&d)[SM]) {
    for (int s = 0; s < SM; ++s) { a[s] = ta[s][(int)t]; d[s] = td[s][(int)t]; }
  }, A, bb);
  for (int s = 0; s < SM; ++s) printf("%08x %08x ", bits(A[s]), bits(bb[s]));
  for (int s = 0; s < SM; ++s) {
    float A1, b1;
    step_fwd(method, h, ta[s], td[s], A1, b1);
    printf("%08x %08x ", bits(A1), bits(b1));
  }
  printf("\n");
  return true;
}

int main() {
  char what[16];
  int method;
  while (scanf("%15s", what) == 1) {
    float h, a[4], d[4], g[2];
    if (!strcmp(what, "counts")) {
      if (scanf("%d", &method) != 1) return 1;
      printf("%d %d\n", fixed_step_times(method), fixed_step_evals(method));
    } else if (!strcmp(what, "coeffs")) {
      int sm;
      if (scanf("%d %d %f", &sm, &method, &h) != 3 || !(sm == 5 ? coeffs<5>(method, h) : sm == 8 ? coeffs<8>(method, h) : false)) return 1;
    } else {
      if (scanf("%d %f", &method, &h) != 2 || !read_floats(a, 4) || !read_floats(d, 4)) return 1;
      if (!strcmp(what, "fwd")) {
        float A, b;
        step_fwd(method, h, a, d, A, b);
        printf("%.9g %.9g\n", A, b);
      } else if (!strcmp(what, "bwd")) {
        if (!read_floats(g, 2)) return 1;
        float ga[4], gd[4];
        step_bwd(method, h, a, d, g[0], g[1], ga, gd);
        printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", ga[0], ga[1], ga[2], ga[3], gd[0], gd[1], gd[2], gd[3]);
      } else if (!strcmp(what, "radj")) {
        if (!read_floats(g, 2)) return 1;
        float gaq[4], gdq[4];
        radj_stage_grads(method, h, a, d, g[0], g[1], gaq, gdq);
        printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", radj_M(method, h, d), gaq[0], gaq[1], gaq[2], gaq[3], gdq[0], gdq[1], gdq[2],
               gdq[3]);
      } else {
        return 1;
      }
    }
  }
  return 0;
}
