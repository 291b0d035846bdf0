// rf_step_bwd (csrc/refine_step.h: the reverse of one grid step's coefficients, as refine_kernel.hip executes it) on the host, for
// tests/test_refine_cpu.py to compare with tests/kernel_math.py::step_coeffs_bwd.  Reads lines "method h a0 a1 a2 a3 d0 d1 d2 d3 gA gb" from
// standard input and prints "ga0 ga1 ga2 ga3 gd0 gd1 gd2 gd3" (%.9g: every float32 exactly) for each.  No device, no HIP call.
// Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 refine_step.cpp
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../structured_latent_odes_amd/csrc/refine_step.h"

int main() {
  int method;
  float h, a[4], d[4], gA, gb;
  while (scanf("%d %f %f %f %f %f %f %f %f %f %f %f", &method, &h, &a[0], &a[1], &a[2], &a[3], &d[0], &d[1], &d[2], &d[3], &gA, &gb) == 12) {
    float ga[4], gd[4];
    rf_step_bwd(method, h, a, d, gA, gb, ga, gd);
    printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", ga[0], ga[1], ga[2], ga[3], gd[0], gd[1], gd[2], gd[3]);
  }
  return 0;
}
