// The reverse of one grid step's coefficients, the routine of refine_kernel.hip (R7) -- in a header of its own, host- and device-callable,
// so that tests/refine_step/refine_step.cpp can hold it to tests/kernel_math.py::step_coeffs_bwd without a device.  ode_kernel.hip keeps its
// own copy (step_bwd); unifying the two is a later change.
#pragma once
#include "../../include/slode.h"

// Reverse mode of fwd_step_coeffs for one state component: (gA, gb) -> ga[r], gd[r] of the step's stages (tests/kernel_math.py::step_coeffs_bwd;
// stages beyond the method's own get 0)
__host__ __device__ __forceinline__ void rf_step_bwd(int method, float h, const float (&a)[4], const float (&d)[4], float gA, float gb, float (&ga)[4],
                                            float (&gd)[4]) {
  if (method == SLODE_EULER) {
    gd[0] = -h * gA; ga[0] = h * gb;
    ga[1] = gd[1] = ga[2] = gd[2] = ga[3] = gd[3] = 0.f;
  } else if (method == SLODE_MIDPOINT) {
    const float m = 1.f - 0.5f * h * d[0], c = 0.5f * h * a[0];
    ga[1] = h * gb;
    gd[1] = -h * (m * gA + c * gb);
    const float gm = -h * d[1] * gA, gc = -h * d[1] * gb;
    gd[0] = -0.5f * h * gm; ga[0] = 0.5f * h * gc;
    ga[2] = gd[2] = ga[3] = gd[3] = 0.f;
  } else {   // torchdiffeq's rk4: the 3/8 rule
    const float third = 1.0f / 3.0f, h3 = h * third, G = h * 0.125f;
    const float p1 = a[0], q1 = -d[0];
    const float c2 = h3 * p1, m2 = 1.f + h3 * q1;
    const float p2 = a[1] - d[1] * c2, q2 = -d[1] * m2;
    const float c3 = h * (p2 - p1 * third), m3 = 1.f + h * (q2 - q1 * third);
    const float p3 = a[2] - d[2] * c3, q3 = -d[2] * m3;
    const float c4 = h * (p1 - p2 + p3), m4 = 1.f + h * (q1 - q2 + q3);
    float gp1 = G * gb, gq1 = G * gA;
    const float gp4 = G * gb, gq4 = G * gA;
    float gp2 = 3.f * G * gb, gp3 = 3.f * G * gb, gq2 = 3.f * G * gA, gq3 = 3.f * G * gA;
    ga[3] = gp4; gd[3] = -c4 * gp4 - m4 * gq4;
    const float gc4 = -d[3] * gp4, gm4 = -d[3] * gq4;
    gp1 += h * gc4; gp2 -= h * gc4; gp3 += h * gc4;
    gq1 += h * gm4; gq2 -= h * gm4; gq3 += h * gm4;
    ga[2] = gp3; gd[2] = -c3 * gp3 - m3 * gq3;
    const float gc3 = -d[2] * gp3, gm3 = -d[2] * gq3;
    gp2 += h * gc3; gp1 -= h3 * gc3;
    gq2 += h * gm3; gq1 -= h3 * gm3;
    ga[1] = gp2; gd[1] = -c2 * gp2 - m2 * gq2;
    const float gc2 = -d[1] * gp2, gm2 = -d[1] * gq2;
    gp1 += h3 * gc2; gq1 += h3 * gm2;
    ga[0] = gp1; gd[0] = -gq1;
  }
}

