// The arithmetic of one fixed-grid step (euler / midpoint / torchdiffeq's rk4, the 3/8 rule) of x' = a(t, z) - d(t, z) x, written once for
// the training kernel (ode_kernel.hip), the refinement kernel (refine_kernel.hip) and the eval-side forward (slode_forward.h): the stage
// counts, the step coefficients x' = A x + b in two shapes, their reverse mode, and the backward step of reference_adjoint.  Everything is
// host- and device-callable and needs include/slode.h alone, so that tests/fixed_step/fixed_step.cpp holds every routine to
// tests/kernel_math.py and to the oracle without a device (tests/test_fixed_step_cpu.py).
#pragma once
#include "../../include/slode.h"

// ---- stage counts: the only definition of the rule ------------------------------------------------------------------
// the distinct stage times of one step (the rows of the stage-time table per step): euler 1, midpoint 2, rk4 3
__host__ __device__ constexpr int fixed_step_times(int method) { return method == SLODE_EULER ? 1 : (method == SLODE_MIDPOINT ? 2 : 3); }
// the evaluations of a, d one step reads: euler 1, midpoint 2, rk4 4 (its last is the next step's first); times: fixed_step_times(method)
// where the caller holds it already (a kernel, in its arguments)
__host__ __device__ constexpr int fixed_step_evals(int method, int times) { return method == SLODE_RK4 ? 4 : times; }
__host__ __device__ constexpr int fixed_step_evals(int method) { return fixed_step_evals(method, fixed_step_times(method)); }

// ---- step coefficients ------------------------------------------------------------------------------------------
// step_fwd and fwd_step_coeffs are the SAME arithmetic in two shapes -- one state component from its four stage values; all SM components,
// stage by stage, around the caller's evaluator -- operation for operation, so that the eval-side calls reproduce the training kernel's
// states.  tests/test_fixed_step_cpu.py holds the two equal bit for bit in the host build: a change to one is a change to both.

// Step coefficients x' = A x + b for one state component (tests/kernel_math.py::step_coeffs).
// a*/d*: stage values; for rk4 index 3 is the next step's first stage.
__host__ __device__ __forceinline__ void step_fwd(int method, float h, const float a[4], const float d[4], float& A, float& b) {
  if (method == SLODE_EULER) {
    A = 1.f - h * d[0];
    b = h * a[0];
  } else if (method == SLODE_MIDPOINT) {
    const float m = 1.f - 0.5f * h * d[0], c = 0.5f * h * a[0];
    A = 1.f - h * d[1] * m;
    b = h * (a[1] - d[1] * c);
  } else {
    const float h3 = h * (1.0f / 3.0f);
    const float p1 = a[0], q1 = -d[0];
    const float c2 = h3 * p1, m2 = 1.f + h3 * q1;
    const float p2 = a[1] - d[1] * c2, q2 = -d[1] * m2;
    const float c3 = h * (p2 - p1 * (1.0f / 3.0f)), m3 = 1.f + h * (q2 - q1 * (1.0f / 3.0f));
    const float p3 = a[2] - d[2] * c3, q3 = -d[2] * m3;
    const float c4 = h * (p1 - p2 + p3), m4 = 1.f + h * (q1 - q2 + q3);
    const float p4 = a[3] - d[3] * c4, q4 = -d[3] * m4;
    const float G = h * 0.125f;
    A = 1.f + G * (q1 + 3.f * (q2 + q3) + q4);
    b = G * (p1 + 3.f * (p2 + p3) + p4);
  }
}

// x' = A x + b of one grid step of size h (f = a(t, z) - d(t, z) x: tests/kernel_math.py step_coeffs); st: the step's stage times;
// ad(t, a, d): the caller's evaluator of a(t, z), d(t, z) -- eval_stats reads the weights from global memory, the others from the LDS rows
template <int SM, class AD>
__host__ __device__ __forceinline__ void fwd_step_coeffs(int method, float h, const float* st, const AD& ad, float (&A)[SM], float (&bb)[SM]) {
  float a[SM], d[SM];
  ad(st[0], a, d);
  if (method == SLODE_EULER) {
#pragma unroll
    for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s]; bb[s] = h * a[s]; }
  } else if (method == SLODE_MIDPOINT) {
    float m[SM], c[SM];
#pragma unroll
    for (int s = 0; s < SM; ++s) { m[s] = 1.f - 0.5f * h * d[s]; c[s] = 0.5f * h * a[s]; }
    ad(st[1], a, d);
#pragma unroll
    for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s] * m[s]; bb[s] = h * (a[s] - d[s] * c[s]); }
  } else {   // torchdiffeq's rk4: the 3/8 rule
    const float third = 1.0f / 3.0f, h3 = h * third;
    float p1[SM], q1[SM], p2[SM], q2[SM], c[SM], m[SM];
#pragma unroll
    for (int s = 0; s < SM; ++s) { p1[s] = a[s]; q1[s] = -d[s]; c[s] = h3 * p1[s]; m[s] = 1.f + h3 * q1[s]; }
    ad(st[1], a, d);
#pragma unroll
    for (int s = 0; s < SM; ++s) {
      p2[s] = a[s] - d[s] * c[s]; q2[s] = -d[s] * m[s];
      c[s] = h * (p2[s] - p1[s] * third); m[s] = 1.f + h * (q2[s] - q1[s] * third);
    }
    ad(st[2], a, d);
#pragma unroll
    for (int s = 0; s < SM; ++s) {
      const float p3 = a[s] - d[s] * c[s], q3 = -d[s] * m[s];
      c[s] = h * (p1[s] - p2[s] + p3); m[s] = 1.f + h * (q1[s] - q2[s] + q3);
      A[s] = q1[s] + 3.f * (q2[s] + q3); bb[s] = p1[s] + 3.f * (p2[s] + p3);   // (partial sums: q4 / p4 follow)
    }
    ad(st[3], a, d);
    const float G = h * 0.125f;
#pragma unroll
    for (int s = 0; s < SM; ++s) {
      const float p4 = a[s] - d[s] * c[s], q4 = -d[s] * m[s];
      A[s] = 1.f + G * (A[s] + q4); bb[s] = G * (bb[s] + p4);
    }
  }
}

// Reverse mode of the step coefficients for one state component: (gA, gb) -> ga[r], gd[r] of the step's stages
// (tests/kernel_math.py::step_coeffs_bwd; stages beyond the method's own get 0)
__host__ __device__ __forceinline__ void step_bwd(int method, float h, const float (&a)[4], const float (&d)[4], float gA, float gb, float (&ga)[4],
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

// ---- grad_mode = reference_adjoint: torchdiffeq.odeint_adjoint's backward for the fixed-grid solvers (blackbox_ode.py:40-42, the
// reference default; oracle: _OdeintAdjoint).  From node n+1 back to node n (hb = t_n - t_{n+1} < 0) the augmented state
// (y, lam, g_theta) takes ONE step of the same method, y restarting from the stored forward value:
//   dlam/dt = +d(t) lam  =>  lam_n = M lam_{n+1} (+ dLoss/dx_n),      dg_theta/dt = -lam (a' dxa/dtheta - y d' dxd/dtheta).
// D[j] = d at the j-th BACKWARD stage: node n+1, then the forward stages of step n in reverse order (rk4: r = 2, 1, 0).
__host__ __device__ __forceinline__ float radj_M(int method, float hb, const float D[4]) {
  if (method == SLODE_EULER) return 1.f + hb * D[0];
  if (method == SLODE_MIDPOINT) return 1.f + hb * D[1] * (1.f + 0.5f * hb * D[0]);
  const float h3 = hb * (1.0f / 3.0f);
  const float m2 = 1.f + h3 * D[0];
  const float m3 = 1.f + hb * (D[1] * m2 - D[0] * (1.0f / 3.0f));
  const float m4 = 1.f + hb * (D[0] - D[1] * m2 + D[2] * m3);
  return 1.f + hb * 0.125f * (D[0] + 3.f * (D[1] * m2 + D[2] * m3) + D[3] * m4);
}
// Quadrature of the parameter adjoint over one backward step: per backward stage j the weights of dxa/dtheta and dxd/dtheta
// BEFORE the sigmoid derivatives: gaq[j] = -w_j lam_j, gdq[j] = +w_j lam_j y_j  (w = hb * RK weights).
__host__ __device__ __forceinline__ void radj_stage_grads(int method, float hb, const float A[4], const float D[4], float lam, float y,
                                                 float gaq[4], float gdq[4]) {
  gaq[0] = gaq[1] = gaq[2] = gaq[3] = 0.f;
  gdq[0] = gdq[1] = gdq[2] = gdq[3] = 0.f;
  if (method == SLODE_EULER) {
    gaq[0] = -hb * lam;
    gdq[0] = hb * lam * y;
  } else if (method == SLODE_MIDPOINT) {
    const float ym = y + 0.5f * hb * (A[0] - D[0] * y), lm = (1.f + 0.5f * hb * D[0]) * lam;
    gaq[1] = -hb * lm;
    gdq[1] = hb * lm * ym;
  } else {
    const float h3 = hb * (1.0f / 3.0f), w1 = hb * 0.125f, w3 = hb * 0.375f;
    const float k1 = A[0] - D[0] * y, m2 = 1.f + h3 * D[0];
    const float y2 = y + h3 * k1, k2 = A[1] - D[1] * y2;
    const float m3 = 1.f + hb * (D[1] * m2 - D[0] * (1.0f / 3.0f));
    const float y3 = y + hb * (k2 - k1 * (1.0f / 3.0f)), k3 = A[2] - D[2] * y3;
    const float m4 = 1.f + hb * (D[0] - D[1] * m2 + D[2] * m3);
    const float y4 = y + hb * (k1 - k2 + k3);
    gaq[0] = -w1 * lam;            gdq[0] = w1 * lam * y;
    gaq[1] = -w3 * m2 * lam;       gdq[1] = w3 * m2 * lam * y2;
    gaq[2] = -w3 * m3 * lam;       gdq[2] = w3 * m3 * lam * y3;
    gaq[3] = -w1 * m4 * lam;       gdq[3] = w1 * m4 * lam * y4;
  }
}
