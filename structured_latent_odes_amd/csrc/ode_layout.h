// The layout arithmetic of the fused ODE / ELBO kernel (ode_kernel.hip): how a workgroup carves its LDS and how many threads a
// trajectory takes.  Host- and device-callable; ode_elbo_kernel computes its LdsMap from its template arguments with these routines, and
// ode_select.h sizes the launch with the same ones.  Bodies moved here from ode_kernel.hip unchanged.
#pragma once
#include "slode_common.h"

namespace {   // (internal linkage, as in the translation unit they came from)

struct LdsMap {  // offsets in floats
  int ts, sig, A, x, lam, st, stn, ax, ct, gm, hp, tau, ps, ord, sgs, ewt, epre, epre0, esw, ms, sf, par, uu, auxh, auxd, auxgo, z, gzl, gpl, gls, u, wt, pre0,
      hid0, x0, go, gp0, gu, red, pf, meta, total;
};

__host__ __device__ constexpr int pad4(int n) { return (n + 3) & ~3; }
// samples by which NQ = nthreads / 2S chunks of ceil(nt / NQ) samples overhang the stage-time table; 0 when that is more than 8 rows
__host__ __device__ constexpr int ode_pad_rows(int nt, int nthreads, int S) {
  const int nq = nthreads / (2 * S), cl = (nt + nq - 1) / nq, over = nq * cl - nt;
  return over <= 8 ? over : 0;
}
__host__ __device__ constexpr bool ode_full_chunks(int nt, int nthreads, int S) {
  const int nq = nthreads / (2 * S), cl = (nt + nq - 1) / nq;
  return nq * cl - nt <= 8;
}
__host__ __device__ inline int imax2(int a, int b) { return a > b ? a : b; }
// Long latents (L >= 32: the proc family's 50): only the parameters the solver phases re-read stay in LDS -- [init b1 | W2 | b2] and
// [dyn b_h | W_g | b_g | W_d | b_d] -- the prior nets, the L-wide rows of the init net and of the hidden layer and the label heads are
// read from global memory (L2 / L1 hits: every workgroup reads the same 20 KB) by the few phases that touch them once per trajectory.
// 22 KB of LDS per workgroup less: 4 workgroups per CU instead of 2 for BASELINE config[2]'s shapes.
__host__ __device__ constexpr bool ode_cold_global(int L_) { return L_ >= 32; }
__host__ __device__ constexpr int ode_hot_r1(int S, int H) { return H + S * H + S; }            // b1 | W2 | b2
__host__ __device__ constexpr int ode_hot_r2(int S, int H) { return H + 2 * (S * H + S); }      // b_h | W_g | b_g | W_d | b_d
__host__ __device__ constexpr int ode_hot_floats(int S, int H) { return ode_hot_r1(S, H) + ode_hot_r2(S, H); }

// `one`: loop-free form (one workgroup per trajectory): softplus(constant_std) stays in registers, no s_sig.
// The block A | x | lam | st is one work region: besides the scan operands it holds, at different times, the piecewise-linear table of
// the dynamics heads (P1), the stage-0 exchange rows / dLoss/dmu (P1, P3), the per-sample gradient rows G[nt][2S] (P5 -> P6) and the
// staged encoder head weights (P7).
// `scorer`: the shape-specialised solver-free scorer (ALG 3) touches neither the scan operands A / lam, nor the sample rows, the chunk
// sums, GM | GT or the event arrays: they get no space (their offsets alias what follows; nothing reads or writes them).
__host__ __device__ inline LdsMap lds_map(int T, int S, int H, int C, int L, int Q, int nt, int npar, int nthreads, int naux, bool one,
                                          bool scorer = false) {
  LdsMap m;
  int o = 0;
  if (scorer) {
    m.ts = o; o += pad4(nt);
    m.sig = o; o += one ? 0 : pad4(C * T);
    m.ax = pad4(T * S);
    m.A = o; m.lam = o;                 // (unused)
    m.x = o; o += m.ax;
    m.st = o; m.stn = pad4(Q * C * T); o += m.stn;   // dLoss/dmu [Q*C][T]
    m.ct = o; m.gm = o;                 // (unused)
    m.hp = o; o += pad4(4 * Q * C * S);
    m.tau = m.ps = m.ord = m.sgs = m.ewt = m.epre = m.epre0 = m.esw = m.ms = m.sf = o;   // (unused)
  } else {
  // P6 reads the sample rows in chunks of CL = ceil(nt / NQ) samples: when the last chunk overhangs the table by a few samples, zero
  // pad rows (and pad stage times) make every chunk full, and the contraction needs no bounds at all (ode_pad_rows)
  const int padr = ode_pad_rows(nt, nthreads, S);
  m.ts = o; o += pad4(nt + padr);
  m.sig = o; o += one ? 0 : pad4(C * T);
  const int tabn = (H + 1) * 4 * S;   // table rows [H+1][V (2S) | slope (2S)]
  m.ax = imax2(pad4(T * S), pad4((tabn + 2) / 3));
  m.A = o; o += m.ax;
  m.x = o; o += m.ax;
  m.lam = o; o += m.ax;
  int stn = imax2(((2 * S + 4) & ~3) * T, Q * C * T);   // stage-0 exchange rows [T][SP]; dLoss/dmu [Q*C][T]
  stn = imax2(stn, (nt + padr) * 2 * S - 3 * m.ax);     // G rows (+ pad rows) overlay the whole block
  m.st = o; m.stn = pad4(stn); o += m.stn;
  m.ct = o; o += pad4((nthreads / (2 * S) + 1) * 4 * S);   // chunk sums [NQ (+1: total)][sum g (2S) | sum g t (2S)]
  m.gm = o; o += 2 * 2 * S * 32;                        // GM | GT: [2][2S][32] (unit H = the constant-1 unit)
  m.hp = o; o += pad4(4 * Q * C * S);                   // head-weight partials [hsplit][Q*C*S]
  m.tau = o; o += 32;
  m.ps = o; o += 32;
  m.ord = o; o += 32;
  m.sgs = o; o += 32;
  m.ewt = o; o += 32;
  m.epre = o; o += 32;
  m.epre0 = o; o += 32;
  m.esw = o; o += 32 * 2 * S;                           // events in table order: sign * W[c][unit], [32][2S]
  m.ms = o; o += 32;
  m.sf = o; o += 32;
  }
  m.uu = o; o += SLODE_MAX_NU;
  m.z = o; o += pad4(L);
  m.gzl = o; o += pad4(L);
  m.gpl = o; o += pad4(2 * L);  // [d(-log p)/d prior loc | eps]
  m.gls = o; o += pad4(2 * L);  // [d(-log p)/d prior log-scale | guide scale]
  m.u = o; o += 32;
  m.wt = o; o += 32;
  m.pre0 = o; o += 32;
  m.hid0 = o; o += 32;
  m.x0 = o; o += 8;
  m.go = o; o += 8;
  m.gp0 = o; o += 32;
  m.gu = o; o += 32;
  m.red = o; o += 16;
  m.pf = o; o += 3 * pad4(L);
  m.meta = o; o += pad4(L) * 8;   // per latent dim: prior-net offsets (ints), see setup
  // everything above depends on (T, S, C, L, Q, method, nthreads) only: compile-time offsets in the shape-specialised instantiations
  m.auxh = o; o += naux * 32;   // label heads scored in the main loss only
  m.auxd = o; o += naux * 32;
  m.auxgo = o; o += pad4(naux * 12);
  m.par = o; o += pad4(npar);      // [priors | init net | dynamics | heads]: the gradient of every element goes straight to the slab
  m.total = o;
  return m;
}

__host__ __device__ constexpr int ode_threads_for(int T, int Q, int C, int S) {
  // waves >= 1 carry the head-gradient role (one (q,c,s) entry per thread) next to the adjoint scan on wave 0
  const int nt = ((T + 63) / 64) * 64, need = 64 + ((Q * C * S + 63) / 64) * 64;
  return nt < need ? need : nt;
}

// Register budget = 512 / (waves per SIMD the declared block size forces).  Loop-free forms fit 128 (S = 5) / 168-256 (S = 8, short
// grids) without spilling.  The persistent-loop forms hoist kernel-argument loads and need more: the specialised ones declare their
// exact block size, the generic ones cap the grid length they accept (512 threads) -- NO instantiation may spill a VGPR
// (tools/check_spills.py).
__host__ __device__ constexpr int ode_max_threads(int S, int T_, int C_, int Q_, bool one, bool bwd) {
  if (!one && bwd) return T_ > 0 ? ode_threads_for(T_, Q_, C_, S) : 512;
  return (S > 5 || (T_ > 0 && T_ <= 128)) ? 768 : 1024;
}

__host__ __device__ constexpr int ode_block_bound(int S, int T_, int C_, int Q_, bool one, bool bwd, int pk) {
  return pk > 1 ? pk * ode_threads_for(T_ ? T_ : 1, Q_ ? Q_ : 1, C_ ? C_ : 1, S) : ode_max_threads(S, T_, C_, Q_, one, bwd);
}

}  // namespace
