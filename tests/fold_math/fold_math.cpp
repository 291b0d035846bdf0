// csrc/fold_math.h -- the arithmetic of the fold W_eff[m][kappa(c, t)] = sum_f sum_j lin[m][f][t - j] * w'[f][c][j] as enc_chain_kernel (one
// output per quad) and weff_kernel (a window of FW time points per quad) execute it -- on the host, for tests/test_fold_math_cpu.py.
// Reads one request per line from standard input:
//   fold JM T C K P F t_major, then the F * n_pool values of one lin.weight row and the F * C * J values of w'
// and prints one line of 9 * C * T words for it: the bit patterns of the row of W_eff in memory order (kappa), first from
// fold_out_partial, then from fold_window_partial with FW = 1, 2, 4, 8 on the row as it is (clamped index, select-zero), then with FW = 1,
// 2, 4, 8 on its zero-padded copy (fold_padded_at, as weff_kernel stages it; the copy is the middle of three rows, the other two NaN, so
// that a read outside the row's own zeros shows) -- items as fold_item orders them, time points at or beyond T dropped; a kappa no item wrote
// prints as ffffffff.  The four lanes of a quad are run one after the other and meet in fold_quad_sum.
// No device, no HIP call.  Build (host pass only): hipcc -x hip --cuda-host-only -std=c++17 fold_math.cpp
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../structured_latent_odes_amd/csrc/fold_math.h"

static unsigned bits(float x) {
  unsigned u;
  memcpy(&u, &x, sizeof u);
  return u;
}

struct Shape { int T, C, F, n_pool, t_major; };

template <int JM>
static void single(const Shape& s, const float* lin, const float* wp, std::vector<unsigned>& out) {
  for (int c = 0; c < s.C; ++c)
    for (int t = 0; t < s.T; ++t) {
      float p[FOLD_WFG];
      for (int fh = 0; fh < FOLD_WFG; ++fh) p[fh] = fold_out_partial<JM>(s.F, s.C, s.n_pool, lin, wp, c, t, fh);
      out[fold_kappa(s.T, s.C, s.t_major, c, t)] = bits(fold_quad_sum(p));
    }
}

template <int JM, int FW, bool PADDED>
static void windowed(const Shape& s, const float* lin, const float* wp, std::vector<unsigned>& out) {
  const int n_it = s.C * fold_windows(s.T, FW);
  constexpr int PAD = fold_pad(JM, FW);
  // the padded copy of three rows: NaN, this row, NaN (the zeros between the filter rows are shared with the neighbours, as in the kernel)
  std::vector<float> copy(PADDED ? fold_padded_size(3, s.F, s.n_pool, PAD) : 0, 0.f);
  if (PADDED)
    for (int fr = 0; fr < 3 * s.F; ++fr)
      for (int q = 0; q < s.n_pool; ++q)
        copy[fold_padded_at(fr, q, s.n_pool, PAD)] = fr / s.F == 1 ? lin[(fr - s.F) * s.n_pool + q] : NAN;
  const float* wlm = PADDED ? copy.data() + fold_padded_at(s.F, 0, s.n_pool, PAD) : lin;
  const int stride = PADDED ? s.n_pool + PAD : s.n_pool;
  for (int it = 0; it < n_it; ++it) {
    int m, c, t0;
    fold_item(it, s.T, s.C, s.t_major, FW, m, c, t0);
    float r[FOLD_WFG][FW];
    for (int fh = 0; fh < FOLD_WFG; ++fh) fold_window_partial<JM, FW, fold_window_batch(JM), PADDED>(s.F, s.C, s.n_pool, stride, wlm, wp, c, t0, fh, r[fh]);
    for (int w = 0; w < FW; ++w) {
      const float p[FOLD_WFG] = {r[0][w], r[1][w], r[2][w], r[3][w]};
      if (m == 0 && t0 + w < s.T) out[fold_kappa(s.T, s.C, s.t_major, c, t0 + w)] = bits(fold_quad_sum(p));
    }
  }
}

template <int JM>
static void row(const Shape& s, const float* lin, const float* wp) {
  const int CT = s.C * s.T;
  std::vector<unsigned> out(9 * CT, 0xffffffffu), part(CT);
  for (int v = 0; v < 9; ++v) {
    part.assign(CT, 0xffffffffu);
    if (v == 0) single<JM>(s, lin, wp, part);
    else if (v == 1) windowed<JM, 1, false>(s, lin, wp, part);
    else if (v == 2) windowed<JM, 2, false>(s, lin, wp, part);
    else if (v == 3) windowed<JM, 4, false>(s, lin, wp, part);
    else if (v == 4) windowed<JM, 8, false>(s, lin, wp, part);
    else if (v == 5) windowed<JM, 1, true>(s, lin, wp, part);
    else if (v == 6) windowed<JM, 2, true>(s, lin, wp, part);
    else if (v == 7) windowed<JM, 4, true>(s, lin, wp, part);
    else windowed<JM, 8, true>(s, lin, wp, part);
    for (int i = 0; i < CT; ++i) out[v * CT + i] = part[i];
  }
  for (unsigned u : out) printf("%08x ", u);
  printf("\n");
}

int main() {
  char what[16];
  while (scanf("%15s", what) == 1) {
    int JM, K, P;
    Shape s;
    if (strcmp(what, "fold") || scanf("%d %d %d %d %d %d %d", &JM, &s.T, &s.C, &K, &P, &s.F, &s.t_major) != 7) return 1;
    const int J = K + P - 1;
    s.n_pool = s.T - K + 1 - P + 1;
    if (s.n_pool < 1 || J > JM || (JM != 14 && JM != 24) || s.C < 1 || s.F < 1) return 1;
    std::vector<float> lin((size_t)s.F * s.n_pool), wj((size_t)s.F * s.C * J), wp((size_t)s.F * s.C * JM, 0.f);
    for (float& x : lin)
      if (scanf("%f", &x) != 1) return 1;
    for (float& x : wj)
      if (scanf("%f", &x) != 1) return 1;
    for (int fc = 0; fc < s.F * s.C; ++fc)   // rows padded to JM, zero beyond J, as the kernels stage w'
      for (int j = 0; j < J; ++j) wp[(size_t)fc * JM + j] = wj[(size_t)fc * J + j];
    if (JM == 14) row<14>(s, lin.data(), wp.data());
    else row<24>(s, lin.data(), wp.data());
  }
  return 0;
}
