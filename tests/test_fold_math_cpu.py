"""CPU tests of csrc/fold_math.h, the one definition of the fold's arithmetic W_eff[m][kappa(c, t)] = sum_f sum_j lin[m][f][t - j] w'[f][c][j]
that the fold launch (weff_kernel: a register window of TW time points per quad) and the in-launch fold (enc_chain_kernel: one output per
quad) execute: both shapes compiled for the host (tests/fold_math/fold_math.cpp) and run on one random row of lin.weight per case.

* the windowed shape equals the single-output shape BIT FOR BIT for every TW in {1, 2, 4, 8}, and writes every kappa of the row -- on the
  row as it lies in memory (clamped index, select-zero: rows too long to stage) and on its zero-padded copy (the staged rows: a tap outside
  [0, n_pool) reads a zero of the copy; the copy lies between two rows of NaN, so a read beyond the row's own zeros shows);
* both agree with the fp64 sum to fp32 rounding.  The bound is the standard forward error of a recursive fp32 sum of products held in
  fused multiply-adds: an output is four lanes' values, each two chains (even / odd taps) of ceil(F / 4) * JM / 2 fused multiply-adds
  (one rounding each), joined by three additions -- n = ceil(F / 4) * JM / 2 + 3 roundings on the longest path, so
      |got - want| <= n * u / (1 - n * u) * sum_f sum_j |lin[m][f][t - j] * w'[f][c][j]|,        u = 2^-24
  (Higham, Accuracy and Stability of Numerical Algorithms, 3.1; the products are exact inside the fused multiply-adds).

Inputs are float32 values; lin ~ N(0, 1), w' ~ N(0, 1) (no structure that would hide a wrong tap: every product matters)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWS = (1, 2, 4, 8)
JM_SHORT, JM_LONG = 14, 24        # the two instantiations of the fold kernels: J = K + P - 1 <= 14 (every reference config), else the tap bound

CASES = {
    # name: (T, C, K, P, F, t_major)
    "metric_T200_C3": (200, 3, 10, 5, 10, 1),            # the metric encoder, kappa = t C + c
    "C4_c_major_T100": (100, 4, 10, 5, 10, 0),           # kappa = c T + t
    "T300_C4": (300, 4, 10, 5, 10, 1),
    "long_tap_T90_K12_P6": (90, 3, 12, 6, 4, 1),         # J = 17 > 14: the JM = 24 instantiation
    "long_tap_c_major_K16_P8": (61, 4, 16, 8, 5, 0),     # J = 23, the largest; F = 5 leaves the fourth lane of the quad without a filter
    "T23_n_pool_10": (23, 3, 10, 5, 10, 1),              # no TW > 1 divides T
    "T23_c_major": (23, 3, 10, 5, 10, 0),
    "T14_n_pool_1": (14, 3, 10, 5, 10, 1),               # T = K + P - 1: every tap index is clamped
    "T14_c_major_C4": (14, 4, 10, 5, 10, 0),
    "F10_split_3_3_3_1": (50, 3, 10, 5, 10, 1),          # (the metric filter count: the quad's lanes own 3 / 3 / 3 / 1 filters)
    "F16_K3_P2": (37, 4, 3, 2, 16, 0),                   # the filter bound: four filters per lane, one batch of reads; J = 4 << JM
}


def _case(name):
    """(request line, lin [F][n_pool], w' [F][C][J], JM) of one random row"""
    T, C, K, P, F, t_major = CASES[name]
    n_pool, J = T - K + 1 - P + 1, K + P - 1
    JM = JM_SHORT if J <= JM_SHORT else JM_LONG
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    lin = rng.normal(size=(F, n_pool)).astype(np.float32)
    wp = rng.normal(size=(F, C, J)).astype(np.float32)
    words = ["fold", str(JM), str(T), str(C), str(K), str(P), str(F), str(t_major)]
    words += ["%.9g" % x for x in lin.ravel()] + ["%.9g" % x for x in wp.ravel()]
    return " ".join(words), lin, wp, JM


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """the host program, built once and run once on every case: name -> uint32 [9][C * T] (single-output shape, then TW = 1, 2, 4, 8 on the
    row, then on its padded copy)"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present: the host program is not built")
    exe = str(tmp_path_factory.mktemp("fold_math") / "fold_math")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-O1", os.path.join(ROOT, "tests", "fold_math", "fold_math.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = list(CASES)
    r = subprocess.run([exe], input="\n".join(_case(n)[0] for n in names) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(names)
    out = {}
    for n, ln in zip(names, lines):
        T, C = CASES[n][0], CASES[n][1]
        out[n] = np.array([int(w, 16) for w in ln.split()], dtype=np.uint32).reshape(9, C * T)
    return out


def test_the_cases_reach_both_instantiations_and_the_edges():
    jm = {n: _case(n)[3] for n in CASES}
    assert set(jm.values()) == {JM_SHORT, JM_LONG} and jm["metric_T200_C3"] == JM_SHORT and jm["long_tap_T90_K12_P6"] == JM_LONG
    T, C, K, P, F, _ = CASES["T14_n_pool_1"]
    assert T == K + P - 1 and T - K + 1 - P + 1 == 1
    assert all(CASES["T23_n_pool_10"][0] % tw for tw in TWS if tw > 1) and 23 - 10 + 1 - 5 + 1 == 10
    assert {CASES[n][5] for n in CASES} == {0, 1}


@pytest.mark.parametrize("name", list(CASES))
def test_windowed_equals_single_output_bit_for_bit(rows, name):
    got = rows[name]
    assert not np.any(got == 0xFFFFFFFF), "a kappa of the row was not written (or a NaN pattern)"
    for i, tw in enumerate(TWS + TWS):
        bad = np.nonzero(got[1 + i] != got[0])[0]
        assert bad.size == 0, (name, "TW = %d" % tw, "padded" if i >= len(TWS) else "in place", bad[:8], got[0][bad[:8]], got[1 + i][bad[:8]])
    assert len(np.unique(got[0])) > got.shape[1] // 2                                      # (the outputs are not all one value)


@pytest.mark.parametrize("name", list(CASES))
def test_both_shapes_match_the_fp64_sum_to_fp32_rounding(rows, name):
    T, C, K, P, F, t_major = CASES[name]
    _, lin, wp, JM = _case(name)
    n_pool, J = T - K + 1 - P + 1, K + P - 1
    lin64, wp64 = lin.astype(np.float64), wp.astype(np.float64)
    want, mag = np.zeros(C * T), np.zeros(C * T)
    for c in range(C):
        for t in range(T):
            j = np.arange(J)
            j = j[(t - j >= 0) & (t - j < n_pool)]
            terms = lin64[:, t - j] * wp64[:, c, j]                                         # [F][taps in range]
            kap = t * C + c if t_major else c * T + t
            want[kap], mag[kap] = terms.sum(), np.abs(terms).sum()
    n = -(-F // 4) * (JM // 2) + 3
    u = 2.0 ** -24
    bound = n * u / (1 - n * u) * mag
    worst = 0.0
    for i in range(9):
        got = rows[name][i].view(np.float32).astype(np.float64)
        err = np.abs(got - want)
        worst = max(worst, (err / bound).max())
        assert np.all(err <= bound), (name, i, int(np.argmax(err / bound)), float((err / bound).max()))
    print("%s: worst error / bound %.3f (n = %d roundings)" % (name, worst, n))
