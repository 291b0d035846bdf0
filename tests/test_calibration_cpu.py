"""CPU tests of the calibration pass (slode_calibration and slode_calibration_plan): the header and the exports, the plan against a hand
count of the LDS pieces and of the scratch, the chunk rule, the refusal ladder on a hand-filled handle
(tests/calibration_refusals/calibration_refusals.cpp), the numpy restatement of the accumulation and the merge against fp64 at the bound of
tests/calibration_util.py, the integer outputs across chunk sizes, the nominal levels, the condition of the comparison rule on the fp64
oracle, and the model-level calls on an engine double."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

from tests import calibration_util as KU
from tests import eval_stats_util as EU
from tests import lds_util as LU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 160 * 1024


# ---- header and exports --------------------------------------------------------------------------------------------------------------
def test_header_version_and_exports():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    version = int(re.search(r"#define SLODE_VERSION (\d+)", hdr).group(1))
    lib = L.load()
    assert version == lib.slode_version() >= 200 and "0.2.0" in hdr
    for name in ("slode_calibration_plan", "slode_calibration"):
        assert hasattr(lib, name) and name in L.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr), name
    for kernel in ("calibration", "calibration_merge"):                                   # the name list of slode_profile_read
        assert "\"%s\"" % kernel in hdr
    phi = [float(re.search(r"#define SLODE_CALIBRATION_%s (\S+?)f\b" % n, hdr).group(1)) for n in ("PHI2", "PHIM2")]
    from math import erf, sqrt
    assert abs(phi[0] - 0.5 * (1 + erf(2 / sqrt(2)))) < 1e-15 and abs(phi[1] - 0.5 * (1 - erf(2 / sqrt(2)))) < 1e-15
    assert (L.CALIBRATION_PHI2, L.CALIBRATION_PHIM2) == tuple(phi) == (KU.PHI2, KU.PHIM2)


# ---- the plan, by hand count ---------------------------------------------------------------------------------------------------------
def _shape(proc=False, **kw):
    """The metric shape (cvs: S 5, C 3, three heads, L 8, H 25, T 200) or the proc shape (S 8, C 4, three heads, L 50, T 100)."""
    from structured_latent_odes_amd import _lib as L
    d = dict(B=1 << 20, T=200, C=3, L=8, S=5, H=25, F=10, K=10, P=5, Hc=50, n_u=2, n_groups=2, method=L.RK4, likelihood=L.ALD,
             quantile_diff=0.475, rtol=1e-7, atol=1e-9)
    if proc:
        d.update(T=100, C=4, L=50, S=8, n_u=9, n_groups=1)
    d.update(kw)
    s = L.Shape(**d)
    if proc:
        s.groups[0] = L.Group(0, 40, 0, 9)
    else:
        s.groups[0], s.groups[1] = L.Group(0, 3, 0, 1), L.Group(3, 3, 1, 1)
    return s


def _pieces(s):
    """Floats of every LDS piece of calibration_kernel (FwdLds, then the fp64 sums 2 x 4 C T, the counts 5 C T, the observations C T, the
    scale table C T for the Gauss likelihood, loc / scale): each rounded up to 4 floats."""
    gauss = s.likelihood == 1
    Q = 1 if gauss else 3
    fwd = LU.fwd_shared_pieces(s.T, s.S, s.C, s.L, s.H, s.n_u, s.likelihood == 1)
    CT = s.C * s.T
    return fwd + [LU.r4(n) for n in (8 * CT, 5 * CT, CT, CT if gauss else 0, s.L, s.L)]


def _hand_scratch(s, M, G, R):
    """(n_partials, bytes): cs [G + 1] ints, the chunk table [n_partials][4] ints, the flags [n_partials] ints, each padded to 16 B, then
    n_partials partials of 4 C T doubles + 5 C T ints, padded to 16 B."""
    pad = LU.r4
    NP = -(-M // R) + G
    return NP, 4 * (pad(G + 1) + 4 * NP + pad(NP)) + NP * ((52 * s.C * s.T + 15) & ~15)


def _plan(s, M, G, ns=7, chunk=0, name="slode_calibration_plan"):
    from structured_latent_odes_amd import _lib as L
    lib = L.load()
    r, n, lds, scr = C.c_int(-1), C.c_int(-1), C.c_size_t(0), C.c_size_t(0)
    rc = getattr(lib, name)(C.byref(s), M, G, ns, chunk, C.byref(r), C.byref(n), C.byref(lds), C.byref(scr))
    return rc, r.value, n.value, lds.value, scr.value, (lib.slode_last_error(None) or b"").decode()


@pytest.mark.parametrize("proc", [False, True])
def test_plan_matches_the_hand_count(proc):
    s = _shape(proc)
    lds = 4 * sum(_pieces(s))
    assert all(4 * n % 16 == 0 for n in _pieces(s)) and lds <= BUDGET
    for M, G, chunk in ((25600, 4, 0), (25600, 4, 8), (1024, 50, 0), (1024, 50, 1), (1000, 50, 64), (0, 3, 0), (7, 1024, 3)):
        R = chunk or {25600: 32, 1024: 1, 0: 1}[M]
        NP, nbytes = _hand_scratch(s, M, G, R)
        assert _plan(s, M, G, chunk=chunk)[:5] == (0, R, NP, lds, nbytes), (M, G, chunk)
    if not proc:                                                                          # the metric shape once in numbers: about 46 KB
        assert _pieces(s)[12:] == [4800, 3000, 600, 0, 8, 8] and lds == 4 * (2984 + 8416) == 45600
    g = _shape(proc, likelihood=1)                                                        # Gauss: one head row fewer, the scale table more
    assert _plan(g, 10, 2)[3] == 4 * sum(_pieces(g)) and _pieces(g)[15] == g.C * g.T
    # T = 300, C = 4: about 88 KB, taken; T = 1024: refused by name
    mid = _shape(T=300, C=4, likelihood=1)
    assert _plan(mid, 10, 2)[3] == 4 * sum(_pieces(mid)) and 85_000 < 4 * sum(_pieces(mid)) < 95_000
    rc, *_, why = _plan(_shape(T=1024), 10, 2)
    assert rc == -1 and "LDS tables of T = 1024" in why and str(4 * sum(_pieces(_shape(T=1024)))) in why


def test_chunk_rule_is_that_of_the_cohort_plan():
    """The smallest power of two <= 64 with ceil(M / R) <= 1024: a function of M alone, and the same as slode_cohort_plan's."""
    s = _shape()
    for M, R in ((0, 1), (1, 1), (1024, 1), (1025, 2), (2048, 2), (2049, 4), (65536, 64), (65537, 64), (10 ** 6, 64)):
        for G in (1, 17, 1024):
            rc, r, n, _, _, _ = _plan(s, M, G)
            assert (rc, r, n) == (0, R, -(-M // R) + G), (M, G)
            assert _plan(s, M, G, name="slode_cohort_plan")[1:3] == (r, n)
    assert _plan(_shape(True), 65536, 4)[1] == 64                                         # not of the shape either


def test_plan_refuses_by_name():
    s = _shape(B=100)
    for kw, word in ((dict(M=-1), "M = -1"), (dict(M=101), "M = 101"), (dict(G=0), "G = 0"), (dict(G=1025), "G = 1025"), (dict(chunk=-1), "chunk = -1"),
                     (dict(chunk=65), "chunk = 65"), (dict(ns=0), "num_samples = 0")):
        a = dict(M=10, G=2, ns=3, chunk=0)
        a.update(kw)
        rc, *_, why = _plan(s, a["M"], a["G"], a["ns"], a["chunk"])
        assert rc == -1 and word in why and "slode_calibration_plan" in why, (kw, why)


# ---- the refusal ladder ----------------------------------------------------------------------------------------------------------------
# case -> (status, words the message must carry), written from include/slode.h: the ladder of slode_cohort_moments for the same is_post
# (observations required on BOTH sides), then members / offsets, M, G, chunk, below, dense observations, scratch, the LDS tables,
# scratch_bytes (SLODE_ENOSPC = -3), the label tensors, the workspace (-3)
_EINVAL, _ENOSPC = -1, -3
_N = "slode_calibration"
LADDER = {
    "handle NULL": (_EINVAL, ["handle is NULL"]), "shape NULL": (_EINVAL, ["shape is NULL"]), "layout NULL": (_EINVAL, ["layout is NULL"]),
    "params NULL": (_EINVAL, ["params is NULL"]), "batch NULL": (_EINVAL, [_N, "batch", "is NULL"]), "times NULL": (_EINVAL, [_N, "times", "is NULL"]),
    "stage_t NULL": (_EINVAL, [_N, "stage_t", "is NULL"]), "workspace NULL": (_EINVAL, [_N, "workspace", "is NULL"]),
    "bad shape": (_EINVAL, ["T out of range"]), "draws 0": (_EINVAL, [_N, "num_samples = 0"]), "draws 2^30": (_EINVAL, ["B x num_samples", "2^30 - 1"]),
    "adaptive method 3": (_EINVAL, ["adaptive solver dopri5"]), "adaptive method 4": (_EINVAL, ["adaptive solver bosh3"]),
    "adaptive method 5": (_EINVAL, ["adaptive solver fehlberg2"]), "adaptive method 6": (_EINVAL, ["adaptive solver adaptive_heun"]),
    "particles 2": (_EINVAL, ["particles = 2"]), "fold_on": (_EINVAL, ["measured arms"]), "ode_pack": (_EINVAL, ["measured arms"]),
    "ode_alg": (_EINVAL, ["measured arms"]), "obs NULL": (_EINVAL, [_N, "batch->obs is NULL"]),
    "post: padded strides": (_EINVAL, ["observation strides (266, 1, 3)", "folded encoder"]), "post: no_fold": (_EINVAL, ["SLODE_NO_FOLD"]),
    "members NULL": (_EINVAL, ["members / offsets is NULL", "M = 3"]), "offsets NULL": (_EINVAL, ["members / offsets is NULL", "M = 3"]),
    "M -1": (_EINVAL, ["M = -1", "[0, B = 4]"]), "M B + 1": (_EINVAL, ["M = 5", "[0, B = 4]"]), "G 0": (_EINVAL, ["G = 0", "[1, 1024]"]),
    "G 1025": (_EINVAL, ["G = 1025", "[1, 1024]"]), "chunk -1": (_EINVAL, ["chunk = -1", "[0, 64]"]), "chunk 65": (_EINVAL, ["chunk = 65", "[0, 64]"]),
    "below NULL": (_EINVAL, ["below is NULL"]),
    "prior: padded strides": (_EINVAL, ["observation strides (266, 1, 3)", "comparisons need dense"]),
    "prior: strides of another T": (_EINVAL, ["observation strides (258, 87, 1)", "comparisons need dense"]),
    "scratch NULL": (_EINVAL, ["scratch is NULL"]), "scratch misaligned": (_EINVAL, ["scratch", "16-byte aligned"]),
    "T 1024: the LDS tables": (_EINVAL, ["LDS tables of T = 1024", "exceed the budget of 163840 B"]),
    "scratch too small": (_ENOSPC, ["scratch_bytes 64 B", "required 67248 B"]),        # M 3, G 2, R 1: 5 partials of 52 x 258 B (padded) + 128 B of tables
    "label columns 3, n_u 2": (_EINVAL, ["3 columns", "n_u is 2"]), "prior without labels": (_EINVAL, ["prior needs the label tensors"]),
    "workspace too small": (_ENOSPC, ["workspace 64 B"]),
    # two conditions at once: the earlier rung speaks
    "adaptive + G 0": (_EINVAL, ["adaptive solver dopri5"]), "draws 0 + below NULL": (_EINVAL, ["num_samples = 0"]),
    "measured arm + obs NULL": (_EINVAL, ["measured arms"]), "obs NULL + members NULL": (_EINVAL, ["batch->obs is NULL"]),
    "members NULL + M -1": (_EINVAL, ["M = -1"]), "M 5 + G 0": (_EINVAL, ["M = 5"]), "G 0 + chunk 65": (_EINVAL, ["G = 0"]),
    "chunk 65 + below NULL": (_EINVAL, ["chunk = 65"]), "prior: below NULL + padded strides": (_EINVAL, ["below is NULL"]),
    "scratch too small + workspace too small": (_ENOSPC, ["scratch_bytes"]),
    "M 0 with NULL lists and optional outputs, scratch too small": (_ENOSPC, ["scratch_bytes 0 B", "required 26912 B"]),   # 2 partials + 64 B
}


def test_calibration_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_calibration, posterior and prior, without a device, in rung order: status, the words of the
    message and the untouched drawing-call counter against LADDER; line by line against tests/golden/calibration_refusals.txt; and the
    memory that stands for the outputs untouched."""
    from tests.refusals_util import refusal_lines
    lines = refusal_lines("calibration_refusals", tmp_path)
    assert len(lines) > 90 and lines[-1] == "memory that stands for the outputs | untouched"
    want = open(os.path.join(ROOT, "tests", "golden", "calibration_refusals.txt")).read().splitlines()
    for i, (g, w) in enumerate(zip(lines, want)):
        assert g == w, "line %d:\n  got  %s\n  want %s" % (i + 1, g, w)
    assert len(lines) == len(want)
    seen = set()
    for line in lines[:-1]:
        name, status, counter, msg = line.split(" | ", 3)
        key = name if name in LADDER else name.split(": ", 1)[1]
        want_status, words = LADDER[key]
        seen.add(key)
        assert int(status) == want_status and counter == "7", line                        # refused, and nothing drawn
        for w in words:
            assert w in msg, (name, w, msg)
    assert seen == set(LADDER)


# ---- numerics: the restatement of M6'' + merge against fp64 ------------------------------------------------------------------------------
def _thin(n, K, C=3, T=11, rel=1e-4, up=1.0002, down=0.9998):
    """Observations and three curves from ONE thin band (CU.thin_band: sd ``rel`` of the level): v_1 scaled by ``up``, v_2 by ``down``, y a
    further value of the band.  The defaults: two sd apart -- every indicator has interior counts, and the curves cross now and then."""
    band = KU.thin_band(n, 3 * K + 1, (C, T), rel=rel)
    v = np.stack([band[:, :K], band[:, K:2 * K] * np.float32(up), band[:, 2 * K:3 * K] * np.float32(down)])
    return band[:, 3 * K].astype(np.float32), v.astype(np.float32)


def _truth(y, v, tau):
    """fp64 on the same fp32 inputs, tau as the kernel holds it: counts [5, C, T], means [4, C], mean |term| [4, C]."""
    t, _ = KU.tau32(tau)
    sm = KU.summands64(y[:, None], v, t.astype(np.float64))                               # y [n, 1, C, T], v [3, n, K, C, T] -> [4, n, K, C, T]
    return KU.indicators(y[:, None], v).sum((1, 2)), sm.mean((1, 2, 4)), np.abs(sm).mean((1, 2, 4))


def _ratios(y, v, tau, R, running=False):
    cnt64, mean64, mabs = _truth(y, v, tau)
    cnt, pin, wid = KU.scheme(y, v, tau, R, running)
    assert np.array_equal(cnt, cnt64) and cnt.dtype == np.int32                           # the counts are exact in either form
    return cnt, np.abs(np.concatenate([pin, wid[None]]).astype(np.float64) - mean64) / KU.accumulation_bar(mabs)


@pytest.mark.parametrize("n,K,R", [(13, 7, 1), (13, 7, 2), (13, 7, 3), (13, 7, 64), (13, 1, 1), (7, 1, 2), (64, 20, 64), (64, 20, 16)])
def test_restated_accumulation_meets_the_bound_where_one_fp32_running_sum_fails(n, K, R):
    """fp32 summands into fp64 slots, the fp64 merge and the fixed tree over t against fp64 at KU.accumulation_bar -- a bound without a
    factor in the number of terms -- on a band two sd wide around the observations and on a band that varies by a few ulp with the curves
    well apart.  On the second every addition of a running fp32 sum rounds the same way: the rejected form misses the bound several times
    over once a chunk holds 1280 terms."""
    tau = np.array([0.5, 0.975, 0.025])
    y, v = _thin(n, K)
    cnt, ratio = _ratios(y, v, tau, R)
    if n * K > 50:
        assert all(0 < cnt[i].sum() < cnt[i].size * n * K for i in range(5))              # every indicator fires somewhere, and not everywhere
    flat = _thin(n, K, rel=1e-6, up=1.25, down=0.75)
    _, ratio_flat = _ratios(*flat, tau, R)
    _, running = _ratios(*flat, tau, R, running=True)
    print("n=%d K=%d R=%d: error / bound %.3f, %.3f; one fp32 running sum: pinball 1, 2 and width %.1f .. %.1f"
          % (n, K, R, ratio.max(), ratio_flat.max(), running[1:].min(), running[1:].max()))
    assert ratio.max() <= 1.0 and ratio_flat.max() <= 1.0
    if min(R, n) * K >= 1024:
        assert running[1:].min() > 1.0                                                    # the case tells the two forms apart


def test_integer_outputs_do_not_depend_on_the_chunk_and_floats_agree_to_rounding():
    tau = np.array([0.5, 0.975, 0.025])
    y, v = _thin(13, 7)
    got = {R: KU.scheme(y, v, tau, R) for R in (1, 2, 64)}
    _, _, mabs = _truth(y, v, tau)
    for R in (2, 64):
        assert np.array_equal(got[R][0], got[1][0])
        d = np.abs(np.concatenate([got[R][1], got[R][2][None]]).astype(np.float64) - np.concatenate([got[1][1], got[1][2][None]]))
        assert np.all(d <= 2 * KU.accumulation_bar(mabs))


def test_tree_sum_is_the_merge_order():
    """t = i, i + 256, ... per thread, the shuffle-down tree per wave, ((w0 + w1) + w2) + w3: exact on integers, T below and above 256."""
    for T in (1, 63, 200, 256, 300, 1024):
        a = np.arange(1.0, T + 1.0)[None].repeat(2, 0)
        assert np.array_equal(KU.tree_sum_t(a), np.full(2, T * (T + 1) / 2))


def test_restated_guards_and_nan():
    """A NaN curve value compares false everywhere; an out-of-range member never indexes (the merge gives its cohort the empty value)."""
    y, v = _thin(3, 2)
    v[1, 0, 0, 0, 0] = np.nan
    ind = KU.indicators(y[0], v[:, 0, 0])
    assert not ind[1, 0, 0] and not ind[3, 0, 0] and not ind[4, 0, 0] and ind[0, 0, 0] == (y[0, 0, 0] < v[0, 0, 0, 0, 0])
    assert np.isnan(KU.summands_f32(y[0], v[:, 0, 0], np.array([0.5, 0.9, 0.1]))[[1, 3], 0, 0]).all()


# ---- nominal levels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_nominal_levels_per_family(fam):
    """ALD: 0.5, 0.5 +- quantile_diff from the config; Gauss: 0.5, Phi(2), Phi(-2)."""
    cfg = EU.model_config(fam)
    mod = importlib.import_module("structured_latent_odes_amd.models.mechanistic_" + fam)
    gauss = importlib.import_module("structured_latent_odes_amd.models.mechanistic_%s_Gauss" % fam).MechanisticModelGauss
    d = float(cfg.quantile_diff)
    for cls, want in ((mod.MechanisticModel, [0.5, 0.5 + d, 0.5 - d]), (gauss, [0.5, KU.PHI2, KU.PHIM2])):
        m = cls.__new__(cls)
        m.config = cfg
        got = cls.calibration_nominal(m)
        assert got.dtype == torch.float64 and got.tolist() == want
    cfg.update(quantile_diff=0.25)
    m = mod.MechanisticModel.__new__(mod.MechanisticModel)
    m.config = cfg
    assert mod.MechanisticModel.calibration_nominal(m).tolist() == [0.5, 0.75, 0.25]
    for case in EU.CASES:
        c = EU.build_case(case, ("eps", 1, 1), B=2)
        want = [0.5, KU.PHI2, KU.PHIM2] if c["ospec"].gauss else [0.5, 0.5 + c["ospec"].quantile_diff, 0.5 - c["ospec"].quantile_diff]
        assert KU.nominal(c["ospec"]).tolist() == want


# ---- the condition of the comparison rule, on the oracle alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EU.CASES))
def test_constructed_observations_give_interior_counts_and_few_near_points(case):
    """The constructed observations (prior, B = 9, ns = 7): head 0's fraction below lies in [0.2, 0.8] in every channel, the ALD cases
    cross somewhere, and the near points stay under NEAR_SHARE -- the rule excuses next to nothing."""
    c, y = KU.constructed_case(case)
    w = KU.oracle_calibration(c, False, np.zeros(9, np.int64), 1, obs=y)
    frac = w["counts"].sum(-1)[:, 0] / (9 * 7 * c["T"])
    print("%s: below %s cross %s near share %.2e" % (case, frac[0], frac[4], w["near_total"]))
    assert np.all((frac[0] >= 0.2) & (frac[0] <= 0.8)) and w["near_total"] <= KU.NEAR_SHARE
    assert (frac[4].max() == 0.0) if c["ospec"].gauss else (frac[4].min() > 0.0)
    assert np.all(w["counts"][3] <= w["counts"][1])                                       # inside is a subset of below v_1


# ---- model level, on an engine double ----------------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self, refuse):
        self.refuse, self.fused, self.batches, self.draws, self.calls = refuse, 0, [], [], []

    def draw_normal(self, rows):
        self.draws.append(rows)
        return torch.arange(rows * 4, dtype=torch.float32).view(rows, 4) % 7 - 3.0

    def make_batch(self, obs, labels, eps=None, particles=1):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def calibration(self, flat, bt, B, is_post, num_samples, members, offsets, G, chunk=0):
        from structured_latent_odes_amd import _lib as L
        self.fused += 1
        self.calls.append((B, bool(is_post), num_samples, members.tolist(), offsets.tolist(), G, chunk, members.dtype, offsets.dtype))
        if self.refuse:
            err = L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        n = (offsets[1:] - offsets[:-1]).to(torch.int32).view(1, G, 1, 1) * num_samples
        below = torch.arange(1, 4, dtype=torch.int32).view(3, 1, 1, 1) * n // 4 + torch.zeros(3, G, 3, 10, dtype=torch.int32)
        return below, below[1] - below[2], torch.zeros(G, 3, 10, dtype=torch.int32), torch.ones(3, G, 3), 2 * torch.ones(G, 3)


def _double(gauss, refuse, labels=("iext",)):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        LABELS, GAUSS = labels, gauss

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse), "flat": torch.zeros(1)})()
            self.config = type("Cfg", (), {"quantile_diff": 0.3})()
            self.decoder = type("D", (), {"constant_std": torch.linspace(-1.0, 1.0, 30).view(3, 10)})()
            self.sample_calls = []

        def _bind(self):
            return self._b

        def recon_samples(self, observations, is_post, num_samples, eps=None, **labels):
            """[B, C, T, ns] curves from the observations and the noise: different per row, draw, channel and curve; they cross."""
            B = observations.shape[0]
            self.sample_calls.append((B, bool(is_post), num_samples, None if eps is None else tuple(eps.shape)))
            base = observations[:, :, :, None] + 0.2 * eps[:, :, 0].t().reshape(B, 1, 1, num_samples) * torch.arange(1.0, 4.0).view(1, 3, 1, 1)
            names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
            shift = (0.0,) if gauss else (0.0, 0.12, -0.12)
            return dict({n: base + s + 0.1 * torch.sin(7.0 * base * (i + 1)) for i, (n, s) in enumerate(zip(names, shift))}, z=None)

    return M()


def test_fused_result_is_counts_over_count_times_draws():
    m = _double(False, 0)
    obs, lab = torch.zeros(8, 3, 10), torch.zeros(8, 1)
    res = m.calibration(obs, True, 4, iext=lab)                                           # default: one cohort, the whole batch
    call = m._b.engine.calls[0]
    assert call[:3] == (8, True, 4) and call[3] == list(range(8)) and call[4] == [0, 8] and call[5:7] == (1, 0) and call[7] == call[8] == torch.int32
    assert set(res) == {"nominal", "below", "below_t", "inside", "inside_t", "cross", "cross_t", "pinball", "width", "count", "keys", "counts"}
    assert res["nominal"].tolist() == [0.5, 0.8, 0.2] and res["count"].tolist() == [8]
    assert tuple(res["below"].shape) == (3, 1, 3) and tuple(res["below_t"].shape) == (3, 1, 3, 10) and tuple(res["inside"].shape) == (1, 3)
    assert res["below_t"][:, 0, 0, 0].tolist() == [0.25, 0.5, 0.75] and res["below"][:, 0, 0].tolist() == [0.25, 0.5, 0.75]
    assert res["counts"]["below"].dtype == torch.int32 and float(res["inside"][0, 0]) == -0.25 and float(res["cross"].abs().max()) == 0.0
    assert m.sample_calls == [] and m._b.engine.batches == [((8, 3, 10), 1, None, 4)]
    # ids with an empty cohort and an excluded trajectory; label names
    ids = torch.tensor([2, -1, 0, 2, 4, 0, -7, 2])
    res = m.calibration(obs, False, 3, cohorts=ids, chunk=5, num_cohorts=6, iext=lab)
    call = m._b.engine.calls[-1]
    assert call[3] == [2, 5, 0, 3, 7, 4] and call[4] == [0, 2, 2, 5, 5, 6, 6] and call[5:7] == (6, 5)
    assert res["count"].tolist() == [2, 0, 3, 0, 1, 0] and torch.isnan(res["below"][:, 1]).all() and torch.isnan(res["below_t"][:, 3]).all()
    res = m.calibration(obs, False, 2, cohorts=("iext",), iext=torch.tensor([1.0, 0, 0, 1, 1, 1, 0, 1]).view(8, 1))
    assert res["keys"].tolist() == [[0.0], [1.0]] and m._b.engine.calls[-1][3:5] == ([1, 2, 6, 0, 3, 4, 5, 7], [0, 3, 8])
    with pytest.raises(ValueError, match="num_samples"):
        m.calibration(obs, True, 0, iext=lab)


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.calibration(torch.zeros(2, 3, 10), True, 5, iext=torch.zeros(2, 1))
    assert m.sample_calls == [] and m._b.engine.draws == []


@pytest.mark.parametrize("gauss", [False, True])
@pytest.mark.parametrize("K", [1, 3])
def test_composed_dict_equals_the_hand_made_reduction(gauss, K, monkeypatch):
    """A refusal: the dict is reduced from recon_samples in chunks of rows -- the integer outputs exactly those of comparisons written out
    here, the float outputs to rounding; the chunking of the rows does not change the counts."""
    g = torch.Generator().manual_seed(4)
    B = 9
    obs = torch.rand(B, 3, 10, generator=g) + 1.0
    eps = torch.randn(K, B, 4, generator=g)
    lab = torch.zeros(B, 1)
    ids = torch.tensor([1, 0, 1, 3, -1, 1, 0, 3, 1])
    results = []
    for chunk_rows in (2 * K, 4 * K, 1 << 16):
        m = _double(gauss, refuse=-1)
        monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", chunk_rows)
        results.append(m.calibration(obs, True, K, cohorts=ids, eps=eps, num_cohorts=5, iext=lab))
        rows = max(1, chunk_rows // K)
        assert m._b.engine.fused == 1 and [c[0] for c in m.sample_calls] == [min(rows, B - lo) for lo in range(0, B, rows)]
    res = results[0]
    for r in results[1:]:
        assert all(torch.equal(r["counts"][n], res["counts"][n]) for n in ("below", "inside", "cross"))
        assert torch.allclose(r["pinball"], res["pinball"], rtol=1e-6, atol=0, equal_nan=True) and torch.allclose(r["width"], res["width"], rtol=1e-6, equal_nan=True)
    m = _double(gauss, 0)
    s = m.recon_samples(obs, True, K, eps=eps, iext=lab)
    if gauss:
        w = 2.0 * torch.nn.functional.softplus(m.decoder.constant_std)[None, :, :, None]
        v = [s["mean"], s["mean"] + w, s["mean"] - w]
    else:
        v = [s["mu_50"], s["mu_75"], s["mu_25"]]
    v = np.stack([x.numpy() for x in v])                                                  # [3, B, C, T, K] fp32
    y = obs.numpy()[..., None]
    tau = m.calibration_nominal().numpy()
    assert tau.tolist() == ([0.5, KU.PHI2, KU.PHIM2] if gauss else [0.5, 0.8, 0.2])
    assert res["count"].tolist() == [2, 4, 0, 2, 0]
    crossed = 0
    for g_ in range(5):
        loc = np.flatnonzero(ids.numpy() == g_)
        if not loc.size:
            assert all(int(res["counts"][n][..., g_, :, :].abs().max()) == 0 for n in ("below", "inside", "cross"))
            assert torch.isnan(res["pinball"][:, g_]).all() and torch.isnan(res["width"][g_]).all() and torch.isnan(res["below"][:, g_]).all()
            continue
        ind = KU.indicators(y[loc], v[:, loc]).sum((1, 4))                                # [5, C, T]
        assert np.array_equal(res["counts"]["below"][:, g_].numpy(), ind[:3]) and np.array_equal(res["counts"]["inside"][g_].numpy(), ind[3])
        assert np.array_equal(res["counts"]["cross"][g_].numpy(), ind[4])
        crossed += int(ind[4].sum())
        sm = KU.summands64(y[loc], v[:, loc], tau).mean((1, 3, 4))                        # [4, C]
        assert np.allclose(res["pinball"][:, g_].numpy(), sm[:3], rtol=1e-5) and np.allclose(res["width"][g_].numpy(), sm[3], rtol=1e-5)
        assert np.array_equal(res["below_t"][:, g_].numpy(), ind[:3] / (loc.size * K)) and np.allclose(res["below"][:, g_].numpy(), ind[:3].sum(-1) / (loc.size * K * 10))
        assert np.allclose(res["inside"][g_].numpy(), ind[3].sum(-1) / (loc.size * K * 10)) and np.array_equal(res["cross_t"][g_].numpy(), ind[4] / (loc.size * K))
    assert (crossed == 0) if gauss else (crossed > 0)
    # no eps: ONE drawing call of K * B rows for the whole batch
    m = _double(gauss, refuse=-1)
    m.calibration(obs, False, K, cohorts=ids, iext=lab)
    assert m._b.engine.draws == [K * B]


def test_save_calibration_pools_batches_exactly(tmp_path):
    """Two batches against their concatenation on the composed route: integer files exactly, float files to rounding; names and shapes."""
    g = torch.Generator().manual_seed(6)
    obs = torch.rand(10, 3, 10, generator=g) + 1.0
    lab = (torch.arange(10) % 2).float().view(10, 1)
    eps = torch.randn(3, 10, 4, generator=g)

    class M2(type(_double(False, -1))):
        def _noise(self, ns, B, e, device=None):                                         # the batches' own rows of one noise tensor
            return eps[:, self.lo:self.lo + B]
    parts = M2()
    parts.lo = 0

    def batches():
        for lo, hi in ((0, 6), (6, 10)):
            parts.lo = lo
            yield {"observations": obs[lo:hi], "iext": lab[lo:hi]}
    files, pooled = parts.save_calibration(str(tmp_path / "two"), batches(), True, 3, cohorts=("iext",))
    whole = M2()
    whole.lo = 0
    files1, one = whole.save_calibration(str(tmp_path / "one"), [{"observations": obs, "iext": lab}], True, 3, cohorts=("iext",))
    names = ["calibration_%s_post.npy" % n for n in ("below", "below_t", "inside", "cross", "pinball", "width")] + ["calibration_nominal.npy", "calibration_count.npy"]
    assert [os.path.basename(f) for f in files] == names and sorted(os.listdir(str(tmp_path / "two"))) == sorted(names)
    shapes = dict(zip(names, [(3, 2, 3), (3, 2, 3, 10), (2, 3), (2, 3), (3, 2, 3), (2, 3), (3,), (2,)]))
    for n in names:
        a, b = np.load(str(tmp_path / "two" / n)), np.load(str(tmp_path / "one" / n))
        assert a.shape == shapes[n], n
        if "pinball" in n or "width" in n:
            assert np.allclose(a, b, rtol=1e-6)
        else:
            assert np.array_equal(a, b), n
    for n in ("below", "inside", "cross"):
        assert pooled["counts"][n].dtype == np.int64 and np.array_equal(pooled["counts"][n], one["counts"][n])
    assert np.load(str(tmp_path / "two" / "calibration_count.npy")).tolist() == [5, 5]
    line = parts.calibration_line(pooled, "post")
    assert line.startswith("calibration_post: tau=0.5000:") and "band=" in line and "crossing=" in line and "pinball=(" in line


def test_engine_signatures():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.calibration_plan).parameters) == ["self", "B", "M", "G", "num_samples", "chunk"]
    assert list(inspect.signature(Engine.calibration).parameters) == ["self", "params", "batch", "B", "is_post", "num_samples", "members", "offsets", "G",
                                                                     "chunk", "below", "inside", "cross", "pinball", "width", "outputs", "scratch"]
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase
    assert list(inspect.signature(MechanisticBase.calibration).parameters) == ["self", "observations", "is_post", "num_samples", "cohorts", "eps", "chunk",
                                                                              "num_cohorts", "labels"]


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_calibration_flag_of_the_training_entry_points(fam, monkeypatch, tmp_path):
    """--calibration reaches train() as calibration=True from each entry point; without it train() gets what it gets today."""
    from structured_latent_odes_amd import training as TR
    tr = importlib.import_module("training_" + fam)
    import inspect
    assert inspect.signature(TR.train).parameters["calibration"].default is False
    seen = []
    monkeypatch.setattr(TR, "train", lambda config, family, a, b, n, **kw: seen.append((family, kw)))
    monkeypatch.chdir(tmp_path)
    assert TR.build_parser().parse_args([]).calibration is False
    for argv in (["--epochs", "1"], ["--epochs", "1", "--calibration"]):
        TR.main(tr.FAMILY, tr.load_config, tr.MechanisticModel, tr.MechanisticModelGauss, argv=argv)
    assert seen == [(fam, {"fused_stats": False}), (fam, {"fused_stats": False, "calibration": True})]
