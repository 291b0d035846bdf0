"""CPU tests of the cohort moments (slode_cohort_moments and slode_cohort_plan): the header and the exports, the plan against a hand count
of the LDS pieces and of the scratch, the default-chunk rule, the refusal ladder on a hand-filled handle
(tests/cohort_refusals/cohort_refusals.cpp), the numpy restatement of the accumulation against fp64 at the accumulation bounds of
tests/cohort_util.py, the restated guards, and the model-level calls on an engine double."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

from tests import cohort_util as CU
from tests import lds_util as LU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 160 * 1024


# ---- header and exports --------------------------------------------------------------------------------------------------------------
def test_header_version_and_exports():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    version = int(re.search(r"#define SLODE_VERSION (\d+)", hdr).group(1))
    lib = L.load()
    assert version == lib.slode_version() >= 190
    assert "0.1.9" in hdr and re.search(r"#define SLODE_COHORT_MAX_G 1024\b", hdr) and L.COHORT_MAX_G == 1024
    assert re.search(r"#define SLODE_COHORT_MAX_CHUNK 64\b", hdr) and L.COHORT_MAX_CHUNK == 64
    for name in ("slode_cohort_plan", "slode_cohort_moments"):
        assert hasattr(lib, name) and name in L.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr), name
    for kernel in ("cohort_plan", "cohort_moments", "cohort_merge"):                     # the name list of slode_profile_read
        assert "\"%s\"" % kernel in hdr


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
    """Floats of every LDS piece of cohort_moments_kernel, from the issue's map (FwdLds + 6 Q C T + C T + loc / scale): each rounded up
    to 4 floats."""
    Q = 1 if s.likelihood == 1 else 3
    fwd = LU.fwd_shared_pieces(s.T, s.S, s.C, s.L, s.H, s.n_u, s.likelihood == 1)
    return fwd + [LU.r4(n) for n in (6 * Q * s.C * s.T, s.C * s.T, s.L, s.L)]


def _hand_scratch(s, M, G, R):
    """(n_partials, bytes): cs [G + 1] ints, the chunk table [n_partials][4] ints, the flags [n_partials] ints, each padded to 16 B, then
    n_partials partials of (5 Q C + C) T floats."""
    Q = 1 if s.likelihood == 1 else 3
    pad = LU.r4
    NP = -(-M // R) + G
    return NP, 4 * (pad(G + 1) + 4 * NP + pad(NP) + NP * pad((5 * Q * s.C + s.C) * s.T))


def _plan(s, M, G, ns=7, chunk=0):
    from structured_latent_odes_amd import _lib as L
    lib = L.load()
    r, n, lds, scr = C.c_int(-1), C.c_int(-1), C.c_size_t(0), C.c_size_t(0)
    rc = lib.slode_cohort_plan(C.byref(s), M, G, ns, chunk, C.byref(r), C.byref(n), C.byref(lds), C.byref(scr))
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
    if not proc:                                                                          # the metric shape once in numbers: about 57 KB
        assert _pieces(s) == [996, 996, 300, 400, 52, 132, 48, 12, 8, 4, 28, 8, 10800, 600, 8, 8] and lds == 57600
        assert _hand_scratch(s, 25600, 4, 32) == (804, 4 * (8 + 4 * 804 + 804 + 804 * 9600))
    # T = 300, C = 4, Q = 3: about 110 KB, taken; T = 1024 with three heads: refused by name
    mid = _shape(T=300, C=4)
    assert _plan(mid, 10, 2)[3] == 4 * sum(_pieces(mid)) and 105_000 < 4 * sum(_pieces(mid)) < 115_000
    rc, *_, why = _plan(_shape(T=1024), 10, 2)
    assert rc == -1 and "LDS tables of T = 1024" in why and str(4 * sum(_pieces(_shape(T=1024)))) in why


def test_default_chunk_is_a_function_of_M_alone():
    """The smallest power of two <= 64 with ceil(M / R) <= 1024."""
    s = _shape()
    for M, R in ((0, 1), (1, 1), (1024, 1), (1025, 2), (2048, 2), (2049, 4), (65536, 64), (65537, 64), (10 ** 6, 64)):
        for G in (1, 17, 1024):
            rc, r, n, _, _, _ = _plan(s, M, G)
            assert (rc, r, n) == (0, R, -(-M // R) + G), (M, G)
    assert _plan(_shape(True), 65536, 4)[1] == 64                                         # not of the shape either


def test_plan_refuses_by_name():
    s = _shape(B=100)
    for kw, word in ((dict(M=-1), "M = -1"), (dict(M=101), "M = 101"), (dict(G=0), "G = 0"), (dict(G=1025), "G = 1025"), (dict(chunk=-1), "chunk = -1"),
                     (dict(chunk=65), "chunk = 65"), (dict(ns=0), "num_samples = 0")):
        a = dict(M=10, G=2, ns=3, chunk=0)
        a.update(kw)
        rc, *_, why = _plan(s, a["M"], a["G"], a["ns"], a["chunk"])
        assert rc == -1 and word in why and "slode_cohort_plan" in why, (kw, why)


# ---- the refusal ladder ----------------------------------------------------------------------------------------------------------------
# case -> (status, words the message must carry), written from include/slode.h: the ladder of slode_recon_moments for the same is_post
# first (the call's name in place of its own), then members / offsets, M, G, chunk, mean, the observations obs_mean / l1 need, scratch,
# the LDS tables, scratch_bytes (SLODE_ENOSPC = -3), the label tensors, the workspace (-3)
_EINVAL, _ENOSPC = -1, -3
LADDER = {
    "handle NULL": (_EINVAL, ["handle is NULL"]), "shape NULL": (_EINVAL, ["shape is NULL"]), "layout NULL": (_EINVAL, ["layout is NULL"]),
    "params NULL": (_EINVAL, ["params is NULL"]), "batch NULL": (_EINVAL, ["slode_cohort_moments", "batch", "is NULL"]),
    "times NULL": (_EINVAL, ["slode_cohort_moments", "times", "is NULL"]), "stage_t NULL": (_EINVAL, ["slode_cohort_moments", "stage_t", "is NULL"]),
    "workspace NULL": (_EINVAL, ["slode_cohort_moments", "workspace", "is NULL"]), "bad shape": (_EINVAL, ["T out of range"]),
    "draws 0": (_EINVAL, ["slode_cohort_moments", "num_samples = 0"]), "draws 2^30": (_EINVAL, ["B x num_samples", "2^30 - 1"]),
    "adaptive method 3": (_EINVAL, ["adaptive solver dopri5"]), "adaptive method 4": (_EINVAL, ["adaptive solver bosh3"]),
    "adaptive method 5": (_EINVAL, ["adaptive solver fehlberg2"]), "adaptive method 6": (_EINVAL, ["adaptive solver adaptive_heun"]),
    "particles 2": (_EINVAL, ["particles = 2"]), "fold_on": (_EINVAL, ["measured arms"]), "ode_pack": (_EINVAL, ["measured arms"]),
    "ode_alg": (_EINVAL, ["measured arms"]),
    "post: obs NULL": (_EINVAL, ["posterior needs observations"]), "post: padded strides": (_EINVAL, ["observation strides (266, 1, 3)", "folded encoder"]),
    "post: no_fold": (_EINVAL, ["SLODE_NO_FOLD"]),
    "members NULL": (_EINVAL, ["members / offsets is NULL", "M = 3"]), "offsets NULL": (_EINVAL, ["members / offsets is NULL", "M = 3"]),
    "M -1": (_EINVAL, ["M = -1", "[0, B = 4]"]), "M B + 1": (_EINVAL, ["M = 5", "[0, B = 4]"]), "G 0": (_EINVAL, ["G = 0", "[1, 1024]"]),
    "G 1025": (_EINVAL, ["G = 1025", "[1, 1024]"]), "chunk -1": (_EINVAL, ["chunk = -1", "[0, 64]"]), "chunk 65": (_EINVAL, ["chunk = 65", "[0, 64]"]),
    "mean NULL": (_EINVAL, ["mean is NULL"]),
    "prior: obs_mean without observations": (_EINVAL, ["obs_mean / l1 need observations"]),
    "prior: l1 without observations": (_EINVAL, ["obs_mean / l1 need observations"]),
    "prior: obs_mean with padded strides": (_EINVAL, ["observation strides (266, 1, 3)", "obs_mean / l1 need dense"]),
    "prior: l1 with strides of another T": (_EINVAL, ["observation strides (258, 87, 1)", "obs_mean / l1 need dense"]),
    "scratch NULL": (_EINVAL, ["scratch is NULL"]), "scratch misaligned": (_EINVAL, ["scratch", "16-byte aligned"]),
    "T 1024: the LDS tables": (_EINVAL, ["LDS tables of T = 1024", "exceed the budget of 163840 B"]),
    "scratch too small": (_ENOSPC, ["scratch_bytes 64 B", "required 82688 B"]),        # M 3, G 2, R 1: 5 partials of 48 x 86 floats + 128 B of tables
    "label columns 3, n_u 2": (_EINVAL, ["3 columns", "n_u is 2"]), "prior without labels": (_EINVAL, ["prior needs the label tensors"]),
    "workspace too small": (_ENOSPC, ["workspace 64 B"]),
    # two conditions at once: the earlier rung speaks; a slode_recon_moments refusal before a cohort-only one
    "adaptive + G 0": (_EINVAL, ["adaptive solver dopri5"]), "draws 0 + mean NULL": (_EINVAL, ["num_samples = 0"]),
    "particles 2 + chunk 65": (_EINVAL, ["particles = 2"]), "post: padded strides + members NULL": (_EINVAL, ["observation strides"]),
    "members NULL + M -1": (_EINVAL, ["M = -1"]), "M 5 + G 0": (_EINVAL, ["M = 5"]), "G 0 + chunk 65": (_EINVAL, ["G = 0"]),
    "chunk 65 + mean NULL": (_EINVAL, ["chunk = 65"]), "scratch too small + workspace too small": (_ENOSPC, ["scratch_bytes"]),
    "M 0 with NULL lists, scratch too small": (_ENOSPC, ["scratch_bytes 0 B", "required 33088 B"]),   # 2 partials + 64 B of tables
}


def test_cohort_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_cohort_moments, posterior and prior, without a device: status, the words of the message and
    the untouched drawing-call counter against LADDER; and line by line -- status, counter and the full message, which check speaks first
    when two conditions hold included -- against tests/golden/cohort_refusals.txt, recorded from the library before the draw-walking calls
    shared one host tail."""
    from tests.refusals_util import refusal_lines
    lines = refusal_lines("cohort_refusals", tmp_path)
    assert len(lines) > 90
    want = open(os.path.join(ROOT, "tests", "golden", "cohort_refusals.txt")).read().splitlines()
    for i, (g, w) in enumerate(zip(lines, want)):
        assert g == w, "line %d:\n  got  %s\n  want %s" % (i + 1, g, w)
    assert len(lines) == len(want)
    seen = set()
    for line in lines:
        name, status, counter, msg = line.split(" | ", 3)
        key = name if name in LADDER else name.split(": ", 1)[1]
        want_status, words = LADDER[key]
        seen.add(key)
        assert int(status) == want_status and counter == "7", line                        # refused, and nothing drawn
        for w in words:
            assert w in msg, (name, w, msg)
    assert seen == set(LADDER)


# ---- numerics: the restatement of M6' + merge against fp64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,R", [(13, 7, 1), (13, 7, 2), (13, 7, 3), (13, 7, 64), (13, 1, 1), (13, 1, 2), (13, 1, 3), (13, 1, 64), (64, 20, 64), (7, 1, 2)])
def test_restated_accumulation_meets_the_bounds_where_a_plain_sum_of_squares_fails(n, K, R):
    """Thin bands (sd 1e-4 of the level): fp32 chunk partials + the fp64 Chan merge against fp64 at CU.accumulation_bars; the unshifted
    form (sums of v and v^2) misses the sd bound on the same inputs."""
    vals = CU.thin_band(n, K)
    mean64, sd64, sdb64 = CU.moments64(vals)
    D = CU.chunk_spread(vals.astype(np.float64), R)
    assert np.all(D <= CU.SPREAD * sd64) and (sd64 > 0).mean() > 0.9 and float(np.median(sd64 / np.abs(mean64))) < 1e-3
    bm, bs, bb = CU.accumulation_bars(mean64, sd64, sdb64, D, R, K)
    mean, sd, sdb = CU.cohort_scheme_f32(vals, R)
    rm, rs, rb = np.abs(mean - mean64) / bm, np.abs(sd - sd64) / bs, np.abs(sdb - sdb64) / bb
    plain = np.abs(CU.cohort_scheme_f32(vals, R, CU.chunk_partial_plain_f32)[1] - sd64) / bs
    print("n=%d K=%d R=%d: error / bound: mean %.3f, sd %.3f, sd_subjects %.3f; relative sd error %.1e; a plain sum of squares: %.1f (median %.1f)"
          % (n, K, R, rm.max(), rs.max(), rb.max(), (np.abs(sd - sd64) / sd64).max(), plain.max(), np.median(plain)))
    assert rm.max() <= 1.0 and rs.max() <= 1.0 and rb.max() <= 1.0
    if R * K > 1:                                                                         # (a partial of ONE value is exact in either form)
        assert np.median(plain) > 1.0                                                     # the case tells the two forms apart
    if K == 1:
        assert np.array_equal(sd, sdb)


def test_singletons_and_single_values():
    """One member per cohort: sd_subjects is exactly 0 and (mean, sd) are the member's own moments; one value: both sds exactly 0."""
    vals = CU.thin_band(1, 9)
    mean, sd, sdb = CU.cohort_scheme_f32(vals, 3)
    assert float(np.abs(sdb).max()) == 0.0
    m64, s64, _ = CU.moments64(vals)
    assert np.all(np.abs(mean - m64) <= 2 * CU.U * np.abs(m64) + 10 * CU.U * s64) and np.all(np.abs(sd - s64) <= 1e-3 * s64)
    mean, sd, sdb = CU.cohort_scheme_f32(vals[:, :1], 1)
    assert np.array_equal(mean, vals[0, 0]) and float(np.abs(sd).max()) == 0.0 and float(np.abs(sdb).max()) == 0.0


def _restated_call(vals, members, offsets, B, R, clip=-np.inf):
    """The guards of the kernels restated: offsets clamped to [0, M] (a decreasing pair: empty), positions clamped to [0, M), a member
    index outside [0, B) never used as an index -- it flags its chunk, and the merge turns its cohort into NaN; the clip by comparison.
    vals [B, K, ...]; returns mean [G, ...]."""
    M, G = len(members), len(offsets) - 1
    out = []
    for g in range(G):
        lo, hi = (min(max(int(o), 0), M) for o in offsets[g:g + 2])
        n, bad, partials = max(hi - lo, 0), False, []
        for first in range(lo, lo + n, R):
            rows = []
            for pos in range(first, min(first + R, lo + n)):
                b = int(members[min(max(pos, 0), M - 1)])
                if b < 0 or b >= B:
                    bad = True
                    continue
                v = vals[b].copy()
                v[v < clip] = clip                                                          # a comparison: NaN stays NaN
                rows.append(v)
            if rows:
                partials.append(CU.chunk_partial_f32(np.stack(rows)))
        out.append(np.full(vals.shape[2:], np.nan, np.float32) if bad or not n else CU.merge64(partials, vals.shape[1])[0])
    return np.stack(out)


def test_restated_guards():
    vals = CU.thin_band(9, 2, shape=(4,))
    members, offsets = CU.member_lists([0, 1, 1, 2, 0, -1, 2, 2, 1], 3)
    good = _restated_call(vals, members, offsets, 9, 2)
    assert np.isfinite(good).all()
    for bad_index in (-1, 9, 1 << 30):                                                    # a bad member: NaN for its cohort only
        m = members.copy()
        m[3] = bad_index                                                                  # position 3: cohort 1
        got = _restated_call(vals, m, offsets, 9, 2)
        assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], good[[0, 2]])
    # offsets beyond M or decreasing: nothing out of bounds, the cohort is clamped or empty
    got = _restated_call(vals, members, np.array([0, 2, 1 << 30, 5]), 9, 2)
    assert np.array_equal(got[0], good[0]) and np.isfinite(got[1]).all() and np.isnan(got[2]).all()
    # the clip keeps NaN and replaces what lies below it
    v = vals.copy()
    v[0, 0, 0] = np.nan
    got = _restated_call(v, members, offsets, 9, 2, clip=1.5)
    assert np.isnan(got[0, 0]) and np.isfinite(got[0, 1:]).all() and np.all(got[np.isfinite(got)] >= 1.5)


# ---- model level, on an engine double ----------------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self, refuse, Q):
        self.refuse, self.Q, self.fused, self.batches, self.draws, self.calls = refuse, Q, 0, [], [], []

    def draw_normal(self, rows):
        self.draws.append(rows)
        return torch.arange(rows * 4, dtype=torch.float32).view(rows, 4)

    def make_batch(self, obs, labels, eps=None, particles=1):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def cohort_moments(self, flat, bt, B, is_post, num_samples, members, offsets, G, chunk=0, clip_min=None):
        from structured_latent_odes_amd import _lib as L
        self.fused += 1
        self.calls.append((B, bool(is_post), num_samples, members.tolist(), offsets.tolist(), G, chunk, clip_min, members.dtype, offsets.dtype))
        if self.refuse:
            err = L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        q = torch.arange(self.Q, dtype=torch.float32).view(self.Q, 1, 1, 1)
        z = torch.zeros(self.Q, G, 3, 10)
        return q + z, 10 + q + z, 20 + q + z, torch.zeros(G, 3, 10), torch.ones(G, 3)


def _double(gauss, refuse, labels=("iext",)):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        LABELS, GAUSS = labels, gauss

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3), "flat": torch.zeros(1)})()
            self.sample_calls = []

        def _bind(self):
            return self._b

        def recon_samples(self, observations, is_post, num_samples, eps=None, **labels):
            """[B, C, T, ns] curves from the observations' first value and the noise: different per row, draw, channel and curve."""
            B = observations.shape[0]
            self.sample_calls.append((B, bool(is_post), num_samples, None if eps is None else tuple(eps.shape)))
            base = observations[:, :, :, None] * 0.5 + eps[:, :, 0].t().reshape(B, 1, 1, num_samples) * torch.arange(1.0, 4.0).view(1, 3, 1, 1)
            names = ("mean",) if gauss else ("mu_75", "mu_50", "mu_25")
            return dict({n: base - 1.0 + 0.25 * i for i, n in enumerate(names)}, z=None)

    return M()


def test_cohort_index_on_cvs_and_proc_labels():
    m = _double(False, 0, labels=("iext", "rtpr"))
    iext = torch.tensor([0.0, 1.0, 0.0, 1.0, 1.0, 0.0]).view(6, 1)
    rtpr = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.0, 0.0]).view(6, 1)
    ids, keys = m.cohort_index(iext=iext, rtpr=rtpr)
    assert ids.dtype == torch.int64 and ids.tolist() == [0, 2, 1, 3, 2, 0] and keys.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    ids, keys = m.cohort_index(by=("rtpr",), iext=iext, rtpr=rtpr)
    assert ids.tolist() == [0, 0, 1, 1, 0, 0] and keys.tolist() == [[0.0], [1.0]]
    with pytest.raises(ValueError, match="rtpr"):
        m.cohort_index(iext=iext)
    # proc: (device one-hot, treatment columns): wide labels, rows compared as a whole
    p = _double(False, 0, labels=("aR", "aS", "C12", "C6"))
    aR = torch.eye(3)[[0, 1, 0, 2, 1]]
    aS = torch.eye(4)[[0, 0, 0, 1, 0]]
    c12, c6 = torch.tensor([0.5, 0.5, 0.5, 0.1, 0.25]).view(5, 1), torch.zeros(5, 1)
    ids, keys = p.cohort_index(aR=aR, aS=aS, C12=c12, C6=c6)
    assert tuple(keys.shape) == (4, 9) and ids[0] == ids[2] and len(set(ids.tolist())) == 4
    ids, keys = p.cohort_index(by=("aR", "aS"), aR=aR, aS=aS, C12=c12, C6=c6)
    assert tuple(keys.shape) == (3, 7) and ids[1] == ids[4]


def test_member_lists_negative_ids_and_empty_cohorts():
    m = _double(False, 0)
    obs, lab = torch.zeros(8, 3, 10), torch.zeros(8, 1)
    ids = torch.tensor([2, -1, 0, 2, 4, 0, -7, 2])
    res = m.cohort_moments(obs, True, 3, ids, chunk=5, clip_min=0.0, num_cohorts=6, iext=lab)
    call = m._b.engine.calls[0]
    assert call[:3] == (8, True, 3) and call[3] == [2, 5, 0, 3, 7, 4] and call[4] == [0, 2, 2, 5, 5, 6, 6] and call[5:8] == (6, 5, 0.0)
    assert call[8] == call[9] == torch.int32
    assert res["count"].tolist() == [2, 0, 3, 0, 1, 0] and res["keys"].reshape(-1).tolist() == list(range(6))
    assert set(res) == {"mu_50", "mu_75", "mu_25", "observations", "l1", "count", "keys"}
    for q, n in enumerate(("mu_50", "mu_75", "mu_25")):                                  # the engine's head order
        assert [float(x[0, 0, 0]) for x in res[n]] == [q, 10 + q, 20 + q] and all(tuple(x.shape) == (6, 3, 10) for x in res[n])
    assert m._b.engine.batches == [((8, 3, 10), 1, None, 3)] and m.sample_calls == []
    assert m.cohort_moments(obs, True, 3, ids, iext=lab)["count"].tolist() == [2, 0, 3, 0, 1]      # G = max id + 1
    with pytest.raises(ValueError, match="num_samples"):
        m.cohort_moments(obs, True, 0, ids, iext=lab)
    with pytest.raises(ValueError, match="beyond num_cohorts"):
        m.cohort_moments(obs, True, 2, ids, num_cohorts=3, iext=lab)
    with pytest.raises(ValueError, match="no cohort"):
        m.cohort_moments(obs, True, 2, torch.full((8,), -1), iext=lab)
    # label names: cohort_index
    res = m.cohort_moments(obs, False, 2, ("iext",), iext=torch.tensor([1.0, 0, 0, 1, 1, 1, 0, 1]).view(8, 1))
    assert res["keys"].tolist() == [[0.0], [1.0]] and m._b.engine.calls[-1][3:5] == ([1, 2, 6, 0, 3, 4, 5, 7], [0, 3, 8])


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.cohort_moments(torch.zeros(2, 3, 10), True, 5, torch.tensor([0, 1]), iext=torch.zeros(2, 1))
    assert m.sample_calls == [] and m._b.engine.draws == []


@pytest.mark.parametrize("gauss", [False, True])
@pytest.mark.parametrize("K", [1, 3])
def test_composed_dict_equals_the_notebook_arithmetic(gauss, K, monkeypatch):
    """A refusal: the dict is reduced from recon_samples in chunks of rows -- equal to np.mean / np.std(..., 0) / the L1 written out here,
    for K = 1 (the notebooks' np.std(data[loc], 0)) and K = 3; the chunking does not change it; clip_min acts on the samples."""
    g = torch.Generator().manual_seed(4)
    B = 9
    obs = torch.rand(B, 3, 10, generator=g) + 1.0
    eps = torch.randn(K, B, 4, generator=g)
    lab = torch.zeros(B, 1)
    ids = torch.tensor([1, 0, 1, 3, -1, 1, 0, 3, 1])
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    for clip in (None, 0.0):
        results = []
        for chunk_rows in (2 * K, 4 * K, 1 << 16):
            m = _double(gauss, refuse=-1)
            monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", chunk_rows)
            results.append(m.cohort_moments(obs, True, K, ids, eps=eps, clip_min=clip, num_cohorts=5, iext=lab))
            rows = max(1, chunk_rows // K)
            assert m._b.engine.fused == 1 and [c[0] for c in m.sample_calls] == [min(rows, B - lo) for lo in range(0, B, rows)]
        samples = _double(gauss, 0).recon_samples(obs, True, K, eps=eps, iext=lab)
        res = results[0]
        assert res["count"].tolist() == [2, 4, 0, 2, 0]
        for r in results[1:]:
            for n in names:
                assert all(torch.allclose(a, b, rtol=1e-6, atol=0, equal_nan=True) for a, b in zip(r[n], res[n]))
        for g_ in range(5):
            loc = np.flatnonzero(ids.numpy() == g_)
            if not loc.size:
                assert all(torch.isnan(x[g_]).all() for n in names for x in res[n]) and torch.isnan(res["observations"][g_]).all() and torch.isnan(res["l1"][g_]).all()
                continue
            mean_y = np.mean(obs.numpy().astype(np.float64)[loc], 0)
            assert np.allclose(res["observations"][g_].numpy(), mean_y, rtol=1e-6)
            for n in names:
                data = samples[n].numpy().astype(np.float64)                               # [B, C, T, K]
                if clip is not None:
                    data[data < clip] = clip
                sel = data[loc]
                assert np.allclose(res[n][0][g_].numpy(), np.mean(np.mean(sel, 3), 0), rtol=1e-6, atol=1e-7)
                assert np.allclose(res[n][1][g_].numpy(), np.std(np.moveaxis(sel, 3, 1).reshape(-1, 3, 10), 0), rtol=1e-5, atol=1e-6)
                assert np.allclose(res[n][2][g_].numpy(), np.std(np.mean(sel, 3), 0), rtol=1e-5, atol=1e-6)
                if K == 1:
                    assert np.allclose(res[n][2][g_].numpy(), np.std(sel[..., 0], 0), rtol=1e-5, atol=1e-6) and torch.allclose(res[n][1][g_], res[n][2][g_], rtol=1e-5, atol=1e-6)
            d0 = samples[names[0]].numpy().astype(np.float64)
            if clip is not None:
                d0[d0 < clip] = clip
            mean_mu = np.mean(np.mean(d0[loc], 3), 0)
            assert np.allclose(res["l1"][g_].numpy(), np.sum(np.abs(mean_y - mean_mu), -1), rtol=1e-5)
    # no eps: ONE drawing call of K * B rows for the whole batch
    m = _double(gauss, refuse=-1)
    m.cohort_moments(obs, False, K, ids, iext=lab)
    assert m._b.engine.draws == [K * B]


def test_save_cohort_moments_file_names(tmp_path):
    m = _double(False, refuse=0)
    obs, ids = torch.zeros(4, 3, 10), torch.tensor([0, 1, 1, 0])
    files = m.save_cohort_moments(str(tmp_path / "r"), obs, True, 4, ids, iext=torch.zeros(4, 1))
    files += m.save_cohort_moments(str(tmp_path / "r"), obs, False, 4, ids, iext=torch.zeros(4, 1))
    want = sorted(["%s_%s_cohort_%s.npy" % (c, p, k) for c in ("mu_50", "mu_75", "mu_25") for p in ("post", "prior") for k in ("mean", "sd", "sd_subjects")]
                  + ["observations_cohort_mean.npy", "cohort_keys.npy", "cohort_count.npy", "l1_post_cohort.npy", "l1_prior_cohort.npy"])
    assert sorted(set(os.path.basename(f) for f in files)) == want == sorted(os.listdir(str(tmp_path / "r")))
    shapes = {"cohort_keys.npy": (2, 1), "cohort_count.npy": (2,), "l1_post_cohort.npy": (2, 3), "l1_prior_cohort.npy": (2, 3)}
    assert all(np.load(f).shape == shapes.get(os.path.basename(f), (2, 3, 10)) for f in files)
    assert float(np.load(str(tmp_path / "r" / "mu_75_post_cohort_sd_subjects.npy"))[0, 0, 0]) == 21.0


def test_engine_signatures():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.cohort_plan).parameters) == ["self", "B", "M", "G", "num_samples", "chunk"]
    assert list(inspect.signature(Engine.cohort_moments).parameters) == ["self", "params", "batch", "B", "is_post", "num_samples", "members", "offsets", "G",
                                                                        "chunk", "clip_min", "mean", "sd", "sd_subjects", "obs_mean", "l1", "outputs", "scratch"]


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_cohort_curves_flag_of_the_training_entry_points(fam, monkeypatch, tmp_path):
    """--cohort-curves reaches train() as cohort_curves=True from each entry point; without it train() gets what it gets today."""
    from structured_latent_odes_amd import training as TR
    tr = importlib.import_module("training_" + fam)
    seen = []
    monkeypatch.setattr(TR, "train", lambda config, family, a, b, n, **kw: seen.append((family, kw)))
    monkeypatch.chdir(tmp_path)
    assert TR.build_parser().parse_args([]).cohort_curves is False
    for argv in (["--epochs", "1"], ["--epochs", "1", "--cohort-curves"]):
        TR.main(tr.FAMILY, tr.load_config, tr.MechanisticModel, tr.MechanisticModelGauss, argv=argv)
    assert seen == [(fam, {"fused_stats": False}), (fam, {"fused_stats": False, "cohort_curves": True})]
