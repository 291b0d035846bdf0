"""CPU tests of the sample quantiles: the C ABI of slode_recon_quantiles / slode_quantile_plan, the numpy restatement of the rank, depth and
selection rules against np.quantile, the plan's ladder against the restated rule, the refusal ladder on a hand-filled handle
(tests/quantile_refusals/quantile_refusals.cpp), and the Python layer on an engine double (the dict, the route switch, the files, the flags)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import draws_ladder_util as DL
from tests import lds_util as LU
from tests import quantile_util as QU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "is_post", "num_samples", "n_levels", "levels", "tile", "out", "workspace",
        "workspace_bytes", "stream"]
PLAN_ARGS = ["s", "num_samples", "n_levels", "levels", "tile", "tile_out", "sweeps", "depth_lo", "depth_hi", "lds_bytes"]


def _arg_names(hdr, name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    return [a.split()[-1].lstrip("*") for a in args], m


def test_abi_exports_recon_quantiles_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_recon_quantiles", "slode_quantile_plan"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 260 and "0.2.6" in hdr
    for earlier in ("0.2.5: slode_curve_summary", "0.2.4: slode_latent_attribution", "0.2.3: slode_pointwise_density", "0.1.5: slode_recon_moments"):
        assert earlier in hdr                                                             # the earlier version lines are kept
    names, m = _arg_names(hdr, "slode_recon_quantiles")
    assert names == ARGS and _arg_names(hdr, "slode_quantile_plan")[0] == PLAN_ARGS
    at = lib.slode_recon_quantiles.argtypes
    assert len(at) == len(ARGS) and all(at[i] is C.c_int for i in (7, 8, 9, 11)) and at[14] is C.c_size_t
    assert len(lib.slode_quantile_plan.argtypes) == len(PLAN_ARGS)
    assert int(re.search(r"#define\s+SLODE_QUANTILE_MAX_LEVELS\s+(\d+)", hdr).group(1)) == L.QUANTILE_MAX_LEVELS == QU.MAX_LEVELS == 8
    doc = hdr[hdr.index("sample quantiles of the head curves as ONE call"):m.start()]
    for word in ("NULL handle", "num_samples < 1", "adaptive solver", "dopri5", "particles > 1", "SLODE_NO_FOLD", "SLODE_ODE_ALG", "SLODE_EINVAL",
                 "n + num_samples", '"recon_quantiles"', "floor(h)", "min(lo + 1, K - 1)", "fma(g", "HOST array", "out NULL", "n_levels outside [1, 8]",
                 "outside [0, 1] or NaN", "tile < 0 or tile > T", "no atomics", "unspecified", "160 KiB", "slode_quantile_plan", "duplicates allowed"):
        assert word in doc, word
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_RECON_QUANTILES_LDS_MAX\s+\(160 \* 1024\)", common) and L.RECON_QUANTILES_LDS_MAX == QU.LDS_MAX
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "recon_quantiles_kernel.hip" in srcs
    assert "slode_recon_quantiles" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_recon_quantiles(None, None, None, None, None, None, None, 1, 8, 2, None, 0, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_engine_and_model_signatures():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase
    assert list(inspect.signature(Engine.recon_quantiles).parameters) == ["self", "params", "batch", "B", "is_post", "num_samples", "levels", "out", "tile",
                                                                         "particles"]
    assert list(inspect.signature(Engine.quantile_plan).parameters) == ["self", "B", "num_samples", "levels", "tile"]
    sig = inspect.signature(MechanisticBase.recon_quantiles).parameters
    assert list(sig)[:8] == ["self", "observations", "is_post", "num_samples", "levels", "eps", "tile", "max_sweeps"]
    assert sig["levels"].default == (0.025, 0.975) and sig["tile"].default == 0 and sig["max_sweeps"].default == 2 and sig["eps"].default is None


# ---- the rank, depth and selection rules -----------------------------------------------------------------------------------------------------
KS = (1, 2, 7, 200, 1024)


def test_depths_of_the_documented_examples():
    assert QU.depths((0.025, 0.975), 200) == (6, 6) and QU.depths((0.0, 1.0), 200) == (1, 1) and QU.depths((0.5,), 200) == (200, 0)
    assert QU.depths((0.5,), 7) == (4, 0)                                                  # one rank, served from the bottom on the tie
    assert QU.depths((0.0, 1.0), 2) == (2, 0) and QU.depths((0.3,), 1) == (1, 0)
    for K in KS:
        for levels in QU.LEVEL_SETS.values():
            m_lo, m_hi = QU.depths(levels, K)
            lo, hi, g = QU.ranks(levels, K)
            assert 1 <= m_lo and 0 <= m_hi and m_lo + m_hi <= K
            for r in list(lo) + [h for h, gg in zip(hi, g) if gg != 0.0]:                # every needed rank lies in one of the two buffers
                assert r < m_lo or K - 1 - r < m_hi, (K, levels, r)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(QU.LEVEL_SETS))
def test_select_against_numpy_quantile(name, K):
    """ranks / select on random fp32 data against np.quantile(method="linear") in fp64 on the same fp32 values: within 5 2^-24 max(|v_lo|,
    |v_hi|); exact wherever g == 0 (levels 0 and 1, K = 1, q (K - 1) an integer)."""
    levels = QU.LEVEL_SETS[name]
    rng = np.random.default_rng(K + len(levels))
    v = np.sort((rng.standard_normal((K, 5, 11)) * np.exp(rng.uniform(-3, 3, (1, 5, 1)))).astype(np.float32), axis=0)
    got = QU.select(v, levels)
    want = np.quantile(v.astype(np.float64), np.asarray(levels, dtype=np.float64), axis=0, method="linear")
    assert got.dtype == np.float32 and got.shape == want.shape == (len(levels), 5, 11)
    ratio = np.abs(got.astype(np.float64) - want) / np.maximum(QU.numpy_bar(v, levels), 1e-300)
    print("%s K=%d: error / bar %.3f" % (name, K, ratio.max()))
    assert ratio.max() <= 1.0
    lo, hi, g = QU.ranks(levels, K)
    for i, q in enumerate(levels):
        if g[i] == 0.0:
            assert np.array_equal(got[i], v[lo[i]]), (name, K, q)
        if q == 0.0:
            assert np.array_equal(got[i], v.min(0))
        if q == 1.0:
            assert np.array_equal(got[i], v.max(0))
    assert K > 1 or all(np.array_equal(got[i], v[0]) for i in range(len(levels)))


def test_integer_ranks_are_exact():
    v = np.sort(np.random.default_rng(3).standard_normal((201, 17)).astype(np.float32), axis=0)
    levels = (0.005, 0.25, 0.5, 0.995)                                                     # q x 200 = 1, 50, 100, 199
    lo, hi, g = QU.ranks(levels, 201)
    assert lo.tolist() == [1, 50, 100, 199] and np.all(g[[1, 2]] == 0.0)
    got = QU.select(v, levels)
    assert np.array_equal(got[1], v[50]) and np.array_equal(got[2], v[100])


# ---- the plan's ladder -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald", "challenge_gauss"])
def test_plan_against_the_restated_rule(case, K):
    from structured_latent_odes_amd import _lib as L
    eng = LU.host_engine(case)
    T = eng.T
    for name, levels in QU.LEVEL_SETS.items():
        for tile in (0, 1, T):
            want = QU.plan(eng.spec, T, K, levels, tile)
            if want is None:
                with pytest.raises(L.SlodeError, match="slode_quantile_plan: (tile = %d does not fit|depth = )" % tile):
                    eng.quantile_plan(8, K, levels, tile)
                assert tile != 1                                                          # one time point fits at every size of this table
                continue
            got = eng.quantile_plan(8, K, levels, tile)
            assert got == want, (case, K, name, tile, got, want)
            tl, sweeps, m_lo, m_hi, lds = got
            assert lds <= QU.LDS_MAX and m_lo + m_hi <= K and (m_lo, m_hi) == QU.depths(levels, K) and sweeps == -(-T // tl)
            assert tile == 0 or tl == tile
            if tile == 0 and sweeps > 1:                                                  # the fewest sweeps: one fewer would not fit
                assert QU.plan(eng.spec, T, K, levels, -(-T // (sweeps - 1))) is None


def test_plan_of_the_metric_shape():
    """cvs, T = 200: the band at K = 200 keeps 12 values per column and fits in one sweep; the median keeps all 200 and needs several."""
    eng = LU.host_engine("cvs_ald", T=200)
    band, median = eng.quantile_plan(1024, 200, (0.025, 0.975)), eng.quantile_plan(1024, 200, (0.5,))
    assert band[:4] == (200, 1, 6, 6) and median[2:4] == (200, 0) and median[1] > 8
    print("cvs T=200 K=200: band %s, median %s" % (band, median))


# case -> call column, status and the words its message must carry, written from include/slode.h in rung order
_N = "slode_recon_quantiles"
_BOTH, _POST, _PRIOR, _PLAN = ("post", "prior"), ("post",), ("prior",), ("plan",)
_BIG = "T 1024, S 8, C 4, median of"
_WS = ["workspace 64 B < required"]
_HEAD, _LABELS, _TWO = DL.shared_rungs(_N, "batch / times / stage_t / workspace", "sort recon_samples instead")
LADDER = _HEAD + [
    ("out NULL", _BOTH, -1, [_N, "out is NULL"]), ("n_levels 0", _BOTH, -1, [_N, "n_levels = 0 out of range [1, 8]"]),
    ("n_levels 9", _BOTH, -1, [_N, "n_levels = 9 out of range [1, 8]"]), ("levels NULL", _BOTH, -1, [_N, "levels is NULL"]),
    ("levels[1] 1.5", _BOTH, -1, [_N, "levels[1] = 1.5 is not in [0, 1]"]), ("levels[0] -0.001", _BOTH, -1, [_N, "levels[0] = -0.001 is not in [0, 1]"]),
    ("levels[1] NaN", _BOTH, -1, [_N, "levels[1] = nan is not in [0, 1]"]),
    ("levels[2] NaN beyond n_levels = 2: not read; workspace too small", _BOTH, -3, _WS),
    ("tile -1", _BOTH, -1, [_N, "tile = -1 out of range [0, T = 86]"]), ("tile T + 1", _BOTH, -1, [_N, "tile = 87 out of range [0, T = 86]"]),
    ("LDS: %s 1024, tile 4" % _BIG, _BOTH, -1, [_N, "tile = 4 does not fit", "LDS tables", "depth = 1024 + 0 (267520 B", "budget of 163840 B", "tile = 0"]),
    ("LDS: %s 4096, tile 0" % _BIG, _BOTH, -1, [_N, "depth = 4096 + 0 of num_samples = 4096", "one time point", "(267520 B of a budget of 163840 B)",
                                              "sort recon_samples instead"]),
    ("%s 1024, tile 0: fits; workspace too small" % _BIG, _BOTH, -3, _WS),
    ("unordered and duplicate levels: taken; workspace too small", _BOTH, -3, _WS),
] + _LABELS + [
] + _TWO + [                                                                          # two conditions at once: the earlier rung speaks
    ("no_fold + out NULL", _POST, -1, ["observation strides"]),
    ("out NULL + n_levels 0", _BOTH, -1, ["out is NULL"]), ("n_levels 9 + levels[0] NaN", _BOTH, -1, ["n_levels = 9"]),
    ("levels[0] NaN + tile -1", _BOTH, -1, ["levels[0] = nan"]), ("tile -1 + LDS", _BOTH, -1, ["tile = -1 out of range [0, T = 1024]"]),
    ("LDS + label columns 3", _BOTH, -1, ["depth = 4096 + 0"]), ("label columns 3 + workspace too small", _BOTH, -1, ["label tensors have 3 columns"]),
    # the plan
    ("shape NULL", _PLAN, -1, ["slode_quantile_plan", "shape is NULL"]), ("bad shape", _PLAN, -1, ["slode_quantile_plan", "T out of range"]),
    ("sweeps NULL", _PLAN, -1, ["slode_quantile_plan", "sweeps", "is NULL"]), ("num_samples 0", _PLAN, -1, ["slode_quantile_plan", "num_samples = 0 < 1"]),
    ("n_levels 9", _PLAN, -1, ["slode_quantile_plan", "n_levels = 9"]), ("levels NULL", _PLAN, -1, ["slode_quantile_plan", "levels is NULL"]),
    ("levels[1] NaN", _PLAN, -1, ["slode_quantile_plan", "levels[1] = nan"]), ("tile T + 1", _PLAN, -1, ["slode_quantile_plan", "tile = 87"]),
    ("LDS: %s 1024, tile 4" % _BIG, _PLAN, -1, ["slode_quantile_plan", "tile = 4 does not fit", "(267520 B"]),
    ("LDS: %s 4096, tile 0" % _BIG, _PLAN, -1, ["slode_quantile_plan", "depth = 4096 + 0", "(267520 B"]),
]


def test_quantile_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_recon_quantiles (posterior and prior) and of slode_quantile_plan without a device, in rung order:
    status, the words of the message and the untouched drawing-call counter against LADDER; line by line against
    tests/golden/quantile_refusals.txt; the rungs shared with slode_recon_moments carry the texts tests/golden/eval_refusals.txt records for
    it on that side, the call's name, its list of required pointers and its advice apart; the call's LDS figures are the plan's; and the
    memory that stands for the outputs untouched."""
    _, shared, figures = DL.check_ladder("quantile_refusals", tmp_path, LADDER, _N, "sort recon_samples instead")
    assert len(figures) == 2 and all(len(v) == 1 for v in figures.values())            # the call's figures are the plan's
    assert shared >= 40


# ---- the Python layer on an engine double ---------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self, refuse, Q, sweeps=1, plan_refuses=False):
        from structured_latent_odes_amd import _lib as L
        self.L, self.refuse, self.Q, self.sweeps, self.plan_refuses = L, refuse, Q, sweeps, plan_refuses
        self.calls, self.plans, self.batches, self.draws, self.counter = [], [], [], [], 5

    def _raise(self, status):
        err = self.L.SlodeError("libslode call failed (%d)" % status)
        err.status = status
        raise err

    def rng_state(self):
        return (0, 0, self.counter)

    def rng_set_counter(self, n):
        self.counter = int(n)

    def draw_normal(self, rows):
        self.draws.append(rows)
        self.counter += 1
        return torch.linspace(-1.0, 1.0, rows * 4).view(rows, 4)

    def make_batch(self, obs, labels, eps=None, particles=1, eps_shape=None):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def quantile_plan(self, B, num_samples, levels, tile=0):
        self.plans.append((B, num_samples, tuple(levels), tile))
        if self.plan_refuses:
            self._raise(-1)
        return (tile or 6, self.sweeps, 1, 1, 4096)

    def recon_quantiles(self, flat, bt, B, is_post, num_samples, levels, out=None, tile=0):
        self.calls.append((bool(is_post), num_samples, tuple(levels), out, tile))
        if self.refuse:
            self._raise(self.refuse)
        lv = torch.arange(len(levels), dtype=torch.float32).view(-1, 1, 1, 1, 1)
        return lv + 10.0 * torch.arange(self.Q, dtype=torch.float32).view(1, self.Q, 1, 1, 1) + torch.zeros(len(levels), self.Q, B, 3, 6)


def _double(gauss, refuse=0, **kw):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        FAMILY, GAUSS = "cvs", gauss
        LABELS = ("iext", "rtpr")

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3, **kw), "flat": torch.zeros(1)})()
            self.times = torch.tensor([0.0, 1.0, 3.0, 4.0, 8.0, 9.0])
            self.sampled = []

        def _bind(self):
            return self._b

        def recon_samples(self, observations, is_post, num_samples, eps=None, **labels):
            """curve value = (t - 4)^2 / 4 - eps[., ., 0] on channel 0, its negative on channel 1, a constant 1 on channel 2 (+ 100 per head)."""
            self.sampled.append((observations.shape[0], num_samples))
            e = eps[:, :, 0].permute(1, 0).reshape(-1, 1, 1, num_samples)
            base = ((self.times - 4.0) ** 2 / 4.0).view(1, 1, 6, 1) - e
            v = torch.cat([base, -base, torch.ones_like(base)], 1)
            return {n: v + 100.0 * i for i, n in enumerate(("mean",) if gauss else ("mu_50", "mu_75", "mu_25"))}

    return M()


LABELS = dict(iext=torch.zeros(7, 1), rtpr=torch.ones(7, 1))
OBS = torch.zeros(7, 3, 6)


@pytest.mark.parametrize("gauss", [False, True])
def test_model_level_call_uses_the_engine_once(gauss):
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss)
    eng = m._b.engine
    res = m.recon_quantiles(OBS, True, 5, **LABELS)
    assert eng.calls == [(True, 5, (0.025, 0.975), None, 0)] and eng.plans == [(7, 5, (0.025, 0.975), 0)]
    assert eng.batches == [((7, 3, 6), 2, None, 5)] and eng.draws == [] and m.sampled == []
    assert set(res) == set(names) | {"levels"} and res["levels"].tolist() == [0.025, 0.975] and res["levels"].dtype == torch.float64
    for q, n in enumerate(names):
        assert tuple(res[n].shape) == (2, 7, 3, 6) and float(res[n][0, 0, 0, 0]) == 10.0 * q and float(res[n][1, 0, 0, 0]) == 10.0 * q + 1.0
    five = m.recon_quantiles(OBS, False, 5, levels=torch.tensor(QU.LEVEL_SETS["five"], dtype=torch.float64), eps=torch.zeros(5, 7, 4), tile=3, **LABELS)
    assert eng.calls[-1] == (False, 5, QU.LEVEL_SETS["five"], None, 3) and eng.batches[-1] == ((7, 3, 6), 2, (5, 7, 4), 5)
    assert tuple(five[names[0]].shape) == (5, 7, 3, 6)
    for bad, match in ((dict(levels=()), "1 to 8"), (dict(levels=[0.1] * 9), "1 to 8"), (dict(levels=(0.5, 1.5)), r"\[0, 1\]"),
                       (dict(levels=(float("nan"),)), r"\[0, 1\]"), (dict(tile=-1), "tile"), (dict(tile=7), "tile")):
        with pytest.raises(ValueError, match=match):
            m.recon_quantiles(OBS, True, 5, **dict(LABELS, **bad))
    with pytest.raises(ValueError, match="num_samples"):
        m.recon_quantiles(OBS, True, 0, **LABELS)
    assert len(eng.calls) == 2


def _want_composed(m, names, levels, ns=5):
    """The composed result by the numpy restatement: the double's curves on the double's noise, sorted, QU.select."""
    eps = torch.linspace(-1.0, 1.0, 7 * ns * 4).view(ns, 7, 4)
    curves = m.recon_samples(OBS, True, ns, eps=eps)
    m.sampled.pop()
    return {n: QU.select(np.sort(curves[n].permute(3, 0, 1, 2).numpy(), axis=0), levels) for n in names}


@pytest.mark.parametrize("route", ["engine refuses", "plan refuses", "sweeps > max_sweeps"])
@pytest.mark.parametrize("gauss", [False, True])
def test_composed_route_exactly_when_refused_or_beyond_max_sweeps(gauss, route, monkeypatch):
    """The composed route: one drawing call for the whole batch, recon_samples over chunks of trajectories, a sort along the draws and the
    same rank rule -- equal to the numpy restatement bitwise, independent of the chunking; the counter ends num_samples further."""
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, **{"engine refuses": dict(refuse=-1), "plan refuses": dict(plan_refuses=True), "sweeps > max_sweeps": dict(sweeps=3)}[route])
    eng = m._b.engine
    levels = QU.LEVEL_SETS["eight"]
    res = m.recon_quantiles(OBS, True, 5, levels=levels, **LABELS)
    assert len(eng.calls) == (1 if route == "engine refuses" else 0) and len(eng.plans) == 1
    assert eng.draws == [35] and m.sampled == [(7, 5)] and eng.counter == 5 + 5
    want = _want_composed(m, names, levels)
    for n in names:
        assert res[n].dtype == torch.float32 and np.array_equal(res[n].numpy(), want[n]), n
    # channel 2 is constant: every level returns it; levels 0 and 1 are the extremes of the draws
    assert torch.all(res[names[0]][:, :, 2] == 1.0)
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)                                  # 15 // 5 = 3 rows per chunk: 3 + 3 + 1
    m.sampled.clear()
    chunked = m.recon_quantiles(OBS, True, 5, levels=levels, **LABELS)
    assert m.sampled == [(3, 5), (3, 5), (1, 5)] and eng.draws == [35, 35] and eng.counter == 5 + 10
    assert all(torch.equal(chunked[n], res[n]) for n in names)
    given = m.recon_quantiles(OBS, True, 5, levels=levels, eps=torch.linspace(-1.0, 1.0, 140).view(5, 7, 4), **LABELS)
    assert all(torch.equal(given[n], res[n]) for n in names) and eng.counter == 5 + 10   # explicit noise draws nothing


def test_max_sweeps_switch():
    m = _double(False, sweeps=2)
    m.recon_quantiles(OBS, True, 5, **LABELS)
    assert len(m._b.engine.calls) == 1 and m.sampled == []                                 # sweeps == max_sweeps: the engine
    m.recon_quantiles(OBS, True, 5, max_sweeps=1, **LABELS)
    assert len(m._b.engine.calls) == 1 and m.sampled == [(7, 5)]
    m = _double(False, sweeps=40)
    m.recon_quantiles(OBS, True, 5, max_sweeps=40, **LABELS)
    assert len(m._b.engine.calls) == 1 and m.sampled == []


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.recon_quantiles(OBS, True, 5, **LABELS)
    assert m.sampled == [] and m._b.engine.draws == []


def test_save_recon_quantiles_files_and_line(tmp_path):
    m = _double(False)
    batches = [dict(observations=torch.zeros(B, 3, 6), iext=torch.zeros(B, 1), rtpr=torch.zeros(B, 1)) for B in (2, 3)]
    files = m.save_recon_quantiles(str(tmp_path / "r"), batches, False, 4, levels=(0.9, 0.1, 0.5))
    want = ["%s_prior_sample_quantiles.npy" % n for n in ("mu_50", "mu_75", "mu_25")] + ["sample_quantile_levels.npy"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "r"))) == sorted(want)
    lv = np.load(files[-1])
    assert lv.dtype == np.float64 and lv.tolist() == [0.9, 0.1, 0.5]
    q = np.load(files[0])
    assert q.shape == (5, 3, 3, 6) and q.dtype == np.float32 and q[0, :, 0, 0].tolist() == [0.0, 1.0, 2.0] and np.load(files[1])[4, 2, 2, 5] == 12.0
    obs = np.full((5, 3, 6), 0.5)
    obs[0] = 1.5                                                                           # the band is [1, 0] by the double's values: lowest level 0.1 -> 1
    line = m.quantile_line(q, lv, obs, "prior")
    assert line == "sample_quantiles_prior: n=5  levels=[0.1, 0.9]  mean_width=-1  inside=0.000", line
    assert m.quantile_line(q[:, :2], np.array([0.1, 0.9]), obs, "post").endswith("mean_width=1  inside=0.800")


def test_training_entry_points_take_the_flags():
    import inspect
    from structured_latent_odes_amd import training as TR
    sig = inspect.signature(TR.train).parameters
    assert sig["sample_quantiles"].default == 0 and tuple(sig["quantile_levels"].default) == (0.025, 0.975)
    a = TR.build_parser().parse_args(["--sample-quantiles", "64", "--quantile-levels", "0,0.5,1"])
    assert (a.sample_quantiles, a.quantile_levels) == (64, [0.0, 0.5, 1.0])
    d = TR.build_parser().parse_args([])
    assert (d.sample_quantiles, d.quantile_levels) == (0, [0.025, 0.975])
