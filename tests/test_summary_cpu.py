"""CPU tests of the curve summaries: the C ABI of slode_curve_summary / slode_curve_summary_plan, the plan against a hand count of the
kernel's tables (with and without p_beyond, a shape that fits only without), the refusal ladder on a hand-filled handle
(tests/summary_refusals/summary_refusals.cpp), every condition the GPU tests ask shown to hold for the fp64 oracle alone (the near share of
the tests' threshold, the tolerant rules on the oracle perturbed by half a bar, the summation bar against a wrong weight table), the numpy
restatement of the moments over draws, and the Python layer on an engine double (the dict, the composed route, the files)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import draws_ladder_util as DL
from tests import eval_stats_util as EU
from tests import lds_util as LU
from tests import recon_moments_util as RU
from tests import summary_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "is_post", "num_samples", "thr", "sense", "mean", "sd", "p_beyond", "workspace",
        "workspace_bytes", "stream"]


def test_abi_exports_curve_summary_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_curve_summary", "slode_curve_summary_plan"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 250 and "0.2.5" in hdr
    for earlier in ("0.2.4: slode_latent_attribution", "0.2.3: slode_pointwise_density", "0.2.2: slode_posterior_refine", "0.1.5: slode_recon_moments"):
        assert earlier in hdr                                                             # the earlier version lines are kept
    m = re.search(r"int\s+slode_curve_summary\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_curve_summary.argtypes
    assert len(at) == len(ARGS) and at[7] is C.c_int and at[8] is C.c_int and at[10] is C.c_int and at[15] is C.c_size_t
    assert re.search(r"int\s+slode_curve_summary_plan\s*\(\s*const slode_shape\*\s*s,\s*int want_p_beyond,\s*size_t\*\s*lds_bytes\s*\)\s*;", hdr)
    assert int(re.search(r"#define\s+SLODE_SUMMARY_SLOTS\s+(\d+)", hdr).group(1)) == L.SUMMARY_SLOTS == len(L.SUMMARY_NAMES) == 8
    assert L.SUMMARY_NAMES == SU.NAMES
    doc = hdr[hdr.index("curve summaries as ONE call"):m.start()]
    for word in ("NULL handle", "num_samples < 1", "adaptive solver", "dopri5", "particles > 1", "SLODE_NO_FOLD", "SLODE_ODE_ALG", "LDS tables",
                 "SLODE_EINVAL", "n + 1", "POPULATION", "t_peak", "t_trough", "time_beyond", "t_hit", "crossed", "smallest i", "HOST array",
                 "P(cross)", "NaN", '"curve_summary"', "p_beyond", "sense", "mean NULL", "no atomics", "half mirror", "slode_curve_summary_plan"):
        assert word in doc, word
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_CURVE_SUMMARY_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_curve_summary_lds_bytes" in common
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "curve_summary_kernel.hip" in srcs
    assert "slode_curve_summary" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_curve_summary(None, None, None, None, None, None, None, 1, 8, None, 1, None, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_engine_signature():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.curve_summary).parameters)[:11] == ["self", "params", "batch", "B", "is_post", "num_samples", "thr", "sense",
                                                                            "mean", "sd", "p_beyond"]
    assert list(inspect.signature(Engine.curve_summary_plan).parameters) == ["self", "B", "want_p_beyond"]


def _hand_count(eng, want_p):
    """The shared forward pieces (step table 2 (T - 1) S, one row of 2 + 2 S floats rounded up to four per hidden unit, the transposed first
    layers L x 2 H, their biases 2 H, the init net's output layer H S + S, the head weights Q C S, the dynamics biases 2 S, z, the labels, the
    init net's hidden layer, x0), loc | scale, then the grid T and the node weights T, the value table Q C T, the counts Q C T only with p_beyond, and the
    moment triples 3 Q C 8; every piece rounded up to 16 bytes."""
    sp, T = eng.spec, eng.T
    Ld, Cn, Q = sp.latent_dim, sp.n_channels, 1 if sp.gauss else 3
    return 4 * (LU.spec_shared_floats(sp, T) + 2 * LU.r4(Ld) + 2 * LU.r4(T) + LU.r4(Q * Cn * T) * (2 if want_p else 1) + LU.r4(3 * Q * Cn * 8))


@pytest.mark.parametrize("case", list(EU.CASES))
def test_plan_against_a_hand_count_of_the_tables(case):
    eng = LU.host_engine(case)
    sp = eng.spec
    with_p, without = eng.curve_summary_plan(8, True), eng.curve_summary_plan(8, False)
    assert with_p == _hand_count(eng, True) and without == _hand_count(eng, False)
    assert with_p - without == 4 * LU.r4((1 if sp.gauss else 3) * sp.n_channels * eng.T)         # the counters cost exactly one Q C T table


def test_plan_of_a_shape_that_fits_only_without_the_counters():
    """T = 1024, S = 8, ALD, C = 4 (proc): the step table alone is 2 x 1023 x 8 x 4 B = 64 KB and the two Q C T tables are 48 KB each."""
    from structured_latent_odes_amd import _lib as L
    eng = LU.host_engine("proc_ald", T=1024)
    sp = eng.spec
    assert (sp.ode_state_dim, sp.n_channels, sp.gauss) == (8, 4, False)
    assert 2 * LU.r4(1023 * 8) * 4 == 65472 and LU.r4(12 * 1024) * 4 == 48 * 1024
    without, want = eng.curve_summary_plan(8, False), _hand_count(eng, True)
    assert without == _hand_count(eng, False) <= 160 * 1024 < want
    with pytest.raises(L.SlodeError, match=r"T = 1024, S = 8, C = 4, with p_beyond \(%d B\) exceed the budget of 163840 B" % want):
        eng.curve_summary_plan(8, True)


# case -> call column, status and the words its message must carry, written from include/slode.h in rung order
_N = "slode_curve_summary"
_BOTH, _POST, _PRIOR, _PLAN = ("post", "prior"), ("post",), ("prior",), ("plan",)
_BIG = "T 1024, S 8, C 4"
_HEAD, _LABELS, _TWO = DL.shared_rungs(_N, "batch / times / stage_t / workspace", "reduce recon_samples instead")
LADDER = _HEAD + [
    ("mean NULL", _BOTH, -1, [_N, "mean is NULL"]), ("sense 0", _BOTH, -1, [_N, "sense = 0"]), ("sense 2", _BOTH, -1, [_N, "sense = 2"]),
    ("thr[1] NaN", _BOTH, -1, [_N, "thr[1] = nan is not finite"]), ("thr[2] inf", _BOTH, -1, [_N, "thr[2] = inf is not finite"]),
    ("thr[3] NaN beyond C = 3: not read; workspace too small", _BOTH, -3, ["workspace 64 B < required"]),
    ("p_beyond without thr", _BOTH, -1, [_N, "p_beyond needs a threshold"]),
    ("LDS: %s, with p_beyond" % _BIG, _BOTH, -1, [_N, "LDS tables", "T = 1024, S = 8, C = 4, with p_beyond (178464 B", "counts", "drop p_beyond"]),
    ("%s, without p_beyond: fits; workspace too small" % _BIG, _BOTH, -3, ["workspace 64 B < required"]),
] + _LABELS + [
    ("sd, p_beyond and thr NULL, sense -1; workspace too small", _BOTH, -3, ["workspace 64 B < required"]),
] + _TWO + [                                                                          # two conditions at once: the earlier rung speaks
    ("no_fold + mean NULL", _POST, -1, ["observation strides"]),
    ("mean NULL + sense 0", _BOTH, -1, ["mean is NULL"]), ("sense 0 + thr[0] NaN", _BOTH, -1, ["sense = 0"]),
    ("thr[0] NaN + LDS", _BOTH, -1, ["thr[0] = nan"]), ("p_beyond without thr + LDS", _BOTH, -1, ["p_beyond needs a threshold"]),
    ("LDS + label columns 3", _BOTH, -1, ["LDS tables"]), ("label columns 3 + workspace too small", _BOTH, -1, ["label tensors have 3 columns"]),
    # the plan
    ("shape NULL", _PLAN, -1, ["slode_curve_summary_plan", "shape is NULL"]), ("bad shape", _PLAN, -1, ["slode_curve_summary_plan", "T out of range"]),
    ("lds_bytes NULL", _PLAN, -1, ["slode_curve_summary_plan", "lds_bytes is NULL"]),
    ("LDS: %s, with p_beyond" % _BIG, _PLAN, -1, ["slode_curve_summary_plan", "LDS tables", "with p_beyond (178464 B)"]),
]


def test_summary_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_curve_summary (posterior and prior) and of slode_curve_summary_plan without a device, in rung
    order: status, the words of the message and the untouched drawing-call counter against LADDER; line by line against
    tests/golden/summary_refusals.txt; the rungs shared with slode_recon_moments carry the texts tests/golden/eval_refusals.txt records for
    it on that side, the call's name and its list of required pointers apart (the advice is the same); the call's LDS figure is the plan's;
    and the memory that stands for the outputs untouched."""
    _, shared, figures = DL.check_ladder("summary_refusals", tmp_path, LADDER, _N, "reduce recon_samples instead")
    assert set().union(*figures.values()) == {"178464"}                                # the call's figure is the plan's
    assert shared >= 50


# ---- the numpy restatement on curves whose functionals are known ----------------------------------------------------------------------------
def test_functionals_on_constructed_curves():
    times = np.array([0.0, 1.0, 3.0, 4.0, 8.0], dtype=np.float32)
    w = SU.weights_f32(times)
    assert w.tolist() == [0.5, 1.5, 1.5, 2.5, 2.0] and float(w.sum()) == 8.0
    v = np.array([[[1.0, 3.0, 3.0, 0.0, 0.0], [2.0, 2.0, 2.0, 2.0, 2.0]]], dtype=np.float32)             # ties: the first index wins
    f = SU.functionals(v, times, thr=[2.5, 2.0], sense=1)
    assert f[0, 0].tolist() == [3.0, 1.0, 0.0, 4.0, 0.5 + 4.5 + 4.5, 3.0, 1.0, 1.0]
    assert f[0, 1, :6].tolist() == [2.0, 0.0, 2.0, 0.0, 16.0, 0.0] and np.isnan(f[0, 1, 6]) and f[0, 1, 7] == 0.0   # v > thr is strict
    g = SU.functionals(v, times, thr=[2.5, 2.5], sense=-1)
    assert g[0, 0, 5:].tolist() == [0.5 + 2.5 + 2.0, 0.0, 1.0] and g[0, 1, 5:].tolist() == [8.0, 0.0, 1.0]
    n = SU.functionals(v, times)
    assert np.array_equal(n[..., :5], f[..., :5]) and np.isnan(n[..., 5:]).all()


def test_moments_over_draws_take_t_hit_over_the_crossing_draws():
    f = np.zeros((4, 2, 8), dtype=np.float32)
    f[:, 0, 6], f[:, 0, 7] = [np.nan, 2.0, np.nan, 4.0], [0, 1, 0, 1]
    f[:, 1, 6], f[:, 1, 7] = np.nan, 0
    f[:, :, 0] = [[1, 5], [2, 5], [3, 5], [6, 5]]
    mean, sd = SU.draw_moments_f32(f)
    assert mean[0, 6] == 3.0 and sd[0, 6] == 1.0 and mean[0, 7] == 0.5 and sd[0, 7] == 0.5
    assert np.isnan(mean[1, 6]) and np.isnan(sd[1, 6]) and mean[1, 7] == 0.0 and sd[1, 7] == 0.0
    assert mean[0, 0] == 3.0 and sd[1, 0] == 0.0
    one_mean, one_sd = SU.draw_moments_f32(f[1:2])
    assert np.array_equal(one_mean[0], f[1, 0]) and np.all(one_sd[0] == 0.0)             # one draw: sd exactly 0, the mean is the draw


# ---- every condition the GPU tests assert, on the oracle alone ------------------------------------------------------------------------------
ORACLE_CASES = ["cvs_ald", "cvs_gauss", "challenge_gauss", "proc_ald", "proc_gauss"]


@functools.lru_cache(maxsize=None)
def _oracle(case, is_post):
    c = RU.build(case, "rk4", B=13, ns=7)
    v = SU.oracle_draws(c, is_post)
    return c, v, SU.thresholds(v)


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_oracle_threshold_lies_inside_the_curves_and_has_few_near_points(case, is_post):
    """The median threshold: most rows cross it, and the points within one bar of it are under the cap NEAR_SHARE of all points."""
    c, v, thr = _oracle(case, is_post)
    crossing = float(SU.beyond(v, thr.astype(np.float64), 1).any(-1).mean())
    share = float(SU.near(v, thr).mean())
    print("%s %s: thr %s, rows that cross %.2f, near share %.2e" % (case, "post" if is_post else "prior", thr, crossing, share))
    assert 0.5 <= crossing <= 1.0 and share <= SU.NEAR_SHARE


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_oracle_perturbed_by_half_a_bar_meets_every_rule(case, is_post):
    """A stand-in for the device: the oracle's curves moved by up to half a bar and rounded to fp32.  Its functionals meet the tolerant
    rules, the continuous bars and the count rule -- both senses, nothing excluded."""
    c, v, thr = _oracle(case, is_post)
    rng = np.random.default_rng(5)
    v32 = RU._f32(v + 0.5 * SU.bar(v) * rng.uniform(-1, 1, v.shape))
    times = c["times"].numpy()
    span = float(times[-1] - times[0])
    for sense in (1, -1):
        f = SU.functionals(v32, times, thr, sense)                                       # [Q, ns, B, C, 8]
        bad = SU.tolerant_violations(f, v, times, thr, sense)
        assert all(n == 0 for _, n in bad), (case, sense, bad)
        want = SU.functionals(v, times, thr.astype(np.float64), sense)
        gm, gs = SU.draw_moments_f32(np.moveaxis(f, 1, 0))
        wm, ws = SU.oracle_moments(np.moveaxis(want, 1, 0))
        SU.check_continuous(gm.astype(np.float64), gs.astype(np.float64), wm, ws, np.abs(v).max(-1).max(1), span, "%s sense %d" % (case, sense))
        p = RU._f32(SU.beyond(v32, thr, sense).sum(1)) / np.float32(7)
        SU.check_counts(p, 7, np.moveaxis(v, 1, 0), thr, sense, "%s sense %d" % (case, sense))


@pytest.mark.parametrize("case", ["cvs_ald", "challenge_gauss"])
def test_summation_bar_discriminates_a_wrong_weight_table(case):
    """Any fixed order of the fp32 sum stays within the bar of the fp64 sum of the fp32 terms -- shown on three orders, the kernel's among
    them -- and a table whose end weights are not halved misses it by a wide margin on all but the curves that vanish at both ends."""
    c, v, thr = _oracle(case, True)
    times = c["times"].numpy()
    v32 = RU._f32(v)
    w = SU.weights_f32(times)
    want = SU.functionals(v32, times)[..., 4]
    bar_auc, _ = SU.sum_bars(v32, times)
    terms = RU._f32(w * v32)
    T = terms.shape[-1]

    def sequential(x, order):
        acc = np.zeros(x.shape[:-1], np.float32)
        for i in order:
            acc = RU._f32(acc + x[..., i])
        return acc

    def kernel_order(x):
        lanes = [sequential(x, range(l, T, 16)) for l in range(16)]
        for step in (1, 2):
            lanes = [RU._f32(lanes[l] + lanes[l ^ step]) for l in range(16)]
        lanes = [RU._f32(lanes[l] + lanes[(l & 8) | (7 - (l & 7))]) for l in range(16)]
        return RU._f32(lanes[0] + lanes[15])
    for name, got in (("left to right", sequential(terms, range(T))), ("right to left", sequential(terms, range(T - 1, -1, -1))),
                      ("the kernel's rows", kernel_order(terms))):
        r = float((np.abs(got - want) / bar_auc).max())
        print("%s, %s: error / bar %.3f" % (case, name, r))
        assert r <= 1.0
    wrong = SU.functionals(v32, times, w=SU.weights_ends_not_halved(times))[..., 4]
    r = np.abs(wrong - want) / bar_auc
    print("%s, end weights not halved: error / bar median %.1f, min %.2f, share of curves beyond the bar %.3f" % (case, np.median(r), r.min(), (r > 1.0).mean()))
    assert np.median(r) > 10.0 and (r > 1.0).mean() > 0.9           # (a curve that is 0 at both ends cannot tell the two tables apart)


# ---- the Python layer on an engine double ---------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self, refuse, Q):
        from structured_latent_odes_amd import _lib as L
        self.L, self.refuse, self.Q = L, refuse, Q
        self.calls, self.batches, self.draws = [], [], []

    def draw_normal(self, rows):
        self.draws.append(rows)
        return torch.linspace(-1.0, 1.0, rows * 4).view(rows, 4)

    def make_batch(self, obs, labels, eps=None, particles=1, eps_shape=None):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def curve_summary(self, flat, bt, B, is_post, num_samples, thr, sense, mean, sd=None, p_beyond=None):
        self.calls.append((bool(is_post), num_samples, thr, sense, mean, sd, p_beyond))
        if self.refuse:
            err = self.L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        m = torch.arange(8, dtype=torch.float32).view(1, 1, 1, 8) + 10.0 * torch.arange(self.Q, dtype=torch.float32).view(self.Q, 1, 1, 1) + torch.zeros(self.Q, B, 3, 8)
        return m, m + 0.5, (torch.full((self.Q, B, 3, 6), 0.25) if p_beyond else None)


def _double(gauss, refuse):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        FAMILY, GAUSS = "cvs", gauss
        LABELS = ("iext", "rtpr")

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3), "flat": torch.zeros(1)})()
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


@pytest.mark.parametrize("gauss", [False, True])
def test_model_level_call_uses_the_engine_once(gauss):
    obs = torch.zeros(7, 3, 6)
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, 0)
    eng = m._b.engine
    res = m.curve_summary(obs, True, 5, thresholds=torch.tensor([1.0, 2.0, 3.0]), sense="below", pointwise=True, **LABELS)
    assert eng.calls == [(True, 5, [1.0, 2.0, 3.0], -1, None, True, True)] and eng.batches == [((7, 3, 6), 2, None, 5)] and eng.draws == []
    assert set(res) == set(names)
    for q, n in enumerate(names):
        assert set(res[n]) == set(SU.NAMES) | {"p_beyond"} and tuple(res[n]["p_beyond"].shape) == (7, 3, 6)
        for j, k in enumerate(SU.NAMES):
            mean, sd = res[n][k]
            assert tuple(mean.shape) == tuple(sd.shape) == (7, 3) and float(mean[0, 0]) == 10.0 * q + j and float(sd[0, 0]) == 10.0 * q + j + 0.5
    plain = m.curve_summary(obs, False, 5, eps=torch.zeros(5, 7, 4), **LABELS)
    assert eng.calls[-1] == (False, 5, None, 1, None, True, None) and eng.batches[-1] == ((7, 3, 6), 2, (5, 7, 4), 5)
    assert all(set(plain[n]) == set(SU.NAMES) for n in names)
    for bad, match in ((dict(sense="up"), "sense"), (dict(thresholds=[1.0, 2.0]), "one per channel"), (dict(pointwise=True), "needs thresholds")):
        with pytest.raises(ValueError, match=match):
            m.curve_summary(obs, True, 5, **dict(LABELS, **bad))
    with pytest.raises(ValueError, match="num_samples"):
        m.curve_summary(obs, True, 0, **LABELS)
    assert len(eng.calls) == 2


@pytest.mark.parametrize("gauss", [False, True])
def test_composed_route_on_a_refusal(gauss, monkeypatch):
    """The engine refuses (status -1): one drawing call for the whole batch, recon_samples in chunks, the functionals in torch on the same
    definitions -- equal to the numpy restatement on the same curves, first index on ties, t_hit over the crossing draws, independent of the
    chunking."""
    obs = torch.zeros(7, 3, 6)
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, -1)
    eng = m._b.engine
    thr = [0.5, -0.5, 1.0]
    res = m.curve_summary(obs, True, 5, thresholds=thr, sense="above", pointwise=True, **LABELS)
    assert len(eng.calls) == 1 and eng.draws == [35] and m.sampled == [(7, 5)]
    eps = torch.linspace(-1.0, 1.0, 35 * 4).view(5, 7, 4)
    curves = m.recon_samples(obs, True, 5, eps=eps)
    times = m.times.numpy()
    for i, n in enumerate(names):
        v = curves[n].permute(3, 0, 1, 2).numpy()                                           # [ns, B, C, T]
        wm, ws = SU.oracle_moments(SU.functionals(v, times, np.array(thr, np.float32), 1))
        for j, k in enumerate(SU.NAMES):
            gm, gs = (t.double().numpy() for t in res[n][k])
            assert np.allclose(gm, wm[..., j], rtol=1e-5, atol=1e-6, equal_nan=True), (n, k)
            assert np.allclose(gs, ws[..., j], rtol=1e-4, atol=1e-4, equal_nan=True), (n, k)
        assert np.array_equal(res[n]["p_beyond"].numpy(), RU._f32(SU.beyond(v, np.array(thr, np.float32), 1).sum(0)) / np.float32(5))
    r = res[names[0]]
    # channel 2 is constant 1 and thr is 1: never strictly above -- crossed 0, t_hit NaN; every point attains both extremes: t = t_0
    assert float(r["crossed"][0][0, 2]) == 0.0 and torch.isnan(r["t_hit"][0][:, 2]).all()
    assert float(r["t_peak"][0][0, 2]) == 0.0 and float(r["t_trough"][0][0, 2]) == 0.0 and float(r["auc"][0][0, 2]) == 9.0
    # channel 0 is a parabola with its minimum at t = 4: t = 9 lies higher than t = 0 and t = 8, which tie
    assert float(r["t_trough"][0][0, 0]) == 4.0 and float(r["t_peak"][0][0, 0]) == 9.0
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)                                  # 15 // 5 = 3 rows per chunk: 3 + 3 + 1
    m.sampled.clear()
    chunked = m.curve_summary(obs, True, 5, thresholds=thr, sense="above", pointwise=True, **LABELS)
    assert m.sampled == [(3, 5), (3, 5), (1, 5)] and eng.draws == [35, 35]
    for n in names:
        for k in SU.NAMES:
            assert all(torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num())
                       for a, b in zip(chunked[n][k], res[n][k])), (n, k)
        assert torch.equal(chunked[n]["p_beyond"], res[n]["p_beyond"])
    none = m.curve_summary(obs, True, 5, **LABELS)
    assert all(torch.isnan(none[n][k][0]).all() for n in names for k in ("time_beyond", "t_hit", "crossed")) and "p_beyond" not in none[names[0]]


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.curve_summary(torch.zeros(7, 3, 6), True, 5, **LABELS)
    assert m.sampled == [] and m._b.engine.draws == []


def test_save_curve_summary_files_and_line(tmp_path):
    m = _double(False, 0)
    batches = [dict(observations=torch.zeros(B, 3, 6), iext=torch.zeros(B, 1), rtpr=torch.zeros(B, 1)) for B in (2, 3)]
    files = m.save_curve_summary(str(tmp_path / "r"), batches, False, 4, thresholds=[1.0, 2.0, 3.0], sense="below")
    want = ["summary_%s_prior_%s.npy" % (n, k) for n in ("mu_50", "mu_75", "mu_25") for k in ("mean", "sd")] + ["summary_slots.npy"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "r"))) == sorted(want)
    assert np.load(files[-1]).tolist() == list(SU.NAMES)
    mean, sd = np.load(files[0]), np.load(files[1])
    assert mean.shape == sd.shape == (5, 3, 8) and mean.dtype == np.float32 and mean[0, 0].tolist() == list(range(8)) and sd[0, 0, 0] == 0.5
    line = m.summary_line(mean, "prior", True)
    assert line.startswith("curve_summary_prior: n=5  c0 peak=0 t_peak=1 auc=4 p_cross=7.000 t_hit=6") and " c2 peak=" in line
    assert "p_cross" not in m.summary_line(mean, "post", False)


def test_training_entry_points_take_the_flag():
    import inspect
    from structured_latent_odes_amd import training as TR
    sig = inspect.signature(TR.train).parameters
    assert sig["curve_summary"].default == 0 and sig["summary_thresholds"].default is None and sig["summary_sense"].default == "above"
    a = TR.build_parser().parse_args(["--curve-summary", "64", "--summary-thresholds", "0.5,1,2.5", "--summary-sense", "below"])
    assert (a.curve_summary, a.summary_thresholds, a.summary_sense) == (64, [0.5, 1.0, 2.5], "below")
    d = TR.build_parser().parse_args([])
    assert (d.curve_summary, d.summary_thresholds, d.summary_sense) == (0, None, "above")
