"""CPU tests of the forecast summaries: the C ABI of slode_forecast_summary / slode_forecast_summary_plan, the plan against a hand count of
the kernel's carve (which has no num_samples term), the refusal ladder on a hand-filled handle
(tests/forecast_summary_refusals/forecast_summary_refusals.cpp), the numpy restatement of the kernel's order -- row walk, combine, per-window
merge -- against the fp64 functionals and against itself across windows, the `since` rule, and the Python layer on an engine double (the
dict, the composed route on status -1 alone, the files, the training flag)."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import draws_ladder_util as DL
from tests import forecast_summary_util as FSU
from tests import lds_util as LU
from tests import recon_moments_util as RU
from tests import summary_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 160 * 1024
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "is_post", "num_samples", "times_out", "stage_t_out", "T_out", "first_point", "window",
        "thr", "sense", "mean", "sd", "workspace", "workspace_bytes", "stream"]


# ---- header and exports --------------------------------------------------------------------------------------------------------------------
def test_abi_exports_forecast_summary_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_forecast_summary", "slode_forecast_summary_plan"):
        assert hasattr(lib, name) and name in L.EXPORTS
    version = re.search(r"#define\s+SLODE_VERSION\s+(\d+)\s*/\*(.*?)\*/", hdr)
    assert int(version.group(1)) == lib.slode_version() == 290 and "slode_forecast_summary, slode_forecast_summary_plan" in version.group(2)
    m = re.search(r"int\s+slode_forecast_summary\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_forecast_summary.argtypes
    assert len(at) == len(ARGS) and all(at[i] is C.c_int for i in (7, 8, 11, 12, 13, 15)) and at[19] is C.c_size_t
    assert re.search(r"int\s+slode_forecast_summary_plan\s*\(\s*const slode_shape\*\s*s,\s*int T_out,\s*int window,\s*int\*\s*window_out,\s*size_t\*\s*lds_bytes\s*\)\s*;", hdr)
    doc = re.sub(r"\s*\n \*\s*", " ", hdr[hdr.index("forecast summaries:"):m.start()])      # (the comment's line breaks are not the text's)
    for word in ("no num_samples term", "POPULATION", "first_point", "one-point sub-grid gives 0", "already beyond at first_point", "NaN where none crosses",
                 "no p_beyond[T_out] output", "ONE drawing call", '"forecast_summary"', "draws outer, windows inner", "strict improvement",
                 "bit for bit slode_curve_summary's", "SLODE_EINVAL", "the plan's refusal", "capturable"):
        assert word in doc, word
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_FORECAST_SUMMARY_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_forecast_summary_lds_bytes" in common
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "forecast_summary_kernel.hip" in srcs
    assert "slode_forecast_summary" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    profile_doc = hdr[:hdr.index("int slode_profile_read(")]
    assert '"forecast_summary"' in profile_doc[profile_doc.rindex("/*"):]                  # the launch name is documented at slode_profile_read
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_forecast_summary(*([None] * 7), 1, 8, None, None, 50, 0, 0, None, 1, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_engine_signatures():
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.forecast_summary).parameters) == [
        "self", "params", "batch", "B", "is_post", "num_samples", "times_out", "first_point", "thr", "sense", "mean", "sd", "window"]
    d = {k: p.default for k, p in inspect.signature(Engine.forecast_summary).parameters.items()}
    assert (d["first_point"], d["thr"], d["sense"], d["mean"], d["sd"], d["window"]) == (0, None, 1, None, None, 0)
    assert list(inspect.signature(Engine.forecast_summary_plan).parameters) == ["self", "T_out", "window"]         # no num_samples, no B


# ---- the plan, by hand count ---------------------------------------------------------------------------------------------------------------
def _pieces(eng, W):
    """Floats of every LDS piece of the kernel for a window of W steps, each rounded up to four: the staged weights of the shared forward
    pieces (everything but their step table), loc | scale, ONE carry [S], the window's step table 2 W S, its grid and node weights W + 1
    each, its values Q C (W + 1), the moment triples 3 Q C 8.  Nothing is sized by num_samples or by T_out."""
    sp = eng.spec
    S, QC = sp.ode_state_dim, (1 if sp.gauss else 3) * sp.n_channels
    staged = LU.fwd_shared_pieces(eng.T, S, sp.n_channels, sp.latent_dim, sp.ode_hidden_dim, sp.n_u, sp.gauss)[2:]
    return staged + [LU.r4(n) for n in (sp.latent_dim, sp.latent_dim, S, W * S, W * S, W + 1, W + 1, QC * (W + 1), 3 * QC * 8)]


def _hand_bytes(eng, W):
    return 4 * sum(_pieces(eng, W))


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald", "cvs_gauss", "proc_gauss"])
def test_plan_against_a_hand_count_of_the_carve(case):
    eng = LU.host_engine(case)
    fits = lambda W: _hand_bytes(eng, W) <= BUDGET                                        # noqa: E731
    # a grid that fits in one window: the whole grid
    assert eng.forecast_summary_plan(400, 0) == (399, _hand_bytes(eng, 399)) and fits(399)
    assert eng.forecast_summary_plan(2, 0) == (1, _hand_bytes(eng, 1))
    # T_out = 2^20: the largest multiple of 256 steps that fits
    W, nbytes = eng.forecast_summary_plan(1 << 20, 0)
    assert W % 256 == 0 and W >= 256 and nbytes == _hand_bytes(eng, W) and fits(W) and not fits(W + 256)
    # an explicit window is honoured, and clamped to T_out - 1
    assert eng.forecast_summary_plan(4096, 77) == (77, _hand_bytes(eng, 77))
    assert eng.forecast_summary_plan(50, 1 << 20) == (49, _hand_bytes(eng, 49))
    for W in (1, 13, 49, 77, 256, 399):
        assert all(4 * n % 16 == 0 for n in _pieces(eng, W))
    # one more step costs its two step-table rows, its time, its weight and its values (W = 4 -> 8: every piece stays a multiple of 16 B)
    sp = eng.spec
    QC = (1 if sp.gauss else 3) * sp.n_channels
    assert eng.forecast_summary_plan(4096, 8)[1] - eng.forecast_summary_plan(4096, 4)[1] == 4 * 4 * (2 * sp.ode_state_dim + 2 + QC)


def test_plan_in_numbers_and_its_refusals():
    """cvs ALD (S 5, C 3, three heads): 21 floats per step; T_out = 400 in one window is 38,496 B.  proc ALD (S 8, C 4): 30 floats per step."""
    from structured_latent_odes_amd import _lib as L
    cvs, proc = LU.host_engine("cvs_ald"), LU.host_engine("proc_ald")
    assert _pieces(cvs, 399)[-9:] == [8, 8, 8, 1996, 1996, 400, 400, 3600, 216]
    assert _pieces(proc, 399)[-6:] == [3192, 3192, 400, 400, 4800, 288]
    for eng, name in ((cvs, "cvs"), (proc, "proc")):
        print("%s: T_out 400 one window %d B; default window at T_out 2^20: %d steps, %d B" % ((name, eng.forecast_summary_plan(400, 0)[1]) + eng.forecast_summary_plan(1 << 20, 0)))
    with pytest.raises(L.SlodeError, match=r"slode_forecast_summary_plan: window = 30000 does not fit.*S = 5, C = 3 \(%d B" % _hand_bytes(cvs, 30000)):
        cvs.forecast_summary_plan(1 << 20, 30000)
    for bad, word in (((1, 0), "T_out = 1 out of range"), (((1 << 20) + 1, 0), "T_out = 1048577 out of range"), ((300, -1), "window = -1 < 0")):
        with pytest.raises(L.SlodeError, match=word):
            cvs.forecast_summary_plan(*bad)


# ---- the refusal ladder --------------------------------------------------------------------------------------------------------------------
_N = "slode_forecast_summary"
_P = "slode_forecast_summary_plan"
_ADVICE = "reduce forecast_samples instead"
_BOTH, _POST, _PLAN = DL.BOTH, DL.POST, DL.PLAN
_HEAD, _LABELS, _TWO = DL.shared_rungs(_N, "batch / times / stage_t / workspace", _ADVICE)
_UNFIT = [_N, "does not fit", "S = 5, C = 3", "staged weights, carry, step table, grid and node weights, value table, moment triples", "pass window = 0"]
LADDER = _HEAD + [
    ("times_out NULL", _BOTH, -1, [_N, "times_out / stage_t_out is NULL"]), ("stage_t_out NULL", _BOTH, -1, [_N, "times_out / stage_t_out is NULL"]),
    ("T_out 1", _BOTH, -1, [_N, "T_out = 1 out of range [2, 1048576]"]), ("T_out 2^20 + 1", _BOTH, -1, [_N, "T_out = 1048577 out of range"]),
    ("first_point -1", _BOTH, -1, [_N, "first_point = -1 out of range [0, T_out - 1 = 94]"]),
    ("first_point T_out", _BOTH, -1, [_N, "first_point = 95 out of range [0, T_out - 1 = 94]"]),
    ("first_point T_out - 1: taken so far; workspace too small", _BOTH, -3, DL.WS),
    ("sense 0", _BOTH, -1, [_N, "sense = 0"]), ("sense 2", _BOTH, -1, [_N, "sense = 2"]),
    ("thr[1] NaN", _BOTH, -1, [_N, "thr[1] = nan is not finite"]), ("thr[3] NaN beyond C = 3: not read; workspace too small", _BOTH, -3, DL.WS),
    ("mean NULL", _BOTH, -1, [_N, "mean is NULL"]), ("window -1", _BOTH, -1, [_N, "window = -1 < 0"]),
    ("LDS: window 30000 of T_out 2^20", _BOTH, -1, _UNFIT + ["window = 30000"]),
    ("LDS: window 2^20 clamped to T_out - 1 = 19999", _BOTH, -1, _UNFIT + ["window = 19999"]),
    ("num_samples 10000, T_out 2^20, window 0: fits; workspace too small", _BOTH, -3, DL.WS),
] + _LABELS[:-1] + [
    ("workspace too small", _BOTH, -3, DL.WS), ("sd and thr NULL, sense -1, first_point 0; workspace too small", _BOTH, -3, DL.WS),
] + _TWO + [                                                                          # two conditions at once: the earlier rung speaks
    ("no_fold + times_out NULL", _POST, -1, ["observation strides"]), ("times_out NULL + T_out 1", _BOTH, -1, ["times_out / stage_t_out is NULL"]),
    ("T_out 1 + first_point -1", _BOTH, -1, ["T_out = 1 out of range"]), ("first_point -1 + sense 0", _BOTH, -1, ["first_point = -1"]),
    ("sense 0 + thr[0] NaN", _BOTH, -1, ["sense = 0"]), ("thr[0] NaN + mean NULL", _BOTH, -1, ["thr[0] = nan"]),
    ("mean NULL + window -1", _BOTH, -1, ["mean is NULL"]), ("window -1 + label columns 3", _BOTH, -1, ["window = -1"]),
    ("unfit window + label columns 3", _BOTH, -1, ["window = 19999 does not fit"]),
    ("label columns 3 + workspace too small", _BOTH, -1, ["label tensors have 3 columns"]),
    # the plan
    ("shape NULL", _PLAN, -1, [_P, "shape is NULL"]), ("bad shape", _PLAN, -1, [_P, "T out of range"]),
    ("window_out NULL", _PLAN, -1, [_P, "window_out / lds_bytes is NULL"]), ("lds_bytes NULL", _PLAN, -1, [_P, "window_out / lds_bytes is NULL"]),
    ("T_out 1", _PLAN, -1, [_P, "T_out = 1 out of range"]), ("T_out 2^20 + 1", _PLAN, -1, [_P, "T_out = 1048577 out of range"]),
    ("window -1", _PLAN, -1, [_P, "window = -1 < 0"]), ("LDS: window 30000 of T_out 2^20", _PLAN, -1, [_P, "window = 30000 does not fit"]),
]


def test_forecast_summary_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_forecast_summary and of slode_forecast_summary_plan without a device, in rung order: status, the
    words of the message and the untouched drawing-call counter against LADDER; line by line against
    tests/golden/forecast_summary_refusals.txt; the rungs shared with slode_recon_moments carry the texts tests/golden/eval_refusals.txt
    records for it, the call's name, its list of required pointers and its advice apart; the call's LDS figure is the plan's; and the memory
    that stands for the outputs untouched."""
    _, shared, figures = DL.check_ladder("forecast_summary_refusals", tmp_path, LADDER, _N, _ADVICE)
    assert all(len(v) == 1 for v in figures.values()), figures                          # both sides and the plan name the same bytes
    assert shared >= 40


# ---- the numpy restatement of the kernel's order -----------------------------------------------------------------------------------------------
def _smooth(N, Cn, T, seed):
    """[N, C, T] fp32 random smooth curves on an uneven increasing grid [T] fp32: three sines of random phase and a drift."""
    r = np.random.RandomState(seed)
    t = np.cumsum(r.uniform(0.05, 0.2, T)).astype(np.float32)
    ph, am, fr = r.uniform(0, 6.28, (3, N, Cn, 1)), r.uniform(0.2, 1.5, (3, N, Cn, 1)), r.uniform(0.3, 2.0, (3, N, Cn, 1))
    v = sum(am[i] * np.sin(fr[i] * t + ph[i]) for i in range(3)) + r.uniform(-0.05, 0.05, (N, Cn, 1)) * t
    return RU._f32(v), t


@pytest.mark.parametrize("T,i0,W", [(50, 0, 0), (50, 17, 16), (50, 49, 7), (300, 123, 70), (300, 0, 0), (40, 13, 13), (40, 14, 13), (2, 1, 1), (2, 0, 1),
                                     (95, 85, 1)])
def test_restatement_against_the_fp64_functionals(T, i0, W):
    """On random smooth curves the restatement -- fma chains per lane, four combine steps, per-window merge -- agrees with SU.functionals in
    fp64 on the sub-grid: the selection slots exactly (smooth random curves have no exact ties), the two sums within SU.sum_bars (the order of
    a sum of T terms moves it by at most (T + 1) u sum |term|, the windows' partial sums included)."""
    v, t = _smooth(6, 3, T, seed=T + i0)
    thr = RU._f32(np.median(v[..., i0:], axis=(0, 2)))
    for sense in (1, -1):
        got = FSU.restatement(v, t, i0, W, thr, sense).astype(np.float64)
        sub = v[..., i0:]
        want = SU.functionals(sub, t[i0:], thr, sense, w=FSU.weights_from(t, i0)[i0:])
        assert np.array_equal(FSU.weights_from(t, i0)[i0:], SU.weights_f32(t[i0:]))      # the sub-grid's own trapezoid weights, bit for bit
        for slot in (0, 1, 2, 3, 6, 7):
            assert np.array_equal(got[..., slot], want[..., slot], equal_nan=True), (SU.NAMES[slot], sense)
        bar_auc, bar_tb = SU.sum_bars(sub, t[i0:])
        assert np.all(np.abs(got[..., 4] - want[..., 4]) <= bar_auc + 1e-45) and np.all(np.abs(got[..., 5] - want[..., 5]) <= bar_tb + 1e-45)
    bare = FSU.restatement(v, t, i0, W)
    assert np.isnan(bare[..., 5:]).all() and np.array_equal(bare[..., :5], FSU.restatement(v, t, i0, W, thr, 1)[..., :5])
    if i0 == T - 1:
        assert np.all(got[..., 4] == 0.0) and np.array_equal(got[..., 0], got[..., 2])    # a one-point sub-grid: no area, peak == trough


def test_merge_is_window_invariant_on_planted_ties():
    """Curves whose extreme and whose first crossing are attained at several points on both sides of window boundaries: the selection slots
    of the restatement are EXACTLY those of one window for every window, and the earliest point wins."""
    T, i0 = 50, 5
    t = np.linspace(0.0, 4.9, T).astype(np.float32)
    v = np.zeros((2, 1, T), np.float32)
    v[0, 0, [3, 7, 8, 15, 16, 17, 32, 33, 49]] = 2.0        # the maximum at 7 (3 lies before i0), again at the slots around W = 8 / 16 / 32
    v[0, 0, [4, 12, 24, 25, 48]] = -1.0                    # the minimum first at 12
    v[1, 0, :] = 1.0                                       # every point ties
    thr = np.array([1.5], np.float32)
    one = FSU.restatement(v, t, i0, 0, thr, 1)
    assert one[0, 0].tolist()[:4] == [2.0, float(t[7]), -1.0, float(t[12])] and float(one[0, 0, 6]) == float(t[7]) and float(one[0, 0, 7]) == 1.0
    assert one[1, 0].tolist()[:4] == [1.0, float(t[5]), 1.0, float(t[5])] and np.isnan(one[1, 0, 6]) and float(one[1, 0, 7]) == 0.0
    for W in (1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 32, 48, 49):
        got = FSU.restatement(v, t, i0, W, thr, 1)
        for slot in (0, 1, 2, 3, 6, 7):
            assert np.array_equal(got[..., slot], one[..., slot], equal_nan=True), (W, SU.NAMES[slot])
    # the points a window walks: window 0 owns point 0, window w > 0 the points n_lo + 1 .. n_hi; every point at or beyond i0 exactly once
    for W in (1, 7, 16, 49, 0):
        pts = [g for lo, hi in FSU.window_points(T, W, i0) for g in range(lo, hi)]
        assert pts == list(range(i0, T)), W
    assert FSU.window_points(50, 16, 0) == [(0, 17), (17, 33), (33, 49), (49, 50)] and FSU.window_points(50, 16, 33) == [(33, 49), (49, 50)]
    assert FSU.window_points(50, 16, 32) == [(32, 33), (33, 49), (49, 50)]


def test_row_walk_keeps_its_sentinels_in_short_windows():
    """Windows of fewer than 16 points leave lanes without a point: their (-inf / +inf, n) sentinels lose every combine step, the idle lanes
    add exact zeros, and a window that does not cross leaves ihit at n."""
    w = np.array([0.5, 1.0, 0.25], np.float32)
    r = FSU.row_walk(np.array([[1.0, 3.0, 3.0], [-2.0, -2.0, -5.0]], np.float32), w, np.array([2.0, 0.0], np.float32), 1)
    assert r["vmax"].tolist() == [3.0, -2.0] and r["imax"].tolist() == [1, 0] and r["vmin"].tolist() == [1.0, -5.0] and r["imin"].tolist() == [0, 2]
    assert r["ihit"].tolist() == [1, 3] and r["tb"].tolist() == [1.25, 0.0] and r["auc"].tolist() == [4.25, -4.25]
    one = FSU.row_walk(np.array([[7.0]], np.float32), np.array([0.0], np.float32), None, 1)
    assert (one["vmax"][0], one["imax"][0], one["vmin"][0], one["imin"][0], one["auc"][0]) == (7.0, 0, 7.0, 0, 0.0)


# ---- since -> first_point --------------------------------------------------------------------------------------------------------------------
def test_since_gives_the_first_point_that_has_reached_it():
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase as M
    up = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.5])
    assert [M._first_point(up, s) for s in (None, 0.0, -3.0, 0.25, 0.5, 1.0, 1.01, 2.5)] == [0, 0, 0, 1, 1, 2, 3, 4]
    down = torch.tensor([2.0, 1.0, 0.5, -1.0])
    assert [M._first_point(down, s) for s in (None, 2.0, 5.0, 1.5, 1.0, 0.0, -1.0)] == [0, 0, 0, 1, 1, 3, 3]
    for grid, s in ((up, 2.51), (down, -1.5)):
        with pytest.raises(ValueError, match="beyond the output grid"):
            M._first_point(grid, s)
    assert M._first_point(up.tolist(), 1.0) == 2 and M._first_point(up.double(), np.float32(1.5)) == 3
    for grid in (up, down):
        for s in (None, float(grid[2]), float(grid[-1])):
            assert M._first_point(grid, s) == FSU.first_point(grid.numpy(), s)
    assert "synchronises" in M.forecast_summary.__doc__ and "cohort_index" in M.forecast_summary.__doc__


# ---- the Python layer on an engine double ------------------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self, refuse, Q):
        self.refuse, self.Q, self.calls, self.batches, self.draws, self.counter = refuse, Q, [], [], [], 10

    def draw_normal(self, rows):
        self.draws.append(rows)
        self.counter += 1
        return torch.linspace(-1.0, 1.0, rows * 4).view(rows, 4)

    def rng_state(self):
        return (0, 0, self.counter)

    def make_batch(self, obs, labels, eps=None, particles=1):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def forecast_summary(self, flat, bt, B, is_post, num_samples, times_out, first_point=0, thr=None, sense=1, mean=None, sd=None, window=0):
        from structured_latent_odes_amd import _lib as L
        self.calls.append((B, bool(is_post), num_samples, int(times_out.numel()), first_point, thr, sense, mean, sd, window))
        if self.refuse:
            err = L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        self.counter += 1
        f = torch.arange(8, dtype=torch.float32).view(1, 1, 1, 8) + 10.0 * torch.arange(self.Q, dtype=torch.float32).view(self.Q, 1, 1, 1) + torch.zeros(self.Q, B, 3, 8)
        return f, f + 0.5


def _double(gauss, refuse):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        LABELS, GAUSS = ("iext",), gauss

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3), "flat": torch.zeros(1)})()
            self.times = torch.tensor([0.0, 1.0, 3.0, 4.0])
            self.device = torch.device("cpu")
            self.sampled = []

        def _bind(self):
            return self._b

        def forecast_samples(self, observations, is_post, num_samples, times_out, eps=None, states=False, **labels):
            """(t - 4)^2 / 4 - eps[., ., 0] on channel 0, its negative on channel 1, the row index on channel 2 (+ 100 per head)."""
            B = observations.shape[0]
            self.sampled.append((B, bool(is_post), num_samples, int(times_out.numel()), tuple(eps.shape)))
            e = eps[:, :, 0].permute(1, 0).reshape(B, 1, 1, num_samples)
            base = ((times_out - 4.0) ** 2 / 4.0).view(1, 1, -1, 1) - e
            v = torch.cat([base, -base, observations[:, :1, :1].reshape(B, 1, 1, 1).expand_as(base)], 1)
            return dict({n: v + 100.0 * i for i, n in enumerate(("mean",) if gauss else ("mu_50", "mu_75", "mu_25"))}, z=None)

    return M()


OBS = torch.arange(7, dtype=torch.float32).view(7, 1, 1).expand(7, 3, 4).contiguous()
LAB = torch.zeros(7, 1)


@pytest.mark.parametrize("gauss", [False, True])
def test_model_level_call_uses_the_engine(gauss):
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, 0)
    eng = m._b.engine
    t_out = m.horizon_times(4)                                                           # 0 1 3 4 | 5 6 7 8
    res = m.forecast_summary(OBS, True, 5, t_out, since=4.0, thresholds=torch.tensor([1.0, 2.0, 3.0]), sense="below", window=3, iext=LAB)
    assert eng.calls == [(7, True, 5, 8, 3, [1.0, 2.0, 3.0], -1, None, True, 3)] and eng.batches == [((7, 3, 4), 1, None, 5)]
    assert eng.draws == [] and eng.counter == 11 and m.sampled == [] and set(res) == set(names)
    for q, n in enumerate(names):
        assert set(res[n]) == set(SU.NAMES) | {"first_point"} and res[n]["first_point"] == 3
        for j, k in enumerate(SU.NAMES):
            mean, sd = res[n][k]
            assert tuple(mean.shape) == tuple(sd.shape) == (7, 3) and float(mean[0, 0]) == 10.0 * q + j and float(sd[0, 0]) == 10.0 * q + j + 0.5
    m.forecast_summary(OBS, False, 5, t_out, eps=torch.zeros(5, 7, 4), iext=LAB)         # since None: 0; no thresholds: None reaches the engine
    assert eng.calls[-1] == (7, False, 5, 8, 0, None, 1, None, True, 0) and eng.batches[-1] == ((7, 3, 4), 1, (5, 7, 4), 5)
    n_calls = len(eng.calls)
    for bad, match in ((dict(since=8.5), "beyond the output grid"), (dict(sense="up"), "sense"), (dict(thresholds=[1.0, 2.0]), "one per channel"),
                       (dict(num_samples=0), "num_samples"), (dict(times_out=t_out[1:]), "first time")):
        kw = dict(dict(is_post=True, num_samples=5, times_out=t_out), **bad)
        with pytest.raises(ValueError, match=match):
            m.forecast_summary(OBS, iext=LAB, **kw)
    assert len(eng.calls) == n_calls and eng.draws == []                                 # the ValueErrors come before any engine call


@pytest.mark.parametrize("gauss", [False, True])
def test_composed_route_on_a_refusal(gauss, monkeypatch):
    """The engine refuses (status -1): one drawing call for the whole batch, forecast_samples per chunk, the functionals in torch on
    times_out[first_point:] -- equal to SU.functionals on the same curves sliced the same way -- independent of the chunking."""
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, -1)
    eng = m._b.engine
    t_out = m.horizon_times(4)
    thr = [0.5, -0.5, 2.5]
    res = m.forecast_summary(OBS, True, 5, t_out, since=3.5, thresholds=thr, sense="above", iext=LAB)
    assert len(eng.calls) == 1 and eng.draws == [35] and m.sampled == [(7, True, 5, 8, (5, 7, 4))]
    eps = torch.linspace(-1.0, 1.0, 35 * 4).view(5, 7, 4)
    curves = m.forecast_samples(OBS, True, 5, t_out, eps=eps, iext=LAB)
    tt = t_out.numpy()
    for n in names:
        assert res[n]["first_point"] == 3
        f = SU.functionals(curves[n][:, :, 3:].permute(3, 0, 1, 2).numpy(), tt[3:], np.array(thr, np.float32), 1)
        wm, ws = SU.oracle_moments(f)
        for j, k in enumerate(SU.NAMES):
            gm, gs = (x.double().numpy() for x in res[n][k])
            assert np.allclose(gm, wm[..., j], rtol=1e-5, atol=1e-5, equal_nan=True) and np.allclose(gs, ws[..., j], rtol=1e-4, atol=1e-4, equal_nan=True), (n, k)
    r = res[names[0]]
    # channel 2 is the row index, constant in time: it crosses 2.5 from row 3 on, at the first point used; the area is the value times 8 - 4
    assert r["crossed"][0][:, 2].tolist() == [0.0] * 3 + [1.0] * 4 and r["t_hit"][0][3:, 2].tolist() == [4.0] * 4 and torch.isnan(r["t_hit"][0][:3, 2]).all()
    assert r["auc"][0][:, 2].tolist() == [4.0 * b for b in range(7)] and r["t_peak"][0][:, 2].tolist() == [4.0] * 7
    # channel 0 rises from t = 4 on: its peak is at the grid's end, its trough at the first point used
    assert r["t_peak"][0][:, 0].tolist() == [8.0] * 7 and r["t_trough"][0][:, 0].tolist() == [4.0] * 7
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)                                 # 15 // 5 = 3 rows per chunk: 3 + 3 + 1
    m.sampled.clear()
    chunked = m.forecast_summary(OBS, True, 5, t_out, since=3.5, thresholds=thr, sense="above", iext=LAB)
    assert [s[0] for s in m.sampled] == [3, 3, 1] and eng.draws == [35, 35]
    for n in names:
        for k in SU.NAMES:
            assert all(torch.equal(a.nan_to_num(nan=7e33), b.nan_to_num(nan=7e33)) for a, b in zip(chunked[n][k], res[n][k])), (n, k)
    none = m.forecast_summary(OBS, True, 5, t_out, iext=LAB)
    assert all(torch.isnan(none[n][k][0]).all() for n in names for k in ("time_beyond", "t_hit", "crossed")) and none[names[0]]["first_point"] == 0
    last = m.forecast_summary(OBS, True, 5, t_out, since=8.0, thresholds=thr, iext=LAB)   # one point: no area, peak == trough
    assert last[names[0]]["first_point"] == 7 and float(last[names[0]]["auc"][0].abs().max()) == 0.0
    assert torch.equal(last[names[0]]["peak"][0], last[names[0]]["trough"][0])


def test_summary_weights_take_a_grid_and_keep_todays_default():
    m = _double(False, 0)
    t, w = m._summary_weights(torch.device("cpu"))
    assert torch.equal(t, m.times) and w.tolist() == [0.5, 1.5, 1.5, 0.5]
    t2, w2 = m._summary_weights(torch.device("cpu"), grid=[1.0, 2.0, 4.0])
    assert t2.tolist() == [1.0, 2.0, 4.0] and w2.tolist() == [0.5, 1.5, 1.0]
    assert list(inspect.signature(type(m)._summary_weights).parameters) == ["self", "device", "grid"]


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.forecast_summary(OBS, True, 5, m.horizon_times(2), iext=LAB)
    assert m.sampled == [] and m._b.engine.draws == []


def test_save_forecast_summary_file_names_and_line(tmp_path):
    m = _double(False, 0)
    t_out = m.horizon_times(3)
    batches = [dict(observations=torch.zeros(B, 3, 4), iext=torch.zeros(B, 1)) for B in (2, 3)]
    for is_post in (True, False):
        files = m.save_forecast_summary(str(tmp_path / "r"), batches, is_post, 4, t_out, since=4.0, thresholds=[1.0, 2.0, 3.0], sense="below")
        tag = "post" if is_post else "prior"
        want = ["summary_%s_%s_forecast_%s.npy" % (n, tag, k) for n in ("mu_50", "mu_75", "mu_25") for k in ("mean", "sd")] + ["forecast_times.npy"]
        assert [os.path.basename(f) for f in files] == want
        mean, sd = np.load(files[0]), np.load(files[1])
        assert mean.shape == sd.shape == (5, 3, 8) and mean.dtype == np.float32 and mean[0, 0].tolist() == list(range(8)) and sd[4, 2, 0] == 0.5
        assert np.array_equal(np.load(files[-1]), t_out.numpy())
    assert len(os.listdir(str(tmp_path / "r"))) == 13 and all(c[4] == 3 and c[5] == [1.0, 2.0, 3.0] and c[6] == -1 for c in m._b.engine.calls)
    line = m.summary_line(mean, "mu_50", True, name="forecast_summary")
    assert line.startswith("forecast_summary_mu_50: n=5  c0 peak=0 ") and "p_cross=7.000 t_hit=6" in line
    assert m.summary_line(mean, "post", False).startswith("curve_summary_post: n=5")      # the default keeps today's line


def test_forecast_summary_flag_needs_forecast_steps(monkeypatch, tmp_path, capsys):
    from structured_latent_odes_amd import training as TR
    assert inspect.signature(TR.train).parameters["forecast_summary"].default == 0
    assert TR.build_parser().parse_args([]).forecast_summary == 0
    tr = importlib.import_module("training_cvs")
    with pytest.raises(ValueError, match="forecast_summary needs forecast_steps"):
        TR.train(None, "cvs", None, None, forecast_summary=3)
    seen = []
    monkeypatch.setattr(TR, "train", lambda config, family, a, b, n, **kw: seen.append(kw))
    monkeypatch.chdir(tmp_path)
    for argv in (["--forecast-summary", "3"], ["--forecast-summary", "3", "--forecast-steps", "0"]):
        with pytest.raises(SystemExit) as ei:
            TR.main(tr.FAMILY, tr.load_config, tr.MechanisticModel, tr.MechanisticModelGauss, argv=["--epochs", "1"] + argv)
        assert ei.value.code == 2 and "--forecast-summary needs --forecast-steps" in capsys.readouterr().err
    assert seen == []
    TR.main(tr.FAMILY, tr.load_config, tr.MechanisticModel, tr.MechanisticModelGauss,
            argv=["--epochs", "1", "--forecast-steps", "5", "--forecast-summary", "3", "--summary-thresholds", "0.5,1,2.5", "--summary-sense", "below"])
    TR.main(tr.FAMILY, tr.load_config, tr.MechanisticModel, tr.MechanisticModelGauss, argv=["--epochs", "1", "--forecast-steps", "5"])
    assert seen == [{"fused_stats": False, "forecast_steps": 5, "forecast_summary": 3, "summary_thresholds": [0.5, 1.0, 2.5], "summary_sense": "below"},
                    {"fused_stats": False, "forecast_steps": 5}]
    for script in ("training_cvs.py", "training_challenge.py", "training_proc.py"):
        assert "main(" in open(os.path.join(ROOT, script)).read()                           # the three entry points run training.main: its parser
