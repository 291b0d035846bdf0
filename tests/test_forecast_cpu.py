"""CPU tests of the forecast moments (slode_forecast_moments and its neighbours): the header and the exports, the window plan against a
hand count of the LDS pieces, the refusal ladder on a hand-filled handle (tests/forecast_refusals/forecast_refusals.cpp), the numpy
restatement of a solve walked in windows, the conditioning of every (case, T_out, solver) the GPU tests solve, and the model-level calls
on an engine double."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import forecast_util as FU
from tests import lds_util as LU
from tests import recon_moments_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 160 * 1024


# ---- header and exports --------------------------------------------------------------------------------------------------------------
def test_header_version_and_exports():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    version = int(re.search(r"#define SLODE_VERSION (\d+)", hdr).group(1))
    lib = L.load()
    assert version == lib.slode_version() >= 180
    assert "0.1.8" in hdr and re.search(r"#define SLODE_FORECAST_MAX_T \(1 << 20\)", hdr) and L.FORECAST_MAX_T == 1 << 20
    for name in ("slode_stage_times_n", "slode_num_stage_times_n", "slode_forecast_plan", "slode_forecast_moments"):
        assert hasattr(lib, name) and name in L.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr), name
    assert "\"forecast_moments\"" in hdr                                                # the name list of slode_profile_read


# ---- the plan, by hand count ---------------------------------------------------------------------------------------------------------
def _shape(proc=False, **kw):
    """The metric shape (cvs: S 5, C 3, three heads, L 8, H 25) or the proc shape (S 8, C 4, three heads, L 50)."""
    from structured_latent_odes_amd import _lib as L
    d = dict(B=4, T=200, C=3, L=8, S=5, H=25, F=10, K=10, P=5, Hc=50, n_u=2, n_groups=2, method=L.RK4, likelihood=L.ALD,
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


def _pieces(s, ns, states, W):
    """Floats of every LDS piece of the kernel for a window of W steps, counted from the issue's map: each rounded up to 4 floats."""
    Q = 1 if s.likelihood == 1 else 3
    staged = LU.fwd_shared_pieces(s.T, s.S, s.C, s.L, s.H, s.n_u, s.likelihood == 1)[2:]    # (the step table is the window's: below)
    window = [W * s.S, W * s.S, 3 * Q * s.C * (W + 1)] + ([3 * s.S * (W + 1)] if states else [])
    return staged + [LU.r4(n) for n in [s.L, s.L, ns * s.S] + window]              # loc | scale, carry[ns][S], the window's tables


def _hand_bytes(s, ns, states, W):
    return 4 * sum(_pieces(s, ns, states, W))


def _plan(s, T_out, ns, states, window):
    from structured_latent_odes_amd import _lib as L
    lib = L.load()
    w, nbytes = C.c_int(-1), C.c_size_t(0)
    rc = lib.slode_forecast_plan(C.byref(s), T_out, ns, int(states), window, C.byref(w), C.byref(nbytes))
    return rc, w.value, nbytes.value, (lib.slode_last_error(None) or b"").decode()


@pytest.mark.parametrize("proc", [False, True])
def test_plan_matches_the_hand_count(proc):
    s = _shape(proc)
    ns = 64
    for states in (False, True):
        # the training grid's length: one window
        rc, W, nbytes, _ = _plan(s, 200, ns, states, 0)
        assert (rc, W, nbytes) == (0, 199, _hand_bytes(s, ns, states, 199)) and nbytes <= BUDGET
        # T_out = 4096: the largest multiple of 256 steps that fits
        rc, W, nbytes, _ = _plan(s, 4096, ns, states, 0)
        assert rc == 0 and W % 256 == 0 and 256 <= W < 4095, W
        assert nbytes == _hand_bytes(s, ns, states, W) <= BUDGET < _hand_bytes(s, ns, states, W + 256)
        # an explicit window is honoured, and clamped to T_out - 1
        assert _plan(s, 4096, ns, states, 77)[:3] == (0, 77, _hand_bytes(s, ns, states, 77))
        assert _plan(s, 50, ns, states, 1 << 20)[:3] == (0, 49, _hand_bytes(s, ns, states, 49))
        assert _plan(s, 2, 1, states, 0)[:3] == (0, 1, _hand_bytes(s, 1, states, 1))
        # every piece is a multiple of 16 B, at every window the plan can hand out
        for W in (1, 49, 77, 199, 256):
            assert all(4 * n % 16 == 0 for n in _pieces(s, ns, states, W)) and _hand_bytes(s, ns, states, W) % 16 == 0
    # the hand count of the metric shape itself, once, in numbers: W = 199, ns = 64, no states
    if not proc:
        assert _pieces(s, 64, False, 199) == [300, 400, 52, 132, 48, 12, 8, 4, 28, 8, 8, 8, 320, 996, 996, 5400]


def test_plan_steps_down_to_64_and_to_single_steps_and_refuses_by_name():
    s = _shape(True)
    # a carry table that leaves room for fewer than 256 steps, then for fewer than 64 (proc: 2 W S + 3 Q C (W + 1) = 52 W + 36 floats)
    fits = lambda ns, W: _hand_bytes(s, ns, False, W) <= BUDGET
    ns = 4000
    while not (fits(ns, 64) and not fits(ns, 256)):
        ns += 50
        assert ns < 6000
    rc, W, nbytes, _ = _plan(s, 4096, ns, False, 0)
    assert rc == 0 and W % 64 == 0 and 64 <= W < 256 and fits(ns, W) and not fits(ns, W + 64) and nbytes == _hand_bytes(s, ns, False, W)
    while not (fits(ns, 1) and not fits(ns, 64)):
        ns += 10
        assert ns < 6000
    rc, W, nbytes, _ = _plan(s, 4096, ns, False, 0)
    assert rc == 0 and 1 <= W < 64 and fits(ns, W) and not fits(ns, W + 1), W
    # not one step beside the carry: refused, naming num_samples
    rc, _, _, why = _plan(s, 4096, 6000, False, 0)
    assert rc == -1 and "num_samples = 6000" in why and "carry" in why
    # an explicit window whose tables do not fit: refused, naming the window
    rc, _, _, why = _plan(_shape(), 5000, 64, True, 4000)
    assert rc == -1 and "window = 4000 does not fit" in why
    for bad, word in ((dict(T_out=1), "T_out = 1"), (dict(T_out=(1 << 20) + 1), "T_out"), (dict(ns=0), "num_samples = 0"), (dict(window=-1), "window = -1")):
        kw = dict(T_out=300, ns=4, window=0)
        kw.update(bad)
        rc, _, _, why = _plan(_shape(), kw["T_out"], kw["ns"], False, kw["window"])
        assert rc == -1 and word in why, (bad, why)


def test_num_stage_times_n():
    from structured_latent_odes_amd import _lib as L
    lib = L.load()
    for method, R in ((L.EULER, 1), (L.MIDPOINT, 2), (L.RK4, 3)):
        s = _shape(method=method)
        assert lib.slode_num_stage_times_n(C.byref(s), 200) == lib.slode_num_stage_times(C.byref(s)) == R * 199 + 1
        assert lib.slode_num_stage_times_n(C.byref(s), 1 << 20) == R * ((1 << 20) - 1) + 1
        assert lib.slode_num_stage_times_n(C.byref(s), 1) == -1 and lib.slode_num_stage_times_n(C.byref(s), (1 << 20) + 1) == -1


# ---- the refusal ladder ----------------------------------------------------------------------------------------------------------------
def test_forecast_refusals_match_the_recorded_ladder(tmp_path):
    """Every refusing configuration of slode_forecast_moments (posterior and prior) and of slode_stage_times_n on a hand-filled handle: no
    device, no HIP call, no call that would be taken.  Status, message and the untouched drawing-call counter, line by line against
    tests/golden/forecast_refusals.txt -- which check speaks first when two conditions hold included."""
    from tests.refusals_util import refusal_lines
    got = refusal_lines("forecast_refusals", tmp_path)
    want = open(os.path.join(ROOT, "tests", "golden", "forecast_refusals.txt")).read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d:\n  got  %s\n  want %s" % (i + 1, g, w)
    assert len(got) == len(want) and len(want) > 90
    for line in got:
        name, status, counter, _ = line.split(" | ", 3)
        assert counter == "7" and int(status) < 0, line                                  # refused, and nothing drawn
    # the rungs shared with slode_recon_moments carry its recorded texts, the call's name apart
    recon = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "eval_refusals.txt")).read().splitlines():
        case, call, status, _, msg = line.split(" | ", 4)
        if call == "recon_moments":
            recon[case] = (status, msg.replace("slode_recon_moments", "slode_forecast_moments").replace("recon_samples", "forecast_samples"))
    mine = {l.split(" | ", 3)[0]: (l.split(" | ", 3)[1], l.split(" | ", 3)[3]) for l in got}
    for case in ("handle NULL", "shape NULL", "layout NULL", "params NULL", "bad shape", "draws 0", "draws 2^30", "adaptive method 3", "particles 2",
                 "fold_on", "ode_pack", "ode_alg", "obs NULL", "padded strides", "no_fold", "label columns 3, n_u 2", "workspace too small"):
        assert mine["post: " + case] == recon[case], case


# ---- a solve walked in windows -----------------------------------------------------------------------------------------------------------
def _steps(ns=6, n_steps=137, S=5, seed=5):
    """Affine steps like the solver's: A in (0.9, 1), b in (0, 0.1), x0 in (0, 1); fp64."""
    g = np.random.default_rng(seed)
    return 1.0 - 0.1 * g.random((ns, n_steps, S)), 0.1 * g.random((ns, n_steps, S)), g.random((ns, S))


@pytest.mark.parametrize("W", [1, 13, 19, 64, 136, 137, 500])
def test_windowed_solve_equals_the_unwindowed_one(W):
    """Windows outer, draws inner, only the carry kept: in fp64 the curves are those of the plain recurrence exactly (the same operations
    in the same order per draw); in fp32 against fp64 both forms sit within the same rounding bound: two roundings of at most 2^-24 relative per step, steps that contract
    (A < 1), so 2 n_steps 2^-24 of the level."""
    A, b, x0 = _steps()
    want = FU.affine_solve(A, b, x0)
    got = FU.windowed_solve(A, b, x0, W)
    assert not np.isnan(got).any() and np.array_equal(got, want)
    A32, b32, x32 = (v.astype(np.float32) for v in (A, b, x0))
    ref = FU.affine_solve(A32.astype(np.float64), b32.astype(np.float64), x32.astype(np.float64))
    bound = 2 * A.shape[1] * 2.0 ** -24 * np.maximum(1.0, np.abs(ref).max())
    for form in (FU.affine_solve(A32, b32, x32), FU.windowed_solve(A32, b32, x32, W)):
        assert form.dtype == np.float32 and np.abs(form - ref).max() <= bound
    assert [hi - lo for lo, hi in FU.windows(39, 13)] == [13, 13, 13] and [hi - lo for lo, hi in FU.windows(39, 19)] == [19, 19, 1]


def test_shifted_moments_per_window_meet_the_accumulation_bars():
    """The running moments are kept per window (slot j of window w = time point w W + j) and written after the window's last draw: every
    (t, s) still sees the draws in the order k = 0 .. ns - 1, so the moments are those of the unwindowed curves and meet RU.accumulation_bars."""
    ns, W = 20, 19
    A, b, x0 = _steps(ns=ns, n_steps=39)
    curves = FU.windowed_solve(*(v.astype(np.float32) for v in (A, b, x0 * 1e-3 + 0.5)), W)       # x0 close together: sd << level
    mean = np.full(curves.shape[1:], np.nan, np.float32)
    sd = np.full_like(mean, np.nan)
    for lo, hi in FU.windows(39, W):
        pts = slice(0 if lo == 0 else lo + 1, hi + 1)
        mean[pts], sd[pts] = RU.shifted_moments_f32(curves[:, pts])
    whole = RU.shifted_moments_f32(curves)
    assert np.array_equal(mean, whole[0]) and np.array_equal(sd, whole[1])
    v64 = curves.astype(np.float64)
    want_mean, want_sd = v64.mean(0), v64.std(0)
    assert np.all(np.abs(v64 - v64[0]).max(0) <= RU.SPREAD * want_sd)
    bar_mean, bar_sd = RU.accumulation_bars(want_mean, want_sd, ns)
    assert np.all(np.abs(mean - want_mean) <= bar_mean) and np.all(np.abs(sd - want_sd) <= bar_sd)


# ---- the conditioning of the GPU cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,T_out,solver", FU.PARITY + FU.WINDOWS, ids=["%s-%s-%s" % (c, t or "T+9", s) for c, t, s in FU.PARITY + FU.WINDOWS])
def test_fp32_oracle_stays_within_a_quarter_of_the_bars(case, T_out, solver):
    """The oracle (O.solve_ode on times_out + F.linear heads) evaluated in fp32 against fp64, B = 3, ns = 3, posterior and prior: head
    values and states within 0.25 of the suite's bars, 1e-4 max(1, |mu|) for the mean and 2e-4 for the sd -- the bars of the GPU tests
    then measure the kernel, not the conditioning of the case."""
    c = FU.build(case, solver, B=3, ns=3, T_out=T_out)
    worst = 0.0
    for is_post in (True, False):
        want = FU.oracle_moments(c, is_post)
        got = FU.oracle_moments(c, is_post, dtype=torch.float32)
        for i in (0, 2):                                                                  # heads, states: (mean, sd) pairs
            scale = np.maximum(1.0, np.abs(want[i]))
            rm = float((np.abs(got[i] - want[i]) / (RU.MEAN_BAR * scale)).max())
            rs = float((np.abs(got[i + 1] - want[i + 1]) / (RU.SD_BAR * scale)).max())
            worst = max(worst, rm, rs)
    print("%s T_out = %d %s: fp32 oracle error / bar %.3f" % (case, c["T_out"], solver, worst))
    assert worst <= 0.25


# ---- model level, on an engine double ----------------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self, refuse, Q, S=2):
        self.refuse, self.Q, self.S, self.fused, self.batches, self.draws, self.calls = refuse, Q, S, 0, [], [], []

    def draw_normal(self, rows):
        self.draws.append(rows)
        return torch.arange(rows * 4, dtype=torch.float32).view(rows, 4)

    def make_batch(self, obs, labels, eps=None, particles=1):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def forecast_moments(self, flat, bt, B, is_post, num_samples, times_out, states=False, window=0):
        from structured_latent_odes_amd import _lib as L
        self.fused += 1
        self.calls.append((B, bool(is_post), num_samples, int(times_out.numel()), bool(states), window))
        if self.refuse:
            err = L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        T = times_out.numel()
        q = torch.arange(self.Q, dtype=torch.float32).view(self.Q, 1, 1, 1)
        xs = torch.zeros(B, self.S, T) if states else None
        return q + torch.zeros(self.Q, B, 3, T), -q + torch.zeros(self.Q, B, 3, T), xs, xs


def _double(gauss, refuse, times=None):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        LABELS, GAUSS = ("iext",), gauss

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3), "flat": torch.zeros(1)})()
            self.times = torch.tensor([0.5, 1.0, 2.0, 2.5]) if times is None else times
            self.device = torch.device("cpu")
            self.sample_calls = []

        def _bind(self):
            return self._b

        def forecast_samples(self, observations, is_post, num_samples, times_out, eps=None, states=False, **labels):
            """Curves = row index + draw index (+ 100 per curve name): their moments are known in closed form."""
            B, T = observations.shape[0], times_out.numel()
            self.sample_calls.append((B, bool(is_post), num_samples, T, None if eps is None else tuple(eps.shape), labels["iext"].shape[0]))
            base = observations[:, :1, :1].reshape(B, 1, 1, 1) + torch.arange(num_samples, dtype=torch.float32).view(1, 1, 1, -1)
            names = ("mean",) if gauss else ("mu_75", "mu_50", "mu_25")
            res = {n: (base + 100.0 * i).expand(B, 3, T, num_samples) for i, n in enumerate(names)}
            if states:
                res["solution_xt"] = (base - 7.0).expand(B, T, 2, num_samples)
            return dict(res, z=None)

    return M()


def test_horizon_times():
    m = _double(False, 0)
    assert torch.equal(m.horizon_times(0), m.times)
    assert torch.allclose(m.horizon_times(3), torch.tensor([0.5, 1.0, 2.0, 2.5, 3.0, 3.5, 4.0]))
    assert torch.allclose(m.horizon_times(0, refine=2), torch.tensor([0.5, 0.75, 1.0, 1.5, 2.0, 2.25, 2.5]))
    assert torch.allclose(m.horizon_times(2, refine=2), torch.tensor([0.5, 0.75, 1.0, 1.5, 2.0, 2.25, 2.5, 2.75, 3.0]))
    t = m.horizon_times(5, refine=3)
    assert t.dtype == torch.float32 and t.numel() == 3 * 3 + 1 + 5 and float(t[0]) == 0.5 and bool((t[1:] > t[:-1]).all())
    assert torch.equal(t[:10:3], m.times)                                               # the training points stay exactly
    with pytest.raises(ValueError):
        m.horizon_times(-1)
    with pytest.raises(ValueError):
        m.horizon_times(1, refine=0)


@pytest.mark.parametrize("gauss", [False, True])
def test_model_level_call_uses_the_engine_and_falls_back_when_it_refuses(gauss, monkeypatch):
    obs = torch.arange(7, dtype=torch.float32).view(7, 1, 1).expand(7, 3, 4).contiguous()
    lab = torch.zeros(7, 1)
    heads = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, refuse=0)
    t_out = m.horizon_times(6)
    res = m.forecast_moments(obs, True, 5, t_out, states=True, window=3, iext=lab)
    assert set(res) == set(heads) | {"solution_xt"} and m.sample_calls == [] and m._b.engine.calls == [(7, True, 5, 10, True, 3)]
    assert m._b.engine.batches == [((7, 3, 4), 1, None, 5)]
    for q, n in enumerate(heads):                                                         # the engine's head order
        assert tuple(res[n][0].shape) == tuple(res[n][1].shape) == (7, 3, 10) and float(res[n][0][0, 0, 0]) == q and float(res[n][1][0, 0, 0]) == -q
    assert tuple(res["solution_xt"][0].shape) == tuple(res["solution_xt"][1].shape) == (7, 10, 2)
    assert set(m.forecast_moments(obs, False, 5, t_out, iext=lab)) == set(heads)
    # times_out must begin at the model's first time
    with pytest.raises(ValueError, match="first time"):
        m.forecast_moments(obs, True, 5, t_out[1:], iext=lab)
    with pytest.raises(ValueError, match="first time"):
        m._forecast_times(t_out + 0.25)                                                 # (the check forecast_samples makes too)
    with pytest.raises(ValueError, match="num_samples"):
        m.forecast_moments(obs, True, 0, t_out, iext=lab)
    # a refusal: the chunked composition from forecast_samples; explicit eps is sliced with the rows; the result does not depend on the chunks
    eps = torch.zeros(5, 7, 4)
    results = []
    for chunk_rows in (15, 10, 1 << 16):                                                  # 3 + 3 + 1 rows, 2 + 2 + 2 + 1, all 7
        m = _double(gauss, refuse=-1)
        monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", chunk_rows)
        results.append(m.forecast_moments(obs, False, 5, t_out, eps=eps, states=True, iext=lab))
        rows = max(1, chunk_rows // 5)
        assert m._b.engine.fused == 1 and [c[0] for c in m.sample_calls] == [min(rows, 7 - lo) for lo in range(0, 7, rows)]
        assert all(c[1:5] == (False, 5, 10, (5, c[0], 4)) and c[5] == c[0] for c in m.sample_calls)
    for res in results:
        assert set(res) == set(heads) | {"solution_xt"}
        for n in res:
            assert all(torch.equal(a, b) for a, b in zip(res[n], results[0][n]))
    for i, n in enumerate(("mean",) if gauss else ("mu_75", "mu_50", "mu_25")):
        mean, sd = results[0][n]
        assert tuple(mean.shape) == tuple(sd.shape) == (7, 3, 10) and mean.dtype == torch.float32
        assert torch.allclose(mean[:, 0, 0], torch.arange(7.0) + 2.0 + 100.0 * i)
        assert torch.allclose(sd, torch.full_like(sd, float(np.std(np.arange(5.0)))))
    assert tuple(results[0]["solution_xt"][0].shape) == (7, 10, 2) and torch.allclose(results[0]["solution_xt"][0][:, 0, 0], torch.arange(7.0) - 5.0)
    # no eps: ONE drawing call of ns * B rows for the whole batch
    m = _double(gauss, refuse=-1)
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)
    m.forecast_moments(obs, True, 5, t_out, iext=lab)
    assert m._b.engine.draws == [35] and [c[4] for c in m.sample_calls] == [(5, 3, 4), (5, 3, 4), (5, 1, 4)]


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.forecast_moments(torch.zeros(2, 3, 4), True, 5, m.horizon_times(2), iext=torch.zeros(2, 1))
    assert m.sample_calls == [] and m._b.engine.draws == []


def test_save_forecast_moments_file_names(tmp_path):
    m = _double(False, refuse=0)
    obs, t_out = torch.zeros(2, 3, 4), m.horizon_times(3)
    files = m.save_forecast_moments(str(tmp_path / "r"), obs, True, 4, t_out, iext=torch.zeros(2, 1))
    files += m.save_forecast_moments(str(tmp_path / "r"), obs, False, 4, t_out, iext=torch.zeros(2, 1))
    want = sorted(["%s_%s_forecast_%s.npy" % (c, p, k) for c in ("mu_50", "mu_75", "mu_25") for p in ("post", "prior") for k in ("mean", "sd")]
                  + ["forecast_times.npy"])
    assert sorted(set(os.path.basename(f) for f in files)) == want == sorted(os.listdir(str(tmp_path / "r")))
    assert all(np.load(f).shape == ((7,) if f.endswith("forecast_times.npy") else (2, 3, 7)) for f in files)
    assert np.array_equal(np.load(str(tmp_path / "r" / "forecast_times.npy")), t_out.numpy())


def test_engine_signatures():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.forecast_moments).parameters) == ["self", "params", "batch", "B", "is_post", "num_samples", "times_out", "mean", "sd",
                                                                          "x_mean", "x_sd", "states", "window"]
    assert list(inspect.signature(Engine.ode_solve).parameters) == ["self", "params", "z", "times"]
    assert list(inspect.signature(Engine.forecast_grid).parameters) == ["self", "times_out"]


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_forecast_steps_flag_of_the_training_entry_points(fam, monkeypatch, tmp_path):
    """--forecast-steps N reaches train() as forecast_steps=N from each entry point; without it train() gets what it gets today."""
    from structured_latent_odes_amd import training as TR
    tr = importlib.import_module("training_" + fam)
    seen = []
    monkeypatch.setattr(TR, "train", lambda config, family, a, b, n, **kw: seen.append((family, kw)))
    monkeypatch.chdir(tmp_path)
    assert TR.build_parser().parse_args([]).forecast_steps == 0
    for argv in (["--epochs", "1"], ["--epochs", "1", "--forecast-steps", "5"]):
        TR.main(tr.FAMILY, tr.load_config, tr.MechanisticModel, tr.MechanisticModelGauss, argv=argv)
    assert seen == [(fam, {"fused_stats": False}), (fam, {"fused_stats": False, "forecast_steps": 5})]
