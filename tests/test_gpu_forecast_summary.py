"""GPU tests of the forecast summaries (slode_forecast_summary; Engine.forecast_summary; MechanisticBase.forecast_summary /
save_forecast_summary; --forecast-summary).

What is exact and what has a bar (tests/summary_util.py, tests/forecast_summary_util.py).  The draw's curve is slode_forecast_moments' for the
same window, so at num_samples = 1 that call returns the kernel's own fp32 values: extremes, first indices and crossing are selections on
them and are held to numpy EXACTLY; the two sums are held to the numpy restatement of the kernel's order -- per-lane fma chain, four combine
steps, per-window merge -- BITWISE.  With one window, first_point = 0 and times_out = times the whole result is slode_curve_summary's bit for
bit.  Against the fp64 oracle on the output grid (FU.oracle_values sliced at first_point) the continuous slots have the bars of
recon_moments (SU.check_continuous) and the discontinuous ones the tolerant rules of SU.tolerant_violations, nothing excluded; no tolerance
of this file's own.  Outputs are pre-filled with a sentinel: every element must be written, by this call."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import forecast_summary_util as FSU
from tests import forecast_util as FU
from tests import recon_moments_util as RU
from tests import summary_util as SU
from tests.eval_gpu_util import DEV, _captured, _count_calls, _device_batch, _engine, _eps_dev, _forecast, _model, _padded, _refused, _summary
from tests.eval_gpu_util import _same as _same_arrays

pytestmark = pytest.mark.gpu
FILL = -12345.5            # the outputs are pre-filled with it (NaN is a value the call writes): every element must be written
_same = functools.partial(_same_arrays, equal_nan=True)


def _fs(eng, flat, c, is_post, thr, sense=1, i0=0, window=0, eps="case", ns=None, sd=True, obs_d=None, labels=None):
    """Engine.forecast_summary on the case's batch and output grid -> numpy (mean, sd), sd None where not asked."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q, Cn = (1 if c["ospec"].gauss else 3), c["obs"].shape[1]
    mean = torch.full((Q, c["B"], Cn, 8), FILL, device=DEV)
    sd_t = torch.full_like(mean, FILL) if sd else None
    got = eng.forecast_summary(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], is_post, ns, c["times_out"], first_point=i0,
                               thr=None if thr is None else [float(x) for x in thr], sense=sense, mean=mean, sd=sd_t, window=window)
    assert got[0] is mean and got[1] is sd_t
    out = tuple(None if t is None else t.cpu().numpy() for t in (mean, sd_t))
    assert all(t is None or not (t == FILL).any() for t in out), "an output element was not written"
    return out


def _against_the_oracle(eng, flat, c, tag, i0s, window=0, per_draw=True, senses=(1, -1)):
    """Continuous bars and the crossing rule on one call with the case's draws; with ``per_draw`` the tolerant rules at num_samples = 1.
    Returns {(is_post, i0, sense): (mean, sd)} and the oracle's sliced draws, for the caller to compare runs with."""
    t_all = c["times_out"].numpy()
    obs_d, labels = _device_batch(c)
    ns, runs, truth = c["ns"], {}, {}
    for is_post in (True, False):
        v_all = FU.oracle_values(c, is_post)[0]                                            # [Q, ns, B, C, T_out]
        for i0 in i0s:
            v, times = v_all[..., i0:], t_all[i0:]
            thr = SU.thresholds(v)
            vk = np.moveaxis(v, 1, 0)
            truth[(is_post, i0)] = (v, thr)
            for sense in senses:
                t = "%s %s i0 %d window %d sense %d" % (tag, "post" if is_post else "prior", i0, window, sense)
                mean, sd = _fs(eng, flat, c, is_post, thr, sense, i0, window, obs_d=obs_d, labels=labels)
                wm, ws = SU.oracle_moments(SU.functionals(vk, times, thr.astype(np.float64), sense))
                SU.check_continuous(mean.astype(np.float64), sd.astype(np.float64), wm, ws, np.abs(v).max(-1).max(1), float(times[-1] - times[0]), t)
                cross_o = SU.beyond(vk, thr.astype(np.float64), sense).any(-1).mean(0)
                assert np.all(np.abs(mean[..., 7] - cross_o) <= SU.near(vk, thr).any(-1).sum(0) / ns + 1e-6), t
                runs[(is_post, i0, sense)] = (mean, sd)
                if per_draw:
                    eps = c["eps"].to(DEV)
                    got = np.stack([_fs(eng, flat, c, is_post, thr, sense, i0, window, eps=eps[k].contiguous(), ns=1, sd=False, obs_d=obs_d, labels=labels)[0]
                                    for k in range(ns)])
                    bad = SU.tolerant_violations(got.astype(np.float64), vk, times, thr, sense)
                    print("%s: rows that break a tolerant rule %s" % (t, bad))
                    assert all(n == 0 for _, n in bad), (t, bad)
    return runs, truth


def _within_twice_the_bars(a, b, v, span, tag):
    """Two runs of the same case agree in the continuous slots within twice the bars (each sits within one bar of the oracle)."""
    vmax = np.maximum(1.0, np.abs(v).max(-1).max(1))
    for slot in (0, 2):
        scale = np.maximum(1.0, np.maximum(np.abs(a[0][..., slot]), np.abs(b[0][..., slot])).astype(np.float64))
        assert np.all(np.abs(a[0][..., slot].astype(np.float64) - b[0][..., slot]) <= 2 * RU.MEAN_BAR * scale), (tag, SU.NAMES[slot])
        assert np.all(np.abs(a[1][..., slot].astype(np.float64) - b[1][..., slot]) <= 2 * RU.SD_BAR * scale), (tag, SU.NAMES[slot], "sd")
    assert np.all(np.abs(a[0][..., 4].astype(np.float64) - b[0][..., 4]) <= 2 * span * RU.MEAN_BAR * vmax), (tag, "auc")


# ---- (1) oracle parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,T_out,solver", FU.PARITY, ids=["%s-%s" % (c, s) for c, _, s in FU.PARITY])
def test_parity_with_the_fp64_oracle(case, T_out, solver):
    """Six model classes x three fixed-grid solvers x {posterior, prior} x both senses on T_out = T + 9: the whole grid (since = None) and
    from the last training time on (first_point = T - 1: ten points), the default window."""
    c = FU.build(case, solver, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(float("nan"))
    i_last = FSU.first_point(c["times_out"].numpy(), float(c["times"][-1]))
    assert i_last == c["T"] - 1 and FSU.first_point(c["times_out"].numpy(), None) == 0
    _against_the_oracle(eng, flat, c, "%s/%s" % (case, solver), (0, i_last))


# ---- (2) the training grid: slode_curve_summary's bits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss", "challenge_gauss"])
def test_same_grid_one_window_is_curve_summary_bit_for_bit(case):
    """times_out = times, window = 0, first_point = 0: mean and sd equal slode_curve_summary's under torch.equal's rule (NaN where it has NaN),
    with explicit eps and with in-kernel noise from the same counter."""
    c = FU.build(case, "rk4", ns=7, T_out=EU.CASES[case][3])
    assert torch.equal(c["times_out"], c["times"].to(torch.float32))
    eng = _engine(c)
    flat = eng.pack(c["p"])
    assert eng.forecast_summary_plan(c["T"], 0)[0] == c["T"] - 1
    for is_post in (True, False):
        thr = SU.thresholds(SU.oracle_draws(c, is_post))
        for sense in (1, -1):
            want = _summary(eng, flat, c, is_post, thr, sense, p=False)
            got = _fs(eng, flat, c, is_post, thr, sense)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (case, is_post, sense)
        eng.rng_seed(41)
        eng.rng_set_counter(9)
        want = _summary(eng, flat, c, is_post, thr, 1, eps=None, p=False)
        eng.rng_set_counter(9)
        got = _fs(eng, flat, c, is_post, thr, 1, eps=None)
        assert eng.rng_state()[2] == 10 and _same(got[0], want[0]) and _same(got[1], want[1]), (case, is_post, "drawn")
        bare_w, bare_g = _summary(eng, flat, c, is_post, None, p=False), _fs(eng, flat, c, is_post, None)
        assert _same(bare_g[0], bare_w[0]) and _same(bare_g[1], bare_w[1]) and np.isnan(bare_g[0][..., 5:]).all()


# ---- (3) windows -------------------------------------------------------------------------------------------------------------------------------
def test_windows_on_a_grid_shorter_than_the_training_grid():
    """cvs_gauss (T = 86), T_out = 40: window 13 (three full windows), 19 (the last window is one step), 39 (one window, given), 0 (one
    window, chosen) and 1 (one-point rows) -- each against the oracle, from point 0 and from point 14 (the first slot of window 13's second
    window); 39 and 0 bitwise equal; the windowed runs against the single-window run within twice the bars.  T_out = 2: one step."""
    c = FU.build("cvs_gauss", "rk4", B=8, ns=7, T_out=40)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(float("nan"))
    assert eng.forecast_summary_plan(40, 0)[0] == 39 and eng.forecast_summary_plan(40, 13)[0] == 13
    runs = {}
    for W in (13, 19, 39, 0, 1):
        runs[W], truth = _against_the_oracle(eng, flat, c, "T_out 40", (0, 14), window=W, per_draw=W in (13, 1))
    t = c["times_out"].numpy()
    for key in runs[0]:
        assert _same(runs[39][key][0], runs[0][key][0]) and _same(runs[39][key][1], runs[0][key][1])          # the same window, given or chosen
        for W in (13, 19, 1):
            _within_twice_the_bars(runs[W][key], runs[0][key], truth[key[:2]][0], float(t[-1] - t[key[1]]), "window %d against one window %s" % (W, key))
    c2 = FU.build("cvs_gauss", "rk4", B=8, ns=7, T_out=2)
    _against_the_oracle(eng, flat, c2, "T_out 2", (0,))


def test_one_window_of_two_thread_rounds_and_a_window_of_70():
    """T_out = 300 in one window: two rounds of thread <-> step / point, the four-point trips of the row walk and then its remainder loop;
    window 70: five windows, the last of 19 steps.  From point 0 and from point 123 (inside the second window of 70)."""
    c = FU.build("cvs_gauss", "rk4", B=8, ns=7, T_out=300)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(float("nan"))
    assert eng.forecast_summary_plan(300, 0)[0] == 299
    one, truth = _against_the_oracle(eng, flat, c, "T_out 300", (0, 123), per_draw=False)
    win, _ = _against_the_oracle(eng, flat, c, "T_out 300", (0, 123), window=70, per_draw=False)
    t = c["times_out"].numpy()
    for key in one:
        _within_twice_the_bars(win[key], one[key], truth[key[:2]][0], float(t[-1] - t[key[1]]), "window 70 against one window %s" % (key,))


def test_beyond_the_largest_training_grid():
    """T_out = 1100 > 1024 (SLODE_MAX_T), B = 3, ns = 3: the default window (the whole grid fits this kernel's carve) and window = 256 (five
    windows, the last of 75 steps), from the last training time on."""
    c = FU.build("cvs_gauss", "rk4", B=3, ns=3, T_out=1100)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(float("nan"))
    i0 = FSU.first_point(c["times_out"].numpy(), float(c["times"][-1]))
    a, truth = _against_the_oracle(eng, flat, c, "T_out 1100, default window %d" % eng.forecast_summary_plan(1100, 0)[0], (i0,), per_draw=False)
    b, _ = _against_the_oracle(eng, flat, c, "T_out 1100", (i0,), window=256, per_draw=False)
    t = c["times_out"].numpy()
    for key in a:
        _within_twice_the_bars(b[key], a[key], truth[key[:2]][0], float(t[-1] - t[i0]), "window 256 against the default %s" % (key,))


def test_windows_on_the_proc_shape_at_run_time_s(monkeypatch):
    """proc_gauss (S = 8, C = 4), T_out = 600, window = 64 (ten windows, the last of 23 steps), B = 5: the run-time-S instantiation."""
    c = FU.build("proc_gauss", "midpoint", B=5, ns=7, T_out=600)
    eng = _engine(c, monkeypatch, {"SLODE_ODE_GENERIC": "1"})
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(float("nan"))
    _against_the_oracle(eng, flat, c, "proc_gauss T_out 600 generic", (0, 200), window=64, per_draw=False)


# ---- (4) the kernel's own curve, exactly -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,solver", [("cvs_ald", "midpoint"), ("cvs_gauss", "rk4")])
def test_per_draw_exactness_on_the_kernels_own_curve(case, solver):
    """ns = 1, windows 1, 7, 16 and the whole grid on T_out = 50, first_point 0, 17 and 49: slode_forecast_moments at ns = 1 with the same
    window returns the draw's curve in the kernel's bits; peak, trough, t_peak, t_trough, t_hit and crossed equal the numpy selection on it
    exactly, auc and time_beyond equal the numpy restatement of the kernel's order bitwise, sd is exactly 0."""
    c = FU.build(case, solver, B=8, ns=7, T_out=50)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    t = c["times_out"].numpy()
    for is_post in (True, False):
        row = c["eps"][3].to(DEV).contiguous()
        for W in (1, 7, 16, 0):
            curve = _forecast(eng, flat, c, is_post, window=W, eps=row, ns=1, states=False, sd=False, obs_d=obs_d, labels=labels)[0].cpu().numpy()
            assert curve.dtype == np.float32 and np.isfinite(curve).all()
            for i0 in (0, 17, 49):
                thr = RU._f32(np.median(curve[0][..., i0:], axis=(0, 2)))
                for sense in (1, -1):
                    mean, sd = _fs(eng, flat, c, is_post, thr, sense, i0, W, eps=row, ns=1, obs_d=obs_d, labels=labels)
                    want = SU.functionals(curve[..., i0:], t[i0:], thr, sense)
                    for slot in (0, 1, 2, 3, 6, 7):
                        assert np.array_equal(mean[..., slot].astype(np.float64), want[..., slot], equal_nan=True), (case, is_post, W, i0, sense, SU.NAMES[slot])
                    rest = FSU.restatement(curve, t, i0, W, thr, sense)
                    assert _same(mean[..., 4], rest[..., 4]) and _same(mean[..., 5], rest[..., 5]), (case, is_post, W, i0, sense)
                    assert _same(mean, rest)
                    assert np.array_equal(np.isnan(sd), np.isnan(mean)) and np.all(sd[~np.isnan(sd)] == 0.0)


# ---- (5) ties and boundaries ----------------------------------------------------------------------------------------------------------------------
def test_ties_and_window_boundaries_on_a_curve_of_zeros():
    """Head weights zeroed: every value is 0 and every point ties.  Windows 1, 7, 16 and whole on T_out = 50; first_point = the first slot of a
    window, the last slot of a window, 0 and T_out - 1.  t_peak = t_trough = t[i0] exactly; auc = 0; thr = -1, above: crossed = 1, t_hit =
    t[i0], time_beyond = the restated sum of w bitwise; thr = +1: crossed = 0, t_hit NaN, time_beyond = 0; at T_out - 1 peak == trough."""
    c = FU.build("cvs_ald", "rk4", B=4, ns=3, T_out=50)
    c["p"] = dict(c["p"])
    for k in FU.head_keys(c["ospec"]):
        c["p"][k] = torch.zeros_like(c["p"][k])
    eng = _engine(c)
    flat = eng.pack(c["p"])
    t = c["times_out"].numpy()
    Cn = c["obs"].shape[1]
    zeros = np.zeros((3, c["B"], Cn, 50), np.float32)
    for W in (1, 7, 16, 0):
        first, last = (W + 1, 2 * W) if W else (0, 49)
        for i0 in sorted({first, last, 0, 49}):
            for is_post in (True, False):
                mean, sd = _fs(eng, flat, c, is_post, [-1.0] * Cn, 1, i0, W)
                tag = (W, i0, is_post)
                assert np.all(mean[..., 0] == 0.0) and np.all(mean[..., 2] == 0.0) and np.all(mean[..., 1] == t[i0]) and np.all(mean[..., 3] == t[i0]), tag
                assert np.all(mean[..., 4] == 0.0) and np.all(mean[..., 7] == 1.0) and np.all(mean[..., 6] == t[i0]) and np.all(sd == 0.0), tag
                assert _same(mean[..., 5], FSU.restatement(zeros, t, i0, W, [-1.0] * Cn, 1)[..., 5]), tag
                assert np.all(mean[..., 5] == 0.0) if i0 == 49 else np.all(mean[..., 5] > 0.0), tag
                mean, sd = _fs(eng, flat, c, is_post, [1.0] * Cn, 1, i0, W)
                assert np.all(mean[..., 7] == 0.0) and np.isnan(mean[..., 6]).all() and np.isnan(sd[..., 6]).all() and np.all(mean[..., 5] == 0.0), tag
                assert np.all(mean[..., 1] == t[i0]) and np.all(mean[..., 3] == t[i0]) and np.array_equal(mean[..., 0], mean[..., 2]), tag
    # first_point = 0 is the default (since = None): bitwise
    obs_d, labels = _device_batch(c)
    bt = eng.make_batch(obs_d, labels, _eps_dev(c["eps"]), particles=3)
    a = eng.forecast_summary(flat, bt, c["B"], True, 3, c["times_out"], thr=[-1.0] * Cn, sd=True, window=7)
    b = eng.forecast_summary(flat, bt, c["B"], True, 3, c["times_out"], first_point=0, thr=[-1.0] * Cn, sd=True, window=7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- (6) reproducibility -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "cvs_gauss"])
def test_bitwise_reproducible_and_independent_of_the_grid(case, monkeypatch):
    """window = 16, T_out = 50 (four windows, the last of one step), first_point 20.  Two calls: bitwise equal.  One workgroup per trajectory
    against a 3-workgroup loop: bitwise equal.  In-kernel noise against the same rows passed explicitly: bitwise equal; the counter is left
    at n + 1."""
    c = FU.build(case, {"cvs_ald": "midpoint", "cvs_gauss": "rk4"}[case], ns=7, T_out=50)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        thr = SU.thresholds(FU.oracle_values(c, is_post)[0][..., 20:])
        a = _fs(eng, flat, c, is_post, thr, 1, 20, 16)
        for other in (_fs(eng, flat, c, is_post, thr, 1, 20, 16), _fs(loop, flat, c, is_post, thr, 1, 20, 16)):
            assert all(_same(x, y) for x, y in zip(a, other))
        assert np.isfinite(a[0][..., :6]).all()
        for e in (eng, loop):
            e.rng_seed(77, first_trajectory=1000)
            e.rng_set_counter(5)
        drawn = _fs(eng, flat, c, is_post, thr, 1, 20, 16, eps=None)
        assert eng.rng_state() == (77, 1000, 6)
        rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
        given = _fs(eng, flat, c, is_post, thr, 1, 20, 16, eps=rows)
        assert eng.rng_state() == (77, 1000, 6)                                          # explicit noise draws nothing
        drawn_loop = _fs(loop, flat, c, is_post, thr, 1, 20, 16, eps=None)
        assert all(_same(x, y) and _same(x, z) for x, y, z in zip(drawn, given, drawn_loop))


# ---- (7) outputs, launches, capture, refusals ----------------------------------------------------------------------------------------------------
def test_sd_is_optional_launch_names_and_graph_capture():
    """sd = None leaves the mean bitwise unchanged.  Posterior: "weff", "enc_fwd2", "forecast_summary" on one stream; prior:
    "forecast_summary" alone.  One capture and one replay of a posterior call equal the stream-launched call bitwise (the threshold travels
    by value: nothing is read from the host at replay)."""
    c = FU.build("cvs_ald", "midpoint", ns=7, T_out=50)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    thr = [float(x) for x in SU.thresholds(FU.oracle_values(c, True)[0][..., 20:])]
    full = _fs(eng, flat, c, True, thr, 1, 20, 16)
    lean = _fs(eng, flat, c, True, thr, 1, 20, 16, sd=False)
    assert lean[1] is None and _same(lean[0], full[0])
    eng.profile_enable(True)
    _fs(eng, flat, c, True, thr, 1, 20, 16)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "forecast_summary"]
    _fs(eng, flat, c, False, thr, 1, 20, 16)
    assert [n for n, _ in eng.profile_read()] == ["forecast_summary"]
    eng.profile_enable(False)
    outs = [torch.zeros(3, c["B"], 3, 8, device=DEV), torch.zeros(3, c["B"], 3, 8, device=DEV)]
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    eng.forecast_grid(c["times_out"])                                                   # (built before the capture: the call itself only enqueues)
    want = _captured(lambda: eng.forecast_summary(flat, bt, c["B"], True, 7, c["times_out"], 20, thr, 1, outs[0], outs[1], 16), outs)
    assert all(_same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(outs, want)) and float(outs[0].nan_to_num().abs().max()) > 0.0
    assert _same(outs[0].cpu().numpy(), full[0]) and _same(outs[1].cpu().numpy(), full[1])


def test_refusals_write_nothing_and_draw_nothing(monkeypatch):
    c = FU.build("cvs_ald", "rk4", B=5, ns=2, T_out=50)
    obs_d, labels = _device_batch(c)

    def refused(eng, match, times_out=None, obs=obs_d, **kw):
        flat = eng.pack(c["p"])
        t_out = c["times_out"] if times_out is None else times_out
        outs = [torch.full((3, 5, 3, 8), FILL, device=DEV), torch.full((3, 5, 3, 8), FILL, device=DEV)]
        args = dict(dict(first_point=0, thr=(0.1, 0.2, 0.3), sense=1, window=0), **kw)
        err = _refused(eng, lambda: eng.forecast_summary(flat, eng.make_batch(obs, labels, None), 5, True, 2, t_out, mean=outs[0], sd=outs[1], **args), match)
        assert err.status == -1 and "slode_forecast_summary" in str(err)
        torch.cuda.synchronize(DEV)
        assert all(bool((t == FILL).all()) for t in outs)

    refused(_engine(c, monkeypatch, solver="dopri5"), "adaptive solver dopri5 .*reduce forecast_samples instead")
    eng = _engine(c, monkeypatch)
    refused(eng, "first_point = 50 out of range \\[0, T_out - 1 = 49\\]", first_point=50)
    refused(eng, "first_point = -1 out of range", first_point=-1)
    refused(eng, "sense = 0", sense=0)
    refused(eng, "thr\\[1\\] = nan is not finite", thr=(0.1, float("nan"), 0.3))
    refused(eng, "window = -2 < 0", window=-2)
    refused(eng, "window = 19999 does not fit", times_out=FU.grid(c["times"], 20000), window=19999)
    refused(eng, "observation strides", obs=_padded(obs_d))
    refused(_engine(c, monkeypatch, {"SLODE_ODE_ALG": "1"}), "measured arms")
    with pytest.raises(ValueError, match="one per channel"):
        eng.forecast_summary(eng.pack(c["p"]), eng.make_batch(obs_d, labels, None), 5, True, 2, c["times_out"], thr=(0.1, 0.2))


# ---- (8) the model layer -----------------------------------------------------------------------------------------------------------------------
def _curves(m, batch, is_post, eps, t_out):
    """[Q, ns, B, C, T_out] fp64: the materialising route's curves of the same draws (forecast_samples)."""
    res = m.forecast_samples(is_post=is_post, num_samples=eps.shape[0], times_out=t_out, eps=eps, **batch)
    return np.stack([res[n].double().permute(3, 0, 1, 2).cpu().numpy() for n in m.MOMENT_HEADS[bool(m.GAUSS)]])


def _check_model(res, m, v, t_out, i0, thr, sense, tag):
    """The dict against the curves v [Q, ns, B, C, T_out] of the same draws, sliced at i0: the continuous slots by the bars, P(cross) by
    the near rule (two fp32 evaluations, each within the bar of the truth; the rule is applied with the bar itself, the stricter reading)."""
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    times = t_out.float().cpu().numpy()[i0:]
    vs = v[..., i0:]
    vk = np.moveaxis(vs, 1, 0)
    wm, ws = SU.oracle_moments(SU.functionals(vk, times, np.asarray(thr, np.float64), sense))
    mean = np.stack([np.stack([res[n][k][0].double().cpu().numpy() for k in SU.NAMES], -1) for n in names])
    sd = np.stack([np.stack([res[n][k][1].double().cpu().numpy() for k in SU.NAMES], -1) for n in names])
    SU.check_continuous(mean, sd, wm, ws, np.abs(vs).max(-1).max(1), float(times[-1] - times[0]), tag)
    cross_o = SU.beyond(vk, np.asarray(thr, np.float64), sense).any(-1).mean(0)
    assert np.all(np.abs(mean[..., 7] - cross_o) <= SU.near(vk, thr).any(-1).sum(0) / vs.shape[1] + 1e-6), tag
    assert all(res[n]["first_point"] == i0 for n in names)


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_fused_and_composed_routes_agree(fam):
    """horizon_times(9), since = the last training time: the fused call (launch names; the counter at n + 1) and the composed route (a
    padded observation tensor, which the engine refuses) on the same noise, each against the materialised curves of those draws."""
    m, batch = _model(fam)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    t_out, since, ns = m.horizon_times(9), float(torch.as_tensor(m.times).reshape(-1)[-1]), 6
    for is_post in (True, False):
        eng.rng_seed(21)
        eng.rng_set_counter(3)
        eps = eng.rng_normal(3, ns * B).view(ns, B, -1)
        v = _curves(m, batch, is_post, eps, t_out)
        thr = SU.thresholds(v[..., T - 1:])
        eng.profile_enable(True)
        res = m.forecast_summary(is_post=is_post, num_samples=ns, times_out=t_out, since=since, thresholds=torch.tensor(thr), sense="above", **batch)
        assert [k for k, _ in eng.profile_read()] == (["weff", "enc_fwd2", "forecast_summary"] if is_post else ["forecast_summary"])
        eng.profile_enable(False)
        assert eng.rng_state() == (21, 0, 4) and set(res) == set(names)
        for n in names:
            assert set(res[n]) == set(SU.NAMES) | {"first_point"} and all(tuple(t.shape) == (B, Cn) for k in SU.NAMES for t in res[n][k])
        _check_model(res, m, v, t_out, T - 1, thr, 1, "%s %s fused" % (fam, "post" if is_post else "prior"))
        if is_post:
            composed = m.forecast_summary(is_post=True, num_samples=ns, times_out=t_out, since=since, thresholds=thr, sense="above", eps=eps,
                                          **dict(batch, observations=_padded(batch["observations"])))
            _check_model(composed, m, v, t_out, T - 1, thr, 1, "%s composed" % fam)
        whole = m.forecast_summary(is_post=is_post, num_samples=ns, times_out=t_out, eps=eps, **batch)
        assert whole[names[0]]["first_point"] == 0 and all(torch.isnan(whole[n][k][0]).all() for n in names for k in SU.NAMES[5:])


@pytest.mark.parametrize("why", ["dopri5", "strided"])
def test_model_level_call_is_total_over_what_the_engine_refuses(why, monkeypatch):
    """An adaptive-solver model and a padded observation tensor: the engine refuses once, forecast_summary composes the dict from
    forecast_samples -- one drawing call, the counter at n + 1 -- and agrees with those curves reduced here; strided: chunked composed runs
    equal the unchunked one bitwise."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch)
    eng = m._bind().engine
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    B, T = batch["observations"].shape[0], batch["observations"].shape[2]
    names, ns, t_out = m.MOMENT_HEADS[bool(m.GAUSS)], 6, m.horizon_times(9)
    since = float(torch.as_tensor(m.times).reshape(-1)[-3])
    calls = _count_calls(monkeypatch, eng, "forecast_summary")
    eng.rng_seed(11)
    eng.rng_set_counter(2)
    eps = eng.rng_normal(2, ns * B).view(ns, B, -1)
    v = _curves(m, batch, True, eps, t_out)
    thr = SU.thresholds(v[..., T - 3:])
    drawn = m.forecast_summary(is_post=True, num_samples=ns, times_out=t_out, since=since, thresholds=thr, sense="below", **batch)
    assert eng.rng_state() == (11, 0, 3) and len(calls) == 1                        # refused once, then composed
    given = m.forecast_summary(is_post=True, num_samples=ns, times_out=t_out, since=since, thresholds=thr, sense="below", eps=eps, **batch)
    if why == "strided":                                                               # (dopri5's step sizes depend on the launch's batch: not bitwise)
        assert all(torch.equal(given[n][k][0].nan_to_num(), drawn[n][k][0].nan_to_num()) for n in names for k in SU.NAMES)
        monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 5 * ns)                       # four chunks of 5 rows: ONE drawing call, the same rows
        chunked = m.forecast_summary(is_post=True, num_samples=ns, times_out=t_out, since=since, thresholds=thr, sense="below", eps=eps, **batch)
        assert all(torch.equal(chunked[n][k][j].nan_to_num(), given[n][k][j].nan_to_num()) for n in names for k in SU.NAMES for j in (0, 1))
    _check_model(given, m, v, t_out, T - 3, thr, -1, "%s composed" % why)


def test_output_files(tmp_path):
    """save_forecast_summary over two batches: summary_<curve>_post_forecast_{mean,sd}.npy [n, C, 8] and forecast_times.npy, equal to
    forecast_summary from the same generator state, the trajectories in loader order."""
    m, batch = _model("challenge")
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    halves = [{k: v[:9] for k, v in batch.items()}, {k: v[9:] for k, v in batch.items()}]
    halves = [dict(h, observations=h["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)) for h in halves]
    thr, t_out = [0.3] * Cn, m.horizon_times(5)
    since = float(torch.as_tensor(m.times).reshape(-1)[-1])
    eng.rng_seed(8)
    files = m.save_forecast_summary(str(tmp_path / "fs"), halves, True, 5, t_out, since=since, thresholds=thr, sense="above")
    assert eng.rng_state()[2] == 2
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    want = ["summary_%s_post_forecast_%s.npy" % (n, k) for n in names for k in ("mean", "sd")] + ["forecast_times.npy"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "fs"))) == sorted(want)
    assert np.array_equal(np.load(files[-1]), t_out.cpu().numpy())
    mean, sd = np.load(files[0]), np.load(files[1])
    assert mean.shape == sd.shape == (B, Cn, 8) and mean.dtype == np.float32 and np.isfinite(mean[..., :6]).all()
    eng.rng_set_counter(1)
    res = m.forecast_summary(is_post=True, num_samples=5, times_out=t_out, since=since, thresholds=thr, **halves[1])
    assert np.array_equal(mean[9:, :, 0], res[names[0]]["peak"][0].cpu().numpy()) and np.array_equal(sd[9:, :, 4], res[names[0]]["auc"][1].cpu().numpy())
    assert np.all(mean[:, :, 1] >= since) and res[names[0]]["first_point"] == T - 1
    print(m.summary_line(mean, names[0], True, name="forecast_summary"))


def test_training_entry_point_with_forecast_summary(tmp_path, capsys):
    tr = importlib.import_module("training_cvs")
    cfg = EU.model_config("cvs")
    cfg.update(num_epochs=0, mini_batch_size=16, seq_len=86, num_samples=5)
    tr.train(cfg, batches_per_epoch=1, forecast_steps=5, forecast_summary=3, summary_thresholds=[0.5, 0.5, 0.5], results_dir=str(tmp_path / "res"))
    out = capsys.readouterr().out
    assert "FINAL TEST:" in out and all(("forecast_summary_%s: n=16  c0 peak=" % n) in out for n in ("mu_50", "mu_75", "mu_25")) and "p_cross=" in out
    got = sorted(os.listdir(str(tmp_path / "res")))
    assert got == sorted(["%s_post_forecast_%s.npy" % (cv, k) for cv in ("mu_50", "mu_75", "mu_25") for k in ("mean", "sd")] + ["forecast_times.npy"]
                         + ["summary_%s_post_forecast_%s.npy" % (cv, k) for cv in ("mu_50", "mu_75", "mu_25") for k in ("mean", "sd")])
    assert np.load(str(tmp_path / "res" / "summary_mu_50_post_forecast_mean.npy")).shape == (16, 3, 8)
    assert np.load(str(tmp_path / "res" / "forecast_times.npy")).shape == (91,)
