"""GPU tests of the forecast moments (slode_forecast_moments / Engine.forecast_moments / MechanisticBase.forecast_moments /
save_forecast_moments / --forecast-steps) against the fp64 oracle on the output grid (tests/forecast_util.py: O.solve_ode on times_out and
the heads as F.linear), against slode_recon_moments on the training grid, and against the materialising path.
Bars: those of tests/recon_moments_util.py -- 1e-4 max(1, |mu|) for a mean, 2e-4 max(1, |mu|) for an sd -- for the head curves and,
with |x| in place of |mu|, for the states.  tests/test_forecast_cpu.py holds the fp32 oracle of every (case, T_out, solver) used here to a
quarter of them.  Workspaces are NaN-poisoned and outputs NaN-prefilled: every element must be written, by this call."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import forecast_util as FU
from tests import recon_moments_util as RU
from tests.eval_gpu_util import DEV, _captured, _device_batch, _engine, _eps_dev, _model, _padded, _refused
from tests.eval_gpu_util import _forecast

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _check_oracle(got, c, is_post, tag, eps=None):
    want = FU.oracle_moments(c, is_post, eps)
    RU.check(got[0], got[1], want[0], want[1], tag + " heads")
    if got[2] is not None:
        RU.check(got[2], got[3], want[2], want[3], tag + " states")
    return want


def _within(a, b, want, factor, tag):
    """Two runs of the same case agree within ``factor`` x the bars (each sits within one bar of the oracle)."""
    for i, (x, y) in enumerate(zip(a, b)):
        scale = np.maximum(1.0, np.abs(want[i - i % 2]))
        bar = (RU.MEAN_BAR, RU.SD_BAR)[i % 2] * scale * factor
        d = np.abs(x.double().cpu().numpy() - y.double().cpu().numpy())
        assert np.isfinite(d).all() and float((d / bar).max()) <= 1.0, (tag, i, float((d / bar).max()))


# ---- oracle parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_forecast_matches_the_fp64_oracle(case, solver):
    """Six model classes x three fixed-grid solvers x {posterior, prior}: T_out = T + 9, the grid extended at its last spacing, the default
    window, heads and states."""
    c = FU.build(case, solver, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(NAN)
    for is_post in (True, False):
        _check_oracle(_forecast(eng, flat, c, is_post), c, is_post, "%s/%s/%s" % (case, solver, "post" if is_post else "prior"))


# ---- windows -----------------------------------------------------------------------------------------------------------------------------
def test_windows_on_a_grid_shorter_than_the_training_grid():
    """cvs_gauss (T = 86), T_out = 40: window 13 (three full windows), 19 (the last window is one step), 39 (one window, given), 0 (one
    window, chosen) -- each against the oracle, and the windowed runs against the unwindowed one within twice the bars.  T_out = 2: one step."""
    c = FU.build("cvs_gauss", "rk4", B=9, ns=7, T_out=40)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(NAN)
    assert eng.forecast_plan(c["B"], 40, 7, True, 0)[0] == 39 and eng.forecast_plan(c["B"], 40, 7, True, 13)[0] == 13
    for is_post in (True, False):
        runs = {}
        for W in (13, 19, 39, 0):
            runs[W] = _forecast(eng, flat, c, is_post, window=W)
            want = _check_oracle(runs[W], c, is_post, "T_out 40, window %d, %s" % (W, "post" if is_post else "prior"))
        assert all(torch.equal(a, b) for a, b in zip(runs[39], runs[0]))               # the same window, given or chosen
        for W in (13, 19):
            _within(runs[W], runs[0], want, 2.0, "window %d against one window" % W)
    c2 = FU.build("cvs_gauss", "rk4", B=9, ns=7, T_out=2)
    for is_post in (True, False):
        _check_oracle(_forecast(eng, flat, c2, is_post), c2, is_post, "T_out 2")


def test_single_window_of_two_thread_rounds():
    """T_out = 300 in one window: the 256 threads take two rounds of steps (M4) and of time points (M6 / M7)."""
    c = FU.build("cvs_gauss", "rk4", B=9, ns=7, T_out=300)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(NAN)
    assert eng.forecast_plan(c["B"], 300, 7, True, 0)[0] == 299
    for is_post in (True, False):
        _check_oracle(_forecast(eng, flat, c, is_post), c, is_post, "T_out 300")


def test_beyond_the_largest_training_grid():
    """T_out = 1100 > 1024 (SLODE_MAX_T), B = 3, ns = 3: the default window and window = 256 (five windows, the last of 75 steps)."""
    c = FU.build("cvs_gauss", "rk4", B=3, ns=3, T_out=1100)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(NAN)
    for is_post in (True, False):
        a = _forecast(eng, flat, c, is_post)
        want = _check_oracle(a, c, is_post, "T_out 1100, default window %d" % eng.forecast_plan(3, 1100, 3, True, 0)[0])
        b = _forecast(eng, flat, c, is_post, window=256)
        _check_oracle(b, c, is_post, "T_out 1100, window 256")
        _within(a, b, want, 2.0, "T_out 1100: window 256 against the default")


@pytest.mark.parametrize("env", [{"SLODE_ODE_GENERIC": "1"}, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}], ids=["generic", "loop-grid2"])
def test_windows_on_the_proc_shape(env, monkeypatch):
    """proc_gauss (S = 8, C = 4), T_out = 600, window = 64 (ten windows, the last of 23 steps), B = 5: the run-time-S instantiation, and
    the persistent loop (5 trajectories on 2 workgroups)."""
    c = FU.build("proc_gauss", "midpoint", B=5, ns=7, T_out=600)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(c["B"]).fill_(NAN)
    for is_post in (True, False):
        _check_oracle(_forecast(eng, flat, c, is_post, window=64), c, is_post, "proc_gauss T_out 600 window 64 %s" % env)


# ---- the training grid: the parent's call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_same_grid_as_recon_moments(case):
    """times_out = times, window = 0: the operations are those of slode_recon_moments on the same noise -- mean bitwise equal; sd equal
    too, or within the sd bar of RU.accumulation_bars should the compiler contract M7's s2 - s1 * s1 * inv differently in the two units."""
    c = FU.build(case, "rk4", ns=7, T_out=EU.CASES[case][3])
    assert torch.equal(c["times_out"], c["times"].to(torch.float32))
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    for is_post in (True, False):
        Q = 1 if c["ospec"].gauss else 3
        mean = torch.full((Q, c["B"], c["obs"].shape[1], c["T"]), NAN, device=DEV)
        sd = torch.full_like(mean, NAN)
        eng.recon_moments(flat, eng.make_batch(obs_d, labels, _eps_dev(c["eps"]), particles=7), c["B"], is_post, 7, mean, sd)
        got = _forecast(eng, flat, c, is_post, obs_d=obs_d, labels=labels)
        assert torch.equal(got[0], mean)
        same = torch.equal(got[1], sd)
        print("%s %s: sd bitwise equal to recon_moments: %s" % (case, "post" if is_post else "prior", same))
        if not same:
            bar = RU.accumulation_bars(mean.double().cpu().numpy(), sd.double().cpu().numpy(), 7)[1]
            assert np.all(np.abs(got[1].double().cpu().numpy() - sd.double().cpu().numpy()) <= bar)


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "cvs_gauss"])
def test_bitwise_reproducible_and_independent_of_the_grid(case, monkeypatch):
    """window = 16, T_out = 50 (four windows, the last of one step).  Two calls: bitwise equal.  One workgroup per trajectory against a
    3-workgroup loop: bitwise equal.  In-kernel noise against the same rows passed explicitly: bitwise equal; the counter moves by exactly
    one.  ns = 1: sd exactly 0 and the mean is the draw (the ns = 1 call on that row alone)."""
    c = FU.build(case, {"cvs_ald": "midpoint", "cvs_gauss": "rk4"}[case], ns=7, T_out=50)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        a = _forecast(eng, flat, c, is_post, window=16)
        b = _forecast(eng, flat, c, is_post, window=16)
        l = _forecast(loop, flat, c, is_post, window=16)
        assert all(torch.equal(x, y) and torch.equal(x, z) and bool(torch.isfinite(x).all()) for x, y, z in zip(a, b, l))
        for e in (eng, loop):
            e.rng_seed(77, first_trajectory=1000)
            e.rng_set_counter(5)
        drawn = _forecast(eng, flat, c, is_post, window=16, eps=None)
        assert eng.rng_state() == (77, 1000, 6)
        rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
        given = _forecast(eng, flat, c, is_post, window=16, eps=rows)
        assert eng.rng_state() == (77, 1000, 6)                                          # explicit noise draws nothing
        drawn_loop = _forecast(loop, flat, c, is_post, window=16, eps=None)
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(drawn, given, drawn_loop))
        one = _forecast(eng, flat, c, is_post, window=16, eps=rows[0].contiguous(), ns=1)
        assert float(one[1].abs().max()) == 0.0 and float(one[3].abs().max()) == 0.0
        _check_oracle(one, c, is_post, "ns = 1", eps=rows[:1].cpu())


# ---- outputs -----------------------------------------------------------------------------------------------------------------------------
def test_optional_outputs_in_every_combination():
    """sd, x_mean, x_sd NULL in every combination: what is given equals the all-outputs call bitwise; two sentinel tensors beside the
    outputs stay NaN.  (x_mean and x_sd both NULL: the kernel keeps no state tables.)"""
    c = FU.build("cvs_ald", "midpoint", B=5, ns=3, T_out=50)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    full = _forecast(eng, flat, c, True, window=16)
    for sd in (True, False):
        for xm in (True, False):
            for xs in (True, False):
                got = _forecast(eng, flat, c, True, window=16, sd=sd, x_mean=xm, x_sd=xs)
                assert [t is not None for t in got] == [True, sd, xm, xs]
                assert all(t is None or torch.equal(t, f) for t, f in zip(got, full)), (sd, xm, xs)
    # the wrapper: no states unless asked
    obs_d, labels = _device_batch(c)
    bt = eng.make_batch(obs_d, labels, _eps_dev(c["eps"]), particles=3)
    mean, sd, xm, xs = eng.forecast_moments(flat, bt, c["B"], True, 3, c["times_out"], window=16)
    assert xm is None and xs is None and torch.equal(mean, full[0]) and torch.equal(sd, full[1])
    mean, sd, xm, xs = eng.forecast_moments(flat, bt, c["B"], True, 3, c["times_out"], states=True, window=16)
    assert torch.equal(xm, full[2]) and torch.equal(xs, full[3])


# ---- launches and capture ----------------------------------------------------------------------------------------------------------------
def test_launches_and_graph_capture():
    """Posterior: "weff", "enc_fwd2", "forecast_moments" on one stream; prior: "forecast_moments" alone.  One capture and one replay of a
    posterior call equal the stream-launched call bitwise."""
    c = FU.build("cvs_ald", "midpoint", ns=7, T_out=50)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eng.profile_enable(True)
    _forecast(eng, flat, c, True, window=16)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "forecast_moments"]
    _forecast(eng, flat, c, False, window=16)
    assert [n for n, _ in eng.profile_read()] == ["forecast_moments"]
    eng.profile_enable(False)
    B, S = c["B"], c["S"]
    outs = [torch.zeros(3, B, 3, 50, device=DEV), torch.zeros(3, B, 3, 50, device=DEV), torch.zeros(B, S, 50, device=DEV), torch.zeros(B, S, 50, device=DEV)]
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    eng.forecast_grid(c["times_out"])                                                   # (built before the capture: the call itself only enqueues)
    want = _captured(lambda: eng.forecast_moments(flat, bt, B, True, 7, c["times_out"], *outs, window=16), outs)
    assert all(torch.equal(t, w) and float(w.abs().sum()) > 0 for t, w in zip(outs, want))


# ---- refusals on a real handle -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_draw_nothing(monkeypatch):
    c = FU.build("cvs_ald", "rk4", B=5, ns=2, T_out=50)
    obs_d, labels = _device_batch(c)

    def refused(eng, match, times_out=None, window=0):
        flat = eng.pack(c["p"])
        t_out = c["times_out"] if times_out is None else times_out
        outs = [torch.full((3, 5, 3, t_out.numel()), NAN, device=DEV), torch.full((3, 5, 3, t_out.numel()), NAN, device=DEV),
                torch.full((5, 5, t_out.numel()), NAN, device=DEV), torch.full((5, 5, t_out.numel()), NAN, device=DEV)]
        err = _refused(eng, lambda: eng.forecast_moments(flat, eng.make_batch(obs_d, labels, None), 5, True, 2, t_out, *outs, window=window), match)
        assert err.status == -1
        torch.cuda.synchronize(DEV)
        assert all(bool(torch.isnan(t).all()) for t in outs)

    refused(_engine(c, monkeypatch, solver="dopri5"), "adaptive solver dopri5")
    eng = _engine(c, monkeypatch)
    refused(eng, "window = 19999 does not fit", times_out=FU.grid(c["times"], 20000), window=19999)
    refused(eng, "window = -2", window=-2)
    with pytest.raises(ValueError, match="outside"):                                   # the wrapper's own check of the grid's length ...
        eng.forecast_grid(c["times_out"][:1])
    tt, st = eng.forecast_grid(c["times_out"])                                          # ... and the library's, on the raw call
    flat, ws, mean = eng.pack(c["p"]), eng.workspace(5), torch.full((3, 5, 3, 50), NAN, device=DEV)
    for bad in (1, (1 << 20) + 1):
        bt = eng.make_batch(obs_d, labels, None)
        rc = eng.lib.slode_forecast_moments(eng.handle, C.byref(eng.shape(5)), C.byref(eng.layout), eng._p(flat), eng._p(eng._times), eng._p(eng._stage_t),
                                            C.byref(bt), 1, 2, eng._p(tt), eng._p(st), bad, 0, eng._p(mean), None, None, None,
                                            eng._p(ws), ws.numel() * 4, eng._stream())
        assert rc == -1 and ("T_out = %d out of range" % bad) in eng.lib.slode_last_error(eng.handle).decode()
    torch.cuda.synchronize(DEV)
    assert bool(torch.isnan(mean).all()) and eng.rng_state()[2] == 4


# ---- model level -------------------------------------------------------------------------------------------------------------------------
def _agree(got, want64, tag):
    for n in want64:
        RU.check(got[n][0], got[n][1], want64[n][0].cpu().numpy(), want64[n][1].cpu().numpy(), "%s %s" % (tag, n))


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_fused_route_agrees_with_the_materialising_one(fam):
    """From the same generator state: forecast_moments (one engine call) against forecast_samples reduced in fp64, heads and states, on
    horizon_times(9); both leave the counter at n + 1; shapes [B, C, T_out] and [B, T_out, S]."""
    m, batch = _model(fam)
    eng = m._bind().engine
    t_out = m.horizon_times(9)
    B, T_out = batch["observations"].shape[0], 86 + 9
    for is_post in (True, False):
        eng.rng_seed(5)
        got = m.forecast_moments(is_post=is_post, num_samples=6, times_out=t_out, states=True, **batch)
        assert eng.rng_state()[2] == 1
        eng.rng_set_counter(0)
        res = m.forecast_samples(is_post=is_post, num_samples=6, times_out=t_out, states=True, **batch)
        assert eng.rng_state()[2] == 1
        names = [n for n in res if n != "z"]
        assert set(names) == set(got) and tuple(got["mu_50"][0].shape) == (B, batch["observations"].shape[1], T_out)
        assert tuple(got["solution_xt"][0].shape) == tuple(got["solution_xt"][1].shape) == (B, T_out, m._bind().engine.spec.ode_state_dim)
        _agree(got, {n: (res[n].double().mean(-1), res[n].double().std(-1, unbiased=False)) for n in names}, "%s %s" % (fam, is_post))


@pytest.mark.parametrize("why", ["dopri5", "strided"])
def test_model_level_call_is_total_over_what_the_engine_refuses(why, monkeypatch):
    """An adaptive-solver model and a padded observation tensor: the engine refuses, forecast_moments composes the dict from
    forecast_samples -- bitwise that reduction made by hand from the same generator state, whatever the chunking.  strided: the composed
    result agrees within the bars with the fused call on the same observations made dense, on the same explicit noise."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch)
    eng = m._bind().engine
    dense = dict(batch)
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    names, ns, t_out = ("mu_50", "mu_75", "mu_25", "solution_xt"), 6, m.horizon_times(9)
    B, L = batch["observations"].shape[0], m.latent_dim
    eng.rng_seed(11)
    got = m.forecast_moments(is_post=True, num_samples=ns, times_out=t_out, states=True, **batch)
    assert eng.rng_state()[2] == 1
    eng.rng_set_counter(0)
    res = m.forecast_samples(is_post=True, num_samples=ns, times_out=t_out, states=True, **batch)
    for n in names:
        assert torch.equal(got[n][0], res[n].mean(-1)) and torch.equal(got[n][1], res[n].std(-1, unbiased=False)) and bool(torch.isfinite(got[n][0]).all())
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 5 * ns)                           # four chunks of 5 rows: ONE drawing call, the same rows
    eng.rng_set_counter(0)
    chunked = m.forecast_moments(is_post=True, num_samples=ns, times_out=t_out, states=True, **batch)
    assert eng.rng_state()[2] == 1
    if why == "strided":                                                               # (dopri5's step sizes depend on the launch's batch: not bitwise)
        assert all(torch.equal(chunked[n][0], got[n][0]) and torch.equal(chunked[n][1], got[n][1]) for n in names)
        eps = torch.randn(ns, B, L, generator=torch.Generator().manual_seed(2)).to(DEV)
        composed = m.forecast_moments(is_post=True, num_samples=ns, times_out=t_out, eps=eps, states=True, **batch)
        eng.profile_enable(True)
        fused = m.forecast_moments(is_post=True, num_samples=ns, times_out=t_out, eps=eps, states=True, **dense)
        assert [n for n, _ in eng.profile_read()][-1] == "forecast_moments"              # the fused route, not the composition
        _agree(composed, {n: (fused[n][0].double(), fused[n][1].double()) for n in names}, "composed against fused")


def test_output_files(tmp_path):
    """save_forecast_moments: <curve>_<post|prior>_forecast_{mean,sd}.npy, [B, C, T_out] each, and forecast_times.npy."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    B, t_out = batch["observations"].shape[0], m.horizon_times(5)
    eng.rng_seed(8)
    files = m.save_forecast_moments(str(tmp_path / "f"), is_post=True, num_samples=5, times_out=t_out, **batch)
    files += m.save_forecast_moments(str(tmp_path / "f"), is_post=False, num_samples=5, times_out=t_out, **batch)
    want = sorted(["%s_%s_forecast_%s.npy" % (cv, p, k) for cv in ("mu_50", "mu_75", "mu_25") for p in ("post", "prior") for k in ("mean", "sd")]
                  + ["forecast_times.npy"])
    assert sorted(set(os.path.basename(f) for f in files)) == want == sorted(os.listdir(str(tmp_path / "f")))
    eng.rng_set_counter(0)
    res = m.forecast_moments(is_post=True, num_samples=5, times_out=t_out, **batch)
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float32 and np.isfinite(a).all() and a.shape == ((91,) if f.endswith("forecast_times.npy") else (B, 3, 91))
    assert np.array_equal(np.load(str(tmp_path / "f" / "mu_75_post_forecast_sd.npy")), res["mu_75"][1].cpu().numpy())
    assert np.array_equal(np.load(str(tmp_path / "f" / "forecast_times.npy")), t_out.cpu().numpy())


def test_training_entry_point_with_forecast_steps(tmp_path, capsys):
    tr = importlib.import_module("training_cvs")
    cfg = EU.model_config("cvs")
    cfg.update(num_epochs=0, mini_batch_size=16, seq_len=86, num_samples=5)
    tr.train(cfg, batches_per_epoch=1, forecast_steps=5, results_dir=str(tmp_path / "res"))
    assert "FINAL TEST:" in capsys.readouterr().out
    got = sorted(os.listdir(str(tmp_path / "res")))
    assert got == sorted(["%s_post_forecast_%s.npy" % (cv, k) for cv in ("mu_50", "mu_75", "mu_25") for k in ("mean", "sd")] + ["forecast_times.npy"])
    assert np.load(str(tmp_path / "res" / "mu_50_post_forecast_mean.npy")).shape == (16, 3, 91)
    assert np.load(str(tmp_path / "res" / "forecast_times.npy")).shape == (91,)
