"""GPU tests of the sample quantiles (slode_recon_quantiles; Engine.recon_quantiles; MechanisticModel.recon_quantiles).

What is exact and what has a bar (tests/quantile_util.py): an order statistic is a selection among the kernel's own fp32 curve values -- the
values slode_recon_moments returns for one draw -- so one call over K draws is held to np.sort of the K per-draw curves and QU.select
BITWISE, for every level set, tile and launch grid.  Against the fp64 oracle an order statistic is 1-Lipschitz in the sup norm over the
draws: every output lies within RU.MEAN_BAR max(1, max_k |v_k|) of np.quantile on the oracle's draws, with nothing excluded."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import quantile_util as QU
from tests import recon_moments_util as RU
from tests import summary_util as SU
from tests.eval_gpu_util import (ADAPTIVE, DEV, ENV_KEYS, SIZES, WIDTHS, _captured, _count_calls, _device_batch, _engine, _eps_dev, _model,
                                 _model_curves, _padded, _peak, _per_draw_curves, _recon_moments, _refused, _same as _same_arrays)
from tests.eval_gpu_util import _quantiles

pytestmark = pytest.mark.gpu
FILL = -12345.5            # the outputs are pre-filled with it: every element must be written
SETS = list(QU.LEVEL_SETS)


_same = functools.partial(_same_arrays, equal_nan=False)


@functools.lru_cache(maxsize=None)
def _per_draw(case, is_post):
    """Computed once, shared by tests 1 and 2: B = 13, K = 7, explicit eps.  The kernel's own fp32 curves per draw (recon_moments with
    num_samples = 1), stacked [7, Q, B, C, T]."""
    c = RU.build(case, "rk4", B=13, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    return c, eng, flat, _per_draw_curves(eng, flat, c, is_post, obs_d, labels)


PER_DRAW = ["cvs_ald", "proc_gauss", "challenge_gauss"]


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", PER_DRAW)
def test_exact_selection_among_the_kernels_own_curves(case, is_post):
    """(1) One call with num_samples = 7 equals QU.select of the seven sorted per-draw curves of recon_moments bitwise, for every level set;
    levels 0 and 1 are the min / max of the stack exactly; K = 1: every level returns the curve itself."""
    c, eng, flat, curves = _per_draw(case, is_post)
    srt = np.sort(curves, axis=0)
    for name in SETS:
        levels = QU.LEVEL_SETS[name]
        got = _quantiles(eng, flat, c, is_post, levels)
        want = QU.select(srt, levels)
        assert _same(got, want), (case, name, np.argwhere(got != want)[:5])
        for i, q in enumerate(levels):
            if q == 0.0:
                assert np.array_equal(got[i], curves.min(0))
            if q == 1.0:
                assert np.array_equal(got[i], curves.max(0))
    one = _quantiles(eng, flat, c, is_post, QU.LEVEL_SETS["eight"], eps=c["eps"][3].to(DEV).contiguous(), ns=1)
    assert all(np.array_equal(one[i], curves[3]) for i in range(8))


@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_tiling_grid_and_noise_source_independence(case, monkeypatch):
    """(2) tile in {1, 16, T} and the auto tile; 2 and 5 workgroups (persistent loop); in-kernel noise against the same rows from
    slode_rng_normal on the same counter: all bitwise equal; the counter moves by num_samples whatever the number of sweeps."""
    c, eng, flat, curves = _per_draw(case, True)
    T, B = c["T"], c["B"]
    loops = [_engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": g}) for g in ("2", "5")]
    for is_post in (True, False):
        for name in ("band", "eight"):
            levels = QU.LEVEL_SETS[name]
            base = _quantiles(eng, flat, c, is_post, levels)
            for tile in (1, 16, T):
                assert _same(_quantiles(eng, flat, c, is_post, levels, tile=tile), base), (case, name, tile)
            for lp in loops:
                assert _same(_quantiles(lp, flat, c, is_post, levels), base) and _same(_quantiles(lp, flat, c, is_post, levels, tile=16), base)
        levels = QU.LEVEL_SETS["five"]
        for e in [eng] + loops:
            e.rng_seed(77, first_trajectory=1000)
        rows = eng.rng_normal(5, 7 * B).view(7, B, -1).contiguous()
        given = _quantiles(eng, flat, c, is_post, levels, eps=rows)
        for e in [eng] + loops:
            for tile in (0, 1, 16):
                e.rng_set_counter(5)
                drawn = _quantiles(e, flat, c, is_post, levels, eps=None, tile=tile)
                assert e.rng_state() == (77, 1000, 5 + 7), (tile, e.rng_state())
                assert _same(drawn, given), (case, is_post, tile)
        eng.rng_set_counter(5)
        _quantiles(eng, flat, c, is_post, levels, eps=rows)
        assert eng.rng_state() == (77, 1000, 5)                                   # explicit noise draws nothing


def _against_the_oracle(eng, flat, c, tag, level_names, check_plan=None):
    """(3) Every output within RU.MEAN_BAR max(1, max_k |v_k|) of np.quantile(method="linear") on the oracle's draws; nothing excluded."""
    obs_d, labels = _device_batch(c)
    for is_post in (True, False):
        v = np.moveaxis(SU.oracle_draws(c, is_post), 1, 0)                                 # [ns, Q, B, C, T]
        bar = QU.oracle_bar(v)
        for name in level_names:
            levels = QU.LEVEL_SETS[name]
            got = _quantiles(eng, flat, c, is_post, levels, obs_d=obs_d, labels=labels).astype(np.float64)
            want = np.quantile(v, np.asarray(levels, dtype=np.float64), axis=0, method="linear")
            r = float((np.abs(got - want) / bar).max())
            print("%s %s %s: error / bar %.3e" % (tag, "post" if is_post else "prior", name, r))
            assert np.isfinite(got).all() and r <= 1.0, (tag, is_post, name, r)
    if check_plan:
        check_plan()


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_against_the_fp64_oracle(case, solver):
    c = RU.build(case, solver, ns=7)
    eng = _engine(c)
    _against_the_oracle(eng, eng.pack(c["p"]), c, "%s/%s" % (case, solver), SETS)


@pytest.mark.parametrize("case,B,ns,env", SIZES, ids=["%s-B%d-ns%d%s" % (c, B, ns, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, ns, e in SIZES])
def test_sizes_and_instantiations(case, B, ns, env, monkeypatch):
    """(4) B on both sides of the 64- and 256-thread edges, the persistent loop on 5 and 2 workgroups, the run-time-S build, ns in {1, 2, 7,
    200}, T = 300 (two rounds of thread <-> t in one tile) and T = 86, NaN-poisoned workspace, pre-filled outputs.  ns = 200: the band
    (D = 12, one sweep) and the median (D = 200, several sweeps)."""
    c = RU.build(case, "rk4", B=B, ns=ns)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))

    def check_plan():
        if ns == 200:
            band, median = eng.quantile_plan(B, ns, QU.LEVEL_SETS["band"]), eng.quantile_plan(B, ns, QU.LEVEL_SETS["median"])
            print("plans at ns = 200: band %s, median %s" % (band, median))
            assert band[1:4] == (1, 6, 6) and median[2:4] == (200, 0) and median[1] > 1
    _against_the_oracle(eng, flat, c, "%s B=%d ns=%d %s" % (case, B, ns, env), ("band", "median") if ns == 200 else ("five", "envelope"), check_plan)


def test_refusals_by_name_and_nothing_left_behind(monkeypatch):
    """(5) Every refusal names its reason, draws nothing and launches nothing; afterwards recon_moments is bitwise what it was before."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd import engine as E
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)
    eng = _engine(c, monkeypatch)
    flat = eng.pack(c["p"])
    before = [t.cpu().numpy() for t in _recon_moments(eng, flat, c, True)]

    def refused(e, match, obs=obs_d, ns=2, particles=1, is_post=True, null_obs=False, levels=(0.025, 0.975), tile=0):
        fl = e.pack(c["p"])
        bt = e.make_batch(obs, labels, None)
        if null_obs:
            bt.obs = None
        err = _refused(e, lambda: e.recon_quantiles(fl, bt, c["B"], is_post, ns, levels, None, tile, particles=particles), match)
        assert err.status == -1 and "slode_recon_quantiles" in str(err)

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s .*sort recon_samples instead" % solver, is_post=solver != "bosh3")
    eng = _engine(c, monkeypatch)
    for is_post in (True, False):
        refused(eng, "particles = 2", particles=2, is_post=is_post)
        refused(eng, "num_samples = 0", ns=0, is_post=is_post)
        refused(eng, "exceeds 2\\^30 - 1 noise rows", ns=2 ** 30, is_post=is_post)
        refused(eng, "n_levels = 0 out of range \\[1, 8\\]", levels=(), is_post=is_post)
        refused(eng, "n_levels = 9 out of range \\[1, 8\\]", levels=(0.5,) * 9, is_post=is_post)
        refused(eng, "levels\\[1\\] = 1.25 is not in \\[0, 1\\]", levels=(0.5, 1.25), is_post=is_post)
        refused(eng, "levels\\[0\\] = nan is not in \\[0, 1\\]", levels=(float("nan"),), is_post=is_post)
        refused(eng, "tile = -1 out of range", tile=-1, is_post=is_post)
        refused(eng, "tile = %d out of range" % (c["T"] + 1), tile=c["T"] + 1, is_post=is_post)
    refused(eng, "batch->obs is NULL", null_obs=True)
    refused(eng, "observation strides", obs=_padded(obs_d))
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    # LDS: T = 1024 with S = 8, C = 4, three heads; a median of 1024 draws fits one time point per sweep, a given tile of 4 does not; 4096 draws: none
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    big = E.Engine(E.proc_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    big.profile_enable(True)
    flat0 = torch.zeros(big.n_params, device=DEV)
    bt = big.make_batch(torch.zeros(2, 4, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["proc"]], None)
    for is_post in (True, False):
        with pytest.raises(L.SlodeError, match="tile = 4 does not fit: the LDS tables of T = 1024, S = 8, C = 4, depth = 1024 \\+ 0"):
            big.recon_quantiles(flat0, bt, 2, is_post, 1024, (0.5,), None, 4)
        with pytest.raises(L.SlodeError, match="depth = 4096 \\+ 0 of num_samples = 4096.*sort recon_samples instead"):
            big.recon_quantiles(flat0, bt, 2, is_post, 4096, (0.5,))
    assert big.rng_state()[2] == 0
    with pytest.raises(L.SlodeError, match="no profiled step"):
        big.profile_read()
    assert big.quantile_plan(2, 1024, (0.5,))[:4] == (1, 1024, 1024, 0)
    out = big.recon_quantiles(flat0, bt, 2, False, 4096, (0.0, 1.0))                        # the envelope of 4096 draws: D = 2, one sweep
    assert [n for n, _ in big.profile_read()] == ["recon_quantiles"] and bool(torch.isfinite(out).all())
    # the refusals left nothing behind
    eng = _engine(c, monkeypatch)
    after = [t.cpu().numpy() for t in _recon_moments(eng, eng.pack(c["p"]), c, True)]
    assert all(_same(a, b) for a, b in zip(before, after))


def test_launches_and_graph_capture():
    """(6) Posterior: "weff", "enc_fwd2", "recon_quantiles" on one stream; prior: "recon_quantiles" alone, whatever the number of sweeps.  One
    capture and one replay equal the stream-launched call bitwise; capturing executes nothing (the level table travels by value)."""
    c = RU.build("cvs_ald", "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    levels = QU.LEVEL_SETS["five"]
    eng.profile_enable(True)
    for tile in (0, 16):
        _quantiles(eng, flat, c, True, levels, tile=tile)
        assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "recon_quantiles"]
        _quantiles(eng, flat, c, False, levels, tile=tile)
        assert [n for n, _ in eng.profile_read()] == ["recon_quantiles"]
    eng.profile_enable(False)
    outs = [torch.zeros(5, 3, c["B"], 3, c["T"], device=DEV)]
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    want = _captured(lambda: eng.recon_quantiles(flat, bt, c["B"], True, 7, levels, outs[0], 16), outs)
    assert _same(outs[0].cpu().numpy(), want[0].cpu().numpy()) and float(outs[0].abs().max()) > 0.0
    assert _same(outs[0].cpu().numpy(), _quantiles(eng, flat, c, True, levels))


# ---- the model layer ---------------------------------------------------------------------------------------------------------------------
def _check_model(res, m, v, levels, tag):
    """The dict against np.quantile of the decoder's curves v [ns, Q, B, C, T] of the same draws, within the bar of test 3: recon_samples'
    curves come from the decoder's kernels (slode_ode_solve_fwd + slode_decode_heads), another fp32 evaluation of the same curve, each
    within the per-value bar of the truth; they stand in for the oracle and the bar itself is applied, which is the stricter reading."""
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    got = np.stack([res[n].double().cpu().numpy() for n in names], 1)                      # [Lv, Q, B, C, T]
    want = np.quantile(v, np.asarray(levels, dtype=np.float64), axis=0, method="linear")
    r = float((np.abs(got - want) / QU.oracle_bar(v)).max())
    print("%s: error / bar %.3e" % (tag, r))
    assert r <= 1.0, (tag, r)


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_dict_keys_and_shapes(fam):
    m, batch = _model(fam)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    ns, levels = 6, QU.LEVEL_SETS["five"]
    for is_post in (True, False):
        eng.rng_seed(21)
        eng.rng_set_counter(3)
        eps = eng.rng_normal(3, ns * B).view(ns, B, -1)
        v = _model_curves(m, batch, is_post, eps, heads_axis=1)
        eng.profile_enable(True)
        res = m.recon_quantiles(is_post=is_post, num_samples=ns, levels=levels, **batch)
        assert [k for k, _ in eng.profile_read()] == (["weff", "enc_fwd2", "recon_quantiles"] if is_post else ["recon_quantiles"])
        eng.profile_enable(False)
        assert eng.rng_state() == (21, 0, 3 + ns) and set(res) == set(names) | {"levels"} and res["levels"].tolist() == list(levels)
        assert all(tuple(res[n].shape) == (5, B, Cn, T) and res[n].dtype == torch.float32 for n in names)
        _check_model(res, m, v, levels, "%s %s" % (fam, "post" if is_post else "prior"))
        given = m.recon_quantiles(is_post=is_post, num_samples=ns, levels=levels, eps=eps, **batch)
        assert all(torch.equal(given[n], res[n]) for n in names)
        default = m.recon_quantiles(is_post=is_post, num_samples=ns, eps=eps, **batch)
        assert default["levels"].tolist() == [0.025, 0.975] and bool((default[names[0]][0] <= default[names[0]][1]).all())


@pytest.mark.parametrize("why", ["dopri5", "strided"])
def test_composed_route_where_the_engine_refuses(why, monkeypatch):
    """dopri5, a padded observation tensor: the engine refuses, recon_quantiles sorts recon_samples -- one drawing call, the counter moved by
    num_samples as the engine call leaves it -- and equals the restatement on those curves BITWISE (the composed curves have recon_samples'
    bits: a sort and QU.select of them is the whole computation).  On the fixed-grid model the engine route (dense observations, same noise)
    has the fused kernel's bits, not recon_samples': the two agree within the bar of test 3."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch)
    eng = m._bind().engine
    B, ns, levels = batch["observations"].shape[0], 6, QU.LEVEL_SETS["eight"]
    dense = dict(batch)
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    calls = _count_calls(monkeypatch, eng, "recon_quantiles")
    eng.rng_seed(11)
    eng.rng_set_counter(2)
    eps = eng.rng_normal(2, ns * B).view(ns, B, -1)
    v = _model_curves(m, batch, True, eps, heads_axis=1)
    drawn = m.recon_quantiles(is_post=True, num_samples=ns, levels=levels, **batch)
    assert eng.rng_state() == (11, 0, 2 + ns) and len(calls) == 1                     # refused once, then composed
    given = m.recon_quantiles(is_post=True, num_samples=ns, levels=levels, eps=eps, **batch)
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    assert all(torch.equal(given[n], drawn[n]) for n in names)
    want = QU.select(np.sort(v.astype(np.float32), axis=0), levels)                         # [Lv, Q, B, C, T]
    assert all(_same(given[n].cpu().numpy(), want[:, q]) for q, n in enumerate(names))
    _check_model(given, m, v, levels, "%s composed" % why)
    if why == "strided":
        calls.clear()
        fused = m.recon_quantiles(is_post=True, num_samples=ns, levels=levels, eps=eps, **dense)
        assert len(calls) == 1
        _check_model(fused, m, v, levels, "fused against the composed route's curves")


def test_max_sweeps_switch(monkeypatch):
    """A median at 200 draws keeps 200 values per column -- at T = 86 more than 2 sweeps: the composed route by default, the engine with
    max_sweeps raised; both within the bar."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    B, ns = 2, 200
    batch = {k: v[:B] for k, v in batch.items()}
    batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    sweeps = eng.quantile_plan(B, ns, (0.5,))[1]
    assert sweeps > 2
    calls = _count_calls(monkeypatch, eng, "recon_quantiles")
    eng.rng_seed(5)
    eps = eng.rng_normal(0, ns * B).view(ns, B, -1)
    v = _model_curves(m, batch, True, eps, heads_axis=1)
    composed = m.recon_quantiles(is_post=True, num_samples=ns, levels=(0.5,), eps=eps, **batch)
    assert calls == []
    fused = m.recon_quantiles(is_post=True, num_samples=ns, levels=(0.5,), eps=eps, max_sweeps=sweeps, **batch)
    assert calls == [1]
    band = m.recon_quantiles(is_post=True, num_samples=ns, eps=eps, **batch)
    assert calls == [1, 1]                                                              # the band: one sweep, the engine
    _check_model(composed, m, v, (0.5,), "median composed")
    _check_model(fused, m, v, (0.5,), "median fused, %d sweeps" % sweeps)
    _check_model(band, m, v, (0.025, 0.975), "band fused")


def test_memory_stays_below_one_materialised_tensor():
    """After a warm-up call, the peak of torch.cuda.max_memory_allocated of the fused call at B = 64, K = 64 over the allocation before it
    stays below ONE materialised [B, C, T, K] tensor."""
    m, batch = _model("cvs")
    batch = {k: torch.cat([v] * 4)[:64].contiguous() for k, v in batch.items()}
    batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    m.recon_quantiles(is_post=True, num_samples=8, **batch)
    eng.profile_enable(True)
    peak = _peak(lambda: m.recon_quantiles(is_post=True, num_samples=64, **batch))
    assert [n for n, _ in eng.profile_read()][-1] == "recon_quantiles"           # the fused route, not the composition
    eng.profile_enable(False)
    one = B * Cn * T * 64 * 4
    print("peak over the allocation before the call: fused B=64 K=64 %d B; one materialised [B, C, T, K] tensor %d B" % (peak, one))
    assert B == 64 and peak < one


def test_output_files(tmp_path):
    """save_recon_quantiles over two batches: the arrays and the levels, equal to recon_quantiles from the same generator state, the
    trajectories in loader order."""
    m, batch = _model("challenge")
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    halves = [{k: v[:9] for k, v in batch.items()}, {k: v[9:] for k, v in batch.items()}]
    halves = [dict(h, observations=h["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)) for h in halves]
    levels = (0.1, 0.5, 0.9)
    eng.rng_seed(8)
    files = m.save_recon_quantiles(str(tmp_path / "q"), halves, True, 5, levels)
    assert eng.rng_state()[2] == 10
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    want = ["%s_post_sample_quantiles.npy" % n for n in names] + ["sample_quantile_levels.npy"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "q"))) == sorted(want)
    assert np.load(files[-1]).tolist() == list(levels)
    q = np.load(files[0])
    assert q.shape == (B, 3, Cn, T) and q.dtype == np.float32 and np.isfinite(q).all() and (q[:, 0] <= q[:, 1]).all() and (q[:, 1] <= q[:, 2]).all()
    eng.rng_set_counter(5)
    res = m.recon_quantiles(is_post=True, num_samples=5, levels=levels, **halves[1])
    assert np.array_equal(q[9:], res[names[0]].transpose(0, 1).cpu().numpy())
    print(m.quantile_line(q, np.load(files[-1]), batch["observations"].cpu().numpy(), "post"))
