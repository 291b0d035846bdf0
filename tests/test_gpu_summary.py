"""GPU tests of the curve summaries (slode_curve_summary; Engine.curve_summary; MechanisticModel.curve_summary).

What is exact and what has a bar (tests/summary_util.py): extremes, first indices, crossing and the p_beyond counts are comparisons and
selections on the kernel's own fp32 curve values -- the values slode_recon_moments returns for one draw -- and are held to numpy on those
values EXACTLY; the two sums are held to (T + 1) 2^-24 sum |term| of the fp64 sum of the fp32 terms; the moments over draws are held to the
numpy restatement of the shifted accumulation bitwise.  Against the fp64 oracle the continuous slots have the bars of recon_moments and the
discontinuous ones the tolerant rules of SU.tolerant_violations, with nothing excluded.  The thresholds are the medians of the oracle's
central curves (SU.thresholds): inside the curves' range, with a near share under 1e-3 (asserted)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import recon_moments_util as RU
from tests import summary_util as SU
from tests.eval_gpu_util import (ADAPTIVE, DEV, ENV_KEYS, SIZES, WIDTHS, _captured, _count_calls, _device_batch, _engine, _eps_dev, _model,
                                 _model_curves, _padded, _peak, _per_draw_curves, _refused, _same as _same_arrays)
from tests.eval_gpu_util import _summary

pytestmark = pytest.mark.gpu
FILL = -12345.5            # the outputs are pre-filled with it (NaN is a value the call writes): every element must be written


_same = functools.partial(_same_arrays, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _per_draw(case, is_post):
    """Computed once, shared by tests 1 and 2: B = 13, K = 7, explicit eps.  Per draw, the kernel's own fp32 curves (recon_moments with
    num_samples = 1) and the functionals, sd and counts of curve_summary with num_samples = 1, both senses; the thresholds from the oracle."""
    c = RU.build(case, "rk4", B=13, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    thr = SU.thresholds(SU.oracle_draws(c, is_post))
    eps = c["eps"].to(DEV)
    f = {sense: [_summary(eng, flat, c, is_post, thr, sense, eps=eps[k].contiguous(), ns=1, obs_d=obs_d, labels=labels) for k in range(7)]
         for sense in (1, -1)}
    return c, eng, flat, thr, _per_draw_curves(eng, flat, c, is_post, obs_d, labels), f


PER_DRAW = ["cvs_ald", "proc_gauss", "challenge_gauss"]


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", PER_DRAW)
def test_per_draw_exactness_against_the_kernels_own_curves(case, is_post):
    """(1) Slots 0 - 3, 6, 7 and the counts equal numpy's on the fp32 curves of recon_moments exactly (first index on ties, t_* elements of
    times); slots 4 and 5 within the summation bar; sd exactly 0 where not NaN.  challenge_gauss has second grid points within two bars of
    the extreme on most rows: only a same-bits comparison can hold t_peak there."""
    c, eng, flat, thr, curves, f = _per_draw(case, is_post)
    times = c["times"].numpy()
    for sense in (1, -1):
        for k in range(7):
            mean, sd, pb = f[sense][k]
            want = SU.functionals(curves[k], times, thr, sense)
            for slot in (0, 1, 2, 3, 6, 7):
                assert np.array_equal(mean[..., slot].astype(np.float64), want[..., slot], equal_nan=True), (case, sense, k, SU.NAMES[slot])
            bar_auc, bar_tb = SU.sum_bars(curves[k], times)
            ra, rt = np.abs(mean[..., 4] - want[..., 4]) / bar_auc, np.abs(mean[..., 5] - want[..., 5]) / bar_tb
            assert ra.max() <= 1.0 and rt.max() <= 1.0, (case, sense, k, ra.max(), rt.max())
            assert np.array_equal(pb, SU.beyond(curves[k], thr, sense).astype(np.float32)), (case, sense, k)
            assert np.array_equal(np.isnan(sd), np.isnan(mean)) and np.all(sd[~np.isnan(sd)] == 0.0)
    print("%s %s: thr %s, rows that cross %.2f" % (case, "post" if is_post else "prior", thr, np.mean([m[0][..., 7] for m in f[1]])))


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", PER_DRAW)
def test_moments_over_draws_bitwise(case, is_post):
    """(2) One call with num_samples = 7 on the same noise equals SU.draw_moments_f32 of the seven per-draw values bitwise (slot 6 over the
    crossing draws, NaN where none); p_beyond is the sum of the per-draw counts over 7.  A threshold above every curve: slots 5 and 7
    exactly 0, slot 6 NaN, p_beyond all 0; one below every curve: crossed = 1, t_hit = t_0, time_beyond = sum w_i within the bar."""
    c, eng, flat, thr, curves, f = _per_draw(case, is_post)
    times = c["times"].numpy()
    for sense in (1, -1):
        mean, sd, pb = _summary(eng, flat, c, is_post, thr, sense)
        wm, ws = SU.draw_moments_f32(np.stack([m[0] for m in f[sense]]))
        assert _same(mean, wm), (case, sense, np.argwhere(~((mean == wm) | (np.isnan(mean) & np.isnan(wm))))[:5])
        assert _same(sd, ws), (case, sense, np.argwhere(~((sd == ws) | (np.isnan(sd) & np.isnan(ws))))[:5])
        assert _same(pb, RU._f32(np.stack([m[2] for m in f[sense]]).sum(0)) / np.float32(7))
    Cn = curves.shape[3]
    hi, lo = [float(curves.max()) + 1.0] * Cn, [float(curves.min()) - 1.0] * Cn
    w = SU.weights_f32(times).astype(np.float64)
    for thr_c, sense in ((hi, 1), (lo, -1)):                                              # never beyond
        mean, sd, pb = _summary(eng, flat, c, is_post, thr_c, sense)
        assert np.all(mean[..., 5] == 0.0) and np.all(mean[..., 7] == 0.0) and np.all(sd[..., 5] == 0.0) and np.all(sd[..., 7] == 0.0)
        assert np.isnan(mean[..., 6]).all() and np.isnan(sd[..., 6]).all() and np.all(pb == 0.0)
    for thr_c, sense in ((lo, 1), (hi, -1)):                                              # always beyond
        mean, sd, pb = _summary(eng, flat, c, is_post, thr_c, sense)
        assert np.all(mean[..., 7] == 1.0) and np.all(mean[..., 6] == times[0]) and np.all(sd[..., 6] == 0.0) and np.all(pb == 1.0)
        assert np.abs(mean[..., 5] - w.sum()).max() <= (c["T"] + 1) * SU.U * w.sum() + SU.U * w.sum()


def _against_the_oracle(eng, flat, c, tag, per_draw):
    """(3) Continuous bars and the count rule on one call with the case's draws; with ``per_draw`` the tolerant rules at num_samples = 1."""
    times = c["times"].numpy()
    span = float(times[-1] - times[0])
    obs_d, labels = _device_batch(c)
    ns = c["ns"]
    for is_post in (True, False):
        v = SU.oracle_draws(c, is_post)                                                    # [Q, ns, B, C, T]
        thr = SU.thresholds(v)
        vk = np.moveaxis(v, 1, 0)
        for sense in (1, -1):
            t = "%s %s sense %d" % (tag, "post" if is_post else "prior", sense)
            mean, sd, pb = _summary(eng, flat, c, is_post, thr, sense, obs_d=obs_d, labels=labels)
            wm, ws = SU.oracle_moments(SU.functionals(vk, times, thr.astype(np.float64), sense))
            SU.check_continuous(mean.astype(np.float64), sd.astype(np.float64), wm, ws, np.abs(v).max(-1).max(1), span, t)
            SU.check_counts(pb, ns, vk, thr, sense, t)
            cross_o = SU.beyond(vk, thr.astype(np.float64), sense).any(-1).mean(0)
            assert np.all(np.abs(mean[..., 7] - cross_o) <= SU.near(vk, thr).any(-1).sum(0) / ns + 1e-6), t
        if per_draw:
            eps = c["eps"].to(DEV)
            for sense in (1, -1):
                got = np.stack([_summary(eng, flat, c, is_post, thr, sense, eps=eps[k].contiguous() if ns > 1 else eps[0].contiguous(), ns=1, sd=False, p=False,
                                         obs_d=obs_d, labels=labels)[0] for k in range(ns)])
                bad = SU.tolerant_violations(got.astype(np.float64), vk, times, thr, sense)
                print("%s %s sense %d: rows that break a tolerant rule %s" % (tag, "post" if is_post else "prior", sense, bad))
                assert all(n == 0 for _, n in bad), (tag, is_post, sense, bad)


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_against_the_fp64_oracle(case, solver):
    c = RU.build(case, solver, ns=7)
    eng = _engine(c)
    _against_the_oracle(eng, eng.pack(c["p"]), c, "%s/%s" % (case, solver), per_draw=True)


@pytest.mark.parametrize("case,B,ns,env", SIZES, ids=["%s-B%d-ns%d%s" % (c, B, ns, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, ns, e in SIZES])
def test_sizes_and_instantiations(case, B, ns, env, monkeypatch):
    """(4) B on both sides of the 64- and 256-thread edges, the persistent loop on 5 and 2 workgroups, the run-time-S build, ns in {1, 2, 7,
    200}, T = 300 (two rounds of thread <-> t) and T = 86 (ragged row walks; T = 142 is challenge_ald in the oracle test), NaN-poisoned
    workspace, pre-filled outputs."""
    c = RU.build(case, "rk4", B=B, ns=ns)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    _against_the_oracle(eng, flat, c, "%s B=%d ns=%d %s" % (case, B, ns, env), per_draw=False)


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_noise_and_independence(case, monkeypatch):
    """(5) In-kernel noise equals the same rows passed explicitly, bitwise, and the counter ends at n + 1; two grids are bitwise equal; a
    repeat is bitwise equal; p_beyond = None and sd = None leave the other outputs bitwise unchanged; thr = None gives NaN in slots 5 - 7
    and leaves slots 0 - 4 bitwise unchanged."""
    c = RU.build(case, "midpoint", ns=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        thr = SU.thresholds(SU.oracle_draws(c, is_post))
        a = _summary(eng, flat, c, is_post, thr)
        for other in (_summary(eng, flat, c, is_post, thr), _summary(loop, flat, c, is_post, thr)):
            assert all(_same(x, y) for x, y in zip(a, other))
        lean = _summary(eng, flat, c, is_post, thr, sd=False, p=False)
        assert _same(lean[0], a[0]) and lean[1] is None and lean[2] is None
        assert _same(_summary(eng, flat, c, is_post, thr, p=False)[1], a[1])
        bare = _summary(eng, flat, c, is_post, None, p=False)
        assert np.isnan(bare[0][..., 5:]).all() and np.isnan(bare[1][..., 5:]).all()
        assert _same(bare[0][..., :5], a[0][..., :5]) and _same(bare[1][..., :5], a[1][..., :5])
        for e in (eng, loop):
            e.rng_seed(77, first_trajectory=1000)
            e.rng_set_counter(5)
        drawn = _summary(eng, flat, c, is_post, thr, eps=None)
        assert eng.rng_state() == (77, 1000, 6)
        rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
        given = _summary(eng, flat, c, is_post, thr, eps=rows)
        assert eng.rng_state() == (77, 1000, 6)                                   # explicit noise draws nothing
        drawn_loop = _summary(loop, flat, c, is_post, thr, eps=None)
        assert all(_same(x, y) and _same(x, z) for x, y, z in zip(drawn, given, drawn_loop))


def test_launches_and_graph_capture():
    """(6) Posterior: "weff", "enc_fwd2", "curve_summary" on one stream; prior: "curve_summary" alone.  One capture and one replay equal the
    stream-launched call bitwise; capturing executes nothing (the threshold travels by value: nothing is read from the host at replay)."""
    c = RU.build("cvs_ald", "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    thr = [float(x) for x in SU.thresholds(SU.oracle_draws(c, True))]
    eng.profile_enable(True)
    _summary(eng, flat, c, True, thr)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "curve_summary"]
    _summary(eng, flat, c, False, thr)
    assert [n for n, _ in eng.profile_read()] == ["curve_summary"]
    eng.profile_enable(False)
    outs = [torch.zeros(3, c["B"], 3, 8, device=DEV), torch.zeros(3, c["B"], 3, 8, device=DEV), torch.zeros(3, c["B"], 3, c["T"], device=DEV)]
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    want = _captured(lambda: eng.curve_summary(flat, bt, c["B"], True, 7, thr, 1, *outs), outs)
    assert all(_same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(outs, want)) and float(outs[2].abs().max()) > 0.0


def test_refusals_by_name(monkeypatch):
    """(7) Every refusal names its reason, draws nothing and launches nothing (rng_state, profile_read)."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd import engine as E
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)

    def refused(eng, match, obs=obs_d, ns=2, particles=1, is_post=True, null_obs=False, thr=(0.1, 0.2, 0.3), sense=1, p=None):
        flat = eng.pack(c["p"])
        bt = eng.make_batch(obs, labels, None)
        if null_obs:
            bt.obs = None
        err = _refused(eng, lambda: eng.curve_summary(flat, bt, c["B"], is_post, ns, thr, sense, None, True, p, particles=particles), match)
        assert err.status == -1 and "slode_curve_summary" in str(err)

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s .*reduce recon_samples instead" % solver, is_post=solver != "bosh3")
    eng = _engine(c, monkeypatch)
    for is_post in (True, False):
        refused(eng, "particles = 2", particles=2, is_post=is_post)
        refused(eng, "num_samples = 0", ns=0, is_post=is_post)
        refused(eng, "exceeds 2\\^30 - 1 noise rows", ns=2 ** 30, is_post=is_post)
        refused(eng, "sense = 0", sense=0, is_post=is_post)
        refused(eng, "thr\\[1\\] = nan is not finite", thr=(0.1, float("nan"), 0.3), is_post=is_post)
        refused(eng, "thr\\[2\\] = -inf is not finite", thr=(0.1, 0.2, float("-inf")), is_post=is_post)
        refused(eng, "p_beyond needs a threshold", thr=None, p=True, is_post=is_post)
    with pytest.raises(ValueError, match="one per channel"):
        eng.curve_summary(eng.pack(c["p"]), eng.make_batch(obs_d, labels, None), c["B"], True, 2, (0.1, 0.2), 1, None)
    refused(eng, "batch->obs is NULL", null_obs=True)
    refused(eng, "observation strides", obs=_padded(obs_d))
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    # tables beyond the LDS of one CU only with the counters: T = 1024 with S = 8, C = 4, three heads
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    big = E.Engine(E.proc_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    big.profile_enable(True)
    flat0 = torch.zeros(big.n_params, device=DEV)
    bt = big.make_batch(torch.zeros(2, 4, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["proc"]], None)
    for is_post in (True, False):
        with pytest.raises(L.SlodeError, match="LDS tables of T = 1024, S = 8, C = 4, with p_beyond .*drop p_beyond"):
            big.curve_summary(flat0, bt, 2, is_post, 2, [0.5] * 4, 1, None, True, True)
    assert big.rng_state()[2] == 0
    with pytest.raises(L.SlodeError, match="no profiled step"):
        big.profile_read()
    with pytest.raises(L.SlodeError, match="with p_beyond"):
        big.curve_summary_plan(2, True)
    assert big.curve_summary_plan(2, False) <= 160 * 1024
    mean, sd, pb = big.curve_summary(flat0, bt, 2, False, 2, [0.5] * 4, 1, None, True)     # without the counters the same shape is taken
    assert [n for n, _ in big.profile_read()] == ["curve_summary"] and pb is None and bool(torch.isfinite(mean[..., :6]).all())


# ---- the model layer ---------------------------------------------------------------------------------------------------------------------
def _check_model(res, m, v, thr, sense, tag, per_draw=None):
    """The dict against the decoder's curves v [Q, ns, B, C, T] of the same draws: continuous slots by the bars, counts by the count rule
    (two fp32 evaluations, each within the bar of the truth: the decoder's curves stand in for the oracle at twice the bar -- here the
    rule is applied with the bar itself, which is the stricter reading)."""
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    times = torch.as_tensor(m.times).float().cpu().numpy()
    vk = np.moveaxis(v, 1, 0)
    wm, ws = SU.oracle_moments(SU.functionals(vk, times, np.asarray(thr, np.float64), sense))
    mean = np.stack([np.stack([res[n][k][0].double().cpu().numpy() for k in SU.NAMES], -1) for n in names])
    sd = np.stack([np.stack([res[n][k][1].double().cpu().numpy() for k in SU.NAMES], -1) for n in names])
    SU.check_continuous(mean, sd, wm, ws, np.abs(v).max(-1).max(1), float(times[-1] - times[0]), tag)
    if "p_beyond" in res[names[0]]:
        SU.check_counts(np.stack([res[n]["p_beyond"].cpu().numpy() for n in names]), v.shape[1], vk, thr, sense, tag)


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_dict_keys_and_shapes(fam):
    m, batch = _model(fam)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    ns = 6
    for is_post in (True, False):
        eng.rng_seed(21)
        eng.rng_set_counter(3)
        eps = eng.rng_normal(3, ns * B).view(ns, B, -1)
        v = _model_curves(m, batch, is_post, eps)
        thr = SU.thresholds(v)
        eng.profile_enable(True)
        res = m.curve_summary(is_post=is_post, num_samples=ns, thresholds=torch.tensor(thr), sense="above", pointwise=True, **batch)
        assert [k for k, _ in eng.profile_read()] == (["weff", "enc_fwd2", "curve_summary"] if is_post else ["curve_summary"])
        eng.profile_enable(False)
        assert eng.rng_state() == (21, 0, 4) and set(res) == set(names)
        for n in names:
            assert set(res[n]) == set(SU.NAMES) | {"p_beyond"} and tuple(res[n]["p_beyond"].shape) == (B, Cn, T)
            assert all(tuple(t.shape) == (B, Cn) for k in SU.NAMES for t in res[n][k])
        _check_model(res, m, v, thr, 1, "%s %s" % (fam, "post" if is_post else "prior"))
        plain = m.curve_summary(is_post=is_post, num_samples=ns, eps=eps, **batch)
        assert all(torch.equal(plain[n][k][0], res[n][k][0]) for n in names for k in SU.NAMES[:5])
        assert all(torch.isnan(plain[n][k][0]).all() for n in names for k in SU.NAMES[5:]) and "p_beyond" not in plain[names[0]]


@pytest.mark.parametrize("why", ["dopri5", "strided"])
def test_composed_route_where_the_engine_refuses(why, monkeypatch):
    """dopri5, a padded observation tensor: the engine refuses, curve_summary composes the dict from recon_samples -- one drawing call, the
    counter at n + 1 -- and agrees with those curves reduced here; on the fixed-grid model the fused call (dense observations, same noise)
    agrees with the composed route's curves within the same bars, the discontinuous slots per draw by the tolerant rules."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch)
    eng = m._bind().engine
    B, ns = batch["observations"].shape[0], 6
    dense = dict(batch)
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    calls = _count_calls(monkeypatch, eng, "curve_summary")
    eng.rng_seed(11)
    eng.rng_set_counter(2)
    eps = eng.rng_normal(2, ns * B).view(ns, B, -1)
    v = _model_curves(m, batch, True, eps)
    thr = SU.thresholds(v)
    drawn = m.curve_summary(is_post=True, num_samples=ns, thresholds=thr, sense="below", pointwise=True, **batch)
    assert eng.rng_state() == (11, 0, 3) and len(calls) == 1                        # refused once, then composed
    given = m.curve_summary(is_post=True, num_samples=ns, thresholds=thr, sense="below", pointwise=True, eps=eps, **batch)
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    assert all(torch.equal(given[n][k][0].nan_to_num(), drawn[n][k][0].nan_to_num()) for n in names for k in SU.NAMES)
    _check_model(given, m, v, thr, -1, "%s composed" % why)
    if why == "strided":
        calls.clear()
        fused = m.curve_summary(is_post=True, num_samples=ns, thresholds=thr, sense="below", pointwise=True, eps=eps, **dense)
        assert len(calls) == 1
        _check_model(fused, m, v, thr, -1, "fused against the composed route's curves")
        times = torch.as_tensor(m.times).float().cpu().numpy()
        got = []
        for k in range(ns):
            one = m.curve_summary(is_post=True, num_samples=1, thresholds=thr, sense="below", eps=eps[k:k + 1], **dense)
            got.append(np.stack([np.stack([one[n][s][0].double().cpu().numpy() for s in SU.NAMES], -1) for n in names]))
        bad = SU.tolerant_violations(np.stack(got), np.moveaxis(v, 1, 0), times, thr, -1)
        print("fused per draw against the composed route's curves: rows that break a tolerant rule %s" % (bad,))
        assert all(n == 0 for _, n in bad), bad


def test_memory_stays_below_one_materialised_tensor():
    """After a warm-up call, the peak of torch.cuda.max_memory_allocated of the fused call at B = 64, K = 64 over the allocation before it
    stays below ONE materialised [B, C, T, K] tensor."""
    m, batch = _model("cvs")
    batch = {k: torch.cat([v] * 4)[:64].contiguous() for k, v in batch.items()}
    batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    thr = [0.5] * Cn
    m.curve_summary(is_post=True, num_samples=8, thresholds=thr, pointwise=True, **batch)
    eng.profile_enable(True)
    peak = _peak(lambda: m.curve_summary(is_post=True, num_samples=64, thresholds=thr, pointwise=True, **batch))
    assert [n for n, _ in eng.profile_read()][-1] == "curve_summary"           # the fused route, not the composition
    eng.profile_enable(False)
    one = B * Cn * T * 64 * 4
    print("peak over the allocation before the call: fused B=64 K=64 %d B; one materialised [B, C, T, K] tensor %d B" % (peak, one))
    assert B == 64 and peak < one


def test_output_files(tmp_path):
    """save_curve_summary over two batches: the arrays and the slot names, equal to curve_summary from the same generator state, the
    trajectories in loader order."""
    m, batch = _model("challenge")
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    halves = [{k: v[:9] for k, v in batch.items()}, {k: v[9:] for k, v in batch.items()}]
    halves = [dict(h, observations=h["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)) for h in halves]
    thr = [0.3] * Cn
    eng.rng_seed(8)
    files = m.save_curve_summary(str(tmp_path / "cs"), halves, True, 5, thresholds=thr, sense="above")
    assert eng.rng_state()[2] == 2
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    want = ["summary_%s_post_%s.npy" % (n, k) for n in names for k in ("mean", "sd")] + ["summary_slots.npy"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "cs"))) == sorted(want)
    assert np.load(files[-1]).tolist() == list(SU.NAMES)
    mean, sd = np.load(files[0]), np.load(files[1])
    assert mean.shape == sd.shape == (B, Cn, 8) and mean.dtype == np.float32 and np.isfinite(mean[..., :6]).all()
    eng.rng_set_counter(1)
    res = m.curve_summary(is_post=True, num_samples=5, thresholds=thr, **halves[1])
    assert np.array_equal(mean[9:, :, 0], res[names[0]]["peak"][0].cpu().numpy()) and np.array_equal(sd[9:, :, 4], res[names[0]]["auc"][1].cpu().numpy())
    print(m.summary_line(mean, "post", True))
