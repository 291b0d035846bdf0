"""GPU tests of PSIS leave-one-out (slode_pointwise_loo): the exact parts against the kernel's own per-draw log-densities (K single-draw
pointwise_density calls), the fit against the fp64 numpy restatement of tests/loo_util.py on those same values, the whole against the fp64
oracle of tests/pointwise_util.py, the boundaries of the smoothing, invariance (tile, grid, noise source), the mask and the summary, a given
posterior, the refusals, the launches, capture and replay, the model layer and --loo.  Shapes: B <= 3 and T in {14, 20} (the conv encoder
takes no window shorter than 14 points), one T = 300 challenge case in which a thread owns two time points; the model layer on the
86-point model of tests/eval_stats_util.py."""
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import loo_util as LU
from tests import pointwise_util as PU
from tests.eval_gpu_util import (ADAPTIVE, _captured, _check_fit, _check_own_sums, _density, _device_batch, _engine, _lay, _loo, _model, _own_l, _padded,
                                 _peak, _refused)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("K", [1, 4, 20, 21, 64])
def test_exact_parts_and_the_fit_on_the_kernels_own_log_densities(K):
    """Explicit noise.  tail_out == sort(l, 0)[:M + 1] and the lppd plane == pointwise_density's plane 0, both bitwise; at K = 1
    elpd_loo == lppd == l_0 bitwise; elpd_loo and khat against the restatement on those same values (the split check of the fit)."""
    case, T = (("cvs_ald", 20), ("cvs_gauss", 14), ("proc_gauss", 20), ("challenge_ald", 14), ("proc_ald", 20))[(1, 4, 20, 21, 64).index(K)]
    c = LU.build(case, T, 3, K)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    l = _own_l(eng, flat, c, obs_d, labels)
    point, summary, tail = _loo(eng, flat, c, obs_d=obs_d, labels=labels)
    M = LU.tail_len(K)
    assert np.array_equal(tail.cpu().numpy(), np.sort(l, 0)[:M + 1])
    assert torch.equal(point[2], _density(eng, flat, c, c["eps"], K, obs_d, labels)[0])
    if K == 1:
        assert np.array_equal(point[2].cpu().numpy(), l[0]) and torch.equal(point[0], point[2]) and torch.isinf(point[1]).all()
    assert torch.all(point[0] <= point[2] + 2.0 ** -21 * (1 + point[2].abs()))
    _check_fit(point, l.astype(np.float64), "%s K=%d" % (case, K))
    _check_own_sums(point, summary)


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_planes_match_the_fp64_oracle(case, solver):
    """K = 64, explicit noise, six model classes x three solvers, against the restatement on the ORACLE's l_k.  Bars: the restatement's
    sensitivity to perturbations of l_k by bar_k[i] (tests/pointwise_util.py).  Left out: points whose khat bar exceeds 0.05 -- at most 2 %
    of the points -- or the ALD crossing exclusion of tests/pointwise_util.py under its own cap; the union at most 2 % of the points and at
    least half the trajectories without a left-out point, all asserted on the oracle alone (LU.left_out; a configuration that missed at
    the default noise seed has another: LU.ORACLE_SEEDS)."""
    c = LU.build(case, 20 if "ald" in case else 14, 3, 64, solver, seed=LU.ORACLE_SEEDS.get((case, solver), 21))
    want = PU.oracle_points(c)
    eb, kb = LU.bars(want["ell"], want["bar"])
    skip = LU.left_out(want, kb, "%s %s" % (case, solver))
    e, k = LU.psis(want["ell"])
    eng = _engine(c)
    point, summary, _ = _loo(eng, eng.pack(c["p"]), c, tail=False)
    got = point.double().cpu().numpy()
    assert np.isfinite(got[0]).all() and np.array_equal(np.isinf(got[1])[~skip], np.isinf(k)[~skip])
    re = np.where(skip, 0.0, np.abs(got[0] - e) / eb)
    rk = np.where(skip | np.isinf(k), 0.0, np.abs(np.where(np.isinf(got[1]), 0.0, got[1]) - np.where(np.isinf(k), 0.0, k)) / kb)
    rl = np.where(want["excl"].any(0), 0.0, np.abs(got[2] - LU.lppd(want["ell"])) / (want["bar"].max(0) + 2.0 ** -22 * np.abs(got[2])))
    print("%s %s: error / bar: elpd_loo %.3f, khat %.3f, lppd %.3f (left out %d of %d points)" % (case, solver, re.max(), rk.max(), rl.max(), int(skip.sum()), skip.size))
    assert re.max() <= 1.0 and rk.max() <= 1.0 and rl.max() <= 1.0
    _check_own_sums(point, summary)


def test_boundaries_of_the_smoothing():
    """K = 20 (M = 4): khat = +inf everywhere and elpd_loo is the plain importance-sampling estimate; K = 21: the first smoothing;
    duplicated noise rows that tie with the cutoff shorten the tail (n_tail < M); all rows equal: elpd_loo within 2^-22 |l| of l."""
    c = LU.build("cvs_gauss", 14, 3, 21)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    l = _own_l(eng, flat, c, obs_d, labels).astype(np.float64)
    p20 = _loo(eng, flat, c, K=20, eps=c["eps"][:20], obs_d=obs_d, labels=labels)[0].double().cpu().numpy()
    harmonic = -np.log(np.exp(-(l[:20] - l[:20].min(0))).mean(0)) + l[:20].min(0)
    assert np.isinf(p20[1]).all() and np.all(np.abs(p20[0] - harmonic) <= 20 * 2.0 ** -23 * np.maximum(1.0, np.abs(harmonic)))
    p21 = _loo(eng, flat, c, obs_d=obs_d, labels=labels)[0]
    assert torch.isfinite(p21[1]).all()
    # 64 draws of which rows 0 .. 15 are one row: wherever that row is among the 14 smallest it ties with the cutoff
    cd = LU.build("cvs_gauss", 14, 3, 64)
    cd["eps"][:16] = cd["eps"][0]
    ld = _own_l(eng, flat, cd, obs_d, labels).astype(np.float64)
    n_tail = np.array([LU.psis_point(ld[:, i, j, t])[2] for i in range(3) for j in range(3) for t in range(14)])
    assert n_tail.min() < 13 and n_tail.max() == 13                                       # both kinds of point occur
    pd_, _, td = _loo(eng, flat, cd, obs_d=obs_d, labels=labels)
    assert np.array_equal(td.cpu().numpy(), np.sort(ld, 0)[:14].astype(np.float32))
    _check_fit(pd_, ld, "duplicated rows")
    ce = LU.build("cvs_gauss", 14, 3, 21)
    ce["eps"][:] = ce["eps"][0]
    pe = _loo(eng, flat, ce, obs_d=obs_d, labels=labels)[0]
    l0 = torch.from_numpy(_own_l(eng, flat, ce, obs_d, labels)[0]).to(DEV)
    assert torch.isinf(pe[1]).all() and torch.all((pe[0] - l0).abs() <= 2.0 ** -22 * l0.abs())


@pytest.mark.parametrize("K,B", [(21, 2), (64, 1)])
def test_a_thread_owns_two_time_points(K, B):
    """The 300-point challenge window in ONE sweep (the plan's tile is 300: threads 0 .. 43 own the points t and t + 256 of every channel in
    the fold, the sorted buffer and the finish).  tail_out and lppd bitwise against K single-draw pointwise_density calls, the fit against
    the restatement on those values, at every point."""
    c = LU.build("challenge_gauss", 300, B, K)
    eng = _engine(c)
    assert eng.loo_plan(B, K)[:2] == (300, 1)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    l = _own_l(eng, flat, c, obs_d, labels)
    point, summary, tail = _loo(eng, flat, c, obs_d=obs_d, labels=labels)
    assert np.array_equal(tail.cpu().numpy(), np.sort(l, 0)[:LU.tail_len(K) + 1])
    assert torch.equal(point[2], _density(eng, flat, c, c["eps"], K, obs_d, labels)[0])
    _check_fit(point, l.astype(np.float64), "challenge_gauss T=300 K=%d" % K)
    _check_own_sums(point, summary)


def test_many_draws_take_more_than_one_sweep():
    """K = 1024 at B = 2 on the 300-point challenge window: depth 97, more than one sweep.  With l from 1024 single-draw
    pointwise_density calls: tail_out and the lppd plane bitwise at every point; elpd_loo (the fp32 sum over 1024 draws less the fp64 tail)
    and khat inside the bars of the split check on every seventh time point and on the points around the sweeps' and the threads' seams."""
    K = 1024
    c = LU.build("challenge_gauss", 300, 2, K)
    eng = _engine(c)
    tile, sweeps, depth, lds = eng.loo_plan(2, K)
    assert depth == 97 and sweeps > 1 and tile < 256 and lds <= 160 * 1024
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    l = _own_l(eng, flat, c, obs_d, labels)
    point, summary, tail = _loo(eng, flat, c, obs_d=obs_d, labels=labels)
    assert np.array_equal(tail.cpu().numpy(), np.sort(l, 0)[:97])
    assert torch.equal(point[2], _density(eng, flat, c, c["eps"], K, obs_d, labels)[0])
    _check_own_sums(point, summary)
    ts = sorted(t for t in set(range(0, 300, 7)) | {tile - 1, tile, 2 * tile - 1, 2 * tile, 255, 256, 299} if t < 300)
    _check_fit(point[:, :, :, ts], l[:, :, :, ts].astype(np.float64), "challenge_gauss T=300 K=1024")


def test_bitwise_independent_of_tile_grid_and_noise_source(monkeypatch):
    """tile in {1, 7, T, auto}, 2 and 5 workgroups, and in-kernel noise against the rows rng_normal(n + k, B) passed explicitly: every
    output bitwise equal; the counter goes n -> n + K once whatever the sweeps, and stays for explicit noise."""
    c = LU.build("cvs_ald", 20, 3, 21)
    eng = _engine(c, monkeypatch)
    flat = eng.pack(c["p"])
    mask = _lay(PU.prefix_mask(c), True)
    base = _loo(eng, flat, c, mask=mask)
    assert all(torch.isfinite(x[~torch.isinf(x)]).all() for x in base)
    for tile in (1, 7, 20):
        assert eng.loo_plan(3, 21, tile)[1] == -(-20 // tile)
        assert all(torch.equal(x, y) for x, y in zip(base, _loo(eng, flat, c, mask=mask, tile=tile)))
    loops = [_engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": g}) for g in ("2", "5")]
    for e in loops:
        assert all(torch.equal(x, y) for x, y in zip(base, _loo(e, flat, c, mask=mask, tile=7)))
    for e in [eng] + loops:
        e.rng_seed(77, first_trajectory=1000)
        e.rng_set_counter(5)
    drawn = _loo(eng, flat, c, eps=None, mask=mask, tile=7)                                # three sweeps, one count
    assert eng.rng_state() == (77, 1000, 26)
    rows = torch.stack([eng.rng_normal(5 + k, 3) for k in range(21)]).contiguous()
    given = _loo(eng, flat, c, eps=rows, mask=mask)
    assert eng.rng_state() == (77, 1000, 26)
    drawn_loop = _loo(loops[0], flat, c, eps=None, mask=mask)
    assert loops[0].rng_state() == (77, 1000, 26)
    for x, y, z in zip(drawn, given, drawn_loop):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("case", ["cvs_gauss", "proc_ald"])
def test_mask_partitions_the_summary_and_never_touches_the_planes(case):
    """Both dense layouts (cvs: the [B,C,T] view of [B,T,C]; proc: contiguous): the planes with a mask are bitwise those without; the
    slots are the fp64 sums of the call's own planes over the two sides."""
    c = LU.build(case, 20, 3, 24)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    m = PU.prefix_mask(c)
    m[1, 0, 2] = 0.0
    m[2] = 0.0                                                                            # a trajectory with no point in: max khat = -inf
    masked = _loo(eng, flat, c, mask=_lay(m, c["fam"] != "proc"))
    plain = _loo(eng, flat, c)
    assert torch.equal(masked[0], plain[0]) and torch.equal(masked[2], plain[2])
    _check_own_sums(masked[0], masked[1], m.numpy())
    _check_own_sums(plain[0], plain[1])
    assert masked[1][2, 4].item() == float("-inf") and masked[1][2, 2].item() == 0.0


def test_posterior_input_and_refusals_leave_pointwise_density_unchanged(monkeypatch):
    """loc / scale read back from a J = 0 posterior_refine: bitwise the default call; a refined posterior moves the result.  Every refusal
    names its reason, draws nothing, launches nothing, writes nothing -- and pointwise_density afterwards is bitwise what it was."""
    from structured_latent_odes_amd import _lib as L
    c = LU.build("cvs_ald", 20, 3, 21)
    eng = _engine(c, monkeypatch)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    B, Cn, T = c["obs"].shape
    before = _density(eng, flat, c, c["eps"], 21, obs_d, labels)
    bt = eng.make_batch(obs_d, labels, c["eps"][:4].to(DEV).contiguous(), particles=4)
    loc0, scale0 = eng.posterior_refine(flat, bt, B, 4, 0, grad0=False, trace=False, best_step=False)[:2]
    base = _loo(eng, flat, c, obs_d=obs_d, labels=labels)
    same = _loo(eng, flat, c, obs_d=obs_d, labels=labels, loc=loc0, scale=scale0)
    assert all(torch.equal(x, y) for x, y in zip(base, same))
    loc, scale = eng.posterior_refine(flat, bt, B, 4, 3, grad0=False, trace=False, best_step=False)[:2]
    moved = _loo(eng, flat, c, obs_d=obs_d, labels=labels, loc=loc, scale=scale)
    assert not torch.equal(base[0], moved[0]) and torch.isfinite(moved[0]).all()

    def refused(e, match, obs=obs_d, K=21, raw=None, **kw):
        f = e.pack(c["p"])
        point = torch.full((3, B, Cn, T), float("nan"), device=DEV)
        summary = torch.full((B, 8), float("nan"), device=DEV)
        b2 = e.make_batch(obs, labels, None)
        if raw is None:
            call = lambda: e.pointwise_loo(f, b2, B, K, point=point, summary=summary, **kw)
        else:                                                                            # what Engine.pointwise_loo cannot express
            call = lambda: e._batch_call(e.lib.slode_pointwise_loo, f, b2, B, 1, K, *(x if isinstance(x, int) else e._p(x) for x in raw(point, summary)))
        _refused(e, call, match)
        torch.cuda.synchronize(DEV)
        assert torch.isnan(point).all() and torch.isnan(summary).all()

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s" % solver)
    refused(eng, "num_draws = 0", K=0)
    refused(eng, "observation strides", obs=_padded(obs_d))
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    eng = _engine(c, monkeypatch)
    some = torch.zeros(B, c["eps"].shape[2], device=DEV)
    refused(eng, "scale is NULL", raw=lambda p, s: (None, some, None, 0, p, s, None))
    refused(eng, "loc is NULL", raw=lambda p, s: (None, None, some, 0, p, s, None))
    refused(eng, "point / summary is NULL", raw=lambda p, s: (None, None, None, 0, None, s, None))
    refused(eng, "16-byte aligned", raw=lambda p, s: (None, None, None, 0, p, s.view(-1)[1:], None))
    refused(eng, "tile = -1", raw=lambda p, s: (None, None, None, -1, p, s, None))
    refused(eng, "tile = 21", raw=lambda p, s: (None, None, None, 21, p, s, None))
    refused(eng, "num_draws = 33554432", K=1 << 25)
    with pytest.raises(L.SlodeError, match="num_draws = 33554432"):
        eng.loo_plan(B, 1 << 25)
    assert torch.equal(before, _density(eng, flat, c, c["eps"], 21, obs_d, labels))


def test_launches_and_graph_capture():
    """Three launches, "weff", "enc_fwd2", "pointwise_loo", on one stream, with and without a given posterior and over several sweeps.
    One capture and one replay of a call with explicit noise equal the stream-launched call bitwise."""
    c = LU.build("cvs_ald", 20, 3, 21)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    B, Cn, T = c["obs"].shape
    some = torch.ones(B, c["eps"].shape[2], device=DEV)
    for kw in ({}, dict(loc=some, scale=some), dict(tile=7)):
        eng.profile_enable(True)
        _loo(eng, flat, c, obs_d=obs_d, labels=labels, **kw)
        assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "pointwise_loo"]
        eng.profile_enable(False)
    point, summary, tail = torch.zeros(3, B, Cn, T, device=DEV), torch.zeros(B, 8, device=DEV), torch.zeros(6, B, Cn, T, device=DEV)
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=21)
    want = _captured(lambda: eng.pointwise_loo(flat, bt, B, 21, point=point, summary=summary, tail=tail), (point, summary, tail))
    assert all(torch.equal(x, y) for x, y in zip((point, summary, tail), want)) and want[0].abs().sum().item() > 0.0


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_call_its_files_and_its_peak_allocation(fam, tmp_path):
    """pointwise_loo(num_draws=24) on three trajectories: the dict's shapes, p_loo = lppd - elpd_loo, bitwise Engine.pointwise_loo from the
    same generator state, lppd bitwise pointwise_density's; the composed route (forced) within the fit's bars of the fused one on the same
    noise; save_pointwise_loo over two batches; the fused call allocates less than one [B, C, T, K] tensor beyond its outputs."""
    m, batch = _model(fam)
    batch = {k: v[:3].contiguous() if k != "observations" else v[:3] for k, v in batch.items()}
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    K = 24
    eng.rng_seed(4321, first_trajectory=300)
    eng.rng_set_counter(9)
    res = m.pointwise_loo(num_draws=K, **batch)
    assert eng.rng_state() == (4321, 300, 9 + K)
    planes = ("elpd_loo", "khat", "lppd", "p_loo")
    assert set(res) == set(planes) | set(m.LOO_NAMES)
    assert all(tuple(res[n].shape) == (B, Cn, T) for n in planes) and all(tuple(res[n].shape) == (B,) for n in m.LOO_NAMES)
    assert torch.equal(res["p_loo"], res["lppd"] - res["elpd_loo"]) and torch.isfinite(res["elpd_loo"]).all() and torch.isfinite(res["khat"]).all()
    eng.rng_set_counter(9)
    labs = [batch[l].reshape(B, -1).to(torch.float32).contiguous() for l in m.LABELS]
    point, summary, _ = eng.pointwise_loo(m._bind().flat, eng.make_batch(batch["observations"], labs, None, particles=K), B, K)
    assert torch.equal(point[0], res["elpd_loo"]) and torch.equal(point[1], res["khat"]) and torch.equal(summary[:, 0], res["elpd_loo_in"])
    eng.rng_set_counter(9)
    assert torch.equal(res["lppd"], m.pointwise_density(num_draws=K, **batch)["lppd"])
    _check_own_sums(point, summary)
    eps = torch.randn(64, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(2)).to(DEV)  # (K = 64: the parity size)
    fused = m.pointwise_loo(num_draws=64, eps=eps, return_tail=True, **batch)
    composed = m.pointwise_loo(num_draws=64, eps=eps, return_tail=True, max_sweeps=0, **batch)  # (every plan needs more than 0 sweeps)
    assert set(fused) == set(composed) and torch.equal(fused["n_in"], composed["n_in"])
    assert torch.allclose(fused["tail"], composed["tail"], rtol=2e-4, atol=2e-4) and torch.allclose(fused["lppd"], composed["lppd"], rtol=2e-4, atol=2e-4)
    # (the two routes differ in their fp32 curves; the smoothing amplifies that at a few ill-conditioned points: the 2 % of the oracle test)
    d = (fused["elpd_loo"] - composed["elpd_loo"]).abs() / (1.0 + fused["elpd_loo"].abs())
    assert torch.quantile(d.flatten(), 0.98).item() <= 1e-3
    # khat: both routes smooth the same points, and all but the 2 % of the oracle test agree within its bar cap of 0.05
    assert torch.equal(torch.isinf(fused["khat"]), torch.isinf(composed["khat"]))
    dk = torch.where(torch.isinf(fused["khat"]), torch.zeros_like(d), (fused["khat"] - composed["khat"]).abs())
    print("%s: fused against composed at K = 64: khat differs by more than 0.05 at %.4f of the points (largest %.4f); elpd_loo 98th percentile %.2e"
          % (fam, (dk > 0.05).float().mean().item(), dk.max().item(), torch.quantile(d.flatten(), 0.98).item()))
    assert (dk > 0.05).float().mean().item() <= 0.02
    eng.rng_set_counter(9)
    files = m.save_pointwise_loo(str(tmp_path / "res"), [batch, batch], K)
    assert [os.path.basename(f) for f in files] == ["pointwise_elpd_loo_post.npy", "pointwise_khat_post.npy", "loo_post.npy"]
    arrays = [np.load(f) for f in files]
    assert [a.shape for a in arrays] == [(2 * B, Cn, T)] * 2 + [(2 * B, 8)] and all(a.dtype == np.float32 for a in arrays)
    assert np.array_equal(arrays[0][:B], res["elpd_loo"].cpu().numpy()) and np.array_equal(arrays[2][:B], summary.cpu().numpy())
    obs = batch["observations"].repeat(20, 1, 1) if fam == "proc" else batch["observations"].permute(0, 2, 1).repeat(20, 1, 1).contiguous().permute(0, 2, 1)
    wide = dict({k: v.repeat(20, *([1] * (v.dim() - 1))) for k, v in batch.items() if k != "observations"}, observations=obs)
    m.pointwise_loo(num_draws=64, **wide)                                                 # (workspace and batch tensors exist from here on)
    peak = _peak(lambda: m.pointwise_loo(num_draws=64, **wide))
    outputs = (3 + 1) * 60 * Cn * T * 4 + 60 * 8 * 4
    assert peak - outputs < 60 * Cn * T * 64 * 4, (peak, outputs)


def test_adaptive_solver_takes_the_composed_route():
    m, batch = _model("cvs", solver="dopri5")
    batch = {k: v[:3].contiguous() if k != "observations" else v[:3] for k, v in batch.items()}
    eng = m._bind().engine
    eng.rng_seed(5, first_trajectory=0)
    eng.rng_set_counter(3)
    got = m.pointwise_loo(num_draws=21, **batch)
    assert eng.rng_state()[2] == 3 + 21                                                   # the counter moves as on the engine route
    assert torch.isfinite(got["elpd_loo"]).all() and torch.isfinite(got["khat"]).all() and torch.all(got["elpd_loo"] <= got["lppd"] + 1e-5)


def test_training_entry_point_with_loo(tmp_path, monkeypatch, capsys):
    """One --loo 21 run of training.main on a synthetic loader, one epoch: the three files beside the run's other files and the line."""
    from structured_latent_odes_amd import training as T
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.models.mechanistic_cvs_Gauss import MechanisticModelGauss

    def load_config():
        cfg = EU.model_config("cvs")
        cfg.update(mini_batch_size=16, seq_len=86)
        return cfg

    monkeypatch.chdir(tmp_path)
    T.main("cvs", load_config, MechanisticModel, MechanisticModelGauss, ["--epochs", "1", "--batches-per-epoch", "1", "--loo", "21"])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("loo: ")]
    assert "FINAL TEST:" in out and len(line) == 1 and line[0].startswith("loo: K=21  n=16  elpd_loo=") and "share(khat>0.7)=" in line[0]
    assert not [ln for ln in out.splitlines() if ln.startswith("waic: ")]                 # off unless asked for
    res = tmp_path / ("results_%s" % load_config().model)
    table, k = np.load(str(res / "loo_post.npy")), np.load(str(res / "pointwise_khat_post.npy"))
    assert table.shape == (16, 8) and k.shape == (16, 3, 86) and np.isfinite(table).all() and np.all(table[:, 2] == 3 * 86)
    assert line[0] == MechanisticModel.loo_line(table, k, 21)
