"""The eval-side statistics AWAY from the initialisation: the entries of tests/eval_regime_util.py (each call's own small case under the
regimes of tests/regime_util.py) through the HIP kernels.  tests/test_gpu_regimes.py holds the forward these calls share (through
traj_bounds); this file holds what each kernel does with the draws afterwards -- folds, sorted buffers, the on-chip fp64 Pareto fit, ranks,
counts and ratios -- in two ways per call: the split check (the statistic against its restatement on the kernel's OWN per-draw values, which
separates it from the forward) and the oracle check (against the fp64 oracle at the call's own bars under the bar rule of
tests/regime_util.py; the fp32 CPU oracle's distances are computed here, never taken from a kernel).  tests/test_eval_regimes_cpu.py asserts
on the oracles alone every condition relied on here.  Outputs are pre-filled with NaN (or the util's fill value); every test prints its worst
error-to-bar ratio.  Shapes: B <= 4, T <= 300, K <= 64."""
import numpy as np
import pytest
import torch

from tests import attribution_util as AU
from tests import band_util as BU
from tests import calibration_util as KU
from tests import cohort_util as CU
from tests import eval_regime_util as E
from tests import forecast_util as FU
from tests import intervene_util as IU
from tests import loo_util as LU
from tests import mechanism_util as MU
from tests import pointwise_util as PU
from tests import quantile_util as QU
from tests import recon_moments_util as RU
from tests import refine_util as RFU
from tests import regime_util as G
from tests import summary_util as SU
from tests import traj_bounds_util as TU
from tests.eval_gpu_util import (_attr, _band, _band_check_exact as _band_exact, _band_check_oracle as _band_oracle, _calib, _calib_own_curves as _own_curves,
                                 _check_fit, _check_own_sums, _cohort, _cohort_per_draw, _cohort_truth, _density, _device_batch, _engine, _forecast, _iv, _loo,
                                 _mech, _own_l, _per_draw_curves, _quantiles, _recon_moments, _summary)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POST, IMP = 0, 1


# ---- pointwise_density -------------------------------------------------------------------------------------------------------------------------
def _pw(eng, flat, c, weights, K=None, eps=None, obs_d=None, labels=None):
    """Engine.pointwise_density on the case's batch (``eps``: other noise rows, [K, B, L]); outputs pre-filled with NaN."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    e = c["eps"] if eps is None else eps
    K = e.shape[0] if K is None else K
    e = (e[0] if K == 1 else e).to(DEV).contiguous()
    B, Cn, T = c["obs"].shape
    point = torch.full((3, B, Cn, T), float("nan"), device=DEV)
    summary = torch.full((B, 8), float("nan"), device=DEV)
    loss = torch.full((K, B), float("nan"), device=DEV) if weights == IMP else False
    eng.pointwise_density(flat, eng.make_batch(obs_d, labels, e, particles=K), B, K, weights, point=point, summary=summary, loss_kb=loss)
    return point, summary, loss


@pytest.mark.parametrize("name,regime", E.DENSITY_ENTRIES)
def test_pointwise_density(name, regime):
    """Posterior mode, K = 8, B = 4.  Oracle check: planes and slots against PU.fold64 of the oracle's l at PU.bars under the bar rule, with
    PU.conditions asserted.  Split check: the planes against fold64 of the kernel's own per-draw l (8 single-draw calls): K 2^-23
    max(1, |value|) for lppd and mean_ll; for var_ll the same relative bar plus 2^-22 (max_k |l_k - mean|)^2, the rounding of the fp32
    differences that enter the kernel's fp64 shifted sums."""
    c = E.density_case(name, regime)
    tag = "density %s %s" % (name, regime)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    K, B = c["eps"].shape[:2]
    point, summary, _ = _pw(eng, flat, c, POST, obs_d=obs_d, labels=labels)
    lw = PU.log_weights(K, B)
    E.Density(c, tag).check(point, summary, lw, "posterior")
    assert torch.equal(summary[:, 7], torch.full((B,), float(K), device=DEV))
    own = np.stack([_pw(eng, flat, c, POST, eps=c["eps"][k:k + 1], obs_d=obs_d, labels=labels)[0][0].cpu().numpy() for k in range(K)]).astype(np.float64)
    planes, _ = PU.fold64(own, lw)
    got = point.double().cpu().numpy()
    rel = K * 2.0 ** -23 * np.maximum(1.0, np.abs(planes))
    bars = np.stack([rel[0], rel[1], rel[2] + 2.0 ** -22 * np.abs(own - planes[1][None]).max(0) ** 2])
    r = np.abs(got - planes) / bars
    print("%s split check: error / bar: lppd %.3f, mean_ll %.3f, var_ll %.3f (largest |l| %.3g, largest var_ll %.3g)"
          % (tag, r[0].max(), r[1].max(), r[2].max(), np.abs(own).max(), planes[2].max()))
    assert r.max() <= 1.0, (tag, r.max((1, 2, 3)))


@pytest.mark.parametrize("name", E.CASES)
def test_pointwise_density_importance_fold(name):
    """Importance mode at tight_noise with the noise scaled (E.IMPORTANCE_NOISE) so that the weights are not one-hot -- asserted on the
    reference weights (the fp64 oracle's losses): 1.5 < ESS < K - 0.5 on at least half the trajectories.  As
    test_gpu_pointwise.test_importance_fold_on_non_degenerate_weights: the kernel's own loss_kb for the weights (the losses themselves
    against TU.oracle_rows under the bar rule), the oracle's l for the points."""
    c = E.density_case(name, "tight_noise", importance=True)
    tag = "density %s tight_noise noise x %g" % (name, E.IMPORTANCE_NOISE[name])
    want, r32 = G.bounds_oracles(c)
    assert E.spread_weights(TU.reduce64(want["loss"])[2]), TU.reduce64(want["loss"])[2]
    eng = _engine(c)
    point, summary, loss = _pw(eng, eng.pack(c["p"]), c, IMP)
    loss = loss.double().cpu().numpy()
    rl = np.abs(loss - want["loss"]) / (TU.REL * want["mag"])
    print("%s importance: loss_kb error / bar %.3f (fp32 oracle / suite bar %.2f)" % (tag, rl.max(), r32))
    assert rl.max() <= 1.0
    K, B = loss.shape
    E.Density(c, tag).check(point, summary, PU.log_weights(K, B, loss), "importance")
    ess = TU.reduce64(loss)[2]
    assert np.all(np.abs(summary[:, 7].double().cpu().numpy() - ess) <= 1e-5 * K) and E.spread_weights(ess), ess


# ---- pointwise_loo -----------------------------------------------------------------------------------------------------------------------------
_loo_runs = {}


def _loo_run(name, regime, K):
    """(case, engine, packed parameters, device batch, the kernel's own l [K, B, C, T], (point, summary, tail)): once per entry."""
    key = (name, regime, K)
    if key not in _loo_runs:
        c = E.loo_case(name, regime, K)
        eng = _engine(c)
        flat = eng.pack(c["p"])
        obs_d, labels = _device_batch(c)
        _loo_runs[key] = (c, eng, flat, obs_d, labels, _own_l(eng, flat, c, obs_d, labels), _loo(eng, flat, c, obs_d=obs_d, labels=labels))
    return _loo_runs[key]


@pytest.mark.parametrize("name,regime,K", E.LOO_ENTRIES)
def test_pointwise_loo_on_the_kernels_own_log_densities(name, regime, K):
    """(a) The split check at EVERY point, no exclusion: tail_out == sort(l, 0)[:M + 1] and the lppd plane == pointwise_density's plane 0,
    both bitwise; elpd_loo and khat against the restatement on the kernel's own l (eval_gpu_util._check_fit: isinf(khat) agrees with the
    restatement everywhere, and no point's khat bar is infinite).  The Gauss entries put 10 - 40 % of their points on the log DBL_MIN clamp
    of the cutoff and on tails shorter than M (khat = +inf through n_tail < 5 included), every entry a quarter and more at khat > 1
    (tests/test_eval_regimes_cpu.py).  (c) The slots against the fp64 sums of the call's own planes."""
    c, eng, flat, obs_d, labels, l, (point, summary, tail) = _loo_run(name, regime, K)
    assert np.array_equal(tail.cpu().numpy(), np.sort(l, 0)[:LU.tail_len(K) + 1])
    assert torch.equal(point[2], _density(eng, flat, c, c["eps"], K, obs_d, labels)[0])
    assert torch.isfinite(point[0]).all() and torch.all(point[0] <= point[2] + 2.0 ** -21 * (1 + point[2].abs()))
    r = E.loo_reach(l)
    print("loo %s %s K=%d on the kernel's own l: %s" % (name, regime, K, r))
    _check_fit(point, l.astype(np.float64), "loo %s %s K=%d" % (name, regime, K), finite_bars=True)
    _check_own_sums(point, summary)


@pytest.mark.parametrize("name,regime,K", E.LOO_ENTRIES)
def test_pointwise_loo_against_the_fp64_oracle(name, regime, K):
    """(b) elpd_loo against LU.psis of the ORACLE's l at LU.bars' elpd bar and lppd at the bar of
    test_gpu_loo.test_planes_match_the_fp64_oracle, both at every point outside the ALD crossing exclusion, under the bar rule.  khat at
    the oracle level only where its bar is <= 0.05; the share of the points left out is printed and NOT capped: LU.left_out's 2 % cannot
    hold in these regimes -- measured on the oracle 10 - 23 % per entry, for every seed tried, because khat really is that sensitive to a
    1e-5 relative change of a curve once khat > 1 -- and the split check above holds khat at every point."""
    c, eng, flat, obs_d, labels, l, (point, summary, tail) = _loo_run(name, regime, K)
    o = E.Loo(c)
    assert E.crossing_ok(o.want)
    got = point.double().cpu().numpy()
    fe, fl = E.factor(o.r32[0]), E.factor(o.r32[1])
    re = np.where(o.crossing, 0.0, np.abs(got[0] - o.e) / (o.eb * fe))
    rl = np.where(o.crossing, 0.0, np.abs(got[2] - o.lppd) / (o.lb * fl))
    lvl = o.khat_level
    assert np.array_equal(np.isinf(got[1])[lvl], np.isinf(o.k)[lvl])
    fin = lvl & np.isfinite(o.k)
    rk = np.abs(np.where(fin, got[1], 0.0) - np.where(fin, o.k, 0.0)) / o.kb
    print("loo %s %s K=%d against the oracle: error / bar: elpd_loo %.3f, lppd %.3f, khat %.3f; bar factors %.2f, %.2f (fp32 oracle / suite bar %.3f, %.3f); "
          "khat compared at %.3f of the points (left out %.3f, %d on a crossing)"
          % (name, regime, K, re.max(), rl.max(), rk.max(), fe, fl, o.r32[0], o.r32[1], lvl.mean(), 1.0 - lvl.mean(), int(o.crossing.sum())))
    assert re.max() <= 1.0 and rl.max() <= 1.0 and rk.max() <= 1.0
    _check_own_sums(point, summary)


def test_pointwise_loo_is_bitwise_independent_of_tile_and_grid(monkeypatch):
    """(d) challenge_gauss at `all`, K = 64: tile in {1, 7, T, auto} and 2 and 5 workgroups in the persistent loop -- every output bitwise
    equal.  The clamp and the short tails must not depend on the sweep structure."""
    name, regime, K = "challenge_gauss", "all", 64
    c = E.loo_case(name, regime, K)
    eng = _engine(c, monkeypatch)
    flat = eng.pack(c["p"])
    base = _loo(eng, flat, c)
    T = c["T"]
    assert torch.isinf(base[0][1]).any() and torch.isfinite(base[0][1]).any() and torch.isfinite(base[0][0]).all()
    for tile in (1, 7, T):
        assert eng.loo_plan(c["B"], K, tile)[1] == -(-T // tile)
        assert all(torch.equal(x, y) for x, y in zip(base, _loo(eng, flat, c, tile=tile))), tile
    for grid in ("2", "5"):
        loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": grid})
        for tile in (0, 7):
            assert all(torch.equal(x, y) for x, y in zip(base, _loo(loop, flat, c, tile=tile))), (grid, tile)


# ---- posterior_refine --------------------------------------------------------------------------------------------------------------------------
def _refine(eng, flat, c, J):
    obs_d, labels = _device_batch(c)
    B, L, K = c["B"], c["ospec"].latent_dim, c["eps"].shape[0]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = eng.posterior_refine(flat, eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=K), B, K, J, RFU.LR, loc=nan(B, L), scale=nan(B, L),
                               elbo=nan(B, 2), grad0=nan(B, 2 * L), trace=nan(J + 1, B), best_step=torch.full((B,), -7, dtype=torch.int32, device=DEV))
    return {k: v.detach().double().cpu().numpy() for k, v in zip(("loc", "scale", "elbo", "grad0", "trace", "best_step"), out)}, obs_d, labels


@pytest.mark.parametrize("name,regime", E.REFINE_ENTRIES)
def test_posterior_refine(name, regime):
    """J = 0: elbo0 against slot 0 of traj_bounds to one fp32 ulp; grad0 against fp64 autograd, norm-wise per trajectory, under the bar
    rule.  J = 4: the fp64 oracle objective at the returned (loc, scale) equals elbo[:, 1] within the bar (RFU.objective_at; under the bar
    rule at that point), elbo[:, 1] <= elbo[:, 0], best_step == argmin(trace).  The trace is NOT compared with the fp64 loop here: Adam's
    steps at 1 / scale = 1e3 across the jumps of the ALD likelihood (and through Gauss scales of 1e-3) are no conditioned comparison --
    a first step of lr sign(g) moves the objective by thousands of bars, and which side of a jump an iterate lands on is decided by the
    last bit of a curve.  What the call returns is held instead: the posterior it hands back scores what it says."""
    c = E.refine_case(name, regime)
    tag = "refine %s %s" % (name, regime)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    o = E.refine_oracles(c)
    r0, obs_d, labels = _refine(eng, flat, c, 0)
    K = c["eps"].shape[0]
    bounds, _ = eng.traj_bounds(flat, eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=K), c["B"], K)
    want0 = bounds[:, 0].double().cpu().numpy()
    ulp = np.spacing(np.abs(want0).astype(np.float32)).astype(np.float64)
    assert all(np.isfinite(v).all() for v in r0.values()), tag
    assert np.all(np.abs(r0["elbo"][:, 0] - want0) <= ulp) and np.array_equal(r0["elbo"][:, 0], r0["elbo"][:, 1]) and not r0["best_step"].any()
    ge = RFU.norm_err(r0["grad0"], o["grad"])
    fe = np.abs(r0["elbo"][:, 0] - o["F"]) / o["f_bar"]
    r4, _, _ = _refine(eng, flat, c, RFU.J)
    F, bar, r32 = E.refine_objective_bar(c, r4["loc"], r4["scale"])
    err = np.abs(r4["elbo"][:, 1] - F) / bar
    print("%s: elbo0 against the oracle %.3f bar, grad0 %.2e / bar %.2e (fp32 oracle / suite bars %.2f, %.2f); J = 4: elbo against the oracle at the "
          "returned posterior %.3f bar (fp32 oracle / suite bar %.2f), best steps %s, improvement %.3g .. %.3g"
          % (tag, fe.max(), ge.max(), o["g_bar"], o["r32"][0], o["r32"][1], err.max(), r32, r4["best_step"].astype(int).tolist(),
             (r4["elbo"][:, 0] - r4["elbo"][:, 1]).min(), (r4["elbo"][:, 0] - r4["elbo"][:, 1]).max()))
    assert all(np.isfinite(v).all() for v in r4.values()), tag
    assert fe.max() <= 1.0 and ge.max() <= o["g_bar"], (tag, fe, ge)
    assert err.max() <= 1.0, (tag, err)
    assert np.array_equal(r4["elbo"][:, 0], r4["trace"][0]) and np.array_equal(r4["elbo"][:, 1], r4["trace"].min(0))
    assert np.all(r4["elbo"][:, 1] <= r4["elbo"][:, 0]) and np.array_equal(r4["best_step"], r4["trace"].argmin(0))
    assert np.array_equal(r4["elbo"][:, 0], r0["elbo"][:, 0])


# ---- the whole-curve calls -----------------------------------------------------------------------------------------------------------------------
# One entry = (call, case, regime): E.curve_case (B = 4, 7 draws, rk4; prior_scales on PRIOR draws, every other regime on posterior draws).
# Per entry: the SPLIT check against the call's restatement on the kernel's own per-draw curves (recon_moments with num_samples = 1), bitwise
# wherever the call's own test file is bitwise, and the ORACLE check at the call's own bars (under the bar rule where the util's oracle takes
# a dtype).  At `ties` channel 0 is exactly +0.0 in every draw -- sd exactly 0 in both precisions on a whole channel -- against observations
# of +0.0 and -0.0: that channel gets assertions of its own (what include/slode.h documents for a constant curve), and the comparison rules
# that excuse NEAR points (calibration, curve_summary: every point of a constant curve at its own threshold is near) run on the other channels.
U24 = 2.0 ** -24
BOUNDED = MU.ALL & ~(1 << MU.NAMES.index("set_point"))       # state, production, degradation, net_rate
_entries = {}


def _entry(call, name, regime, ns=E.CURVE_NS, curves=True):
    """(case, engine, packed parameters, device batch, is_post, the kernel's own curve of every draw [K, Q, B, C, T] (None unless ``curves``)):
    once per case, the calls on one build sharing it."""
    c = E.curve_case(call, name, regime, ns)
    post = E.is_post(regime)
    if id(c) not in _entries:
        eng = _engine(c)
        _entries[id(c)] = [c, eng, eng.pack(c["p"])] + list(_device_batch(c)) + [post, None]
    e = _entries[id(c)]
    if curves and e[6] is None:
        e[6] = _per_draw_curves(e[1], e[2], c, post, e[3], e[4])
    return tuple(e[:6]) + (e[6] if curves else None,)


def _plus_zero(a):
    a = np.asarray(a)
    return bool((a == 0.0).all()) and not bool(np.signbit(a).any())


def _ratio(err, bar):
    """Worst |err| / bar; an element whose bar is 0 must have no error."""
    err, bar = np.abs(np.asarray(err, np.float64)), np.asarray(bar, np.float64)
    assert np.all(err[bar == 0] == 0), "an element with a zero bar is off"
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


def _moments_against_own_curves(mean, sd, curves, tag):
    """mean / sd [Q, B, C, T] of a call that accumulates as recon_moments does, against np.mean / np.std (fp64) of the kernel's own per-draw
    curves at RU.accumulation_bars (their condition asserted); an element whose draws are all equal: mean that value, sd 0, exactly.
    The bars are relative: they hold for normal fp32 numbers.  A state that has decayed into the subnormal range (tripled dynamics weights
    over 200 - 300 time points: |x| below 2^-126) is rounded to a multiple of 2^-149 by every operation, so the mean's bar gets (n + 2)
    2^-149 for its n + 2 roundings; the squares d^2 of differences below 2^-75 vanish altogether, an absolute error of at most (n + 2)
    2^-149 on the variance, hence sqrt((n + 2) 2^-149) = 1e-22 on the sd (|sqrt a - sqrt b| <= sqrt |a - b|)."""
    v = curves.astype(np.float64)
    wm, ws = v.mean(0), v.std(0)
    assert np.all(np.abs(v - v[0]).max(0) <= RU.SPREAD * ws)
    bm, bs = RU.accumulation_bars(wm, ws, v.shape[0])
    tiny = (v.shape[0] + 2) * 2.0 ** -149
    bm, bs = bm + tiny * (np.abs(v).max(0) > 0), bs + np.sqrt(tiny) * (ws > 0)
    same = (curves == curves[0]).all(0)
    assert np.array_equal(mean[same], curves[0][same]) and not sd[same].any(), tag
    rm, rs = _ratio(mean - wm, bm), _ratio(sd - ws, bs)
    xm, xs = RU.shifted_moments_f32(curves)
    print("%s split check: error / accumulation bar: mean %.3f, sd %.3f (bitwise the restatement: mean %s, sd %s; %d elements with equal draws)"
          % (tag, rm, rs, np.array_equal(mean, xm), np.array_equal(sd, xs), int(same.sum())))
    assert rm <= 1.0 and rs <= 1.0, (tag, rm, rs)


def _moments_against_the_oracle(mean, sd, call, name, regime, tag):
    """RU.check's bars under the bar rule (E.moment_bars); returns the oracle's draws."""
    v64, v32 = E.draws(call, name, regime)
    m, s, bm, bs, r32 = E.moment_bars(v64, v32)
    rm, rs = _ratio(mean - m, bm), _ratio(sd - s, bs)
    print("%s oracle check: error / bar: mean %.3f, sd %.3f (fp32 oracle / suite bar %.3f, %.3f; level %.1f)" % (tag, rm, rs, r32[0], r32[1], np.abs(m).max()))
    assert np.isfinite(mean).all() and np.isfinite(sd).all() and rm <= 1.0 and rs <= 1.0, (tag, rm, rs)
    return v64, v32


@pytest.mark.parametrize("name,regime", E.curve_entries("recon_moments"))
def test_recon_moments(name, regime):
    c, eng, flat, obs_d, labels, post, curves = _entry("recon_moments", name, regime)
    tag = "recon_moments %s %s" % (name, regime)
    mean, sd = (t.cpu().numpy() for t in _recon_moments(eng, flat, c, post, obs_d=obs_d, labels=labels))
    _moments_against_own_curves(mean, sd, curves, tag)
    _moments_against_the_oracle(mean, sd, "recon_moments", name, regime, tag)
    if regime == "ties":
        assert _plus_zero(curves[:, :, :, 0]) and _plus_zero(mean[:, :, 0]) and _plus_zero(sd[:, :, 0])


@pytest.mark.parametrize("name,regime", E.curve_entries("recon_quantiles"))
def test_recon_quantiles(name, regime):
    """Split: every level set equals QU.select of the sorted per-draw curves BITWISE.  Oracle: within QU.oracle_bar of np.quantile on the
    oracle's draws, under the bar rule.  ties: every order statistic of channel 0 is exactly +0.0."""
    c, eng, flat, obs_d, labels, post, curves = _entry("recon_quantiles", name, regime)
    tag = "recon_quantiles %s %s" % (name, regime)
    srt = np.sort(curves, axis=0)
    v64, v32 = (np.moveaxis(v, 1, 0) for v in E.draws("recon_quantiles", name, regime))
    bar = QU.oracle_bar(v64)
    worst = worst32 = 0.0
    for key, levels in QU.LEVEL_SETS.items():
        got = _quantiles(eng, flat, c, post, levels, obs_d=obs_d, labels=labels)
        want = QU.select(srt, levels)
        assert got.dtype == want.dtype and np.array_equal(got, want), (tag, key, np.argwhere(got != want)[:5])
        lv = np.asarray(levels, dtype=np.float64)
        q64, q32 = np.quantile(v64, lv, axis=0, method="linear"), np.quantile(v32, lv, axis=0, method="linear")
        r32 = float((np.abs(q32 - q64) / bar).max())
        worst, worst32 = max(worst, float((np.abs(got - q64) / (bar * E.factor(r32))).max())), max(worst32, r32)
        if regime == "ties":
            assert _plus_zero(got[:, :, :, 0]), (tag, key)
    print("%s: bitwise the selection among the kernel's own curves at %d level sets; oracle check: error / bar %.3f (fp32 oracle / suite bar %.3f)"
          % (tag, len(QU.LEVEL_SETS), worst, worst32))
    assert worst <= 1.0


@pytest.mark.parametrize("ns", E.BAND_NS)
@pytest.mark.parametrize("name,regime", E.curve_entries("joint_band"))
def test_joint_band(name, regime, ns):
    """sd_floor = 0, K = 7 and 33.  Split: mean / sd are the bits of recon_moments; dev, crit, joint, obs_dev and the point counts equal
    the numpy restatement on the kernel's own curves EXACTLY (eval_gpu_util._band_check_exact).  Oracle: _band_check_oracle's bars --
    the recon_moments bars carried through the quotient, so they grow as 1 / sd: at sd / level = 5e-5 (challenge_gauss at `all`) a
    deviation's bar exceeds its range and only the exact check holds it, which is why it is there.  No level is asked to be clear of near
    draws (BU.CLEAR_LEVEL's share is a condition of the initialisation cases); instead every deviation obeys dev <= sqrt(K - 1) + 0.01
    (|v - m| carries at most 2 ulp of the level, 2^-23, against an sd of at least 4.8e-5 of it: 2.5e-3 of a unit).
    ties: channel 0 has no participating point: points 0, dev 0 in every draw, obs_dev 0 for observations of +0.0 and -0.0 alike, crit 0,
    joint 1 at every level (include/slode.h: "no point: 0")."""
    c, eng, flat, obs_d, labels, post, curves = _entry("joint_band", name, regime, ns)
    tag = "joint_band %s %s K=%d" % (name, regime, ns)
    levels = BU.COUNT_LEVELS + (0.95, BU.CLEAR_LEVEL[ns])
    r = _band(eng, flat, c, post, levels, obs_d=obs_d, labels=labels)
    mean, sd = (t.cpu().numpy() for t in _recon_moments(eng, flat, c, post, obs_d=obs_d, labels=labels))
    assert np.array_equal(r["mean"], mean) and np.array_equal(r["sd"], sd), tag
    _band_exact(r, curves, c["obs"].numpy(), levels, 0.0, tag)
    v64 = E.oracle_draws(c, post)
    wd, wc, wo, share = _band_oracle(r, v64, c["obs"].double().numpy(), levels, 0.0, tag)
    print("%s: exact on the kernel's own curves; oracle check: worst error / bar dev %.3e crit %.3e obs_dev %.3e; near share at the informative levels %.2e; "
          "largest dev %.4f (sqrt(K - 1) = %.4f), largest obs_dev %.3g" % (tag, wd, wc, wo, share, r["dev"].max(), np.sqrt(ns - 1.0), r["obs_dev"].max()))
    assert np.isfinite(r["dev"]).all() and np.isfinite(r["obs_dev"]).all() and r["dev"].max() <= np.sqrt(ns - 1.0) + 0.01
    live = r["points"] > 0
    assert np.all(r["joint"][live][:, 3] == 1.0)                                           # the clear level: z above sqrt(K - 1) + 0.01
    if regime == "ties":
        assert not r["points"][:, :, 0].any() and np.all(r["points"][:, :, 1:] == c["T"])
        assert _plus_zero(r["dev"][:, :, 0]) and _plus_zero(r["obs_dev"][:, :, 0]) and _plus_zero(r["crit"][:, :, 0]) and np.all(r["joint"][:, :, 0] == 1.0)
        assert _plus_zero(r["mean"][:, :, 0]) and _plus_zero(r["sd"][:, :, 0])
    else:
        assert live.all()


def _channels(regime):
    """The channels a near-point rule can be applied to: all of them, but not the constant channel 0 of `ties`."""
    return slice(1, None) if regime == "ties" else slice(None)


@pytest.mark.parametrize("name,regime", E.curve_entries("curve_summary"))
def test_curve_summary(name, regime):
    """Thresholds: E.summary_thresholds of the oracle's draws (a level of each channel's values that is not on a plateau).  Split: per draw (num_samples = 1) slots 0 - 3, 6, 7 and the counts equal
    SU.functionals of the kernel's own curve exactly, slots 4 and 5 within SU.sum_bars; the 7-draw call equals SU.draw_moments_f32 of those
    per-draw values BITWISE and p_beyond their sum over 7.  Oracle: SU.check_continuous and SU.check_counts (the near share a condition,
    tests/test_eval_regimes_cpu.py) on every channel but the constant one.
    ties, channel 0 (a curve that is +0.0 at every time in every draw, thr = 0 = its own value): peak = trough = +0.0 at t_peak = t_trough =
    t_0 (the smallest index wins ties), auc = 0, and with a strict comparison never beyond in either sense: time_beyond = crossed = 0,
    t_hit NaN, p_beyond 0; every sd 0 but t_hit's, NaN."""
    c, eng, flat, obs_d, labels, post, curves = _entry("curve_summary", name, regime)
    tag = "curve_summary %s %s" % (name, regime)
    times = c["times"].numpy()
    v64 = E.draws("curve_summary", name, regime)[0]
    thr, _ = E.summary_thresholds(v64, regime)
    vk, ch = np.moveaxis(v64, 1, 0), _channels(regime)
    eps = c["eps"].to(DEV)
    K = eps.shape[0]
    for sense in (1, -1):
        per = [_summary(eng, flat, c, post, thr, sense, eps=eps[k].contiguous(), ns=1, obs_d=obs_d, labels=labels) for k in range(K)]
        worst = 0.0
        for k, (m1, s1, p1) in enumerate(per):
            want = SU.functionals(curves[k], times, thr, sense)
            for slot in (0, 1, 2, 3, 6, 7):
                assert np.array_equal(m1[..., slot].astype(np.float64), want[..., slot], equal_nan=True), (tag, sense, k, SU.NAMES[slot])
            bar_auc, bar_tb = SU.sum_bars(curves[k], times)
            worst = max(worst, _ratio(m1[..., 4] - want[..., 4], bar_auc), _ratio(m1[..., 5] - want[..., 5], np.full(m1[..., 5].shape, bar_tb)))
            assert np.array_equal(p1, SU.beyond(curves[k], thr, sense).astype(np.float32)), (tag, sense, k)
            assert np.array_equal(np.isnan(s1), np.isnan(m1)) and np.all(s1[~np.isnan(s1)] == 0.0)
        assert worst <= 1.0, (tag, sense, worst)
        mean, sd, pb = _summary(eng, flat, c, post, thr, sense, obs_d=obs_d, labels=labels)
        wm, ws = SU.draw_moments_f32(np.stack([m[0] for m in per]))
        assert np.array_equal(mean, wm, equal_nan=True) and np.array_equal(sd, ws, equal_nan=True), (tag, sense)
        assert np.array_equal(pb, RU._f32(np.stack([m[2] for m in per]).sum(0)) / np.float32(K)), (tag, sense)
        t = "%s sense %d" % (tag, sense)
        om, osd = SU.oracle_moments(SU.functionals(vk[:, :, :, ch], times, thr[ch].astype(np.float64), sense))
        SU.check_continuous(mean[:, :, ch].astype(np.float64), sd[:, :, ch].astype(np.float64), om, osd, np.abs(v64[:, :, :, ch]).max(-1).max(1),
                            float(times[-1] - times[0]), t)
        SU.check_counts(pb[:, :, ch], K, vk[:, :, :, ch], thr[ch], sense, t)
        print("%s: per-draw functionals exact, sums / bar %.3f, moments over the draws bitwise" % (t, worst))
        if regime == "ties":
            assert thr[0] == 0.0
            m0, s0 = mean[:, :, 0], sd[:, :, 0]
            assert _plus_zero(m0[..., [0, 2, 4, 5, 7]]) and np.all(m0[..., [1, 3]] == times[0]) and np.isnan(m0[..., 6]).all()
            assert _plus_zero(s0[..., [0, 1, 2, 3, 4, 5, 7]]) and np.isnan(s0[..., 6]).all() and _plus_zero(pb[:, :, 0])


def _calibration_floats(got, y, v, tau, ids, G, tag):
    """pinball [3, G, C] and width [G, C] against the fp64 means of the exact summands of the kernel's own curves -- (y - v) w with the
    kernel's fp32 weights w = fl(tau) or fl(fl(tau) - 1), and v_1 - v_2 -- at KU.accumulation_bar: 5 u x the mean |summand| of the cell, no
    factor in the number of terms (tests/calibration_util.py)."""
    t32, tm32 = (x.astype(np.float64) for x in KU.tau32(tau))                              # the kernel's weights: fl(tau), fl(fl(tau) - 1)
    y64, v64 = y[None].astype(np.float64), v.astype(np.float64)
    sm = np.stack(np.broadcast_arrays(*([(y64 - v64[j]) * np.where(y64 < v64[j], tm32[j], t32[j]) for j in range(3)] + [v64[1] - v64[2]])))   # [4, K, B, C, T]
    worst = 0.0
    for g in range(G):
        sel = np.flatnonzero(np.asarray(ids) == g)
        if not sel.size:
            assert torch.isnan(got[3][:, g]).all() and torch.isnan(got[4][g]).all()
            continue
        want, mag = sm[:, :, sel].mean((1, 2, 4)), np.abs(sm[:, :, sel]).mean((1, 2, 4))   # [4, C]
        have = np.concatenate([got[3][:, g].double().cpu().numpy(), got[4][g].double().cpu().numpy()[None]])
        worst = max(worst, _ratio(have - want, KU.accumulation_bar(mag)))
    print("%s split check: pinball and width against the fp64 means of the own curves' summands: error / accumulation bar %.3f" % (tag, worst))
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("name,regime", E.curve_entries("calibration"))
def test_calibration(name, regime):
    """Cohorts E.COHORT_IDS (two members, one, none; one trajectory in no cohort), chunk 2.  Split: the counts by the comparison rule on
    the kernel's own curves (as test_gpu_calibration.test_counts_are_those_of_the_kernels_own_curves; cells that differ printed) and the
    float outputs at KU.accumulation_bar.  Oracle: KU.check.  Both rules excuse NEAR points under a cap, so at `ties` they run on channels
    1 .. and channel 0 -- every curve exactly +0.0 (Gauss: mean 0, the band +- 2 s), a third of its observations exact ties of either sign
    of zero -- is compared EXACTLY with KU.indicators on the same values: y < v is false at a tie whatever the sign of the zero, so a tie
    counts in no `below`, is `inside` only through v_2 <= y (Gauss), and three equal curves never cross."""
    c, eng, flat, obs_d, labels, post, _ = _entry("calibration", name, regime)
    tag = "calibration %s %s" % (name, regime)
    ids, G, K = np.array(E.COHORT_IDS), E.COHORT_G, c["eps"].shape[0]
    eps = c["eps"].to(DEV).contiguous()
    got = _calib(eng, flat, c, post, ids, G, chunk=E.COHORT_CHUNK, eps=eps, obs_d=obs_d, labels=labels)
    v = _own_curves(eng, flat, c, post, eps, obs_d, labels)                                # [3, K, B, C, T]
    y, tau, ch = c["obs"].numpy(), KU.nominal(c["ospec"]), _channels(regime)
    cut = lambda g: (g[0][:, :, ch], g[1][:, ch], g[2][:, ch], g[3][:, :, ch], g[4][:, ch])
    cells = KU.check(cut(got), KU.reduce_by_cohort(y[:, ch], v[:, :, :, ch], tau, ids, G), tag + " own curves", K)
    print("%s: cells that differ from the kernels' own curves: %s" % (tag, cells))
    _calibration_floats(got, y, v, tau, ids, G, tag)
    KU.check(cut(got), KU.reduce_by_cohort(c["obs"].double().numpy()[:, ch], KU.oracle_curves(c, post)[:, :, :, ch], tau, ids, G), tag + " oracle", K)
    assert int(got[0][:, 2].abs().max()) == 0 and torch.isnan(got[3][:, 2]).all() and torch.isnan(got[4][2]).all()        # the empty cohort
    if regime == "ties":
        assert _plus_zero(v[0][:, :, 0]) and int(((y[:, 0] == 0) & np.signbit(y[:, 0])).sum()) > 0 and int(((y[:, 0] == 0) & ~np.signbit(y[:, 0])).sum()) > 0
        want = KU.reduce_by_cohort(y[:, :1], v[:, :, :, :1], tau, ids, G)["counts"]       # [5, G, 1, T]
        have = [got[0][0], got[0][1], got[0][2], got[1], got[2]]
        for i, x in enumerate(have):
            assert np.array_equal(x[:, 0].cpu().numpy().astype(np.int64), want[i][:, 0]), (tag, KU.NAMES[i], "channel 0")
        tie = y[:, 0] == 0                                                                   # [B, T]: below0 counts no tie
        for g in range(G):
            sel = np.flatnonzero(ids == g)
            if sel.size:
                assert int(got[0][0][g, 0].cpu().numpy()[tie[sel].all(0)].sum()) == 0


def _arm_curves(eng, flat, c, post, obs_d, labels, mask):
    """[K, Q, B, C, T] fp32: the kernel's own curves of one arm -- recon_moments with num_samples = 1 on the rows where(block, e', e)."""
    sel = torch.from_numpy(AU.block_dims(c["ospec"], mask))
    rows = torch.where(sel, c["eps2"][1], c["eps2"][0])
    return _per_draw_curves(eng, flat, dict(c, eps=rows), post, obs_d, labels)


@pytest.mark.parametrize("name,regime", E.curve_entries("latent_attribution"))
def test_latent_attribution(name, regime):
    """Every arm of the family (AU.arm_masks).  Split: the base mean / sd as recon_moments' on the base rows; msd of every arm against
    1 / (2 ns) sum d^2 in fp64 of the kernel's own curves of both arms within (ns + 4) u msd (d = fl(v_a - v): u on d, 2 u on d^2; ns fma
    roundings of a running sum that never exceeds the final one; two products), printed: whether bitwise AU.msd_f32.  Oracle: AU.check.
    ties: channel 0 is +0.0 in every arm and every draw: mean +0.0, sd 0, msd exactly 0 for every arm (the model layer's index of a curve
    without variance is NaN: MechanisticBase.latent_attribution, tests/test_attribution_cpu.py)."""
    c, eng, flat, obs_d, labels, post, curves = _entry("latent_attribution", name, regime)
    tag = "latent_attribution %s %s" % (name, regime)
    masks, _, _ = AU.arm_masks(c["ospec"])
    ns = c["eps"].shape[0]
    mean, sd, msd = _attr(eng, flat, c, post, masks, obs_d=obs_d, labels=labels)
    _moments_against_own_curves(mean.cpu().numpy(), sd.cpu().numpy(), curves, tag)
    m = msd.cpu().numpy()
    worst, bitwise = 0.0, True
    for a, mask in enumerate(masks):
        arm = _arm_curves(eng, flat, c, post, obs_d, labels, mask)
        want = 0.5 * np.mean((arm.astype(np.float64) - curves.astype(np.float64)) ** 2, 0)
        worst = max(worst, _ratio(m[a] - want, (ns + 4) * U24 * want))
        bitwise = bitwise and np.array_equal(m[a], AU.msd_f32(curves, arm))
    print("%s split check: msd error / bar %.3f over %d arms (bitwise the restatement: %s; largest msd %.3g)" % (tag, worst, len(masks), bitwise, m.max()))
    assert worst <= 1.0, (tag, worst)
    AU.check((mean, sd, msd), AU.oracle_moments(c, post, masks), tag + " oracle check")
    if regime == "ties":
        assert _plus_zero(mean[:, :, 0].cpu().numpy()) and _plus_zero(sd[:, :, 0].cpu().numpy()) and _plus_zero(m[:, :, :, 0])
        assert float(m[:, :, :, 1:].max()) > 0.0


@pytest.mark.parametrize("name,regime", E.curve_entries("mechanism_moments"))
def test_mechanism_moments(name, regime):
    """MU.build's conditioned case under the regime.  All five slots where the oracle's smallest degradation stays at least MU.MIN_D (the
    condition of the set point's bar), else the bounded four.  Split: the 7-draw call equals RU.shifted_moments_f32 of seven one-draw calls
    BITWISE.  Oracle: MU.BARS under the bar rule (MU.oracle_draws in fp32).  The states are not head curves: `ties` has no constant row
    here; it feeds the encoder observations of +-0.0."""
    c, eng, flat, obs_d, labels, post, _ = _entry("mechanism_moments", name, regime, curves=False)
    tag = "mechanism_moments %s %s" % (name, regime)
    d64, d32 = MU.oracle_draws(c, post), MU.oracle_draws(c, post, dtype=torch.float32)
    slots = MU.ALL if MU.min_degradation(d64) >= MU.MIN_D else BOUNDED
    sel = [q for q in range(MU.SLOTS) if (slots >> q) & 1]
    eps = c["eps"].to(DEV)
    per = np.stack([_mech(eng, flat, c, post, slots, eps=eps[k].contiguous(), ns=1, sd=False, obs_d=obs_d, labels=labels)[0] for k in range(eps.shape[0])])
    mean, sd = _mech(eng, flat, c, post, slots, obs_d=obs_d, labels=labels)
    with np.errstate(all="ignore"):
        wm, ws = RU.shifted_moments_f32(per)
    assert np.array_equal(mean, wm, equal_nan=True) and np.array_equal(sd, ws, equal_nan=True), tag
    (m64, s64), (m32, s32) = MU.moments(d64), MU.moments(d32.astype(np.float64))
    line, worst = [], 0.0
    for j, q in enumerate(sel):
        scale = np.maximum(1.0, np.abs(m64[q]))
        mb, sb = MU.BARS[MU.NAMES[q]]
        rm32, rs32 = float((np.abs(m32[q] - m64[q]) / (mb * scale)).max()), float((np.abs(s32[q] - s64[q]) / (sb * scale)).max())
        rm, rs = float((np.abs(mean[j] - m64[q]) / (mb * scale * E.factor(rm32))).max()), float((np.abs(sd[j] - s64[q]) / (sb * scale * E.factor(rs32))).max())
        line.append("%s %.3f %.3f (fp32 %.3f %.3f)" % (MU.NAMES[q], rm, rs, rm32, rs32))
        worst = max(worst, rm, rs)
    print("%s: moments over the draws bitwise; oracle check, error / bar (mean, sd) per slot: %s; smallest d %.1e" % (tag, "; ".join(line), MU.min_degradation(d64)))
    assert np.isfinite(mean).all() and np.isfinite(sd).all() and worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("name,regime", E.curve_entries("intervene_moments"))
def test_intervene_moments(name, regime):
    """The family's last mask (all groups; proc: the pair {C12, C6} swapped), labels rolled by one row.  Split: the counterfactual moments
    against the fp64 moments of the kernel's own counterfactual curves (one-draw calls: cf_mean = the draw) and the effect's against those
    of e_k = fl(v_cf,k - v_f,k), both at RU.accumulation_bars; printed: whether bitwise IU.paired_moments_f32.  Oracle: IU.check.
    ties: channel 0 is +0.0 in both arms: all four outputs exactly +0.0 / 0 there."""
    c, eng, flat, obs_d, labels, post, vf = _entry("intervene_moments", name, regime)
    tag = "intervene_moments %s %s" % (name, regime)
    _, mask, cols = IU.MASKS[c["fam"]][-1]
    u_cf = IU.cf_labels(c["u"], cols)
    eps = c["eps"].to(DEV)
    vcf = np.stack([_iv(eng, flat, c, mask, u_cf, eps=eps[k].contiguous(), obs_d=obs_d, labels=labels, ns=1)[0].cpu().numpy() for k in range(eps.shape[0])])
    got = _iv(eng, flat, c, mask, u_cf, obs_d=obs_d, labels=labels)
    cm, cs, em, es = (t.cpu().numpy() for t in got)
    _moments_against_own_curves(cm, cs, vcf, tag + " cf")
    _moments_against_own_curves(em, es, (vcf - vf).astype(np.float32), tag + " effect")
    print("%s: bitwise the restatement: %s" % (tag, [np.array_equal(x, y) for x, y in zip((cm, cs, em, es), IU.paired_moments_f32(vf, vcf))]))
    IU.check(got, IU.oracle_moments(c, mask, u_cf), tag + " oracle check")
    if regime == "ties":
        assert all(_plus_zero(x[:, :, 0]) for x in (cm, cs, em, es)) and float(np.abs(em[:, :, 1:]).max()) > 0.0


@pytest.mark.parametrize("name,regime", E.curve_entries("cohort_moments"))
def test_cohort_moments(name, regime):
    """Cohorts E.COHORT_IDS, chunk 2.  Split: mean, sd, sd_subjects against the fp64 moments by cohort of the kernel's own per-draw values
    (one-draw calls on singleton cohorts) at CU.accumulation_bars, an sd that is exactly 0 in fp64 exactly 0 here; obs_mean and l1 through
    CU.check's own bars.  Oracle: CU.check.  raw_units: the L1 runs on observations of 12 y - 4.
    ties: channel 0: mean +0.0, both sds 0, and l1 the sum over t of |mean observation|, whose ties enter as +0.0 or -0.0."""
    c, eng, flat, obs_d, labels, post, _ = _entry("cohort_moments", name, regime, curves=False)
    tag = "cohort_moments %s %s" % (name, regime)
    ids, G, R, K = np.array(E.COHORT_IDS), E.COHORT_G, E.COHORT_CHUNK, c["eps"].shape[0]
    eps = c["eps"].to(DEV).contiguous()
    vals = _cohort_per_draw(eng, flat, c, post, eps, obs_d, labels)                        # [B, K, Q, C, T]
    got = _cohort(eng, flat, c, post, ids, G, chunk=R, eps=eps, obs_d=obs_d, labels=labels)
    mean, sd, sdb = (x.cpu().numpy() for x in got[:3])
    wm, ws, wb, D = _cohort_truth(vals, ids, G, R)
    bm, bs, bb = CU.accumulation_bars(wm, ws, wb, D, R, K)
    live = ~np.isnan(wm)
    assert np.isnan(mean[~live]).all() and np.all(D[live & (ws > 0)] <= CU.SPREAD * ws[live & (ws > 0)])
    ratios = []
    for x, w, b in ((mean, wm, bm), (sd, ws, bs), (sdb, wb, bb)):
        ok = live & (w != 0) if x is not mean else live
        assert not x[live & ~ok].any()                                                      # an sd of exactly 0 in fp64: exactly 0
        ratios.append(_ratio((x - w)[ok], np.where(np.isfinite(b), b, 0.0)[ok]))
    print("%s split check: error / accumulation bar: mean %.3f, sd %.3f, sd_subjects %.3f" % ((tag,) + tuple(ratios)))
    assert max(ratios) <= 1.0, (tag, ratios)
    CU.check(got, CU.oracle_cohorts(c, post, ids, G), c["obs"], R, tag + " oracle check")
    if regime == "ties":
        for g in (0, 1):
            assert _plus_zero(mean[:, g, 0]) and _plus_zero(sd[:, g, 0]) and _plus_zero(sdb[:, g, 0])
            om = got[3][g, 0].double().cpu().numpy()
            assert abs(float(got[4][g, 0]) - np.abs(om).sum()) <= c["T"] * U24 * np.abs(om).sum()


@pytest.mark.parametrize("name,regime", E.curve_entries("forecast_moments"))
def test_forecast_moments(name, regime):
    """FU.build's grid (the case's own and nine more steps), the default window, heads and states.  Split: heads and states against the fp64
    moments of the kernel's own per-draw values (one-draw calls) at RU.accumulation_bars.  Oracle: RU.check's bars under the bar rule
    (FU.oracle_moments in fp32).  ties: the head curves of channel 0 stay +0.0 beyond the window as inside it."""
    c, eng, flat, obs_d, labels, post, _ = _entry("forecast_moments", name, regime, curves=False)
    tag = "forecast_moments %s %s" % (name, regime)
    eps = c["eps"].to(DEV)
    per = [_forecast(eng, flat, c, post, eps=eps[k].contiguous(), ns=1, sd=False, x_sd=False, obs_d=obs_d, labels=labels) for k in range(eps.shape[0])]
    got = [t.cpu().numpy() for t in _forecast(eng, flat, c, post, obs_d=obs_d, labels=labels)]
    _moments_against_own_curves(got[0], got[1], np.stack([p[0].cpu().numpy() for p in per]), tag + " heads")
    _moments_against_own_curves(got[2], got[3], np.stack([p[2].cpu().numpy() for p in per]), tag + " states")
    w64, w32 = FU.oracle_moments(c, post), FU.oracle_moments(c, post, dtype=torch.float32)
    line, worst = [], 0.0
    for i, what in ((0, "heads"), (2, "states")):
        scale = np.maximum(1.0, np.abs(w64[i]))
        r32m, r32s = float((np.abs(w32[i] - w64[i]) / (RU.MEAN_BAR * scale)).max()), float((np.abs(w32[i + 1] - w64[i + 1]) / (RU.SD_BAR * scale)).max())
        rm = float((np.abs(got[i] - w64[i]) / (RU.MEAN_BAR * scale * E.factor(r32m))).max())
        rs = float((np.abs(got[i + 1] - w64[i + 1]) / (RU.SD_BAR * scale * E.factor(r32s))).max())
        line.append("%s mean %.3f sd %.3f (fp32 oracle / suite bar %.3f, %.3f)" % (what, rm, rs, r32m, r32s))
        worst = max(worst, rm, rs)
    print("%s oracle check: error / bar: %s" % (tag, "; ".join(line)))
    assert all(np.isfinite(g).all() for g in got) and worst <= 1.0, (tag, worst)
    if regime == "ties":
        assert _plus_zero(got[0][:, :, 0]) and _plus_zero(got[1][:, :, 0])
