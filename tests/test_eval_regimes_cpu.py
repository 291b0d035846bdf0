"""The entries of tests/eval_regime_util.py do what tests/test_gpu_eval_regimes.py relies on, on the oracles alone: every entry is finite in
fp64 and fp32, keeps the conditions of its exclusions, reaches the branches it is there for, and leaves the fp32 CPU oracle within a
quarter of every bar the GPU tests hold the kernels to.  One line per entry: the tables of eval_regime_util's docstring and of DESIGN.md; a
change of a seed or of a library that moves them fails here, before it takes a GPU test off a branch.  No GPU."""
import numpy as np
import pytest
import torch

from tests import eval_regime_util as E
from tests import pointwise_util as PU
from tests import regime_util as G
from tests import traj_bounds_util as TU


# ---- pointwise_loo -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,regime,K", E.LOO_ENTRIES)
def test_loo_entries(name, regime, K):
    """The recorded seed is the first from 21 up that meets both conditions (crossing exclusion within PU.CAP, clear_of_kinks within
    KINK_SHARE of the observations).  Every Gauss entry at tight_noise and all has at least 10 % of its points on the log DBL_MIN clamp and
    at least 10 % at khat = +inf through n_tail < 5; every entry at least 25 % of its points at khat > 1.  The oracle-level bars are not
    raised (the fp32 oracle sits within 3 % of them); the share of the points whose khat is not compared at the oracle level is printed
    and stays under a third."""
    seed = E.LOO_SEEDS.get((name, regime), E.SEED_FROM)
    assert E.find_seed(lambda s: E.loo_build(name, regime, K, s), E.loo_ok) == seed
    c = E.loo_case(name, regime, K)
    o = E.Loo(c)
    assert np.isfinite(o.want["ell"]).all() and np.isfinite(o.e).all() and np.isfinite(o.eb).all()
    r = E.loo_reach(o.want["ell"])
    out = 1.0 - o.khat_level.mean()
    print("loo %-16s %-12s K=%d seed %d moved %d: %s; fp32 oracle / bar: elpd_loo %.3f, lppd %.3f; khat left out at the oracle level %.3f; "
          "elpd bar median %.1e, largest %.1e at |elpd| up to %.1e"
          % (name, regime, K, seed, c["moved"], r, o.r32[0], o.r32[1], out, np.median(o.eb), o.eb.max(), np.abs(o.e).max()))
    n = r["points"]
    if E.gauss(name) and regime in ("tight_noise", "all"):
        assert r["clamp"] >= 0.10 * n and r["inf_short"] >= 0.10 * n and r["short"] >= r["inf_short"]
    assert r["k1"] >= 0.25 * n and r["k07"] >= r["k1"]
    assert max(o.r32) <= 0.25 and out <= 1.0 / 3.0
    assert np.array_equal(np.isinf(o.k32), np.isinf(o.k))


# ---- pointwise_density -------------------------------------------------------------------------------------------------------------------------
# (entry) -> ceiling of the bar factor, about 3 x the largest measured (the table of tests/eval_regime_util.py): every other bar is the suite's
DENSITY_RAISED = {("cvs_ald", "all"): 6.0, ("challenge_gauss", "all"): 12.0}


@pytest.mark.parametrize("name,regime", E.DENSITY_ENTRIES)
def test_density_entries(name, regime):
    c = E.density_case(name, regime)
    assert E.density_ok(c)
    d = E.Density(c, "%s %s" % (name, regime))
    K, B = c["eps"].shape[:2]
    r32 = d.fold(PU.log_weights(K, B))[4]
    f = [E.factor(r) for r in r32]
    print("density %-16s %-12s moved %d: fp32 oracle / suite bar: lppd %.3f, mean_ll %.3f, var_ll %.3f, slots %.3f -> bar factors %s; largest |l| %.3g"
          % (name, regime, c["moved"], r32[0], r32[1], r32[2], r32[3], ["%.2f" % x for x in f], np.abs(d.want["ell"]).max()))
    assert np.isfinite(d.want["ell"]).all() and np.isfinite(d.w32["ell"]).all()
    # (one-sided: the fp32 oracle's distance moves by a factor of two between BLAS builds, so an entry of the table may also come out unraised)
    assert max(f) <= DENSITY_RAISED.get((name, regime), 1.0), "the table of tests/eval_regime_util.py moved"


@pytest.mark.parametrize("name", E.CASES)
def test_density_importance_entries(name):
    """tight_noise with the noise scaled: the weights of the fp64 oracle's losses are not one-hot and not uniform."""
    c = E.density_case(name, "tight_noise", importance=True)
    assert E.density_ok(c)
    want, r32 = G.bounds_oracles(c)
    ess = TU.reduce64(want["loss"])[2]
    print("density %-16s tight_noise noise x %g: ESS of the oracle's weights %s; fp32 oracle / per-row bar %.2f" % (name, E.IMPORTANCE_NOISE[name], np.round(ess, 2), r32))
    assert E.spread_weights(ess) and r32 <= 0.5
    one_hot = E.density_case(name, "tight_noise")
    assert not E.spread_weights(TU.reduce64(TU.oracle_rows(one_hot)["loss"])[2])          # at the noise as drawn the weights are one-hot


# ---- posterior_refine --------------------------------------------------------------------------------------------------------------------------
REFINE_RAISED = {("challenge_gauss", "all"): 8.0}          # ceiling of the factor on the bar of F, as DENSITY_RAISED; no gradient bar is raised


@pytest.mark.parametrize("name,regime", E.REFINE_ENTRIES)
def test_refine_entries(name, regime):
    """The fp32 oracle of F and of dF / d(loc, log scale) at the encoder's posterior against the fp64 oracle, in units of RFU's bars."""
    c = E.refine_case(name, regime)
    assert E.kinks_ok(c)
    o = E.refine_oracles(c)
    print("refine %-16s %-12s moved %d: fp32 oracle / suite bar: F %.3f, grad0 %.3f -> F bar x %.2f, grad0 bar %.1e; |F| up to %.3g"
          % (name, regime, c["moved"], o["r32"][0], o["r32"][1], float((o["f_bar"] / (E.RFU.REL * o["mag"])).max()), o["g_bar"], np.abs(o["F"]).max()))
    assert np.isfinite(o["F"]).all() and np.isfinite(o["grad"]).all()
    assert E.factor(o["r32"][0]) <= REFINE_RAISED.get((name, regime), 1.0) and o["g_bar"] == E.RFU.GRAD_REL, "the table of tests/eval_regime_util.py moved"


# ---- the whole-curve calls ---------------------------------------------------------------------------------------------------------------------
def _channels(regime):
    return slice(1, None) if regime == "ties" else slice(None)


@pytest.mark.parametrize("regime", ["ties", "all", "prior_scales", "raw_units"])
@pytest.mark.parametrize("name", E.CASES)
def test_curve_entries(name, regime):
    """The head curves of every (case, regime) the whole-curve entries use (RU.build at B = 4, 7 draws; the band's 33): clear_of_kinks within
    KINK_SHARE, finite in both precisions, the fp32 oracle's mean / sd within a quarter of RU.MEAN_BAR / RU.SD_BAR (no bar is raised), and
    what they reach.  ties: channel 0 is exactly +0.0 in every draw in fp64 AND in fp32 -- a whole channel, a third (ALD) or a quarter
    (challenge) of the elements, at sd exactly 0 -- against observations of both signs of zero."""
    for ns in E.BAND_NS:
        c = E.curve_case("joint_band", name, regime, ns)
        assert E.kinks_ok(c), (ns, c["moved"])
    c = E.curve_case("recon_moments", name, regime)
    v64, v32 = E.draws("recon_moments", name, regime)
    m, s, bm, bs, r32 = E.moment_bars(v64, v32)
    r = E.curve_reach(v64, v32)
    print("curves %-16s %-12s (%s draws) moved %d: level %.1f, smallest sd / level %.1e, zero-sd elements %d (fp64) %d (fp32) of %d; fp32 oracle / suite bar: mean %.3f, sd %.3f"
          % (name, regime, "posterior" if E.is_post(regime) else "prior", c["moved"], r["level"], r["sd_over_level"], r["zero_sd"][0], r["zero_sd"][1], r["elements"], r32[0], r32[1]))
    assert np.isfinite(v64).all() and np.isfinite(v32).all() and max(r32) <= 0.25
    Q, _, B, C, T = v64.shape
    if regime == "ties":
        assert E.constant_channel(v64) and E.constant_channel(v32) and r["zero_sd"] == (Q * B * T, Q * B * T)
        y0 = c["obs"][:, 0].numpy()
        assert ((y0 == 0) & np.signbit(y0)).sum() > 0 and ((y0 == 0) & ~np.signbit(y0)).sum() > 0
    else:
        assert r["zero_sd"] == (0, 0)


@pytest.mark.parametrize("name,regime", E.curve_entries("curve_summary"))
def test_curve_summary_conditions(name, regime):
    """The near share of SU.check_counts (a condition of the count rule) at E.summary_thresholds on the channels the rule runs on; ties: the
    threshold of the constant channel is its own value, 0, so every point of it is near -- that channel is compared exactly instead."""
    from tests import summary_util as SU
    v64 = E.draws("curve_summary", name, regime)[0]
    thr, took = E.summary_thresholds(v64, regime)
    ch = _channels(regime)
    share = float(SU.near(np.moveaxis(v64, 1, 0)[:, :, :, ch], thr[ch]).mean())
    print("curve_summary %-16s %-12s thr %s (levels %s) near share %.2e; at the medians %.2e"
          % (name, regime, thr, took, share, float(SU.near(np.moveaxis(v64, 1, 0)[:, :, :, ch], SU.thresholds(v64)[ch]).mean())))
    lo, hi = v64[0].min((0, 1, 3)), v64[0].max((0, 1, 3))
    assert np.all((thr >= lo) & (thr <= hi))                                              # inside the range of the channel's curves
    assert share <= SU.NEAR_SHARE
    if regime == "ties":
        assert thr[0] == 0.0 and bool(SU.near(np.moveaxis(v64, 1, 0)[:, :, :, :1], thr[:1]).all())


@pytest.mark.parametrize("name,regime", E.curve_entries("calibration"))
def test_calibration_conditions(name, regime):
    """KU.check's cap on the near (point, indicator) pairs, on the oracle, on the channels the rule runs on."""
    from tests import calibration_util as KU
    c = E.curve_case("calibration", name, regime)
    ch = _channels(regime)
    want = KU.reduce_by_cohort(c["obs"].double().numpy()[:, ch], KU.oracle_curves(c, E.is_post(regime))[:, :, :, ch], KU.nominal(c["ospec"]), np.array(E.COHORT_IDS), E.COHORT_G)
    frac = want["counts"][0].sum((1, 2)) / np.maximum(want["count"] * 7 * want["counts"].shape[2] * want["counts"].shape[3], 1)
    print("calibration %-16s %-12s near share %.2e (per indicator %s); head-0 fraction below per cohort %s" % (name, regime, want["near_total"], want["near_share"], np.round(frac, 3)))
    assert want["near_total"] <= KU.NEAR_SHARE


@pytest.mark.parametrize("name,regime", E.curve_entries("mechanism_moments"))
def test_mechanism_entries(name, regime):
    """MU.build's conditioned case under the regime: finite in both precisions; which slots are compared (all five where the oracle's smallest
    degradation is at least MU.MIN_D) and the fp32 oracle's distance per slot in units of MU.BARS."""
    from tests import mechanism_util as MU
    c = E.curve_case("mechanism_moments", name, regime)
    d64, d32 = MU.oracle_draws(c, True), MU.oracle_draws(c, True, dtype=torch.float32).astype(np.float64)
    five = MU.min_degradation(d64) >= MU.MIN_D
    (m64, s64), (m32, s32) = MU.moments(d64), MU.moments(d32)
    row = []
    for q in ([0, 1, 2, 3, 4] if five else [0, 1, 2, 4]):
        scale = np.maximum(1.0, np.abs(m64[q]))
        mb, sb = MU.BARS[MU.NAMES[q]]
        row.append((MU.NAMES[q], float((np.abs(m32[q] - m64[q]) / (mb * scale)).max()), float((np.abs(s32[q] - s64[q]) / (sb * scale)).max())))
        assert np.isfinite(m64[q]).all() and np.isfinite(m32[q]).all()
    print("mechanism %-16s %-12s smallest d %.1e (%s slots); fp32 oracle / suite bar (mean, sd): %s" % (name, regime, MU.min_degradation(d64), "five" if five else "the bounded four",
                                                                                                    "; ".join("%s %.3f %.3f" % r for r in row)))
    assert E.kinks_ok(c)


@pytest.mark.parametrize("name,regime", E.curve_entries("forecast_moments"))
def test_forecast_entries(name, regime):
    from tests import forecast_util as FU, recon_moments_util as RU
    c = E.curve_case("forecast_moments", name, regime)
    w64, w32 = FU.oracle_moments(c, True), FU.oracle_moments(c, True, dtype=torch.float32)
    row = []
    for i in (0, 2):
        scale = np.maximum(1.0, np.abs(w64[i]))
        row += [float((np.abs(w32[i] - w64[i]) / (RU.MEAN_BAR * scale)).max()), float((np.abs(w32[i + 1] - w64[i + 1]) / (RU.SD_BAR * scale)).max())]
    print("forecast %-16s %-12s T_out %d: fp32 oracle / suite bar: heads mean %.3f sd %.3f, states mean %.3f sd %.3f; largest |state| %.1f"
          % ((name, regime, c["T_out"]) + tuple(row) + (float(np.abs(w64[2]).max()),)))
    assert all(np.isfinite(w).all() for w in w64 + w32) and E.kinks_ok(c)
