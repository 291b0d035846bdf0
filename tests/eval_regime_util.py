"""Test infrastructure of tests/test_eval_regimes_cpu.py and tests/test_gpu_eval_regimes.py: the eval-side calls under the regimes of
tests/regime_util.py -- the table of (call, case, regime, seed) the GPU file runs, the cases themselves (regime_util.apply on each call's
own small build), what an entry reaches (the branches of the STATISTIC: tests/test_gpu_regimes.py holds the forward), and the bar rule of
regime_util.bar applied to the calls' oracles.  Not imported by the product.

Cases: cvs_ald, challenge_gauss, proc_ald (the S = 8 instantiation).  Scored-draw calls (pointwise_density, pointwise_loo, posterior_refine;
the last does not take proc): tight_noise and all, fitted for the Gauss case only -- residuals of the order of a scale put too many ALD points
on a crossing to keep pointwise_util.CAP -- and not ties: the sum over the three heads cannot tell the tie conventions apart
(tests/test_gpu_regimes.py).  Whole-curve calls: CURVE_CALLS below.  No entry had to be dropped.

Bars: each call's own util sets them, unchanged; where the util's oracle takes a dtype the bar is that, or 4 x the fp32 CPU oracle's distance
from fp64 on that case and that quantity where that is larger (`factor`), computed in the test, never from a kernel's output.  Measured on
the oracles (tests/test_eval_regimes_cpu.py prints these rows and asserts what is said here); fp32 oracle's distance / suite bar, "x": raised.
The figures move by a factor of two between BLAS builds and thread counts (cvs_ald density at `all`: 0.45 here, 1.05 on another host): the
rule follows them, the ceilings of the CPU test leave a factor of three.
  pointwise_density, K = 8, B = 4 (lppd | mean_ll | var_ll | slots)              pointwise_loo, K = 64, B = 3, T = 14 / 20 (elpd_loo | lppd)
    cvs_ald          tight_noise  0.05 0.02 0.02 0.00                             0.004 0.007   seed 26  khat left out at the oracle level 0.100
    cvs_ald          all          0.25 0.45 0.27 0.02   x 1.0 1.8 1.1 (1)         0.006 0.021   seed 21  0.139
    challenge_gauss  tight_noise  0.05 0.05 0.03 0.00                             0.005 0.007   seed 21  0.214
    challenge_gauss  all          0.49 1.03 0.51 0.19   x 2.0 4.1 2.0 (2)         0.007 0.010   seed 21  0.185   (K = 21: 0.008 0.020, 0.173)
    challenge_gauss  fitted       0.03 0.05 0.03 0.02                             0.005 0.006   seed 21  0.226
    proc_ald         tight_noise  0.01 0.01 0.01 0.00                             0.003 0.006   seed 25  0.104
    proc_ald         all          0.07 0.08 0.04 0.01                             0.004 0.011   seed 21  0.100
  (1), (2): l = sum of terms of size |r| / scale against |l| up to 1e4 (1) and 9e6 (2): at posterior scales over four decades and tripled
  weights one fp32 ulp of a curve that reaches 145 is 1e-5, a hundredth of the smallest likelihood scale, and r = y - mu cancels.
  posterior_refine, K = 3, B = 4 (F | grad0): at most 0.13 | 0.06, except challenge_gauss at `all`: F 0.67, bar x 2.7 (the same cancellation,
  summed over 1200 points per trajectory: |F| reaches 1.8e8).  No gradient bar is raised.
  No LOO bar is raised: LU.bars is the restatement's own sensitivity to the per-term bars, which scales with the regime by itself (elpd bar:
  median 2e-4 .. 5e-2 nat, largest 0.12 .. 130 nat at |elpd| up to 2e6).  LU.left_out's 2 % cap on the points whose oracle-level khat bar
  exceeds 0.05 cannot hold here -- the share is 0.10 .. 0.23 in every entry, for every seed: khat is that sensitive to a 1e-5 relative
  change of a curve once khat > 1 -- so the oracle check compares khat where its bar is <= 0.05 and prints the share; the split check
  (the restatement on the kernel's OWN per-draw values) holds khat at every point.
What the LOO entries reach (`loo_reach` on the fp64 oracle's l; points | cutoff on the log DBL_MIN clamp | n_tail < M | khat = +inf, all of
them through n_tail < 5 | khat > 0.7 | khat > 1 | largest draw spread in nat):
    cvs_ald          tight_noise  180   0   0   0   95   80  2.0e2         challenge_gauss  all, K = 64   168  68  68  64  134  133  7.2e5
    cvs_ald          all          180   0   0   0   73   67  3.4e2         challenge_gauss  all, K = 21   168  66  65  65  140  135  6.2e5
    challenge_gauss  tight_noise  168  37  37  29  103   97  4.4e4         proc_ald         tight_noise   240   0   0   0   90   68  2.2e2
    challenge_gauss  fitted       168  18  17  12   94   82  5.3e3         proc_ald         all           240   0   0   0  113   93  6.8e2
  At the initialisation no point has a draw spread near 708 nat, n_tail < M needs duplicated noise rows and khat = +inf needs K <= 20.
Importance mode of pointwise_density at tight_noise: at the noise as drawn, and at the suite's 1e-3 (PU.SPREAD), every weight is 0 or 1;
IMPORTANCE_NOISE scales it until the oracle's weights have 1.5 < ESS < 7.5 on at least half the trajectories (ESS per trajectory: cvs_ald
1.0 1.9 2.0 1.9, challenge_gauss 4.0 3.5 1.4 1.4, proc_ald 1.4 1.8 3.4 3.6).
Whole-curve entries (`curve_reach`; B = 4, 7 draws; level | smallest sd / level | elements with sd exactly 0, the same in fp64 and fp32 |
fp32 oracle / RU.MEAN_BAR, RU.SD_BAR -- no bar is raised):
    cvs_ald          ties 118.6 1.3e-2 2400 of 7200 0.01 0.01 | all 145.0 6.2e-3 0 0.15 0.13 | prior_scales 110.6 4.5e-2 0 0.14 0.07 | raw_units 118.6 1.3e-2 0 0.05 0.02
    challenge_gauss  ties   4.4 2.1e-2 1200 of 4800 0.02 0.01 | all   2.9 4.8e-5 0 0.20 0.09 | prior_scales  15.9 6.0e-2 0 0.04 0.02 | raw_units   4.7 1.1e-2 0 0.03 0.01
    proc_ald         ties   6.3 1.2e-2 1200 of 4800 0.00 0.00 | all  11.6 2.9e-2 0 0.09 0.02 | prior_scales   9.8 4.4e-2 0 0.01 0.01 | raw_units   6.9 8.0e-3 0 0.01 0.00
  ties: channel 0 is exactly +0.0 in every draw, in both precisions, against observations of +0.0 and -0.0.  The rules that excuse NEAR
  points under a cap (calibration, curve_summary: every point of a constant curve at its own value is near) run on the other channels and
  channel 0 is compared exactly.  mechanism_moments (MU.build's conditioned grid): all five slots at ties (smallest d 1.9e-2 .. 0.14), the
  bounded four at `all` (d down to 4e-33: the set point's bar has no meaning there); fp32 oracle / MU.BARS at most 0.10.  forecast_moments:
  at most 0.22."""
import numpy as np
import torch

from tests import loo_util as LU
from tests import pointwise_util as PU
from tests import refine_util as RFU
from tests import regime_util as G

CASES = ("cvs_ald", "challenge_gauss", "proc_ald")
SEED_FROM, SEED_TO = 21, 60


def gauss(name):
    return name.endswith("gauss")


def scored_regimes(name):
    """tight_noise and all; fitted for a Gauss family only (residuals of the order of a scale put too many ALD points on a crossing)."""
    return ("tight_noise", "all") + (("fitted",) if gauss(name) else ())


def apply(regime, c):
    """regime_util.apply with ``moved`` counted once per ELEMENT: with K draws clear_of_kinks runs K passes over three heads and
    regime_util sums the passes; the share that has to stay under KINK_SHARE is that of the observations that end up somewhere else."""
    out = G.apply(regime, c)
    _, obs = G.REGIMES[regime](c["ospec"], c["p"], c["obs"], c["u"], c["eps"], c["times"])
    moved = out["obs"] != obs
    if regime == "ties":
        moved = moved[:, 1:]
    return dict(out, moved=int(moved.sum()))


def kinks_ok(c):
    return c["moved"] <= G.KINK_SHARE * c["obs"].numel()


# ---- pointwise_loo ---------------------------------------------------------------------------------------------------------------------------
LOO_B = 3


def loo_T(name):
    return 14 if gauss(name) else 20


def loo_build(name, regime, K, seed):
    return apply(regime, LU.build(name, loo_T(name), LOO_B, K, seed=seed))


# The noise seed per (case, regime) where the suite's default, 21, does not meet both conditions: the first seed from 21 up (searched to
# 60) at which the ALD crossing exclusion keeps PU.CAP and the observations clear_of_kinks moves stay within KINK_SHARE (`loo_ok`), found on
# the fp64 oracle alone, as LU.ORACLE_SEEDS; tests/test_eval_regimes_cpu.py repeats the search.  No (case, regime) had to be dropped.
LOO_SEEDS = {("cvs_ald", "tight_noise"): 26, ("proc_ald", "tight_noise"): 25}
LOO_ENTRIES = [(name, regime, 64) for name in CASES for regime in scored_regimes(name)] + [("challenge_gauss", "all", 21)]


def loo_case(name, regime, K):
    return loo_build(name, regime, K, LOO_SEEDS.get((name, regime), SEED_FROM))


def crossing_ok(want):
    """The ALD crossing exclusion keeps PU.CAP, for the (draw, point) pairs and for the points (PU.conditions without the trajectories)."""
    return want["excl"].mean() <= PU.CAP and want["excl"].any(0).mean() <= PU.CAP


def find_seed(build, ok):
    """The first seed from SEED_FROM to SEED_TO at which ``ok(build(seed))``, or None."""
    for seed in range(SEED_FROM, SEED_TO + 1):
        if ok(build(seed)):
            return seed
    return None


def loo_ok(c):
    return kinks_ok(c) and crossing_ok(PU.oracle_points(c))


def loo_reach(l):
    """What the K per-draw log-densities l [K, ...] of an entry reach in the restatement: dict(points, clamp (points whose cutoff is the
    log DBL_MIN clamp), short (n_tail < M), inf (khat = +inf), inf_short (khat = +inf through n_tail < 5), k07, k1 (khat > 0.7, > 1,
    +inf included), spread (largest max_k l - min_k l))."""
    l = np.asarray(l, np.float64)
    K = l.shape[0]
    M = LU.tail_len(K)
    flat = np.sort(l.reshape(K, -1), 0)
    a_M = flat[0] - flat[M]
    fit = [LU.psis_point(flat[:, i]) for i in range(flat.shape[1])]
    khat, n = np.array([f[1] for f in fit]), np.array([f[2] for f in fit])
    return dict(points=flat.shape[1], clamp=int((a_M < LU.LOG_DBL_MIN).sum()), short=int((n < M).sum()), inf=int(np.isinf(khat).sum()),
                inf_short=int((np.isinf(khat) & (n < 5)).sum()), k07=int((khat > 0.7).sum()), k1=int((khat > 1.0).sum()),
                spread=float((flat[-1] - flat[0]).max()))


# ---- pointwise_density -----------------------------------------------------------------------------------------------------------------------
DENSITY_B, DENSITY_K = 4, 8


def density_build(name, regime, seed, noise=1.0):
    c = PU.build(name, "rk4", DENSITY_B, DENSITY_K, seed)
    c["eps"] = noise * c["eps"]
    return apply(regime, c)


# importance mode, tight_noise: the factor on the noise at which the weights of the fp64 oracle's losses are not one-hot (effective sample
# size between 1.5 and K - 0.5 on at least half the trajectories); at the suite's 1e-3 (PU.SPREAD) every weight is 0 or 1 at these scales
DENSITY_SEED = PU.NOISE_SEED
IMPORTANCE_NOISE = {"cvs_ald": 1e-4, "challenge_gauss": 3e-7, "proc_ald": 1e-4}
DENSITY_ENTRIES = [(name, regime) for name in CASES for regime in scored_regimes(name)]


def density_case(name, regime, importance=False):
    return density_build(name, regime, DENSITY_SEED, IMPORTANCE_NOISE[name] if importance else 1.0)


def spread_weights(ess, K=DENSITY_K):
    """At least half the trajectories have 1.5 < ESS < K - 0.5."""
    ess = np.asarray(ess)
    return 2 * int(((ess > 1.5) & (ess < K - 0.5)).sum()) >= ess.size


def density_ok(c):
    if not kinks_ok(c):
        return False
    want = PU.oracle_points(c)
    return crossing_ok(want) and 2 * int((~want["excl"].any(0).any((1, 2))).sum()) >= want["excl"].shape[1]


# ---- posterior_refine ------------------------------------------------------------------------------------------------------------------------
REFINE_B, REFINE_K = 4, 3


REFINE_ENTRIES = [(name, regime) for name in CASES if not name.startswith("proc") for regime in scored_regimes(name)]


def refine_case(name, regime):
    return apply(regime, RFU.build(name, "rk4", REFINE_B, REFINE_K))


def refine_oracles(c):
    """The fp64 and the fp32 CPU oracle of F and dF/d(loc, rho) at the encoder's posterior (RFU.value_and_grad), and the bars under the
    rule: dict(F, mag, grad (fp64), f_bar [B] = REL mag x factor, g_bar = max(GRAD_REL, 4 x fp32 distance), r32 = (F, grad) distances in
    units of the suite's bars)."""
    out = {}
    for dt in (torch.float64, torch.float32):
        loc, rho = RFU.encoder(c, dt)
        F, mag, g = RFU.value_and_grad(c, loc, rho, dtype=dt)
        out[dt] = (F.double().numpy(), mag.double().numpy(), g.double().numpy())
    F, mag, g = out[torch.float64]
    rf = float((np.abs(out[torch.float32][0] - F) / (RFU.REL * mag)).max())
    rg = float(RFU.norm_err(out[torch.float32][2], g).max())
    return dict(F=F, mag=mag, grad=g, f_bar=RFU.REL * mag * factor(rf), g_bar=G.bar(RFU.GRAD_REL, rg), r32=(rf, rg / RFU.GRAD_REL))


def refine_objective_bar(c, loc, scale):
    """(F, bar) [B] of the fp64 oracle objective at a given (loc, scale): REL mag, raised to 4 x the fp32 oracle's distance at that point."""
    F, mag = RFU.objective_at(c, loc, scale)
    with torch.no_grad():
        F32, _ = RFU.objective(c, torch.as_tensor(loc, dtype=torch.float32), torch.as_tensor(scale, dtype=torch.float32).log(), dtype=torch.float32)
    r = float((np.abs(F32.double().numpy() - F) / (RFU.REL * mag)).max())
    return F, RFU.REL * mag * factor(r), r


# ---- the bar rule on the scored-draw oracles ---------------------------------------------------------------------------------------------------
def _worst(err, bar, skip=None):
    r = np.abs(err) / np.maximum(bar, 1e-300)
    return float(np.where(skip, 0.0, r).max()) if skip is not None else float(r.max())


def factor(r32):
    """regime_util.bar as a factor on a bar: 1, or 4 x the fp32 CPU oracle's distance in units of that bar where that is larger."""
    return max(1.0, 4.0 * r32)


class Density:
    """Both oracles of one density entry (PU.oracle_points in fp64 and fp32) and, for given log-weights, the reference planes and slots,
    their bars (PU.bars) and the fp32 oracle's distance in units of each bar: per plane over the points outside the crossing exclusion, the
    slots over the trajectories without an excluded point."""

    def __init__(self, c, tag):
        self.c, self.tag = c, tag
        self.want, self.w32 = PU.oracle_points(c), PU.oracle_points(c, dtype=torch.float32)
        self.pts, self.clean = PU.conditions(self.want, tag)

    def fold(self, lw, mask=None):
        planes, slots = PU.fold64(self.want["ell"], lw, mask)
        pb, sb = PU.bars(self.want["bar"], lw, planes, mask)
        p32, s32 = PU.fold64(self.w32["ell"], lw, mask)
        r32 = [_worst(p32[j] - planes[j], pb[j], self.pts) for j in range(3)]
        cols = [0, 1, 2, 4, 5]
        r32.append(_worst((s32 - slots)[self.clean][:, cols], np.where(sb > 0, sb, 1.0)[self.clean][:, cols]) if self.clean.any() else 0.0)
        return planes, slots, pb, sb, r32

    def check(self, point, summary, lw, what):
        """PU.check under the bar rule; returns (worst error / bar per plane and for the slots, the factors)."""
        got, gs = point.detach().double().cpu().numpy(), summary.detach().double().cpu().numpy()
        planes, slots, pb, sb, r32 = self.fold(lw)
        f = [factor(r) for r in r32]
        assert np.isfinite(got).all() and np.isfinite(gs).all(), what
        worst = [_worst(got[j] - planes[j], pb[j] * f[j], self.pts) for j in range(3)]
        cols = [0, 1, 2, 4, 5]
        err, sbc = np.abs(gs[self.clean][:, cols] - slots[self.clean][:, cols]), sb[self.clean][:, cols] * f[3]
        rs = np.where(sbc > 0, err / np.maximum(sbc, 1e-300), err)
        worst.append(float(rs.max()) if rs.size else 0.0)
        print("%s %s: error / bar: lppd %.3f, mean_ll %.3f, var_ll %.3f, slots %.3f; bar factors %s (fp32 oracle / suite bar %s); excluded %d of %d points"
              % (self.tag, what, worst[0], worst[1], worst[2], worst[3], ["%.2f" % x for x in f], ["%.2f" % x for x in r32], int(self.pts.sum()), self.pts.size))
        assert max(worst) <= 1.0, (self.tag, what, worst)
        assert np.array_equal(gs[:, 3], slots[:, 3]) and np.array_equal(gs[:, 6], slots[:, 6])
        assert np.all(got[2] >= 0.0) and np.all(got[0] >= got[1] - 2.0 ** -21 * (1.0 + np.abs(got[1])))
        PU.check_own_sums(point, summary, self.tag + " " + what)
        return worst, f


class Loo:
    """Both oracles of one LOO entry, the restatement on each (elpd_loo, khat, lppd), LU.bars on the fp64 oracle's l and the fp32 oracle's
    distance in units of the elpd_loo and lppd bars over the points outside the crossing exclusion."""

    def __init__(self, c):
        self.want, w32 = PU.oracle_points(c), PU.oracle_points(c, dtype=torch.float32)
        ell = self.want["ell"]
        self.crossing = self.want["excl"].any(0)
        self.e, self.k = LU.psis(ell)
        self.eb, self.kb = LU.bars(ell, self.want["bar"])
        self.lppd = LU.lppd(ell)
        self.lb = self.want["bar"].max(0) + 2.0 ** -22 * np.abs(self.lppd)
        e32, self.k32 = LU.psis(w32["ell"])
        self.r32 = (_worst(e32 - self.e, self.eb, self.crossing), _worst(LU.lppd(w32["ell"]) - self.lppd, self.lb, self.crossing))
        self.khat_level = ~self.crossing & (self.kb <= 0.05)            # where khat is compared at the oracle level


# ---- the whole-curve calls -------------------------------------------------------------------------------------------------------------------
CURVE_B, CURVE_NS = 4, 7
# call -> its regimes: ties and all on posterior draws for every call; prior_scales (PRIOR draws) where the statistic sorts or divides by a
# spread (quantiles, the band, the attribution indices); raw_units where the statistic reads the observations (the band's obs_dev, the
# calibration counts, the cohort L1)
CURVE_CALLS = {"recon_moments": ("ties", "all"), "recon_quantiles": ("ties", "all", "prior_scales"), "joint_band": ("ties", "all", "prior_scales", "raw_units"),
               "calibration": ("ties", "all", "raw_units"), "curve_summary": ("ties", "all"), "latent_attribution": ("ties", "all", "prior_scales"),
               "mechanism_moments": ("ties", "all"), "intervene_moments": ("ties", "all"), "cohort_moments": ("ties", "all", "raw_units"),
               "forecast_moments": ("ties", "all")}
BAND_NS = (7, 33)
COHORT_IDS, COHORT_G, COHORT_CHUNK = (0, 1, 0, -1), 3, 2          # B = 4: a two-member cohort, a singleton, an empty one, one trajectory in none


def curve_entries(call):
    return [(name, regime) for name in CASES for regime in CURVE_CALLS[call]]


def is_post(regime):
    """prior_scales moves the prior nets: its entries draw from the PRIOR; every other regime from the posterior."""
    return regime != "prior_scales"


_curve_cases = {}


def curve_case(call, name, regime, ns=CURVE_NS):
    """regime_util.apply on the call's own small build (B = 4, ``ns`` draws, rk4): RU.build for the calls on the head curves, AU.build
    (second noise tensor), MU.build (the conditioned grid), FU.build (the output grid).  Computed once per key, shared, not to be changed."""
    from tests import attribution_util as AU, forecast_util as FU, mechanism_util as MU, recon_moments_util as RU
    build = {"latent_attribution": AU.build, "mechanism_moments": MU.build, "forecast_moments": FU.build}.get(call, RU.build)
    key = (build.__module__, name, regime, ns)
    if key not in _curve_cases:
        _curve_cases[key] = apply(regime, build(name, "rk4", B=CURVE_B, ns=ns))
    return _curve_cases[key]


def oracle_draws(c, post, dtype=torch.float64, eps=None):
    """[Q, ns, B, C, T] float64 numpy: the oracle's head curves of every draw (cohort_util.oracle_draws) computed in ``dtype``."""
    from oracle import slode_oracle as O
    from tests import recon_moments_util as RU
    ospec = c["ospec"]
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    e = (c["eps"] if eps is None else eps).to(dtype)
    ns, B, L = e.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p, c["obs"].to(dtype), ospec.pool_size) if post else O.prior_loc_scale(p, ospec, c["u"].to(dtype))
        mu = RU.oracle_curves(p, ospec, (loc.unsqueeze(0) + scale.unsqueeze(0) * e).reshape(ns * B, L), c["times"].to(dtype), ospec.solver)
    return mu.reshape(mu.shape[0], ns, B, mu.shape[2], mu.shape[3]).double().numpy()


_draws = {}


def draws(call, name, regime, ns=CURVE_NS):
    """(v64, v32) of ``curve_case``'s entry: once per key."""
    c = curve_case(call, name, regime, ns)
    key = (id(c),)
    if key not in _draws:
        _draws[key] = tuple(oracle_draws(c, is_post(regime), dt) for dt in (torch.float64, torch.float32))
        for a in _draws[key]:
            a.setflags(write=False)
    return _draws[key]


def moment_bars(v64, v32):
    """(mean64, sd64, mean bar, sd bar [Q, B, C, T], (fp32 oracle's worst mean and sd distance in units of RU.MEAN_BAR / RU.SD_BAR)): the
    bars of recon_moments_util.check under the bar rule."""
    from tests import recon_moments_util as RU
    m, s = v64.mean(1), v64.std(1)
    scale = np.maximum(1.0, np.abs(m))
    rm = float((np.abs(v32.mean(1) - m) / (RU.MEAN_BAR * scale)).max())
    rs = float((np.abs(v32.std(1) - s) / (RU.SD_BAR * scale)).max())
    return m, s, RU.MEAN_BAR * scale * factor(rm), RU.SD_BAR * scale * factor(rs), (rm, rs)


def curve_reach(v64, v32):
    """What an entry's curves reach: dict(level (largest |mean|), sd_over_level (smallest sd / max(1, |mean|) over the elements whose sd is
    not zero), zero_sd (elements with sd exactly 0, fp64 and fp32), elements)."""
    m, s, s32 = v64.mean(1), v64.std(1), v32.std(1)
    live = s > 0
    return dict(level=float(np.abs(m).max()), sd_over_level=float((s[live] / np.maximum(1.0, np.abs(m[live]))).min()), zero_sd=(int((s == 0).sum()), int((s32 == 0).sum())),
                elements=int(s.size))


def constant_channel(v):
    """Channel 0 of draws [Q, ns, B, C, T] is exactly +0.0 in every draw (the ties regime)."""
    ch = v[:, :, :, 0]
    return bool((ch == 0.0).all()) and not bool(np.signbit(ch).any())


SUMMARY_LEVELS = (0.5, 0.3, 0.7, 0.1, 0.9, 0.02, 0.98)


def summary_thresholds(v64, regime):
    """(thr [C] fp32, the quantile level taken per channel): summary_util.thresholds takes the median of the oracle's head-0 values of a
    channel.  Away from the initialisation the curves run into plateaus that the draws share to within a bar (challenge_gauss at `all`:
    sd / level 5e-5), and a threshold ON a plateau makes a seventh of all points near it, where the count rule says nothing.  Per channel:
    the first level of SUMMARY_LEVELS at which the near share of that channel is at most half of summary_util.NEAR_SHARE -- decided on the
    oracle alone.  The constant channel of `ties` keeps its median, 0: it is compared exactly, not by the rule."""
    from tests import summary_util as SU
    vk = np.moveaxis(v64, 1, 0)
    C = v64.shape[3]
    thr, took = np.zeros(C, np.float32), []
    for ch in range(C):
        vals = v64[0][:, :, ch].reshape(-1)
        for q in SUMMARY_LEVELS:
            t = np.float32(np.quantile(vals, q))
            if (regime == "ties" and ch == 0) or SU.near(vk[:, :, :, ch:ch + 1], np.array([t])).mean() <= 0.5 * SU.NEAR_SHARE:
                break
        else:
            raise AssertionError("no level of SUMMARY_LEVELS keeps channel %d clear of near points" % ch)
        thr[ch] = t
        took.append(q)
    return thr, took
