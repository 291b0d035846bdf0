"""Test infrastructure of the pointwise predictive density (slode_pointwise_density): the fp64 oracle of the per-point log-likelihood
l_k[i] -- the pieces of oracle/slode_oracle.py composed WITHOUT the sums over the points -- the fp64 fold of K draws to the call's three
planes and eight slots for given log-weights, and the bars.  Builds on tests/traj_bounds_util.py.  Not imported by the product.

Bars (derived, not chosen).  The project's parity bar is REL = 1e-5 on a value, so a head curve is trusted to dmu = REL max(1, |mu|) and a
point term to
    bar_k[i] = sum_q |dl/dmu_q| dmu_q + REL sum_q |term_q|,     dl/dmu = side weight / scale (ALD), |r| / scale^2 (Gauss)
(a relative bar on |l| alone is wrong: r = y - mu cancels at |mu| up to 126 in these cases).  From it: lppd within max_k bar_k (logsumexp
is non-expansive in the sup norm) + 2^-22 |value|; mean_ll within sum_k w_k bar_k; var_ll within 2 sd d + d^2, d = max_k bar_k; a slot
within the fp64 sum of its points' bars; n_in / n_out exact.  In importance mode the reference fold takes the kernel's OWN loss_kb for the
weights and the oracle's l for the points (the split of traj_bounds_util.check_reduction: 0.05 nat in a loss moves the weights by percents,
and that is the scorer's error, held by the traj_bounds tests).

The ALD exclusion.  For tau != 0.5 the term jumps in mu at y = mu.  A (draw, point) pair is excluded from the per-point
comparisons where the fp64 oracle has |y - mu_q| <= 10 REL max(1, |y|, |mu_q|) for the q75 or the q25 head; a point where any of its draws
is.  At most CAP = 0.1 % of a configuration's points may be excluded -- a condition, asserted on the oracle (tests/test_pointwise_cpu.py);
the slots are compared on trajectories without an excluded point, which must be at least half of them (``conditions``: beyond K = 64 draws
per point the cap can only hold for the pairs, and says so)."""
import numpy as np
import torch

from oracle import slode_oracle as O
from tests import eval_stats_util as EU
from tests import traj_bounds_util as TU

REL = TU.REL
CAP = 1e-3
NOISE_SEED = TU.NOISE_SEED
SLOTS = 8

# every configuration the GPU tests compare with the oracle: (case, solver, B or None: the case's own, K, noise scale)
PARITY = [(case, solver, None, 4, 1.0) for case in EU.CASES for solver in EU.SOLVERS]
SIZES = [("cvs_gauss", 63, 2, {}), ("cvs_gauss", 65, 2, {}), ("cvs_gauss", 257, 2, {}), ("cvs_ald", 3, 200, {}), ("challenge_gauss", 2, 64, {}),
         ("proc_gauss", 65, 2, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}), ("cvs_ald", 9, 7, {"SLODE_ODE_GENERIC": "1"}),
         ("proc_ald", 9, 2, {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}), ("cvs_gauss", 5, 1, {})]
SPREAD = [("cvs_ald", "rk4", None, 8, 1e-3), ("challenge_gauss", "rk4", None, 8, 1e-3)]     # non-degenerate importance weights
CONFIGS = PARITY + [(case, "rk4", B, K, 1.0) for case, B, K, _ in SIZES] + SPREAD


def config(cfg, seed=NOISE_SEED):
    """The case of one entry of CONFIGS: its noise scaled in place."""
    case, solver, B, K, scale = cfg
    c = build(case, solver, B, K, seed)
    c["eps"] = scale * c["eps"]
    return c


def build(case, solver="rk4", B=None, K=4, seed=NOISE_SEED):
    """TU.build with the noise seed as an argument (the default: its own)."""
    return dict(EU.build_case(case, ("eps", K, seed), solver, B), K=K)


def oracle_points(c, eps=None, dtype=torch.float64, posterior=None):
    """Per (draw, trajectory, channel, time): dict(ell, bar [K, B, C, T] float64, excl [K, B, C, T] bool) computed in ``dtype``.  ell: the
    sum over the heads of the log-likelihood terms of the point; ``posterior`` = (loc, scale) replaces the encoder's."""
    ospec = c["ospec"]
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    obs, times = c["obs"].to(dtype), c["times"].to(dtype)
    e = (c["eps"] if eps is None else eps).to(dtype)
    K, B, L = e.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p, obs, ospec.pool_size) if posterior is None else (t.to(dtype) for t in posterior)
        z = (loc.unsqueeze(0) + scale.unsqueeze(0) * e).reshape(K * B, L)
        ob = obs.repeat(K, 1, 1)
        if ospec.gauss:
            _, mean, std = O.decoder_gauss(p, z, times, ospec.solver)
            r = ob - mean
            ell = -torch.log(std) - 0.5 * np.log(2 * np.pi) - 0.5 * (r / std) ** 2
            bar = r.abs() / std ** 2 * REL * mean.abs().clamp_min(1.0) + REL * ell.abs()
            excl = torch.zeros_like(ell, dtype=torch.bool)
        else:
            _, mu75, mu50, mu25, std = O.decoder_ald(p, z, times, ospec.solver)
            d = ospec.quantile_diff
            ell, bar, excl = 0.0, 0.0, torch.zeros_like(mu50, dtype=torch.bool)
            for mu, tau in ((mu50, 0.5), (mu75, 0.5 + d), (mu25, 0.5 - d)):
                side = torch.where(ob.ge(mu), torch.full_like(mu, tau), torch.full_like(mu, 1 - tau))
                term = side * (-torch.log(2 * std) - (ob - mu).abs() / std)
                ell = ell + term
                bar = bar + side / std * REL * mu.abs().clamp_min(1.0) + REL * term.abs()
                if tau != 0.5:
                    excl |= (ob - mu).abs() <= 10 * REL * torch.maximum(torch.ones_like(mu), torch.maximum(ob.abs(), mu.abs()))
    shp = (K, B) + tuple(obs.shape[1:])
    return dict(ell=ell.double().reshape(shp).numpy(), bar=bar.double().reshape(shp).numpy(), excl=excl.reshape(shp).numpy())


def log_weights(K, B, loss=None):
    """[K, B] normalised log-weights in fp64: -log K (posterior mode), or -loss - logsumexp(-loss) of per-draw losses [K, B]."""
    if loss is None:
        return np.full((K, B), -np.log(float(K)))
    a = -np.asarray(loss, dtype=np.float64)
    m = a.max(0)
    return a - (m + np.log(np.exp(a - m[None]).sum(0)))[None]


def fold64(ell, lw, mask=None):
    """The call's outputs from ell [K, B, C, T] and normalised log-weights lw [K, B], in fp64: planes [3, B, C, T] (lppd | mean_ll | var_ll)
    and slots [B, 8].  mask [B, C, T]: in where > 0 (None: every point in)."""
    ell, lw = np.asarray(ell, np.float64), np.asarray(lw, np.float64)
    K, B, C, T = ell.shape
    a = lw[:, :, None, None] + ell
    m = a.max(0)
    lppd = m + np.log(np.exp(a - m[None]).sum(0))
    w = np.exp(lw)[:, :, None, None]
    mean = (w * ell).sum(0)
    var = (w * (ell - mean[None]) ** 2).sum(0)
    inn = np.ones((B, C, T), bool) if mask is None else np.asarray(mask) > 0
    slots = np.zeros((B, SLOTS))
    for j, (v, sel) in enumerate(((lppd, inn), (var, inn), (mean, inn), (np.ones_like(mean), inn), (lppd, ~inn), (mean, ~inn), (np.ones_like(mean), ~inn))):
        slots[:, j] = (v * sel).sum((1, 2))
    slots[:, 7] = 1.0 / (np.exp(lw) ** 2).sum(0)
    return np.stack([lppd, mean, var]), slots


def bars(bar, lw, planes, mask=None):
    """(plane bars [3, B, C, T], slot bars [B, 7]) of the module docstring for the reference ``planes`` under the log-weights ``lw``."""
    w = np.exp(np.asarray(lw, np.float64))[:, :, None, None]
    d = bar.max(0)
    pb = np.stack([d + 2.0 ** -22 * np.abs(planes[0]), (w * bar).sum(0), 2.0 * np.sqrt(planes[2]) * d + d * d])
    B = bar.shape[1]
    inn = np.ones(bar.shape[1:], bool) if mask is None else np.asarray(mask) > 0
    sb = np.zeros((B, 7))
    for j, (v, sel) in enumerate(((pb[0], inn), (pb[2], inn), (pb[1], inn), (None, inn), (pb[0], ~inn), (pb[1], ~inn), (None, ~inn))):
        sb[:, j] = 0.0 if v is None else (v * sel).sum((1, 2))
    return pb, sb


MANY_DRAWS = 64      # above this K the cap counts (draw, point) pairs, not points: see ``conditions``


def excluded(want):
    """(points [B, C, T] excluded, their share of the points, trajectories [B] without an excluded point)."""
    pts = want["excl"].any(0)
    return pts, pts.mean(), ~pts.any((1, 2))


def conditions(want, tag):
    """The conditions of the exclusion, on the oracle alone: ``(excluded points, trajectories whose slots are compared with the oracle)``.
    The share of excluded (draw, point) pairs is at most CAP in every configuration.  Up to K = MANY_DRAWS the share of excluded POINTS is
    at most CAP as well, and at least half of the trajectories have no excluded point: their slots are compared with the oracle.  Beyond
    it (SIZES' K = 200 on cvs_ald: 13 of 360,000 pairs, 3.6e-5, the rate of the K = 4 cases -- but a point is excluded where ANY of its 200
    draws is, 11 of 1,800 points, which no noise seed can bring under 0.1 %) the points are still compared one by one outside the
    exclusion, and no slot is compared with the oracle: the slots are held to the fp64 sum of the kernel's own planes (``check_own_sums``,
    every trajectory, in every configuration), which separates the reduction from the scorer."""
    pts, share, clean = excluded(want)
    K = want["excl"].shape[0]
    assert want["excl"].mean() <= CAP, (tag, "excluded share of the (draw, point) pairs", want["excl"].mean())
    if K > MANY_DRAWS:
        return pts, np.zeros_like(clean)
    assert share <= CAP, (tag, "excluded share of the points", share)
    assert clean.sum() * 2 >= clean.size, (tag, "trajectories without an excluded point", int(clean.sum()), clean.size)
    return pts, clean


def check_own_sums(point, summary, tag, mask=None):
    """Slots 0 - 6 against the fp64 sums of the kernel's OWN planes over the in / out points: a sum of fp32 values formed in fp64 and rounded
    once is within 2^-23 of its magnitude (+ the fp64 rounding of n additions, 2^-50 of the sum of magnitudes); the counts exact."""
    got, gs = point.detach().double().cpu().numpy(), summary.detach().double().cpu().numpy()
    B, C, T = got.shape[1:]
    inn = np.ones((B, C, T), bool) if mask is None else np.asarray(mask) > 0
    worst = 0.0
    for j, (v, sel) in enumerate(((got[0], inn), (got[2], inn), (got[1], inn), (np.ones_like(got[0]), inn), (got[0], ~inn), (got[1], ~inn),
                                  (np.ones_like(got[0]), ~inn))):
        s, mag = (v * sel).sum((1, 2)), (np.abs(v) * sel).sum((1, 2))
        tol = 2.0 ** -23 * np.abs(s) + 2.0 ** -50 * mag
        assert np.all(np.abs(gs[:, j] - s) <= tol), (tag, "slot %d against the sum of the call's own planes" % j, np.abs(gs[:, j] - s).max())
        worst = max(worst, float((np.abs(gs[:, j] - s) / np.maximum(tol, 1e-300)).max()))
    print("%s: slots against the fp64 sums of the call's own planes: worst error / bar %.3f" % (tag, worst))


def check(point, summary, want, lw, tag, mask=None):
    """The kernel's planes and slots against the fold of the oracle's ell under ``lw``, at the bars.  Prints the worst ratios first;
    returns them (planes 0-2, slots)."""
    got, gs = point.detach().double().cpu().numpy(), summary.detach().double().cpu().numpy()
    planes, slots = fold64(want["ell"], lw, mask)
    pb, sb = bars(want["bar"], lw, planes, mask)
    pts, clean = conditions(want, tag)
    assert np.isfinite(got).all() and np.isfinite(gs).all(), tag
    rp = np.where(pts[None], 0.0, np.abs(got - planes) / pb.clip(1e-300))
    cols = (0, 1, 2, 4, 5)
    err, sbc = np.abs(gs[clean][:, cols] - slots[clean][:, cols]), sb[clean][:, cols]
    rs = np.where(sbc > 0, err / sbc.clip(1e-300), err)                                   # (no point on that side of the mask: 0 exactly)
    worst = [float(rp[j].max()) for j in range(3)] + [float(rs.max()) if rs.size else 0.0]
    print("%s: error / bar: lppd %.3f, mean_ll %.3f, var_ll %.3f, slots %.3f (excluded points %d of %d, slots compared on %d of %d trajectories)"
          % (tag, worst[0], worst[1], worst[2], worst[3], int(pts.sum()), pts.size, int(clean.sum()), clean.size))
    for j, n in enumerate(("lppd", "mean_ll", "var_ll")):
        assert worst[j] <= 1.0, (tag, n, worst[j])
    assert worst[3] <= 1.0, (tag, "slots", worst[3])
    assert np.array_equal(gs[:, 3], slots[:, 3]) and np.array_equal(gs[:, 6], slots[:, 6]), (tag, "n_in / n_out")
    assert np.all(got[2] >= 0.0), (tag, "var_ll < 0")
    # Jensen, to the rounding of the two values (each rounded once: 2^-24 |value|) and of the fp32 log-weights, exp and log behind lppd
    assert np.all(got[0] >= got[1] - 2.0 ** -21 * (1.0 + np.abs(got[1]))), (tag, "lppd < mean_ll", (got[1] - got[0]).max())
    check_own_sums(point, summary, tag, mask)
    return worst


def masked_loss(rows, want, mask):
    """The fp64 oracle's per-draw losses [K, B] (TU.oracle_rows) with the mask's weights on the likelihood terms: loss + sum_i (1 - w_i) ell_i."""
    w = np.asarray(mask, np.float64)
    return rows["loss"] + ((1.0 - w)[None] * want["ell"]).sum((2, 3))


def prefix_mask(c, t0=None):
    """[B, C, T] float32: 1 on the first t0 time points (default: T // 2 + 3), 0 after them."""
    B, C, T = c["obs"].shape
    m = torch.zeros(B, C, T)
    m[:, :, :(T // 2 + 3 if t0 is None else t0)] = 1.0
    return m
