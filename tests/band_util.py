"""Test infrastructure of the simultaneous bands (slode_joint_band): the level rule restated, the numpy restatement of the deviations on given
curves, moments and floor, the order statistics and counts on given deviations, the bars that carry the recon_moments bars through the
quotient, the hand count of the kernel's LDS tables.  Not imported by the product.

What is exact and what has a bar.  dev_k = max_t fl(fl(|v_k(t) - m(t)|) / s(t)) is two correctly rounded fp32 operations per point and a
selection over t; crit is a selection among the K deviations; joint is a count over them: on the kernel's own curve values, mean and sd all
three are held to numpy EXACTLY.  Against the fp64 oracle a curve value and the mean are within RU.MEAN_BAR scale and the sd within RU.SD_BAR
scale (scale = max(1, |mean64|)), so a point's quotient moves by at most (2 MEAN_BAR scale + e64 SD_BAR scale) / sd64 (to first order in
SD_BAR scale / sd64), and e64 <= dev64: `dev_bar`.  A maximum is 1-Lipschitz in the sup norm, and so is an order statistic: crit is held to
the largest bar over the draws of its curve.  A draw may change sides of z only if the oracle's deviation is within its bar of z."""
import math
from statistics import NormalDist

import numpy as np

from tests import lds_util as LU
from tests import recon_moments_util as RU
from tests import summary_util as SU

_f32 = RU._f32
NEAR_SHARE = SU.NEAR_SHARE
COUNT_LEVELS = (0.5, 0.9)                   # informative levels of the count rule: z = 0.674, 1.645, inside the deviations' range
CLEAR_LEVEL = {7: 0.995, 33: 1.0}           # per K: a level whose z (2.807; inf) clears sqrt(K - 1) (2.449; 5.657) by more than the worst bar
FILL = -12345.5            # the outputs are pre-filled with it: every element must be written


def level_rule(levels, K):
    """(ranks, z) as the issue states them, in double: r = min(K, max(1, ceil(level K - 1e-9))), z = Phi^-1((1 + level) / 2) (inf at 1)."""
    ranks = [min(K, max(1, int(math.ceil(float(p) * K - 1e-9)))) for p in levels]
    z = [math.inf if float(p) >= 1.0 else NormalDist().inv_cdf((1.0 + float(p)) / 2.0) for p in levels]
    return ranks, z


def dev_f32(curves, mean, sd, floor=0.0):
    """curves [K, ..., T], mean / sd [..., T], all fp32 -> (dev [K, ...], points [...]): per point fl(fl(|v - m|) / s) where s > floor, the
    maximum over those points, 0 where there is none."""
    v, m, s = _f32(curves), _f32(mean), _f32(sd)
    on = s > np.float32(floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = _f32(_f32(np.abs(_f32(v - m))) / s)
    e = np.where(on, e, np.float32(-1.0))
    return _f32(np.maximum(e.max(-1), np.float32(0.0))), on.sum(-1)


def crit_joint(dev, levels):
    """dev [K, ...] fp32 -> (crit [..., Lv] = np.sort(dev)[r - 1], joint [..., Lv] = #{dev <= float32(z)} / K in fp32)."""
    K = dev.shape[0]
    ranks, z = level_rule(levels, K)
    srt = np.sort(_f32(dev), axis=0)
    crit = np.stack([srt[r - 1] for r in ranks], -1)
    joint = np.stack([_f32(_f32((dev <= np.float32(zj)).sum(0)) / np.float32(K)) for zj in z], -1)
    return crit, joint


def oracle_dev(v64, y64=None, floor=0.0):
    """v64 [K, ..., T] fp64 (the oracle's draws of one side) -> dict: mean, sd [..., T]; dev [K, ...]; points [...]; obs_dev [...] with y64."""
    m, s = v64.mean(0), v64.std(0)
    on = s > floor
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(on, np.abs(v64 - m) / s, -1.0)
        out = dict(mean=m, sd=s, dev=np.maximum(e.max(-1), 0.0), points=on.sum(-1))
        if y64 is not None:
            out["obs_dev"] = np.maximum(np.where(on, np.abs(y64 - m) / s, -1.0).max(-1), 0.0)
    return out


def dev_bar(o, on=None):
    """The bar of every deviation [K, ...] of ``oracle_dev``'s dict: max over the participating t of (2 MEAN_BAR scale + dev64 SD_BAR scale)
    / sd64, scale = max(1, |mean64|)."""
    scale = np.maximum(1.0, np.abs(o["mean"]))
    on = (o["sd"] > 0.0) if on is None else on
    with np.errstate(divide="ignore", invalid="ignore"):
        per_t = (2.0 * RU.MEAN_BAR * scale + o["dev"][..., None] * RU.SD_BAR * scale) / o["sd"]
    return np.where(on, per_t, 0.0).max(-1)


def floor_in_gap(sd, lo=0.0, hi=1.0):
    """(floor, ratio): the geometric middle of the widest relative gap between neighbours of the sorted positive values of ``sd`` whose rank
    lies in [lo, hi] of them, and that gap's ratio: no value lies within a factor sqrt(ratio) of the floor."""
    s = np.unique(np.asarray(sd, dtype=np.float64).reshape(-1))
    s = s[s > 0.0]
    a, b = int(lo * (s.size - 1)), max(int(hi * (s.size - 1)), int(lo * (s.size - 1)) + 1)
    r = s[a + 1:b + 1] / s[a:b]
    i = int(r.argmax())
    return float(np.sqrt(s[a + i] * s[a + i + 1])), float(r[i])


def plan_bytes(T, S, C, L, H, n_u, gauss, K, generic=False):
    """The hand count of the kernel's LDS tables in bytes, every piece rounded to 16 B: the shared pieces (step table 2 (T - 1) S, the H
    rows of 2 + 2 S floats rounded to four, w1 2 H L, b1 2 H, w2 H S + S, head weights Q C S, biases 2 S, z L, labels max(n_u, 1), h0 H,
    x0 S), the moment table 3 Q C T whose third slot is the value table of the second sweep, the deviations Q C K, loc | scale."""
    r4, Q = LU.r4, 1 if gauss else 3
    return 4 * (LU.fwd_shared_floats(T, S, C, L, H, n_u, gauss, generic) + r4(3 * Q * C * T) + r4(Q * C * K) + 2 * r4(L))
