"""Test infrastructure of the sample quantiles (slode_recon_quantiles): the numpy restatement of the rank rule, the depth rule, the plan and
the selection with its fp32 interpolation, and the bars.  Not imported by the product.

An order statistic is a SELECTION among the draw values: on the kernel's own fp32 curve values the restatement is exact (bitwise).  Against
np.quantile(method="linear") in fp64 on the same fp32 values the interpolation differs by at most three fp32 roundings (g, the difference,
the fma), each relative to a magnitude no larger than 2 max(|v_lo|, |v_hi|): the bar 5 2^-24 max(|v_lo|, |v_hi|).  Against the fp64 oracle an
order statistic is 1-Lipschitz in the sup norm over the draws, so the per-value bar of the head curves (RU.MEAN_BAR) carries over with the
largest draw value as its scale."""
import numpy as np

from tests import lds_util as LU
from tests import recon_moments_util as RU

U = 2.0 ** -24
MAX_LEVELS = 8
LDS_MAX = 160 * 1024
# the level sets of the tests: the envelope, the band, the median, five levels, eight levels (unordered, with a duplicate)
LEVEL_SETS = {"envelope": (0.0, 1.0), "band": (0.025, 0.975), "median": (0.5,), "five": (0.05, 0.25, 0.5, 0.75, 0.95),
              "eight": (0.975, 0.0, 0.5, 0.25, 1.0, 0.5, 0.025, 0.75)}


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def ranks(levels, K):
    """(lo, hi, g32) per level: h = q (K - 1) in fp64, lo = floor(h), hi = min(lo + 1, K - 1), g = float32(h - lo)."""
    h = np.asarray(levels, dtype=np.float64) * (K - 1)
    lo = np.clip(np.floor(h).astype(np.int64), 0, K - 1)
    return lo, np.minimum(lo + 1, K - 1), _f32(h - lo)


def depths(levels, K):
    """(m_lo, m_hi): every needed rank r (lo of every level; hi where g != 0 -- an upper rank without weight is not read) from the bottom
    buffer (cost r + 1) or the top one (cost K - r), whichever costs less, the bottom on a tie; the largest cost given to each side;
    m_lo + m_hi >= K: everything is kept, (K, 0)."""
    lo, hi, g = ranks(levels, K)
    m_lo = m_hi = 0
    for r in list(lo) + [h for h, gg in zip(hi, g) if gg != 0.0]:
        r = int(r)
        if r + 1 <= K - r:
            m_lo = max(m_lo, r + 1)
        else:
            m_hi = max(m_hi, K - r)
    return (K, 0) if m_lo + m_hi >= K else (m_lo, m_hi)


def select(v_sorted_f32, levels):
    """The kernel's store on values sorted along axis 0 ([K, ...] fp32): out = fma(g, v[hi] - v[lo], v[lo]) -- the difference rounded to
    fp32, the fma emulated in fp64 (the product of two fp32 values is exact there) and rounded once.  [Lv, ...] fp32."""
    v = _f32(v_sorted_f32)
    lo, hi, g = ranks(levels, v.shape[0])
    out = []
    for l, h, gg in zip(lo, hi, g):
        dv = _f32(v[h] - v[l])
        out.append(_f32(np.float64(gg) * dv.astype(np.float64) + v[l].astype(np.float64)))
    return np.stack(out)


def numpy_bar(v_sorted_f32, levels):
    """5 2^-24 max(|v_lo|, |v_hi|) per level and value: the bar of ``select`` against np.quantile in fp64 on the same fp32 values."""
    v = np.abs(_f32(v_sorted_f32).astype(np.float64))
    lo, hi, _ = ranks(levels, v.shape[0])
    return np.stack([5.0 * U * np.maximum(v[l], v[h]) for l, h in zip(lo, hi)])


def oracle_bar(draws64):
    """RU.MEAN_BAR max(1, max_k |v_k|) per value of the oracle's draws [K, ...]."""
    return RU.MEAN_BAR * np.maximum(1.0, np.abs(draws64).max(0))


def fixed_floats(spec, T):
    """The floats of the kernel's LDS pieces that do not depend on the plan: the shared forward pieces (step table 2 (T - 1) S, one row of
    2 + 2 S floats rounded up to four per hidden unit, the transposed first layers L x 2 H, their biases 2 H, the init net's output layer
    H S + S, the head weights Q C S, the dynamics biases 2 S, z, the labels, the init net's hidden layer, x0), loc | scale and the level table
    3 x 8; every piece rounded up to 16 bytes."""
    return LU.spec_shared_floats(spec, T) + 2 * LU.r4(spec.latent_dim) + LU.r4(3 * MAX_LEVELS)


def plan(spec, T, K, levels, tile=0):
    """(tile, sweeps, m_lo, m_hi, lds_bytes) as slode_quantile_plan states it, or None where it refuses: tile = 0 takes the fewest sweeps whose
    tile = ceil(T / sweeps) fits the budget; a given tile is taken as it is."""
    m_lo, m_hi = depths(levels, K)
    QC = (1 if spec.gauss else 3) * spec.n_channels

    def nbytes(tl):
        return 4 * (fixed_floats(spec, T) + LU.r4((m_lo + m_hi) * QC * tl))
    if tile > 0:
        tl = tile
        if nbytes(tl) > LDS_MAX:
            return None
    else:
        if nbytes(1) > LDS_MAX:
            return None
        sw = 1
        while nbytes(-(-T // sw)) > LDS_MAX:
            sw += 1
        tl = -(-T // sw)
    return tl, -(-T // tl), m_lo, m_hi, nbytes(tl)
