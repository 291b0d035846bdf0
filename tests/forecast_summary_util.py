"""Test infrastructure of the forecast summaries (slode_forecast_summary): the fp64 truth -- tests/forecast_util.py's oracle draws on the output
grid, sliced at first_point, through tests/summary_util.py's functionals and moments -- the `since` rule, and the numpy restatement of
forecast_summary_kernel's order: the per-lane left-to-right fma chain of the 16-lane row walk, the four DPP combine steps with the tie rule,
and the per-window merge.  Not imported by the product.

Bars.  None of its own: against the oracle the sliced curves are curve summaries on the sub-grid times_out[i0:], held by SU.check_continuous and
SU.tolerant_violations unchanged (an index that flips next to a near-tie is theirs to handle)."""
import numpy as np

from tests import forecast_util as FU
from tests import recon_moments_util as RU
from tests import summary_util as SU

_f32 = RU._f32
_fma32 = RU._fma32
PARTNER = [np.arange(16) ^ 1, np.arange(16) ^ 2, (np.arange(16) & 8) | (7 - (np.arange(16) & 7)), 15 - np.arange(16)]   # xor 1, xor 2, half mirror, mirror


def first_point(times_out, since):
    """The first index whose time has reached ``since`` in the grid's own direction (None: 0) -- restated from the model's rule."""
    if since is None:
        return 0
    t = _f32(np.asarray(times_out)).reshape(-1)
    s = np.float32(since)
    reached = t >= s if t[-1] >= t[0] else t <= s
    assert reached.any()
    return int(np.flatnonzero(reached)[0])


def weights_from(times_out, i0):
    """The node weights of the sub-grid [i0, T_out) as the kernel forms them, indexed by the GLOBAL point (entries below i0 are never read):
    0.5f (t[min(g + 1, T_out - 1)] - t[max(g - 1, i0)])."""
    t = _f32(times_out)
    g = np.arange(t.size)
    return _f32(np.float32(0.5) * _f32(t[np.minimum(g + 1, t.size - 1)] - t[np.maximum(g - 1, i0)]))


def oracle_functionals(c, is_post, i0, thr, sense, eps=None):
    """(v64 [Q, ns, B, C, T_out - i0], f64 [ns, Q, B, C, 8]): the oracle's draws on times_out sliced at i0 and their functionals on the sub-grid."""
    v = FU.oracle_values(c, is_post, eps)[0][..., i0:]
    t = c["times_out"].numpy()[i0:]
    return v, SU.functionals(np.moveaxis(v, 1, 0), t, None if thr is None else np.asarray(thr, np.float64), sense)


# ---- the kernel's order ------------------------------------------------------------------------------------------------------------------
def row_walk(v, w, thr, sense):
    """summary_row_walk on n points of N curves: v [N, n] fp32, w [n] fp32, thr [N] fp32 or None.  Lane l walks the points l, l + 16, ... in
    increasing order; then the four combine steps.  Returns dict of [N] arrays: vmax, imax, vmin, imin, auc, tb, ihit (index n: none)."""
    N, n = v.shape
    vmax, vmin = np.full((N, 16), -np.inf, np.float32), np.full((N, 16), np.inf, np.float32)
    imax, imin, ihit = (np.full((N, 16), n, np.int64) for _ in range(3))
    auc, tb = np.zeros((N, 16), np.float32), np.zeros((N, 16), np.float32)
    for p in range(n):
        l, x, wp = p % 16, v[:, p], np.broadcast_to(w[p], (N,))
        up = x > vmax[:, l]
        vmax[:, l], imax[:, l] = np.where(up, x, vmax[:, l]), np.where(up, p, imax[:, l])
        dn = x < vmin[:, l]
        vmin[:, l], imin[:, l] = np.where(dn, x, vmin[:, l]), np.where(dn, p, imin[:, l])
        auc[:, l] = _fma32(wp, x, auc[:, l])
        if thr is not None:
            hit = x > thr if sense > 0 else x < thr
            tb[:, l] = _f32(tb[:, l] + np.where(hit, wp, np.float32(0)))
            ihit[:, l] = np.where(hit & (ihit[:, l] == n), p, ihit[:, l])
    for part in PARTNER:
        ov, oi = vmax[:, part], imax[:, part]
        take = (ov > vmax) | ((ov == vmax) & (oi < imax))
        vmax, imax = np.where(take, ov, vmax), np.where(take, oi, imax)
        ov, oi = vmin[:, part], imin[:, part]
        take = (ov < vmin) | ((ov == vmin) & (oi < imin))
        vmin, imin = np.where(take, ov, vmin), np.where(take, oi, imin)
        auc, tb = _f32(auc + auc[:, part]), _f32(tb + tb[:, part])
        ihit = np.minimum(ihit, ihit[:, part])
    for a in (vmax, imax, vmin, imin, auc, tb, ihit):
        assert np.all((a == a[:, :1]) | (a != a)), "every lane of the row holds the same values after the combine"
    return dict(vmax=vmax[:, 0], imax=imax[:, 0], vmin=vmin[:, 0], imin=imin[:, 0], auc=auc[:, 0], tb=tb[:, 0], ihit=ihit[:, 0])


def window_points(T_out, W, i0):
    """[(first global point, one past the last)] of the points each window walks: window 0 owns the points 0 .. W, window w > 0 the points
    n_lo + 1 .. n_hi, cut at i0; windows with no point at or beyond i0 are left out."""
    NS, out = T_out - 1, []
    W = NS if W <= 0 or W > NS else W
    for n_lo in range(0, NS, W):
        n_hi = min(n_lo + W, NS)
        lo = max(n_lo + (0 if n_lo == 0 else 1), i0)
        if lo <= n_hi:
            out.append((lo, n_hi + 1))
    return out


def restatement(v, times_out, i0, W, thr=None, sense=1):
    """The eight functionals [..., C, 8] fp32 of the curves v [..., C, T_out] fp32 in forecast_summary_kernel's order: the row walk per
    window on the points at or beyond i0, the windows merged in time order -- an extreme moves on strict improvement only and carries its
    time, auc and time_beyond add in window order starting from 0, the first hit stays.  thr [C] or None (slots 5 - 7 NaN)."""
    v = _f32(v)
    lead, Cn, T = v.shape[:-2], v.shape[-2], v.shape[-1]
    flat = v.reshape(-1, T)
    N = flat.shape[0]
    t, w = _f32(times_out), weights_from(times_out, i0)
    th = None if thr is None else np.broadcast_to(_f32(thr), lead + (Cn,)).reshape(-1)
    vmax, vmin = np.full(N, -np.inf, np.float32), np.full(N, np.inf, np.float32)
    tmax, tmin, thit = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
    auc, tb, hit = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, bool)
    for lo, hi in window_points(T, W, i0):
        r = row_walk(flat[:, lo:hi], w[lo:hi], th, sense)
        tw, n = t[lo:hi], hi - lo
        up = r["vmax"] > vmax
        vmax, tmax = np.where(up, r["vmax"], vmax), np.where(up, tw[np.minimum(r["imax"], n - 1)], tmax)
        dn = r["vmin"] < vmin
        vmin, tmin = np.where(dn, r["vmin"], vmin), np.where(dn, tw[np.minimum(r["imin"], n - 1)], tmin)
        auc, tb = _f32(auc + r["auc"]), _f32(tb + r["tb"])
        new = ~hit & (r["ihit"] < n)
        thit, hit = np.where(new, tw[np.minimum(r["ihit"], n - 1)], thit), hit | new
    nan = np.full(N, np.nan, np.float32)
    f = np.stack([vmax, tmax, vmin, tmin, auc] + ([nan, nan, nan] if thr is None else [tb, np.where(hit, thit, nan), hit.astype(np.float32)]), -1)
    return _f32(f).reshape(lead + (Cn, 8))
