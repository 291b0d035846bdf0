"""Test infrastructure of the curve summaries (slode_curve_summary): the numpy restatement of the eight functionals on given curves, the
moments over draws as the kernel accumulates them, the summation bars, the thresholds of the tests, the near points of a threshold and the
tolerant rules that hold the discontinuous slots to the fp64 oracle.  Not imported by the product.

Slots: 0 peak, 1 t_peak, 2 trough, 3 t_trough, 4 auc, 5 time_beyond, 6 t_hit, 7 crossed.

Bars.  Slots 0 - 3, 6, 7 and the p_beyond counts are comparisons and selections on the kernel's own fp32 curve values: exact, first index on
ties.  Slots 4 and 5 are sums of T terms in some fixed order: whatever the order, the result is within (T + 1) u sum |term| of the exact sum of
the fp32 terms (T - 1 additions and one rounding of every product; u = 2^-24) -- `sum_bars`.  Against the fp64 oracle a curve value is within
RU.MEAN_BAR max(1, |v|) (`bar`): an extreme is 1-Lipschitz in the sup norm, the area is (t_{T-1} - t_0)-Lipschitz, and a point counts as NEAR
the threshold when the oracle's value is within its bar of it -- only there may a comparison of the kernel's value differ from the oracle's."""
import numpy as np

from tests import calibration_util as CAL
from tests import cohort_util as CU
from tests import recon_moments_util as RU

NAMES = ("peak", "t_peak", "trough", "t_trough", "auc", "time_beyond", "t_hit", "crossed")
U = 2.0 ** -24
NEAR_SHARE = CAL.NEAR_SHARE
_f32 = RU._f32


def weights_f32(times):
    """The trapezoid node weights [T], formed in fp32 as the kernel forms them: 0.5 (t_{min(i+1, T-1)} - t_{max(i-1, 0)})."""
    t = _f32(times)
    i = np.arange(t.size)
    return _f32(np.float32(0.5) * _f32(t[np.minimum(i + 1, t.size - 1)] - t[np.maximum(i - 1, 0)]))


def weights_ends_not_halved(times):
    """A deliberately wrong table: the end weights are whole intervals (the summation bar must tell it from the right one)."""
    w = weights_f32(times).copy()
    w[0] *= 2
    w[-1] *= 2
    return w


def beyond(v, thr, sense):
    """v [..., C, T] against thr [C]: bool, false on NaN."""
    th = np.asarray(thr).reshape((-1, 1))
    return v > th if sense > 0 else v < th


def first_index(mask):
    """[...]: the smallest index along the last axis at which ``mask`` holds, T where none does."""
    T = mask.shape[-1]
    return np.where(mask, np.arange(T), T).min(-1)


def functionals(v, times, thr=None, sense=1, w=None):
    """The eight functionals [..., C, 8] (fp64) of the curves v [..., C, T] on their own values: extremes and first indices exactly; the
    two sums as the fp64 sum of the terms in the dtype of ``v`` (fp32 curves: the fp32 products w_i v_i)."""
    t = np.asarray(times, dtype=v.dtype)
    w = (weights_f32(times) if w is None else w).astype(v.dtype)
    T = v.shape[-1]
    f = np.full(v.shape[:-1] + (8,), np.nan)
    f[..., 0], f[..., 2] = v.max(-1), v.min(-1)
    f[..., 1] = t[first_index(v == v.max(-1, keepdims=True))]
    f[..., 3] = t[first_index(v == v.min(-1, keepdims=True))]
    f[..., 4] = (w * v).astype(v.dtype).astype(np.float64).sum(-1)
    if thr is not None:
        bd = beyond(v, np.asarray(thr, dtype=v.dtype), sense)
        ih = first_index(bd)
        f[..., 5] = np.where(bd, w, 0).astype(np.float64).sum(-1)
        f[..., 6] = np.where(ih < T, t[np.minimum(ih, T - 1)], np.nan)
        f[..., 7] = ih < T
    return f


def sum_bars(v, times, w=None):
    """(bar of auc [..., C], bar of time_beyond: a scalar): (T + 1) u sum |w_i v_i| and (T + 1) u sum w_i."""
    w = (weights_f32(times) if w is None else w).astype(np.float64)
    T = v.shape[-1]
    return (T + 1) * U * np.abs(w * v.astype(np.float64)).sum(-1), (T + 1) * U * np.abs(w).sum()


def draw_moments_f32(f):
    """f [ns, ..., 8] fp32, the per-draw functionals in draw order: (mean, sd) [..., 8] as the kernel accumulates them --
    RU.shifted_moments_f32 over all draws; slot 6 over the crossing draws alone (shifted by the first of them, divided by their count), NaN
    where none crosses."""
    f = _f32(f)
    mean, sd = RU.shifted_moments_f32(f)
    mean, sd = mean.copy(), sd.copy()
    hit = f[..., 7] == 1
    flat_f, flat_h = f[..., 6].reshape(f.shape[0], -1), hit.reshape(f.shape[0], -1)
    m6, s6 = np.full(flat_f.shape[1], np.nan, np.float32), np.full(flat_f.shape[1], np.nan, np.float32)
    for r in range(flat_f.shape[1]):
        vals = flat_f[flat_h[:, r], r]
        if vals.size:
            m6[r], s6[r] = RU.shifted_moments_f32(vals)
    mean[..., 6], sd[..., 6] = m6.reshape(mean.shape[:-1]), s6.reshape(sd.shape[:-1])
    return mean, sd


def oracle_moments(f64):
    """f64 [ns, ..., 8]: np.mean / np.std over the draws in fp64; slot 6 over the crossing draws (NaN where none)."""
    with np.errstate(invalid="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore")
        return np.nanmean(f64, 0), np.nanstd(f64, 0)


def bar(v):
    return RU.MEAN_BAR * np.maximum(1.0, np.abs(v))


def near(v64, thr):
    """bool like v64 [..., C, T]: the oracle's value is within its bar of thr[c]."""
    return np.abs(v64 - np.asarray(thr, dtype=np.float64).reshape((-1, 1))) <= bar(v64)


def thresholds(draws64):
    """thr [C] fp32: the median over draws, members and time of the oracle's head-0 curve of every channel (draws64 [Q, ns, B, C, T]):
    a level inside the curves' range."""
    return _f32(np.median(np.moveaxis(draws64[0], 2, 0).reshape(draws64.shape[3], -1), axis=1))


def oracle_draws(c, is_post, eps=None):
    return CU.oracle_draws(c, is_post, eps)


def tolerant_violations(got, v64, times, thr, sense):
    """The tolerant rules of the discontinuous slots for per-draw functionals ``got`` [..., C, 8] of the device against the oracle's curves
    v64 [..., C, T] of the same draws -- nothing excluded.  Returns the list of (rule, number of rows that break it):
      t_peak    a grid time at which the oracle's curve is within two bars of the oracle's maximum (t_trough likewise);
      t_hit     = t_j: no i < j has the oracle's value beyond thr by more than a bar, and v_j is not short of thr by more than a bar;
      crossed   equals the oracle's unless the row has a near point;
      time_beyond  within the sum of w_i over the row's near points plus the summation bar of sum_bars."""
    t64 = np.asarray(_f32(times), dtype=np.float64)
    w = weights_f32(times).astype(np.float64)
    T = v64.shape[-1]
    b = bar(v64)
    bad = []

    def index_of(tv):
        j = np.abs(tv[..., None] - t64).argmin(-1)
        return j, t64[j] == tv
    for slot, ext, sgn in ((1, v64.max(-1, keepdims=True), 1.0), (3, v64.min(-1, keepdims=True), -1.0)):
        j, on_grid = index_of(got[..., slot])
        vj = np.take_along_axis(v64, j[..., None], -1)
        ok = on_grid & ((sgn * (ext - vj))[..., 0] <= 2 * np.take_along_axis(b, j[..., None], -1)[..., 0])
        bad.append((NAMES[slot], int((~ok).sum())))
    if thr is not None:
        th = np.asarray(thr, dtype=np.float64).reshape((-1, 1))
        excess = (v64 - th) * (1.0 if sense > 0 else -1.0)          # > 0: beyond
        nr = near(v64, thr)
        o_cross = (excess > 0).any(-1)
        g_cross = got[..., 7] == 1
        bad.append(("crossed", int(((g_cross != o_cross) & ~nr.any(-1)).sum())))
        hit = got[..., 6]
        assert np.array_equal(np.isnan(hit), ~g_cross), "t_hit is NaN exactly where crossed is 0"
        j, on_grid = index_of(np.where(g_cross, hit, t64[0]))
        clearly = excess > b                                           # beyond by more than a bar
        earlier = (clearly & (np.arange(T) < j[..., None])).any(-1)
        short = np.take_along_axis(excess, j[..., None], -1)[..., 0] < -np.take_along_axis(b, j[..., None], -1)[..., 0]
        bad.append(("t_hit", int((g_cross & (~on_grid | earlier | short)).sum())))
        bad.append(("t_hit missed", int((~g_cross & clearly.any(-1)).sum())))
        o_tb = np.where(excess > 0, w, 0.0).sum(-1)
        slack = np.where(nr, w, 0.0).sum(-1) + (T + 1) * U * w.sum()
        bad.append(("time_beyond", int((np.abs(got[..., 5] - o_tb) > slack).sum())))
    return bad


def check_continuous(mean, sd, want_mean, want_sd, vmax, span, tag):
    """peak / trough mean within RU.MEAN_BAR max(1, |oracle|), their sd within RU.SD_BAR times the same; auc mean within span MEAN_BAR
    max(1, max |v|).  Prints the worst ratios, then asserts."""
    r = []
    for slot in (0, 2):
        scale = np.maximum(1.0, np.abs(want_mean[..., slot]))
        r.append(float((np.abs(mean[..., slot] - want_mean[..., slot]) / (RU.MEAN_BAR * scale)).max()))
        r.append(float((np.abs(sd[..., slot] - want_sd[..., slot]) / (RU.SD_BAR * scale)).max()))
    r.append(float((np.abs(mean[..., 4] - want_mean[..., 4]) / (span * RU.MEAN_BAR * np.maximum(1.0, vmax))).max()))
    print("%s: error / bar  peak mean %.3e sd %.3e  trough mean %.3e sd %.3e  auc mean %.3e" % ((tag,) + tuple(r)))
    assert max(r) <= 1.0, (tag, r)


def check_counts(p, ns, v64, thr, sense, tag):
    """p_beyond [..., C, T] of the device against the oracle's draws v64 [ns, ..., C, T]: the counts differ by at most the near draws of
    their cell and by nothing elsewhere; the near share is under NEAR_SHARE (a condition of the test, asserted)."""
    counts = np.rint(p.astype(np.float64) * ns)
    assert np.array_equal(_f32(counts) / np.float32(ns), p), (tag, "p_beyond is count / ns")
    nr = near(v64, thr)
    share = float(nr.mean())
    want = beyond(v64, np.asarray(thr, dtype=np.float64), sense).sum(0)
    print("%s: near share %.2e, cells that differ %d" % (tag, share, int((counts != want).sum())))
    assert share <= NEAR_SHARE, (tag, share)
    assert np.all(np.abs(counts - want) <= nr.sum(0)), tag
