"""Test infrastructure of the counterfactual summaries (slode_intervene_summary): the hypothesis tables of the tests, the fp64 truth composed
from tests/intervene_util.py (oracle_arms, once per hypothesis row) and tests/summary_util.py (functionals), the two thresholds, and the numpy
restatement of the kernel's three accumulations.  Not imported by the product.

Hypotheses.  Rows 0 .. V - 1 of the batch's own labels over every label column (every prior group intervened): hypothesis v gives every
trajectory the labels of trajectory v.

Thresholds, per channel, over the factual arm and all counterfactual arms pooled (head curve 0):
  (a) "median": the median of the curve values -- nearly every draw crosses it (summary_util.thresholds' rule on the pooled curves);
  (b) "peaks":  the median of the per-curve peaks -- about half of the draws cross it, and crossing differs between arms.
A point is NEAR a threshold when the oracle's value is within its bar of it (summary_util.near); the tests assert that the near share stays
under summary_util.NEAR_SHARE in every arm.

Bars against the oracle.  factual and cf are curve summaries: summary_util's rules unchanged.  An effect is a difference of two values that
each sit inside their bar, so its error is at most the SUM of the two arms' bars (as tests/intervene_util.py derives for curves); effect sds
within twice that.  The effect on `crossed` is a difference of two shares of draws, each off by at most the near draws of its cell."""
import numpy as np
import torch

from tests import intervene_util as IU
from tests import recon_moments_util as RU
from tests import summary_util as SU

_f32 = RU._f32
V = 3
FAMILY_MASK = {"cvs": 3, "challenge": 1, "proc": 1}        # every prior group of the family


def hypothesis_rows(c, V=V, rows=None):
    """[V, n_u] fp32: the label rows of trajectories ``rows`` (default 0 .. V - 1) of the case's batch."""
    rows = list(range(V)) if rows is None else list(rows)
    return c["u"][rows].clone().to(torch.float32)


def oracle(c, hyp_u, mask):
    """(v_f [Q, ns, B, C, T], v_cf [V, Q, ns, B, C, T]) fp64: IU.oracle_arms once per hypothesis row, that row given to every trajectory."""
    B = c["B"]
    vf, arms = None, []
    for v in range(hyp_u.shape[0]):
        f, cf = IU.oracle_arms(c, mask, hyp_u[v:v + 1].expand(B, -1).contiguous())
        vf = f if vf is None else vf
        arms.append(cf)
    return vf, np.stack(arms)


def thresholds(vf, vcf, kind):
    """thr [C] fp32 from head curve 0 of the factual arm and all arms pooled ([*, ns, B, C, T]): "median" of the values, "peaks": the
    median of the per-curve maxima."""
    pool = np.concatenate([vf[0][None], vcf[:, 0]], 0)                                    # [1 + V, ns, B, C, T]
    Cn = pool.shape[3]
    per_c = np.moveaxis(pool, 3, 0)                                                        # [C, 1 + V, ns, B, T]
    if kind == "median":
        return _f32(np.median(per_c.reshape(Cn, -1), axis=1))
    return _f32(np.median(per_c.max(-1).reshape(Cn, -1), axis=1))


def functionals64(vf, vcf, times, thr, sense):
    """(f_f [ns, Q, B, C, 8], f_v [V, ns, Q, B, C, 8]) fp64 of the oracle's curves."""
    th = None if thr is None else np.asarray(thr, np.float64)
    ff = SU.functionals(np.moveaxis(vf, 1, 0), times, th, sense)
    fv = np.stack([SU.functionals(np.moveaxis(a, 1, 0), times, th, sense) for a in vcf])
    return ff, fv


def effect64(ff, fv):
    """The paired differences [ns, ..., 8] fp64: slot 6 NaN unless both arms cross (NaN - x = NaN)."""
    return fv - ff


def oracle_moments(ff, fv):
    """dict of (mean, sd) fp64: "f" [Q, B, C, 8], "cf" and "eff" [V, Q, B, C, 8] (np.nanmean / np.nanstd over the draws)."""
    return dict(f=SU.oracle_moments(ff), cf=tuple(np.stack(x) for x in zip(*[SU.oracle_moments(a) for a in fv])),
                eff=tuple(np.stack(x) for x in zip(*[SU.oracle_moments(effect64(ff, a)) for a in fv])))


def effect_moments_f32(ff, fv):
    """The kernel's effect accumulation, operation by operation in fp32: ff, fv [ns, ..., 8] fp32 per-draw functionals of the two arms in
    draw order (slot 7 in {0, 1}; slot 6 of a draw that does not cross: anything); e = fl(f_v - f_f); slots 0 - 5 and 7 over all draws
    (RU.shifted_moments_f32), slot 6 over the draws that cross in BOTH arms, shifted by the first of them and divided by their count,
    NaN where there is none."""
    ff, fv = _f32(ff), _f32(fv)
    e = _f32(np.where(np.isnan(fv) | np.isnan(ff), np.float32(0), fv) - np.where(np.isnan(ff) | np.isnan(fv), np.float32(0), ff))
    mean, sd = RU.shifted_moments_f32(e)
    mean, sd = mean.copy(), sd.copy()
    both = (ff[..., 7] == 1) & (fv[..., 7] == 1)
    flat_e, flat_b = e[..., 6].reshape(e.shape[0], -1), both.reshape(e.shape[0], -1)
    m6, s6 = np.full(flat_e.shape[1], np.nan, np.float32), np.full(flat_e.shape[1], np.nan, np.float32)
    for r in range(flat_e.shape[1]):
        vals = flat_e[flat_b[:, r], r]
        if vals.size:
            m6[r], s6[r] = RU.shifted_moments_f32(vals)
    mean[..., 6], sd[..., 6] = m6.reshape(mean.shape[:-1]), s6.reshape(sd.shape[:-1])
    return mean, sd


def restatement_f32(ff, fv):
    """dict of (mean, sd) fp32 as the kernel accumulates them from the per-draw rows ff [ns, Q, B, C, 8], fv [V, ns, Q, B, C, 8]."""
    return dict(f=SU.draw_moments_f32(ff), cf=tuple(np.stack(x) for x in zip(*[SU.draw_moments_f32(a) for a in fv])),
                eff=tuple(np.stack(x) for x in zip(*[effect_moments_f32(ff, a) for a in fv])))


def near_share(vf, vcf, thr):
    """The largest share of points within one bar of the threshold over the arms (factual, then every hypothesis)."""
    return max([float(SU.near(vf, thr).mean())] + [float(SU.near(a, thr).mean()) for a in vcf])


def check_effect(eff_mean, eff_sd, want, ff64, fv64, vf, vcf, times, thr, ns, tag):
    """The effect set of the device against the oracle: means of peak, trough and auc within the SUM of the two arms' bars (peak / trough:
    RU.MEAN_BAR max(1, |oracle mean|) per arm; auc: span RU.MEAN_BAR max(1, max |v|) per arm), their sds within twice that; the effect on
    `crossed` off by at most the near draws of the cell in either arm over ns.  Prints the worst ratios, then asserts."""
    span = float(times[-1] - times[0])
    fm = SU.oracle_moments(ff64)[0]                                                        # [Q, B, C, 8] (NaN: slot 6 of a cell no draw crosses)
    r = []
    for v in range(vcf.shape[0]):
        cm = SU.oracle_moments(fv64[v])[0]
        for slot in (0, 2):
            bar = RU.MEAN_BAR * (np.maximum(1.0, np.abs(fm[..., slot])) + np.maximum(1.0, np.abs(cm[..., slot])))
            r.append(float((np.abs(eff_mean[v][..., slot] - want[0][v][..., slot]) / bar).max()))
            r.append(float((np.abs(eff_sd[v][..., slot] - want[1][v][..., slot]) / (2 * bar)).max()))
        bar = span * RU.MEAN_BAR * (np.maximum(1.0, np.abs(vf).max(-1).max(1)) + np.maximum(1.0, np.abs(vcf[v]).max(-1).max(1)))
        r.append(float((np.abs(eff_mean[v][..., 4] - want[0][v][..., 4]) / bar).max()))
        r.append(float((np.abs(eff_sd[v][..., 4] - want[1][v][..., 4]) / (2 * bar)).max()))
        if thr is not None:
            nr = SU.near(np.moveaxis(vf, 1, 0), thr).any(-1).sum(0) + SU.near(np.moveaxis(vcf[v], 1, 0), thr).any(-1).sum(0)
            assert np.all(np.abs(eff_mean[v][..., 7] - want[0][v][..., 7]) <= nr / ns + 1e-6), (tag, v, "crossed")
    print("%s: effect error / bar, worst %.3e" % (tag, max(r)))
    assert max(r) <= 1.0, (tag, r)
