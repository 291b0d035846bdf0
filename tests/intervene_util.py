"""Test infrastructure of the counterfactual curves (slode_intervene_moments): the counterfactual labels, the masks per family, the fp64
oracle -- encoder, conditional priors on the swapped labels, the group offsets of spec.prior_groups, decoder and heads of
oracle/slode_oracle.py composed through tests/recon_moments_util.py, then np.mean / np.std over the draws of v_cf and of v_cf - v_f -- the
bars, and the numpy restatement of the kernel's two shifted accumulations.  Not imported by the product.

Bars.  cf: the project's per-value bar, RU.MEAN_BAR / RU.SD_BAR x max(1, |oracle cf mean|), as RU.check.  The effect is a difference of two
values that each sit inside that bar, so its error is at most the sum of the two: eff_mean within
RU.MEAN_BAR (max(1, |mean_f|) + max(1, |mean_cf|)), eff_sd within RU.SD_BAR times the same sum."""
import numpy as np
import torch

from oracle import slode_oracle as O
from tests import eval_stats_util as EU
from tests import recon_moments_util as RU

# family -> [(tag, group_mask, label columns that take the counterfactual value (None: all))]: each single prior group, all groups; proc
# (one prior group over all four labels) also with the pair {C12, C6} alone swapped
MASKS = {
    "cvs": [("iext", 1, None), ("rtpr", 2, None), ("all", 3, None)],
    "challenge": [("all", 1, None)],
    "proc": [("all", 1, None), ("C12+C6", 1, (7, 8))],
}


def cf_labels(u, cols=None):
    """The batch's own labels rolled by one row (one-hot columns stay one-hot); with `cols`, only those columns."""
    r = torch.roll(u, 1, 0)
    if cols is None:
        return r
    out = u.clone()
    out[:, list(cols)] = r[:, list(cols)]
    return out


def group_columns(ospec, mask):
    """Label columns read by the groups of `mask`."""
    return sorted(q for g, gr in enumerate(ospec.prior_groups) if (mask >> g) & 1 for q in range(gr.u_off, gr.u_off + gr.u_dim))


def oracle_arms(c, mask, u_cf, eps=None):
    """(v_f, v_cf), each [Q, ns, B, C, T] fp64 numpy: both arms of every draw on ONE noise row."""
    ospec, p64 = c["ospec"], EU.f64(c["p"])
    obs, times = c["obs"].double(), c["times"].double()
    e = (c["eps"] if eps is None else eps).double()
    ns, B, L = e.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p64, obs, ospec.pool_size)
        cloc, cscale = loc.clone(), scale.clone()
        ploc, pscale = O.prior_loc_scale(p64, ospec, u_cf.double())
        for g, gr in enumerate(ospec.prior_groups):
            if (mask >> g) & 1:
                sl = slice(gr.z_off, gr.z_off + gr.z_dim)
                cloc[:, sl], cscale[:, sl] = ploc[:, sl], pscale[:, sl]
        arms = []
        for lo, sc in ((loc, scale), (cloc, cscale)):
            z = (lo.unsqueeze(0) + sc.unsqueeze(0) * e).reshape(ns * B, L)
            mu = RU.oracle_curves(p64, ospec, z, times, ospec.solver)
            arms.append(mu.reshape(mu.shape[0], ns, B, mu.shape[2], mu.shape[3]).numpy())
    return arms[0], arms[1]


def oracle_moments(c, mask, u_cf, eps=None):
    """dict(cf_mean, cf_sd, eff_mean, eff_sd, f_mean, f_sd), [Q, B, C, T] fp64."""
    vf, vcf = oracle_arms(c, mask, u_cf, eps)
    d = vcf - vf
    return dict(cf_mean=np.mean(vcf, 1), cf_sd=np.std(vcf, 1), eff_mean=np.mean(d, 1), eff_sd=np.std(d, 1), f_mean=np.mean(vf, 1), f_sd=np.std(vf, 1))


def effect_scale(f_mean, cf_mean):
    return np.maximum(1.0, np.abs(f_mean)) + np.maximum(1.0, np.abs(cf_mean))


def _np(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def check(got, want, tag):
    """got = (cf_mean, cf_sd, eff_mean, eff_sd); prints the worst ratios error / bar, then asserts the four bars."""
    cm, cs, em, es = (_np(t) for t in got)
    for a in (cm, cs, em, es):
        assert np.isfinite(a).all(), (tag, "not finite / not written")
    s_cf = np.maximum(1.0, np.abs(want["cf_mean"]))
    s_eff = effect_scale(want["f_mean"], want["cf_mean"])
    r = (float((np.abs(cm - want["cf_mean"]) / (RU.MEAN_BAR * s_cf)).max()), float((np.abs(cs - want["cf_sd"]) / (RU.SD_BAR * s_cf)).max()),
         float((np.abs(em - want["eff_mean"]) / (RU.MEAN_BAR * s_eff)).max()), float((np.abs(es - want["eff_sd"]) / (RU.SD_BAR * s_eff)).max()))
    print("%s: error / bar: cf mean %.3e, cf sd %.3e, effect mean %.3e, effect sd %.3e (largest |effect mean| %.3e, effect sd %.3e)"
          % ((tag,) + r + (float(np.abs(want["eff_mean"]).max()), float(want["eff_sd"].max()))))
    for name, v in zip(("cf mean", "cf sd", "effect mean", "effect sd"), r):
        assert v <= 1.0, (tag, name, v)


def paired_moments_f32(vf, vcf):
    """The kernel's two accumulations (phases M6 / M7), operation by operation in fp32: the shifted moments of v_cf and those of
    e_k = fl(v_cf_k - v_f_k), draws in the order k = 0 .. ns - 1.  Returns (cf_mean, cf_sd, eff_mean, eff_sd)."""
    vf, vcf = np.asarray(vf, dtype=np.float32), np.asarray(vcf, dtype=np.float32)
    return RU.shifted_moments_f32(vcf) + RU.shifted_moments_f32((vcf - vf).astype(np.float32))
