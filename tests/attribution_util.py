"""Test infrastructure of the latent attribution (slode_latent_attribution): the blocks and arm masks per family, the seeded cases with
their two noise rows, the fp64 oracle -- the composition of tests/intervene_util.py::oracle_arms (encoder or conditional priors, decoder and
heads of oracle/slode_oracle.py through tests/recon_moments_util.py) with an arm's where(mask, e', e) noise in place of swapped labels -- the
bars, and the numpy restatement of the kernel's fma accumulation.  Not imported by the product.

Bars.  mean / sd of the base curve: RU.check, the project's per-value bar.  msd[a] = 1 / (2 ns) sum_k d_k^2 with d_k = v_a,k - v_k: both
arms of a draw each sit inside the per-value bar, so every difference carries an error |delta d| <= E = RU.MEAN_BAR (max(1, |mean_f|) +
max(1, |mean_a|)), and d^2 one of at most 2 |d| E + E^2; summed and halved: (1 / ns) sum_k (|d_k| E + E^2 / 2), the d_k taken from the
oracle.  To it the fp32 accumulation adds at most ns 2^-24 msd: ns fma roundings, each at most 2^-24 of a running sum that never exceeds
the final one (msd_f32 below, checked against fp64 on its own)."""
import numpy as np
import torch

from oracle import slode_oracle as O
from tests import eval_stats_util as EU
from tests import recon_moments_util as RU

FRESH_SEED = 47
U24 = 2.0 ** -24


def n_blocks(ospec):
    """Prior groups, plus the rest block when some latent dim lies in no group."""
    return len(ospec.prior_groups) + (1 if sum(g.z_dim for g in ospec.prior_groups) < ospec.latent_dim else 0)


def block_dims(ospec, mask):
    """bool [L]: the latent dims of the blocks of `mask` (bit g: prior group g; bit n_groups: the rest)."""
    sel, rest = np.zeros(ospec.latent_dim, dtype=bool), np.ones(ospec.latent_dim, dtype=bool)
    for g, gr in enumerate(ospec.prior_groups):
        rest[gr.z_off:gr.z_off + gr.z_dim] = False
        if (mask >> g) & 1:
            sel[gr.z_off:gr.z_off + gr.z_dim] = True
    if (mask >> len(ospec.prior_groups)) & 1:
        sel |= rest
    return sel


def arm_masks(ospec):
    """(masks, single, complement): every single block and every complement of one, equal masks once; per block the index of its two arms."""
    P = n_blocks(ospec)
    every = (1 << P) - 1
    masks, single, comp = [], [], []
    for p in range(P):
        for m, idx in ((1 << p, single), (every ^ (1 << p), comp)):
            if m not in masks:
                masks.append(m)
            idx.append(masks.index(m))
    return masks, single, comp


def build(case, solver="rk4", B=None, ns=7):
    """RU.build's case with ``eps2`` [2, ns, B, L]: its own noise as the base rows, a second seeded draw as the fresh rows."""
    c = RU.build(case, solver, B, ns)
    fresh = torch.randn(c["eps"].shape, generator=torch.Generator().manual_seed(FRESH_SEED + ns))
    c["eps2"] = torch.stack([c["eps"], fresh])
    return c


def oracle_arms(c, is_post, masks, eps2=None):
    """(v, [v_a for a in masks]), each [Q, ns, B, C, T] fp64 numpy: the base curves and every arm's, on the same two noise rows."""
    ospec, p64 = c["ospec"], EU.f64(c["p"])
    obs, u, times = c["obs"].double(), c["u"].double(), c["times"].double()
    e2 = (c["eps2"] if eps2 is None else eps2).double()
    _, ns, B, L = e2.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p64, obs, ospec.pool_size) if is_post else O.prior_loc_scale(p64, ospec, u)

        def curves(e):
            z = (loc.unsqueeze(0) + scale.unsqueeze(0) * e).reshape(ns * B, L)
            mu = RU.oracle_curves(p64, ospec, z, times, ospec.solver)
            return mu.reshape(mu.shape[0], ns, B, mu.shape[2], mu.shape[3]).numpy()
        base = curves(e2[0])
        arms = [curves(torch.where(torch.from_numpy(block_dims(ospec, m)), e2[1], e2[0])) for m in masks]
    return base, arms


def msd64(v, va):
    return 0.5 * np.mean((va - v) ** 2, 1)


def msd_bar(v, va):
    """The bar of msd (module docstring) from the oracle's curves of both arms, [Q, B, C, T]."""
    ns = v.shape[1]
    E = RU.MEAN_BAR * (np.maximum(1.0, np.abs(np.mean(v, 1))) + np.maximum(1.0, np.abs(np.mean(va, 1))))
    return np.mean(np.abs(va - v) * E[:, None] + 0.5 * E[:, None] ** 2, 1) + ns * U24 * msd64(v, va)


def oracle_moments(c, is_post, masks, eps2=None):
    """dict(mean, sd [Q, B, C, T]; msd, bar [A, Q, B, C, T]) in fp64."""
    v, arms = oracle_arms(c, is_post, masks, eps2)
    return dict(mean=np.mean(v, 1), sd=np.std(v, 1), msd=np.stack([msd64(v, a) for a in arms]), bar=np.stack([msd_bar(v, a) for a in arms]))


def indices(var, total, first):
    """(total_index, first_index) [..., C] in fp64: sum_t / sum_t var, NaN where the curve has no variance."""
    den = var.sum(-1)
    den = np.where(den == 0, np.nan, den)
    return total.sum(-1) / den, first.sum(-1) / den


def _np(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def check(got, want, tag):
    """got = (mean, sd, msd); prints the worst ratios error / bar, asserts RU's two bars and the msd bar.  Returns the msd ratio."""
    mean, sd, msd = got
    RU.check(mean, sd, want["mean"], want["sd"], tag + " base")
    m = _np(msd)
    assert m.shape == want["msd"].shape and np.isfinite(m).all(), (tag, "msd not finite / not written")
    r = float((np.abs(m - want["msd"]) / want["bar"]).max())
    print("%s: msd error / bar %.3e (largest msd %.3e)" % (tag, r, float(want["msd"].max())))
    assert r <= 1.0, (tag, "msd", r)
    return r


# ---- the accumulation of attribution_kernel (phases M6 / M7), operation by operation in fp32 ---------------------------------------------
def msd_f32(v, va):
    """v, va [ns, ...] fp32, draws in the order k = 0 .. ns - 1: d = fl(v_a - v); s = fma(d, d, s) from s = 0; msd = fl(fl(0.5 s) fl(1 / ns))."""
    v, va = np.asarray(v, dtype=np.float32), np.asarray(va, dtype=np.float32)
    ns = v.shape[0]
    s = np.zeros_like(v[0])
    for k in range(ns):
        d = (va[k] - v[k]).astype(np.float32)
        s = RU._fma32(d, d, s)
    inv = np.float32(1.0) / np.float32(ns)
    return ((np.float32(0.5) * s).astype(np.float32) * inv).astype(np.float32)
