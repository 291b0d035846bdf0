"""Test infrastructure of the sample moments of the reconstruction (slode_recon_moments): the numpy restatement of the kernel's
accumulation, the seeded cases (those of tests/eval_stats_util.py at any B) and the fp64 oracle's moments -- encoder / conditional
priors, decoder and heads of oracle/slode_oracle.py composed here, then mean and std(ddof = 0) over the draws.  Not imported by the
product."""
import numpy as np
import torch

from oracle import slode_oracle as O
from tests import eval_stats_util as EU

NOISE_SEED = 31
MEAN_BAR, SD_BAR = 1e-4, 2e-4     # x max(1, |oracle mean curve|): the per-value bar of the head curves, and twice it (module docstring of the GPU test)


# ---- the accumulation of recon_moments_kernel (phases M6 / M7), operation by operation in fp32 ---------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64; one rounding of the fp64 sum, then to fp32."""
    return _f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def shifted_moments_f32(vals):
    """vals [ns, ...] fp32, draws in the order k = 0 .. ns - 1: v0 = vals[0]; s1 += v - v0; s2 = fma(dv, dv, s2);
    mean = fma(s1, 1 / ns, v0); sd = sqrt(max(s2 - s1 * s1 / ns, 0) / ns)."""
    vals = _f32(vals)
    ns = vals.shape[0]
    v0 = vals[0]
    s1, s2 = np.zeros_like(v0), np.zeros_like(v0)
    for k in range(1, ns):
        dv = _f32(vals[k] - v0)
        s1 = _f32(s1 + dv)
        s2 = _fma32(dv, dv, s2)
    inv = np.float32(1.0) / np.float32(ns)
    mean = _fma32(s1, np.broadcast_to(inv, s1.shape), v0)
    var = _f32(np.maximum(_f32(s2 - _f32(_f32(s1 * s1) * inv)), np.float32(0.0)) * inv)
    return mean, _f32(np.sqrt(var))


def plain_moments_f32(vals):
    """The form the kernel does NOT use: fp32 sums of v and v^2, var = E[v^2] - E[v]^2."""
    vals = _f32(vals)
    ns = vals.shape[0]
    s1, s2 = np.zeros_like(vals[0]), np.zeros_like(vals[0])
    for k in range(ns):
        s1 = _f32(s1 + vals[k])
        s2 = _fma32(vals[k], vals[k], s2)
    inv = np.float32(1.0) / np.float32(ns)
    mean = _f32(s1 * inv)
    return mean, _f32(np.sqrt(np.maximum(_f32(_f32(s2 * inv) - _f32(mean * mean)), np.float32(0.0))))


SPREAD = 10.0     # condition of accumulation_bars: no draw further than this many sd from the first draw


def accumulation_bars(mean64, sd64, ns):
    """Worst-case rounding bounds of the shifted form, u = 2^-24, n = ns, for draws with D = max_k |v_k - v0| <= SPREAD sd (asserted by the
    caller).  The inputs are exact fp32 values, so the only errors are those of the accumulation:
      d_k = fl(v_k - v0): |error| <= u D;  s1: n - 1 additions, |error| <= n u sum|d_k| <= n^2 u D;  s2 likewise <= (n + 2) u n D^2.
      mean = fl(v0 + s1 / n): <= u |mean| + (n + 1) u D                                   -> bar u |mean| + SPREAD (n + 1) u sd
      var = (s2 - s1^2 / n) / n: <= [(n + 2) n + 2 n^2] u D^2 / n <= 3 (n + 1) u D^2;  sd error = var error / (2 sd)
                                                                                          -> bar 1.5 SPREAD^2 (n + 1) u sd
    Neither sd bound has a term in |mean|: that is the point of the shift."""
    u = 2.0 ** -24
    return u * np.abs(mean64) + SPREAD * (ns + 1) * u * sd64, 1.5 * SPREAD ** 2 * (ns + 1) * u * sd64


# ---- seeded cases and the fp64 oracle ------------------------------------------------------------------------------------------------
def build(case, solver="rk4", B=None, ns=7):
    """EU.build_case's parameters (the label heads not moved: no curve reads them) and synthetic batch at any B, and [ns, B, L] noise."""
    return dict(EU.build_case(case, ("eps", ns, NOISE_SEED + ns), solver, B, jitter_heads=False), ns=ns)


def oracle_curves(p64, ospec, z, times, solver):
    """[Q, N, C, T] in the engine's head order: mu_50, mu_75, mu_25 (ALD) or mean (Gauss)."""
    if ospec.gauss:
        return torch.stack([O.decoder_gauss(p64, z, times, solver)[1]])
    _, mu75, mu50, mu25, _ = O.decoder_ald(p64, z, times, solver)
    return torch.stack([mu50, mu75, mu25])


def oracle_moments(c, is_post, eps=None):
    """(mean, sd) [Q, B, C, T] in fp64: z = loc + scale * eps_k for every draw, the oracle's curves, np.mean / np.std over the draws."""
    ospec, p64 = c["ospec"], EU.f64(c["p"])
    obs, u, times = c["obs"].double(), c["u"].double(), c["times"].double()
    e = (c["eps"] if eps is None else eps).double()
    ns, B, L = e.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p64, obs, ospec.pool_size) if is_post else O.prior_loc_scale(p64, ospec, u)
        z = (loc.unsqueeze(0) + scale.unsqueeze(0) * e).reshape(ns * B, L)
        mu = oracle_curves(p64, ospec, z, times, ospec.solver)
    mu = mu.reshape(mu.shape[0], ns, B, mu.shape[2], mu.shape[3]).numpy()
    return np.mean(mu, 1), np.std(mu, 1)


def check(mean, sd, want_mean, want_sd, tag):
    """Prints the worst ratios error / bar, then asserts both bars."""
    m, s = mean.detach().double().cpu().numpy(), sd.detach().double().cpu().numpy()
    scale = np.maximum(1.0, np.abs(want_mean))
    rm, rs = float((np.abs(m - want_mean) / (MEAN_BAR * scale)).max()), float((np.abs(s - want_sd) / (SD_BAR * scale)).max())
    print("%s: mean error / bar %.3e, sd error / bar %.3e (largest sd %.3e)" % (tag, rm, rs, float(want_sd.max())))
    assert np.isfinite(m).all() and np.isfinite(s).all(), tag
    assert rm <= 1.0, (tag, "mean", rm)
    assert rs <= 1.0, (tag, "sd", rs)
