"""Test infrastructure of tests/test_regimes_cpu.py and tests/test_gpu_regimes.py: the suite's seeded cases moved away from the
initialisation -- REGIMES, pure CPU transformations (ospec, p, obs, u, eps, times) -> (p, obs) built from fixed constants and seeded CPU
generators, so that a case is reproducible from its name -- and the comparison helpers: the fp64 oracle and the fp32 CPU oracle of a
case, the per-tensor distances, and the bars derived from them.  Not imported by the product.

Every other parity test perturbs O.init_params by 0.05 randn and reads O.synthetic_batch: the likelihood scale is softplus(0.01 +- 0.05)
= 0.70, the posterior and prior scales are about 1, the observations lie in [0, 1] and never equal their prediction.  The regimes:
  tight_noise       decoder.constant_std[c, t] = linspace(-7, 2, C T) laid out t-major (every channel sees the whole range), then column
                    t = 0 set to 19.5 and column t = 1 to 20.5 (the two sides of softplus's x > 20 branch); proc's constant_std_C_12 /
                    constant_std_C_6 set to -3.  Likelihood scales 9e-4 .. 20.5.
  posterior_scales  encoder.z_scale.0.bias += linspace(-7, 1.5, L): posterior scales about 1e-3 .. 13 across the latent dimensions.
  prior_scales      per prior group: ...sequential_mlp.1.1.0.bias += linspace(-4, 3, z_dim), ...1.0.0.bias += linspace(-3, 3, z_dim).
  trained_weights   every decoder.ode_model.*weight x 3, encoder.lin.weight x 4 (tanh saturates), encoder.z_loc.weight x 3.
  raw_units         obs = 12 obs - 4 (negative and far outside the unit interval), layout kept.
  ties              row 0 of every decoder.output_*.0.weight zeroed: channel 0's prediction is exactly +0.0 in any precision and summation
                    order; obs[:, 0, ::3] = 0.0, obs[:, 0, 1::6] = -0.0.  The quantile weight of a tie is tau (obs >= mu), the residual's
                    sign 0, the row-0 head gradient of a tie exactly 0.  A Gauss family gets zero residuals.
  fitted            tight_noise, then obs = mu_50 (or mean) of the fp64 oracle at this eps + min(std, 0.5) x Laplace(0, 1) noise (inverse cdf
                    of a seeded uniform clamped to [1e-6, 1 - 1e-6]), cast to fp32, in the case's layout: residuals of the order of a small
                    scale, as training produces.  The prediction depends on the observations through the encoder, so one pass leaves the
                    median residual at 1 .. 24 scales (the curves reach O(100)); the construction is applied FITTED_PASSES = 4 times with
                    the same noise, each pass reading the observations of the one before: the fewest passes that bring the median residual
                    of every case under 2 scales (3 passes: up to 2.2; 4: 0.5 .. 1.3).  A converged fit would put about 1.2 % of the elements
                    within the kink margin (P(|scale x Laplace| < 1e-4) over scales down to 9e-4); at 4 passes clear_of_kinks moves 0 .. 0.8 %.
  all               tight_noise, posterior_scales, prior_scales, trained_weights, raw_units composed in that order.
After the regime every observation that is not a constructed tie goes through full_size_util.clear_of_kinks (margin 1e-4: the quantile
likelihood's gradient jumps at a tie, so two correct fp32 summation orders may land on different sides); it may move at most 1 % of a case
(`apply` records the count; ties: channel 0 is exempt, its ties are exact by construction).

Bars (the project's rule, as in tests/mechanism_util.py and tests/test_gpu_eval_side.py): a quantity's bar is the suite's bar for that kind
of value -- -ELBO 1e-5 relative, a gradient tensor 5e-4 norm-wise (a tensor that is zero on the oracle must come back exactly zero), encoder
loc / scale 2e-5, trajectories 1e-5 max(1, |x|), small nets 1e-6 .. 2e-6, a per-row loss 1e-5 x mag (tests/traj_bounds_util.py) -- unless
4 x the distance of the fp32 CPU oracle from the fp64 oracle on that case and that tensor, scaled the same way, exceeds it: the bar is then
that larger figure (`bar`).  The fp32 distance is computed in the test, per case and per tensor (`Oracles`); no bar comes from a kernel's
output.

The fp32 oracle's distances (`fp32_row` is one line per case; tests/test_regimes_cpu.py runs it on every case, prints the rows and asserts
what is said here).  Worst over the five compiled shapes (c0, c1, c2, c4, ref of tests/test_gpu_instantiations.SHAPES) at B = 12, exact mode;
loss relative, gradients norm-wise per tensor, the worst tensor; "x": a bar the rule raised:
  regime            main loss       main gradient, worst tensor                              bar      aux loss       aux gradient, worst tensor       bar
  tight_noise       2.0e-07 (c1)    9.4e-07 (c0 decoder.output_q25.0.weight)                 5.0e-04  1.1e-07 (c1)   1.4e-06 (c0 q_rtpr ...3.bias)    5.0e-04
  posterior_scales  4.4e-07 (c4)    8.1e-07 (c4 ...dynamics_hidden.weight)                   5.0e-04  2.6e-07 (c1)   4.3e-04 (c0 encoder.z_loc.bias)  1.7e-03 x
  prior_scales      2.1e-07 (c2)    2.4e-06 (c2 encoder.z_scale.0.bias)                      5.0e-04  1.1e-07 (c1)   1.4e-06 (c0 q_rtpr ...3.bias)    5.0e-04
  trained_weights   5.3e-07 (c2)    1.9e-05 (c4 ...dyanmics_degradation.weight)              5.0e-04  9.2e-08 (c4)   2.0e-06 (c0 encoder.z_loc.weight) 5.0e-04
  raw_units         2.5e-07 (c4)    6.6e-06 (c4 encoder.conv.weight)                         5.0e-04  4.4e-08 (c0)   2.9e-06 (c4 encoder.lin.weight)  5.0e-04
  ties              3.0e-07 (c4)    1.0e-06 (c2 encoder.z_scale.0.bias)                      5.0e-04  8.5e-08 (ref)  1.1e-06 (c1 q_rtpr ...1.module.weight) 5.0e-04
  fitted            1.7e-06 (c4)    4.5e-03 (c4 decoder.ode_model.latent_to_ode_net.2.bias)  1.8e-02 x 1.2e-07 (c0)  2.4e-05 (c4 encoder.conv.bias)   5.0e-04
  all               4.6e-07 (c4)    3.3e-05 (c4 ...dyanmics_degradation.weight)              5.0e-04  5.6e-07 (c1)   6.5e-04 (c0 encoder.z_loc.bias)  2.6e-03 x
Every loss bar is the suite's 1e-5.  Raised gradient bars, all of them: c0's auxiliary loss at posterior_scales and all (encoder.z_loc.*:
d/d loc of log N(loc + scale eps; loc, scale) cancels to zero between terms of size 1 / scale = 1e3) and c4's main loss at fitted (a Gauss
likelihood with scales down to 1e-3 fitted to curves that reach 300: one fp32 ulp of the curve is a thirtieth of the scale).  The block of
decoder.constant_std with a raw value below -4: 9.8e-8 .. 2.5e-7 (bar 5e-4), c4 fitted 1.4e-4 (bar 5.6e-4).
Per-row losses of the bounds cases (six model classes, B = 4, K = 3, rk4; `bounds_oracles`), fp32 oracle's worst distance / the suite's
per-row bar: at most 0.34, except challenge_gauss at trained_weights 1.00 and all 1.31 (bars x 4.0 and x 5.3) and the fitted Gauss rows,
cvs_gauss 7.7 and challenge_gauss 34 (bars x 31 and x 137; the conditioning of c4 fitted, row by row).
What a regime reaches (`reach`; these and the bounds cases): likelihood scales 9.7e-4 .. 20.5; posterior scale ratios 4.0e3 .. 5.6e4; prior
scale ratios 2.0e3 .. 5.9e6 (c0's prior groups have one dimension each: no spread, the scale moves to e^-4 of its own); share of encoder
units with |tanh| > 0.99 at trained_weights 0.45 .. 0.73 (0.89 .. 0.97 at all), largest state 1.009 .. 300; 528 .. 1800 exact ties per
case, the same in both precisions; fitted: median residual 0.5 .. 1.3 scales.
"""
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

from oracle import slode_oracle as O
from tests import full_size_util as U
from tests import traj_bounds_util as TU

LOSS_BAR, GRAD_BAR = 1e-5, 5e-4
KINK_MARGIN, KINK_SHARE = 1e-4, 0.01
FITTED_SEED = 101
FITTED_PASSES = 4           # the encoder reads the observations: see `fitted` in the module docstring
SMALL_STD_RAW = -4.0        # the sub-block of decoder.constant_std compared on its own (tight_noise, fitted): raw value below this


# ---- the regimes ---------------------------------------------------------------------------------------------------------------------------
def _relaid(new, like):
    """``new`` [B, C, T] in the dense layout of ``like``: contiguous, or the [B,C,T] view of a contiguous [B,T,C] tensor."""
    new = new.to(like.dtype)
    return new.contiguous() if like.is_contiguous() else new.permute(0, 2, 1).contiguous().permute(0, 2, 1)


def _one_draw(eps):
    return eps[0] if eps.dim() == 3 else eps


def tight_noise(ospec, p, obs, u, eps, times):
    p = dict(p)
    C, T = p["decoder.constant_std"].shape
    cs = torch.linspace(-7.0, 2.0, C * T).reshape(T, C).t().contiguous()
    cs[:, 0], cs[:, 1] = 19.5, 20.5
    p["decoder.constant_std"] = cs
    for k in ("constant_std_C_12", "constant_std_C_6"):
        if k in p:
            p[k] = torch.full_like(p[k], -3.0)
    return p, obs


def posterior_scales(ospec, p, obs, u, eps, times):
    p = dict(p)
    k = "encoder.z_scale.0.bias"
    p[k] = p[k] + torch.linspace(-7.0, 1.5, p[k].numel())
    return p, obs


def prior_scales(ospec, p, obs, u, eps, times):
    p = dict(p)
    for g in ospec.prior_groups:
        ks, kl = g.prefix + "sequential_mlp.1.1.0.bias", g.prefix + "sequential_mlp.1.0.0.bias"
        p[ks] = p[ks] + torch.linspace(-4.0, 3.0, g.z_dim)
        p[kl] = p[kl] + torch.linspace(-3.0, 3.0, g.z_dim)
    return p, obs


def trained_weights(ospec, p, obs, u, eps, times):
    p = dict(p)
    for k in p:
        if k.startswith("decoder.ode_model.") and k.endswith("weight"):
            p[k] = p[k] * 3.0
    p["encoder.lin.weight"] = p["encoder.lin.weight"] * 4.0
    p["encoder.z_loc.weight"] = p["encoder.z_loc.weight"] * 3.0
    return p, obs


def raw_units(ospec, p, obs, u, eps, times):
    return p, _relaid(12.0 * obs - 4.0, obs)


def ties(ospec, p, obs, u, eps, times):
    p = dict(p)
    for k in p:
        if k.startswith("decoder.output_") and k.endswith(".0.weight"):
            w = p[k].clone()
            w[0] = 0.0
            p[k] = w
    o = obs.clone()
    o[:, 0, ::3] = 0.0
    o[:, 0, 1::6] = -0.0
    return p, o


def _centre_and_std(ospec, p, obs, u, eps, times, dtype=torch.float64):
    """(mu_50 | mean, std) [B, C, T] of the oracle at the first draw of ``eps``."""
    with torch.no_grad():
        _, parts = O.main_loss({k: v.to(dtype) for k, v in p.items()}, ospec, obs.to(dtype), u.to(dtype), _one_draw(eps).to(dtype),
                               times.to(dtype), return_parts=True)
    dec = parts["dec"]
    return (dec[1], dec[2]) if ospec.gauss else (dec[2], dec[4])


def fitted(ospec, p, obs, u, eps, times):
    p, _ = tight_noise(ospec, p, obs, u, eps, times)
    q = torch.rand(obs.shape, generator=torch.Generator().manual_seed(FITTED_SEED), dtype=torch.float64).clamp(1e-6, 1.0 - 1e-6) - 0.5
    noise = -torch.sign(q) * torch.log1p(-2.0 * q.abs())                                  # inverse cdf of Laplace(0, 1)
    for _ in range(FITTED_PASSES):
        centre, std = _centre_and_std(ospec, p, obs, u, eps, times)
        obs = _relaid(centre + std.clamp_max(0.5) * noise, obs)
    return p, obs


def everything(ospec, p, obs, u, eps, times):
    for f in (tight_noise, posterior_scales, prior_scales, trained_weights, raw_units):
        p, obs = f(ospec, p, obs, u, eps, times)
    return p, obs


REGIMES = {"tight_noise": tight_noise, "posterior_scales": posterior_scales, "prior_scales": prior_scales,
           "trained_weights": trained_weights, "raw_units": raw_units, "ties": ties, "fitted": fitted, "all": everything}
BOUNDS_REGIMES = ("tight_noise", "prior_scales", "trained_weights", "fitted", "all")      # those of the per-trajectory bounds


def _clear(p, ospec, obs, u, eps, times):
    """U.clear_of_kinks for every draw of ``eps`` ([B, L] or [K, B, L]); returns (obs, elements moved)."""
    moved = 0
    for e in (eps if eps.dim() == 3 else eps[None]):
        obs, n = U.clear_of_kinks(p, ospec, obs, u, e, times, margin=KINK_MARGIN)
        moved += n
    return obs, moved


def apply(regime, c):
    """The case ``c`` (a dict with ospec, p, obs, u, eps, times) under ``regime``: a new dict with p and obs replaced, ``regime`` and
    ``moved`` (elements clear_of_kinks moved) added.  ties: channel 0 keeps its constructed values."""
    args = (c["u"], c["eps"], c["times"])
    p, obs = REGIMES[regime](c["ospec"], c["p"], c["obs"], *args)
    cleared, moved = _clear(p, c["ospec"], obs, *args)
    if regime == "ties" and not c["ospec"].gauss:
        moved = int((cleared[:, 1:] != obs[:, 1:]).sum())
        cleared[:, 0] = obs[:, 0]
    assert cleared.stride() == c["obs"].stride() and cleared.dtype == c["obs"].dtype
    return dict(c, p=p, obs=cleared, regime=regime, moved=moved)


# ---- the seeded cases ----------------------------------------------------------------------------------------------------------------------
def shape_case(fam, kw, T, B, mode="exact", seed=17):
    """The case of tests/test_gpu_instantiations._case (parameters: init_params + 0.05 randn of ``seed``; synthetic_batch) at any B."""
    ospec = dataclasses.replace(U.OSPEC[fam](**kw), grad_mode=mode)
    S = 8 if fam == "proc" else 5
    obs, u, eps, times = O.synthetic_batch(ospec, B, T)
    return dict(fam=fam, kw=kw, T=T, S=S, B=B, ospec=ospec, p=U.params(ospec, T, S, seed), obs=obs, u=u, eps=eps, times=times)


# ---- the two oracles of a case and the bars ------------------------------------------------------------------------------------------------
def oracle32(c, which="main"):
    """U.oracle's dict on fp32 tensors: the same oracle in the precision of the kernels, on the CPU."""
    q = {k: v.detach().float().requires_grad_(True) for k, v in c["p"].items()}
    if which == "main":
        loss, parts = O.main_loss(q, c["ospec"], c["obs"], c["u"], c["eps"], c["times"], return_parts=True)
    else:
        loss, parts = O.aux_loss(q, c["ospec"], c["obs"], c["u"], c["eps"]), None
    out = dict(loss=loss.detach())
    if parts is not None:
        out.update(x=parts["dec"][0].detach(), z=parts["z"].detach())
    loss.backward()
    out["grads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in q.items()}
    return out


def bar(suite, fp32_distance):
    """The bar rule: the suite's bar, or 4 x the fp32 CPU oracle's distance where that is larger."""
    return max(suite, 4.0 * fp32_distance)


def small_std_block(c):
    """Mask [C, T] of decoder.constant_std's entries with a raw value below SMALL_STD_RAW (scales under softplus(-4) = 0.018)."""
    return c["p"]["decoder.constant_std"] < SMALL_STD_RAW


def block_rel(got, want, mask):
    return U.rel(got.detach().cpu()[mask], want.detach().cpu()[mask])


class Oracles:
    """Both oracles of one case and one loss (which = "main" | "aux"), the fp32 oracle's distances and the bars that follow from them."""

    def __init__(self, c, which="main"):
        self.c, self.which = c, which
        self.o64 = U.oracle(c["p"], c["ospec"], c["obs"], c["u"], c["eps"], c["times"], which=which)
        self.o32 = oracle32(c, which)
        self.loss32 = U.loss_err(self.o32["loss"], self.o64["loss"])
        self.grad32 = U.tensor_errors(self.o32["grads"], self.o64["grads"])
        self.zero = {k for k, w in self.o64["grads"].items() if float(w.abs().max()) == 0.0}
        self.loss_bar = bar(LOSS_BAR, self.loss32)
        self.grad_bar = {k: (0.0 if k in self.zero else bar(GRAD_BAR, e)) for k, e in self.grad32.items()}

    def finite(self):
        return all(bool(torch.isfinite(o["loss"]).all()) and all(bool(torch.isfinite(g).all()) for g in o["grads"].values())
                   for o in (self.o64, self.o32))

    def worst32(self):
        k = max((k for k in self.grad32 if k not in self.zero), key=self.grad32.get)
        return k, self.grad32[k]

    def block(self, name, mask):
        """(fp32 distance, bar) of the sub-block ``mask`` of gradient tensor ``name``, norm-wise over the block."""
        d = block_rel(self.o32["grads"][name], self.o64["grads"][name], mask)
        return d, bar(GRAD_BAR, d)

    def check(self, loss, grads, what):
        """A kernel's loss (tensor or float) and unpacked gradient tensors against the fp64 oracle at the bars; returns the report line
        (worst error against its bar) after printing it."""
        le = U.loss_err(loss, self.o64["loss"])
        err = U.tensor_errors(grads, self.o64["grads"])
        ratio = {k: (e / self.grad_bar[k] if self.grad_bar[k] > 0 else (0.0 if e == 0.0 else float("inf"))) for k, e in err.items()}
        worst = max(ratio, key=ratio.get)
        line = ("%s %s: loss %.2e / bar %.2e (fp32 oracle %.2e); worst tensor %s %.2e / bar %.2e (fp32 oracle %.2e)"
                % (what, self.which, le, self.loss_bar, self.loss32, worst, err[worst], self.grad_bar[worst], self.grad32[worst]))
        print(line)
        assert le <= self.loss_bar, (what, self.which, "loss", le, self.loss_bar)
        bad = {k: (err[k], self.grad_bar[k]) for k in err if not err[k] <= self.grad_bar[k]}
        assert not bad, (what, self.which, "gradient tensors off the oracle (error, bar)", bad)
        return line


# ---- what a regime reaches (fp64 oracle unless dtype says otherwise) -----------------------------------------------------------------------
def reach(c, dtype=torch.float64):
    """dict: lik_scale (min, max), post_ratio, prior_ratio (largest / smallest scale), tanh_share (|h| > 0.99), state_max, ties (elements of
    channel 0 with obs == centre prediction), fit_median (median |obs - centre| / std), all on the first draw of eps."""
    ospec = c["ospec"]
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    obs, u, eps, times = c["obs"].to(dtype), c["u"].to(dtype), _one_draw(c["eps"]).to(dtype), c["times"].to(dtype)
    with torch.no_grad():
        _, parts = O.main_loss(p, ospec, obs, u, eps, times, return_parts=True)
        dec = parts["dec"]
        centre, std = (dec[1], dec[2]) if ospec.gauss else (dec[2], dec[4])
        _, pscale = O.prior_loc_scale(p, ospec, u)
        n_u = ospec.latent_dim - ospec.z_eps_dim
        h = F.avg_pool1d(F.conv1d(obs, p["encoder.conv.weight"], p["encoder.conv.bias"]), ospec.pool_size, stride=1)
        h = torch.tanh(F.linear(h.reshape(h.size(0), -1), p["encoder.lin.weight"], p["encoder.lin.bias"]))
    return dict(lik_scale=(float(std.min()), float(std.max())), post_ratio=float(parts["scale"].max() / parts["scale"].min()),
                prior_ratio=float(pscale[:, :n_u].max() / pscale[:, :n_u].min()), tanh_share=float((h.abs() > 0.99).double().mean()),
                state_max=float(dec[0].abs().max()), ties=int((obs[:, 0] == centre[:, 0]).sum()),
                fit_median=float(((obs - centre).abs() / std).median()))


# ---- the per-trajectory bounds and the moments under the bar rule --------------------------------------------------------------------------
def bounds_oracles(c):
    """TU.oracle_rows in fp64 and in fp32, and ``want``: the fp64 rows with ``mag`` scaled so that TU.check_oracle's bar 1e-5 x mag becomes
    the bar rule's -- 4 x the fp32 oracle's worst ratio (over the per-draw losses and slots 0, 1, 3, each on its own bar) where that
    exceeds 1.  Returns (want, worst fp32 ratio)."""
    w64, w32 = TU.oracle_rows(c), TU.oracle_rows(c, dtype=torch.float32)
    b = TU.REL * w64["mag"]
    m64, iw64, _ = TU.reduce64(w64["loss"])
    m32, iw32, _ = TU.reduce64(w32["loss"])
    r = max(float((np.abs(w32["loss"] - w64["loss"]) / b).max()), float((np.abs(m32 - m64) / b.mean(0)).max()),
            float((np.abs(iw32 - iw64) / b.max(0)).max()), float((np.abs(w32["nll"].mean(0) - w64["nll"].mean(0)) / b.mean(0)).max()))
    return dict(w64, mag=w64["mag"] * max(1.0, 4.0 * r)), r


def moments(c, is_post, dtype=torch.float64):
    """tests/recon_moments_util.oracle_moments computed in ``dtype``: (mean, sd) [Q, B, C, T] as float64 numpy arrays."""
    from tests import recon_moments_util as RU
    ospec = c["ospec"]
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    e = c["eps"].to(dtype)
    ns, B, L = e.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p, c["obs"].to(dtype), ospec.pool_size) if is_post else O.prior_loc_scale(p, ospec, c["u"].to(dtype))
        z = (loc.unsqueeze(0) + scale.unsqueeze(0) * e).reshape(ns * B, L)
        mu = RU.oracle_curves(p, ospec, z, c["times"].to(dtype), ospec.solver)
    mu = mu.reshape(mu.shape[0], ns, B, mu.shape[2], mu.shape[3]).double().numpy()
    return np.mean(mu, 1), np.std(mu, 1)


# ---- the table of the module docstring -----------------------------------------------------------------------------------------------------
def fp32_row(name, regime, main, aux):
    """One line of the table: the fp32 oracle's loss distance and its worst tensor, main and auxiliary, with the bars that follow."""
    cells = []
    for o in (main, aux):
        k, e = o.worst32()
        cells.append("loss %.1e bar %.1e%s  grad %.1e (%s) bar %.1e%s" % (o.loss32, o.loss_bar, "x" if o.loss_bar > LOSS_BAR else " ", e, k,
                                                                       o.grad_bar[k], "x" if o.grad_bar[k] > GRAD_BAR else " "))
    return "%-34s %-17s main: %s | aux: %s" % (name, regime, cells[0], cells[1])
