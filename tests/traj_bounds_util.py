"""Test infrastructure of the per-trajectory bounds (slode_traj_bounds): the seeded cases (those of tests/eval_stats_util.py, at any B),
the per-row oracle -- the pieces of oracle/slode_oracle.py's main_loss composed WITHOUT the sums over the batch -- the fp64 reduction of
K per-draw losses to the call's slots, and the bars.  Not imported by the product.

Bars.  The project's bar on the batch-summed loss is 1e-5 relative (test_gpu_parity, test_gpu_eval_stats).  One row can cancel between
its terms, so for a single (draw, trajectory) the relative bar becomes a bar on the term magnitudes:
    bar[k, b] = 1e-5 * (|ll| + |log p| + |log q| + |46 * labels|).
Slots 0 (mean loss) and 3 (mean NLL) against the oracle: mean_k bar (a mean of values within their bars).  Slot 1 against the oracle:
max_k bar (logsumexp is non-expansive in the sup norm).  Slots 1 and 2 against the fp64 reduction of the kernel's OWN loss_kb -- the check
that separates the reduction from the scorer, and the only meaningful one of the ESS (0.05 nat in a loss moves it by tens of percent):
slot 1 within 2^-22 |value| + K 2^-23, slot 2 within 1e-5 K."""
import numpy as np
import torch
from torch.distributions import Laplace, Normal

from oracle import slode_oracle as O
from tests import eval_stats_util as EU

NOISE_SEED = 33
REL = 1e-5


def build(case, solver="rk4", B=None, K=4):
    """EU.build_case's parameters (label heads moved) and synthetic batch (seed 7) at any B, and the [K, B, L] noise of seed 33."""
    return dict(EU.build_case(case, ("eps", K, NOISE_SEED), solver, B), K=K)


def oracle_rows(c, eps=None, rows=None, dtype=torch.float64):
    """Per (draw, trajectory), nothing summed over the batch: dict(loss [K, B], nll [K, B], mag [K, B]) as float64 numpy arrays, computed
    in ``dtype``.  loss = -(ll + log p - log q) - 46 * labels (proc), the main loss of the 1-row batch obs[b:b+1], u[b:b+1], eps[k, b:b+1];
    mag = |ll| + |log p| + |log q| + |46 * labels|.  ``rows``: a slice of the batch (the oracle then runs on those rows only)."""
    ospec = c["ospec"]
    rows = slice(None) if rows is None else rows
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    obs, u, times = c["obs"][rows].to(dtype), c["u"][rows].to(dtype), c["times"].to(dtype)
    e = (c["eps"] if eps is None else eps)[:, rows].to(dtype)
    K, B, L = e.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p, obs, ospec.pool_size)
        ploc, pscale = O.prior_loc_scale(p, ospec, u)
        z = loc.unsqueeze(0) + scale.unsqueeze(0) * e                                   # [K, B, L]
        log_q = Normal(loc, scale).log_prob(z).sum(-1)
        log_p = Normal(ploc, pscale).log_prob(z).sum(-1)
        zf = z.reshape(K * B, L)
        ob = obs.repeat(K, 1, 1)                                                        # row k * B + b: trajectory b
        if ospec.gauss:
            _, mean, std = O.decoder_gauss(p, zf, times, ospec.solver)
            ll = Normal(mean, std).log_prob(ob).sum((1, 2))
        else:
            _, mu75, mu50, mu25, std = O.decoder_ald(p, zf, times, ospec.solver)
            d = ospec.quantile_diff
            ll = 0.0
            for mu, tau in ((mu50, 0.5), (mu75, 0.5 + d), (mu25, 0.5 - d)):             # the ALD masks, elementwise (O.ald_loglik)
                lp = Laplace(mu, std).log_prob(ob)
                ll = ll + (torch.where(ob.ge(mu), torch.full_like(lp, tau), torch.full_like(lp, 1 - tau)) * lp).sum((1, 2))
        ll = ll.reshape(K, B)
        lab = torch.zeros(K, B, dtype=dtype)
        if ospec.labels_in_main:
            for k in range(K):
                for b in range(B):
                    lab[k, b] = ospec.aux_mult * O._label_terms(p, ospec, z[k, b:b + 1], u[b:b + 1])
        loss = -(ll + log_p - log_q) - lab
        mag = ll.abs() + log_p.abs() + log_q.abs() + lab.abs()
    return dict(loss=loss.double().numpy(), nll=(-ll).double().numpy(), mag=mag.double().numpy())


def reduce64(loss):
    """The call's slots 0, 1, 2 from K per-draw losses [K, B], in fp64: mean, -log(1/K sum exp(-loss)), (sum w)^2 / sum w^2."""
    loss = np.asarray(loss, dtype=np.float64)
    mn = loss.min(0)
    w = np.exp(mn[None] - loss)
    return loss.mean(0), mn - np.log(w.mean(0)), w.sum(0) ** 2 / (w ** 2).sum(0)


def check_reduction(bounds, loss_kb, tag):
    """Slots 1 and 2 (and 0, to fp32 rounding) against the fp64 reduction of the kernel's own loss_kb."""
    b, l = bounds.detach().double().cpu().numpy(), loss_kb.detach().double().cpu().numpy()
    K = l.shape[0]
    m, iw, ess = reduce64(l)
    r0 = np.abs(b[:, 0] - m) / (2.0 ** -23 * np.abs(m) + 1e-300)
    r1 = np.abs(b[:, 1] - iw) / (2.0 ** -22 * np.abs(iw) + K * 2.0 ** -23)
    r2 = np.abs(b[:, 2] - ess) / (1e-5 * K)
    print("%s: own reduction: slot 0 error / fp32 ulp %.3f, slot 1 error / bar %.3f, slot 2 error / bar %.3e (ESS %.2f .. %.2f)"
          % (tag, r0.max(), r1.max(), r2.max(), b[:, 2].min(), b[:, 2].max()))
    assert np.isfinite(b).all() and np.isfinite(l).all(), tag
    assert r0.max() <= 1.0, (tag, "slot 0", r0.max())
    assert r1.max() <= 1.0, (tag, "slot 1", r1.max())
    assert r2.max() <= 1.0, (tag, "slot 2", r2.max())
    assert np.all(b[:, 2] >= 1.0) and np.all(b[:, 2] <= K), (tag, "ESS outside [1, K]")
    assert np.all(b[:, 1] <= b[:, 0] + 2.0 ** -22 * np.abs(b[:, 0])), (tag, "slot 1 > slot 0")


def check_oracle(bounds, loss_kb, want, tag, rows=None):
    """loss_kb within bar; slots 0 and 3 within mean_k bar, slot 1 within max_k bar of the fp64 oracle.  Prints the worst ratios first."""
    rows = slice(None) if rows is None else rows
    b, l = bounds.detach().double().cpu().numpy()[rows], loss_kb.detach().double().cpu().numpy()[:, rows]
    bar = REL * want["mag"]
    m, iw, _ = reduce64(want["loss"])
    rl = np.abs(l - want["loss"]) / bar
    r0 = np.abs(b[:, 0] - m) / bar.mean(0)
    r3 = np.abs(b[:, 3] - want["nll"].mean(0)) / bar.mean(0)
    r1 = np.abs(b[:, 1] - iw) / bar.max(0)
    print("%s: error / bar: loss_kb %.3f, slot 0 %.3f, slot 1 %.3f, slot 3 %.3f" % (tag, rl.max(), r0.max(), r1.max(), r3.max()))
    assert np.isfinite(b).all() and np.isfinite(l).all(), tag
    assert rl.max() <= 1.0, (tag, "loss_kb", rl.max())
    assert r0.max() <= 1.0, (tag, "slot 0", r0.max())
    assert r1.max() <= 1.0, (tag, "slot 1", r1.max())
    assert r3.max() <= 1.0, (tag, "slot 3", r3.max())
