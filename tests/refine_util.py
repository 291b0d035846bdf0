"""Test infrastructure of the posterior refinement (slode_posterior_refine): the per-trajectory objective on the fp64 oracle --
tests/traj_bounds_util.oracle_rows with a weight on every likelihood term, without no_grad and with (loc, rho = log scale) as leaves -- its
gradient, the Adam / best-iterate loop of the call in fp64 and in fp32, a numpy transcription of the kernel's backward formulas
(tests/kernel_math.py: reverse scan, step_coeffs_bwd, a / d, hidden layer, init net; here: the weighted likelihood gradient and the KL terms),
and the bars.  Not imported by the product.

Objective, per trajectory b, on noise rows eps[k][b] that stay fixed:
    F(phi) = 1/K sum_k loss_k,  loss_k = -(sum_{c,t,q} w[b,c,t] ll[c,t,q] + log p(z_k | u) - log q(z_k)),  z_k = loc + exp(rho) eps_k.

Bars.  ``bar[b] = 1e-5 * mag[b]``, mag = mean_k (|ll_w| + |log p| + |log q|) with the weights applied: the project's 1e-5 bar on a loss, taken
on the term magnitudes because one row can cancel between its terms (tests/traj_bounds_util.py).  The gradient bar is the project's: 5e-4
norm-wise per trajectory.  The trace of J = 4 Adam steps is held to (1 + 4 rho) bar, where rho is the largest deviation, in units of bar,
between this module's loop run in fp32 and in fp64 on the CPU over every case of CASES x SOLVERS x {no mask, prefix mask}: an fp32
implementation of the same loop cannot be asked to do better than a few times that.  Measured here (tests/test_refine_cpu.py prints and
bounds it): the largest deviation is 0.158 bar (challenge_gauss / midpoint, T = 300); RHO below rounds it up.

Why the trace and not the iterates: Adam's first step is lr * sign(g); a latent dimension whose gradient is near zero may flip sign between
two correct implementations.  Its effect on F is below the bar."""
import numpy as np
import torch
from torch.distributions import Laplace, Normal

from oracle import slode_oracle as O
from tests import kernel_math as KM
from tests import traj_bounds_util as TU

CASES = ("cvs_ald", "cvs_gauss", "challenge_ald", "challenge_gauss")        # the families the call takes (proc scores labels in its main loss)
SOLVERS = ("euler", "midpoint", "rk4")
B, K, J, LR = 5, 3, 4, 0.05
REL = 1e-5
GRAD_REL = 5e-4
RHO = 0.16                                                                   # measured: challenge_gauss (T = 300) 0.11 - 0.158, the other cases below 0.04
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def build(case, solver="rk4", B=B, K=K):
    return TU.build(case, solver, B=B, K=K)


def prefix_mask(c):
    """Weights [B, C, T]: 1 on the first half of the window, 0 on the second."""
    w = torch.ones_like(c["obs"])
    w[:, :, c["T"] // 2:] = 0.0
    return w


def weighted_loglik(ospec, dec, ob, w):
    """sum over (c, t, q) of w * ll, per row: ``dec`` = the decoder's output on the rows, ``ob`` / ``w`` [rows, C, T]."""
    if ospec.gauss:
        _, mean, std = dec
        return (w * Normal(mean, std).log_prob(ob)).sum((1, 2))
    _, mu75, mu50, mu25, std = dec
    d = ospec.quantile_diff
    ll = 0.0
    for mu, tau in ((mu50, 0.5), (mu75, 0.5 + d), (mu25, 0.5 - d)):
        lp = Laplace(mu, std).log_prob(ob)
        ll = ll + (w * torch.where(ob.ge(mu), torch.full_like(lp, tau), torch.full_like(lp, 1 - tau)) * lp).sum((1, 2))
    return ll


def _inputs(c, eps, w, dtype):
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    obs, u, times = c["obs"].to(dtype), c["u"].to(dtype), c["times"].to(dtype)
    e = (c["eps"] if eps is None else eps).to(dtype)
    w = torch.ones_like(obs) if w is None else w.to(dtype)
    return p, obs, u, times, e, w


def encoder(c, dtype=torch.float64):
    """phi_0 = (loc, rho = log scale) of the encoder, [B, L] each."""
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    with torch.no_grad():
        loc, scale = O.encoder_conv(p, c["obs"].to(dtype), c["ospec"].pool_size)
    return loc, scale.log()


def objective(c, loc, rho, eps=None, w=None, dtype=torch.float64):
    """F [B] (differentiable in loc, rho) and mag [B] (detached)."""
    ospec = c["ospec"]
    p, obs, u, times, e, w = _inputs(c, eps, w, dtype)
    Kd, Bd, L = e.shape
    scale = rho.exp()
    ploc, pscale = O.prior_loc_scale(p, ospec, u)
    z = loc.unsqueeze(0) + scale.unsqueeze(0) * e
    log_q = Normal(loc, scale).log_prob(z).sum(-1)
    log_p = Normal(ploc, pscale).log_prob(z).sum(-1)
    zf = z.reshape(Kd * Bd, L)
    dec = (O.decoder_gauss if ospec.gauss else O.decoder_ald)(p, zf, times, ospec.solver)
    ll = weighted_loglik(ospec, dec, obs.repeat(Kd, 1, 1), w.repeat(Kd, 1, 1)).reshape(Kd, Bd)
    loss = -(ll + log_p - log_q)
    mag = (ll.abs() + log_p.abs() + log_q.abs()).detach()
    return loss.mean(0), mag.mean(0)


def value_and_grad(c, loc, rho, eps=None, w=None, dtype=torch.float64):
    """F [B], mag [B], dF/d(loc, rho) [B, 2 L] by autograd (the trajectories are independent: the gradient of sum_b F_b)."""
    loc, rho = loc.detach().clone().requires_grad_(True), rho.detach().clone().requires_grad_(True)
    F, mag = objective(c, loc, rho, eps, w, dtype)
    gl, gr = torch.autograd.grad(F.sum(), (loc, rho))
    return F.detach(), mag, torch.cat([gl, gr], 1)


def refine(c, eps=None, w=None, J=J, lr=LR, dtype=torch.float64, bias_correction=True):
    """The call's loop in ``dtype``: dict(trace [J + 1, B], mag [B] (at phi_0), grad0 [B, 2 L], loc, scale [B, L] (the best iterate), elbo0,
    elbo [B], best_step [B]) as float64 numpy arrays.  ``bias_correction=False``: the wrong loop the trace test must tell apart."""
    loc, rho = encoder(c, dtype)
    m_l, v_l, m_r, v_r = (torch.zeros_like(loc) for _ in range(4))
    trace, best, mag0, grad0 = [], None, None, None
    for j in range(J + 1):
        if j < J or j == 0:
            F, mag, g = value_and_grad(c, loc, rho, eps, w, dtype)
        else:
            with torch.no_grad():
                F, mag = objective(c, loc, rho, eps, w, dtype)
        if j == 0:
            mag0, grad0 = mag, g
            best = dict(F=F.clone(), loc=loc.clone(), rho=rho.clone(), j=torch.zeros(F.shape[0], dtype=torch.long))
        else:
            better = F < best["F"]
            best["F"] = torch.where(better, F, best["F"])
            best["loc"] = torch.where(better[:, None], loc, best["loc"])
            best["rho"] = torch.where(better[:, None], rho, best["rho"])
            best["j"] = torch.where(better, torch.full_like(best["j"], j), best["j"])
        trace.append(F)
        if j < J:
            L = loc.shape[1]
            gl, gr = g[:, :L], g[:, L:]
            c1, c2 = (1 - BETA1 ** (j + 1), 1 - BETA2 ** (j + 1)) if bias_correction else (1.0, 1.0)
            m_l, v_l = BETA1 * m_l + (1 - BETA1) * gl, BETA2 * v_l + (1 - BETA2) * gl * gl
            m_r, v_r = BETA1 * m_r + (1 - BETA1) * gr, BETA2 * v_r + (1 - BETA2) * gr * gr
            loc = loc - lr * (m_l / c1) / ((v_l / c2).sqrt() + ADAM_EPS)
            rho = rho - lr * (m_r / c1) / ((v_r / c2).sqrt() + ADAM_EPS)
    n = lambda t: t.double().numpy()
    return dict(trace=n(torch.stack(trace)), mag=n(mag0), grad0=n(grad0), loc=n(best["loc"]), scale=n(best["rho"].exp()), elbo0=n(trace[0]),
                elbo=n(best["F"]), best_step=best["j"].numpy())


def objective_at(c, loc, scale, eps=None, w=None):
    """F [B] and mag [B] of the fp64 oracle at a given (loc, scale) (numpy or tensors)."""
    with torch.no_grad():
        F, mag = objective(c, torch.as_tensor(loc, dtype=torch.float64), torch.as_tensor(scale, dtype=torch.float64).log(), eps, w)
    return F.numpy(), mag.numpy()


# ---- the kernel's backward formulas, transcribed (fp64 numpy) ---------------------------------------------------------------------------
def kernel_grad(c, loc, rho, eps=None, w=None):
    """dF/d(loc, rho) [B, 2 L] by the formulas refine_kernel.hip executes: per draw, g_x[t][s] = -sum_{c,q} w dll/dmu hw[qc][s] (Gauss:
    dll/dmu = r inv^2; ALD: inv (y >= mu ? tau : -(1 - tau))); the reverse affine scan, step_coeffs_bwd, the a / d evaluator, the hidden
    layer and the init net (tests/kernel_math.ode_backward); d(-log p)/dz = (z - pl) ips^2, d(log q)/d loc = 0, d(log q)/d rho = -1;
    g_loc += g_z, g_rho += g_z scale eps - 1; the mean over the draws."""
    ospec = c["ospec"]
    pn = {k: v.double().numpy() for k, v in c["p"].items()}
    obs, u, times = c["obs"].double().numpy(), c["u"].double().numpy(), c["times"].double().numpy()
    e = (c["eps"] if eps is None else eps).double().numpy()
    w = np.ones_like(obs) if w is None else w.double().numpy()
    loc, rho = np.asarray(loc, np.float64), np.asarray(rho, np.float64)
    sc = np.exp(rho)
    with torch.no_grad():
        ploc, pscale = O.prior_loc_scale({k: v.double() for k, v in c["p"].items()}, ospec, c["u"].double())
    pl, ips = ploc.numpy(), 1.0 / pscale.numpy()
    inv = 1.0 / KM.softplus(pn["decoder.constant_std"])[None]                             # [1, C, T]
    if ospec.gauss:
        heads = [("decoder.output_mean.0.weight", None)]
    else:
        d = ospec.quantile_diff
        heads = [("decoder.output_q50.0.weight", 0.5), ("decoder.output_q75.0.weight", 0.5 + d), ("decoder.output_q25.0.weight", 0.5 - d)]
    g_loc, g_rho = np.zeros_like(loc), np.zeros_like(rho)
    for k in range(e.shape[0]):
        z = loc + sc * e[k]
        x, sv = KM.ode_forward(pn, z, times, ospec.solver)
        gx = np.zeros_like(x)
        for key, tau in heads:
            W = pn[key]
            mu = np.einsum("bts,cs->bct", x, W)
            r = obs - mu
            dll = r * inv * inv if tau is None else inv * np.where(obs >= mu, tau, -(1 - tau))
            gx -= np.einsum("bct,cs->bts", w * dll, W)
        gz, _ = KM.ode_backward(pn, z, times, ospec.solver, x, sv, gx)
        gz = gz + (z - pl) * ips * ips
        g_loc += gz
        g_rho += gz * sc * e[k] - 1.0
    return np.concatenate([g_loc, g_rho], 1) / e.shape[0]


def norm_err(got, want):
    """Norm-wise relative error per row."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)


_REF = {}


def reference(case, solver, masked=False, B=B, K=K):
    """(c, w, the fp64 loop's result): computed once per key, shared among the tests, left unchanged."""
    key = (case, solver, masked, B, K)
    if key not in _REF:
        c = build(case, solver, B, K)
        w = prefix_mask(c) if masked else None
        _REF[key] = (c, w, refine(c, w=w))
    return _REF[key]
