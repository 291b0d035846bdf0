"""Time the fused posterior refinement (slode_posterior_refine: J Adam steps per trajectory on its own (loc, log scale), one kernel) against the
composed route, in ONE process: the same objective written with torch -- Normal / Laplace log-probabilities on the curves of
``decoder.forward`` (``OdeModel.solve_ODE`` and the head modules under torch autograd: slode_ode_solve_fwd / _bwd, slode_decode_heads /
_bwd, existing library calls only) -- and ``torch.optim.Adam`` on the two leaves, a dozen launches and more per iteration.  Shape: the metric
shape (cvs, B = 1024, T = 200, rk4, exact gradients), K = 8 draws (explicit noise, the same rows for both legs), J in {10, 50}.  Device
events around each leg on the current stream; warmed; the legs ALTERNATE `--rounds` times and each reports its median and its spread (max -
min) in milliseconds; also the kernels of one fused call from slode_profile_read, and the largest difference between the two legs' final
-ELBO per trajectory relative to its magnitude (same loop, different arithmetic: a cross-check, not a gate).  Prints one JSON line; --out
writes it to a file.

    python tools/refine_bench.py --out profiles/refine.json
"""
import torch
from torch.distributions import Laplace, Normal

import eval_bench as EB

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200,
                                  dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2, adjoint_solver=False)),
}
STEPS = (10, 50)
LR = 0.05


def composed(m, batch, eps, J, lr):
    """The loop of the fused call on torch autograd: returns (loc, scale, F [J + 1, B]) of the LAST iterate's trace (no best-iterate pick)."""
    obs = batch["observations"]
    labels = {l: batch[l] for l in m.LABELS}
    K, B, L = eps.shape
    with torch.no_grad():
        loc, scale = m._loc_scale(obs, True, labels)
        ploc, pscale = m._prior_loc_scale(labels)
    loc, rho = loc.clone().requires_grad_(True), scale.log().requires_grad_(True)
    opt = torch.optim.Adam([loc, rho], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    ob = obs.repeat(K, 1, 1)
    d = float(m.config.quantile_diff) if not m.GAUSS else 0.0
    trace = []

    def objective():
        sc = rho.exp()
        z = loc.unsqueeze(0) + sc.unsqueeze(0) * eps
        kl = Normal(loc, sc).log_prob(z).sum(-1) - Normal(ploc, pscale).log_prob(z).sum(-1)
        out = m.decoder.forward(z=z.reshape(K * B, L))
        if m.GAUSS:
            ll = Normal(out[1], out[2]).log_prob(ob).sum((1, 2))
        else:
            _, mu75, mu50, mu25, std = out
            ll = 0.0
            for mu, tau in ((mu50, 0.5), (mu75, 0.5 + d), (mu25, 0.5 - d)):
                lp = Laplace(mu, std).log_prob(ob)
                ll = ll + (torch.where(ob >= mu, tau, 1.0 - tau) * lp).sum((1, 2))
        return (kl - ll.reshape(K, B)).mean(0)

    for _ in range(J):
        opt.zero_grad(set_to_none=True)
        F = objective()
        trace.append(F.detach())
        F.sum().backward()
        opt.step()
    with torch.no_grad():
        trace.append(objective())
    return loc.detach(), rho.detach().exp(), torch.stack(trace)


def run_shape(name, K, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    b = m._bind()
    eng, flat = b.engine, b.flat
    eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
    bt = eng.make_batch(batch["observations"], [batch[l].to(torch.float32).contiguous() for l in m.LABELS], eps, particles=K)
    res = {"B": B, "T": T, "K": K, "lr": LR, "rounds": rounds, "steps": {}}
    for J in STEPS:
        legs = {"posterior_refine": lambda: eng.posterior_refine(flat, bt, B, K, J, LR),
                "composed_torch_autograd": lambda: composed(m, batch, eps, J, LR)}
        pt = EB.alternate(legs, rounds, dev, warm=1, peak=False)
        pt["ratio_composed_over_fused"] = pt["composed_torch_autograd"]["median_ms"] / pt["posterior_refine"]["median_ms"]
        eng.profile_enable(True)
        _, _, elbo, _, trace, _ = legs["posterior_refine"]()
        pt["posterior_refine"]["kernels_us"] = eng.profile_read()
        eng.profile_enable(False)
        _, _, ctrace = composed(m, batch, eps, J, LR)
        pt["mean_elbo_before"] = float(elbo[:, 0].double().mean().item())
        pt["mean_elbo_after"] = float(elbo[:, 1].double().mean().item())
        pt["composed_mean_elbo_after"] = float(ctrace.min(0).values.double().mean().item())
        pt["final_trace_max_rel_difference"] = float(((trace[-1] - ctrace[-1]).abs() / ctrace[-1].abs()).max().item())
        res["steps"]["J%d" % J] = pt
    return res


if __name__ == "__main__":
    EB.main("refine_bench", SHAPES, run_shape, "--draws", 8)
