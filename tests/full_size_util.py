"""Helpers of tests/test_gpu_full_size.py (test infrastructure): inputs built like test_gpu_instantiations.py, the fp64 oracle in one
pass (loss, every gradient tensor, the trajectories and the latent sample), and comparisons that report the worst per-tensor error."""
import dataclasses

import torch

from oracle import slode_oracle as O

OSPEC = {"cvs": O.cvs_spec, "challenge": O.challenge_spec, "proc": O.proc_spec}


def params(ospec, T, S, seed=17):
    """O.init_params moved off the near-zero initialisation by 0.05 randn, so that every gradient path carries weight."""
    p = O.init_params(ospec, T=T, S=S)
    g = torch.Generator().manual_seed(seed)
    return {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in p.items()}


def oracle(p, ospec, obs, u, eps, times, which="main", grads=True):
    """fp64 oracle: dict(loss, grads {name: tensor}, x [B,T,S], z [B,L]); which = "main" | "aux" (aux: no x / z); grads=False: the
    forward alone (no autograd graph)."""
    q = {k: v.detach().double().requires_grad_(grads) for k, v in p.items()}
    args = (obs.double(), u.double(), eps.double())
    with torch.set_grad_enabled(grads):
        if which == "main":
            loss, parts = O.main_loss(q, ospec, *args, times.double(), return_parts=True)
        else:
            loss, parts = O.aux_loss(q, ospec, *args), None
    out = dict(loss=loss.detach())
    if parts is not None:
        out.update(x=parts["dec"][0].detach(), z=parts["z"].detach())
    if grads:
        loss.backward()
        out["grads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in q.items()}
    return out


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def loss_err(got, want):
    got = got.item() if isinstance(got, torch.Tensor) else float(got)
    return abs(got - want.item()) / abs(want.item())


def tensor_errors(got, want):
    """{name: error}: norm-wise relative error per tensor; a tensor whose oracle gradient is zero must come back exactly zero (its
    error is then the largest magnitude returned, 0 if it is)."""
    out = {}
    for k, v in got.items():
        w = want[k].double()
        out[k] = rel(v, w) if float(w.abs().max()) != 0.0 else float(v.abs().max())
    return out


def check_grads(got, want, bar=5e-4, what="", sens=None):
    """Every tensor within `bar` (+ 3 x sens[name] when `sens` is given: the oracle's own sensitivity to the adaptive step sequence, see
    step_sensitivity); returns (worst name, worst error) so that callers can report the margin."""
    err = tensor_errors(got, want)
    worst = max(err, key=err.get)
    bad = {k: e for k, e in err.items() if not e <= bar + (3.0 * sens[k] if sens is not None else 0.0)}
    assert not bad, ("%s: gradient tensors off the oracle" % what, bad, "worst", worst, err[worst])
    return worst, err[worst]


def step_sensitivity(loose, tight):
    """{name: error} of the oracle's gradient at the engine's tolerances against the oracle's at tight ones, and the same for the loss
    (key "loss") and the trajectories (key "x", traj_err): how far two adaptive step sequences that both meet the tolerances put the result
    apart.  Gradients that integrate relu' of the dynamics' hidden layer over time (dynamics_hidden, and through z the encoder) see an
    O(step) quadrature error at every kink."""
    out = tensor_errors(loose["grads"], tight["grads"])
    out["loss"] = loss_err(loose["loss"], tight["loss"])
    out["x"] = traj_err(loose["x"], tight["x"])
    return out


def worst_sensitivity(sens):
    """(name, value) of the tensor the step sequence moves most."""
    tens = {k: v for k, v in sens.items() if k not in ("loss", "x")}
    k = max(tens, key=tens.get)
    return k, tens[k]


def dopri5_kmax(B, S):
    """Record capacity per trajectory of the dopri5 training step (accepted steps): 2^26 / (B (S + 2)) within [64, 2048], as
    tests/test_host_cpu.py pins it in the workspace size."""
    return max(64, min(2048, (1 << 26) // (B * (S + 2))))


def traj_err(x, want):
    """max |x - want| / max(1, |want|) element-wise (test_gpu_parity._close)."""
    x, want = x.double().cpu(), want.double().cpu()
    return ((x - want).abs() / want.abs().clamp_min(1.0)).max().item()


def additivity_per_tensor(eng, parts, g_all, bar=1e-5):
    """The additivity bar of the flat gradient (the sum of the gradients of the parts of a batch == the whole batch's), tensor by tensor: a
    tensor that is wholly wrong hides under the flat norm (most of which is dynamics_hidden.weight) but not here.  Returns {name: error}
    of the tensors over `bar` (a tensor that is zero for the whole batch must sum to exactly zero)."""
    whole = eng.unpack(g_all.double().cpu())
    summed = eng.unpack(sum(g.double().cpu() for g in parts))
    out = {}
    for k, w in whole.items():
        n = w.norm()
        e = ((summed[k] - w).norm() / n).item() if n > 0 else (summed[k] - w).abs().max().item()
        if not e <= bar:
            out[k] = e
    return out


def clear_of_kinks(p, ospec, obs, u, eps, times, margin=1e-4):
    """obs with every element that lies within `margin` of a predicted quantile (fp64 oracle) moved to `margin` from it, on its own side;
    returns (obs, number of elements moved).  The quantile likelihood's gradient jumps where an observation equals its prediction (the
    weight switches between tau and 1 - tau): an element closer than the fp32 rounding of the prediction lands on either side depending
    on summation order, so two launches that sum in different orders (another encoder tile, another batch split) can differ there by far
    more than rounding -- the oracle itself is discontinuous at that point.  Same layout as obs."""
    if ospec.gauss:
        return obs, 0
    with torch.no_grad():
        _, parts = O.main_loss({k: v.double() for k, v in p.items()}, ospec, obs.double(), u.double(), eps.double(), times.double(),
                               return_parts=True)
    out, moved = obs.clone(), 0
    for mu in parts["dec"][1:4]:
        d = out.double() - mu
        near = d.abs() < margin
        if near.any():
            out[near] = (mu + torch.where(d >= 0, margin, -margin))[near].to(out.dtype)
            moved += int(near.sum())
    return out, moved


def engine(fam, kw, T, dev, mode=None):
    from structured_latent_odes_amd import engine as E
    espec = {"cvs": E.cvs_spec, "challenge": E.challenge_spec, "proc": E.proc_spec}[fam](**kw)
    if mode is not None:
        espec = dataclasses.replace(espec, grad_mode=mode)
    return E.Engine(espec, T, dev)


def to_device(obs, dev):
    """The batch layout the data loaders hand over: contiguous [B,C,T] stays so (proc), a [B,C,T] view of [B,T,C] stays a view."""
    if obs.is_contiguous():
        return obs.to(dev)
    return obs.permute(0, 2, 1).contiguous().to(dev).permute(0, 2, 1)
