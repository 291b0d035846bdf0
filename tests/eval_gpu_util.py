"""What the GPU tests of the fifteen eval-side calls (test_gpu_eval_stats, test_gpu_recon_moments, test_gpu_intervene, test_gpu_forecast,
test_gpu_cohort, test_gpu_calibration, test_gpu_traj_bounds, test_gpu_label_evidence, test_gpu_refine, test_gpu_pointwise, and the
whole-curve calls' test_gpu_attribution, test_gpu_summary, test_gpu_quantiles, test_gpu_mechanism, test_gpu_band) share: an engine for a
seeded case (tests/eval_stats_util.py) with the handle's environment switches under control, the case's batch on the device, the model of
the model-level tests with its 17-trajectory batch, the checks every call gets -- refusal, capture and replay, peak allocation -- and what
the whole-curve tests compare with: the kernel's own curve of every draw, the model's own curves, bitwise agreement, the count of engine
calls.  A plain module: not a conftest, not imported by the product."""
import importlib

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU

DEV = torch.device("cuda:0")
WIDTHS = {"cvs": (1, 1), "challenge": (1, 1), "proc": (3, 4, 1, 1)}
ENV_KEYS = ("SLODE_ODE_LOOP", "SLODE_ODE_GRID", "SLODE_ODE_GENERIC", "SLODE_ODE_ALG", "SLODE_ODE_PACK", "SLODE_FOLD_NEXT", "SLODE_NO_FOLD")
ADAPTIVE = ("dopri5", "bosh3", "fehlberg2", "adaptive_heun")


def _set_env(monkeypatch, env):
    """The handle's environment switches: all cleared, then ``env`` set (nothing is touched without ``monkeypatch``)."""
    if monkeypatch is not None:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)


def _engine(c, monkeypatch=None, env=None, solver=None):
    from structured_latent_odes_amd import engine as E
    _set_env(monkeypatch, env)
    kw = dict(c["kw"])
    if solver:
        kw["solver"] = solver
    eng = E.Engine({"cvs": E.cvs_spec, "challenge": E.challenge_spec, "proc": E.proc_spec}[c["fam"]](**kw), c["T"], DEV)
    eng.set_times(c["times"])
    return eng


def _device_batch(c):
    """Observations in the family's layout -- the [B,C,T] view of a contiguous [B,T,C] tensor (cvs / challenge) or contiguous [B,C,T]
    (proc): the two dense layouts the folded encoder takes -- and the label tensors one by one."""
    obs = c["obs"]
    obs_d = obs.to(DEV).contiguous() if c["fam"] == "proc" else obs.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
    labels, o = [], 0
    for w in WIDTHS[c["fam"]]:
        labels.append(c["u"][:, o:o + w].contiguous().to(DEV))
        o += w
    return obs_d, labels


def _lay(t, t_major):
    """A host [B, C, T] tensor on the device in one of the two dense layouts: the [B,C,T] view of a contiguous [B,T,C] tensor, or contiguous."""
    return t.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1) if t_major else t.to(DEV).contiguous()


def _eps_dev(eps):
    return (eps[0] if eps.shape[0] == 1 else eps).to(DEV).contiguous()       # one draw: [B, L], as make_batch takes it


def _recon_moments(eng, flat, c, is_post, eps="case", obs_d=None, labels=None, ns=None):
    """Engine.recon_moments on the case's batch; outputs pre-filled with NaN: every element must be written."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q = 1 if c["ospec"].gauss else 3
    mean = torch.full((Q, c["B"], c["obs"].shape[1], c["T"]), float("nan"), device=DEV)
    sd = torch.full_like(mean, float("nan"))
    eng.recon_moments(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], is_post, ns, mean, sd)
    return mean, sd


# (case, B, ns, env) of the tests "sizes and instantiations" of recon_moments and intervene_moments
SIZES = [("cvs_gauss", 63, 2, {}), ("cvs_gauss", 65, 7, {}), ("cvs_gauss", 255, 2, {}), ("cvs_gauss", 257, 1, {}), ("cvs_ald", 3, 200, {}),
         ("proc_gauss", 65, 2, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}), ("challenge_gauss", 2, 200, {}),
         ("cvs_ald", 9, 7, {"SLODE_ODE_GENERIC": "1"}), ("proc_ald", 9, 2, {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"})]


def _padded(obs):
    """``obs`` as the ``[..., :T]`` view of a tensor three points longer: the same values, a row stride no fused call takes."""
    wide = torch.zeros(obs.shape[0], obs.shape[1], obs.shape[2] + 3, device=DEV)
    wide[:, :, :obs.shape[2]] = obs
    return wide[:, :, :obs.shape[2]]


def _on_device(batch, fam):
    """A host batch of ``EU.model_state`` on the device, the observations in the family's layout (``_device_batch``)."""
    batch = {k: v.to(DEV) for k, v in batch.items()}
    if fam != "proc":
        batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    return batch


def _model_batches(fam, solver=None, monkeypatch=None, env=None):
    """The model of ``EU.model_state(fam)`` on the device (``solver`` replaces rk4) and the host batches of its pass."""
    _set_env(monkeypatch, env)
    twin, state, batches, times = EU.model_state(fam)
    cfg = EU.model_config(fam)
    if solver:
        cfg.update(solver=solver)
    m = importlib.import_module("structured_latent_odes_amd.models.mechanistic_" + fam).MechanisticModel(cfg, DEV, times.to(DEV))
    m.load_state_dict(state)
    return m, batches


def _model(fam, solver=None, monkeypatch=None, env=None):
    """``_model_batches`` with the third batch (17 trajectories) on the device."""
    m, batches = _model_batches(fam, solver, monkeypatch, env)
    return m, _on_device(batches[2], fam)


def _peak(fn):
    """Peak of torch.cuda.max_memory_allocated during ``fn()`` over the allocation before the call."""
    torch.cuda.synchronize(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    out = fn()
    torch.cuda.synchronize(DEV)
    del out
    return torch.cuda.max_memory_allocated(DEV) - before


def _refused(eng, call, match, error=None):
    """``call()`` on ``eng`` raises ``error`` (SlodeError by default) matching ``match``, draws nothing (seed 3, counter 4 before and after)
    and launches nothing (profile on: "no profiled step").  Returns the exception: its status is the call site's to check."""
    from structured_latent_odes_amd import _lib as L
    eng.rng_seed(3)
    eng.rng_set_counter(4)
    eng.profile_enable(True)
    with pytest.raises(error or L.SlodeError, match=match) as ei:
        call()
    assert eng.rng_state() == (3, 0, 4)
    with pytest.raises(L.SlodeError, match="no profiled step"):
        eng.profile_read()
    return ei.value


def _captured(call, outs):
    """``call`` writes the zero-filled tensors ``outs``.  Launched on a side stream; then, outputs zeroed, captured on that stream
    (capturing executes nothing) and replayed once.  Returns the stream-launched values, for the caller to compare ``outs`` with."""
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    want = [t.clone() for t in outs]
    for t in outs:
        t.zero_()
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call()
    torch.cuda.synchronize(DEV)
    assert all(t.abs().sum().item() == 0.0 for t in outs), "capturing must not execute anything"
    g.replay()
    torch.cuda.synchronize(DEV)
    return want


# ---- the whole-curve calls (attribution, summary, quantiles, mechanism, band) ---------------------------------------------------------------
def _same(a, b, equal_nan):
    """Bitwise agreement of two numpy arrays: dtype, shape, every element; ``equal_nan``: whether a NaN agrees with a NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=equal_nan)


def _per_draw_curves(eng, flat, c, is_post, obs_d, labels):
    """[K, Q, B, C, T] fp32: the kernel's own curve of every draw -- recon_moments with num_samples = 1 on that draw's noise row."""
    eps = c["eps"].to(DEV)
    return np.stack([_recon_moments(eng, flat, c, is_post, eps=eps[k].contiguous(), obs_d=obs_d, labels=labels, ns=1)[0].cpu().numpy()
                     for k in range(eps.shape[0])])


def _model_curves(m, batch, is_post, eps, heads_axis=0):
    """[Q, ns, B, C, T] fp64 (``heads_axis`` = 1: [ns, Q, B, C, T]): the model's own decoder on the same draws (recon_samples)."""
    res = m.recon_samples(is_post=is_post, num_samples=eps.shape[0], eps=eps, **batch)
    return np.stack([res[n].double().permute(3, 0, 1, 2).cpu().numpy() for n in m.MOMENT_HEADS[bool(m.GAUSS)]], heads_axis)


def _count_calls(monkeypatch, eng, name, note=lambda args: 1):
    """The list that takes ``note(positional arguments)`` of every call of the engine method ``name`` from now on."""
    calls, real = [], getattr(eng, name)
    monkeypatch.setattr(eng, name, lambda *a, **k: (calls.append(note(a)), real(*a, **k))[1])
    return calls
