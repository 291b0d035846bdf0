"""What the GPU tests of the four eval-side calls (test_gpu_eval_stats, test_gpu_recon_moments, test_gpu_traj_bounds, test_gpu_intervene)
share: an engine for a seeded case (tests/eval_stats_util.py) with the handle's environment switches under control, and the case's batch
on the device.  A plain module: not a conftest, not imported by the product."""
import torch

DEV = torch.device("cuda:0")
WIDTHS = {"cvs": (1, 1), "challenge": (1, 1), "proc": (3, 4, 1, 1)}
ENV_KEYS = ("SLODE_ODE_LOOP", "SLODE_ODE_GRID", "SLODE_ODE_GENERIC", "SLODE_ODE_ALG", "SLODE_ODE_PACK", "SLODE_FOLD_NEXT", "SLODE_NO_FOLD")
ADAPTIVE = ("dopri5", "bosh3", "fehlberg2", "adaptive_heun")


def _engine(c, monkeypatch=None, env=None, solver=None):
    from structured_latent_odes_amd import engine as E
    if monkeypatch is not None:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
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


def _eps_dev(eps):
    return (eps[0] if eps.shape[0] == 1 else eps).to(DEV).contiguous()       # one draw: [B, L], as make_batch takes it
