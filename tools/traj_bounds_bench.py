"""Time the per-trajectory bounds against the only existing call that scores K draws per trajectory, in ONE process: the loss-only
slode_svi_step with particles = K (which yields the batch SUM alone: one scalar) against slode_traj_bounds (the K per-draw losses of every
trajectory and their four summaries).  Shapes: the metric shape (cvs, B = 1024, T = 200, rk4) and config[4]'s shard (challenge-Gauss,
B = 512, T = 300, rk4), K = 64, in-kernel noise.  Device events around each call on the current stream; warmed; the two legs ALTERNATE
`--rounds` times and each reports its median and its spread (max - min) in milliseconds.  Also the kernels of one call of each leg from
slode_profile_read.  Prints one JSON line; --out writes it to a file.

    python tools/traj_bounds_bench.py --out profiles/traj_bounds.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
    "config4_challenge_gauss_B512_T300_rk4": ("challenge", "mechanistic_challenge_Gauss", "MechanisticModelGauss", 512, 300, dict()),
}


def _timed(fn, dev):
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def run_shape(name, K, rounds, dev):
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd import configs as CF
    from structured_latent_odes_amd.synthetic import synthetic_batch
    fam, mod, cls, B, T, kw = SHAPES[name]
    cfg = getattr(CF, "load_config_" + fam)()
    cfg.update(seq_len=T, solver="rk4", num_particles=1, **kw)
    torch.manual_seed(3)
    obs, labels, times = synthetic_batch(fam, B, T, cfg.obs_dim, seed=7)
    m = getattr(importlib.import_module("structured_latent_odes_amd.models." + mod), cls)(cfg, dev, times.to(dev))
    b = m._bind()
    eng, flat = b.engine, b.flat
    labs = [labels[l].to(dev).reshape(B, -1).to(torch.float32).contiguous() for l in m.LABELS]
    bt = eng.make_batch(obs.to(dev), labs, None, particles=K)
    loss_out = torch.zeros(1, device=dev)
    bounds = torch.zeros(B, L.BOUND_SLOTS, device=dev)
    loss_kb = torch.zeros(K, B, device=dev)
    legs = {"svi_step_loss_only_particles_K": lambda: eng.svi_step(L.SVI_MAIN, flat, bt, B, loss_out, None, particles=K),
            "traj_bounds": lambda: eng.traj_bounds(flat, bt, B, K, bounds, loss_kb)}
    res = {"B": B, "T": T, "K": K, "rounds": rounds}
    for leg in legs.values():                                      # warm: workspaces, per-shape set-up, code objects
        leg()
        leg()
    t = {k: [] for k in legs}
    for _ in range(rounds):                                        # alternating legs
        for k, leg in legs.items():
            t[k].append(_timed(leg, dev))
    for k, v in t.items():
        res[k] = {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "all_ms": v}
    eng.profile_enable(True)
    for k, leg in legs.items():
        leg()
        res[k]["kernels_us"] = eng.profile_read()
    eng.profile_enable(False)
    # the two legs score the same K draws when they start from the same generator state: the sum of the -ELBO slot is the step's loss
    eng.rng_seed(1)
    legs["svi_step_loss_only_particles_K"]()
    eng.rng_seed(1)
    legs["traj_bounds"]()
    res["loss_svi_step"] = float(loss_out.item())
    res["sum_of_elbo_slot"] = float(bounds[:, 0].double().sum().item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": "traj_bounds_bench", "device": torch.cuda.get_device_name(dev),
           "shapes": {n: run_shape(n, a.draws, a.rounds, dev) for n in SHAPES}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
