"""Time the per-trajectory bounds against the only existing call that scores K draws per trajectory, in ONE process: the loss-only
slode_svi_step with particles = K (which yields the batch SUM alone: one scalar) against slode_traj_bounds (the K per-draw losses of every
trajectory and their four summaries).  Shapes: the metric shape (cvs, B = 1024, T = 200, rk4) and config[4]'s shard (challenge-Gauss,
B = 512, T = 300, rk4), K = 64, in-kernel noise.  Device events around each call on the current stream; warmed; the two legs ALTERNATE
`--rounds` times and each reports its median and its spread (max - min) in milliseconds.  Also the kernels of one call of each leg from
slode_profile_read.  Prints one JSON line; --out writes it to a file.

    python tools/traj_bounds_bench.py --out profiles/traj_bounds.json
"""
import torch

import eval_bench as EB

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
    "config4_challenge_gauss_B512_T300_rk4": ("challenge", "mechanistic_challenge_Gauss", "MechanisticModelGauss", 512, 300, dict()),
}


def run_shape(name, K, rounds, dev):
    from structured_latent_odes_amd import _lib as L
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    b = m._bind()
    eng, flat = b.engine, b.flat
    bt = eng.make_batch(batch["observations"], [batch[l].to(torch.float32).contiguous() for l in m.LABELS], None, particles=K)
    loss_out = torch.zeros(1, device=dev)
    bounds = torch.zeros(B, L.BOUND_SLOTS, device=dev)
    loss_kb = torch.zeros(K, B, device=dev)
    legs = {"svi_step_loss_only_particles_K": lambda: eng.svi_step(L.SVI_MAIN, flat, bt, B, loss_out, None, particles=K),
            "traj_bounds": lambda: eng.traj_bounds(flat, bt, B, K, bounds, loss_kb)}
    res = {"B": B, "T": T, "K": K, "rounds": rounds}
    res.update(EB.alternate(legs, rounds, dev, warm=2, peak=False))
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


if __name__ == "__main__":
    EB.main("traj_bounds_bench", SHAPES, run_shape, "--draws", 64)
