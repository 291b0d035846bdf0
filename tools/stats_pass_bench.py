"""Time one statistics pass of the epoch loop, unfused against fused, in ONE process: training.input_pred_stats (evaluate_loss x 2, recon,
label prediction: five to seven read-backs per batch) against training.input_pred_stats_fused (one slode_eval_stats call per batch, one
read-back per pass).  Shapes: the metric shape (cvs, B = 1024, T = 200, rk4) and config[4]'s shard (challenge-Gauss, B = 512, T = 300,
rk4).  A pass = 50 batches already on the device; warmed; device-synchronised at both ends; the two legs ALTERNATE `--rounds` times and each
leg reports its median and its spread (max - min) in microseconds per batch, posterior and prior.  Also the kernels of one fused call
from slode_profile_read.  Prints one JSON line; --out writes it to a file.

    python tools/stats_pass_bench.py --out profiles/eval_stats_pass.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stats_pass_bench.py --rounds 1      # the kernel's time on the profiler's clock
"""
import statistics
import time

import torch

import eval_bench as EB

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
    "config4_challenge_gauss_B512_T300_rk4": ("challenge", "mechanistic_challenge_Gauss", "MechanisticModelGauss", 512, 300, dict()),
}


def _pass_us(fn, n_batches, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e6 * (time.perf_counter() - t0) / n_batches


def run_shape(name, n_batches, rounds, dev):
    from structured_latent_odes_amd import training as TR
    from structured_latent_odes_amd.svi import SVI
    fam, B, T = SHAPES[name][0], *SHAPES[name][3:5]
    m, one = EB.model_and_batch(SHAPES[name], dev)
    batches = [one] * n_batches                                    # already on the device, labels [B, width]: batch_to_device is a no-op copy
    losses = [SVI(m.model, m.guide, None), SVI(m.model_meta, m.guide_meta, None)]
    legs = {"baseline": lambda post: TR.input_pred_stats(batches, m, losses, post, dev, fam),
            "fused": lambda post: TR.input_pred_stats_fused(batches, m, post, dev, fam)}
    res = {"B": B, "T": T, "batches_per_pass": n_batches, "rounds": rounds}
    for post in (True, False):
        for leg in legs.values():                                  # warm: workspaces, per-shape set-up
            leg(post)
        t = {k: [] for k in legs}
        for _ in range(rounds):                                    # alternating legs
            for k, leg in legs.items():
                t[k].append(_pass_us(lambda: leg(post), n_batches, dev))
        key = "posterior" if post else "prior"
        res[key] = {k: {"median_us_per_batch": statistics.median(v), "spread_us_per_batch": max(v) - min(v), "all": v} for k, v in t.items()}
        res[key]["faster_by_more_than_baseline_spread"] = bool(
            res[key]["baseline"]["median_us_per_batch"] - res[key]["fused"]["median_us_per_batch"] > res[key]["baseline"]["spread_us_per_batch"])
    eng = m._bind().engine
    eng.profile_enable(True)
    m.eval_stats(is_post=True, **one)
    res["fused_call_kernels_us"] = eng.profile_read()
    eng.profile_enable(False)
    return res


if __name__ == "__main__":
    EB.main("stats_pass_bench", SHAPES, run_shape, "--batches", 50)
