"""Time the Monte-Carlo summary of `multiple_samples`, materialising against fused, in ONE process: MechanisticBase.recon_samples
followed by mean / std(unbiased=False) over the sample axis (what the evaluation does with the saved arrays) against
MechanisticBase.recon_moments (one slode_recon_moments call).  Shapes: the metric shape (cvs, B = 1024, T = 200, rk4) and config[4]'s
shard (challenge-Gauss, B = 512, T = 300, rk4), num_samples = 200, posterior and prior.  Device events around each call on the current
stream; warmed; the two legs ALTERNATE `--rounds` times and each reports its median and its spread (max - min) in milliseconds, and
torch.cuda.max_memory_allocated over the allocation before the call.  Also the kernels of one fused call from slode_profile_read.
Prints one JSON line; --out writes it to a file.

    python tools/recon_moments_bench.py --out profiles/recon_moments.json
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
    """(milliseconds between two device events around fn, peak allocation over the allocation before the call)."""
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    del out
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated(dev) - before


def run_shape(name, ns, rounds, dev):
    from structured_latent_odes_amd import configs as CF
    from structured_latent_odes_amd.synthetic import synthetic_batch
    fam, mod, cls, B, T, kw = SHAPES[name]
    cfg = getattr(CF, "load_config_" + fam)()
    cfg.update(seq_len=T, solver="rk4", num_particles=1, **kw)
    torch.manual_seed(3)
    obs, labels, times = synthetic_batch(fam, B, T, cfg.obs_dim, seed=7)
    m = getattr(importlib.import_module("structured_latent_odes_amd.models." + mod), cls)(cfg, dev, times.to(dev))
    batch = {"observations": obs.to(dev)}
    batch.update({k: v.to(dev).reshape(B, -1) for k, v in labels.items()})
    names = m.MOMENT_HEADS[bool(m.GAUSS)]

    def baseline(post):
        res = m.recon_samples(is_post=post, num_samples=ns, **batch)
        return {n: (res[n].mean(dim=-1), res[n].std(dim=-1, unbiased=False)) for n in names}

    legs = {"baseline": baseline, "fused": lambda post: m.recon_moments(is_post=post, num_samples=ns, **batch)}
    res = {"B": B, "T": T, "num_samples": ns, "rounds": rounds}
    for post in (True, False):
        for leg in legs.values():                                  # warm: workspaces, per-shape set-up, allocator
            leg(post)
        t, mem = {k: [] for k in legs}, {k: 0 for k in legs}
        for _ in range(rounds):                                    # alternating legs
            for k, leg in legs.items():
                ms, peak = _timed(lambda: leg(post), dev)
                t[k].append(ms)
                mem[k] = max(mem[k], peak)
        key = "posterior" if post else "prior"
        res[key] = {k: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "all_ms": v, "peak_bytes_over_before": mem[k]} for k, v in t.items()}
        eng = m._bind().engine
        eng.profile_enable(True)
        m.recon_moments(is_post=post, num_samples=ns, **batch)
        res[key]["fused_call_kernels_us"] = eng.profile_read()
        eng.profile_enable(False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": "recon_moments_bench", "device": torch.cuda.get_device_name(dev),
           "shapes": {n: run_shape(n, a.samples, a.rounds, dev) for n in SHAPES}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
