"""Time the per-condition curves of the evaluation notebooks three ways, in ONE process:
  fused     MechanisticBase.cohort_moments (one slode_cohort_moments call), at chunk in {0, 1, 8, 64}
  moments   MechanisticBase.recon_moments followed by a torch segmented reduction (index_add over the cohort ids of the per-trajectory
            means and variances): what the library offered before the call existed
  samples   MechanisticBase.recon_samples reduced by cohort in fp64 (the composed route of cohort_moments)
Shapes: cvs B = 1024, T = 200, rk4 with 4 cohorts, and proc B = 1024, T = 100, rk4 with 50 cohorts; num_samples = 200, posterior and
prior.  Device events around each call on the current stream; warmed; the legs ALTERNATE `--rounds` times and each reports its median
and its spread (max - min) in milliseconds, and torch.cuda.max_memory_allocated over the allocation before the call.  Also the kernels
of one fused call (chunk = 0) from slode_profile_read.  Prints one JSON line; --out writes it to a file.

    python tools/cohort_bench.py --out profiles/cohort_moments.json
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
    "cvs_B1024_T200_rk4_G4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, 4, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
    "proc_B1024_T100_rk4_G50": ("proc", "mechanistic_proc", "MechanisticModel", 1024, 100, 50, dict()),
}
CHUNKS = (0, 1, 8, 64)


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


def _segmented(m, res, obs, ids, G):
    """The per-trajectory moments of recon_moments reduced by cohort with index_add (fp32, as a user of the parent commit would)."""
    n = torch.bincount(ids, minlength=G).to(torch.float32).view(G, 1, 1)
    add = lambda x: torch.zeros((G,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device).index_add_(0, ids, x)
    out = {}
    for name, (mean_b, sd_b) in res.items():
        mean = add(mean_b) / n
        between = (add(mean_b * mean_b) / n - mean * mean).clamp_min(0)
        out[name] = (mean, (add(sd_b * sd_b) / n + between).sqrt(), between.sqrt())
    out["observations"] = add(obs.contiguous()) / n
    out["l1"] = (out["observations"] - out[m.MOMENT_HEADS[bool(m.GAUSS)][0]][0]).abs().sum(-1)
    return out


def run_shape(name, ns, rounds, dev):
    from structured_latent_odes_amd import configs as CF
    from structured_latent_odes_amd.synthetic import synthetic_batch
    fam, mod, cls, B, T, G, kw = SHAPES[name]
    cfg = getattr(CF, "load_config_" + fam)()
    cfg.update(seq_len=T, solver="rk4", num_particles=1, **kw)
    torch.manual_seed(3)
    obs, labels, times = synthetic_batch(fam, B, T, cfg.obs_dim, seed=7)
    m = getattr(importlib.import_module("structured_latent_odes_amd.models." + mod), cls)(cfg, dev, times.to(dev))
    batch = {"observations": obs.to(dev)}
    batch.update({k: v.to(dev).reshape(B, -1) for k, v in labels.items()})
    lab = {k: v for k, v in batch.items() if k != "observations"}
    ids = torch.arange(B, device=dev) % G
    count = torch.bincount(ids, minlength=G)
    eng = m._bind().engine

    legs = {"fused_chunk%d" % r: (lambda post, r=r: m.cohort_moments(is_post=post, num_samples=ns, cohorts=ids, chunk=r, **batch)) for r in CHUNKS}
    legs["moments"] = lambda post: _segmented(m, m.recon_moments(is_post=post, num_samples=ns, **batch), batch["observations"], ids, G)
    legs["samples"] = lambda post: m._cohort_composed(batch["observations"], post, ns, ids, G, count, None, None, lab)
    res = {"B": B, "T": T, "G": G, "num_samples": ns, "rounds": rounds, "default_chunk": eng.cohort_plan(B, B, G, ns)[0]}
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
        eng.profile_enable(True)
        m.cohort_moments(is_post=post, num_samples=ns, cohorts=ids, **batch)
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
    out = {"tool": "cohort_bench", "device": torch.cuda.get_device_name(dev),
           "shapes": {n: run_shape(n, a.samples, a.rounds, dev) for n in SHAPES}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
