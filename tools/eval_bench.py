"""What the benches of the eval-side calls share -- the moment calls' recon_moments_bench, intervene_bench, forecast_bench, cohort_bench,
calibration_bench; the scored-draw calls' traj_bounds_bench, label_evidence_bench, refine_bench, pointwise_bench; the whole-curve calls'
attribution_bench, summary_bench, quantile_bench, mechanism_bench, joint_band_bench; and, for the model and the tail, stats_pass_bench:
the model and its batch from a shape tuple, a call timed with device events, the alternating-legs loop with its warm-up and summary, and
the command line with its one JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model_and_batch(shape, dev):
    """``(model, batch)`` of ``shape`` = (family, model module, class, B, T, config overrides): the family's config at rk4 with one
    particle, weights from torch.manual_seed(3), the synthetic batch of seed 7 on ``dev`` with every label as ``[B, width]``."""
    from structured_latent_odes_amd import configs as CF
    from structured_latent_odes_amd.synthetic import synthetic_batch
    fam, mod, cls, B, T, kw = shape
    cfg = getattr(CF, "load_config_" + fam)()
    cfg.update(seq_len=T, solver="rk4", num_particles=1, **kw)
    torch.manual_seed(3)
    obs, labels, times = synthetic_batch(fam, B, T, cfg.obs_dim, seed=7)
    m = getattr(importlib.import_module("structured_latent_odes_amd.models." + mod), cls)(cfg, dev, times.to(dev))
    batch = {"observations": obs.to(dev)}
    batch.update({k: v.to(dev).reshape(B, -1) for k, v in labels.items()})
    return m, batch


def timed(fn, dev):
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


def alternate(legs, rounds, dev, warm=1, peak=True):
    """``{leg: {median_ms, spread_ms, all_ms[, peak_bytes_over_before]}}``: every leg called ``warm`` times (workspaces, per-shape set-up,
    allocator, code objects), then the legs in turn, ``rounds`` times; spread = max - min."""
    for leg in legs.values():
        for _ in range(warm):
            leg()
    t, mem = {k: [] for k in legs}, {k: 0 for k in legs}
    for _ in range(rounds):
        for k, leg in legs.items():
            ms, over = timed(leg, dev)
            t[k].append(ms)
            mem[k] = max(mem[k], over)
    res = {k: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "all_ms": v} for k, v in t.items()}
    if peak:
        for k in res:
            res[k]["peak_bytes_over_before"] = mem[k]
    return res


def main(tool, shapes, run_shape, count, default):
    """The command line of a bench -- ``count`` (its draw or batch count, with ``default``), --rounds, --out -- and its result:
    ``run_shape(name, count, rounds, dev)`` of every shape as one JSON line, printed and written to --out."""
    ap = argparse.ArgumentParser()
    ap.add_argument(count, type=int, default=default)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": tool, "device": torch.cuda.get_device_name(dev),
           "shapes": {n: run_shape(n, getattr(a, count.lstrip("-")), a.rounds, dev) for n in shapes}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
