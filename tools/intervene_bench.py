"""Time the counterfactual curves in ONE process: MechanisticBase.intervention_moments (one slode_intervene_moments call) against
  (b) two recon_moments(is_post=True) calls -- the same number of solves, but they cannot produce the counterfactual arm or the paired sd:
      a yardstick for compute only -- and
  (c) the composed route: counterfactual_samples followed by mean / std(unbiased=False) of the counterfactual arm and of the paired
      difference over the sample axis, built from the calls that existed before this one.
Shapes: the metric shape (cvs, B = 1024, T = 200, rk4) and challenge-Gauss at B = 512, T = 300, rk4; num_samples = 64; every conditional
prior label of the family swapped (rolled by one row).  Device events around each call on the current stream; warmed; the legs ALTERNATE
`--rounds` times and each reports its median and its spread (max - min) in milliseconds, and torch.cuda.max_memory_allocated over the
allocation before the call.  Also the kernels of one fused call from slode_profile_read.  Prints one JSON line; --out writes it to a file.

    python tools/intervene_bench.py --out profiles/intervene_moments.json
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
    "challenge_gauss_B512_T300_rk4": ("challenge", "mechanistic_challenge_Gauss", "MechanisticModelGauss", 512, 300, dict()),
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
    swap = {l: torch.roll(batch[l], 1, 0) for _, ls, _ in m.PRIORS for l in ls}

    def composed():
        res = m.counterfactual_samples(num_samples=ns, intervene=swap, **batch)
        out = {}
        for n in names:
            f, c = res[n]
            d = c - f
            out[n] = (c.mean(dim=-1), c.std(dim=-1, unbiased=False), d.mean(dim=-1), d.std(dim=-1, unbiased=False))
        return out

    legs = {"a_intervene_moments": lambda: m.intervention_moments(num_samples=ns, intervene=swap, **batch),
            "b_two_recon_moments": lambda: (m.recon_moments(is_post=True, num_samples=ns, **batch), m.recon_moments(is_post=True, num_samples=ns, **batch)),
            "c_composed_samples": composed}
    for leg in legs.values():                                      # warm: workspaces, per-shape set-up, allocator
        leg()
    t, mem = {k: [] for k in legs}, {k: 0 for k in legs}
    for _ in range(rounds):                                        # alternating legs
        for k, leg in legs.items():
            ms, peak = _timed(leg, dev)
            t[k].append(ms)
            mem[k] = max(mem[k], peak)
    res = {"B": B, "T": T, "num_samples": ns, "rounds": rounds, "intervened": sorted(swap)}
    res["legs"] = {k: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "all_ms": v, "peak_bytes_over_before": mem[k]} for k, v in t.items()}
    eng = m._bind().engine
    eng.profile_enable(True)
    m.intervention_moments(num_samples=ns, intervene=swap, **batch)
    res["fused_call_kernels_us"] = eng.profile_read()
    assert [k for k, _ in res["fused_call_kernels_us"]] == ["weff", "enc_fwd2", "intervene_moments"], "leg (a) did not take the one engine call"
    m.recon_moments(is_post=True, num_samples=ns, **batch)
    res["one_recon_moments_call_kernels_us"] = eng.profile_read()
    eng.profile_enable(False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": "intervene_bench", "device": torch.cuda.get_device_name(dev),
           "shapes": {n: run_shape(n, a.samples, a.rounds, dev) for n in SHAPES}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
