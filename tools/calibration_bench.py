"""Time the calibration pass three ways, in ONE process:
  fused     MechanisticBase.calibration (one slode_calibration call), M = B in one cohort and in 16 cohorts
  moments   MechanisticBase.recon_moments at the same draw count: the same draw loop with heavier per-value work -- both legs that are
            compared with the fused call run code the library had before it
  samples   the composed route of calibration: recon_samples plus torch comparisons and sums
Shape: cvs B = 1024, T = 200, rk4 (the metric shape); num_samples = --samples (200) and 8; posterior and prior.  Device events around each
call on the current stream; warmed; the legs ALTERNATE `--rounds` times and each reports its median and its spread (max - min) in
milliseconds, and torch.cuda.max_memory_allocated over the allocation before the call.  Also the kernels of one fused call per cohort
count from slode_profile_read.  Prints one JSON line; --out writes it to a file.

    python tools/calibration_bench.py --out profiles/calibration.json
"""
import torch

import eval_bench as EB

SHAPES = {
    "cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
}
COHORTS = (1, 16)
SMALL = 8


def run_shape(name, ns, rounds, dev):
    fam, mod, cls, B, T, kw = SHAPES[name]
    m, batch = EB.model_and_batch((fam, mod, cls, B, T, kw), dev)
    lab = {k: v for k, v in batch.items() if k != "observations"}
    eng = m._bind().engine
    ids = {G: torch.arange(B, device=dev) % G for G in COHORTS}
    count = {G: torch.bincount(ids[G], minlength=G) for G in COHORTS}
    res = {"B": B, "T": T, "rounds": rounds, "default_chunk": eng.calibration_plan(B, B, 1, ns)[0]}
    for K in (ns, SMALL):
        legs = {"fused_G%d" % G: (lambda post, G=G: m.calibration(is_post=post, num_samples=K, cohorts=ids[G], num_cohorts=G, **batch)) for G in COHORTS}
        legs["moments"] = lambda post: m.recon_moments(is_post=post, num_samples=K, **batch)
        legs["samples"] = lambda post: m._calibration_composed(batch["observations"], post, K, ids[16], 16, count[16], None, lab)
        out = res["num_samples_%d" % K] = {}
        for post in (True, False):
            key = "posterior" if post else "prior"
            out[key] = EB.alternate({k: (lambda leg=leg: leg(post)) for k, leg in legs.items()}, rounds, dev)
            eng.profile_enable(True)
            for G in COHORTS:
                legs["fused_G%d" % G](post)
                out[key]["fused_G%d_kernels_us" % G] = eng.profile_read()
            eng.profile_enable(False)
    return res


if __name__ == "__main__":
    EB.main("calibration_bench", SHAPES, run_shape, "--samples", 200)
