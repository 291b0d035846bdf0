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
import torch

import eval_bench as EB

SHAPES = {
    "cvs_B1024_T200_rk4_G4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, 4, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
    "proc_B1024_T100_rk4_G50": ("proc", "mechanistic_proc", "MechanisticModel", 1024, 100, 50, dict()),
}
CHUNKS = (0, 1, 8, 64)


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
    fam, mod, cls, B, T, G, kw = SHAPES[name]
    m, batch = EB.model_and_batch((fam, mod, cls, B, T, kw), dev)
    lab = {k: v for k, v in batch.items() if k != "observations"}
    ids = torch.arange(B, device=dev) % G
    count = torch.bincount(ids, minlength=G)
    eng = m._bind().engine

    legs = {"fused_chunk%d" % r: (lambda post, r=r: m.cohort_moments(is_post=post, num_samples=ns, cohorts=ids, chunk=r, **batch)) for r in CHUNKS}
    legs["moments"] = lambda post: _segmented(m, m.recon_moments(is_post=post, num_samples=ns, **batch), batch["observations"], ids, G)
    legs["samples"] = lambda post: m._cohort_composed(batch["observations"], post, ns, ids, G, count, None, None, lab)
    res = {"B": B, "T": T, "G": G, "num_samples": ns, "rounds": rounds, "default_chunk": eng.cohort_plan(B, B, G, ns)[0]}
    for post in (True, False):
        key = "posterior" if post else "prior"
        res[key] = EB.alternate({k: (lambda leg=leg: leg(post)) for k, leg in legs.items()}, rounds, dev)
        eng.profile_enable(True)
        m.cohort_moments(is_post=post, num_samples=ns, cohorts=ids, **batch)
        res[key]["fused_call_kernels_us"] = eng.profile_read()
        eng.profile_enable(False)
    return res


if __name__ == "__main__":
    EB.main("cohort_bench", SHAPES, run_shape, "--samples", 200)
