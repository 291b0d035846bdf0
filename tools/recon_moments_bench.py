"""Time the Monte-Carlo summary of `multiple_samples`, materialising against fused, in ONE process: MechanisticBase.recon_samples
followed by mean / std(unbiased=False) over the sample axis (what the evaluation does with the saved arrays) against
MechanisticBase.recon_moments (one slode_recon_moments call).  Shapes: the metric shape (cvs, B = 1024, T = 200, rk4) and config[4]'s
shard (challenge-Gauss, B = 512, T = 300, rk4), num_samples = 200, posterior and prior.  Device events around each call on the current
stream; warmed; the two legs ALTERNATE `--rounds` times and each reports its median and its spread (max - min) in milliseconds, and
torch.cuda.max_memory_allocated over the allocation before the call.  Also the kernels of one fused call from slode_profile_read.
Prints one JSON line; --out writes it to a file.

    python tools/recon_moments_bench.py --out profiles/recon_moments.json
"""
import eval_bench as EB

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
    "config4_challenge_gauss_B512_T300_rk4": ("challenge", "mechanistic_challenge_Gauss", "MechanisticModelGauss", 512, 300, dict()),
}


def run_shape(name, ns, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    names = m.MOMENT_HEADS[bool(m.GAUSS)]

    def baseline(post):
        res = m.recon_samples(is_post=post, num_samples=ns, **batch)
        return {n: (res[n].mean(dim=-1), res[n].std(dim=-1, unbiased=False)) for n in names}

    legs = {"baseline": baseline, "fused": lambda post: m.recon_moments(is_post=post, num_samples=ns, **batch)}
    res = {"B": B, "T": T, "num_samples": ns, "rounds": rounds}
    for post in (True, False):
        key = "posterior" if post else "prior"
        res[key] = EB.alternate({k: (lambda leg=leg: leg(post)) for k, leg in legs.items()}, rounds, dev)
        eng = m._bind().engine
        eng.profile_enable(True)
        m.recon_moments(is_post=post, num_samples=ns, **batch)
        res[key]["fused_call_kernels_us"] = eng.profile_read()
        eng.profile_enable(False)
    return res


if __name__ == "__main__":
    EB.main("recon_moments_bench", SHAPES, run_shape, "--samples", 200)
