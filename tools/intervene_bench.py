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
import torch

import eval_bench as EB

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
    "challenge_gauss_B512_T300_rk4": ("challenge", "mechanistic_challenge_Gauss", "MechanisticModelGauss", 512, 300, dict()),
}


def run_shape(name, ns, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
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
    res = {"B": B, "T": T, "num_samples": ns, "rounds": rounds, "intervened": sorted(swap)}
    res["legs"] = EB.alternate(legs, rounds, dev)
    eng = m._bind().engine
    eng.profile_enable(True)
    m.intervention_moments(num_samples=ns, intervene=swap, **batch)
    res["fused_call_kernels_us"] = eng.profile_read()
    assert [k for k, _ in res["fused_call_kernels_us"]] == ["weff", "enc_fwd2", "intervene_moments"], "leg (a) did not take the one engine call"
    m.recon_moments(is_post=True, num_samples=ns, **batch)
    res["one_recon_moments_call_kernels_us"] = eng.profile_read()
    eng.profile_enable(False)
    return res


if __name__ == "__main__":
    EB.main("intervene_bench", SHAPES, run_shape, "--samples", 64)
