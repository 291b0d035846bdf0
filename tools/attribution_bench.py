"""Time the latent attribution in ONE process: MechanisticBase.latent_attribution, posterior, all blocks (one slode_latent_attribution call
with A arms: cvs 6, challenge 2) against
  (b) (1 + A) recon_moments(is_post=True) calls -- the same number of solves, but they cannot produce a paired difference: a yardstick for
      compute only -- and
  (c) the composed route: the same call on observations in a padded tensor, which the engine refuses, so the dict is composed from the
      decoder's per-draw curves of the base and of every arm, built from the calls that existed before this one.
Shapes: the metric shape (cvs, B = 1024, T = 200, rk4) and challenge-Gauss at B = 512, T = 300, rk4; num_samples = 64.  Device events around
each call on the current stream; warmed; the legs ALTERNATE `--rounds` times and each reports its median and its spread (max - min) in
milliseconds, and torch.cuda.max_memory_allocated over the allocation before the call.  Also the kernels of one fused call from
slode_profile_read and the plan's LDS bytes.  Prints one JSON line; --out writes it to a file.

    python tools/attribution_bench.py --out profiles/latent_attribution.json
"""
import torch

import eval_bench as EB
from intervene_bench import SHAPES


def run_shape(name, ns, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    blocks, masks, _, _ = m._attribution_arms(None)
    obs = batch["observations"]
    wide = torch.zeros(obs.shape[0], obs.shape[1], obs.shape[2] + 3, device=dev)
    wide[:, :, :obs.shape[2]] = obs
    padded = dict(batch, observations=wide[:, :, :obs.shape[2]])      # the same values, a row stride no fused call takes

    legs = {"a_latent_attribution": lambda: m.latent_attribution(is_post=True, num_samples=ns, **batch),
            "b_recon_moments_x_arms_plus_1": lambda: [m.recon_moments(is_post=True, num_samples=ns, **batch) for _ in range(1 + len(masks))],
            "c_composed_draws": lambda: m.latent_attribution(is_post=True, num_samples=ns, **padded)}
    res = {"B": B, "T": T, "num_samples": ns, "rounds": rounds, "blocks": blocks, "arm_masks": masks}
    res["legs"] = EB.alternate(legs, rounds, dev)
    eng = m._bind().engine
    res["lds_bytes"] = eng.attribution_plan(B, len(masks))
    eng.profile_enable(True)
    m.latent_attribution(is_post=True, num_samples=ns, **batch)
    res["fused_call_kernels_us"] = eng.profile_read()
    assert [k for k, _ in res["fused_call_kernels_us"]] == ["weff", "enc_fwd2", "latent_attribution"], "leg (a) did not take the one engine call"
    m.recon_moments(is_post=True, num_samples=ns, **batch)
    res["one_recon_moments_call_kernels_us"] = eng.profile_read()
    eng.profile_enable(False)
    return res


if __name__ == "__main__":
    EB.main("attribution_bench", SHAPES, run_shape, "--samples", 64)
