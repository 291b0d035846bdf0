"""Time the mechanism curves (slode_mechanism_moments: mean and sd over the draws of the state, the production a, the degradation d, the set
point a / d and the net rate a - d x at every grid point, folded on chip) in ONE process against
  recon_moments   the same shape and noise: the ceiling -- it walks the same draw loop, evaluates the same stages and reduces Q C curves
                  instead of up to 5 S -- and
  composed        the composed route of ``MechanisticBase.mechanism_moments`` (the same call on observations in a padded tensor, which the
                  engine refuses: ``solve_ODE`` of num_samples x B latents in chunks, the torch modules ``dynamics.prod`` / ``dynamics.degr``
                  on all grid times, five fp32 reductions): the alternative a user has without the call.
Shape: the metric shape (cvs, B = 1024, T = 200, rk4), K in {8, 200} (explicit noise, the same rows for every leg), all five slots and the
state alone.  Device events around each leg on the current stream; warmed; the legs ALTERNATE ``--rounds`` times and each reports its median,
its spread (max - min) and its peak allocation over the allocation before the call; also the kernels of one fused call from
slode_profile_read, the plan's LDS bytes and the largest difference between the fused and the composed means (a cross-check, not a gate).
Prints one JSON line; --out writes it to a file.

    python tools/mechanism_bench.py --rounds 3 --out profiles/mechanism.json
"""
import torch

import eval_bench as EB
from pointwise_bench import DRAWS, SHAPES


def run_shape(name, draws, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    eng = m._bind().engine
    obs = batch["observations"]
    wide = torch.zeros(obs.shape[0], obs.shape[1], obs.shape[2] + 3, device=dev)
    wide[:, :, :obs.shape[2]] = obs
    padded = dict(batch, observations=wide[:, :, :obs.shape[2]])      # the same values, a row stride no fused call takes
    res = {"B": B, "T": T, "rounds": rounds, "lds_bytes": {"five_slots": eng.mechanism_plan(B, 0x1f), "one_slot": eng.mechanism_plan(B, 0x01)},
           "draws": {}}
    for K in (DRAWS if draws <= 0 else (draws,)):
        eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        kw = dict(is_post=True, num_samples=K, eps=eps)
        legs = {"fused": lambda: m.mechanism_moments(**kw, **batch),
                "fused_state": lambda: m.mechanism_moments(quantities=("state",), **kw, **batch),
                "recon_moments": lambda: m.recon_moments(**kw, **batch),
                "composed": lambda: m.mechanism_moments(**kw, **padded)}
        pt = EB.alternate(legs, rounds, dev, warm=1, peak=True)
        pt["ratio_composed_over_fused"] = pt["composed"]["median_ms"] / pt["fused"]["median_ms"]
        for tag in ("fused", "fused_state"):
            pt["ratio_%s_over_recon_moments" % tag] = pt[tag]["median_ms"] / pt["recon_moments"]["median_ms"]
        for tag, want in (("fused", "mechanism_moments"), ("fused_state", "mechanism_moments"), ("recon_moments", "recon_moments")):
            legs[tag]()
            eng.profile_enable(True)
            got = legs[tag]()
            pt[tag]["kernels_us"] = eng.profile_read()
            eng.profile_enable(False)
            assert [k for k, _ in pt[tag]["kernels_us"]] == ["weff", "enc_fwd2", want], "the %s leg did not take the one engine call" % tag
            if tag == "fused":
                fused = got
        want = legs["composed"]()
        diff = {n: (fused[n][0] - want[n][0]).abs() for n in m.MECHANISM_NAMES}                  # (over the finite entries: a / d overflows where d -> 0)
        pt["max_abs_difference_fused_composed"] = {n: float(torch.where(torch.isfinite(v), v, torch.zeros_like(v)).max().item()) for n, v in diff.items()}
        pt["non_finite_set_point_means"] = int((~torch.isfinite(fused["set_point"][0])).sum().item())
        pt["degradation_min_of_the_means"] = float(fused["degradation"][0].min().item())
        res["draws"]["K%d" % K] = pt
    return res


if __name__ == "__main__":
    EB.main("mechanism_bench", SHAPES, run_shape, "--draws", 0)
