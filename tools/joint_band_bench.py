"""Time the simultaneous bands (slode_joint_band: two sweeps over the draws on the same noise -- mean and sd, then every draw's largest
standardised deviation -- and the quantiles of the K deviations, all on chip) in ONE process against
  recon_moments   the same shape and noise: one sweep; two sweeps should cost about twice it -- and
  composed        the composed route of ``MechanisticBase.simultaneous_band`` (the same call on observations in a padded tensor, which the
                  engine refuses: ``recon_samples`` in chunks, torch mean / std / abs / amax / sort): the alternative a user has without the
                  call.
Shape: the metric shape (cvs, B = 1024, T = 200, rk4), K in {8, 200} (explicit noise, the same rows for every leg), levels (0.95,) and eight
levels.  Device events around each leg on the current stream; warmed; the legs ALTERNATE ``--rounds`` times and each reports its median, its
spread (max - min) and its peak allocation over the allocation before the call; also the kernels of one fused call from slode_profile_read,
the plan's LDS bytes, the mean critical value beside z and the mean pointwise joint share, and the largest difference between the fused and
the composed critical values (a cross-check, not a gate).  Prints one JSON line; --out writes it to a file.

    python tools/joint_band_bench.py --rounds 5 --out profiles/joint_band.json
"""
import torch

import eval_bench as EB
from pointwise_bench import DRAWS, SHAPES

ONE, EIGHT = (0.95,), (0.5, 0.8, 0.9, 0.95, 0.975, 0.99, 0.999, 1.0)


def run_shape(name, draws, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    eng = m._bind().engine
    obs = batch["observations"]
    wide = torch.zeros(obs.shape[0], obs.shape[1], obs.shape[2] + 3, device=dev)
    wide[:, :, :obs.shape[2]] = obs
    padded = dict(batch, observations=wide[:, :, :obs.shape[2]])      # the same values, a row stride no fused call takes
    central = m.MOMENT_HEADS[bool(m.GAUSS)][0]
    res = {"B": B, "T": T, "rounds": rounds, "draws": {}}
    for K in (DRAWS if draws <= 0 else (draws,)):
        eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        kw = dict(is_post=True, num_samples=K, eps=eps)
        legs = {"fused": lambda: m.simultaneous_band(levels=ONE, **kw, **batch),
                "fused_eight_levels": lambda: m.simultaneous_band(levels=EIGHT, **kw, **batch),
                "recon_moments": lambda: m.recon_moments(**kw, **batch),
                "composed": lambda: m.simultaneous_band(levels=ONE, **kw, **padded)}
        pt = EB.alternate(legs, rounds, dev, warm=1, peak=True)
        pt["lds_bytes"] = eng.joint_band_plan(B, K)
        pt["ratio_composed_over_fused"] = pt["composed"]["median_ms"] / pt["fused"]["median_ms"]
        pt["ratio_fused_over_recon_moments"] = pt["fused"]["median_ms"] / pt["recon_moments"]["median_ms"]
        for tag, want in (("fused", "joint_band"), ("fused_eight_levels", "joint_band"), ("recon_moments", "recon_moments")):
            legs[tag]()
            eng.profile_enable(True)
            got = legs[tag]()
            pt[tag]["kernels_us"] = eng.profile_read()
            eng.profile_enable(False)
            assert [k for k, _ in pt[tag]["kernels_us"]] == ["weff", "enc_fwd2", want], "the %s leg did not take the one engine call" % tag
            if tag == "fused":
                fused = got
        want = legs["composed"]()
        z = m._band_levels(ONE, K)[0][1]
        pt["band"] = {"z": z, "mean_crit": float(fused[central]["crit"].mean().item()),
                      "mean_pointwise_joint": float(fused[central]["pointwise_joint"].mean().item()),
                      "share_obs_inside": float(fused[central]["obs_inside"].float().mean().item())}
        pt["max_abs_difference_fused_composed_crit"] = float((fused[central]["crit"] - want[central]["crit"]).abs().max().item())
        res["draws"]["K%d" % K] = pt
    return res


if __name__ == "__main__":
    EB.main("joint_band_bench", SHAPES, run_shape, "--draws", 0)
