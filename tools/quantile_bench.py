"""Time the sample quantiles (slode_recon_quantiles: order statistics of every curve value over the draws, the needed ranks kept sorted on
chip) in ONE process against
  recon_moments   the same shape and noise: the floor -- it walks the same draws once and keeps three floats per value -- and
  composed        the composed route of ``MechanisticBase.recon_quantiles`` (the same call on observations in a padded tensor, which the
                  engine refuses: ``recon_samples`` over chunks of trajectories, ``torch.sort`` along the draws, the same rank rule): the
                  alternative a user has without the call.
Shape: the metric shape (cvs, B = 1024, T = 200, rk4), K in {8, 200} (explicit noise, the same rows for every leg).
  band    levels (0.025, 0.975): the auto tile, and the forced tiles that give 2 and 4 sweeps (less LDS per workgroup, more workgroups per CU)
  median  levels (0.5,): the engine at the sweeps the plan chooses (``max_sweeps`` lifted) against the composed route; also at K in
          SCAN, to see where in sweeps the composed route overtakes
Device events around each leg on the current stream; warmed; the legs ALTERNATE ``--rounds`` times and each reports its median, its spread
(max - min) and its peak allocation over the allocation before the call; also the kernels of one fused call from slode_profile_read, the
plans and the largest difference between the fused and the composed band (a cross-check, not a gate).  Prints one JSON line; --out writes
it to a file.

    python tools/quantile_bench.py --rounds 5 --out profiles/recon_quantiles.json
"""
import torch

import eval_bench as EB
from pointwise_bench import DRAWS, SHAPES

BAND, MEDIAN = (0.025, 0.975), (0.5,)
SCAN = (25, 36, 50, 100)        # further draw counts of the median legs: 1, 2, 3 and 5 sweeps at the metric shape (K = 200: 10)


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
    for K in ((DRAWS + SCAN) if draws <= 0 else (draws,)):
        eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        kw = dict(is_post=True, num_samples=K, eps=eps)
        plans = {"band": eng.quantile_plan(B, K, BAND), "median": eng.quantile_plan(B, K, MEDIAN)}
        legs = {"median_fused": lambda: m.recon_quantiles(levels=MEDIAN, max_sweeps=T, **kw, **batch),
                "median_composed": lambda: m.recon_quantiles(levels=MEDIAN, **kw, **padded)}
        if K in DRAWS or draws > 0:
            legs.update({"band_fused": lambda: m.recon_quantiles(levels=BAND, **kw, **batch),
                         "band_fused_2_sweeps": lambda: m.recon_quantiles(levels=BAND, tile=-(-T // 2), **kw, **batch),
                         "band_fused_4_sweeps": lambda: m.recon_quantiles(levels=BAND, tile=-(-T // 4), **kw, **batch),
                         "recon_moments": lambda: m.recon_moments(**kw, **batch),
                         "band_composed": lambda: m.recon_quantiles(levels=BAND, **kw, **padded)})
            plans.update({"band_2_sweeps": eng.quantile_plan(B, K, BAND, -(-T // 2)), "band_4_sweeps": eng.quantile_plan(B, K, BAND, -(-T // 4))})
        pt = EB.alternate(legs, rounds, dev, warm=1, peak=True)
        pt["plans_tile_sweeps_lo_hi_lds"] = plans
        pt["ratio_median_composed_over_fused"] = pt["median_composed"]["median_ms"] / pt["median_fused"]["median_ms"]
        for tag in [t for t in legs if t.endswith("fused") or "sweeps" in t]:
            eng.profile_enable(True)
            got = legs[tag]()
            pt[tag]["kernels_us"] = eng.profile_read()
            assert [k for k, _ in pt[tag]["kernels_us"]] == ["weff", "enc_fwd2", "recon_quantiles"], "the fused leg did not take the one engine call"
            eng.profile_enable(False)
        if "band_fused" in legs:
            pt["ratio_band_composed_over_fused"] = pt["band_composed"]["median_ms"] / pt["band_fused"]["median_ms"]
            pt["ratio_band_fused_over_recon_moments"] = pt["band_fused"]["median_ms"] / pt["recon_moments"]["median_ms"]
            got, want = legs["band_fused"](), legs["band_composed"]()
            pt["max_abs_difference_fused_composed_band"] = float((got[central] - want[central]).abs().max().item())
        res["draws"]["K%d" % K] = pt
    return res


if __name__ == "__main__":
    EB.main("quantile_bench", SHAPES, run_shape, "--draws", 0)
