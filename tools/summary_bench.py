"""Time the curve summaries (slode_curve_summary: peak, time to peak, area and threshold crossing of every draw's curve, folded on chip),
with and without ``p_beyond``, in ONE process against
  recon_moments   the same shape and noise: the ceiling -- it walks the same draws and reduces less -- and
  composed        the composed route of ``MechanisticBase.curve_summary`` (the same call on observations in a padded tensor, which the engine
                  refuses: ``recon_samples`` in chunks and the functionals in torch): the alternative a user has without the call.
Shape: the metric shape (cvs, B = 1024, T = 200, rk4), K in {8, 200} (explicit noise, the same rows for every leg; thresholds: the medians
of one posterior draw's central curves).  Device events around each leg on the current stream; warmed; the legs ALTERNATE ``--rounds`` times
and each reports its median, its spread (max - min) and its peak allocation over the allocation before the call; also the kernels of one
fused call from slode_profile_read, the plan's LDS bytes and the largest difference between the fused and the composed means of the continuous
slots (a cross-check, not a gate).  Prints one JSON line; --out writes it to a file.

    python tools/summary_bench.py --rounds 3 --out profiles/curve_summary.json
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
    central = m.MOMENT_HEADS[bool(m.GAUSS)][0]
    res = {"B": B, "T": T, "rounds": rounds, "lds_bytes": {"with_p_beyond": eng.curve_summary_plan(B, True), "without": eng.curve_summary_plan(B, False)},
           "draws": {}}
    for K in (DRAWS if draws <= 0 else (draws,)):
        eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        one = m.recon_samples(is_post=True, num_samples=1, eps=eps[:1], **batch)[central]
        thr = one.permute(1, 0, 2, 3).reshape(one.shape[1], -1).median(dim=1).values.tolist()
        res.setdefault("thresholds", thr)
        kw = dict(is_post=True, num_samples=K, thresholds=thr, sense="above", eps=eps)
        legs = {"fused": lambda: m.curve_summary(**kw, **batch),
                "fused_p_beyond": lambda: m.curve_summary(pointwise=True, **kw, **batch),
                "recon_moments": lambda: m.recon_moments(is_post=True, num_samples=K, eps=eps, **batch),
                "composed": lambda: m.curve_summary(**kw, **padded),
                "composed_p_beyond": lambda: m.curve_summary(pointwise=True, **kw, **padded)}
        pt = EB.alternate(legs, rounds, dev, warm=1, peak=True)
        for tag in ("", "_p_beyond"):
            pt["ratio_composed_over_fused" + tag] = pt["composed" + tag]["median_ms"] / pt["fused" + tag]["median_ms"]
            pt["ratio_fused%s_over_recon_moments" % tag] = pt["fused" + tag]["median_ms"] / pt["recon_moments"]["median_ms"]
            eng.profile_enable(True)
            got = legs["fused" + tag]()
            pt["fused" + tag]["kernels_us"] = eng.profile_read()
            assert [k for k, _ in pt["fused" + tag]["kernels_us"]] == ["weff", "enc_fwd2", "curve_summary"], "the fused leg did not take the one engine call"
            eng.profile_enable(False)
        legs["recon_moments"]()
        eng.profile_enable(True)
        legs["recon_moments"]()
        pt["recon_moments"]["kernels_us"] = eng.profile_read()
        eng.profile_enable(False)
        want = legs["composed_p_beyond"]()
        pt["max_abs_difference_fused_composed"] = {k: float((got[central][k][0] - want[central][k][0]).abs().max().item()) for k in ("peak", "trough", "auc")}
        pt["max_abs_difference_fused_composed"]["p_beyond"] = float((got[central]["p_beyond"] - want[central]["p_beyond"]).abs().max().item())
        res["draws"]["K%d" % K] = pt
    return res


if __name__ == "__main__":
    EB.main("summary_bench", SHAPES, run_shape, "--draws", 0)
