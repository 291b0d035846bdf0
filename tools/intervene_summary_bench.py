"""Time the counterfactual summaries (slode_intervene_summary: the curve functionals of every subject under V hypothesised inputs with the
paired effects, folded on chip) in ONE process against
  composed        the composed route of ``MechanisticBase.intervention_summary`` (the same call on observations in a padded tensor, which the
                  engine refuses: V x ``counterfactual_samples`` in chunks and the functionals in torch): the alternative a user has without
                  the call, and
  curve_summary   ONE ``curve_summary`` call on the same shape and noise: a compute yardstick -- the fused call solves V + 1 arms per draw,
                  so (V + 1) x this figure is what the structure predicts.
Shape: the metric shape (cvs, B = 1024, T = 200, rk4), K in {8, 200}, V in {4, 16} (explicit noise, the same rows for every leg; thresholds:
the medians of one posterior draw's central curves; hypotheses: a grid over iext x rtpr).  Device events around each leg on the current stream;
warmed; the legs ALTERNATE ``--rounds`` times and each reports its median, its spread (max - min) and its peak allocation over the allocation
before the call; also the kernels of one fused call from slode_profile_read, the plan's LDS bytes and the largest difference between the fused
and the composed effect means of the continuous slots (a cross-check, not a gate).  Prints one JSON line; --out writes it to a file.

    python tools/intervene_summary_bench.py --rounds 3 --out profiles/intervene_summary.json
"""
import torch

import eval_bench as EB
from pointwise_bench import DRAWS, SHAPES

ARMS = {4: dict(iext=[0.0, 1.0], rtpr=[0.0, 1.0]), 16: dict(iext=[0.0, 0.33, 0.67, 1.0], rtpr=[0.0, 0.33, 0.67, 1.0])}


def run_shape(name, draws, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    eng = m._bind().engine
    obs = batch["observations"]
    wide = torch.zeros(obs.shape[0], obs.shape[1], obs.shape[2] + 3, device=dev)
    wide[:, :, :obs.shape[2]] = obs
    padded = dict(batch, observations=wide[:, :, :obs.shape[2]])      # the same values, a row stride no fused call takes
    central = m.MOMENT_HEADS[bool(m.GAUSS)][0]
    res = {"B": B, "T": T, "rounds": rounds, "lds_bytes": {"V%d" % V: eng.intervene_summary_plan(B, V) for V in ARMS}, "draws": {}}
    for K in (DRAWS if draws <= 0 else (draws,)):
        eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        one = m.recon_samples(is_post=True, num_samples=1, eps=eps[:1], **batch)[central]
        thr = one.permute(1, 0, 2, 3).reshape(one.shape[1], -1).median(dim=1).values.tolist()
        res.setdefault("thresholds", thr)
        for V, grid in ARMS.items():
            hyp = m.label_grid(**grid)
            kw = dict(num_samples=K, hypotheses=hyp, thresholds=thr, sense="above", eps=eps)
            legs = {"fused": lambda: m.intervention_summary(**kw, **batch),
                    "curve_summary": lambda: m.curve_summary(is_post=True, num_samples=K, thresholds=thr, sense="above", eps=eps, **batch),
                    "composed": lambda: m.intervention_summary(**kw, **padded)}
            pt = EB.alternate(legs, rounds, dev, warm=1, peak=True)
            pt["ratio_composed_over_fused"] = pt["composed"]["median_ms"] / pt["fused"]["median_ms"]
            pt["ratio_fused_over_arms_times_curve_summary"] = pt["fused"]["median_ms"] / ((V + 1) * pt["curve_summary"]["median_ms"])
            for leg, last in (("fused", "intervene_summary"), ("curve_summary", "curve_summary")):
                eng.profile_enable(True)
                got = legs[leg]()
                pt[leg]["kernels_us"] = eng.profile_read()
                assert [k for k, _ in pt[leg]["kernels_us"]] == ["weff", "enc_fwd2", last], "the %s leg did not take the one engine call" % leg
                eng.profile_enable(False)
                if leg == "fused":
                    fused = got
            pt["ratio_kernel_over_arms_times_curve_summary_kernel"] = pt["fused"]["kernels_us"][-1][1] / ((V + 1) * pt["curve_summary"]["kernels_us"][-1][1])
            want = legs["composed"]()
            pt["max_abs_difference_fused_composed_effect"] = {
                k: float((fused[central]["effect"][k][0] - want[central]["effect"][k][0]).abs().max().item()) for k in ("peak", "trough", "auc")}
            res["draws"]["K%d_V%d" % (K, V)] = pt
    return res


if __name__ == "__main__":
    EB.main("intervene_summary_bench", SHAPES, run_shape, "--draws", 0)
