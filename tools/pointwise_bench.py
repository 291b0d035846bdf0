"""Time the pointwise predictive density (slode_pointwise_density: per-point lppd, mean and variance of the log-likelihood over K posterior
draws, folded on chip) in both weightings against the composed route, in ONE process: ``MechanisticBase._pointwise_composed`` --
``recon_samples`` in chunks of ``MOMENTS_CHUNK_ROWS`` rows, the [rows, C, T, K] curves scored and folded in torch fp64, importance weights
from per-draw losses composed the same way -- and against ``traj_bounds``, the floor of one sweep over the draws.  Shape: the metric shape
(cvs, B = 1024, T = 200, rk4), K in {8, 200} (explicit noise, the same rows for every leg).  Device events around each leg on the current
stream; warmed; the legs ALTERNATE ``--rounds`` times and each reports its median, its spread (max - min) and its peak allocation over the
allocation before the call; also the kernels of one fused call per mode from slode_profile_read and the largest difference between the
fused and the composed planes (same quantity, fp32 on chip against fp64 in torch: a cross-check, not a gate).  Prints one JSON line; --out
writes it to a file.

    python tools/pointwise_bench.py --rounds 3 --out profiles/pointwise.json
"""
import torch

import eval_bench as EB

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200,
                                  dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2, adjoint_solver=False)),
}
DRAWS = (8, 200)


def run_shape(name, draws, rounds, dev):
    from structured_latent_odes_amd import _lib as L
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    b = m._bind()
    eng, flat = b.engine, b.flat
    obs = batch["observations"]
    labels = {l: batch[l] for l in m.LABELS}
    res = {"B": B, "T": T, "rounds": rounds, "draws": {}}
    for K in (DRAWS if draws <= 0 else (draws,)):
        eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        bt = eng.make_batch(obs, [batch[l].to(torch.float32).contiguous() for l in m.LABELS], eps, particles=K)
        legs = {"pointwise_posterior": lambda: eng.pointwise_density(flat, bt, B, K, L.PW_POSTERIOR),
                "pointwise_importance": lambda: eng.pointwise_density(flat, bt, B, K, L.PW_IMPORTANCE),
                "traj_bounds": lambda: eng.traj_bounds(flat, bt, B, K),
                "composed_posterior": lambda: m._pointwise_composed(obs, K, False, None, None, eps, labels),
                "composed_importance": lambda: m._pointwise_composed(obs, K, True, None, None, eps, labels)}
        pt = EB.alternate(legs, rounds, dev, warm=1, peak=True)
        for mode in ("posterior", "importance"):
            pt["ratio_composed_over_fused_" + mode] = pt["composed_" + mode]["median_ms"] / pt["pointwise_" + mode]["median_ms"]
            pt["ratio_fused_%s_over_traj_bounds" % mode] = pt["pointwise_" + mode]["median_ms"] / pt["traj_bounds"]["median_ms"]
            eng.profile_enable(True)
            point, summary, _ = legs["pointwise_" + mode]()
            pt["pointwise_" + mode]["kernels_us"] = eng.profile_read()
            eng.profile_enable(False)
            cpoint, csummary, _ = legs["composed_" + mode]()
            pt["planes_max_abs_difference_" + mode] = [float((point[j] - cpoint[j]).abs().max().item()) for j in range(3)]
            pt["elpd_waic_total_fused_" + mode] = float((summary[:, 0].double() - summary[:, 1].double()).sum().item())
            pt["elpd_waic_total_composed_" + mode] = float((csummary[:, 0].double() - csummary[:, 1].double()).sum().item())
            pt["median_ess_" + mode] = float(summary[:, 7].median().item())
        res["draws"]["K%d" % K] = pt
    return res


if __name__ == "__main__":
    EB.main("pointwise_bench", SHAPES, run_shape, "--draws", 0)
