"""Time PSIS leave-one-out (slode_pointwise_loo: per-point elpd_loo, Pareto khat and lppd over K posterior draws, the M + 1 smallest
log-densities of every point kept sorted on chip, the fit in fp64 in the kernel) against its floor -- ``pointwise_density`` with posterior
weights, one sweep over the same draws with no tail and no fit -- and against the composed route, in ONE process:
``MechanisticBase._loo_composed`` -- ``recon_samples`` in chunks of ``MOMENTS_CHUNK_ROWS`` rows, the [rows, C, T, K] log-densities sorted and
smoothed in torch fp64.  Shape: the metric shape (cvs, B = 1024, T = 200, rk4), K in {8, 64, 200} (explicit noise, the same rows for every
leg).  Device events around each leg on the current stream; warmed; the legs ALTERNATE ``--rounds`` times and each reports its median, its
spread (max - min) and its peak allocation over the allocation before the call.  Also, per K: the plan (tile, sweeps, depth, LDS bytes); the
kernels of one fused call from slode_profile_read; the kernel's draw-loop / finish split -- the same call on noise whose K rows are all
equal runs the same draw loop (every value ties with the cutoff: no tail, no fit, no shift in the sorted buffer), so the difference of the
two ``pointwise_loo`` kernel times is the finish phase plus the buffer's shifts; the largest difference between the fused and the composed
planes (a cross-check, not a gate) and the shares of points with khat > 0.7 and > 0.5.  Prints one JSON line; --out writes it to a file.

    python tools/loo_bench.py --rounds 3 --out profiles/pointwise_loo.json
"""
import torch

import eval_bench as EB
from pointwise_bench import SHAPES

DRAWS = (8, 64, 200)


def _kernel_us(eng, call, name="pointwise_loo"):
    eng.profile_enable(True)
    out = call()
    rows = eng.profile_read()
    eng.profile_enable(False)
    return out, rows, float(sum(us for n, us in rows if n == name))


def run_shape(name, draws, rounds, dev):
    from structured_latent_odes_amd import _lib as L
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    b = m._bind()
    eng, flat = b.engine, b.flat
    obs = batch["observations"]
    labels = {l: batch[l] for l in m.LABELS}
    labs = [batch[l].to(torch.float32).contiguous() for l in m.LABELS]
    res = {"B": B, "T": T, "rounds": rounds, "draws": {}}
    for K in (DRAWS if draws <= 0 else (draws,)):
        eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        bt = eng.make_batch(obs, labs, eps, particles=K)
        flat_eps = eps[:1].expand(K, -1, -1).contiguous()
        bt_flat = eng.make_batch(obs, labs, flat_eps, particles=K)
        legs = {"fused": lambda: eng.pointwise_loo(flat, bt, B, K),
                "pointwise_density_posterior": lambda: eng.pointwise_density(flat, bt, B, K, L.PW_POSTERIOR),
                "composed": lambda: m._loo_composed(obs, K, None, None, eps, labels)}
        pt = EB.alternate(legs, rounds, dev, warm=1, peak=True)
        pt["plan"] = dict(zip(("tile", "sweeps", "depth", "lds_bytes"), eng.loo_plan(B, K)))
        pt["ratio_composed_over_fused"] = pt["composed"]["median_ms"] / pt["fused"]["median_ms"]
        pt["ratio_fused_over_pointwise_density"] = pt["fused"]["median_ms"] / pt["pointwise_density_posterior"]["median_ms"]
        (point, summary, _), rows, us = _kernel_us(eng, legs["fused"])
        pt["fused"]["kernels_us"] = rows
        _, _, us_flat = _kernel_us(eng, lambda: eng.pointwise_loo(flat, bt_flat, B, K))
        _, _, us_floor = _kernel_us(eng, legs["pointwise_density_posterior"], "pointwise_density")
        pt["kernel_split_us"] = {"pointwise_loo": us, "draw_loop_all_rows_equal": us_flat, "finish_and_shifts": us - us_flat,
                                 "pointwise_density_kernel": us_floor}
        cpoint, csummary, _ = legs["composed"]()
        fin = torch.isfinite(point[1]) & torch.isfinite(cpoint[1])
        pt["elpd_loo_max_abs_difference"] = float((point[0] - cpoint[0]).abs().max().item())
        pt["khat_max_abs_difference"] = float((point[1] - cpoint[1])[fin].abs().max().item()) if bool(fin.any()) else 0.0
        pt["lppd_max_abs_difference"] = float((point[2] - cpoint[2]).abs().max().item())
        pt["elpd_loo_total_fused"] = float(summary[:, 0].double().sum().item())
        pt["elpd_loo_total_composed"] = float(csummary[:, 0].double().sum().item())
        pt["share_khat_above_0.7"] = float((point[1] > 0.7).float().mean().item())
        pt["share_khat_above_0.5"] = float((point[1] > 0.5).float().mean().item())
        res["draws"]["K%d" % K] = pt
    return res


if __name__ == "__main__":
    EB.main("loo_bench", SHAPES, run_shape, "--draws", 0)
