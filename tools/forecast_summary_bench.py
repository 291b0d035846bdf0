"""Time the forecast summaries (slode_forecast_summary: peak, AUC and threshold crossing of every draw's curve past the observed window,
folded on chip) in ONE process, posterior, on horizon_times(T) -- the training grid and as many steps again, T_out = 2 T -- from the last
training time on, against
  composed          the composed route of ``MechanisticBase.forecast_summary`` (the same call on observations in a padded tensor, which the
                    engine refuses: ``forecast_samples`` in chunks and the functionals in torch): the alternative a user has without the
                    call -- time and peak allocation over the allocation before the call
  forecast_moments  ONE ``forecast_moments`` call on the same grid and noise: the same solves, per-point moments instead of per-curve ones
and, on the model's own grid with one window and first_point = 0,
  curve_summary     ONE ``curve_summary`` call on the same noise against the fused call there: the same operations -- the cost of the window
                    machinery; the two results are compared bitwise.
Then the window: W = 64, 128, 256 and the whole grid at T_out = 2 T, engine level with preallocated outputs, alternating.
Shape: the metric shape (cvs, B = 1024, T = 200, rk4), K in {8, 200} (explicit noise, the same rows for every leg; thresholds: the medians of
one posterior draw's central curve past the window).  Device events around each leg on the current stream; warmed; the legs of a group
ALTERNATE ``--rounds`` times and each reports its median and its spread (max - min); also the kernels of one fused call from
slode_profile_read, the plan (window, LDS bytes) of every window, and the largest difference between the fused and the composed means of the
continuous slots (a cross-check, not a gate).  Prints one JSON line; --out writes it to a file.  No time is gated.

    python tools/forecast_summary_bench.py --rounds 5 --out profiles/forecast_summary.json
"""
import torch

import eval_bench as EB
from pointwise_bench import DRAWS, SHAPES

WINDOWS = (64, 128, 256, 0)


def run_shape(name, draws, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    b = m._bind()
    eng, flat = b.engine, b.flat
    obs = batch["observations"]
    labels = {k: v for k, v in batch.items() if k != "observations"}
    wide = torch.zeros(obs.shape[0], obs.shape[1], obs.shape[2] + 3, device=dev)
    wide[:, :, :obs.shape[2]] = obs
    padded = dict(batch, observations=wide[:, :, :obs.shape[2]])      # the same values, a row stride no fused call takes
    central = m.MOMENT_HEADS[bool(m.GAUSS)][0]
    Q, C = (1 if m.GAUSS else 3), m.obs_dim
    t_own, t_out = m.horizon_times(0), m.horizon_times(T)
    T_out = int(t_out.numel())
    since = float(t_own[-1])
    i0 = m._first_point(t_out, since)
    eng.forecast_grid(t_own), eng.forecast_grid(t_out)
    res = {"B": B, "T": T, "T_out": T_out, "first_point": i0, "rounds": rounds,
           "plan": {("W%d" % W if W else "whole"): eng.forecast_summary_plan(T_out, W) for W in WINDOWS}, "draws": {}}
    res["plan"]["own_grid"] = eng.forecast_summary_plan(T, 0)
    for K in (DRAWS if draws <= 0 else (draws,)):
        eps = torch.randn(K, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        one = m.forecast_samples(is_post=True, num_samples=1, times_out=t_out, eps=eps[:1], **batch)[central][:, :, i0:]
        thr = one.permute(1, 0, 2, 3).reshape(one.shape[1], -1).median(dim=1).values.tolist()
        res.setdefault("thresholds", thr)
        kw = dict(is_post=True, num_samples=K, times_out=t_out, since=since, thresholds=thr, sense="above", eps=eps)
        legs = {"fused": lambda: m.forecast_summary(**kw, **batch),
                "forecast_moments": lambda: m.forecast_moments(is_post=True, num_samples=K, times_out=t_out, eps=eps, **batch),
                "composed": lambda: m.forecast_summary(**kw, **padded)}
        pt = EB.alternate(legs, rounds, dev, warm=1, peak=True)
        pt["ratio_composed_over_fused"] = pt["composed"]["median_ms"] / pt["fused"]["median_ms"]
        pt["ratio_fused_over_forecast_moments"] = pt["fused"]["median_ms"] / pt["forecast_moments"]["median_ms"]
        for leg, last in (("fused", "forecast_summary"), ("forecast_moments", "forecast_moments")):
            eng.profile_enable(True)
            got = legs[leg]()
            pt[leg]["kernels_us"] = eng.profile_read()
            assert [k for k, _ in pt[leg]["kernels_us"]] == ["weff", "enc_fwd2", last], "the %s leg did not take the one engine call" % leg
            eng.profile_enable(False)
            if leg == "fused":
                fused = got
        want = legs["composed"]()
        pt["max_abs_difference_fused_composed_mean"] = {
            k: float((fused[central][k][0] - want[central][k][0]).abs().max().item()) for k in ("peak", "trough", "auc")}
        # the model's own grid, one window, first_point = 0: curve_summary's operations
        own = {"fused_own_grid": lambda: m.forecast_summary(is_post=True, num_samples=K, times_out=t_own, thresholds=thr, sense="above", eps=eps, **batch),
               "curve_summary": lambda: m.curve_summary(is_post=True, num_samples=K, thresholds=thr, sense="above", eps=eps, **batch)}
        pt["own_grid"] = EB.alternate(own, rounds, dev, warm=1, peak=False)
        pt["own_grid"]["ratio_fused_over_curve_summary"] = pt["own_grid"]["fused_own_grid"]["median_ms"] / pt["own_grid"]["curve_summary"]["median_ms"]
        x, y = own["fused_own_grid"](), own["curve_summary"]()
        pt["own_grid"]["bitwise_equal_to_curve_summary"] = all(
            bool(torch.equal(x[n][k][j].nan_to_num(nan=7e33), y[n][k][j].nan_to_num(nan=7e33))) for n in y for k in m.SUMMARY_NAMES for j in (0, 1))
        # the window, engine level: preallocated outputs, the same batch
        bt = m._draws_batch(obs, labels, eps, K)
        outs = [torch.empty(Q, B, C, 8, device=dev) for _ in range(2)]
        win = {("W%d" % W if W else "whole"): (lambda W=W: eng.forecast_summary(flat, bt, B, True, K, t_out, i0, thr, 1, outs[0], outs[1], W)) for W in WINDOWS}
        pt["windows"] = EB.alternate(win, rounds, dev, warm=1, peak=False)
        eng.profile_enable(True)
        for k, leg in win.items():
            leg()
            pt["windows"][k]["kernel_us"] = eng.profile_read()[-1][1]
        eng.profile_enable(False)
        res["draws"]["K%d" % K] = pt
    return res


if __name__ == "__main__":
    EB.main("forecast_summary_bench", SHAPES, run_shape, "--draws", 0)
