"""Time the forecast moments (slode_forecast_moments) in ONE process, engine level, posterior, num_samples = 64 by default:
  (a) T_out = T, window = 0 against slode_recon_moments on the same batch and noise: the same work -- the cost of the window machinery
  (b) T_out = 4 T (the training grid extended at its last spacing), the default window
  (c) leg (b) with window = 256
  (d) the composed route for (b): MechanisticBase.forecast_samples reduced with mean / std(unbiased=False), where T_out fits
      slode_ode_solve_fwd (at most 1024 points)
Shapes: the metric shape (cvs, B = 1024, T = 200, rk4) and config[4]'s shard (challenge-Gauss, B = 512, T = 300, rk4).  Device events around
each call on the current stream; outputs preallocated, grids built before; warmed; the legs of a group ALTERNATE `--rounds` times and each
reports its median and its spread (max - min) in milliseconds.  Also the kernels of one call per leg from slode_profile_read and the
plan (window, LDS bytes) of each.  Prints one JSON line; --out writes it to a file.  No time is gated.

    python tools/forecast_bench.py --out profiles/forecast_moments.json
"""
import torch

import eval_bench as EB

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
    "config4_challenge_gauss_B512_T300_rk4": ("challenge", "mechanistic_challenge_Gauss", "MechanisticModelGauss", 512, 300, dict()),
}
MAX_COMPOSED_T = 1024     # slode_shape::T of slode_ode_solve_fwd


def run_shape(name, ns, rounds, dev):
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    b = m._bind()
    eng, flat = b.engine, b.flat
    eps = torch.randn(ns, B, m.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
    bt = m._draws_batch(batch["observations"], {k: v for k, v in batch.items() if k != "observations"}, eps, ns)
    Q, C = (1 if m.GAUSS else 3), m.obs_dim
    t_same, t_long = m.horizon_times(0), m.horizon_times(3 * T)
    T_long = int(t_long.numel())
    eng.forecast_grid(t_same), eng.forecast_grid(t_long)
    out_same = [torch.empty(Q, B, C, T, device=dev) for _ in range(2)]
    out_recon = [torch.empty(Q, B, C, T, device=dev) for _ in range(2)]
    out_long = [torch.empty(Q, B, C, T_long, device=dev) for _ in range(2)]
    res = {"B": B, "T": T, "T_long": T_long, "num_samples": ns, "rounds": rounds,
           "plan": {"a_T_out_T_window_0": eng.forecast_plan(B, T, ns), "b_T_out_4T_window_0": eng.forecast_plan(B, T_long, ns),
                    "c_T_out_4T_window_256": eng.forecast_plan(B, T_long, ns, window=256)}}
    same = {"recon_moments": lambda: eng.recon_moments(flat, bt, B, True, ns, *out_recon),
            "a_forecast_T_out_T_window_0": lambda: eng.forecast_moments(flat, bt, B, True, ns, t_same, *out_same)}
    res["same_grid"] = EB.alternate(same, rounds, dev, warm=2, peak=False)
    res["same_grid"]["mean_bitwise_equal"] = bool(torch.equal(out_same[0], out_recon[0]))
    res["same_grid"]["sd_bitwise_equal"] = bool(torch.equal(out_same[1], out_recon[1]))
    long = {"b_forecast_T_out_4T_window_0": lambda: eng.forecast_moments(flat, bt, B, True, ns, t_long, *out_long),
            "c_forecast_T_out_4T_window_256": lambda: eng.forecast_moments(flat, bt, B, True, ns, t_long, *out_long, window=256)}
    if T_long <= MAX_COMPOSED_T:
        names = m.MOMENT_HEADS[bool(m.GAUSS)]

        def composed():
            r = m.forecast_samples(is_post=True, num_samples=ns, times_out=t_long, eps=eps, **batch)
            return {n: (r[n].mean(dim=-1), r[n].std(dim=-1, unbiased=False)) for n in names}
        long["d_composed_T_out_4T"] = composed
    res["long_grid"] = EB.alternate(long, rounds, dev, warm=2, peak=False)
    if T_long > MAX_COMPOSED_T:
        res["long_grid"]["d_composed_T_out_4T"] = "not available: T_out = %d exceeds the %d points slode_ode_solve_fwd takes" % (T_long, MAX_COMPOSED_T)
    eng.profile_enable(True)
    kernels = {}
    for k, leg in list(same.items()) + [(k, v) for k, v in long.items() if k[0] in "bc"]:
        leg()
        kernels[k] = eng.profile_read()
    eng.profile_enable(False)
    res["kernels_us"] = kernels
    return res


if __name__ == "__main__":
    EB.main("forecast_bench", SHAPES, run_shape, "--samples", 64)
