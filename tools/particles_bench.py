#!/usr/bin/env python3
"""What K particles cost: step time of one training step (slode_svi_step with Adam, in-kernel noise) for K in {1, 2, 4, 8} at the
metric shape (cvs, B = 1024, T = 200, rk4) and at BASELINE config[2] (proc, B = 4096, T = 100, dopri5), by device events over a window
of at least 0.5 s after warm-up, with the per-kernel times of one profiled step (Engine.profile_read).  Beside each K: K x the
one-particle step, and one one-particle step at batch B * K, measured in the same call.  Prints one JSON line per row.

  python tools/particles_bench.py [--shape metric|c2|both] [--window 0.5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import slode_oracle as O                                   # noqa: E402
from structured_latent_odes_amd import _lib as L                       # noqa: E402
from structured_latent_odes_amd import engine as E                     # noqa: E402
from structured_latent_odes_amd.svi import FlatAdam                    # noqa: E402

SHAPES = {"metric": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2, solver="rk4"), 1024, 200, 5),
          "c2": ("proc", dict(z_g=10, z_eps=10, solver="dopri5"), 4096, 100, 8)}


def time_step(fam, kw, B, T, S, K, window):
    dev = torch.device("cuda:0")
    ospec = {"cvs": O.cvs_spec, "proc": O.proc_spec}[fam](**kw)
    eng = E.Engine({"cvs": E.cvs_spec, "proc": E.proc_spec}[fam](**kw), T, dev)
    obs, u, _, times = O.synthetic_batch(ospec, B, T)
    eng.set_times(times)
    eng.rng_seed(1)
    flat = eng.pack(O.init_params(ospec, T=T, S=S))
    obs_d = obs.contiguous().to(dev) if fam == "proc" else obs.permute(0, 2, 1).contiguous().to(dev).permute(0, 2, 1)
    bt = eng.make_batch(obs_d, [u.to(dev).contiguous()], None, particles=K)
    opt = FlatAdam(eng, flat, lr=1e-4)
    loss, grads = torch.zeros(1, device=dev), torch.zeros(eng.n_params, device=dev)

    def step():
        opt.t += 1
        eng.svi_step(L.SVI_MAIN, flat, bt, B, loss, grads, adam=(opt.exp_avg, opt.exp_avg_sq, opt.lr, opt.t, opt.betas, opt.eps), particles=K)

    for _ in range(30):
        step()
    torch.cuda.synchronize()
    n, ms = 50, 0.0
    while True:                                                         # grow the block until it covers the window
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1e3 * window:
            break
        n *= 2
    eng.profile_enable(True)
    step()
    kern = {k: round(v, 2) for k, v in eng.profile_read()}
    eng.profile_enable(False)
    assert torch.isfinite(loss).all()
    return 1e3 * ms / n, n, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["metric", "c2", "both"])
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    for name in (["metric", "c2"] if a.shape == "both" else [a.shape]):
        fam, kw, B, T, S = SHAPES[name]
        base = None
        for K in (1, 2, 4, 8):
            us, n, kern = time_step(fam, kw, B, T, S, K, a.window)
            base = us if K == 1 else base
            row = dict(shape=name, B=B, K=K, us_per_step=round(us, 2), steps_timed=n, k_times_one_particle_us=round(K * base, 2), kernels_us=kern)
            if K > 1 and (kw["solver"] != "dopri5" or B * K <= 65536):
                row["one_particle_at_batch_BK_us"] = round(time_step(fam, kw, B * K, T, S, 1, a.window)[0], 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
