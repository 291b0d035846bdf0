"""Accepted steps and times of the adaptive methods (dopri5, bosh3, fehlberg2, adaptive_heun) at the reference shapes, DESIGN 3.3.

For each method and tolerance: one training step (ELBO forward + backward) at cvs B = 1024, T = 200 (config[1]'s shape) and at config[2]
(proc, B = 4096, T = 100, S = 8), the accepted steps per trajectory (Engine.dopri5_step_counts: min / mean / max, number over the record
capacity or out of attempts), and -- when no trajectory overflowed -- the whole step's time (mean of N steps) and the forward-kernel and
reverse-sweep durations of one step (slode_profile_*: each dispatch's begin -> end device timestamps).  One JSON line per case.
Usage: python tools/adaptive_steps.py [method substring] [case substring]"""
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import slode_oracle as O  # noqa: E402
from structured_latent_odes_amd import engine as E  # noqa: E402

CASES = [("cvs B=1024 T=200", "cvs", dict(z_iext=3, z_rtpr=3, z_eps=2), 1024, 200, 5, 0.25),
         ("config[2] B=4096 T=100", "proc", dict(z_g=10, z_eps=10), 4096, 100, 8, 1.0)]
TOLS = [(1e-7, 1e-9), (1e-6, 1e-8), (1e-5, 1e-7), (1e-4, 1e-6)]
METHODS = ["dopri5", "bosh3", "fehlberg2", "adaptive_heun"]


def main():
    only_m = sys.argv[1] if len(sys.argv) > 1 else ""
    only_c = sys.argv[2] if len(sys.argv) > 2 else ""
    dev = torch.device("cuda:0")
    for name, fam, kw, B, T, S, tscale in CASES:
        if only_c not in name:
            continue
        mk_o, mk_e = (O.proc_spec, E.proc_spec) if fam == "proc" else (O.cvs_spec, E.cvs_spec)
        ospec = mk_o(solver="dopri5", **kw)
        p = O.init_params(ospec, T=T, S=S)
        g = torch.Generator().manual_seed(31)
        p = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in p.items()}
        obs, u, eps, times = O.synthetic_batch(ospec, B, T)
        times = times * tscale
        obs_d = obs.contiguous().to(dev) if obs.is_contiguous() else obs.permute(0, 2, 1).contiguous().to(dev).permute(0, 2, 1)
        for method in METHODS:
            if only_m not in method:
                continue
            for rtol, atol in TOLS:
                espec = dataclasses.replace(mk_e(solver=method, **kw), rtol=rtol, atol=atol)
                eng = E.Engine(espec, T, dev)
                eng.set_times(times)
                flat = eng.pack(p)
                loss = torch.zeros(1, device=dev)
                grads = torch.zeros(eng.n_params, device=dev)
                args = (flat, obs_d, u.to(dev), eps.to(dev), loss)
                eng.elbo_step(*args, grads=grads)
                torch.cuda.synchronize()
                n = eng.dopri5_step_counts(B).cpu()
                kmax = max(64, min(2048, (1 << 26) // (B * (S + 2))))
                over, failed = int((n > kmax).sum()), int((n < 0).sum())
                ok = n[(n >= 0)]
                line = dict(case=name, method=method, rtol=rtol, atol=atol, kmax=kmax,
                            steps=[int(ok.min()) if ok.numel() else None, round(float(ok.float().mean()), 1) if ok.numel() else None,
                                   int(ok.max()) if ok.numel() else None],
                            overflow=over, exhausted=failed, loss_finite=bool(torch.isfinite(loss).all()))
                if over == 0 and failed == 0:
                    for _ in range(5):
                        eng.elbo_step(*args, grads=grads)
                    torch.cuda.synchronize()
                    reps = 20
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        eng.elbo_step(*args, grads=grads)
                    e1.record()
                    torch.cuda.synchronize()
                    line["step_ms"] = round(e0.elapsed_time(e1) / reps, 3)
                    eng.profile_enable(True)
                    eng.elbo_step(*args, grads=grads)
                    pr = eng.profile_read()
                    eng.profile_enable(False)
                    line["kernel_us"] = {k: round(v, 1) for k, v in pr if k.startswith("dopri5")}
                print(json.dumps(line), flush=True)
                del eng
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
