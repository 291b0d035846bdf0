"""Time the label evidence against the composed route, in ONE process: slode_label_evidence (V hypotheses, one encoder pass, K solves per
trajectory) against V calls of slode_traj_bounds on the batch with its labels replaced by each hypothesis (V encoder passes, V K solves) --
existing code, not the code under test.  Shape: the metric shape (cvs, B = 1024, T = 200, rk4); K in {8, 200} x V in {4, 16}; in-kernel
noise.  Device events around each leg on the current stream; warmed; the two legs ALTERNATE `--rounds` times and each reports its median and
its spread (max - min) in milliseconds.  Also the kernels of one fused call from slode_profile_read, and -- from the same generator state --
whether column v of the fused result is bitwise the v-th composed call.  Prints one JSON line; --out writes it to a file.

    python tools/label_evidence_bench.py --out profiles/label_evidence.json
"""
import torch

import eval_bench as EB

SHAPES = {
    "metric_cvs_B1024_T200_rk4": ("cvs", "mechanistic_cvs", "MechanisticModel", 1024, 200, dict(z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2)),
}
GRID = [(8, 4), (8, 16), (200, 4), (200, 16)]     # (K, V)


def hypotheses(V, dev):
    """V label rows over (iext, rtpr): {0, 1}^2 first, then real-valued rows (the prior nets are linear in the labels)."""
    v = torch.arange(V, device=dev)
    return [((v & 1).float() + 0.25 * (v >> 2).float())[:, None].contiguous(), (((v >> 1) & 1).float() - 0.125 * (v >> 2).float())[:, None].contiguous()]


def run_shape(name, scale, rounds, dev):
    from structured_latent_odes_amd import _lib as L
    m, batch = EB.model_and_batch(SHAPES[name], dev)
    B, T = SHAPES[name][3:5]
    b = m._bind()
    eng, flat = b.engine, b.flat
    own = [batch[l].to(torch.float32).contiguous() for l in m.LABELS]
    res = {"B": B, "T": T, "rounds": rounds, "points": {}}
    for K0, V in GRID:
        K = max(1, K0 // scale)
        hyp = hypotheses(V, dev)
        bt = eng.make_batch(batch["observations"], own, None, particles=K)
        subst = [eng.make_batch(batch["observations"], [t[v:v + 1].expand(B, -1).contiguous() for t in hyp], None, particles=K) for v in range(V)]
        ev = torch.zeros(B, V, L.EVIDENCE_SLOTS, device=dev)
        best = torch.zeros(B, dtype=torch.int32, device=dev)
        loss = torch.zeros(V, K, B, device=dev)
        bounds = torch.zeros(V, B, L.BOUND_SLOTS, device=dev)
        loss_kb = torch.zeros(V, K, B, device=dev)

        def fused():
            return eng.label_evidence(flat, bt, B, K, hyp, V, None, ev, best, loss)

        def composed():
            for v in range(V):
                eng.traj_bounds(flat, subst[v], B, K, bounds[v], loss_kb[v])

        legs = {"label_evidence": fused, "V_traj_bounds_calls": composed}
        pt = {"K": K, "V": V}
        pt.update(EB.alternate(legs, rounds, dev, warm=2, peak=False))
        pt["ratio_composed_over_fused"] = pt["V_traj_bounds_calls"]["median_ms"] / pt["label_evidence"]["median_ms"]
        eng.profile_enable(True)
        fused()
        pt["label_evidence"]["kernels_us"] = eng.profile_read()
        eng.profile_enable(False)
        # the composed calls draw K calls each: give every one the generator state of the fused call
        eng.rng_seed(1)
        fused()
        same = True
        for v in range(V):
            eng.rng_seed(1)
            eng.traj_bounds(flat, subst[v], B, K, bounds[v], loss_kb[v])
            same = same and torch.equal(ev[:, v, :3], bounds[v, :, :3]) and torch.equal(loss[v], loss_kb[v])
        pt["columns_bitwise_equal_to_traj_bounds"] = bool(same)
        res["points"]["K%d_V%d" % (K, V)] = pt
    return res


if __name__ == "__main__":
    EB.main("label_evidence_bench", SHAPES, run_shape, "--shrink", 1)
