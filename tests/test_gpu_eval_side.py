"""The eval-side kernels (csrc/misc_kernels.hip: decode_heads, decode_heads_bwd_{x,w}, dynamics_eval, init_state, prior_nets,
label_heads, rng_fill; the inference form of the encoder; the forward-only solves behind slode_ode_solve_fwd) at the engine level:
every row at batch sizes on both sides of the 64- and 256-thread block edges, and at the sizes `recon_samples` produces
(200 x 1024 trajectories; above 65,536 the fixed-grid solve switches to its resident-loop form, above 4,096 the adaptive one to eight
lanes per trajectory).  Outputs are caller-allocated through the raw C ABI, NaN inside, sentinels around (tests/eval_side_util.py).
References: the fp64 oracle, fp64 einsums for the head backward."""
import pytest
import torch
import torch.nn.functional as F

from oracle import slode_oracle as O
from tests import adaptive_rk_ref as R
from tests import eval_side_util as V

pytestmark = pytest.mark.gpu

# Per-row bars (V.row_err: max over rows of |row error| / max(|row|, 1)) = the suite's norm-wise bar of the same op, where 4 x the fp32
# CPU oracle's own per-row distance from the fp64 oracle (same inputs, every shape, every B of V.BLOCK_EDGES) stays under it:
#   op                 suite bar (where)                           fp32-vs-fp64 oracle, worst row      4 x
#   initialize_state   1e-6 (test_eval_side_small_nets)            1.03e-7                              4.1e-7
#   prior loc          1e-6 (same)                                 6.28e-8                              2.5e-7
#   prior scale        1e-6 (same)                                 5.29e-7 (proc: exp of a 9-term sum)  2.1e-6  -> bar 2.2e-6
#   label heads        2e-6 (same)                                 2.13e-7                              8.5e-7
#   decode_heads mu    1e-6 (test_decode_heads)                    5.52e-8                              2.2e-7
#   g_x                2e-5 (test_decode_heads_backward)           6.09e-8                              2.4e-7
#   encoder loc/scale  2e-5 (test_encoder_forward)                 1.26e-6 / 6.38e-7                    5.0e-6
# Not per row (one tensor for the whole batch), norm-wise at the suite's bars: std 1e-6, g_heads 2e-5 (fp32 oracle: 7.5e-7), g_cstd 2e-6.
BAR = dict(x0=1e-6, ploc=1e-6, pscale=2.2e-6, labels=2e-6, mu=1e-6, std=1e-6, g_x=2e-5, g_heads=2e-5, g_cstd=2e-6, loc=2e-5, scale=2e-5)


def _dev(c, d, *keys):
    return [d[k].to(c["dev"]).contiguous() for k in keys]


@pytest.mark.parametrize("shape", list(V.SHAPES))
def test_block_edges_every_row(shape):
    """1a.  initialize_state, prior_nets, label_heads, decode_heads, decode_heads_bwd and encoder_fwd(save=False) at B in {1, 63, 64, 65,
    255, 256, 257, 1023, 1025, 4097}: guarded outputs (no NaN left, sentinels untouched), every row against the fp64 oracle at the
    bars of BAR (table above it: the suite's own bars, except the prior scale: suite 1e-6, the fp32 CPU oracle's worst row 5.29e-7 from
    fp64, bar 4 x that = 2.2e-6)."""
    c = V.case_gpu(shape)
    eng, flat = c["eng"], c["flat"]
    worst = {}
    for B in V.BLOCK_EDGES:
        d = V.inputs(c, B)
        ref = V.references(c, d)
        z, u, x, g_mu, g_std = _dev(c, d, "z", "u", "x", "g_mu", "g_std")
        got = {"x0": V.raw_initialize_state(eng, flat, z), "labels": V.raw_label_heads(eng, flat, z)}
        got["ploc"], got["pscale"] = V.raw_prior_nets(eng, flat, u)
        got["mu"], got["std"] = V.raw_decode_heads(eng, flat, x)
        got["g_x"], got["g_heads"], got["g_cstd"] = V.raw_decode_heads_bwd(eng, flat, x, g_mu, g_std)
        got["loc"], got["scale"] = V.raw_encoder_fwd(eng, flat, V.obs_to_device(c, d["obs"]))
        for k, v in got.items():
            e = V.rel(v, ref[k]) if k in ("std", "g_heads", "g_cstd") else V.row_err(v, ref[k], 1 if k == "mu" else 0)
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < BAR[k], (shape, B, k, e, BAR[k])
    print("%s: worst per-row error over B in %s: %s" % (shape, V.BLOCK_EDGES, {k: "%.2e" % v for k, v in worst.items()}))


@pytest.mark.parametrize("shape", list(V.SHAPES))
def test_dynamics_eval_direct(shape):
    """1a / 1b.  Engine-level slode_dynamics_eval at t in {0, 0.75, -3, 1e3}, state in [0, 1] and in [-1, 2), every B of V.BLOCK_EDGES,
    against O.dynamics in fp64: 2e-6 absolute, every element (the bar of the indirect check in test_module_level_autograd_matches_oracle;
    the fp32 CPU oracle sits 2.7e-7 (state in [0, 1]) / 4.2e-7 (state in [-1, 2)) from fp64 on these inputs: 4 x = 1.1e-6 / 1.7e-6)."""
    c = V.case_gpu(shape)
    worst = 0.0
    for B in V.BLOCK_EDGES:
        d = V.inputs(c, B)
        z, s0, s1 = _dev(c, d, "z", "state", "state_wide")
        for t in (0.0, 0.75, -3.0, 1e3):
            for st_d, st in ((s0, d["state"]), (s1, d["state_wide"])):
                got = V.raw_dynamics_eval(c["eng"], c["flat"], t, st_d, z)
                e = (got.double().cpu() - V.dynamics_ref(c, t, st, d["z"])).abs().max().item()
                worst = max(worst, e)
                assert e < 2e-6, (shape, B, t, e)
    print("%s: dynamics_eval worst absolute error %.2e" % (shape, worst))


def _ulp(v):
    """Spacing of fp32 at |v| (fp64 tensor in, fp64 out), not below the smallest normal's."""
    a = v.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


@pytest.mark.parametrize("shape", ["cvs", "proc"])
def test_sample_normal_is_loc_plus_scale_times_the_drawn_noise(shape):
    """1c.  z = sample_normal(loc, scale) at drawing call n in {0, 1, 2^32 - 1, 2^32} equals loc + scale * rng_normal(n) (fp64, from the
    read-back noise) to 1 ulp of fp32, and moves the counter to n + 1; rng_normal / sample_normal at every B of V.BLOCK_EDGES write
    exactly their rows (guarded) and equal the leading rows of the largest draw bitwise; a handle seeded with first_trajectory = f
    gives rows [f, f + B) of the unsharded draw bitwise; rng_normal at B = 200 x 1024 equals the same rows drawn in 4,096-row chunks."""
    from structured_latent_odes_amd import engine as E
    c = V.case_gpu(shape)
    eng, dev, L = c["eng"], c["dev"], c["L"]
    seed = 20240607
    eng.rng_seed(seed)
    g = torch.Generator().manual_seed(5)
    Bmax = max(V.BLOCK_EDGES)
    loc, scale = torch.randn(Bmax, L, generator=g), torch.exp(0.5 * torch.randn(Bmax, L, generator=g))
    for n in (0, 1, 2 ** 32 - 1, 2 ** 32):
        full = V.raw_rng_normal(eng, n, Bmax).clone()
        assert bool(torch.isfinite(full).all()) and 0.9 < float(full.std()) < 1.1 and abs(float(full.mean())) < 0.05
        for B in V.BLOCK_EDGES:
            eps = V.raw_rng_normal(eng, n, B)
            assert torch.equal(eps, full[:B]), (n, B)
            eng.rng_set_counter(n)
            z = V.raw_sample_normal(eng, loc[:B].to(dev).contiguous(), scale[:B].to(dev).contiguous())
            assert eng.rng_state()[2] == n + 1, (n, eng.rng_state())
            want = loc[:B].double() + scale[:B].double() * eps.double().cpu()
            off = ((z.double().cpu() - want).abs() / _ulp(want)).max().item()
            assert off <= 1.0, (n, B, off)
        if n:
            assert not torch.equal(full, V.raw_rng_normal(eng, 0, Bmax))
    # sharded handle: rows [f, f + B) of the unsharded draw
    f, B = 1000, 300
    shard = E.Engine(eng.spec, c["T"], dev)
    shard.rng_seed(seed, first_trajectory=f)
    n = 7
    full = V.raw_rng_normal(eng, n, f + B).clone()
    assert torch.equal(V.raw_rng_normal(shard, n, B), full[f:])
    shard.rng_set_counter(n)
    eng.rng_set_counter(n)
    lo_d, sc_d = loc[:f + B].to(dev).contiguous(), scale[:f + B].to(dev).contiguous()
    z_full = V.raw_sample_normal(eng, lo_d, sc_d).clone()
    assert torch.equal(V.raw_sample_normal(shard, lo_d[f:].contiguous(), sc_d[f:].contiguous()), z_full[f:])
    assert shard.rng_state() == (seed, f, n + 1)
    # what draw_normal(200 * 1024) asks for, against 4,096-row chunks
    big_B = 200 * 1024
    big = V.raw_rng_normal(eng, 3, big_B)
    for s in range(0, big_B, 4096):
        shard.rng_seed(seed, first_trajectory=s)
        assert torch.equal(V.raw_rng_normal(shard, 3, 4096), big[s:s + 4096]), s
    eng.rng_set_counter(3)
    assert torch.equal(eng.draw_normal(big_B), big) and eng.rng_state()[2] == 4


@pytest.mark.parametrize("shape", ["cvs", "challenge_gauss"])
def test_decode_heads_bwd_corners(shape):
    """1d.  Q = 3 (cvs) and Q = 1 (Gauss): no std gradient (g_cstd comes back as zeros) with and without a parameter snapshot; a snapshot
    taken, then the live parameter vector overwritten with NaN: the backward is that of the snapshot, bit for bit -- the property
    _HeadsFn exists for.  Against fp64 einsums at the bars of test_decode_heads_backward (2e-5; g_x per row)."""
    c = V.case_gpu(shape)
    eng, flat = c["eng"], c["flat"]
    B = 257
    d = V.inputs(c, B)
    ref = V.references(c, d)
    x, g_mu, g_std = _dev(c, d, "x", "g_mu", "g_std")
    assert ref["g_heads"].shape[0] == (1 if shape == "challenge_gauss" else 3)
    base = V.raw_decode_heads_bwd(eng, flat, x, g_mu, g_std)
    snap = eng.heads_snapshot(flat)
    for snapshot in (None, snap):
        g_x, g_heads, g_c = V.raw_decode_heads_bwd(eng, flat, x, g_mu, None, snapshot=snapshot)
        assert torch.equal(g_x, base[0]) and torch.equal(g_heads, base[1])
        assert float(g_c.abs().max()) == 0.0
        assert V.row_err(g_x, ref["g_x"]) < 2e-5 and V.rel(g_heads, ref["g_heads"]) < 2e-5
    with_snap = V.raw_decode_heads_bwd(eng, flat, x, g_mu, g_std, snapshot=snap)
    assert all(torch.equal(a, b) for a, b in zip(with_snap, base))
    live = flat.clone()
    live.fill_(float("nan"))                                   # the optimizer moved on (here: as far as it can)
    got = eng.decode_heads_bwd(live, x, g_mu, g_std, snapshot=snap)
    assert all(torch.equal(a, b) for a, b in zip(got, base))
    assert V.rel(got[2], ref["g_cstd"]) < 2e-6
    assert not bool(torch.isfinite(eng.decode_heads_bwd(live, x, g_mu, g_std)[0]).any())     # (and without the snapshot it is the live vector's)


# ---- 2. the sizes multiple_samples produces ---------------------------------------------------------------------------------------
FWD_TOL = dict(dopri5=(1e-6, 1e-8), bosh3=(1e-7, 1e-9), fehlberg2=(1e-7, 1e-9), adaptive_heun=(1e-6, 1e-8))   # test_gpu_adaptive_methods.FWD_TOL; dopri5: test_dopri5_forward_solution_level
LARGE = ([(s, m) for s in ("cvs", "proc") for m in ("euler", "midpoint", "rk4")]
         + [("cvs", m) for m in ("dopri5", "bosh3", "fehlberg2", "adaptive_heun")] + [("proc", "dopri5")])
CHUNK = 4096


def _recon_samples_z(c, B):
    """z = loc + scale * eps with [ns, 1024, L] noise, flattened sample-major: what recon_samples builds (first B rows)."""
    g = torch.Generator().manual_seed(17)
    nb = 1024
    ns = (B + nb - 1) // nb
    loc, scale = 0.5 * torch.randn(nb, c["L"], generator=g), torch.exp(0.3 * torch.randn(nb, c["L"], generator=g) - 1.0)
    eps = torch.randn(ns, nb, c["L"], generator=g)
    return (loc.unsqueeze(0) + scale.unsqueeze(0) * eps).reshape(ns * nb, c["L"])[:B].contiguous()


@pytest.mark.parametrize("B", [65536, 65537, 200 * 1024])
@pytest.mark.parametrize("shape,method", LARGE)
def test_recon_samples_sizes(shape, method, B):
    """ode_solve + decode_heads at B = 65,536, 65,537 and 200 x 1024 trajectories, guarded outputs.  (a) The whole x / mu equals the same
    calls made in chunks of 4,096 rows (one workgroup per trajectory / sixteen lanes per trajectory) bit for bit (torch.equal):
    trajectories are independent and every launch form runs the same operations in the same order.  (b) At most 96 rows
    (V.oracle_rows) against the fp64 oracle: fixed grid at the suite's trajectory bar, 1e-5 * max(1, |x|); adaptive at
    test_forward_solution_level's bar -- err_gpu < 3 * err_ref + 1e-5 against the tight fp64 solve (rtol 1e-10), err_ref that of the
    fp64 restatement of the method at the engine's tolerances -- and within 1e-3; mu of those rows against fp64 heads applied to the
    returned trajectories, 1e-6 per row (test_decode_heads' bar).  The adaptive cvs cases integrate times * 0.25, as every adaptive cvs
    case of the suite does.  The adaptive bar is tight for adaptive_heun (err_ref 7e-7, so 1.2e-5 in all): it holds only while the
    kernels advance state and clock by the same step (dopri5_kernel.hip: dt = fl(t + dt) - t)."""
    adaptive = method in FWD_TOL
    rtol, atol = FWD_TOL.get(method, (None, None))
    c = V.case_gpu(shape, method, rtol, atol, times_scale=0.25 if (adaptive and shape == "cvs") else 1.0)
    eng, flat, dev = c["eng"], c["flat"], c["dev"]
    z = _recon_samples_z(c, B)
    z_d = z.to(dev)
    x = V.raw_ode_solve(eng, flat, z_d)
    mu, std = V.raw_decode_heads(eng, flat, x)
    assert bool(torch.isfinite(x).all())
    same = True
    for s in range(0, B, CHUNK):
        e = min(B, s + CHUNK)
        xc = eng.ode_solve(flat, z_d[s:e].contiguous())
        mc, sc = eng.decode_heads(flat, x[s:e])
        same = same and torch.equal(xc, x[s:e]) and torch.equal(mc, mu[:, s:e]) and torch.equal(sc, std)
        del xc, mc
    assert same, "whole launch and %d-row chunks differ" % CHUNK
    rows = V.oracle_rows(B)
    assert len(rows) <= 96
    zr = z[rows].double()
    xr = x[rows].double().cpu()
    t64 = c["times"].double()
    if adaptive:
        tight = O.solve_ode(c["p64"], zr, t64, "dopri5", rtol=1e-10, atol=1e-12, per_trajectory=True)
        with R.patched(R.TABLEAUS[method]):
            ref = O.solve_ode(c["p64"], zr, t64, "dopri5", rtol=rtol, atol=atol, per_trajectory=True)
        scale = tight.abs().clamp_min(1.0)
        err_gpu = ((xr - tight).abs() / scale).max().item()
        err_ref = ((ref - tight).abs() / scale).max().item()
        print("%s %s B=%d: %d oracle rows, solution error %.2e (fp64 restatement at the same tolerances %.2e)" % (shape, method, B, len(rows), err_gpu, err_ref))
        assert err_gpu < 3.0 * err_ref + 1e-5, (err_gpu, err_ref)
        assert err_gpu < 1e-3
    else:
        want = O.solve_ode(c["p64"], zr, t64, method)
        err = V.elem_err(xr, want)
        print("%s %s B=%d: %d oracle rows, trajectory error %.2e" % (shape, method, B, len(rows), err))
        assert err < 1e-5, err
    W = [c["p64"]["decoder.%s.0.weight" % n] for n in V.head_names(c)]
    want_mu = torch.stack([F.linear(xr, w).permute(0, 2, 1) for w in W])
    assert V.row_err(mu[:, rows], want_mu, 1) < 1e-6
    assert V.rel(std, F.softplus(c["p64"]["decoder.constant_std"])) < 1e-6
    del x, mu
    torch.cuda.empty_cache()
