"""GPU tests of the simultaneous bands (slode_joint_band; Engine.joint_band; MechanisticModel.simultaneous_band).

What is exact and what has a bar (tests/band_util.py).  mean and sd are the bits of slode_recon_moments on the same noise.  A deviation is two
correctly rounded fp32 operations per point and a selection over time; a critical value is a selection among the K deviations; a joint share
is a count over them: on the kernel's own curve values -- those slode_recon_moments returns for one draw -- and the call's own mean and sd
all of them are held to numpy EXACTLY.  Against the fp64 oracle a deviation is held to BU.dev_bar, the recon_moments bars carried through
the quotient, a critical value to the largest such bar over the draws of its curve, and a count may differ only by the draws within their
bar of z.  That bar is 0.01 .. 0.12 of a deviation's unit on these cases (tests/test_band_cpu.py prints the oracle's figures), which puts
0.5 .. 5 % of the draws near an informative z: the near share is asserted under BU.NEAR_SHARE at BU.CLEAR_LEVEL, where no draw can be near,
and the rule that only near draws may differ is applied at the informative levels BU.COUNT_LEVELS with the share printed.

Worst error / bar measured on an MI355X (test_against_the_fp64_oracle, all cases, both sides, K = 7 and 33): deviation 7.3e-3, critical value
2.2e-3, observed deviation 1.5e-3; near share at the informative levels 0.7 .. 4.8 %.  The bars are not tightened to these."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import band_util as BU
from tests import eval_stats_util as EU
from tests import mechanism_util as MU
from tests import recon_moments_util as RU
from tests import summary_util as SU
from tests.eval_gpu_util import (ADAPTIVE, DEV, _captured, _count_calls, _device_batch, _engine, _eps_dev, _model, _model_curves, _padded, _peak,
                                 _per_draw_curves, _recon_moments, _refused, _same as _same_arrays, _set_env)
from tests.eval_gpu_util import _band, _band_check_exact as _check_exact, _band_check_oracle as _check_oracle, _band_outs as _outs

pytestmark = pytest.mark.gpu
FILL = BU.FILL
LEVELS = (0.95, 0.5, 1.0, 0.1)
CASES = ["cvs_ald", "proc_gauss", "challenge_gauss", "proc_ald"]


_same = functools.partial(_same_arrays, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _per_draw(case, is_post, ns=7):
    """Computed once, shared: B = 13, explicit eps; the kernel's own fp32 curves per draw and one call of the band."""
    c = RU.build(case, "rk4", B=13, ns=ns)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    return c, eng, flat, _per_draw_curves(eng, flat, c, is_post, obs_d, labels), _band(eng, flat, c, is_post, obs_d=obs_d, labels=labels)


@functools.lru_cache(maxsize=None)
def _oracle(case, ns, is_post):
    return SU.oracle_draws(RU.build(case, "rk4", B=13, ns=ns), is_post)            # [Q, ns, B, C, T]


# ---- 1. the bits of recon_moments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", CASES)
def test_mean_and_sd_are_the_bits_of_recon_moments(case, is_post):
    for ns in (7, 33):
        c = RU.build(case, "rk4", B=13, ns=ns)
        eng = _engine(c)
        flat = eng.pack(c["p"])
        r = _band(eng, flat, c, is_post)
        mean, sd = _recon_moments(eng, flat, c, is_post)
        assert _same(r["mean"], mean.cpu().numpy()) and _same(r["sd"], sd.cpu().numpy()), (case, ns)
        assert np.all(r["points"] == c["T"])


# ---- 2. exact against the kernel's own curves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", CASES)
def test_exact_against_the_kernels_own_curves(case, is_post):
    """dev_out equals max_t fl(fl(|v - m|) / s) on the per-draw curves of recon_moments(num_samples = 1) with the call's own mean and sd;
    crit equals np.sort(dev)[r - 1]; joint equals the counts over K; obs_dev equals its restatement; points == T.  K = 7."""
    c, eng, flat, curves, r = _per_draw(case, is_post)
    _check_exact(r, curves, c["obs"].numpy(), LEVELS, 0.0, (case, is_post))
    assert np.all(r["points"] == c["T"]) and np.all(r["dev"] > 0.0) and np.all(r["dev"] <= np.float32(math.sqrt(6.0) * (1 + 1e-5)))
    assert np.array_equal(r["crit"][..., 2], r["dev"].max(-1)) and np.array_equal(r["crit"][..., 3], r["dev"].min(-1)) and np.all(r["joint"][..., 2] == 1.0)


def test_exact_at_33_draws():
    """The same at K = 33 (a deviation table wider than a DPP row, ranks 32, 17, 33, 4), one case, both sides."""
    c = RU.build("proc_gauss", "rk4", B=13, ns=33)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    for is_post in (True, False):
        _check_exact(_band(eng, flat, c, is_post, obs_d=obs_d, labels=labels), _per_draw_curves(eng, flat, c, is_post, obs_d, labels), c["obs"].numpy(),
                     LEVELS, 0.0, ("K = 33", is_post))


# ---- 3. against the fp64 oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [7, 33])
@pytest.mark.parametrize("case", CASES)
def test_against_the_fp64_oracle(case, ns):
    """Per draw |dev_k - dev64_k| <= max_t (2 MEAN_BAR scale + dev64 SD_BAR scale) / sd64; crit within the largest such bar of its curve;
    joint: only draws within their bar of z may differ, the near share under NEAR_SHARE at the clear level (where every count is K); mean
    and sd by recon_moments' check; sd_floor = 0 excludes nothing (points == T)."""
    c = RU.build(case, "rk4", B=13, ns=ns)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    levels = BU.COUNT_LEVELS + (0.95, BU.CLEAR_LEVEL[ns])
    y = c["obs"].double().numpy()
    for is_post in (True, False):
        tag = "%s K=%d %s" % (case, ns, "post" if is_post else "prior")
        v = _oracle(case, ns, is_post)
        r = _band(eng, flat, c, is_post, levels)
        RU.check(torch.from_numpy(r["mean"]), torch.from_numpy(r["sd"]), v.mean(1), v.std(1), tag)
        assert np.all(r["points"] == c["T"])
        wd, wc, wo, share = _check_oracle(r, v, y, levels, 0.0, tag, share_at=BU.CLEAR_LEVEL[ns])
        print("%s: worst error / bar  dev %.3e  crit %.3e  obs_dev %.3e;  near share at the informative levels %.2e" % (tag, wd, wc, wo, share))


# ---- 4. the floor ---------------------------------------------------------------------------------------------------------------------------------
def test_sd_floor():
    """cvs_ald, B = 13, K = 7, the noise rows of trajectories 7 .. 12 scaled by 1e-4: their curves' sds lie four decades under the others',
    and a floor in the gap has no oracle sd within a factor 2 of it (asserted).  points equals the oracle's count above the floor (T or
    0), dev equals the restatement over those points and holds its oracle bars, a curve without a participating point has dev 0 in every
    draw, crit 0 and obs_dev 0.  A floor above every sd: dev == 0, crit == 0, points == 0 everywhere.  A floor inside the kernel's OWN sds
    of the unscaled case (partial rows): points and dev equal the restatement exactly."""
    c = RU.build("cvs_ald", "rk4", B=13, ns=7)
    w = torch.ones(13)
    w[7:] = 1e-4
    c = dict(c, eps=(c["eps"] * w.view(1, 13, 1)).contiguous())
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    y = c["obs"].double().numpy()
    for is_post in (True, False):
        v = SU.oracle_draws(c, is_post)
        sds = v.std(1)                                                                      # [Q, B, C, T]
        below, above = float(sds[:, 7:].max()), float(sds[:, :7].min())
        floor = math.sqrt(below * above)
        print("floor %s: the oracle's sds end at %.3e and begin again at %.3e; floor %.3e" % ("post" if is_post else "prior", below, above, floor))
        assert above / below >= 4.0 and not ((sds > floor / 2) & (sds < floor * 2)).any(), (is_post, below, above)
        r = _band(eng, flat, c, is_post, floor=floor, obs_d=obs_d, labels=labels)
        want = (sds > floor).sum(-1)
        assert np.array_equal(r["points"], want.astype(np.float32)) and set(np.unique(want)) == {0, c["T"]}
        assert np.all(want[:, :7] == c["T"]) and np.all(want[:, 7:] == 0)
        curves = _per_draw_curves(eng, flat, c, is_post, obs_d, labels)
        _check_exact(r, curves, c["obs"].numpy(), LEVELS, floor, ("floor", is_post))
        _check_oracle(r, v, y, LEVELS, floor, "floor %s" % is_post)
        assert np.all(r["dev"][:, 7:] == 0.0) and np.all(r["crit"][:, 7:] == 0.0) and np.all(r["obs_dev"][:, 7:] == 0.0) and np.all(r["joint"][:, 7:] == 1.0)
        assert np.all(r["dev"][:, :7] > 0.0)
        top = _band(eng, flat, c, is_post, floor=float(sds.max()) * 2.0 + 1.0, obs_d=obs_d, labels=labels)
        assert all(np.all(top[k] == 0.0) for k in ("dev", "crit", "points", "obs_dev")) and np.all(top["joint"] == 1.0)
        assert _same(top["mean"], r["mean"]) and _same(top["sd"], r["sd"])                  # the floor does not touch the moments
    c0, eng0, flat0, curves0, r0 = _per_draw("cvs_ald", True)
    own = float(np.median(r0["sd"]))                                                           # among the kernel's own sds: rows are cut
    part = _band(eng0, flat0, c0, True, floor=own)
    assert _same(part["sd"], r0["sd"]) and 0 < (part["points"] < c0["T"]).sum() and (part["points"] > 0).any()
    assert np.array_equal(part["points"], (r0["sd"] > np.float32(own)).sum(-1).astype(np.float32))
    _check_exact(part, curves0, c0["obs"].numpy(), LEVELS, own, "own floor")


# ---- 5. invariance ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald", "challenge_gauss"])
def test_grid_noise_source_and_instantiation_invariance(case, monkeypatch):
    """Identical bits for launch grids 1, 3 and the default, for the compile-time-S and the run-time-S instantiation, for a repeat, and for
    in-kernel noise against the same rows read back with rng_normal and passed explicitly; the counter after the call is the counter after
    recon_moments: n + 1, whatever the sweeps."""
    c = RU.build(case, "midpoint", B=13, ns=7)
    eng = _engine(c, monkeypatch)
    others = [_engine(c, monkeypatch, env) for env in ({"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "1"}, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"},
                                                        {"SLODE_ODE_GENERIC": "1"}, {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"})]
    flat = eng.pack(c["p"])
    keys = ("mean", "sd", "crit", "joint", "obs_dev", "points", "dev")
    for is_post in (True, False):
        a = _band(eng, flat, c, is_post)
        for e in [eng] + others:
            b = _band(e, flat, c, is_post)
            assert all(_same(a[k], b[k]) for k in keys), (case, is_post)
        for e in [eng] + others:
            e.rng_seed(77, first_trajectory=1000)
            e.rng_set_counter(5)
        drawn = _band(eng, flat, c, is_post, eps=None)
        assert eng.rng_state() == (77, 1000, 6)
        rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
        given = _band(eng, flat, c, is_post, eps=rows)
        assert eng.rng_state() == (77, 1000, 6)                                             # explicit noise draws nothing
        drawn_loop = _band(others[1], flat, c, is_post, eps=None)
        assert all(_same(drawn[k], given[k]) and _same(drawn[k], drawn_loop[k]) for k in keys), (case, is_post)
        eng.rng_set_counter(5)
        obs_d, labels = _device_batch(c)
        mean, sd = _recon_moments(eng, flat, c, is_post, eps=None, obs_d=obs_d, labels=labels)
        assert eng.rng_state() == (77, 1000, 6) and _same(drawn["mean"], mean.cpu().numpy()) and _same(drawn["sd"], sd.cpu().numpy())


# ---- 6. levels -------------------------------------------------------------------------------------------------------------------------------------
def test_eight_levels_in_scrambled_order():
    """Level 1.0 gives crit == dev.max(), a level with r = 1 gives dev.min(), crit is monotone in the level, duplicates agree, the outputs
    of a level do not depend on the others of the call; joint is monotone in z and 1 at level 1 (z = inf)."""
    c, eng, flat, curves, r4 = _per_draw("cvs_ald", False)
    levels = (0.9, 0.05, 1.0, 0.5, 0.95, 0.3, 0.5, 0.75)
    r = _band(eng, flat, c, False, levels)
    _check_exact(r, curves, c["obs"].numpy(), levels, 0.0, "eight levels")
    assert BU.level_rule(levels, 7)[0] == [7, 1, 7, 4, 7, 3, 4, 6]
    assert _same(r["dev"], r4["dev"]) and np.array_equal(r["crit"][..., 2], r["dev"].max(-1)) and np.array_equal(r["crit"][..., 1], r["dev"].min(-1))
    order = np.argsort(levels, kind="stable")
    assert np.all(np.diff(r["crit"][..., order], axis=-1) >= 0) and np.all(np.diff(r["joint"][..., order], axis=-1) >= 0)
    assert np.array_equal(r["crit"][..., 3], r["crit"][..., 6]) and np.array_equal(r["joint"][..., 3], r["joint"][..., 6]) and np.all(r["joint"][..., 2] == 1.0)
    assert np.array_equal(r["crit"][..., 4], r4["crit"][..., 0]) and np.array_equal(r["joint"][..., 3], r4["joint"][..., 1])
    one = _band(eng, flat, c, False, (0.75,))
    assert np.array_equal(one["crit"][..., 0], r["crit"][..., 7]) and np.array_equal(one["joint"][..., 0], r["joint"][..., 7])


# ---- 7. boundaries ------------------------------------------------------------------------------------------------------------------------------
def _grid_engine(fam, T, B, ns, mp):
    import dataclasses
    from structured_latent_odes_amd import engine as E
    c = MU.grid_case(fam, T, B=B, ns=ns)
    _set_env(mp, {})
    spec = dataclasses.replace({"cvs": E.cvs_spec, "proc": E.proc_spec}[fam](**c["kw"]), filter_size=1, pool_size=1)
    eng = E.Engine(spec, T, DEV)
    eng.set_times(c["times"])
    eng.workspace(c["B"]).fill_(float("nan"))
    return c, eng


@pytest.mark.parametrize("fam,T", [("cvs", 3), ("cvs", 9), ("proc", 17), ("cvs", 257)])
def test_grid_lengths(fam, T, monkeypatch):
    """T < 16 (most lanes of a row have no point), T = 17 (one lane has two), T = 257 (thread 0 takes point 256 alone in its second round):
    every output equals the restatement on the kernel's own curves, both sides; B = 3, K = 5."""
    c, eng = _grid_engine(fam, T, 3, 5, monkeypatch)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    for is_post in (True, False):
        r = _band(eng, flat, c, is_post, obs_d=obs_d, labels=labels)
        _check_exact(r, _per_draw_curves(eng, flat, c, is_post, obs_d, labels), c["obs"].numpy(), LEVELS, 0.0, (fam, T, is_post))
        mean, sd = _recon_moments(eng, flat, c, is_post, obs_d=obs_d, labels=labels)
        assert _same(r["mean"], mean.cpu().numpy()) and _same(r["sd"], sd.cpu().numpy()) and np.all(r["points"] <= T)


@pytest.mark.parametrize("case,B,ns,env", [("cvs_gauss", 1, 2, {}), ("proc_ald", 1, 7, {}), ("cvs_gauss", 65, 2, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}),
                                           ("challenge_ald", 9, 3, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"})],
                         ids=["B1-K2", "B1-K7", "B65-grid5-K2", "B9-grid2-K3"])
def test_batch_and_draw_count_edges(case, B, ns, env, monkeypatch):
    """B = 1; B larger than the grid (the persistent loop: 13 and 5 trajectories per workgroup at the most); K = 2 (dev is 1 in both draws up
    to rounding: each draw lies one sd from the mean of two); NaN-poisoned workspace; T = 142 (challenge_ald)."""
    c = RU.build(case, "rk4", B=B, ns=ns)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    obs_d, labels = _device_batch(c)
    for is_post in (True, False):
        r = _band(eng, flat, c, is_post, obs_d=obs_d, labels=labels)
        _check_exact(r, _per_draw_curves(eng, flat, c, is_post, obs_d, labels), c["obs"].numpy(), LEVELS, 0.0, (case, B, ns, is_post))
        if ns == 2:
            assert np.abs(r["dev"] - 1.0).max() <= 1e-3


def test_largest_draw_count_the_plan_accepts_and_one_more():
    """cvs_ald at T = 200: K = 3617 fills the LDS to 163824 of 163840 B and is taken -- prior, B = 2, every output against the restatement on
    the kernel's own curves, which ONE recon_moments call with num_samples = 1 on K x B trajectories (labels repeated, noise row k B + b)
    returns -- and K = 3618 is refused by name, drawing and launching nothing."""
    c = RU.build("cvs_ald", "rk4", B=2, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    from structured_latent_odes_amd import _lib as L
    lo, hi = 2, 1 << 20
    while hi - lo > 1:                                                                      # the plan is monotone in K
        mid = (lo + hi) // 2
        try:
            eng.joint_band_plan(2, mid)
            lo = mid
        except L.SlodeError:
            hi = mid
    K = lo
    assert K == 3617 and eng.joint_band_plan(2, K) == 163824
    eps = torch.randn(K, 2, c["eps"].shape[2], generator=torch.Generator().manual_seed(3))
    big = dict(c, eps=eps, ns=K)
    obs_d, labels = _device_batch(c)
    r = _band(eng, flat, big, False, obs_d=obs_d, labels=labels)
    wide = dict(c, B=2 * K, obs=c["obs"].repeat(K, 1, 1), u=c["u"].repeat(K, 1), eps=eps.reshape(1, 2 * K, -1), ns=1)
    curves = _recon_moments(eng, flat, wide, False)[0].cpu().numpy()                         # [Q, K * 2, C, T], row k * 2 + b
    curves = np.ascontiguousarray(np.moveaxis(curves.reshape(curves.shape[0], K, 2, curves.shape[2], curves.shape[3]), 1, 0))
    _check_exact(r, curves, c["obs"].numpy(), LEVELS, 0.0, "K = %d" % K)
    mean, sd = _recon_moments(eng, flat, big, False, obs_d=obs_d, labels=labels)
    assert _same(r["mean"], mean.cpu().numpy()) and _same(r["sd"], sd.cpu().numpy())
    outs = _outs(3, 2, 3, c["T"], 1, K + 1)
    bt = eng.make_batch(obs_d, labels, None)
    err = _refused(eng, lambda: eng.joint_band(flat, bt, 2, False, K + 1, [0.95], 0.0, *outs), "LDS tables of T = 200, S = 5, C = 3, num_samples = 3618 \\(163856 B")
    assert err.status == -1 and all(bool((t == FILL).all()) for t in outs)


# ---- 9. refusals at run time --------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_write_nothing(monkeypatch):
    """Every named reason returns SLODE_EINVAL with its message, draws nothing, launches nothing and writes nothing."""
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)
    outs = _outs(3, c["B"], 3, c["T"], 8, 4)

    def refused(eng, match, obs=obs_d, ns=4, is_post=True, null_obs=False, levels=(0.95,), floor=0.0, drop=None, particles=1):
        """Through the entry point itself: the outputs stand for any size, since a refused call writes none of them."""
        flat = eng.pack(c["p"])
        bt = eng.make_batch(obs, labels, None)
        if null_obs:
            bt.obs = None
        arr, n = eng._levels(levels)
        ptrs = [eng._p(None if i == drop else t) for i, t in enumerate(outs)]
        err = _refused(eng, lambda: eng._batch_call(eng.lib.slode_joint_band, flat, bt, c["B"], particles, 1 if is_post else 0, int(ns), n, arr,
                                                    float(floor), *ptrs), match)
        assert err.status == -1 and "slode_joint_band" in str(err) and all(bool((t == FILL).all()) for t in outs)

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s .*reduce recon_samples instead" % solver, is_post=solver != "bosh3")
    eng = _engine(c, monkeypatch)
    for is_post in (True, False):
        refused(eng, "num_samples = 1 < 2 \\(the sd of one draw is 0\\)", ns=1, is_post=is_post)
        refused(eng, "num_samples = 0 < 2", ns=0, is_post=is_post)
        refused(eng, "exceeds 2\\^30 - 1 noise rows", ns=2 ** 30, is_post=is_post)
        refused(eng, "particles = 2", particles=2, is_post=is_post)
        refused(eng, "n_levels = 0 out of range \\[1, 8\\]", levels=(), is_post=is_post)
        refused(eng, "n_levels = 9 out of range", levels=(0.5,) * 9, is_post=is_post)
        refused(eng, "levels\\[1\\] = 0 is not in \\(0, 1\\]", levels=(0.5, 0.0), is_post=is_post)
        refused(eng, "levels\\[0\\] = 1.5 is not in", levels=(1.5,), is_post=is_post)
        refused(eng, "levels\\[0\\] = nan", levels=(float("nan"),), is_post=is_post)
        refused(eng, "sd_floor = -0.5 is negative or not finite", floor=-0.5, is_post=is_post)
        refused(eng, "sd_floor = nan", floor=float("nan"), is_post=is_post)
        refused(eng, "sd_floor = inf", floor=float("inf"), is_post=is_post)
        for drop in (0, 1, 2):
            refused(eng, "mean / sd / crit is NULL", drop=drop, is_post=is_post)
        refused(eng, "observation strides", obs=_padded(obs_d), is_post=is_post)
        refused(eng, "LDS tables of T = 200, S = 5, C = 3, num_samples = 4000 .*exceed the budget of 163840 B", ns=4000, is_post=is_post)
    refused(eng, "batch->obs is NULL", null_obs=True)
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    # the prior takes a batch without observations: the observed deviation is NaN, everything else unchanged
    eng = _engine(c, monkeypatch)
    flat = eng.pack(c["p"])
    c7 = RU.build("cvs_ald", "rk4", ns=7)
    a, b = _band(eng, flat, c7, False), _band(eng, flat, c7, False, null_obs=True)
    assert np.isnan(b["obs_dev"]).all() and all(_same(a[k], b[k]) for k in ("mean", "sd", "crit", "joint", "points", "dev"))


def test_launches_and_graph_capture():
    """Posterior: "weff", "enc_fwd2", "joint_band" on one stream; prior: "joint_band" alone.  One capture and one replay equal the
    stream-launched call bitwise; capturing executes nothing (the levels travel by value: nothing is read from the host at replay)."""
    c = RU.build("cvs_ald", "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eng.profile_enable(True)
    _band(eng, flat, c, True)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "joint_band"]
    _band(eng, flat, c, False)
    assert [n for n, _ in eng.profile_read()] == ["joint_band"]
    eng.profile_enable(False)
    outs = [torch.zeros_like(t) for t in _outs(3, c["B"], 3, c["T"], 2, 7)]
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    want = _captured(lambda: eng.joint_band(flat, bt, c["B"], True, 7, [0.95, 0.5], 0.0, *outs), outs)
    assert all(_same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(outs, want)) and float(outs[2].abs().max()) > 0.0


# ---- 8. the model layer -------------------------------------------------------------------------------------------------------------------------
def _as_engine_outputs(res, names, with_dev=True):
    """The model's dict in the layout of ``_band``."""
    g = lambda k: np.stack([res[n][k].cpu().numpy() for n in names])
    r = dict(mean=g("mean"), sd=g("sd"), crit=np.moveaxis(g("crit"), 1, -1), joint=np.moveaxis(g("pointwise_joint"), 1, -1), obs_dev=g("obs_dev"),
             points=g("points"))
    if with_dev:
        r["dev"] = np.moveaxis(g("dev"), 1, -1)
    return r


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_dict_against_the_engine(fam):
    m, batch = _model(fam)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    ns, levels = 6, (0.9, 0.5)
    for is_post in (True, False):
        eng.rng_seed(21)
        eng.rng_set_counter(3)
        eps = eng.rng_normal(3, ns * B).view(ns, B, -1)
        eng.profile_enable(True)
        res = m.simultaneous_band(is_post=is_post, num_samples=ns, levels=levels, return_draws=True, **batch)
        assert [k for k, _ in eng.profile_read()] == (["weff", "enc_fwd2", "joint_band"] if is_post else ["joint_band"])
        eng.profile_enable(False)
        assert eng.rng_state() == (21, 0, 4) and set(res) == set(names) | {"levels"} and res["levels"].tolist() == list(levels)
        want = eng.joint_band(m._bind().flat, m._draws_batch(batch["observations"], {k: v for k, v in batch.items() if k != "observations"}, eps, ns),
                              B, is_post, ns, list(levels), 0.0, dev=True)
        mean, sd, crit, joint, odev, dev = want
        for q, n in enumerate(names):
            r = res[n]
            assert set(r) == {"mean", "sd", "crit", "lower", "upper", "pointwise_joint", "obs_dev", "obs_inside", "points", "dev"}
            assert torch.equal(r["mean"], mean[q]) and torch.equal(r["sd"], sd[q]) and torch.equal(r["crit"], crit[q].permute(2, 0, 1))
            assert torch.equal(r["pointwise_joint"], joint[q].permute(2, 0, 1)) and torch.equal(r["obs_dev"], odev[q, ..., 0])
            assert torch.equal(r["points"], odev[q, ..., 1]) and torch.equal(r["dev"], dev[q].permute(2, 0, 1)) and bool((r["points"] == T).all())
            assert tuple(r["lower"].shape) == (2, B, Cn, T) and r["obs_inside"].dtype == torch.bool
            assert torch.equal(r["lower"], r["mean"].unsqueeze(0) - r["crit"].unsqueeze(-1) * r["sd"].unsqueeze(0))
            assert torch.equal(r["upper"], r["mean"].unsqueeze(0) + r["crit"].unsqueeze(-1) * r["sd"].unsqueeze(0))
            assert torch.equal(r["obs_inside"], r["obs_dev"].unsqueeze(0) <= r["crit"])
            # what the band is for: the observation lies inside [lower, upper] at every point exactly when obs_inside says so (up to the
            # rounding of the band's own edges: checked away from them)
            y = batch["observations"].unsqueeze(0)
            clear = ((r["obs_dev"].unsqueeze(0) - r["crit"]).abs() > 1e-3 * r["crit"])
            inside = ((y >= r["lower"]) & (y <= r["upper"])).all(-1)
            assert torch.equal(inside[clear], r["obs_inside"][clear])
        rm = m.recon_moments(is_post=is_post, num_samples=ns, eps=eps, **batch)
        assert all(torch.equal(res[n]["mean"], rm[n][0]) and torch.equal(res[n]["sd"], rm[n][1]) for n in names)


def _check_against_curves(r, v, y, levels, tag, factor=1.0):
    """A dict in ``_band``'s layout against fp64 reductions of given curves v [Q, K, B, C, T]: mean, sd and dev within ``factor`` times the
    recon_moments bars carried through the quotient."""
    for q in range(v.shape[0]):
        o = BU.oracle_dev(v[q], y)
        scale = np.maximum(1.0, np.abs(o["mean"]))
        assert np.all(np.abs(r["mean"][q] - o["mean"]) <= factor * RU.MEAN_BAR * scale) and np.all(np.abs(r["sd"][q] - o["sd"]) <= factor * RU.SD_BAR * scale), tag
        bar = factor * BU.dev_bar(o)
        assert np.all(np.abs(np.moveaxis(r["dev"][q].astype(np.float64), -1, 0) - o["dev"]) <= bar), (tag, "dev")
        srt = np.sort(o["dev"], 0)
        for j, rk in enumerate(BU.level_rule(levels, v.shape[1])[0]):
            assert np.all(np.abs(r["crit"][q, ..., j] - srt[rk - 1]) <= bar.max(0)), (tag, "crit", j)


@pytest.mark.parametrize("why", ["dopri5", "strided"])
def test_composed_route_where_the_engine_refuses(why, monkeypatch):
    """dopri5, a padded observation tensor: the engine refuses once, simultaneous_band composes the dict from recon_samples -- one drawing
    call, the counter at n + 1 -- and agrees with fp64 reductions of those curves within the bars; on the fixed-grid model the fused call
    (dense observations, same noise) agrees with the composed route's curves within twice the bars (two fp32 evaluations of the truth)."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch)
    eng = m._bind().engine
    B, ns, levels = batch["observations"].shape[0], 6, (0.9, 0.5)
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    dense = dict(batch)
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    calls = _count_calls(monkeypatch, eng, "joint_band")
    eng.rng_seed(11)
    eng.rng_set_counter(2)
    eps = eng.rng_normal(2, ns * B).view(ns, B, -1)
    v = _model_curves(m, batch, True, eps)
    y = batch["observations"].double().cpu().numpy()
    drawn = m.simultaneous_band(is_post=True, num_samples=ns, levels=levels, return_draws=True, **batch)
    assert eng.rng_state() == (11, 0, 3) and len(calls) == 1                                # refused once, then composed
    given = m.simultaneous_band(is_post=True, num_samples=ns, levels=levels, return_draws=True, eps=eps, **batch)
    assert all(torch.equal(given[n][k], drawn[n][k]) for n in names for k in given[n])
    _check_against_curves(_as_engine_outputs(given, names), v, y, levels, "%s composed" % why)
    assert all(bool((given[n]["points"] == v.shape[-1]).all()) for n in names)
    if why == "strided":
        calls.clear()
        fused = m.simultaneous_band(is_post=True, num_samples=ns, levels=levels, return_draws=True, eps=eps, **dense)
        assert len(calls) == 1
        _check_against_curves(_as_engine_outputs(fused, names), v, y, levels, "fused against the composed route's curves", factor=2.0)


def test_one_draw_more_than_the_plan_takes_is_composed(monkeypatch):
    """The model's shape (cvs, T = 86): the largest K the plan accepts runs fused, one more is refused by the engine (LDS budget) and the
    model composes the same dict from recon_samples; two trajectories."""
    from structured_latent_odes_amd import _lib as L
    m, batch = _model("cvs")
    batch = {k: v[:2].contiguous() for k, v in batch.items()}
    batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    eng = m._bind().engine
    lo, hi = 2, 1 << 20
    while hi - lo > 1:
        mid = (lo + hi) // 2
        try:
            eng.joint_band_plan(2, mid)
            lo = mid
        except L.SlodeError:
            hi = mid
    with pytest.raises(L.SlodeError, match="LDS tables"):
        eng.joint_band_plan(2, lo + 1)
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    for K, route in ((lo, ["weff", "enc_fwd2", "joint_band"]), (lo + 1, None)):
        eps = torch.randn(K, 2, eng.spec.latent_dim, generator=torch.Generator().manual_seed(4)).to(DEV)
        eng.profile_enable(True)
        res = m.simultaneous_band(is_post=True, num_samples=K, levels=(0.95, 0.5), eps=eps, return_draws=True, **batch)
        try:
            kernels = [k for k, _ in eng.profile_read()]
        except L.SlodeError:                                                                # (nothing profiled: no engine call was taken)
            kernels = []
        eng.profile_enable(False)
        assert (kernels == route) if route else ("joint_band" not in kernels), (K, kernels)
        v = _model_curves(m, batch, True, eps)
        _check_against_curves(_as_engine_outputs(res, names), v, batch["observations"].double().cpu().numpy(), (0.95, 0.5), "K = %d" % K, factor=2.0)
    print("cvs T = 86: the plan takes K <= %d" % lo)


def test_memory_stays_below_one_materialised_tensor():
    m, batch = _model("cvs")
    batch = {k: torch.cat([v] * 4)[:64].contiguous() for k, v in batch.items()}
    batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    m.simultaneous_band(is_post=True, num_samples=8, **batch)
    eng.profile_enable(True)
    peak = _peak(lambda: m.simultaneous_band(is_post=True, num_samples=64, **batch))
    assert [n for n, _ in eng.profile_read()][-1] == "joint_band"                           # the fused route, not the composition
    eng.profile_enable(False)
    one = B * Cn * T * 64 * 4
    print("peak over the allocation before the call: fused B=64 K=64 %d B; one materialised [B, C, T, K] tensor %d B" % (peak, one))
    assert B == 64 and peak < one


def test_output_files(tmp_path):
    """save_simultaneous_band over two batches: the arrays and the levels, equal to simultaneous_band from the same generator state, the
    trajectories in loader order; the printed line."""
    m, batch = _model("challenge")
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    halves = [{k: v[:9] for k, v in batch.items()}, {k: v[9:] for k, v in batch.items()}]
    halves = [dict(h, observations=h["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)) for h in halves]
    eng.rng_seed(8)
    files = m.save_simultaneous_band(str(tmp_path / "b"), halves, True, 5, levels=(0.5, 0.95))
    assert eng.rng_state()[2] == 2
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    want = ["%s_post_band_%s.npy" % (n, k) for n in names for k in ("mean", "sd", "crit", "pointwise_joint", "obs_dev")] + ["band_levels.npy"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "b"))) == sorted(want)
    assert np.load(files[-1]).tolist() == [0.5, 0.95]
    mean, crit, joint, odev = (np.load(files[i]) for i in (0, 2, 3, 4))
    assert mean.shape == (B, Cn, T) and crit.shape == joint.shape == (B, 2, Cn) and odev.shape == (B, Cn) and crit.dtype == np.float32
    eng.rng_set_counter(1)
    res = m.simultaneous_band(is_post=True, num_samples=5, levels=(0.5, 0.95), **halves[1])
    assert np.array_equal(crit[9:], res[names[0]]["crit"].transpose(0, 1).cpu().numpy()) and np.array_equal(mean[9:], res[names[0]]["mean"].cpu().numpy())
    assert np.all(crit[:, 0] <= crit[:, 1]) and np.all(crit <= 2.0 + 1e-5)                # sqrt(K - 1) = 2 at five draws
    print(m.band_line(crit, joint, odev, np.load(files[-1]), "post"))


def test_training_entry_point_with_joint_band(tmp_path, monkeypatch, capsys):
    """One --joint-band 6 run of training.main on a synthetic loader, one epoch: the files beside the run's others, and the two lines."""
    import re
    from structured_latent_odes_amd import training as T
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.models.mechanistic_cvs_Gauss import MechanisticModelGauss

    def load_config():
        cfg = EU.model_config("cvs")
        cfg.update(mini_batch_size=16, seq_len=86)
        return cfg

    monkeypatch.chdir(tmp_path)
    T.main("cvs", load_config, MechanisticModel, MechanisticModelGauss, ["--epochs", "1", "--batches-per-epoch", "1", "--joint-band", "6",
                                                                          "--band-levels", "0.5,0.9"])
    out = capsys.readouterr().out
    assert "FINAL TEST:" in out
    res = tmp_path / ("results_%s" % load_config().model)
    for tag in ("post", "prior"):
        m = re.search(r"^joint_band_%s: n=(\d+)  levels=\[0\.5, 0\.9\]  0\.5: crit=([0-9.]+) \(z=0\.674\) pointwise_joint=([0-9.]+) obs_inside=([0-9.]+)  "
                      r"0\.9: crit=([0-9.]+) \(z=1\.645\) pointwise_joint=([0-9.]+) obs_inside=([0-9.]+)$" % tag, out, re.M)
        assert m, out[-2000:]
        n = int(m.group(1))
        assert n >= 16 and float(m.group(2)) <= float(m.group(5)) <= math.sqrt(5.0) + 1e-3 and 0.0 <= float(m.group(3)) <= float(m.group(6)) <= 1.0
        heads = sorted(f[:-len("_%s_band_crit.npy" % tag)] for f in os.listdir(str(res)) if f.endswith("_%s_band_crit.npy" % tag))
        assert heads in (["mean"], ["mu_25", "mu_50", "mu_75"])
        for h in heads:
            crit = np.load(str(res / ("%s_%s_band_crit.npy" % (h, tag))))
            assert crit.shape == (n, 2, 3) and crit.dtype == np.float32 and np.isfinite(crit).all()
            assert np.load(str(res / ("%s_%s_band_mean.npy" % (h, tag)))).shape == np.load(str(res / ("%s_%s_band_sd.npy" % (h, tag)))).shape == (n, 3, 86)
            assert np.load(str(res / ("%s_%s_band_obs_dev.npy" % (h, tag)))).shape == (n, 3)
            assert np.load(str(res / ("%s_%s_band_pointwise_joint.npy" % (h, tag)))).shape == (n, 2, 3)
    assert np.load(str(res / "band_levels.npy")).tolist() == [0.5, 0.9]
