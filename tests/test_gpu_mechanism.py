"""GPU tests of the mechanism curves (slode_mechanism_moments; Engine.mechanism_moments; MechanisticModel.mechanism_moments).

What is exact and what has a bar (tests/mechanism_util.py): at one draw the net rate is fma(-d, x, a) of the call's own state, production and
degradation bitwise, the set point is a / d within one ulp, sd is exactly 0, and the head curves of recon_moments on the same noise are the
fma chain of its head weights over these states bitwise; the moments over draws equal the numpy restatement of the shifted accumulation
bitwise; slot subsets, grids, noise sources, splits and graph replay change no bit.  Against the fp64 oracle every slot has the bar of
MU.BARS x max(1, |oracle mean|).  All five slots are compared on the conditioned cases of MU.build, which meet the condition that keeps the
set point finite (the oracle's smallest d >= MU.MIN_D: MU's docstring, asserted in tests/test_mechanism_cpu.py and here), and the four
bounded slots also on RU.build's cases as they are ("as_built"), whose degradation saturates."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import mechanism_util as MU
from tests import recon_moments_util as RU
from tests.eval_gpu_util import (ADAPTIVE, DEV, ENV_KEYS, WIDTHS, _captured, _count_calls, _device_batch, _engine, _eps_dev, _model, _padded, _peak,
                                 _recon_moments, _refused, _same as _same_arrays, _set_env)
from tests.eval_gpu_util import _mech

pytestmark = pytest.mark.gpu
FILL = -12345.5            # the outputs are pre-filled with it: every element must be written
GUARD = 7.25               # and stand between guard words, which must stay
NG = 64
BOUNDED = 0x17             # state, production, degradation, net_rate
WHICH = {"conditioned": MU.ALL, "as_built": BOUNDED}      # the cases of MU.build: all five slots; RU.build's as they are: the bounded four


_same = functools.partial(_same_arrays, equal_nan=True)


def _take(arr, slots):
    """The rows of an all-slots array that the mask selects, in increasing slot order."""
    return arr[[q for q in range(MU.SLOTS) if (slots >> q) & 1]]


def _check_which(mean, sd, want_mean, want_sd, tag, which, factor=1.0):
    """The slots of ``which`` of all-slots arrays against the oracle at the bars."""
    with np.errstate(all="ignore"):
        MU.check(_take(mean, WHICH[which]).astype(np.float64), _take(sd, WHICH[which]).astype(np.float64), want_mean, want_sd,
                 "%s [%s]" % (tag, which), WHICH[which], factor)


# ---- 1. against the fp64 oracle ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_run(case, solver, B=None, ns=7, env=(), as_built=False):
    """One all-slots call per side on MU.build(case, solver, B, ns) (``as_built``: RU.build's) under the environment ``env``, NaN-filled
    workspace: computed once."""
    c = (RU.build if as_built else MU.build)(case, solver, B=B, ns=ns)
    mp = pytest.MonkeyPatch()
    try:
        eng = _engine(c, mp, dict(env))
        flat = eng.pack(c["p"])
        eng.workspace(c["B"]).fill_(float("nan"))
        return {is_post: _mech(eng, flat, c, is_post) for is_post in (True, False)}
    finally:
        mp.undo()


@pytest.mark.parametrize("which", list(WHICH))
@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_against_the_fp64_oracle(case, solver, which):
    """Every case of EU.CASES x EU.SOLVERS, ns = 7, both sides, all five slots in one call, at the bars: all five on the conditioned case
    (the oracle's smallest d at least MU.MIN_D, asserted), the bounded four also on the case as built."""
    as_built = which == "as_built"
    got = _case_run(case, solver, as_built=as_built)
    for is_post in (True, False):
        wm, ws, d_min = MU.reference(case, solver, None, 7, is_post, as_built)
        assert as_built or d_min >= MU.MIN_D, (case, is_post, d_min)
        _check_which(*got[is_post], wm, ws, "%s/%s/%s (oracle's smallest d %.1e)" % (case, solver, "post" if is_post else "prior", d_min), which)


# ---- 2. one draw ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_one_draw(case, is_post):
    """ns = 1: sd == 0 exactly; net_rate is fma(-degradation, state, production) bitwise; set_point is within one ulp of production /
    degradation in fp32; the head curves of recon_moments at ns = 1 on the same noise are the fma chain of fwd_head_value over these states
    and the head weights, bitwise -- the states are the kernel family's own."""
    c = RU.build(case, "rk4", ns=1)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    mean, sd = _mech(eng, flat, c, is_post)
    x, a, d, sp, nr = mean
    assert sd.shape == mean.shape and np.all(sd == 0.0)                                    # (a non-finite value too: the first draw adds no difference)
    assert _same(nr, MU.net_rate_f32(a, d, x))
    with np.errstate(all="ignore"):
        want = MU.set_point_f32(a, d)
        fin = np.isfinite(want)
        assert np.all(np.abs(sp[fin].astype(np.float64) - want[fin]) <= np.spacing(np.abs(want[fin])))
        assert np.array_equal(sp[~fin], want[~fin], equal_nan=True)                          # d underflows: the quotient's inf or NaN, as it is
    print("%s %s: set_point equals the fp32 quotient bitwise at %.4f of the entries; non-finite %d" % (case, "post" if is_post else "prior",
                                                                                                       float((sp[fin] == want[fin]).mean()), int((~fin).sum())))
    curves = _recon_moments(eng, flat, c, is_post, ns=1)[0].cpu().numpy()                  # [Q, B, C, T]
    for q, hn in enumerate(eng.spec.head_names):
        w = RU._f32(c["p"]["decoder.%s.0.weight" % hn].numpy())                            # [C, S]
        v = np.zeros(curves.shape[1:], np.float32)
        for s in range(c["S"]):
            v = RU._fma32(np.broadcast_to(w[None, :, s, None], v.shape), np.broadcast_to(x[:, None, s, :], v.shape), v)
        assert _same(curves[q], v), (case, hn)


# ---- 3. moments over draws ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_moments_over_draws_bitwise(case, is_post):
    """ns = 7 equals RU.shifted_moments_f32 of seven ns = 1 calls on the rows k of the same noise, bitwise."""
    c = RU.build(case, "midpoint", B=5, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps = c["eps"].to(DEV)
    per = np.stack([_mech(eng, flat, c, is_post, eps=eps[k].contiguous(), ns=1, sd=False, obs_d=obs_d, labels=labels)[0] for k in range(7)])
    mean, sd = _mech(eng, flat, c, is_post, obs_d=obs_d, labels=labels)
    with np.errstate(all="ignore"):
        wm, ws = RU.shifted_moments_f32(per)
    assert _same(mean, wm), np.argwhere(~((mean == wm) | (np.isnan(mean) & np.isnan(wm))))[:5]
    assert _same(sd, ws), np.argwhere(~((sd == ws) | (np.isnan(sd) & np.isnan(ws))))[:5]


# ---- 4. sizes and instantiations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(WHICH))
@pytest.mark.parametrize("case,B,ns,env", MU.SIZES,
                         ids=["%s-B%d-ns%d%s" % (c, B, ns, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, ns, e in MU.SIZES])
def test_sizes_and_instantiations(case, B, ns, env, which):
    """MU.SIZES: B in {1, 3, 65}, the persistent loop on 2 and 5 workgroups, T in {86, 100, 200, 300} (300: two rounds of thread <-> time
    point), S = 5, 8 and the run-time-S build, ns in {1, 2, 7, 200}; NaN-filled workspace, pre-filled outputs between guard words."""
    as_built = which == "as_built"
    got = _case_run(case, "rk4", B, ns, tuple(sorted(env.items())), as_built)
    for is_post in (True, False):
        wm, ws, d_min = MU.reference(case, "rk4", B, ns, is_post, as_built)
        assert as_built or d_min >= MU.MIN_D, (case, B, ns, is_post, d_min)
        _check_which(*got[is_post], wm, ws, "%s B=%d ns=%d %s %s" % (case, B, ns, env, "post" if is_post else "prior"), which)
        if ns == 1:
            assert not _take(got[is_post][1], BOUNDED).any()


@functools.lru_cache(maxsize=None)
def _grid_run(fam, T):
    import dataclasses
    from structured_latent_odes_amd import engine as E
    c = MU.grid_case(fam, T)
    mp = pytest.MonkeyPatch()
    try:
        _set_env(mp, {})
        spec = dataclasses.replace({"cvs": E.cvs_spec, "proc": E.proc_spec}[fam](**c["kw"]), filter_size=1, pool_size=1)
        eng = E.Engine(spec, T, DEV)
        eng.set_times(c["times"])
        eng.workspace(c["B"]).fill_(float("nan"))
        flat = eng.pack(c["p"])
        return {is_post: (_mech(eng, flat, c, is_post), MU.oracle_draws(c, is_post)) for is_post in (True, False)}
    finally:
        mp.undo()


@pytest.mark.parametrize("T", MU.GRID_T)
@pytest.mark.parametrize("fam", ["cvs", "proc"])
def test_grid_lengths(fam, T):
    """T in {2, 3, 257} at S = 5 and S = 8 (T = 86 and 300 are cases of the list above): one step, two steps, and one point beyond a round
    of 256 threads -- thread 0 takes point T - 1 alone in its second round -- both sides, B = 3, ns = 2, all five slots against the oracle
    (MU.grid_case: conditioned; the oracle's smallest d at least MU.MIN_D, asserted)."""
    for is_post, ((mean, sd), draws) in _grid_run(fam, T).items():
        assert MU.min_degradation(draws) >= MU.MIN_D
        _check_which(mean, sd, *MU.moments(draws), "%s T=%d %s" % (fam, T, "post" if is_post else "prior"), "conditioned")


# ---- 5. independence --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_noise_grid_and_slot_independence(case, monkeypatch):
    """A repeat, two grids and in-kernel against explicit noise are bitwise equal, the counter at n + 1; sd not asked for leaves mean bitwise
    unchanged; every slot subset (each single slot, {1, 3}, all) equals the matching rows of the all-slots call bitwise."""
    c = RU.build(case, "midpoint", ns=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        a = _mech(eng, flat, c, is_post)
        for other in (_mech(eng, flat, c, is_post), _mech(loop, flat, c, is_post)):
            assert _same(a[0], other[0]) and _same(a[1], other[1])
        lean = _mech(eng, flat, c, is_post, sd=False)
        assert _same(lean[0], a[0]) and lean[1] is None
        for slots in (0x01, 0x02, 0x04, 0x08, 0x10, 0x0a):
            part = _mech(eng, flat, c, is_post, slots=slots)
            assert _same(part[0], _take(a[0], slots)) and _same(part[1], _take(a[1], slots)), hex(slots)
        for e in (eng, loop):
            e.rng_seed(77, first_trajectory=1000)
            e.rng_set_counter(5)
        drawn = _mech(eng, flat, c, is_post, eps=None)
        assert eng.rng_state() == (77, 1000, 6)
        rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
        given = _mech(eng, flat, c, is_post, eps=rows)
        assert eng.rng_state() == (77, 1000, 6)                                   # explicit noise draws nothing
        drawn_loop = _mech(loop, flat, c, is_post, eps=None)
        assert all(_same(x, y) and _same(x, z) for x, y, z in zip(drawn, given, drawn_loop))


def test_forced_split_in_the_model_call_is_bitwise_the_single_call(monkeypatch):
    m, batch = _model("cvs")
    eng = m._bind().engine
    calls = _count_calls(monkeypatch, eng, "mechanism_moments", lambda a: a[5])
    for is_post in (True, False):
        eng.rng_seed(5)
        eng.rng_set_counter(2)
        single = m.mechanism_moments(is_post=is_post, num_samples=6, **batch)
        assert eng.rng_state() == (5, 0, 3) and calls == [0x1f]
        calls.clear()
        monkeypatch.setattr(type(m), "MECHANISM_SLOTS_PER_CALL", 2)
        eng.rng_set_counter(2)
        split = m.mechanism_moments(is_post=is_post, num_samples=6, **batch)
        assert eng.rng_state() == (5, 0, 3) and calls == [0x03, 0x0c, 0x10]
        calls.clear()
        monkeypatch.setattr(type(m), "MECHANISM_SLOTS_PER_CALL", None)
        for n in MU.NAMES:
            assert all(_same(split[n][k].cpu().numpy(), single[n][k].cpu().numpy()) for k in (0, 1)), n


# ---- 6. launches and capture ----------------------------------------------------------------------------------------------------------------------
def test_launches_and_graph_capture():
    """Posterior: "weff", "enc_fwd2", "mechanism_moments" on one stream; prior: "mechanism_moments" alone.  One capture and one replay equal
    the stream-launched call bitwise; capturing executes nothing."""
    c = RU.build("cvs_ald", "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eng.profile_enable(True)
    _mech(eng, flat, c, True)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "mechanism_moments"]
    _mech(eng, flat, c, False)
    assert [n for n, _ in eng.profile_read()] == ["mechanism_moments"]
    eng.profile_enable(False)
    outs = [torch.zeros(5, c["B"], c["S"], c["T"], device=DEV), torch.zeros(5, c["B"], c["S"], c["T"], device=DEV)]
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    want = _captured(lambda: eng.mechanism_moments(flat, bt, c["B"], True, 7, MU.ALL, *outs), outs)
    assert all(_same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(outs, want)) and float(outs[0].abs().max()) > 0.0


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(monkeypatch):
    """Every refusal names its reason, draws nothing and launches nothing (rng_state, profile_read)."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd import engine as E
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)

    def refused(eng, match, obs=obs_d, ns=2, is_post=True, null_obs=False, slots=MU.ALL):
        flat = eng.pack(c["p"])
        bt = eng.make_batch(obs, labels, None)
        if null_obs:
            bt.obs = None
        err = _refused(eng, lambda: eng.mechanism_moments(flat, bt, c["B"], is_post, ns, slots), match)
        assert err.status == -1 and "slode_mechanism_moments" in str(err)

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s .*compose slode_ode_solve_fwd" % solver, is_post=solver != "bosh3")
    eng = _engine(c, monkeypatch)
    for is_post in (True, False):
        refused(eng, "num_samples = 0", ns=0, is_post=is_post)
        refused(eng, "exceeds 2\\^30 - 1 noise rows", ns=2 ** 30, is_post=is_post)
        refused(eng, "slots = 0x0 selects nothing", slots=0, is_post=is_post)
        refused(eng, "slots = 0x20 .*at or beyond SLODE_MECHANISM_SLOTS = 5", slots=0x20, is_post=is_post)
    refused(eng, "batch->obs is NULL", null_obs=True)
    refused(eng, "observation strides", obs=_padded(obs_d))
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    # tables beyond the LDS of one CU with five slots, within it with one: cvs at T = 1024
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    big = E.Engine(E.cvs_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    big.profile_enable(True)
    flat0 = torch.zeros(big.n_params, device=DEV)
    bt = big.make_batch(torch.zeros(2, 3, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["cvs"]], None)
    for is_post in (True, False):
        with pytest.raises(L.SlodeError, match="LDS tables of T = 1024, S = 5, C = 3, slots = 5 .*fewer slots per call fit"):
            big.mechanism_moments(flat0, bt, 2, is_post, 2, MU.ALL)
    assert big.rng_state()[2] == 0
    with pytest.raises(L.SlodeError, match="no profiled step"):
        big.profile_read()
    with pytest.raises(L.SlodeError, match="slots = 5"):
        big.mechanism_plan(2, MU.ALL)
    assert big.mechanism_plan(2, 0x08) <= 160 * 1024
    mean, sd = big.mechanism_moments(flat0, bt, 2, False, 2, 0x08)                  # one slot of the same shape is taken
    assert [n for n, _ in big.profile_read()] == ["mechanism_moments"] and tuple(mean.shape) == (1, 2, 5, 1024) and bool(torch.isfinite(mean).all())
    assert float((mean - 1.0).abs().max()) == 0.0 and float(sd.abs().max()) == 0.0      # all-zero parameters: a = d = 1/2, the set point is 1


# ---- 8. the model layer -----------------------------------------------------------------------------------------------------------------------
def _model_case(m, batch, eps, solver):
    """The model's own parameters, observations and noise as a case of MU.oracle_draws (posterior: the labels are not read)."""
    from oracle import slode_oracle as O
    from tests.eval_side_util import _p64
    ospec = O.cvs_spec(m.z_dims["iext"], m.z_dims["rtpr"], m.z_dims["epsilon"], solver=solver)
    obs = batch["observations"].detach().cpu()
    return dict(ospec=ospec, p=_p64(m), obs=obs, u=torch.zeros(obs.shape[0], 2), times=torch.as_tensor(m.times).detach().cpu().reshape(-1), eps=eps.cpu())


def _stack(res, k):
    return np.stack([res[n][k].permute(0, 2, 1).cpu().numpy() for n in MU.NAMES])       # [5, B, S, T]


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_dict_keys_and_shapes(fam):
    m, batch = _model(fam)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    S = eng.spec.ode_state_dim
    ns = 6
    for is_post in (True, False):
        eng.rng_seed(21)
        eng.rng_set_counter(3)
        eng.profile_enable(True)
        res = m.mechanism_moments(is_post=is_post, num_samples=ns, **batch)
        assert [k for k, _ in eng.profile_read()] == (["weff", "enc_fwd2", "mechanism_moments"] if is_post else ["mechanism_moments"])
        eng.profile_enable(False)
        assert eng.rng_state() == (21, 0, 4) and set(res) == set(MU.NAMES) | {"quantities"} and res["quantities"] == MU.NAMES
        for n in MU.NAMES:
            assert all(tuple(t.shape) == (B, T, S) and t.dtype == torch.float32 for t in res[n])
        x, a, d = (res[n][0] for n in ("state", "production", "degradation"))
        assert bool(((a >= 0) & (a <= 1) & (d >= 0) & (d <= 1)).all()) and bool(torch.isfinite(x).all())      # sigmoids, saturated or not
        eps = eng.rng_normal(3, ns * B).view(ns, B, -1)
        some = m.mechanism_moments(is_post=is_post, num_samples=ns, quantities=("net_rate", "state"), eps=eps, **batch)
        assert set(some) == {"quantities", "net_rate", "state"} and eng.rng_state() == (21, 0, 4)
        assert all(torch.equal(some[n][k], res[n][k]) for n in ("net_rate", "state") for k in (0, 1))
    with pytest.raises(ValueError, match="quantities"):
        m.mechanism_moments(is_post=True, num_samples=ns, quantities=("state", "flux"), **batch)


@functools.lru_cache(maxsize=None)
def _composed_run(why):
    """The composed route of the cvs model where the engine refuses (dopri5; a padded observation tensor), explicit noise, and the fp64
    oracle on the model's own parameters; for "strided" also the fused call on the dense observations."""
    mp = pytest.MonkeyPatch()
    try:
        m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, mp)
        eng = m._bind().engine
        B, ns = batch["observations"].shape[0], 6
        dense = dict(batch)
        if why == "strided":
            batch["observations"] = _padded(batch["observations"])
        calls = _count_calls(mp, eng, "mechanism_moments")
        eng.rng_seed(11)
        eng.rng_set_counter(2)
        eps = eng.rng_normal(2, ns * B).view(ns, B, -1)
        drawn = m.mechanism_moments(is_post=True, num_samples=ns, **batch)
        state = (eng.rng_state(), len(calls))
        given = m.mechanism_moments(is_post=True, num_samples=ns, eps=eps, **batch)
        same = all(torch.equal(given[n][k].nan_to_num(), drawn[n][k].nan_to_num()) for n in MU.NAMES for k in (0, 1))
        c = _model_case(m, dense, eps, "dopri5" if why == "dopri5" else "rk4")
        want = MU.moments(MU.oracle_draws(c, True))
        fused = None
        if why == "strided":
            calls.clear()
            fused = m.mechanism_moments(is_post=True, num_samples=ns, eps=eps, **dense)
            assert len(calls) == 1
            fused = (_stack(fused, 0), _stack(fused, 1))
        return state, same, (_stack(given, 0), _stack(given, 1)), want, fused
    finally:
        mp.undo()


@pytest.mark.parametrize("why", ["dopri5", "strided"])
def test_composed_route_where_the_engine_refuses(why):
    """dopri5, a padded observation tensor: the engine refuses once, mechanism_moments composes the dict -- one drawing call, the counter at
    n + 1, the same bits from the same rows passed explicitly -- and agrees with the fp64 oracle at the bars.  On the fixed-grid model the
    composed route agrees with the fused call (dense observations, same noise) at twice the bars."""
    state, same, given, want, fused = _composed_run(why)
    assert state == ((11, 0, 3), 1) and same
    which = "conditioned"                                                          # all five slots (the model's own grid and posterior)
    _check_which(given[0], given[1], want[0], want[1], "%s composed" % why, which)
    if fused is not None:
        _check_which(fused[0], fused[1], want[0], want[1], "fused against the oracle", which)
        _check_which(given[0], given[1], fused[0].astype(np.float64), fused[1].astype(np.float64), "composed against fused", which, factor=2.0)


def test_memory_stays_below_one_materialised_tensor():
    """After a warm-up call, the peak of torch.cuda.max_memory_allocated of the fused call at B = 64, ns = 200 over the allocation before it
    stays below ONE [ns, B, T, S] tensor."""
    m, batch = _model("cvs")
    batch = {k: torch.cat([v] * 4)[:64].contiguous() for k, v in batch.items()}
    batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    S = eng.spec.ode_state_dim
    m.mechanism_moments(is_post=True, num_samples=8, **batch)
    eng.profile_enable(True)
    peak = _peak(lambda: m.mechanism_moments(is_post=True, num_samples=200, **batch))
    assert [n for n, _ in eng.profile_read()][-1] == "mechanism_moments"           # the fused route, not the composition
    eng.profile_enable(False)
    one = 200 * B * T * S * 4
    print("peak over the allocation before the call: fused B=64 ns=200 %d B; one [ns, B, T, S] tensor %d B" % (peak, one))
    assert B == 64 and peak < one


def test_output_files(tmp_path):
    """save_mechanism_moments over two batches: the ten arrays [n, T, S], equal to mechanism_moments from the same generator state, the
    trajectories in loader order; the printed line."""
    m, batch = _model("challenge")
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    S = eng.spec.ode_state_dim
    halves = [{k: v[:9] for k, v in batch.items()}, {k: v[9:] for k, v in batch.items()}]
    halves = [dict(h, observations=h["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)) for h in halves]
    eng.rng_seed(8)
    files = m.save_mechanism_moments(str(tmp_path / "mm"), halves, True, 5)
    assert eng.rng_state()[2] == 2
    want = ["mechanism_%s_post_%s.npy" % (n, k) for n in MU.NAMES for k in ("mean", "sd")]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "mm"))) == sorted(want)
    arrays = {os.path.basename(f): np.load(f) for f in files}
    assert all(a.shape == (B, T, S) and a.dtype == np.float32 for a in arrays.values())
    eng.rng_set_counter(1)
    res = m.mechanism_moments(is_post=True, num_samples=5, **halves[1])
    assert np.array_equal(arrays["mechanism_production_post_mean.npy"][9:], res["production"][0].cpu().numpy())
    assert np.array_equal(arrays["mechanism_net_rate_post_sd.npy"][9:], res["net_rate"][1].cpu().numpy())
    line = m.mechanism_line({k: arrays["mechanism_%s_post_mean.npy" % k] for k in ("production", "degradation", "set_point")}, "post")
    print(line)
    assert line.startswith("mechanism_post: n=%d  x0 a=" % B) and " x%d a=" % (S - 1) in line
