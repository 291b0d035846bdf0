"""The batches the project is benchmarked and trained at, against the fp64 oracle tensor by tensor -- not only at B <= 48.

Several launch choices depend on B, so the small-batch cases do not reach the code that runs at full size: the encoder GEMMs' split-K
(ceil(B / 128), capped at 16; the last wave of trajectories runs partly past the batch at B = 1, 129, 2049), enc_fwd2's trajectory tile
(TBE below 2048, 2 TBE from 2048, 4 TBE from 4096; forward-only step), the lanes per trajectory of the adaptive forward solve (16 while
(B + 3) / 4 <= 4 x CUs, 8 beyond) and the grids of the encoder backward, gradient tail and ODE launches.  Every case here runs the whole
batch in one launch, with the workspace and the outputs filled with NaN first, and compares
  * -ELBO within 1e-5 relative, and the forward-only step's (SVI.evaluate_loss) too;
  * EACH gradient tensor within 5e-4 norm-wise (a tensor whose oracle gradient is zero must come back exactly zero);
  * the trajectories of all B trajectories element-wise within 1e-5 max(1, |x|), the latent sample within 2e-5 norm-wise.
The fp32 restatement of the oracle stays within 1.3e-7 (loss) and 2.2e-6 (any tensor) of fp64 at these sizes: a failure is a bug, not
summation order.  Every assertion message carries the worst per-tensor error; run with -s for one margin line per case."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import slode_oracle as O
from tests import full_size_util as U
from tests import rng_math as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")

SHAPES = {
    # name: (family, spec kwargs, T, S)
    "metric": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2, solver="rk4"), 200, 5),          # bench.py's shape (BASELINE config[1])
    "config4": ("challenge", dict(gauss=True, solver="rk4"), 300, 5),                   # a B = 512 shard of BASELINE config[4]
    "config2": ("proc", dict(z_g=10, z_eps=10, solver="rk4"), 100, 8),                  # BASELINE config[2] on the fixed grid
}
_cache = {}


def _case(shape, B, mode="exact", which="main"):
    """Inputs and the fp64 oracle (loss, every gradient tensor, trajectories, latent sample), computed once per module."""
    key = (shape, B, mode, which)
    if key not in _cache:
        fam, kw, T, S = SHAPES[shape]
        ospec = dataclasses.replace(U.OSPEC[fam](**kw), grad_mode=mode)
        p = U.params(ospec, T, S)
        obs, u, eps, times = O.synthetic_batch(ospec, B, T)
        want = U.oracle(p, ospec, obs, u, eps, times, which=which)
        _cache[key] = dict(fam=fam, kw=kw, T=T, S=S, L=ospec.latent_dim, p=p, obs=obs, u=u, eps=eps, times=times, want=want)
    return _cache[key]


def _setup(c, mode):
    eng = U.engine(c["fam"], c["kw"], c["T"], DEV, mode)
    eng.set_times(c["times"])
    flat = eng.pack(c["p"])
    return eng, flat, U.to_device(c["obs"], DEV), c["u"].to(DEV).contiguous(), c["eps"].to(DEV).contiguous()


def _report(what, **errs):
    print("full-size %s: %s" % (what, ", ".join("%s %s" % (k, ("%.2e" % v) if isinstance(v, float) else v) for k, v in errs.items())))


def _main_step_case(shape, B, mode):
    c = _case(shape, B, mode)
    want = c["want"]
    eng, flat, obs_d, u_d, eps_d = _setup(c, mode)
    what = "%s B=%d %s" % (shape, B, mode)
    # the training step
    eng.workspace(B).fill_(NAN)
    loss, grads = torch.full((1,), NAN, device=DEV), torch.full((eng.n_params,), NAN, device=DEV)
    eng.elbo_step(flat, obs_d, u_d, eps_d, loss, grads=grads)
    assert torch.isfinite(loss).all() and torch.isfinite(grads).all(), what
    worst, werr = U.check_grads(eng.unpack(grads), want["grads"], what=what)
    le = U.loss_err(loss, want["loss"])
    assert le < 1e-5, (what, "loss", loss.item(), want["loss"].item(), le, "worst tensor", worst, werr)
    # the forward-only step (enc_fwd2), as SVI.evaluate_loss takes it ...
    eng.workspace(B).fill_(NAN)
    loss_f = torch.full((1,), NAN, device=DEV)
    eng.elbo_step(flat, obs_d, u_d, eps_d, loss_f, grads=None)
    lf = U.loss_err(loss_f, want["loss"])
    assert lf < 1e-5, (what, "forward-only loss", loss_f.item(), want["loss"].item(), lf)
    # ... and with the trajectories and the latent sample handed back: every trajectory of the batch
    eng.workspace(B).fill_(NAN)
    loss_x = torch.full((1,), NAN, device=DEV)
    x = torch.full((B, c["T"], c["S"]), NAN, device=DEV)
    z = torch.full((B, c["L"]), NAN, device=DEV)
    eng.elbo_step(flat, obs_d, u_d, eps_d, loss_x, grads=None, x_out=x, z_out=z)
    assert torch.isfinite(x).all() and torch.isfinite(z).all(), what
    xe, ze = U.traj_err(x, want["x"]), U.rel(z, want["z"])
    per_traj = ((x.double().cpu() - want["x"]).abs() / want["x"].abs().clamp_min(1.0)).flatten(1).amax(1)
    assert xe < 1e-5, (what, "trajectories", xe, "worst trajectory", int(per_traj.argmax()))
    assert ze < 2e-5, (what, "latent sample", ze)
    assert U.loss_err(loss_x, want["loss"]) < 1e-5, (what, loss_x.item(), want["loss"].item())
    _report(what, loss=le, worst_tensor=worst, worst_err=werr, fwd_loss=lf, x=xe, z=ze)


@pytest.mark.parametrize("B", [1, 129, 1024, 2049, 4097])
def test_metric_shape_exact(B):
    """Split-K 1 / 2 / 8 / 16 with ragged last waves, more than 32 trajectories per wave above 2048; enc_fwd2 tiles TBE / 2 TBE / 4 TBE."""
    _main_step_case("metric", B, "exact")


@pytest.mark.parametrize("B", [1024, 4097])
def test_metric_shape_reference_adjoint(B):
    """bench.py's second line: the other backward instantiation."""
    _main_step_case("metric", B, "reference_adjoint")


@pytest.mark.parametrize("mode", ["exact", "reference_adjoint"])
def test_config4_shard(mode):
    """The whole B = 512 shard of config[4] (challenge, Gauss, rk4, T = 300, L = 15) in one launch."""
    _main_step_case("config4", 512, mode)


@pytest.mark.parametrize("B", [2048, 4096])
def test_config2_fixed_grid(B):
    """L = 50: enc_fwd2's MFMA heads in the 2 TBE and 4 TBE tiles, long slab rows."""
    _main_step_case("config2", B, "exact")


@pytest.mark.parametrize("B", [1024, 4097])
def test_aux_step_metric_shape(B):
    """slode_aux_step (the second SVI object of run_batch) on the whole batch."""
    c = _case("metric", B, "exact", which="aux")
    want = c["want"]
    eng, flat, obs_d, u_d, eps_d = _setup(c, "exact")
    what = "aux B=%d" % B
    eng.workspace(B).fill_(NAN)
    loss, grads = torch.full((1,), NAN, device=DEV), torch.full((eng.n_params,), NAN, device=DEV)
    eng.aux_step(flat, obs_d, u_d, eps_d, loss, grads)
    assert torch.isfinite(loss).all() and torch.isfinite(grads).all(), what
    worst, werr = U.check_grads(eng.unpack(grads), want["grads"], what=what)
    le = U.loss_err(loss, want["loss"])
    assert le < 1e-5, (what, loss.item(), want["loss"].item(), le, "worst tensor", worst, werr)
    _report(what, loss=le, worst_tensor=worst, worst_err=werr)


def test_dopri5_config2_both_sides_of_the_lane_switch():
    """config[2] with dopri5 at the engine's default tolerances (rtol 1e-7, atol 1e-9), forward only, at B = 16 x CUs (the last batch the
    forward solve gives 16 lanes per trajectory) and one more (8 lanes): the loss within 2e-5 of the fp64 oracle at rtol 1e-8 / atol 1e-10
    with one controller per trajectory, and every trajectory within 1e-3 (the bars of test_dopri5_forward_solution_level).  The
    trajectories of a per-trajectory controller do not depend on each other, so the smaller launch takes the first rows of the larger
    batch: one oracle solve serves the trajectory checks of both, and the smaller batch's loss is the larger's minus its last row's.
    (The training step at these sizes, gradients included, against the oracle at the engine's own tolerances:
    test_dopri5_config2_training_step_both_sides_of_the_lane_switch.)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B1 = 16 * ncu
    assert (B1 + 3) // 4 <= 4 * ncu < (B1 + 1 + 3) // 4          # dp5_lanes (csrc/slode_api.hip): 16 lanes at B1, 8 at B1 + 1
    B2, T, S = B1 + 1, 100, 8
    kw = dict(z_g=10, z_eps=10, solver="dopri5")
    ospec = O.proc_spec(**kw)
    ospec.solver_kw = dict(rtol=1e-8, atol=1e-10, per_trajectory=True)
    p = U.params(ospec, T, S)
    obs, u, eps, times = O.synthetic_batch(ospec, B2, T)
    whole = U.oracle(p, ospec, obs, u, eps, times, grads=False)
    last = U.oracle(p, ospec, obs[B1:], u[B1:], eps[B1:], times, grads=False)
    eng = U.engine("proc", kw, T, DEV)
    eng.set_times(times)
    flat = eng.pack(p)
    obs_d, u_d, eps_d = obs.to(DEV), u.to(DEV), eps.to(DEV)
    for B, want_loss in ((B1, whole["loss"] - last["loss"]), (B2, whole["loss"])):
        what = "config2 dopri5 B=%d" % B
        eng.workspace(B).fill_(NAN)
        loss = torch.full((1,), NAN, device=DEV)
        eng.elbo_step(flat, obs_d[:B], u_d[:B].contiguous(), eps_d[:B].contiguous(), loss, grads=None)
        le = U.loss_err(loss, want_loss)
        assert le < 2e-5, (what, loss.item(), want_loss.item(), le)
        eng.workspace(B).fill_(NAN)
        loss_x, x = torch.full((1,), NAN, device=DEV), torch.full((B, T, S), NAN, device=DEV)
        eng.elbo_step(flat, obs_d[:B], u_d[:B].contiguous(), eps_d[:B].contiguous(), loss_x, grads=None, x_out=x)
        assert torch.isfinite(x).all(), what
        xe = U.traj_err(x, whole["x"][:B])
        assert xe < 1e-3, (what, "trajectories", xe)
        assert U.loss_err(loss_x, want_loss) < 2e-5, (what, loss_x.item(), want_loss.item())
        _report(what, loss=le, x=xe)


# ---------------------------------------------------------------------------------------------------------------------------------
# dopri5 training steps at full size (BASELINE config[2]) and at the step-record capacity
# ---------------------------------------------------------------------------------------------------------------------------------
DP5 = {
    # name: (family, spec kwargs, T, S, time scale) -- the time scale of the cvs dopri5 cases of test_gpu_parity.py
    "config2": ("proc", dict(z_g=10, z_eps=10, solver="dopri5"), 100, 8, 1.0),
    "cvs": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2, solver="dopri5"), 60, 5, 0.25),
}
ENGINE_TOL = dict(rtol=1e-7, atol=1e-9, per_trajectory=True)   # the engine's defaults (torchdiffeq's), one controller per trajectory
TIGHT_TOL = dict(rtol=1e-10, atol=1e-12, per_trajectory=True)


def _dp5_inputs(shape, B, mode):
    fam, kw, T, S, ts = DP5[shape]
    ospec = dataclasses.replace(U.OSPEC[fam](**kw), grad_mode=mode)
    p = U.params(ospec, T, S)
    obs, u, eps, times = O.synthetic_batch(ospec, B, T)
    return fam, kw, T, S, ospec, p, obs, u, eps, times * ts


def _dp5_oracle(shape, B, mode):
    """fp64 oracle at the engine's tolerances on B trajectories, the same for their first B - 1 (the whole run minus a run of the last
    trajectory: trajectories are independent under a per-trajectory controller), and the oracle's sensitivity to the step sequence per
    tensor, from the first 64 trajectories at the engine's and at tight tolerances (a tight run at full size is out of reach)."""
    key = ("dp5", shape, B, mode)
    if key not in _cache:
        fam, kw, T, S, ospec, p, obs, u, eps, times = _dp5_inputs(shape, B, mode)
        ospec.solver_kw = ENGINE_TOL
        whole = U.oracle(p, ospec, obs, u, eps, times)
        last = U.oracle(p, ospec, obs[B - 1:], u[B - 1:], eps[B - 1:], times)
        first = dict(loss=whole["loss"] - last["loss"], grads={k: v - last["grads"][k] for k, v in whole["grads"].items()},
                     x=whole["x"][:B - 1])
        sl = slice(0, 64)
        loose64 = U.oracle(p, ospec, obs[sl], u[sl], eps[sl], times)
        ospec.solver_kw = TIGHT_TOL
        sens = U.step_sensitivity(loose64, U.oracle(p, ospec, obs[sl], u[sl], eps[sl], times))
        _cache[key] = dict(fam=fam, kw=kw, T=T, S=S, p=p, obs=obs, u=u, eps=eps, times=times, want={B: whole, B - 1: first}, sens=sens)
    return _cache[key]


def _dp5_training_case(shape, B, mode, oracle_B):
    """The training step at B (the first B of the oracle's oracle_B trajectories), workspace and outputs filled with NaN first: the loss
    within 2e-5 + 3x the sensitivity of the loss, every gradient tensor within 5e-4 + 3x its own (test_dopri5_elbo_step_solution_level's
    bars), every trajectory within 2e-4 max(1, |x|), the forward-only loss too.  (The trajectory bar: twice test_dopri5_elbo_step_at_default_
    tolerances' 1e-4 against the TRUE solution -- here both sides carry a solver error of that size.)"""
    c = _dp5_oracle(shape, oracle_B, mode)
    want, sens, T, S = c["want"][B], c["sens"], c["T"], c["S"]
    eng = U.engine(c["fam"], c["kw"], T, DEV, mode)
    assert (eng.spec.rtol, eng.spec.atol) == (ENGINE_TOL["rtol"], ENGINE_TOL["atol"])
    eng.set_times(c["times"])
    flat = eng.pack(c["p"])
    obs_d, u_d, eps_d = U.to_device(c["obs"][:B], DEV), c["u"][:B].to(DEV).contiguous(), c["eps"][:B].to(DEV).contiguous()
    what = "%s dopri5 B=%d %s" % (shape, B, mode)
    eng.workspace(B).fill_(NAN)
    loss, grads = torch.full((1,), NAN, device=DEV), torch.full((eng.n_params,), NAN, device=DEV)
    x = torch.full((B, T, S), NAN, device=DEV)
    eng.elbo_step(flat, obs_d, u_d, eps_d, loss, grads=grads, x_out=x)
    assert torch.isfinite(loss).all() and torch.isfinite(grads).all() and torch.isfinite(x).all(), what
    steps = eng.dopri5_step_counts(B)
    assert int(steps.min()) >= 1 and int(steps.max()) <= U.dopri5_kmax(B, S), (what, int(steps.min()), int(steps.max()))
    worst, werr = U.check_grads(eng.unpack(grads), want["grads"], what=what, sens=sens)
    lbar = 2e-5 + 3.0 * sens["loss"]
    le = U.loss_err(loss, want["loss"])
    assert le < lbar, (what, "loss", loss.item(), want["loss"].item(), le, lbar)
    xe = U.traj_err(x, want["x"])
    assert xe < 2e-4, (what, "trajectories", xe, "oracle's own", sens["x"])
    eng.workspace(B).fill_(NAN)
    loss_f = torch.full((1,), NAN, device=DEV)
    eng.elbo_step(flat, obs_d, u_d, eps_d, loss_f, grads=None)
    lf = U.loss_err(loss_f, want["loss"])
    assert lf < lbar, (what, "forward-only loss", loss_f.item(), want["loss"].item(), lf, lbar)
    ms_name, ms = U.worst_sensitivity(sens)
    _report(what, loss=le, worst_tensor=worst, worst_err=werr, its_sens=sens[worst], fwd_loss=lf, x=xe, loss_sens=sens["loss"],
            x_sens=sens["x"], max_sens_tensor=ms_name, max_sens=ms, steps="%d-%d" % (int(steps.min()), int(steps.max())))


def _lane_switch_batches():
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B1 = 16 * ncu
    assert (B1 + 3) // 4 <= 4 * ncu < (B1 + 1 + 3) // 4          # dp5_lanes (csrc/slode_api.hip): 16 lanes at B1, 8 at B1 + 1
    return B1


@pytest.mark.parametrize("side", ["16_lanes", "8_lanes"])
def test_dopri5_config2_training_step_both_sides_of_the_lane_switch(side):
    """BASELINE config[2] (proc, latent dim 50, T = 100, dopri5 at the engine's default tolerances): the training step at B1 = 16 x CUs
    (16 lanes per trajectory in the forward solve) and at B1 + 1 (8 lanes) against ONE fp64 oracle run at B1 + 1 with the engine's own
    tolerances (the B1 case takes its first B1 trajectories).  The oracle at tight tolerances is affordable on 64 trajectories only: that
    slice gives the sensitivity terms of the bars."""
    B1 = _lane_switch_batches()
    _dp5_training_case("config2", B1 if side == "16_lanes" else B1 + 1, "exact", B1 + 1)


def test_dopri5_config2_training_step_reference_adjoint():
    """The reverse sweep's other instantiation (latent detached inside the dynamics) at B1 + 1 = 16 x CUs + 1."""
    B1 = _lane_switch_batches()
    _dp5_training_case("config2", B1 + 1, "reference_adjoint", B1 + 1)


def test_dopri5_cvs_training_step_full_size():
    """The other template instantiation of both solver kernels (S = 5: cvs, T = 60, times scaled by 1/4 as in test_gpu_parity.py) at
    B1 + 1 = 16 x CUs + 1 (8 lanes per trajectory).  Its fp64 oracle at the engine's tolerances takes about as long as config[2]'s at
    this size (40 s against 34 s for B = 4097 on eight CPU threads), so it runs at the same B."""
    B1 = _lane_switch_batches()
    _dp5_training_case("cvs", B1 + 1, "exact", B1 + 1)


# The step-record capacity: the forward solve records every accepted step (t, dt, y) for the reverse sweep, kmax steps per trajectory,
# kmax = 2^26 / (B (S + 2)) within [64, 2048]: 102 at the largest batch the dopri5 step takes (B = 65,536, S = 8).  The whole batch is
# compared with 16 launches of 4096 trajectories each (kmax = 1638, a sixteenth of the record stride, the 16-lane forward solve).
B_MAX = 65536
N_SLICES = 16


def _engine_with_tol(fam, kw, T, rtol, atol):
    from structured_latent_odes_amd import engine as E
    espec = {"cvs": E.cvs_spec, "challenge": E.challenge_spec, "proc": E.proc_spec}[fam](**kw)
    espec = dataclasses.replace(espec, rtol=rtol, atol=atol)
    return E.Engine(espec, T, DEV)


def _capacity_inputs():
    key = ("capacity",)
    if key not in _cache:
        _cache[key] = _dp5_inputs("config2", B_MAX, "exact")
    return _cache[key]


def _capacity_run(eng, flat, sl, grads=True, x=True):
    """One launch on trajectories `sl` of the B_MAX batch, workspace and outputs NaN first: (loss, grads, x, step counts)."""
    _, _, T, S, _, _, obs, u, eps, _ = _capacity_inputs()
    B = sl.stop - sl.start
    eng.workspace(B).fill_(NAN)
    loss = torch.full((1,), NAN, device=DEV)
    g = torch.full((eng.n_params,), NAN, device=DEV) if grads else None
    xo = torch.full((B, T, S), NAN, device=DEV) if x else None
    eng.elbo_step(flat, obs[sl].to(DEV), u[sl].to(DEV).contiguous(), eps[sl].to(DEV).contiguous(), loss, grads=g, x_out=xo)
    return loss, g, xo, eng.dopri5_step_counts(B)


def _slices(eng, flat):
    n = B_MAX // N_SLICES
    return [_capacity_run(eng, flat, slice(i * n, (i + 1) * n)) for i in range(N_SLICES)]


@pytest.mark.parametrize("rtol", [1e-7, 3e-8])
def test_dopri5_step_records_at_the_largest_batch(rtol):
    """Inside the capacity at B = 65,536 (config[2], kmax = 102): every step count within [1, kmax]; the whole launch against 16 launches
    of 4096: step counts equal, trajectories bitwise equal, the loss additive to 1e-6, every gradient tensor additive to 1e-5 -- the
    record indexing at the largest stride the code allows.  rtol 1e-7 (atol 1e-9): the engine's defaults; rtol 3e-8 (atol 3e-10): the
    records of the longest trajectory fill more than half the capacity (a capacity half as large overflows there)."""
    fam, kw, T, S, ospec, p, obs, u, eps, times = _capacity_inputs()
    kmax = U.dopri5_kmax(B_MAX, S)
    assert kmax == 102
    eng = _engine_with_tol(fam, kw, T, rtol, rtol * 1e-2)
    eng.set_times(times)
    flat = eng.pack(p)
    loss, grads, x, steps = _capacity_run(eng, flat, slice(0, B_MAX))
    lo, hi = int(steps.min()), int(steps.max())
    assert 1 <= lo and hi <= kmax, (lo, hi, kmax)
    if rtol < 1e-7:
        assert hi > kmax // 2, (hi, kmax)
    assert torch.isfinite(loss).all() and torch.isfinite(grads).all() and torch.isfinite(x).all(), "step records overflowed inside kmax"
    parts = _slices(eng, flat)
    n = B_MAX // N_SLICES
    assert torch.equal(steps, torch.cat([q[3] for q in parts])), "step counts of the whole batch and of its slices"
    for i, q in enumerate(parts):
        assert torch.equal(x[i * n:(i + 1) * n], q[2]), ("trajectories of slice", i)
    ls = sum(q[0].double() for q in parts)
    assert abs((ls - loss.double()).item()) / abs(loss.item()) < 1e-6, (loss.item(), ls.item())
    bad = U.additivity_per_tensor(eng, [q[1] for q in parts], grads)
    assert not bad, bad
    _report("capacity B=%d rtol=%g" % (B_MAX, rtol), steps="%d-%d of %d" % (lo, hi, kmax))


OVERFLOW_TOL = (1e-8, 1e-10)   # rtol, atol: measured at B = 65,536, 46 to 111 accepted steps; 189 trajectories over kmax = 102


def test_dopri5_step_record_overflow_poisons_the_whole_gradient():
    """A tolerance at which some trajectories of the B = 65,536 batch take more accepted steps than the records hold (kmax = 102) and the
    rest do not.  Contract: the training step returns a NaN loss and a gradient that is NaN in EVERY element -- never a finite gradient
    without the overflowed trajectories' solver share (as when max_steps is exhausted) -- and SVI.step (Adam in the same launch) leaves no
    parameter with a finite step taken from partial gradients.  The solve itself is complete: step counts report the true counts (> kmax),
    the trajectories are bitwise those of the 16 slices of 4096 (kmax = 1638: no overflow there, finite gradients), and the forward-only
    loss (no records) is finite and equals the slices' sum."""
    from structured_latent_odes_amd.svi import ELBOStep, FlatAdam
    fam, kw, T, S, ospec, p, obs, u, eps, times = _capacity_inputs()
    kmax = U.dopri5_kmax(B_MAX, S)
    eng = _engine_with_tol(fam, kw, T, *OVERFLOW_TOL)
    eng.set_times(times)
    flat = eng.pack(p)
    loss, grads, x, steps = _capacity_run(eng, flat, slice(0, B_MAX))
    over = int((steps > kmax).sum())
    assert 0 < over < B_MAX and int(steps.min()) >= 1, (over, int(steps.min()), int(steps.max()))
    assert torch.isnan(loss).all(), loss.item()
    finite = {k: int(torch.isfinite(v).sum()) for k, v in eng.unpack(grads).items() if not torch.isnan(v).all()}
    assert not finite, ("gradient elements that are not NaN after a record overflow", finite)
    assert torch.isfinite(x).all()
    parts = _slices(eng, flat)
    n = B_MAX // N_SLICES
    assert torch.equal(steps, torch.cat([q[3] for q in parts]))
    for i, q in enumerate(parts):
        assert torch.isfinite(q[0]).all() and torch.isfinite(q[1]).all(), ("slice", i)
        assert torch.equal(x[i * n:(i + 1) * n], q[2]), ("trajectories of slice", i)
    loss_f, _, _, steps_f = _capacity_run(eng, flat, slice(0, B_MAX), grads=False, x=False)
    ls = sum(q[0].double() for q in parts)
    assert torch.isfinite(loss_f).all() and abs((ls - loss_f.double()).item()) / abs(loss_f.item()) < 1e-6, (loss_f.item(), ls.item())
    assert torch.equal(steps_f, steps)
    # through SVI.step: Adam inside the launch
    opt = FlatAdam(eng, flat, lr=1e-3)
    svi = ELBOStep(eng, flat, opt)
    before = flat.detach().clone()
    l_svi = svi.step(obs.to(DEV), eps=eps.to(DEV).contiguous(), u=u.to(DEV).contiguous())
    assert not np.isfinite(l_svi), l_svi
    after = flat.detach()
    moved = torch.isfinite(after) & (after != before)
    assert not bool(moved.any()), ("parameters stepped from a gradient without the overflowed trajectories", int(moved.sum()))
    _report("overflow B=%d rtol=%g" % (B_MAX, OVERFLOW_TOL[0]), over=over, steps="%d-%d of %d" % (int(steps.min()), int(steps.max()), kmax))


def test_dopri5_step_refuses_more_than_65536_trajectories():
    """B = 65,537: the dopri5 ELBO step (training and forward-only) raises SlodeError naming the limit, and writes neither the loss nor the
    gradient (both filled with a sentinel first)."""
    from structured_latent_odes_amd._lib import SlodeError
    fam, kw, T, S, ospec, p, obs, u, eps, times = _capacity_inputs()
    eng = _engine_with_tol(fam, kw, T, ENGINE_TOL["rtol"], ENGINE_TOL["atol"])
    eng.set_times(times)
    flat = eng.pack(p)
    B = B_MAX + 1
    obs_d = torch.cat([obs, obs[:1]]).to(DEV)
    u_d, eps_d = torch.cat([u, u[:1]]).to(DEV), torch.cat([eps, eps[:1]]).to(DEV)
    assert obs_d.shape[0] == B
    for with_grads in (True, False):
        loss = torch.full((1,), 12345.0, device=DEV)
        grads = torch.full((eng.n_params,), 12345.0, device=DEV)
        with pytest.raises(SlodeError, match="65,536"):
            eng.elbo_step(flat, obs_d, u_d, eps_d, loss, grads=grads if with_grads else None)
        torch.cuda.synchronize()
        assert bool((loss == 12345.0).all()) and bool((grads == 12345.0).all()), with_grads


# ---------------------------------------------------------------------------------------------------------------------------------
# The step as bench.py and training_cvs.run_batch take it: ELBOStep + AuxStep on one FlatAdam, noise drawn in the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _model_steps(T=200):
    from structured_latent_odes_amd.configs import load_config_cvs
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.svi import AuxStep, ELBOStep, FlatAdam
    cfg = load_config_cvs()
    cfg.update(seq_len=T, z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2, solver="rk4", mini_batch_size=1024, adjoint_solver=False)
    ospec = O.cvs_spec(3, 3, 2, solver="rk4")
    times = O.synthetic_batch(ospec, 1, T)[3]
    model = MechanisticModel(cfg, DEV, times.to(DEV))
    b = model._bind()
    eng = b.engine
    assert b.n_total == eng.n_params and eng.spec.grad_mode == "exact"
    eng.pack(U.params(ospec, T, 5), flat=b.flat)
    eng.rng_seed(2026)
    opt = FlatAdam(eng, b.flat, lr=cfg.learning_rate)
    return ospec, times, eng, b.flat, opt, ELBOStep(eng, b.flat, opt), AuxStep(model, opt)


def _params_of(eng, flat):
    return {k: v.detach().cpu().clone() for k, v in eng.unpack(flat).items()}


def _run_pair(ospec, times, eng, flat, main, aux, obs, u, eps=None):
    """One main + one auxiliary step as run_batch takes them (labels by name for the auxiliary one, as the loader yields them); returns
    per step (name, loss, gradient, parameters it saw, parameters after, noise it used)."""
    B, L = obs.shape[0], ospec.latent_dim
    obs_d, u_d = U.to_device(obs, DEV), u.to(DEV).contiguous()
    eps_d = eps.to(DEV).contiguous() if eps is not None else None
    out = []
    for name, svi, call in (("main", main, lambda: main.step(obs_d, eps=eps_d, u=u_d)),
                            ("aux", aux, lambda: aux.step(obs_d, eps=eps_d, iext=u_d[:, 0:1].contiguous(), rtpr=u_d[:, 1:2].contiguous()))):
        seed, b0, n = eng.rng_state()
        before = flat.detach().clone()
        loss = call()
        noise = eps if eps is not None else torch.from_numpy(R.normals(seed, n, b0, B, L))
        if eps is None:
            assert eng.rng_state() == (seed, b0, n + 1), name
        out.append((name, loss, svi.grads.detach().clone(), before, flat.detach().clone(), noise))
    return out


def _check_against_oracle(ospec, times, eng, obs, u, steps, what):
    for name, loss, grads, before, _, noise in steps:
        want = U.oracle(_params_of(eng, before), ospec, obs, u, noise, times, which=name)
        assert np.isfinite(loss) and torch.isfinite(grads).all(), (what, name)
        worst, werr = U.check_grads(eng.unpack(grads[:eng.n_params]), want["grads"], what="%s %s" % (what, name))
        le = U.loss_err(loss, want["loss"])
        assert le < 1e-5, (what, name, loss, want["loss"].item(), le, "worst tensor", worst, werr)
        _report("%s %s" % (what, name), loss=le, worst_tensor=worst, worst_err=werr)


def test_bench_step_with_in_kernel_noise():
    """B = 1024: the noise of each step is rebuilt independently (tests/rng_math.py, keyed by the generator state before the step) and fed
    to the oracle; loss and every gradient tensor at the usual bars.  The updated weights equal torch's Adam applied to the ENGINE's own
    gradient within 2e-6 (not to the oracle's: Adam's first steps move every element by about lr, so a near-zero gradient element whose
    sign rounds differently would flip the expected value)."""
    ospec, times, eng, flat, opt, main, aux = _model_steps()
    B, T = 1024, 200
    obs, u, _, _ = O.synthetic_batch(ospec, B, T)
    steps = _run_pair(ospec, times, eng, flat, main, aux, obs, u)
    _check_against_oracle(ospec, times, eng, obs, u, steps, "bench step B=1024")
    w = steps[0][3].clone().requires_grad_(True)
    ref = torch.optim.Adam([w], lr=opt.lr, betas=opt.betas, eps=opt.eps)
    for name, _, grads, _, after, _ in steps:
        w.grad = grads.clone()
        ref.step()
        err = (after - w.detach()).abs().max().item()
        assert err < 2e-6, ("Adam after the %s step" % name, err)


@pytest.mark.parametrize("noise", ["explicit", "drawn"])
def test_batch_size_changes_between_steps(noise):
    """The tail of one drop_last=False epoch and the start of the next: main + auxiliary step with Adam at B = 1024, 37, 1024, 1 on one
    handle.  Every step's loss and gradient tensors against the oracle at the weights THAT step saw: per-B workspaces, the noise counter
    and the kept encoder fold must not go stale when B changes."""
    ospec, times, eng, flat, opt, main, aux = _model_steps()
    T = 200
    for k, B in enumerate([1024, 37, 1024, 1]):
        obs, u, eps, _ = O.synthetic_batch(ospec, B, T, seed=300 + k)
        steps = _run_pair(ospec, times, eng, flat, main, aux, obs, u, eps if noise == "explicit" else None)
        _check_against_oracle(ospec, times, eng, obs, u, steps, "changing B, step %d B=%d %s" % (k, B, noise))
