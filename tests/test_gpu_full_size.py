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
    (Gradients at full size: out of the oracle's reach in seconds; linearity per tensor in test_gpu_parity.py covers them.)"""
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
