"""torchdiffeq's other adaptive Runge-Kutta methods -- bosh3, fehlberg2, adaptive_heun -- through the dopri5 machinery (the kernels of
dopri5_kernel.hip templated on the tableau): solution level, the training step against the fp64 restatement of the same algorithm
(tests/adaptive_rk_ref.py), the 16 / 8-lane forms, the launch boundary, the record overflow contract, the grid check and the reference
API.  Every case fills the workspace and the outputs with NaN first."""
import dataclasses

import pytest
import torch

from oracle import slode_oracle as O
from tests import adaptive_rk_ref as R
from tests import full_size_util as U

pytestmark = pytest.mark.gpu

NEW = ["bosh3", "fehlberg2", "adaptive_heun"]
# Tolerances of the training tests (rtol, atol): the low orders need far more steps than dopri5 at torchdiffeq's defaults (DESIGN 3.3,
# tools/adaptive_steps.py); these keep every trajectory of the B = 38 cases well inside the record (2048 steps) and the oracle's CPU time
# short.
TRAIN_TOL = {"dopri5": (1e-7, 1e-9), "bosh3": (1e-6, 1e-8), "fehlberg2": (1e-6, 1e-8), "adaptive_heun": (1e-5, 1e-7)}
# the solution-level test holds the solve within 1e-3 of the true solution: tighter for the low orders (their error at TRAIN_TOL is larger)
FWD_TOL = {"bosh3": (1e-7, 1e-9), "fehlberg2": (1e-7, 1e-9), "adaptive_heun": (1e-6, 1e-8)}


def _case(fam, method, seed=31):
    from structured_latent_odes_amd import engine as E
    if fam == "proc":
        kw, S, T = dict(z_g=10, z_eps=10), 8, 100
    else:
        kw, S, T = dict(z_iext=3, z_rtpr=3, z_eps=2), 5, 60
    mk_o, mk_e = (O.proc_spec, E.proc_spec) if fam == "proc" else (O.cvs_spec, E.cvs_spec)
    ospec, espec = mk_o(solver="dopri5", **kw), mk_e(solver=method, **kw)
    p = O.init_params(ospec, T=T, S=S)
    g = torch.Generator().manual_seed(seed)
    p = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in p.items()}
    return ospec, espec, p, S, T


def _engine(espec, T, times, dev, rtol=None, atol=None, mode=None):
    from structured_latent_odes_amd import engine as E
    if rtol is not None:
        espec = dataclasses.replace(espec, rtol=rtol, atol=atol)
    if mode is not None:
        espec = dataclasses.replace(espec, grad_mode=mode)
    eng = E.Engine(espec, T, dev)
    eng.set_times(times)
    return eng


def _step(eng, flat, obs_d, u, eps, B, T, S, dev, grads=True):
    loss = torch.full((1,), float("nan"), device=dev)
    g = torch.full((eng.n_params,), float("nan"), device=dev) if grads else None
    x = torch.full((B, T, S), float("nan"), device=dev)
    eng.workspace(B).fill_(float("nan"))
    eng.elbo_step(flat, obs_d, u.to(dev), eps.to(dev), loss, grads=g, x_out=x)
    torch.cuda.synchronize()
    return loss, g, x


@pytest.mark.parametrize("fam", ["cvs", "proc"])
@pytest.mark.parametrize("method", NEW)
def test_forward_solution_level(method, fam):
    """The bare solve of each new method (B = 38: two sixteen-trajectory workgroups and a ragged third) against a tight fp64 solve: as
    close as the same algorithm in fp32 on the CPU (x3 + 1e-5) and within 1e-3 -- the bars of test_dopri5_forward_solution_level."""
    dev = torch.device("cuda:0")
    ospec, espec, p, S, T = _case(fam, method, seed=21)
    rtol, atol = FWD_TOL[method]
    B = 38
    _, _, _, times = O.synthetic_batch(ospec, 4, T)
    if fam == "cvs":
        times = times * 0.25
    g = torch.Generator().manual_seed(21)
    z = torch.randn(B, ospec.latent_dim, generator=g)
    eng = _engine(espec, T, times, dev, rtol, atol)
    x = eng.ode_solve(eng.pack(p), z.to(dev))
    assert torch.isfinite(x).all()
    p64 = {k: v.double() for k, v in p.items()}
    tight = O.solve_ode(p64, z.double(), times.double(), "dopri5", rtol=1e-10, atol=1e-12, per_trajectory=True)
    with R.patched(R.TABLEAUS[method]):
        ref32 = O.solve_ode(p, z, times, "dopri5", rtol=rtol, atol=atol, per_trajectory=True)
    scale = tight.abs().clamp_min(1.0)
    err_gpu = ((x.cpu().double() - tight).abs() / scale).max().item()
    err_ref = ((ref32.double() - tight).abs() / scale).max().item()
    print("%s %s: solution error %.2e (fp32 restatement %.2e)" % (method, fam, err_gpu, err_ref))
    assert err_gpu < 3.0 * err_ref + 1e-5, (err_gpu, err_ref)
    assert err_gpu < 1e-3


@pytest.mark.parametrize("mode", ["exact", "reference_adjoint"])
@pytest.mark.parametrize("method", NEW)
def test_elbo_step_against_oracle(method, mode):
    """The training step (cvs, B = 38) at TRAIN_TOL against the fp64 oracle at tight tolerances: -ELBO and EVERY gradient tensor within
    5e-4 + 3x the oracle's own sensitivity to the step sequence (the fp64 restatement of the same method at the same tolerances against
    the tight solve; the bar of test_dopri5_elbo_step_at_default_tolerances), trajectories within 1e-4 + 3x theirs.  The accepted steps
    per trajectory equal the fp64 restatement's within 3 + 5 % (their sum within 2 %); the forward-only loss scores the same solution; a repeat is bitwise."""
    dev = torch.device("cuda:0")
    ospec, espec, p, S, T = _case("cvs", method)
    ospec.grad_mode = mode
    rtol, atol = TRAIN_TOL[method]
    B = 38
    obs, u, eps, times = O.synthetic_batch(ospec, B, T)
    times = times * 0.25
    eng = _engine(espec, T, times, dev, rtol, atol, mode)
    flat = eng.pack(p)
    obs_d = U.to_device(obs, dev)
    loss, grads, x = _step(eng, flat, obs_d, u, eps, B, T, S, dev)
    assert torch.isfinite(loss).all() and torch.isfinite(grads).all() and torch.isfinite(x).all()
    n = eng.dopri5_step_counts(B).cpu().long()
    assert int(n.min()) >= 1 and int(n.max()) <= U.dopri5_kmax(B, S), n
    ospec.solver_kw = dict(rtol=1e-10, atol=1e-12, per_trajectory=True)
    tight = U.oracle(p, ospec, obs, u, eps, times)
    ospec.solver_kw = dict(rtol=rtol, atol=atol, per_trajectory=True)
    counts = []
    with R.patched(R.TABLEAUS[method], counts):
        loose = U.oracle(p, ospec, obs, u, eps, times)
    sens = U.step_sensitivity(loose, tight)
    # fp32 and fp64 controllers part ways at accept / reject decisions on the tolerance boundary (measured: up to 5 of ~100 steps for bosh3);
    # a wrong error weight or controller exponent moves every trajectory's count the same way
    dn = (n - counts[0]).abs()
    assert bool((dn <= 3 + (0.05 * counts[0]).long()).all()), ("step counts off the fp64 restatement", n.tolist(), counts[0].tolist())
    assert abs(int(n.sum()) - int(counts[0].sum())) <= 0.02 * int(counts[0].sum()), (int(n.sum()), int(counts[0].sum()))
    le = U.loss_err(loss, tight["loss"])
    assert le < 5e-4 + 3.0 * sens["loss"], (le, sens["loss"])
    xe = U.traj_err(x, tight["x"])
    assert xe < 1e-4 + 3.0 * sens["x"], (xe, sens["x"])
    worst, werr = U.check_grads(eng.unpack(grads), tight["grads"], sens=sens, what="%s cvs %s" % (method, mode))
    print("%s %s: steps %d..%d, loss %.2e (sens %.2e), x %.2e (sens %.2e), worst tensor %s %.2e (sens %.2e)"
          % (method, mode, int(n.min()), int(n.max()), le, sens["loss"], xe, sens["x"], worst, werr, sens[worst]))
    loss2, _, x2 = _step(eng, flat, obs_d, u, eps, B, T, S, dev, grads=False)
    assert abs(loss2.item() - loss.item()) <= 2e-6 * abs(loss.item())
    loss3, grads3, x3 = _step(eng, flat, obs_d, u, eps, B, T, S, dev)
    assert torch.equal(loss, loss3) and torch.equal(grads, grads3) and torch.equal(x, x3)


@pytest.mark.parametrize("fam", ["cvs", "proc"])
@pytest.mark.parametrize("method", NEW)
def test_sixteen_lanes_equal_eight_lanes_bitwise(method, fam, monkeypatch):
    """The forward kernel (dopri5_fwd_kernel) at 16 lanes per trajectory against 8 (SLODE_DP5_LPT=8, read in slode_create): trajectories, step counts, -ELBO and
    every gradient element bit for bit.  SLODE_DP5_LPT=32 / 64 are dopri5 only: the step refuses them for the new methods."""
    from structured_latent_odes_amd._lib import SlodeError
    dev = torch.device("cuda:0")
    ospec, espec, p, S, T = _case(fam, method)
    rtol, atol = TRAIN_TOL[method]
    B = 37
    obs, u, eps, times = O.synthetic_batch(ospec, B, T)
    if fam == "cvs":
        times = times * 0.25
    obs_d = U.to_device(obs, dev)
    out = {}
    for lpt in ("16", "8"):
        monkeypatch.setenv("SLODE_DP5_LPT", lpt)
        eng = _engine(espec, T, times, dev, rtol, atol)
        flat = eng.pack(p)
        loss, grads, x = _step(eng, flat, obs_d, u, eps, B, T, S, dev)
        out[lpt] = (loss.cpu(), grads.cpu(), x.cpu(), eng.dopri5_step_counts(B).cpu())
    assert torch.isfinite(out["16"][0]).all()
    for a, b in zip(out["16"], out["8"]):
        assert torch.equal(a, b)
    monkeypatch.setenv("SLODE_DP5_LPT", "32")
    eng = _engine(espec, T, times, dev, rtol, atol)
    with pytest.raises(SlodeError):
        _step(eng, eng.pack(p), obs_d, u, eps, B, T, S, dev)


def test_bosh3_config2_on_both_sides_of_the_lane_switch():
    """bosh3 at BASELINE config[2]'s shape (proc, L = 50, S = 8, T = 100) at B = 4096 (16 lanes per trajectory) and B = 4097 (8 lanes): the
    4097 launch equals launches of 4096 + 1 -- step counts equal, trajectories bitwise, loss and every gradient tensor additive within
    1e-5 -- and a 64-trajectory slice is checked against the fp64 oracle."""
    dev = torch.device("cuda:0")
    ospec, espec, p, S, T = _case("proc", "bosh3")
    rtol, atol = TRAIN_TOL["bosh3"]
    B = 4097
    obs, u, eps, times = O.synthetic_batch(ospec, B, T)
    eng = _engine(espec, T, times, dev, rtol, atol)
    flat = eng.pack(p)
    loss, grads, x = _step(eng, flat, U.to_device(obs, dev), u, eps, B, T, S, dev)
    n = eng.dopri5_step_counts(B).cpu()
    assert torch.isfinite(loss).all() and torch.isfinite(grads).all()
    assert int(n.min()) >= 1 and int(n.max()) <= U.dopri5_kmax(B, S)
    parts = []
    for lo, hi in ((0, 4096), (4096, 4097)):
        l_, g_, x_ = _step(eng, flat, U.to_device(obs[lo:hi], dev), u[lo:hi], eps[lo:hi], hi - lo, T, S, dev)
        assert torch.equal(eng.dopri5_step_counts(hi - lo).cpu(), n[lo:hi])
        assert torch.equal(x_.cpu(), x[lo:hi].cpu())
        parts.append((l_, g_))
    lsum = sum(float(l_.item()) for l_, _ in parts)
    assert abs(lsum - loss.item()) <= 1e-5 * abs(loss.item())
    bad = U.additivity_per_tensor(eng, [g_ for _, g_ in parts], grads)
    assert not bad, bad
    # the slice against the oracle (its own launch: 64 trajectories, 8 lanes)
    sl = slice(0, 64)
    l64, g64, x64 = _step(eng, flat, U.to_device(obs[sl], dev), u[sl], eps[sl], 64, T, S, dev)
    assert torch.equal(x64.cpu(), x[sl].cpu())
    ospec.solver_kw = dict(rtol=1e-10, atol=1e-12, per_trajectory=True)
    tight = U.oracle(p, ospec, obs[sl], u[sl], eps[sl], times)
    ospec.solver_kw = dict(rtol=rtol, atol=atol, per_trajectory=True)
    with R.patched(R.BOSH3):
        loose = U.oracle(p, ospec, obs[sl], u[sl], eps[sl], times)
    sens = U.step_sensitivity(loose, tight)
    assert U.loss_err(l64, tight["loss"]) < 5e-4 + 3.0 * sens["loss"]
    assert U.traj_err(x64, tight["x"]) < 1e-4 + 3.0 * sens["x"]
    U.check_grads(eng.unpack(g64), tight["grads"], sens=sens, what="bosh3 config[2] slice")


def test_record_overflow_returns_nan_gradients():
    """adaptive_heun at torchdiffeq's default tolerances (rtol 1e-7, atol 1e-9), whose step counts exceed the record (B = 38: 2048 steps) but
    not the 20,000 attempts: NaN loss and an all-NaN gradient; the trajectories and the forward-only loss are those of the complete solve."""
    dev = torch.device("cuda:0")
    ospec, espec, p, S, T = _case("cvs", "adaptive_heun")
    B = 38
    obs, u, eps, times = O.synthetic_batch(ospec, B, T)
    times = times * 0.25
    eng = _engine(espec, T, times, dev, 1e-7, 1e-9)
    flat = eng.pack(p)
    obs_d = U.to_device(obs, dev)
    loss, grads, x = _step(eng, flat, obs_d, u, eps, B, T, S, dev)
    n = eng.dopri5_step_counts(B).cpu()
    assert int(n.min()) >= 1 and int(n.max()) > U.dopri5_kmax(B, S), n      # overflowed, not exhausted
    print("adaptive_heun rtol 1e-7: steps %d..%d, %d of %d trajectories over %d" % (int(n.min()), int(n.max()), int((n > U.dopri5_kmax(B, S)).sum()), B, U.dopri5_kmax(B, S)))
    assert torch.isnan(loss).all() and torch.isnan(grads).all()
    assert torch.isfinite(x).all()
    loss_f, _, x_f = _step(eng, flat, obs_d, u, eps, B, T, S, dev, grads=False)
    assert torch.isfinite(loss_f).all()
    assert torch.equal(x_f, x)


@pytest.mark.parametrize("method", NEW)
def test_set_times_refuses_grids_it_cannot_walk(method):
    dev = torch.device("cuda:0")
    ospec, espec, p, S, T = _case("cvs", method)
    _, _, _, times = O.synthetic_batch(ospec, 2, T)
    from structured_latent_odes_amd import engine as E
    eng = E.Engine(espec, T, dev)
    with pytest.raises(ValueError):
        eng.set_times(times.flip(0))
    t2 = times.clone()
    t2[5] = t2[4]
    with pytest.raises(ValueError):
        eng.set_times(t2)
    eng.set_times(times)


def test_reference_api_with_bosh3():
    """A cvs model built with config.solver = "bosh3" runs training.run_batch and recon_samples, and its loss equals the engine-level
    step on the same noise."""
    from structured_latent_odes_amd.configs import load_config_cvs
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.svi import SVI, Adam, Trace_ELBO
    from structured_latent_odes_amd.synthetic import synthetic_batch
    from structured_latent_odes_amd import training
    dev = torch.device("cuda:0")
    T, B = 86, 24
    cfg = load_config_cvs()
    cfg.update(seq_len=T, solver="bosh3")
    torch.manual_seed(3)
    times = torch.arange(0.0, T * 1.0, 1.0, device=dev) * 0.25
    m = MechanisticModel(cfg, dev, times)
    obs, labels, _ = synthetic_batch("cvs", B, T, 3, seed=7)
    batch = {"observations": obs.to(dev), "iext": labels["iext"].to(dev), "rtpr": labels["rtpr"].to(dev)}
    eps = torch.randn(B, m.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
    b = m._bind()
    eng, flat = b.engine, b.flat
    assert eng.spec.solver == "bosh3"
    u = torch.cat([batch["iext"], batch["rtpr"]], 1)
    loss = torch.zeros(1, device=dev)
    eng.elbo_step(flat, batch["observations"], u, eps, loss, grads=torch.zeros(eng.n_params, device=dev))
    svi = SVI(m.model, m.guide, Adam({"lr": 1e-3}), loss=Trace_ELBO(num_particles=1))
    got = svi.evaluate_loss(eps=eps, **batch)
    assert abs(got - loss.item()) <= 1e-6 * abs(loss.item()), (got, loss.item())
    losses = training.run_batch(batch, [svi])
    assert all(torch.isfinite(torch.tensor(losses)))
    n = eng.dopri5_step_counts(B)
    assert int(n.min()) >= 1
    res = m.recon_samples(batch["observations"], True, 3, iext=batch["iext"], rtpr=batch["rtpr"])
    assert res["mu_50"].shape == (B, 3, T, 3) and torch.isfinite(res["mu_50"]).all()


@pytest.mark.parametrize("method", NEW)
def test_step_is_bitwise_repeatable(method):
    dev = torch.device("cuda:0")
    ospec, espec, p, S, T = _case("proc", method)
    rtol, atol = TRAIN_TOL[method]
    B = 300
    obs, u, eps, times = O.synthetic_batch(ospec, B, T)
    eng = _engine(espec, T, times, dev, rtol, atol)
    flat = eng.pack(p)
    obs_d = U.to_device(obs, dev)
    a = _step(eng, flat, obs_d, u, eps, B, T, S, dev)
    b = _step(eng, flat, obs_d, u, eps, B, T, S, dev)
    assert torch.isfinite(a[0]).all()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
