"""GPU tests of the posterior refinement (slode_posterior_refine / Engine.posterior_refine / MechanisticBase.refine_posterior /
save_refined_posterior / recon_samples(posterior=...)) against the fp64 reference loop of tests/refine_util.py.  Bars: that module's
docstring.  Outputs are pre-filled with NaN: every element must be written.  One kernel call and one reference per configuration, shared
among the tests that read them and left unchanged."""
import os

import numpy as np
import pytest
import torch

from tests import refine_util as RU
from tests.eval_gpu_util import _device_batch, _engine, _lay, _model, _refused

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CONFIGS = [(case, solver) for case in RU.CASES for solver in RU.SOLVERS]
NAMES = ("loc", "scale", "elbo", "grad0", "trace", "best_step")


def _refine(eng, flat, c, J, eps="case", K=None, lr=RU.LR, w=None, t_major=True):
    """Engine.posterior_refine on the case's batch -> dict of the six outputs (device tensors)."""
    _, labels = _device_batch(c)
    obs_d = _lay(c["obs"], t_major)
    K = c["K"] if K is None else K
    e = c["eps"] if isinstance(eps, str) else eps
    if e is not None:
        e = (e[0] if K == 1 and e.dim() == 3 else e).to(DEV).contiguous()
    B, L = c["B"], c["ospec"].latent_dim
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = eng.posterior_refine(flat, eng.make_batch(obs_d, labels, e, particles=max(K, 1)), B, K, J, lr, mask=None if w is None else _lay(w, t_major),
                               loc=nan(B, L), scale=nan(B, L), elbo=nan(B, 2), grad0=nan(B, 2 * L), trace=nan(max(J, 0) + 1, B),
                               best_step=torch.full((B,), -7, dtype=torch.int32, device=DEV))
    return dict(zip(NAMES, out))


def _np(r):
    return {k: v.detach().double().cpu().numpy() for k, v in r.items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in NAMES)


_RUNS = {}


def _run(case, solver, masked):
    """(c, w, the fp64 reference, the kernel's outputs as numpy) of J = 4, lr = 0.05, B = 5, K = 3: once per configuration."""
    key = (case, solver, masked)
    if key not in _RUNS:
        c, w, ref = RU.reference(case, solver, masked)
        eng = _engine(c)
        _RUNS[key] = (c, w, ref, _np(_refine(eng, eng.pack(c["p"]), c, RU.J, w=w)))
    return _RUNS[key]


def _check_against_reference(got, ref, tag, J=RU.J):
    """grad0 within 5e-4 norm-wise, the trace within (1 + 4 RHO) bar, elbo0 / elbo / best_step consistent with the trace."""
    bar = RU.REL * ref["mag"]
    ge = RU.norm_err(got["grad0"], ref["grad0"])
    te = np.abs(got["trace"] - ref["trace"]) / bar
    print("%s: grad0 error %.2e (bar %.0e); trace error / bar %.3f (allowed %.2f)" % (tag, ge.max(), RU.GRAD_REL, te.max(), 1 + 4 * RU.RHO))
    assert all(np.isfinite(v).all() for v in got.values()), tag
    assert ge.max() <= RU.GRAD_REL, (tag, ge)
    assert te.max() <= 1 + 4 * RU.RHO, (tag, te)
    assert np.array_equal(got["elbo"][:, 0], got["trace"][0]) and np.array_equal(got["elbo"][:, 1], got["trace"].min(0)), tag
    assert np.array_equal(got["best_step"], got["trace"].argmin(0)), tag                   # (argmin: the lowest index on a tie)


@pytest.mark.parametrize("case,solver", CONFIGS)
def test_zero_steps_return_the_encoder_posterior_and_the_trajectory_bound(case, solver):
    """J = 0: loc / scale are bitwise what the encoder launch left in the workspace (and the unfused encoder's to 1e-5); elbo0 == elbo; both
    equal slot 0 of trajectory_bounds on the same noise to one fp32 ulp; best_step 0; trace [1, B] = elbo0."""
    c = RU.build(case, solver)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    r = _refine(eng, flat, c, 0)
    torch.cuda.synchronize(DEV)
    ws = eng.workspace(c["B"]).cpu().numpy().tobytes()
    assert ws.find(r["loc"].cpu().numpy().tobytes()) >= 0 and ws.find(r["scale"].cpu().numpy().tobytes()) >= 0
    obs_d, labels = _device_batch(c)
    loc, scale, _, _ = eng.encoder_fwd(flat, obs_d, save=False)
    assert torch.allclose(loc, r["loc"], rtol=1e-5, atol=1e-6) and torch.allclose(scale, r["scale"], rtol=1e-5, atol=1e-7)
    assert torch.equal(r["elbo"][:, 0], r["elbo"][:, 1]) and torch.equal(r["trace"][0], r["elbo"][:, 0]) and int(r["best_step"].abs().sum()) == 0
    bounds, _ = eng.traj_bounds(flat, eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=c["K"]), c["B"], c["K"])
    got, want = r["elbo"][:, 0].double().cpu().numpy(), bounds[:, 0].double().cpu().numpy()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("%s/%s: elbo0 against trajectory_bounds: %.2f ulp (bitwise: %s)" % (case, solver, (np.abs(got - want) / ulp).max(), np.array_equal(got, want)))
    assert np.all(np.abs(got - want) <= ulp)
    assert torch.isfinite(r["grad0"]).all()                                                # (asked for: written at J = 0 too)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "prefix"])
@pytest.mark.parametrize("case,solver", CONFIGS)
def test_gradient_and_trace_against_the_fp64_loop(case, solver, masked):
    """grad0 within 5e-4 norm-wise per trajectory of fp64 autograd; trace[j], j = 0 .. 4, within (1 + 4 RHO) bar of the fp64 loop -- with
    and without the prefix mask (the second half of the window zeroed).

    Measured on an MI355X: grad0 errors 1.6e-7 .. 8.2e-7, the largest trace deviation per configuration 0.007 .. 0.042 bar, in all 24
    configurations.  The kernel's Adam arithmetic runs in fp64 on fp64 master copies of (loc, rho) for this test's sake: with fp32 Adam the
    iterates drifted from the fp64 loop's by 5e-7 per step (0.001f against 1 - 0.999f alone is a 7e-6 error of every step length), the
    trace deviations were 0.04 .. 0.39 bar, and cvs_ald / rk4 / prefix missed the bar with 2.13 bar at trace[3] of trajectory 0.  What made
    that entry sensitive remains: the ALD log-likelihood tau_side * (-log(2 s) - |y - mu| / s) is DISCONTINUOUS in mu at y = mu for
    tau != 0.5, and at the third iterate the q75 curve of draw 0 passes the observation (c = 1, t = 76) at 1.1e-6 in the fp64 loop -- a
    jump of (2 tau - 1) |log(2 s)| / K = 0.112 nat = 2.3 bar.  The kernel's iterates now stay within 4.3e-7 of the fp64 loop's at every
    step (the fp32 encoder's own error) and pass that point on the same side, at 4.9e-7."""
    c, w, ref, got = _run(case, solver, masked)
    _check_against_reference(got, ref, "%s/%s masked=%s" % (case, solver, masked))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "prefix"])
@pytest.mark.parametrize("case,solver", CONFIGS)
def test_returned_posterior_scores_what_the_call_says_and_improves(case, solver, masked):
    """The fp64 oracle objective at the returned (loc, scale) equals elbo within bar; elbo <= elbo0 and elbo < elbo0 - bar on EVERY
    trajectory (the reference improves by at least 2 % on all of them: tests/test_refine_cpu.py)."""
    c, w, ref, got = _run(case, solver, masked)
    F, mag = RU.objective_at(c, got["loc"], got["scale"], w=w)
    bar = RU.REL * mag
    err = np.abs(got["elbo"][:, 1] - F) / bar
    gain = (got["elbo"][:, 0] - got["elbo"][:, 1]) / (RU.REL * ref["mag"])
    print("%s/%s masked=%s: elbo against the oracle at the returned posterior %.3f bar; improvement %.0f .. %.0f bars"
          % (case, solver, masked, err.max(), gain.min(), gain.max()))
    assert err.max() <= 1.0
    assert np.all(got["elbo"][:, 1] <= got["elbo"][:, 0]) and np.all(gain > 1.0)


@pytest.mark.parametrize("case,t_major", [("cvs_ald", True), ("cvs_ald", False), ("challenge_gauss", True), ("challenge_gauss", False)])
def test_masks(case, t_major):
    """Both dense observation layouts.  An all-ones mask: bitwise what NULL gives.  Row 1 all zero: its grad0 is the KL terms' alone (fp64
    oracle, 5e-4) and after J = 4 its loc lies closer to the prior loc; the other rows: bitwise as without a mask."""
    from oracle import slode_oracle as O
    c = RU.build(case, "midpoint")
    eng = _engine(c)
    flat = eng.pack(c["p"])
    none = _refine(eng, flat, c, RU.J, t_major=t_major)
    ones = _refine(eng, flat, c, RU.J, w=torch.ones_like(c["obs"]), t_major=t_major)
    assert _same(none, ones) and torch.isfinite(none["trace"]).all()
    w = torch.ones_like(c["obs"])
    w[1] = 0.0
    got = _refine(eng, flat, c, RU.J, w=w, t_major=t_major)
    keep = [0, 2, 3, 4]
    assert all(torch.equal(got[k][..., keep] if k == "trace" else got[k][keep], none[k][..., keep] if k == "trace" else none[k][keep]) for k in NAMES)
    loc, rho = RU.encoder(c)
    with torch.no_grad():
        ploc, pscale = O.prior_loc_scale({k: v.double() for k, v in c["p"].items()}, c["ospec"], c["u"].double())
    e = c["eps"].double()[:, 1]
    gz = (loc[1] + rho[1].exp() * e - ploc[1]) / pscale[1] ** 2
    want = torch.cat([gz.mean(0), (gz * rho[1].exp() * e).mean(0) - 1.0]).numpy()
    g = _np(got)
    err = np.linalg.norm(g["grad0"][1] - want) / np.linalg.norm(want)
    print("%s t_major=%s: grad0 of the fully masked row against the KL terms %.2e" % (case, t_major, err))
    assert err <= RU.GRAD_REL
    assert np.linalg.norm(g["loc"][1] - ploc[1].numpy()) < np.linalg.norm(loc[1].numpy() - ploc[1].numpy())
    _check_against_reference(g, RU.refine(c, w=w), "%s row 1 masked" % case)


SIZES = [("cvs_ald", 9, 3, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}), ("challenge_ald", 5, 3, {"SLODE_ODE_GENERIC": "1"}),
         ("cvs_gauss", 5, 1, {}), ("cvs_gauss", 65, 2, {})]


@pytest.mark.parametrize("case,B,K,env", SIZES, ids=["%s-B%d-K%d%s" % (c, B, K, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, K, e in SIZES])
def test_grids_and_instantiations(case, B, K, env, monkeypatch):
    """B = 9 on 2 workgroups (the persistent loop), the run-time-S instantiation, K = 1, B = 65 (more than one wave of trajectories): rk4, J = 4,
    NaN-poisoned workspace, against the fp64 loop."""
    c = RU.build(case, "rk4", B=B, K=K)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    got = _np(_refine(eng, flat, c, RU.J))
    _check_against_reference(got, RU.refine(c), "%s B=%d K=%d %s" % (case, B, K, env))


def test_bitwise_reproducible_and_independent_of_the_grid_and_of_where_the_noise_is_drawn(monkeypatch):
    """Two calls: bitwise equal.  One workgroup per trajectory against a 3-workgroup loop: bitwise equal.  In-kernel noise of drawing calls
    n .. n + 2 against the rows rng_normal(n + k, B) passed explicitly: bitwise equal; the counter goes n -> n + K (not n + K J) and stays
    for explicit noise."""
    c = RU.build("cvs_ald", "midpoint", B=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    a, b, l = _refine(eng, flat, c, RU.J), _refine(eng, flat, c, RU.J), _refine(loop, flat, c, RU.J)
    assert _same(a, b) and _same(a, l) and torch.isfinite(a["trace"]).all()
    for e in (eng, loop):
        e.rng_seed(77, first_trajectory=1000)
        e.rng_set_counter(5)
    drawn = _refine(eng, flat, c, RU.J, eps=None)
    assert eng.rng_state() == (77, 1000, 5 + c["K"])
    rows = torch.stack([eng.rng_normal(5 + k, c["B"]) for k in range(c["K"])]).contiguous()
    given = _refine(eng, flat, c, RU.J, eps=rows)
    assert eng.rng_state() == (77, 1000, 5 + c["K"])                                       # explicit noise draws nothing
    drawn_loop = _refine(loop, flat, c, RU.J, eps=None)
    assert loop.rng_state() == (77, 1000, 5 + c["K"])
    assert _same(drawn, given) and _same(drawn, drawn_loop) and torch.isfinite(drawn["trace"]).all()
    assert not torch.equal(drawn["trace"], a["trace"])                                   # (other noise: another objective)


def test_launches():
    """Three launches, "weff", "enc_fwd2", "posterior_refine", whatever J."""
    c = RU.build("cvs_gauss", "rk4")
    eng = _engine(c)
    flat = eng.pack(c["p"])
    eng.profile_enable(True)
    _refine(eng, flat, c, RU.J)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "posterior_refine"]
    eng.profile_enable(False)


def test_refusals_by_name(monkeypatch):
    """The call's own rungs on the device (the whole ladder: tests/test_refine_cpu.py): named, nothing drawn, launched or written."""
    c = RU.build("cvs_ald", "rk4")
    obs_d, labels = _device_batch(c)
    B, L = c["B"], c["ospec"].latent_dim

    def refused(eng, match, J=2, lr=0.05, K=2):
        flat = eng.pack(c["p"])
        outs = [torch.full(s, float("nan"), device=DEV) for s in ((B, L), (B, L), (B, 2))]
        _refused(eng, lambda: eng.posterior_refine(flat, eng.make_batch(obs_d, labels, None), B, K, J, lr, loc=outs[0], scale=outs[1], elbo=outs[2]), match)
        torch.cuda.synchronize(DEV)
        assert all(torch.isnan(t).all() for t in outs)

    eng = _engine(c, monkeypatch)
    refused(eng, "num_steps = -1", J=-1)
    refused(eng, "lr = -0.05", lr=-0.05)
    refused(eng, "lr = nan", lr=float("nan"))
    refused(eng, "num_draws = 0", K=0)
    refused(_engine(c, monkeypatch, solver="dopri5"), "adaptive solver dopri5")
    refused(_engine(c, monkeypatch, {"SLODE_ODE_ALG": "1"}), "measured arms")
    refused(eng, "LDS tables", K=30000)


def test_model_level_calls_and_their_files(tmp_path):
    """refine_posterior: the dict, bitwise Engine.posterior_refine from the same generator state; save_refined_posterior: the three files
    of the batches in order; recon_samples(posterior=...) equals the manual decode of the same draws, and without the keyword is unchanged."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    B = batch["observations"].shape[0]
    eng.rng_seed(4321, first_trajectory=300)
    eng.rng_set_counter(9)
    res = m.refine_posterior(num_draws=3, num_steps=4, return_trace=True, **batch)
    assert eng.rng_state() == (4321, 300, 12)
    assert set(res) == {"loc", "scale", "elbo0", "elbo", "best_step", "grad0", "trace"} and tuple(res["trace"].shape) == (5, B)
    assert set(m.refine_posterior(num_draws=2, num_steps=1, **batch)) == {"loc", "scale", "elbo0", "elbo", "best_step"}
    assert torch.all(res["elbo"] <= res["elbo0"]) and torch.all(res["elbo"] < res["elbo0"]) and torch.isfinite(res["trace"]).all()
    eng.rng_set_counter(9)
    labs = [batch[l].reshape(B, -1).to(torch.float32).contiguous() for l in m.LABELS]
    loc, scale, elbo, _, trace, best = eng.posterior_refine(m._bind().flat, eng.make_batch(batch["observations"], labs, None, particles=3), B, 3, 4)
    assert torch.equal(loc, res["loc"]) and torch.equal(scale, res["scale"]) and torch.equal(elbo[:, 1], res["elbo"]) and torch.equal(trace, res["trace"])
    # a bool prefix mask: another objective, still an improvement
    mask = torch.ones_like(batch["observations"], dtype=torch.bool)
    mask[:, :, mask.shape[2] // 2:] = False
    eng.rng_set_counter(9)
    half = m.refine_posterior(num_draws=3, num_steps=4, mask=mask, **batch)
    assert torch.all(half["elbo"] < half["elbo0"]) and not torch.equal(half["elbo0"], res["elbo0"])
    eng.rng_set_counter(9)
    paths = m.save_refined_posterior(str(tmp_path / "res"), [batch, batch], 3, 4)
    assert [os.path.basename(p) for p in paths] == ["refined_loc.npy", "refined_scale.npy", "refined_elbo.npy"]
    tl, ts, te = (np.load(p) for p in paths)
    assert tl.shape == ts.shape == (2 * B, loc.shape[1]) and te.shape == (2 * B, 2) and te.dtype == np.float32
    assert np.array_equal(tl[:B], loc.cpu().numpy()) and np.array_equal(te[:B], elbo.cpu().numpy()) and np.isfinite(te).all()
    # decode the refined posterior: the draws z = loc + scale eps of the given posterior, through the same decode as recon_samples' own
    eps = torch.randn(4, B, loc.shape[1], generator=torch.Generator().manual_seed(2)).to(DEV)
    got = m.recon_samples(batch["observations"], True, 4, eps=eps, posterior=(res["loc"], res["scale"]), **{l: batch[l] for l in m.LABELS})
    z = res["loc"].unsqueeze(0) + res["scale"].unsqueeze(0) * eps
    assert torch.allclose(got["z"], z, rtol=0, atol=1e-6)
    want = m._decoded_draws(got["z"])
    assert all(torch.equal(got[k], want[k]) for k in want)
    plain = m.recon_samples(batch["observations"], True, 4, eps=eps, **{l: batch[l] for l in m.LABELS})
    enc = m.recon_samples(batch["observations"], True, 4, eps=eps, posterior=m._loc_scale(batch["observations"], True, {}), **{l: batch[l] for l in m.LABELS})
    assert all(torch.equal(plain[k], enc[k]) for k in plain) and not torch.equal(plain["z"], got["z"])


def test_model_level_refusals():
    """A proc model (its main loss scores the labels) and a dopri5 model are each refused by name."""
    from structured_latent_odes_amd import _lib as L
    m, batch = _model("proc")
    with pytest.raises(L.SlodeError, match="scores the labels"):
        m.refine_posterior(num_draws=2, num_steps=2, **batch)
    m, batch = _model("cvs", solver="dopri5")
    with pytest.raises(L.SlodeError, match="adaptive solver dopri5"):
        m.refine_posterior(num_draws=2, num_steps=2, **batch)


def test_training_entry_point_with_refine_steps(tmp_path, monkeypatch, capsys):
    """One --refine-steps 3 run of training.main on a synthetic loader, one epoch: the three files and the printed line."""
    from structured_latent_odes_amd import training as T
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.models.mechanistic_cvs_Gauss import MechanisticModelGauss
    from tests import eval_stats_util as EU

    def load_config():
        cfg = EU.model_config("cvs")
        cfg.update(mini_batch_size=16, seq_len=86)
        return cfg

    monkeypatch.chdir(tmp_path)
    T.main("cvs", load_config, MechanisticModel, MechanisticModelGauss, ["--epochs", "1", "--batches-per-epoch", "1", "--refine-steps", "3",
                                                                          "--refine-draws", "2"])
    out = capsys.readouterr().out
    assert "refine_posterior: J=3 K=2  n=16" in out
    table = np.load(str(tmp_path / ("results_%s" % load_config().model) / "refined_elbo.npy"))
    assert table.shape == (16, 2) and np.isfinite(table).all() and np.all(table[:, 1] <= table[:, 0])
