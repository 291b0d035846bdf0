"""GPU tests of the pointwise predictive density (slode_pointwise_density / Engine.pointwise_density / MechanisticBase.pointwise_density /
save_pointwise_density / --waic) against the fp64 oracle of the point terms folded in fp64, against the existing calls it is tied to
(traj_bounds, posterior_refine) and against itself (mask, grids, noise sources).  Bars and the ALD exclusion: module docstring of
tests/pointwise_util.py; tests/test_pointwise_cpu.py shows that every condition asked here holds for the reference alone.  Outputs are
pre-filled with NaN: every element must be written."""
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import pointwise_util as PU
from tests import traj_bounds_util as TU
from tests import refine_util as RU
from tests.eval_gpu_util import ADAPTIVE, _captured, _device_batch, _engine, _lay, _model, _padded, _refused

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POST, IMP = 0, 1


def _like_obs(c, t):
    """A host [B, C, T] tensor on the device in the layout (the strides) of the case's observations (``_device_batch``)."""
    return _lay(t, c["fam"] != "proc")


def _pw(eng, flat, c, weights, eps="case", K=None, obs_d=None, labels=None, mask=None, loc=None, scale=None, particles=1):
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    K = c["K"] if K is None else K
    e = c["eps"] if isinstance(eps, str) else eps
    if e is not None:
        e = (e[0] if K == 1 and e.dim() == 3 else e).to(DEV).contiguous()               # one draw: [B, L], as make_batch takes it
    B, Cn, T = c["obs"].shape
    point = torch.full((3, B, Cn, T), float("nan"), device=DEV)
    summary = torch.full((B, 8), float("nan"), device=DEV)
    loss = torch.full((max(K, 0), B), float("nan"), device=DEV) if weights == IMP else None
    eng.pointwise_density(flat, eng.make_batch(obs_d, labels, e, particles=max(K, 1)), B, K, weights, mask=mask, loc=loc, scale=scale, point=point,
                          summary=summary, loss_kb=loss, particles=particles)
    return point, summary, loss


def _check_both_modes(eng, flat, c, tag, want=None):
    """Both weightings against the oracle's point terms: posterior with lw = -log K; importance with the weights of the call's OWN loss_kb
    (the losses themselves: against the row oracle of traj_bounds, at its bar).  Returns the two results."""
    want = PU.oracle_points(c) if want is None else want
    K, B = c["eps"].shape[:2]
    post = _pw(eng, flat, c, POST)
    PU.check(post[0], post[1], want, PU.log_weights(K, B), tag + " posterior")
    assert torch.equal(post[1][:, 7], torch.full((B,), float(K), device=DEV))
    imp = _pw(eng, flat, c, IMP)
    loss = imp[2].double().cpu().numpy()
    rows = TU.oracle_rows(c)
    rl = np.abs(loss - rows["loss"]) / (TU.REL * rows["mag"])
    print("%s importance: loss_kb error / bar %.3f" % (tag, rl.max()))
    assert rl.max() <= 1.0
    PU.check(imp[0], imp[1], want, PU.log_weights(K, B, loss), tag + " importance")
    ess = TU.reduce64(loss)[2]
    assert np.all(np.abs(imp[1][:, 7].double().cpu().numpy() - ess) <= 1e-5 * K)
    return post, imp


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_planes_and_slots_match_the_fp64_oracle(case, solver):
    """Explicit noise, K = 4; six model classes x three fixed-grid solvers, both weightings; cvs / challenge in the [B,T,C] layout, proc in
    [B,C,T]."""
    c = PU.config((case, solver, None, 4, 1.0))
    eng = _engine(c)
    _check_both_modes(eng, eng.pack(c["p"]), c, "%s/%s" % (case, solver))


@pytest.mark.parametrize("case,B,K,env", PU.SIZES, ids=["%s-B%d-K%d%s" % (c, B, K, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, K, e in PU.SIZES])
def test_sizes_and_instantiations(case, B, K, env, monkeypatch):
    """test_gpu_traj_bounds.py::SIZES: B on both sides of the 64- and 256-thread edges, the persistent loop, the run-time-S instantiation
    with and without the label phase, K in {1, 2, 7, 64, 200}, T = 300 (two rounds of the 256 threads), rk4, NaN-poisoned workspace.
    K = 1: lppd == mean_ll bitwise, var_ll == 0, the ESS exactly 1 in both modes."""
    assert PU.SIZES == __import__("tests.test_gpu_traj_bounds", fromlist=["SIZES"]).SIZES
    c = PU.config((case, "rk4", B, K, 1.0))
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    post, imp = _check_both_modes(eng, flat, c, "%s B=%d K=%d %s" % (case, B, K, env))
    if K == 1:
        for point, summary, _ in (post, imp):
            assert torch.equal(point[0], point[1]) and torch.equal(point[2], torch.zeros_like(point[2]))
            assert torch.equal(summary[:, 7], torch.ones(B, device=DEV)) and torch.equal(summary[:, 0], summary[:, 2])
        assert torch.equal(post[0], imp[0])                                              # lw_0 = 0 exactly in both modes


@pytest.mark.parametrize("cfg", PU.SPREAD, ids=[c[0] for c in PU.SPREAD])
def test_importance_fold_on_non_degenerate_weights(cfg):
    """Noise x 1e-3, K = 8 (tests/test_pointwise_cpu.py: 1.5 < ESS < 7.5 on at least 3 trajectories of the oracle): the importance fold with
    weights that neither collapse onto one draw nor are uniform."""
    c = PU.config(cfg)
    eng = _engine(c)
    _, imp = _check_both_modes(eng, eng.pack(c["p"]), c, "%s noise x 1e-3" % cfg[0])
    ess = imp[1][:, 7].cpu().numpy()
    assert np.sum((ess > 1.5) & (ess < 7.5)) >= 3, ess


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald", "challenge_gauss"])
def test_ties_to_traj_bounds(case):
    """Importance mode, NULL mask: loss_kb bitwise traj_bounds' loss_kb and slot 7 bitwise its ESS (sweep 1 IS its draw loop).  Posterior
    mode: slot 2, the sum of mean_ll, against -(slot 3 of the bounds), the mean NLL, within the mean over k of the row bar."""
    c = PU.config((case, "rk4", None, 4, 1.0))
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    bounds = torch.full((c["B"], 4), float("nan"), device=DEV)
    loss = torch.full((4, c["B"]), float("nan"), device=DEV)
    eng.traj_bounds(flat, eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=4), c["B"], 4, bounds, loss)
    imp = _pw(eng, flat, c, IMP, obs_d=obs_d, labels=labels)
    assert torch.equal(imp[2], loss) and torch.equal(imp[1][:, 7], bounds[:, 2])
    post = _pw(eng, flat, c, POST, obs_d=obs_d, labels=labels)
    bar = (TU.REL * TU.oracle_rows(c)["mag"]).mean(0)
    err = (post[1][:, 2].double() + bounds[:, 3].double()).abs().cpu().numpy()
    print("%s: sum of mean_ll against -mean NLL: error / bar %.3f" % (case, (err / bar).max()))
    assert np.all(err <= bar)


@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_mask(case):
    """An all-ones mask is bitwise the NULL mask, everything, in both modes.  A prefix mask, in both dense layouts: the planes of the
    posterior mode bitwise those of the unmasked call, only the slots repartitioned, n_in + n_out = C T; in importance mode loss_kb follows
    the masked loss of the oracle and the planes the weights of that loss."""
    c = PU.config((case, "rk4", None, 4, 1.0))
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    B, Cn, T = c["obs"].shape
    ones = _like_obs(c, torch.ones(B, Cn, T))
    for w in (POST, IMP):
        a, b = _pw(eng, flat, c, w, obs_d=obs_d, labels=labels), _pw(eng, flat, c, w, obs_d=obs_d, labels=labels, mask=ones)
        assert all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)
    mask = PU.prefix_mask(c)
    mask[1] = 0.0                                                                        # one trajectory with no observed point at all
    mask_d = _like_obs(c, mask)
    assert mask_d.stride() == obs_d.stride()
    want = PU.oracle_points(c)
    plain = _pw(eng, flat, c, POST, obs_d=obs_d, labels=labels)
    post = _pw(eng, flat, c, POST, obs_d=obs_d, labels=labels, mask=mask_d)
    assert torch.equal(post[0], plain[0]) and not torch.equal(post[1], plain[1])
    assert torch.equal(post[1][:, 3] + post[1][:, 6], torch.full((B,), float(Cn * T), device=DEV))
    assert post[1][1, 3].item() == 0.0 and post[1][1, 0].item() == 0.0 and post[1][0, 3].item() == Cn * (T // 2 + 3)
    PU.check(post[0], post[1], want, PU.log_weights(4, B), case + " prefix mask, posterior", mask=mask.numpy())
    imp = _pw(eng, flat, c, IMP, obs_d=obs_d, labels=labels, mask=mask_d)
    rows = TU.oracle_rows(c)
    loss = imp[2].double().cpu().numpy()
    rl = np.abs(loss - PU.masked_loss(rows, want, mask.numpy())) / (TU.REL * rows["mag"])
    print("%s prefix mask: masked loss_kb error / bar %.3f" % (case, rl.max()))
    assert rl.max() <= 1.0 and not torch.equal(imp[2], _pw(eng, flat, c, IMP, obs_d=obs_d, labels=labels)[2])
    PU.check(imp[0], imp[1], want, PU.log_weights(4, B, loss), case + " prefix mask, importance", mask=mask.numpy())


@pytest.mark.parametrize("t_major", [True, False], ids=["BTC", "BCT"])
@pytest.mark.parametrize("case", ["cvs_ald", "challenge_gauss"])
def test_masked_tie_to_posterior_refine(case, t_major):
    """A prefix mask, explicit noise, B = 5, K = 3 (the sizes of tests/refine_util.py), both dense layouts: the -ELBO of posterior_refine at
    J = 0 is bitwise the mean of the importance sweep's masked loss_kb -- both kernels execute one weighted log-likelihood routine
    (tb_loglik_weighted) inside one draw frame.  An fp64 sum of three fp32 values is exact, so the order of the sum does not enter."""
    c = RU.build(case)
    B, K = c["B"], c["K"]
    eng = _engine(c)
    flat = eng.pack(c["p"])
    w = _lay(RU.prefix_mask(c), t_major)
    bt = eng.make_batch(_lay(c["obs"], t_major), _device_batch(c)[1], c["eps"].to(DEV).contiguous(), particles=K)
    elbo = eng.posterior_refine(flat, bt, B, K, 0, mask=w, grad0=False, trace=False, best_step=False)[2]
    loss = eng.pointwise_density(flat, bt, B, K, IMP, mask=w)[2]
    want = (loss.double().sum(0) / K).float()
    print("%s %s: largest |elbo0 - mean masked loss_kb| = %.3e" % (case, "BTC" if t_major else "BCT", (elbo[:, 0] - want).abs().max().item()))
    assert torch.isfinite(want).all() and torch.equal(elbo[:, 0], want)


def test_posterior_input():
    """loc / scale = the encoder's own (read back from a J = 0 posterior_refine) is bitwise the default call; a refined posterior (J = 3)
    against the oracle fed the same (loc, scale), both modes (cvs_gauss: no jump, no exclusion that would depend on the posterior)."""
    c = PU.config(("cvs_gauss", "rk4", None, 4, 1.0))
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    B = c["B"]
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=4)
    loc0, scale0 = eng.posterior_refine(flat, bt, B, 4, 0, grad0=False, trace=False, best_step=False)[:2]
    for w in (POST, IMP):
        a, b = _pw(eng, flat, c, w, obs_d=obs_d, labels=labels), _pw(eng, flat, c, w, obs_d=obs_d, labels=labels, loc=loc0, scale=scale0)
        assert all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)
    loc, scale = eng.posterior_refine(flat, bt, B, 4, 3, grad0=False, trace=False, best_step=False)[:2]
    assert not torch.equal(loc, loc0)
    want = PU.oracle_points(c, posterior=(loc.cpu(), scale.cpu()))
    post = _pw(eng, flat, c, POST, obs_d=obs_d, labels=labels, loc=loc, scale=scale)
    PU.check(post[0], post[1], want, PU.log_weights(4, B), "refined posterior, posterior weights")
    imp = _pw(eng, flat, c, IMP, obs_d=obs_d, labels=labels, loc=loc, scale=scale)
    PU.check(imp[0], imp[1], want, PU.log_weights(4, B, imp[2].double().cpu().numpy()), "refined posterior, importance weights")
    assert not torch.equal(post[0], _pw(eng, flat, c, POST, obs_d=obs_d, labels=labels)[0])


@pytest.mark.parametrize("weights", [POST, IMP], ids=["posterior", "importance"])
@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_bitwise_reproducible_and_independent_of_the_grid_and_of_where_the_noise_is_drawn(case, weights, monkeypatch):
    """Two calls: bitwise equal.  One workgroup per trajectory against a 3-workgroup loop: bitwise equal.  In-kernel noise of drawing calls
    n .. n + 6 against the rows rng_normal(n + k, B) passed explicitly: bitwise equal; the counter goes n -> n + 7 in both modes (the
    second sweep of the importance mode redraws, it does not draw) and stays for explicit noise."""
    c = PU.build(case, "midpoint", K=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    mask = _like_obs(c, PU.prefix_mask(c))
    a, b, l = (_pw(e, flat, c, weights, mask=mask) for e in (eng, eng, loop))
    for x, y, z in zip(a, b, l):
        assert x is None or (torch.equal(x, y) and torch.equal(x, z))
    for e in (eng, loop):
        e.rng_seed(77, first_trajectory=1000)
        e.rng_set_counter(5)
    drawn = _pw(eng, flat, c, weights, eps=None, mask=mask)
    assert eng.rng_state() == (77, 1000, 12)
    rows = torch.stack([eng.rng_normal(5 + k, c["B"]) for k in range(7)]).contiguous()
    given = _pw(eng, flat, c, weights, eps=rows, mask=mask)
    assert eng.rng_state() == (77, 1000, 12)                                             # explicit noise draws nothing
    drawn_loop = _pw(loop, flat, c, weights, eps=None, mask=mask)
    assert loop.rng_state() == (77, 1000, 12)
    for x, y, z in zip(drawn, given, drawn_loop):
        assert x is None or (torch.isfinite(x).all() and torch.equal(x, y) and torch.equal(x, z))


def test_refusals_by_name(monkeypatch):
    """Every refusal names its reason, draws nothing, launches nothing and writes nothing (rng_state, profile_read, outputs still NaN)."""
    from structured_latent_odes_amd import _lib as L
    c = PU.build("cvs_ald", "rk4", K=2)
    obs_d, labels = _device_batch(c)
    B, Cn, T = c["obs"].shape
    Ld = c["eps"].shape[2]

    def refused(eng, match, obs=obs_d, K=2, particles=1, weights=IMP, raw=None, **kw):
        flat = eng.pack(c["p"])
        point = torch.full((3, B, Cn, T), float("nan"), device=DEV)
        summary = torch.full((B, 8), float("nan"), device=DEV)
        loss = torch.full((K, B), float("nan"), device=DEV)
        bt = eng.make_batch(obs, labels, None)
        if raw is None:
            call = lambda: eng.pointwise_density(flat, bt, B, K, weights, point=point, summary=summary, loss_kb=loss if weights == IMP else False,
                                                 particles=particles, **kw)
        else:                                                                            # what Engine.pointwise_density cannot express
            call = lambda: eng._batch_call(eng.lib.slode_pointwise_density, flat, bt, B, 1, K, weights, *(eng._p(t) for t in raw(point, summary, loss)))
        _refused(eng, call, match)
        torch.cuda.synchronize(DEV)
        assert torch.isnan(point).all() and torch.isnan(summary).all() and torch.isnan(loss).all()

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s" % solver)
    eng = _engine(c, monkeypatch)
    refused(eng, "particles = 2", particles=2)
    refused(eng, "num_draws = 0", K=0)
    refused(eng, "num_draws = 0", K=0, weights=POST)
    refused(eng, "observation strides", obs=_padded(obs_d))
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    eng = _engine(c, monkeypatch)
    refused(eng, "weights = 2", weights=2)
    some = torch.zeros(B, Ld, device=DEV)
    refused(eng, "scale is NULL", raw=lambda p, s, l: (None, some, None, p, s, l))
    refused(eng, "loc is NULL", raw=lambda p, s, l: (None, None, some, p, s, l))
    refused(eng, "point / summary is NULL", raw=lambda p, s, l: (None, None, None, None, s, l))
    refused(eng, "16-byte aligned", raw=lambda p, s, l: (None, None, None, p, s.view(-1)[1:], l))
    refused(eng, "importance mode alone", weights=POST, raw=lambda p, s, l: (None, None, None, p, s, l))
    refused(eng, "LDS tables.*num_draws = 30000", K=30000)                              # 5 x 30,000 floats of per-draw values: 600 KB
    with pytest.raises(L.SlodeError, match="num_draws = 30000"):
        eng.pointwise_plan(B, 30000, IMP)
    assert eng.pointwise_plan(B, 30000, POST) == eng.pointwise_plan(B, 1, POST) < 64 * 1024


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_call_and_its_files(fam, tmp_path):
    """pointwise_density(num_draws=4): the dict's shapes, elpd_waic = lppd - p_waic, bitwise Engine.pointwise_density from the same
    generator state; "fit on a prefix, score the suffix" through refine_posterior (cvs, challenge); save_pointwise_density over two
    batches."""
    m, batch = _model(fam)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    eng.rng_seed(4321, first_trajectory=300)
    eng.rng_set_counter(9)
    res = m.pointwise_density(num_draws=4, **batch)
    assert eng.rng_state() == (4321, 300, 13)
    assert set(res) == {"lppd", "mean_ll", "p_waic", "elpd_waic"} | set(m.POINTWISE_NAMES)
    assert all(tuple(res[n].shape) == (B, Cn, T) for n in ("lppd", "mean_ll", "p_waic", "elpd_waic")) and all(tuple(res[n].shape) == (B,) for n in m.POINTWISE_NAMES)
    assert torch.equal(res["elpd_waic"], res["lppd"] - res["p_waic"]) and all(torch.isfinite(v).all() for v in res.values())
    assert torch.all(res["lppd"] >= res["mean_ll"] - 2.0 ** -21 * (1.0 + res["mean_ll"].abs())) and torch.all(res["p_waic"] >= 0)
    eng.rng_set_counter(9)
    labs = [batch[l].reshape(B, -1).to(torch.float32).contiguous() for l in m.LABELS]
    point, summary, _ = eng.pointwise_density(m._bind().flat, eng.make_batch(batch["observations"], labs, None, particles=4), B, 4, POST)
    assert torch.equal(point[0], res["lppd"]) and torch.equal(point[2], res["p_waic"]) and torch.equal(summary[:, 0], res["lppd_in"])
    PU.check_own_sums(point, summary, fam + " model")
    imp = m.pointwise_density(num_draws=4, weights="importance", return_draws=True, **batch)
    assert tuple(imp["loss"].shape) == (4, B) and torch.all(imp["ess"] >= 1.0) and torch.all(imp["ess"] <= 4.0)
    if fam != "proc":                                                                    # (posterior_refine refuses the proc family)
        mask = torch.zeros(B, Cn, T, dtype=torch.bool, device=DEV)
        mask[:, :, :T // 2] = True
        eps = torch.randn(4, B, eng.spec.latent_dim, generator=torch.Generator().manual_seed(2)).to(DEV)
        fit = m.refine_posterior(num_draws=4, num_steps=3, mask=mask, eps=eps, **batch)
        held = m.pointwise_density(num_draws=4, mask=mask, posterior=(fit["loc"], fit["scale"]), eps=eps, **batch)
        assert torch.equal(held["n_out"], torch.full((B,), float(Cn * (T - T // 2)), device=DEV)) and torch.isfinite(held["lppd_out"]).all()
        assert torch.allclose(held["lppd_in"] + held["lppd_out"], held["lppd"].double().sum((1, 2)).float(), rtol=1e-5)
    eng.rng_set_counter(9)
    files = m.save_pointwise_density(str(tmp_path / "res"), [batch, batch], 4)
    assert [os.path.basename(f) for f in files] == ["pointwise_lppd_post.npy", "pointwise_p_waic_post.npy", "pointwise_mean_ll_post.npy", "waic_post.npy"]
    arrays = [np.load(f) for f in files]
    assert [a.shape for a in arrays] == [(2 * B, Cn, T)] * 3 + [(2 * B, 8)] and all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays)
    assert np.array_equal(arrays[0][:B], res["lppd"].cpu().numpy()) and np.array_equal(arrays[3][:B], summary.cpu().numpy())


def test_adaptive_solver_takes_the_composed_route():
    """dopri5: the engine refuses, the dict is composed from recon_samples; it agrees with the fused call of the rk4 model on the same inputs
    in shape and finiteness (another solver: other curves), and satisfies the identities of the quantity itself."""
    m, batch = _model("cvs", solver="dopri5")
    fused, _ = _model("cvs")
    B = batch["observations"].shape[0]
    eps = torch.randn(3, B, m._bind().engine.spec.latent_dim, generator=torch.Generator().manual_seed(2)).to(DEV)
    mask = torch.ones_like(batch["observations"])
    mask[:, :, 40:] = 0.0
    for weights in ("posterior", "importance"):
        got = m.pointwise_density(num_draws=3, weights=weights, mask=mask, eps=eps, return_draws=weights == "importance", **batch)
        want = fused.pointwise_density(num_draws=3, weights=weights, mask=mask, eps=eps, return_draws=weights == "importance", **batch)
        assert set(got) == set(want)
        for n in got:
            assert got[n].shape == want[n].shape and got[n].dtype == want[n].dtype and torch.isfinite(got[n]).all(), n
        assert torch.equal(got["n_in"], want["n_in"]) and torch.equal(got["n_out"], want["n_out"])
        assert torch.all(got["lppd"] >= got["mean_ll"] - 1e-5 * got["mean_ll"].abs()) and torch.all(got["p_waic"] >= 0)


def test_training_entry_point_with_waic(tmp_path, monkeypatch, capsys):
    """One --waic 4 run of training.main on a synthetic loader, one epoch: the four files beside the run's other files and the line."""
    from structured_latent_odes_amd import training as T
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.models.mechanistic_cvs_Gauss import MechanisticModelGauss

    def load_config():
        cfg = EU.model_config("cvs")
        cfg.update(mini_batch_size=16, seq_len=86)
        return cfg

    monkeypatch.chdir(tmp_path)
    T.main("cvs", load_config, MechanisticModel, MechanisticModelGauss, ["--epochs", "1", "--batches-per-epoch", "1", "--waic", "4"])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("waic: ")]
    assert "FINAL TEST:" in out and len(line) == 1 and line[0].startswith("waic: K=4  n=16  elpd_waic=") and "share(p_waic>0.4)=" in line[0]
    res = tmp_path / ("results_%s" % load_config().model)
    table, p = np.load(str(res / "waic_post.npy")), np.load(str(res / "pointwise_p_waic_post.npy"))
    assert table.shape == (16, 8) and p.shape == (16, 3, 86) and np.isfinite(table).all() and np.all(table[:, 7] == 4.0)
    assert line[0] == MechanisticModel.waic_line(table, p, 4)


def test_launches_and_graph_capture():
    """Three launches, "weff", "enc_fwd2", "pointwise_density", on one stream, in both modes and with a given posterior.  One capture and
    one replay of a call with explicit noise equal the stream-launched call bitwise."""
    c = PU.build("cvs_ald", "rk4", K=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    B, Cn, T = c["obs"].shape
    some = torch.ones(B, c["eps"].shape[2], device=DEV)
    for w, kw in ((POST, {}), (IMP, {}), (POST, dict(loc=some, scale=some))):
        eng.profile_enable(True)
        _pw(eng, flat, c, w, obs_d=obs_d, labels=labels, **kw)
        assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "pointwise_density"]
        eng.profile_enable(False)
    point, summary, loss = torch.zeros(3, B, Cn, T, device=DEV), torch.zeros(B, 8, device=DEV), torch.zeros(7, B, device=DEV)
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    want = _captured(lambda: eng.pointwise_density(flat, bt, B, 7, IMP, point=point, summary=summary, loss_kb=loss), (point, summary, loss))
    assert all(torch.equal(x, y) for x, y in zip((point, summary, loss), want)) and want[0].abs().sum().item() > 0.0
