"""The reference's eval-side API on the six model classes (cvs, proc, challenge; ALD and Gauss): recon, classifier / pred_inputs,
recon_samples (`multiple_samples`) at num_samples = 200 and the configured mini_batch_size, Decoder.forward / GaussianDecoder.forward
as autograd modules, and guide() as a differentiable function of the encoder -- each against the fp64 oracle.  The noise is made
known by seeding the engine's generator and reading the drawing call back with rng_normal(n, B)."""
import dataclasses
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import slode_oracle as O
from tests import eval_side_util as V
from tests.eval_side_util import DP5_TOL, _heads64, _p64

pytestmark = pytest.mark.gpu

CLASSES = [(f, g) for f in ("cvs", "proc", "challenge") for g in (False, True)]


def _model(fam, gauss, solver="rk4", adjoint=True, B=None, seed=3):
    """As tests/test_gpu_models.py::_cvs, for every family: config defaults, label heads moved off their 1e-3 initialisation."""
    import importlib
    from structured_latent_odes_amd import configs
    from structured_latent_odes_amd.synthetic import synthetic_batch
    dev = torch.device("cuda:0")
    cfg = getattr(configs, "load_config_" + fam)()
    cfg.update(solver=solver, adjoint_solver=adjoint)
    T = cfg.seq_len
    B = B or cfg.mini_batch_size
    obs, labels, times = synthetic_batch(fam, B, T, cfg.obs_dim, seed=7)
    torch.manual_seed(seed)
    mod = importlib.import_module("structured_latent_odes_amd.models.mechanistic_%s%s" % (fam, "_Gauss" if gauss else ""))
    m = (mod.MechanisticModelGauss if gauss else mod.MechanisticModel)(cfg, dev, times.to(dev))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.startswith("q_"):
                p.add_(0.3 * torch.randn_like(p))
    batch = {"observations": obs.to(dev), **{k: v.to(dev) for k, v in labels.items()}}
    ospec = {"cvs": O.cvs_spec, "proc": O.proc_spec, "challenge": O.challenge_spec}[fam](gauss=gauss, solver=solver)
    ospec = dataclasses.replace(ospec, grad_mode=m.model_spec().grad_mode)
    u = torch.cat([labels[l].reshape(B, -1) for l in m.LABELS], 1).double()
    return m, cfg, batch, ospec, u, times, dev


def _decode64(p, ospec, z, times, solver):
    """(solution, {name: curve}, std) of the oracle's decoder for z, fp64; dopri5 at the engine's default tolerances."""
    kw = DP5_TOL if solver == "dopri5" else {}
    if ospec.gauss:
        sol, mean, std = O.decoder_gauss(p, z, times.double(), solver, **kw)
        return sol, {"mean": mean}, std
    sol, mu75, mu50, mu25, std = O.decoder_ald(p, z, times.double(), solver, **kw)
    return sol, {"mu_75": mu75, "mu_50": mu50, "mu_25": mu25}, std


@pytest.mark.parametrize("solver", ["rk4", "dopri5"])
@pytest.mark.parametrize("fam,gauss", CLASSES)
def test_recon_every_family(fam, gauss, solver):
    """recon(is_post=True / False): z against loc + scale * eps of the oracle's encoder / prior_loc_scale (N(0, 1) dims included) for the
    read-back eps (2e-5 norm-wise: the z bar of test_elbo_loss_and_trajectories); solution_xt, every curve and std against the oracle's
    decoder for that z at the bars of test_recon_classifier_and_state_dict_roundtrip (trajectories 1e-5 * max(1, |x|), curves 1e-5, std
    1e-6 norm-wise); l1 1e-5 relative; the counter moves by exactly one per call.  B = 24, as in that test.  dopri5 (default tolerances):
    the trajectories against the fp64 solve at rtol 1e-10 at test_forward_solution_level's bar (err < 3 * err_ref + 1e-5, err_ref that
    of the fp64 restatement at the engine's tolerances; and < 1e-3), the curves and l1 against fp64 heads applied to the returned
    trajectories (1e-6 per row, test_decode_heads' bar)."""
    m, cfg, batch, ospec, u, times, dev = _model(fam, gauss, solver, B=24)
    eng = m._bind().engine
    p = _p64(m)
    obs64 = batch["observations"].cpu().double()
    B = obs64.shape[0]
    eng.rng_seed(1234)
    for is_post in (True, False):
        n = eng.rng_state()[2]
        r = m.recon(is_post=is_post, **batch)
        assert eng.rng_state()[2] == n + 1
        eps = eng.rng_normal(n, B).cpu().double()
        loc, scale = O.encoder_conv(p, obs64, ospec.pool_size) if is_post else O.prior_loc_scale(p, ospec, u)
        if not is_post:
            assert bool((loc[:, -ospec.z_eps_dim:] == 0).all()) and bool((scale[:, -ospec.z_eps_dim:] == 1).all())
        assert V.rel(r["z"], loc + scale * eps) < 2e-5, (is_post, V.rel(r["z"], loc + scale * eps))
        z = r["z"].cpu().double()
        names = ["mean"] if gauss else ["mu_75", "mu_50", "mu_25"]
        centre = "mean" if gauss else "mu_50"
        if solver == "dopri5":
            tight = O.solve_ode(p, z, times.double(), "dopri5", rtol=1e-10, atol=1e-12, per_trajectory=True)
            ref = O.solve_ode(p, z, times.double(), "dopri5", **DP5_TOL)
            err_gpu, err_ref = V.elem_err(r["solution_xt"], tight), V.elem_err(ref, tight)
            print("%s gauss=%s post=%s dopri5: solution error %.2e (fp64 restatement %.2e)" % (fam, gauss, is_post, err_gpu, err_ref))
            assert err_gpu < 3.0 * err_ref + 1e-5 and err_gpu < 1e-3, (err_gpu, err_ref)
            mus = _heads64(p, ospec, r["solution_xt"].cpu().double())
            std = torch.ones_like(mus[centre]) * F.softplus(p["decoder.constant_std"])
            for k in names:
                assert V.row_err(r[k], mus[k]) < 1e-6, k
        else:
            sol, mus, std = _decode64(p, ospec, z, times, solver)
            assert V.elem_err(r["solution_xt"], sol) < 1e-5, V.elem_err(r["solution_xt"], sol)
            for k in names:
                assert V.rel(r[k], mus[k]) < 1e-5, (k, V.rel(r[k], mus[k]))
        assert tuple(r["std"].shape) == tuple(mus[centre].shape) and V.rel(r["std"], std) < 1e-6
        l1 = (mus[centre] - obs64).abs().mean().item()
        assert abs(float(r["l1"]) - l1) < 1e-5 * l1, (float(r["l1"]), l1)


@pytest.mark.parametrize("fam,gauss", CLASSES)
def test_classifier_and_pred_inputs_decisions(fam, gauss):
    """classifier (cvs) / pred_inputs (proc, challenge): the hard decisions equal the fp64 oracle's for the z the call drew (the drawing
    call replayed on the same loc / scale): sigmoid heads p > 0.5, softmax heads arg-max (lowest index on a tie), Exp-Exp heads the value
    at 2e-6 per row (the bar of test_eval_side_small_nets).  Rows whose fp64 probability is within 1e-4 of 0.5, or whose two largest
    softmax probabilities are within 1e-4, are left out: at most 1 % of the rows of a head, asserted (the label heads sit 0.3 off their
    initialisation, so the logits spread over O(1) and a 1e-4 band around a decision boundary holds about one row in 10^4)."""
    m, cfg, batch, ospec, u, times, dev = _model(fam, gauss)
    eng = m._bind().engine
    p = _p64(m)
    obs = batch["observations"]
    B = obs.shape[0]
    eng.rng_seed(77)
    n = eng.rng_state()[2]
    pred = (m.classifier if fam == "cvs" else m.pred_inputs)(observations=obs)
    assert eng.rng_state()[2] == n + 1
    with torch.no_grad():
        loc, scale = m.encoder.forward(obs)
    eng.rng_set_counter(n)
    z = eng.sample_normal(loc.contiguous(), scale.contiguous()).cpu().double()
    assert V.rel(z, loc.cpu().double() + scale.cpu().double() * eng.rng_normal(n, B).cpu().double()) < 1e-6
    assert set(pred) == set(m.LABELS)
    for (kind, prefix, zo, zd, uo, ud), (attr, group, label, mkind) in zip(ospec.aux_heads, m.AUX):
        zg = z[:, zo:zo + zd]
        got = pred[label].cpu().double()
        assert tuple(got.shape) == (B, ud)
        if kind == "bernoulli":
            pr = O.classifier_sigmoid(p, prefix, zg)
            keep = ((pr - 0.5).abs() >= 1e-4).all(dim=1)
            want = (pr > 0.5).double()
        elif kind == "onehot":
            pr = O.classifier_softmax(p, prefix, zg)
            top = pr.topk(2, dim=1).values
            keep = (top[:, 0] - top[:, 1]) >= 1e-4
            want = torch.zeros_like(pr).scatter_(1, pr.argmax(1, keepdim=True), 1.0)
        else:
            want = O.regressor_exp_exp(p, prefix, zg)[0]
            assert V.row_err(got, want) < 2e-6, (label, V.row_err(got, want))
            continue
        assert int((~keep).sum()) <= 0.01 * B, (label, int((~keep).sum()))
        assert torch.equal(got[keep], want[keep]), label
        assert set(got.unique().tolist()) <= {0.0, 1.0}


def _sample_rows(ns, B):
    rows = V.oracle_rows(ns * B)
    return [(r // B, r % B) for r in rows]


@pytest.mark.parametrize("solver", ["rk4", "dopri5"])
@pytest.mark.parametrize("fam,gauss", CLASSES)
def test_recon_samples_at_200_samples(fam, gauss, solver, tmp_path):
    """recon_samples (`multiple_samples`) at num_samples = 200 and the family's configured mini_batch_size (25,600 / 7,200 / 20,000
    trajectories in one solve; with dopri5 that is the eight-lanes-per-trajectory form): shapes [B, C, T, 200]; with explicit eps and
    with drawn noise (read back), posterior and prior branch: z = loc + scale * eps of the oracle's encoder / priors (2e-5 norm-wise),
    and sample i of row b against the oracle's curves for z[i, b] on the selection V.oracle_rows mapped to (i, b).  rk4: 2e-5 *
    max(1, |mu|), the bar of test_recon_samples_is_one_batched_launch_of_recon.  dopri5 (the engine's default tolerances; recon_samples
    does not return the trajectories): the curves against fp64 heads applied to the fp64 solve at rtol 1e-10, at
    test_forward_solution_level's bar -- err < 3 * err_ref + 1e-5, err_ref the same distance for the fp64 restatement at the engine's
    tolerances -- and within 1e-3.  File names of save_recon_samples."""
    import numpy as np
    m, cfg, batch, ospec, u, times, dev = _model(fam, gauss, solver)
    eng = m._bind().engine
    p = _p64(m)
    ns = 200                                                       # config.num_samples of the reference's proc / challenge configs
    obs = batch["observations"]
    B, L = obs.shape[0], m.latent_dim
    labels = {k: v for k, v in batch.items() if k != "observations"}
    names = ["mean"] if gauss else ["mu_75", "mu_50", "mu_25"]
    pairs = _sample_rows(ns, B)
    ii, bb = [i for i, _ in pairs], [b for _, b in pairs]
    eng.rng_seed(99)
    explicit = torch.randn(ns, B, L, generator=torch.Generator().manual_seed(2)).to(dev)
    for is_post, eps_in in ((True, explicit), (True, None), (False, None)):
        n = eng.rng_state()[2]
        res = m.recon_samples(obs, is_post, ns, eps=eps_in, **labels)
        if eps_in is None:
            assert eng.rng_state()[2] == n + 1
            eps = eng.rng_normal(n, ns * B).view(ns, B, L)
        else:
            assert eng.rng_state()[2] == n
            eps = eps_in
        assert tuple(res["z"].shape) == (ns, B, L)
        loc, scale = O.encoder_conv(p, obs.cpu().double(), ospec.pool_size) if is_post else O.prior_loc_scale(p, ospec, u)
        want_z = loc.unsqueeze(0) + scale.unsqueeze(0) * eps.cpu().double()
        assert V.rel(res["z"], want_z) < 2e-5
        z = res["z"][ii, bb].cpu().double()
        for k in names:
            assert tuple(res[k].shape) == (B, cfg.obs_dim, cfg.seq_len, ns) and bool(torch.isfinite(res[k]).all())
        if solver == "dopri5":
            tight = _heads64(p, ospec, O.solve_ode(p, z, times.double(), "dopri5", rtol=1e-10, atol=1e-12, per_trajectory=True))
            ref = _heads64(p, ospec, O.solve_ode(p, z, times.double(), "dopri5", **DP5_TOL))
            for k in names:
                err_gpu, err_ref = V.elem_err(res[k][bb, :, :, ii], tight[k]), V.elem_err(ref[k], tight[k])
                print("%s gauss=%s post=%s drawn=%s %s: error %.2e (fp64 restatement %.2e)" % (fam, gauss, is_post, eps_in is None, k, err_gpu, err_ref))
                assert err_gpu < 3.0 * err_ref + 1e-5 and err_gpu < 1e-3, (k, is_post, err_gpu, err_ref)
        else:
            _, mus, _ = _decode64(p, ospec, z, times, "rk4")
            for k in names:
                e = V.elem_err(res[k][bb, :, :, ii], mus[k])
                assert e < 2e-5, (k, is_post, e)
    files = m.save_recon_samples(str(tmp_path / "results"), obs[:4], False, 3, **{k: v[:4] for k, v in labels.items()})
    want_files = ["mean_prior_sample.npy"] if gauss else ["mu_25_prior_sample.npy", "mu_50_prior_sample.npy", "mu_75_prior_sample.npy"]
    assert sorted(os.path.basename(f) for f in files) == want_files
    assert np.load(files[0]).shape == (4, cfg.obs_dim, cfg.seq_len, 3)


def _decoder_scalar(outs, ws):
    return sum((w * o).sum() for w, o in zip(ws, outs))


def _oracle_decoder_grads(m, ospec, z, times, ws):
    q = {k: v.requires_grad_(True) for k, v in _p64(m).items()}
    zz = z.detach().cpu().double().requires_grad_(True)
    dec = O.decoder_gauss if ospec.gauss else O.decoder_ald
    outs = dec(q, zz, times.double(), "rk4", grad_mode=ospec.grad_mode)
    _decoder_scalar(outs, [w.cpu().double() for w in ws]).backward()
    return zz.grad, {k: v.grad for k, v in q.items()}


@pytest.mark.parametrize("adam_between", [False, True])
@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("fam,gauss", CLASSES)
def test_decoder_forward_is_an_autograd_module(fam, gauss, adjoint, adam_between):
    """Decoder.forward / GaussianDecoder.forward of all six classes (S = 5 and S = 8), rk4 (the stand-alone solve backward is fixed-grid
    only: an adaptive solver's gradients come with the ELBO step): the scalar sum_k (w_k * out_k).sum() over solution, every curve and
    the expanded std, backward: gradients of z, the ten ODE-net tensors, every head weight and constant_std against fp64 autograd through
    O.decoder_ald / O.decoder_gauss, 5e-4 norm-wise (the suite's gradient bar), adjoint_solver True (torchdiffeq.odeint_adjoint's
    gradients) and False (exact).  adam_between: one fused Adam training step on the model between the forward and the backward -- the
    gradient is still that of the weights the forward saw."""
    from structured_latent_odes_amd.svi import SVI, Adam, Trace_ELBO
    m, cfg, batch, ospec, u, times, dev = _model(fam, gauss, "rk4", adjoint, B=24)
    assert ospec.grad_mode == ("reference_adjoint" if adjoint else "exact")
    m._bind()
    g = torch.Generator().manual_seed(8)
    B = 24
    z = torch.randn(B, m.latent_dim, generator=g).to(dev).requires_grad_(True)
    outs = m.decoder.forward(z)
    assert len(outs) == (3 if gauss else 5) and tuple(outs[-1].shape) == (B, cfg.obs_dim, cfg.seq_len)
    ws = [torch.randn(o.shape, generator=g).to(dev) for o in outs]
    want_z, want = _oracle_decoder_grads(m, ospec, z, times, ws)          # at the forward's weights
    if adam_between:
        svi = SVI(m.model, m.guide, Adam({"lr": 1e-2}), loss=Trace_ELBO(num_particles=1))
        before = m._bind().flat.clone()
        svi.step(**batch)
        assert not torch.equal(before, m._bind().flat)
    for p in m.parameters():
        p.grad = None
    _decoder_scalar(outs, ws).backward()
    assert V.rel(z.grad, want_z) < 5e-4, V.rel(z.grad, want_z)
    checked = 0
    for k, p in m.named_parameters():
        if not k.startswith("decoder.") or ".prod." in k or ".degr." in k:
            continue
        assert p.grad is not None, k
        assert V.rel(p.grad, want[k]) < 5e-4, (k, V.rel(p.grad, want[k]))
        checked += 1
    assert checked == 10 + (1 if gauss else 3) + 1


@pytest.mark.parametrize("fam,gauss", CLASSES)
def test_guide_is_differentiable(fam, gauss):
    """All six classes, rk4, adjoint_solver False (so that z reaches the dynamics too).  The reference's guide samples reparameterised Normal sites: a scalar built from guide(...)'s outputs through decoder.forward
    back-propagates into every encoder.* parameter and equals fp64 autograd through O.encoder_conv -> loc + scale * eps -> O.decoder_*
    for the read-back eps, 5e-4 norm-wise.  The draw and the counter movement are those of the no-grad path (sample_normal)."""
    m, cfg, batch, ospec, u, times, dev = _model(fam, gauss, "rk4", False, B=24)
    eng = m._bind().engine
    obs = batch["observations"]
    labels = {k: v for k, v in batch.items() if k != "observations"}
    eng.rng_seed(5)
    n = eng.rng_state()[2]
    groups = m.guide(obs, **labels)
    assert eng.rng_state()[2] == n + 1
    assert [g.shape[1] for g in groups] == [m.z_dims[k] for k in m.Z_GROUPS]
    z = torch.cat(groups, dim=1)
    assert z.requires_grad
    eps = eng.rng_normal(n, obs.shape[0])
    with torch.no_grad():                                         # the no-grad path draws the same noise
        eng.rng_set_counter(n)
        z_ng = torch.cat(m.guide(obs, **labels), dim=1)
        assert eng.rng_state()[2] == n + 1 and not z_ng.requires_grad
    assert V.rel(z_ng, z) < 1e-6
    outs = m.decoder.forward(z)
    gen = torch.Generator().manual_seed(4)
    ws = [torch.randn(o.shape, generator=gen).to(dev) for o in outs]
    for p in m.parameters():
        p.grad = None
    _decoder_scalar(outs, ws).backward()
    q = {k: v.requires_grad_(True) for k, v in _p64(m).items()}
    loc, scale = O.encoder_conv(q, obs.cpu().double(), ospec.pool_size)
    zz = loc + scale * eps.cpu().double()
    assert V.rel(z, zz) < 2e-5
    dec = O.decoder_gauss if gauss else O.decoder_ald
    _decoder_scalar(dec(q, zz, times.double(), "rk4", grad_mode="exact"), [w.cpu().double() for w in ws]).backward()
    checked = 0
    for k, p in m.named_parameters():
        if k.startswith("encoder."):
            assert p.grad is not None and float(p.grad.abs().max()) > 0, k
            assert V.rel(p.grad, q[k].grad) < 5e-4, (k, V.rel(p.grad, q[k].grad))
            checked += 1
    assert checked == 8
