"""The HIP path against the fp64 oracle AWAY from the initialisation: the suite's seeded cases under the regimes of tests/regime_util.py
(likelihood scales 9e-4 .. 20.5 with both sides of softplus's x > 20 branch, posterior and prior scales over three decades and more,
tripled dynamics weights and a saturated encoder, observations in raw units, exact ties, residuals of the order of a small scale, and all
of it at once).  Every other parity test sits at O.init_params + 0.05 randn on observations in [0, 1].

Bars: the suite's own, by the rule of tests/regime_util.py's docstring (raised to 4 x the fp32 CPU oracle's distance from fp64 where that
is larger; computed here per case and per tensor, never from a kernel's output).  Every case prints its worst error against its bar.
Workspaces and outputs are pre-filled with NaN.  The measured arms (SLODE_ODE_ALG, SLODE_ODE_PACK, SLODE_FOLD_NEXT) stay at the
initialisation regime (tests/test_gpu_instantiations.py).

What `ties` pins: all three quantile heads of channel 0 predict exactly +0.0, and the weights of q75 and q25 are tau and 1 - tau of each
other, so the SUM over the heads of a tie's log-density is the same under `obs >= mu` and `obs > mu` -- neither the loss nor any gradient
can tell the two apart, and the case does not claim to.  It pins what is observable: the residual's sign at a tie is 0 (a sign of +-1
puts 0.5 / std .. 0.975 / std per tie into row 0 of a head's gradient), -0.0 ties like +0.0, and nothing divides by the residual."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import slode_oracle as O
from tests import adaptive_rk_ref as R
from tests import eval_stats_util as EU
from tests import full_size_util as U
from tests import label_evidence_util as LU
from tests import recon_moments_util as RU
from tests import regime_util as G
from tests import traj_bounds_util as TU
from tests.test_gpu_instantiations import FORMS, SHAPES
from tests.test_gpu_parity import CASES as PIECE_CASES

pytestmark = pytest.mark.gpu

B = 12
ENV_KEYS = ("SLODE_ODE_LOOP", "SLODE_ODE_GRID", "SLODE_ODE_GENERIC", "SLODE_ODE_ALG", "SLODE_ODE_PACK", "SLODE_ENC_FUSE", "SLODE_FOLD_NEXT")
_cases, _oracles = {}, {}


def _dev():
    return torch.device("cuda:0")


def _case(shape, regime):
    if (shape, regime) not in _cases:
        fam, kw, T = SHAPES[shape]
        _cases[shape, regime] = G.apply(regime, G.shape_case(fam, kw, T, B))
    return _cases[shape, regime]


def _oracle(shape, regime, mode, which="main"):
    """Both oracles, cached per (shape, regime, mode); the auxiliary loss has no solve and hence no mode."""
    key = (shape, regime, mode if which == "main" else None, which)
    if key not in _oracles:
        c = _case(shape, regime)
        _oracles[key] = G.Oracles(dict(c, ospec=dataclasses.replace(c["ospec"], grad_mode=mode)), which)
    return _oracles[key]


def _engine(c, mode, env, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = U.engine(c["fam"], c["kw"], c["T"], _dev(), mode)          # a fresh handle: the flags are read in slode_create
    eng.set_times(c["times"])
    return eng


def _twice(step, eng, n):
    """``step(loss, grads)`` twice on NaN-filled workspace and outputs: bitwise equal, finite."""
    outs = []
    for _ in range(2):
        eng.workspace(n).fill_(float("nan"))
        loss, grads = torch.full((1,), float("nan"), device=_dev()), torch.full((eng.n_params,), float("nan"), device=_dev())
        step(loss, grads)
        outs.append((loss.clone(), grads.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "not bitwise reproducible"
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    return outs[0]


def _main_step(shape, regime, mode, env, monkeypatch):
    """The training step of one case in one launch form against the fp64 oracle; returns (case, oracles, engine, device inputs, gradients)."""
    c, om = _case(shape, regime), _oracle(shape, regime, mode)
    eng = _engine(c, mode, env, monkeypatch)
    flat, dev = eng.pack(c["p"]), _dev()
    ins = (flat, U.to_device(c["obs"], dev), c["u"].to(dev).contiguous(), c["eps"].to(dev).contiguous())
    loss, grads = _twice(lambda l, g: eng.elbo_step(*ins, l, grads=g), eng, B)
    got = eng.unpack(grads)
    om.check(loss, got, "%s %s %s %s" % (shape, regime, mode, "+".join(env) or "default"))
    loss2 = torch.full((1,), float("nan"), device=dev)
    eng.elbo_step(*ins, loss2, grads=None)                           # the forward-only launch scores the same loss
    assert abs(loss2.item() - loss.item()) <= 2e-6 * abs(loss.item())
    return c, om, eng, ins, got


def _block(om, got, name, mask, what, suite=G.GRAD_BAR):
    d32, _ = om.block(name, mask)
    b = G.bar(suite, d32)
    e = G.block_rel(got[name], om.o64["grads"][name], mask)
    print("%s: %s block of %d entries: %.2e / bar %.2e (fp32 oracle %.2e)" % (what, name, int(mask.sum()), e, b, d32))
    assert e <= b, (what, name, e, b)


# ---- 1. the training step, every compiled shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", list(G.REGIMES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_training_step(shape, regime, monkeypatch):
    """exact mode, the default (specialised, loop-free) form: -ELBO and every gradient tensor, the forward-only loss, the auxiliary step
    against O.aux_loss.  tight_noise / fitted: decoder.constant_std's gradient also on the block of entries with a raw value below -4 (a norm
    over the whole tensor hides the small-scale entries).  ties: row 0 of every head's gradient on its own (module docstring)."""
    c, om, eng, ins, got = _main_step(shape, regime, "exact", {}, monkeypatch)
    what = "%s %s" % (shape, regime)
    if regime in ("tight_noise", "fitted"):
        # at the gradient bar, and at the suite's bar for this factor on its own (g_cstd of test_gpu_parity.test_decode_heads_backward,
        # 2e-6): softplus' is exact to rounding (softplus_gradf), so the block has no reason to sit further from fp64 than that or than
        # 4 x the fp32 oracle.  As 1 - exp(-scale) it sat at 1e-5, a hundred times the fp32 oracle.
        _block(om, got, "decoder.constant_std", G.small_std_block(c), what)
        _block(om, got, "decoder.constant_std", G.small_std_block(c), what + " (softplus')", suite=2e-6)
    if regime == "ties":
        for k in got:
            if k.startswith("decoder.output_"):
                mask = torch.zeros(got[k].shape, dtype=torch.bool)
                mask[0] = True
                _block(om, got, k, mask, what)
    oa = _oracle(shape, regime, "exact", "aux")
    loss, grads = _twice(lambda l, g: eng.aux_step(*ins, l, g), eng, B)
    oa.check(loss, eng.unpack(grads), what)
    loss2 = torch.full((1,), float("nan"), device=_dev())
    eng.aux_step(*ins, loss2, None)
    assert abs(loss2.item() - loss.item()) <= 2e-6 * abs(loss.item())


@pytest.mark.parametrize("regime", ["trained_weights", "fitted", "all"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_training_step_reference_adjoint(shape, regime, monkeypatch):
    _main_step(shape, regime, "reference_adjoint", {}, monkeypatch)


@pytest.mark.parametrize("mode", ["exact", "reference_adjoint"])
@pytest.mark.parametrize("regime", ["fitted", "all"])
@pytest.mark.parametrize("form", [f for f in FORMS if f != "loop_free"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_training_step_other_forms(shape, form, regime, mode, monkeypatch):
    """The persistent loop (5 workgroups, 2-3 trajectories each), the generic kernel, and both."""
    _main_step(shape, regime, mode, FORMS[form], monkeypatch)


@pytest.mark.parametrize("mode", ["exact", "reference_adjoint"])
def test_metric_shape_with_the_separate_encoder_launch(mode, monkeypatch):
    _main_step("c1_cvs_T200_L8_rk4", "all", mode, {"SLODE_ENC_FUSE": "0"}, monkeypatch)


def test_training_step_on_padded_observations(monkeypatch):
    """Observation rows that are not dense (padded in both trailing dimensions) take the layer-by-layer encoder, and the step runs without
    the per-step table of likelihood scales: the kernel evaluates 1 / scale, log(2 scale) and softplus' itself.  Metric shape at tight_noise."""
    shape, regime = "c1_cvs_T200_L8_rk4", "tight_noise"
    c, om = _case(shape, regime), _oracle(shape, regime, "exact")
    eng, dev, T = _engine(c, "exact", {}, monkeypatch), _dev(), c["T"]
    big = torch.zeros(B, T + 7, 5, device=dev)
    big[:, :T, :3] = c["obs"].permute(0, 2, 1).to(dev)
    obs_d = big[:, :T, :3].permute(0, 2, 1)
    assert obs_d.stride() == ((T + 7) * 5, 1, 5)
    ins = (eng.pack(c["p"]), obs_d, c["u"].to(dev).contiguous(), c["eps"].to(dev).contiguous())
    loss, grads = _twice(lambda l, g: eng.elbo_step(*ins, l, grads=g), eng, B)
    got = eng.unpack(grads)
    what = "%s %s padded rows" % (shape, regime)
    om.check(loss, got, what)
    _block(om, got, "decoder.constant_std", G.small_std_block(c), what)
    _block(om, got, "decoder.constant_std", G.small_std_block(c), what + " (softplus')", suite=2e-6)


# ---- 2. the stand-alone pieces, to localise a failure of 1. ---------------------------------------------------------------------------------
def _as(p, dtype):
    return {k: v.to(dtype) for k, v in p.items()}


def _piece(what, got, ref, suite, metric=U.rel):
    """``got`` against ``ref(torch.float64)`` under ``metric`` at the bar rule: ``suite``, or 4 x the distance of ``ref(torch.float32)``."""
    want = ref(torch.float64)
    d32 = metric(ref(torch.float32), want)
    e, b = metric(got, want), G.bar(suite, d32)
    print("%s: %.2e / bar %.2e (fp32 oracle %.2e)" % (what, e, b, d32))
    assert e <= b, (what, e, b)


@pytest.fixture(scope="module", params=[(c, r) for c in PIECE_CASES for r in ("trained_weights", "all")], ids=lambda v: "%s-%s" % v)
def piece(request):
    name, regime = request.param
    fam, kw, n, T = PIECE_CASES[name]
    c = G.apply(regime, G.shape_case(fam, kw, T, n, seed=11))
    eng = U.engine(fam, kw, T, _dev())
    eng.set_times(c["times"])
    return dict(c, eng=eng, flat=eng.pack(c["p"]), obs_d=U.to_device(c["obs"], _dev()), tag="%s %s" % (name, regime))


def test_piece_encoder_forward_and_backward(piece):
    c, eng, dev = piece, piece["eng"], _dev()
    ospec, L = c["ospec"], c["ospec"].latent_dim
    loc, scale, pooled, hid = eng.encoder_fwd(c["flat"], c["obs_d"])
    enc = lambda dt: O.encoder_conv(_as(c["p"], dt), c["obs"].to(dt), ospec.pool_size)
    _piece(c["tag"] + " encoder loc", loc, lambda dt: enc(dt)[0], 2e-5)
    _piece(c["tag"] + " encoder scale", scale, lambda dt: enc(dt)[1], 2e-5)
    g = torch.Generator().manual_seed(8)
    g_loc, g_scale = torch.randn(c["B"], L, generator=g), torch.randn(c["B"], L, generator=g)
    grads = torch.zeros(eng.n_params, device=dev)
    eng.encoder_bwd(c["flat"], c["obs_d"], scale, pooled, hid, g_loc.to(dev), g_scale.to(dev), grads)
    got = eng.unpack(grads)

    def ref(dt):
        q = {k: v.detach().to(dt).clone().requires_grad_(k.startswith("encoder.")) for k, v in c["p"].items()}
        wl, ws = O.encoder_conv(q, c["obs"].to(dt), ospec.pool_size)
        ((wl * g_loc.to(dt)).sum() + (ws * g_scale.to(dt)).sum()).backward()
        return {k: v.grad for k, v in q.items() if k.startswith("encoder.")}
    r64, r32 = ref(torch.float64), ref(torch.float32)
    for k in r64:
        _piece(c["tag"] + " encoder backward " + k, got[k], lambda dt: (r64 if dt == torch.float64 else r32)[k], 2e-4)


def test_piece_ode_solve_forward_and_backward(piece):
    c, eng, dev = piece, piece["eng"], _dev()
    ospec = c["ospec"]
    z = torch.randn(c["B"], ospec.latent_dim, generator=torch.Generator().manual_seed(3))
    x = eng.ode_solve(c["flat"], z.to(dev))
    assert torch.isfinite(x).all()
    _piece(c["tag"] + " trajectories", x, lambda dt: O.solve_ode(_as(c["p"], dt), z.to(dt), c["times"].to(dt), ospec.solver), 1e-5, U.traj_err)
    g = torch.Generator().manual_seed(9)
    z = torch.randn(c["B"], ospec.latent_dim, generator=g)
    gx = torch.randn(c["B"], c["T"], c["S"], generator=g)
    grads = torch.zeros(eng.n_params, device=dev)
    gz = eng.ode_solve_bwd(c["flat"], z.to(dev), gx.to(dev), grads)
    got = eng.unpack(grads)

    def ref(dt):
        q = {k: v.detach().to(dt).clone().requires_grad_("ode_model" in k) for k, v in c["p"].items()}
        zz = z.to(dt).clone().requires_grad_(True)
        (O.solve_ode(q, zz, c["times"].to(dt), ospec.solver) * gx.to(dt)).sum().backward()
        return dict({k: v.grad for k, v in q.items() if "ode_model" in k}, z=zz.grad)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    got["z"] = gz
    for k in r64:
        _piece(c["tag"] + " solve backward " + k, got[k], lambda dt: (r64 if dt == torch.float64 else r32)[k], 5e-4)


def test_piece_small_nets_and_heads(piece):
    c, eng, dev = piece, piece["eng"], _dev()
    ospec = c["ospec"]
    z = torch.randn(c["B"], ospec.latent_dim, generator=torch.Generator().manual_seed(6))
    _piece(c["tag"] + " initialize_state", eng.initialize_state(c["flat"], z.to(dev)), lambda dt: O.initialize_state(_as(c["p"], dt), z.to(dt)), 1e-6)
    loc, scale = eng.prior_nets(c["flat"], c["u"].to(dev).contiguous())
    pri = lambda dt: O.prior_loc_scale(_as(c["p"], dt), ospec, c["u"].to(dt))
    _piece(c["tag"] + " prior loc", loc, lambda dt: pri(dt)[0], 1e-6)
    _piece(c["tag"] + " prior scale", scale, lambda dt: pri(dt)[1], 1e-6)
    probs = eng.label_heads(c["flat"], z.to(dev)).cpu()
    for kind, prefix, zo, zd, uo, ud in ospec.aux_heads:
        f = {"bernoulli": O.classifier_sigmoid, "onehot": O.classifier_softmax}.get(kind) or (lambda p, pre, zg: O.regressor_exp_exp(p, pre, zg)[0])
        _piece(c["tag"] + " label head " + prefix, probs[:, uo:uo + ud], lambda dt: f(_as(c["p"], dt), prefix, z[:, zo:zo + zd].to(dt)), 2e-6)
    # the heads on states of the size the tripled dynamics reach (the suite's decode_heads test feeds rand in [0, 1])
    x = torch.rand(c["B"], c["T"], c["S"], generator=torch.Generator().manual_seed(4)) * 200.0
    mu, std = eng.decode_heads(c["flat"], x.to(dev))
    names = ["decoder.output_mean.0.weight"] if ospec.gauss else ["decoder.output_%s.0.weight" % q for q in ("q50", "q75", "q25")]
    for i, n in enumerate(names):
        _piece(c["tag"] + " head " + n, mu[i], lambda dt: torch.nn.functional.linear(x.to(dt), c["p"][n].to(dt)).permute(0, 2, 1), 1e-6)
    _piece(c["tag"] + " std", std, lambda dt: torch.nn.functional.softplus(c["p"]["decoder.constant_std"].to(dt)), 1e-6)


# ---- 3. the adaptive step --------------------------------------------------------------------------------------------------------------------
AB = 22          # one full sixteen-trajectory workgroup and a ragged one


def _adaptive(method, regime, mode, rtol, atol):
    from structured_latent_odes_amd import engine as E
    dev = _dev()
    kw, S, T = dict(z_iext=3, z_rtpr=3, z_eps=2), 5, 60
    ospec = dataclasses.replace(O.cvs_spec(solver="dopri5", **kw), grad_mode=mode)
    obs, u, eps, times = O.synthetic_batch(ospec, AB, T)
    base = dict(fam="cvs", kw=kw, T=T, S=S, B=AB, ospec=ospec, p=U.params(ospec, T, S, seed=31), obs=obs, u=u, eps=eps, times=times * 0.25)
    tab = R.TABLEAUS[method] if method != "dopri5" else None
    c = G.apply(regime, base)
    espec = dataclasses.replace(E.cvs_spec(solver=method, **kw), grad_mode=mode, rtol=rtol, atol=atol)
    eng = E.Engine(espec, T, dev)
    eng.set_times(c["times"])
    flat, obs_d = eng.pack(c["p"]), U.to_device(c["obs"], dev)
    loss, grads = torch.full((1,), float("nan"), device=dev), torch.full((eng.n_params,), float("nan"), device=dev)
    x = torch.full((AB, T, S), float("nan"), device=dev)
    eng.workspace(AB).fill_(float("nan"))
    eng.elbo_step(flat, obs_d, c["u"].to(dev), c["eps"].to(dev), loss, grads=grads, x_out=x)
    assert torch.isfinite(loss).all() and torch.isfinite(grads).all() and torch.isfinite(x).all()
    n = eng.dopri5_step_counts(AB).cpu()
    kmax = U.dopri5_kmax(AB, S)
    print("%s %s %s: accepted steps %s (record %d)" % (method, regime, mode, n.tolist(), kmax))
    assert int(n.min()) >= 1 and int(n.max()) < kmax, n
    ospec.solver_kw = dict(rtol=1e-10, atol=1e-12, per_trajectory=True)
    tight = U.oracle(c["p"], ospec, c["obs"], c["u"], c["eps"], c["times"])
    ospec.solver_kw = dict(rtol=rtol, atol=atol, per_trajectory=True)
    if tab is None:
        loose = U.oracle(c["p"], ospec, c["obs"], c["u"], c["eps"], c["times"])
    else:
        with R.patched(tab):
            loose = U.oracle(c["p"], ospec, c["obs"], c["u"], c["eps"], c["times"])
    sens = U.step_sensitivity(loose, tight)
    return eng, loss, grads, x, tight, sens


@pytest.mark.parametrize("regime,mode", [("trained_weights", "exact"), ("trained_weights", "reference_adjoint"), ("posterior_scales", "exact")])
def test_dopri5_step_at_default_tolerances(regime, mode):
    """cvs, L = 8, T = 60, times x 0.25, torchdiffeq's default tolerances, against the fp64 oracle at rtol 1e-10 / atol 1e-12 at the bars of
    test_gpu_parity.test_dopri5_elbo_step_at_default_tolerances plus the oracle's own sensitivity to the step sequence."""
    eng, loss, grads, x, tight, sens = _adaptive("dopri5", regime, mode, 1e-7, 1e-9)
    le, xe = U.loss_err(loss, tight["loss"]), U.traj_err(x, tight["x"])
    worst, werr = None, None
    try:
        worst, werr = U.check_grads(eng.unpack(grads), tight["grads"], sens=sens, what="dopri5 %s %s" % (regime, mode))
    finally:
        print("dopri5 %s %s: loss %.2e / bar %.2e, x %.2e / bar %.2e, worst tensor %s %s (largest sensitivity %s %.2e)"
              % ((regime, mode, le, 2e-5 + 3.0 * sens["loss"], xe, 1e-4 + 3.0 * sens["x"], worst, werr) + U.worst_sensitivity(sens)))
    assert le < 2e-5 + 3.0 * sens["loss"], (le, sens["loss"])
    assert xe < 1e-4 + 3.0 * sens["x"], (xe, sens["x"])


def test_bosh3_step_with_trained_weights():
    """The bars of test_gpu_adaptive_methods.test_elbo_step_against_oracle at its tolerances (rtol 1e-6, atol 1e-8)."""
    eng, loss, grads, x, tight, sens = _adaptive("bosh3", "trained_weights", "exact", 1e-6, 1e-8)
    le, xe = U.loss_err(loss, tight["loss"]), U.traj_err(x, tight["x"])
    print("bosh3 trained_weights: loss %.2e / bar %.2e, x %.2e / bar %.2e" % (le, 5e-4 + 3.0 * sens["loss"], xe, 1e-4 + 3.0 * sens["x"]))
    assert le < 5e-4 + 3.0 * sens["loss"], (le, sens["loss"])
    assert xe < 1e-4 + 3.0 * sens["x"], (xe, sens["x"])
    worst, werr = U.check_grads(eng.unpack(grads), tight["grads"], sens=sens, what="bosh3 trained_weights")
    print("bosh3 trained_weights: worst tensor %s %.2e (sensitivity %.2e)" % (worst, werr, sens[worst]))


# ---- 4. the forward the eval-side calls share -----------------------------------------------------------------------------------------------
EB, EK = 4, 3


def _default_hypotheses(c):
    """The tables of MechanisticBase.default_hypotheses: {0, 1}^2 (cvs, challenge); identity rows of aR x identity rows of aS (proc)."""
    if c["fam"] != "proc":
        return LU.binary_grid(c)
    return [torch.eye(3).repeat_interleave(4, 0).contiguous(), torch.eye(4).repeat(3, 1).contiguous(), None, None]


def _bounds(eng, flat, c, u=None):
    from tests.eval_gpu_util import _device_batch
    obs_d, labels = _device_batch(c if u is None else dict(c, u=u))
    bounds = torch.full((EB, 4), float("nan"), device=_dev())
    loss = torch.full((EK, EB), float("nan"), device=_dev())
    eng.traj_bounds(flat, eng.make_batch(obs_d, labels, c["eps"].to(_dev()).contiguous(), particles=EK), EB, EK, bounds, loss)
    return bounds, loss


@pytest.mark.parametrize("regime", G.BOUNDS_REGIMES)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_traj_bounds(case, regime, monkeypatch):
    """slode_forward.h and traj_terms.h, which fifteen calls share, through traj_bounds with explicit eps [K, B, L]: per-draw, per-trajectory
    losses and the slots against TU.oracle_rows under the bar rule, and the call's own reduction.  At `all`, label_evidence on the family's
    default hypotheses stays bitwise the traj_bounds result for those labels."""
    from tests.eval_gpu_util import _device_batch, _engine as eval_engine
    c = G.apply(regime, TU.build(case, "rk4", B=EB, K=EK))
    eng = eval_engine(c, monkeypatch)
    flat = eng.pack(c["p"])
    eng.workspace(EB).fill_(float("nan"))
    bounds, loss = _bounds(eng, flat, c)
    want, r32 = G.bounds_oracles(c)
    tag = "%s %s (fp32 oracle / suite bar %.2f)" % (case, regime, r32)
    TU.check_oracle(bounds, loss, want, tag)
    TU.check_reduction(bounds, loss, tag)
    if regime == "all":
        tabs = _default_hypotheses(c)
        V = next(t for t in tabs if t is not None).shape[0]
        obs_d, labels = _device_batch(c)
        ev = torch.full((EB, V, 4), float("nan"), device=_dev())
        best = torch.full((EB,), -7, dtype=torch.int32, device=_dev())
        lv = torch.full((V, EK, EB), float("nan"), device=_dev())
        hyp = [None if t is None else t.to(_dev()).contiguous() for t in tabs]
        eng.label_evidence(flat, eng.make_batch(obs_d, labels, c["eps"].to(_dev()).contiguous(), particles=EK), EB, EK, hyp, V, None, ev, best, lv)
        assert torch.isfinite(ev).all() and torch.isfinite(lv).all()
        for v in range(V):
            b_v, l_v = _bounds(eng, flat, c, u=LU.substituted(c, tabs, v))
            assert torch.equal(ev[:, v, :3], b_v[:, :3]) and torch.equal(lv[v], l_v), (case, v)


@pytest.mark.parametrize("case", ["cvs_ald", "challenge_gauss"])
def test_recon_moments_at_all(case, monkeypatch):
    """Mean and sd over 7 posterior draws at `all`: tests/recon_moments_util's bars (stated for bounded curves) under the bar rule -- the
    curves now reach O(100)."""
    from tests.eval_gpu_util import _engine as eval_engine, _recon_moments
    c = G.apply("all", RU.build(case, "rk4", B=EB, ns=7))
    eng = eval_engine(c, monkeypatch)
    mean, sd = _recon_moments(eng, eng.pack(c["p"]), c, True)
    m64, s64 = G.moments(c, True)
    m32, s32 = G.moments(c, True, torch.float32)
    scale = np.maximum(1.0, np.abs(m64))
    dm, ds = float((np.abs(m32 - m64) / scale).max()), float((np.abs(s32 - s64) / scale).max())
    bm, bs = G.bar(RU.MEAN_BAR, dm), G.bar(RU.SD_BAR, ds)
    m, s = mean.double().cpu().numpy(), sd.double().cpu().numpy()
    em, es = float((np.abs(m - m64) / scale).max()), float((np.abs(s - s64) / scale).max())
    print("%s all: mean %.2e / bar %.2e (fp32 oracle %.2e), sd %.2e / bar %.2e (fp32 oracle %.2e), largest |mean| %.1f"
          % (case, em, bm, dm, es, bs, ds, float(np.abs(m64).max())))
    assert np.isfinite(m).all() and np.isfinite(s).all()
    assert em <= bm and es <= bs, (case, em, bm, es, bs)
