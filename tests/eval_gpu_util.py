"""What the GPU tests of the fifteen eval-side calls (test_gpu_eval_stats, test_gpu_recon_moments, test_gpu_intervene, test_gpu_forecast,
test_gpu_cohort, test_gpu_calibration, test_gpu_traj_bounds, test_gpu_label_evidence, test_gpu_refine, test_gpu_pointwise, and the
whole-curve calls' test_gpu_attribution, test_gpu_summary, test_gpu_quantiles, test_gpu_mechanism, test_gpu_band) share: an engine for a
seeded case (tests/eval_stats_util.py) with the handle's environment switches under control, the case's batch on the device, the model of
the model-level tests with its 17-trajectory batch, the checks every call gets -- refusal, capture and replay, peak allocation -- and what
the whole-curve tests compare with: the kernel's own curve of every draw, the model's own curves, bitwise agreement, the count of engine
calls; and, since test_gpu_eval_regimes runs every call on the regimes' cases, the one-call helpers of the LOO, whole-curve and cohort
tests with their checks on the kernel's own values (at the end).  A plain module: not a conftest, not imported by the product."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import band_util as BU
from tests import calibration_util as KU
from tests import cohort_util as CU
from tests import eval_stats_util as EU
from tests import loo_util as LU
from tests import mechanism_util as MU
from tests import recon_moments_util as RU

DEV = torch.device("cuda:0")
WIDTHS = {"cvs": (1, 1), "challenge": (1, 1), "proc": (3, 4, 1, 1)}
ENV_KEYS = ("SLODE_ODE_LOOP", "SLODE_ODE_GRID", "SLODE_ODE_GENERIC", "SLODE_ODE_ALG", "SLODE_ODE_PACK", "SLODE_FOLD_NEXT", "SLODE_NO_FOLD")
ADAPTIVE = ("dopri5", "bosh3", "fehlberg2", "adaptive_heun")


def _set_env(monkeypatch, env):
    """The handle's environment switches: all cleared, then ``env`` set (nothing is touched without ``monkeypatch``)."""
    if monkeypatch is not None:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)


def _engine(c, monkeypatch=None, env=None, solver=None):
    from structured_latent_odes_amd import engine as E
    _set_env(monkeypatch, env)
    kw = dict(c["kw"])
    if solver:
        kw["solver"] = solver
    eng = E.Engine({"cvs": E.cvs_spec, "challenge": E.challenge_spec, "proc": E.proc_spec}[c["fam"]](**kw), c["T"], DEV)
    eng.set_times(c["times"])
    return eng


def _device_batch(c):
    """Observations in the family's layout -- the [B,C,T] view of a contiguous [B,T,C] tensor (cvs / challenge) or contiguous [B,C,T]
    (proc): the two dense layouts the folded encoder takes -- and the label tensors one by one."""
    obs = c["obs"]
    obs_d = obs.to(DEV).contiguous() if c["fam"] == "proc" else obs.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
    labels, o = [], 0
    for w in WIDTHS[c["fam"]]:
        labels.append(c["u"][:, o:o + w].contiguous().to(DEV))
        o += w
    return obs_d, labels


def _lay(t, t_major):
    """A host [B, C, T] tensor on the device in one of the two dense layouts: the [B,C,T] view of a contiguous [B,T,C] tensor, or contiguous."""
    return t.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1) if t_major else t.to(DEV).contiguous()


def _eps_dev(eps):
    return (eps[0] if eps.shape[0] == 1 else eps).to(DEV).contiguous()       # one draw: [B, L], as make_batch takes it


def _recon_moments(eng, flat, c, is_post, eps="case", obs_d=None, labels=None, ns=None):
    """Engine.recon_moments on the case's batch; outputs pre-filled with NaN: every element must be written."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q = 1 if c["ospec"].gauss else 3
    mean = torch.full((Q, c["B"], c["obs"].shape[1], c["T"]), float("nan"), device=DEV)
    sd = torch.full_like(mean, float("nan"))
    eng.recon_moments(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], is_post, ns, mean, sd)
    return mean, sd


# (case, B, ns, env) of the tests "sizes and instantiations" of recon_moments and intervene_moments
SIZES = [("cvs_gauss", 63, 2, {}), ("cvs_gauss", 65, 7, {}), ("cvs_gauss", 255, 2, {}), ("cvs_gauss", 257, 1, {}), ("cvs_ald", 3, 200, {}),
         ("proc_gauss", 65, 2, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}), ("challenge_gauss", 2, 200, {}),
         ("cvs_ald", 9, 7, {"SLODE_ODE_GENERIC": "1"}), ("proc_ald", 9, 2, {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"})]


def _padded(obs):
    """``obs`` as the ``[..., :T]`` view of a tensor three points longer: the same values, a row stride no fused call takes."""
    wide = torch.zeros(obs.shape[0], obs.shape[1], obs.shape[2] + 3, device=DEV)
    wide[:, :, :obs.shape[2]] = obs
    return wide[:, :, :obs.shape[2]]


def _on_device(batch, fam):
    """A host batch of ``EU.model_state`` on the device, the observations in the family's layout (``_device_batch``)."""
    batch = {k: v.to(DEV) for k, v in batch.items()}
    if fam != "proc":
        batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    return batch


def _model_batches(fam, solver=None, monkeypatch=None, env=None):
    """The model of ``EU.model_state(fam)`` on the device (``solver`` replaces rk4) and the host batches of its pass."""
    _set_env(monkeypatch, env)
    twin, state, batches, times = EU.model_state(fam)
    cfg = EU.model_config(fam)
    if solver:
        cfg.update(solver=solver)
    m = importlib.import_module("structured_latent_odes_amd.models.mechanistic_" + fam).MechanisticModel(cfg, DEV, times.to(DEV))
    m.load_state_dict(state)
    return m, batches


def _model(fam, solver=None, monkeypatch=None, env=None):
    """``_model_batches`` with the third batch (17 trajectories) on the device."""
    m, batches = _model_batches(fam, solver, monkeypatch, env)
    return m, _on_device(batches[2], fam)


def _peak(fn):
    """Peak of torch.cuda.max_memory_allocated during ``fn()`` over the allocation before the call."""
    torch.cuda.synchronize(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    out = fn()
    torch.cuda.synchronize(DEV)
    del out
    return torch.cuda.max_memory_allocated(DEV) - before


def _refused(eng, call, match, error=None):
    """``call()`` on ``eng`` raises ``error`` (SlodeError by default) matching ``match``, draws nothing (seed 3, counter 4 before and after)
    and launches nothing (profile on: "no profiled step").  Returns the exception: its status is the call site's to check."""
    from structured_latent_odes_amd import _lib as L
    eng.rng_seed(3)
    eng.rng_set_counter(4)
    eng.profile_enable(True)
    with pytest.raises(error or L.SlodeError, match=match) as ei:
        call()
    assert eng.rng_state() == (3, 0, 4)
    with pytest.raises(L.SlodeError, match="no profiled step"):
        eng.profile_read()
    return ei.value


def _captured(call, outs):
    """``call`` writes the zero-filled tensors ``outs``.  Launched on a side stream; then, outputs zeroed, captured on that stream
    (capturing executes nothing) and replayed once.  Returns the stream-launched values, for the caller to compare ``outs`` with."""
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    want = [t.clone() for t in outs]
    for t in outs:
        t.zero_()
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call()
    torch.cuda.synchronize(DEV)
    assert all(t.abs().sum().item() == 0.0 for t in outs), "capturing must not execute anything"
    g.replay()
    torch.cuda.synchronize(DEV)
    return want


# ---- the whole-curve calls (attribution, summary, quantiles, mechanism, band) ---------------------------------------------------------------
def _same(a, b, equal_nan):
    """Bitwise agreement of two numpy arrays: dtype, shape, every element; ``equal_nan``: whether a NaN agrees with a NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=equal_nan)


def _per_draw_curves(eng, flat, c, is_post, obs_d, labels):
    """[K, Q, B, C, T] fp32: the kernel's own curve of every draw -- recon_moments with num_samples = 1 on that draw's noise row."""
    eps = c["eps"].to(DEV)
    return np.stack([_recon_moments(eng, flat, c, is_post, eps=eps[k].contiguous(), obs_d=obs_d, labels=labels, ns=1)[0].cpu().numpy()
                     for k in range(eps.shape[0])])


def _model_curves(m, batch, is_post, eps, heads_axis=0):
    """[Q, ns, B, C, T] fp64 (``heads_axis`` = 1: [ns, Q, B, C, T]): the model's own decoder on the same draws (recon_samples)."""
    res = m.recon_samples(is_post=is_post, num_samples=eps.shape[0], eps=eps, **batch)
    return np.stack([res[n].double().permute(3, 0, 1, 2).cpu().numpy() for n in m.MOMENT_HEADS[bool(m.GAUSS)]], heads_axis)


def _count_calls(monkeypatch, eng, name, note=lambda args: 1):
    """The list that takes ``note(positional arguments)`` of every call of the engine method ``name`` from now on."""
    calls, real = [], getattr(eng, name)
    monkeypatch.setattr(eng, name, lambda *a, **k: (calls.append(note(a)), real(*a, **k))[1])
    return calls


# ---- pointwise_loo (test_gpu_loo, test_gpu_eval_regimes) --------------------------------------------------------------------------------------
def _loo(eng, flat, c, K=None, eps="case", obs_d=None, labels=None, mask=None, loc=None, scale=None, tile=0, tail=True):
    """Engine.pointwise_loo on the case's batch; outputs pre-filled with NaN: every element must be written."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    K = c["K"] if K is None else K
    e = c["eps"] if isinstance(eps, str) else eps
    if e is not None:
        e = (e[0] if K == 1 and e.dim() == 3 else e).to(DEV).contiguous()
    B, Cn, T = c["obs"].shape
    point = torch.full((3, B, Cn, T), float("nan"), device=DEV)
    summary = torch.full((B, 8), float("nan"), device=DEV)
    tl = torch.full((LU.tail_len(K) + 1, B, Cn, T), float("nan"), device=DEV) if tail else None
    eng.pointwise_loo(flat, eng.make_batch(obs_d, labels, e, particles=max(K, 1)), B, K, mask=mask, loc=loc, scale=scale, tile=tile, point=point,
                      summary=summary, tail=tl)
    return point, summary, tl


def _density(eng, flat, c, eps, K, obs_d, labels, **kw):
    B = c["B"]
    e = (eps[0] if K == 1 else eps).to(DEV).contiguous()
    return eng.pointwise_density(flat, eng.make_batch(obs_d, labels, e, particles=K), B, K, 0, loss_kb=False, **kw)[0]


def _own_l(eng, flat, c, obs_d, labels, **kw):
    """[K, B, C, T] fp32: the kernel's own l_k -- plane 0 of pointwise_density with one draw on that draw's noise row."""
    return np.stack([_density(eng, flat, c, c["eps"][k:k + 1], 1, obs_d, labels, **kw)[0].cpu().numpy() for k in range(c["eps"].shape[0])])


def _check_own_sums(point, summary, mask=None):
    """The eight slots against the fp64 sums of the call's own planes: 2^-23 |sum| (+ 2^-50 of the magnitudes); counts and the max exact."""
    got, gs = point.double().cpu().numpy(), summary.double().cpu().numpy()
    inn = np.ones(got.shape[1:], bool) if mask is None else np.asarray(mask) > 0
    for j, (v, sel) in ((0, (got[0], inn)), (1, (got[2], inn)), (5, (got[0], ~inn)), (6, (got[2], ~inn))):
        s, mag = np.where(sel, v, 0.0).sum((1, 2)), np.where(sel, np.abs(v), 0.0).sum((1, 2))
        assert np.all(np.abs(gs[:, j] - s) <= 2.0 ** -23 * np.abs(s) + 2.0 ** -50 * mag), ("slot", j, gs[:, j], s)
    assert np.array_equal(gs[:, 2], inn.sum((1, 2))) and np.array_equal(gs[:, 7], (~inn).sum((1, 2)))
    assert np.array_equal(gs[:, 3], ((got[1] > 0.7) & inn).sum((1, 2)))
    assert np.array_equal(gs[:, 4], np.where(inn, got[1], -np.inf).max((1, 2)))


def _check_fit(point, l, tag, finite_bars=False):
    """elpd_loo and khat against the restatement on the kernel's own l: K 2^-23 max(1, |v|) for elpd_loo (the fp32 running sums), the
    restatement's own sensitivity to 2^-24 |l| for khat.  ``finite_bars``: no point's khat bar may be infinite (a perturbation of 2^-24 |l|
    that switches a point between smoothed and unsmoothed would leave it out).  Returns the worst error-to-bar ratios."""
    K = l.shape[0]
    e, k = LU.psis(l)
    got = point.double().cpu().numpy()
    re = np.abs(got[0] - e) / (K * 2.0 ** -23 * np.maximum(1.0, np.abs(e)))
    kb = LU.khat_bar(l, 2.0 ** -24 * np.abs(l))
    assert np.array_equal(np.isinf(got[1]), np.isinf(k)), tag
    assert not finite_bars or np.isfinite(kb).all(), (tag, "points with an infinite khat bar", int(np.isinf(kb).sum()))
    fin = np.isfinite(k) & np.isfinite(kb)
    rk = np.abs(np.where(fin, got[1], 0.0) - np.where(fin, k, 0.0)) / np.where(fin, kb, 1.0)
    print("%s: error / bar: elpd_loo %.3f, khat %.3f (khat in [%.3f, %.3f], %d of %d points smoothed)"
          % (tag, re.max(), rk.max(), np.min(k), np.max(np.where(np.isfinite(k), k, -np.inf)), int(np.isfinite(k).sum()), k.size))
    assert re.max() <= 1.0 and rk.max() <= 1.0, (tag, re.max(), rk.max())
    return re.max(), rk.max()


# ---- the calls of the whole-curve and cohort tests, one helper per call (their own test files and test_gpu_eval_regimes) ----------------------
FILL = -12345.5            # outputs are pre-filled with it where NaN is a value the call writes: every element must be written
NAN = float("nan")
BAND_LEVELS = (0.95, 0.5, 1.0, 0.1)
CALIB_ALL = ("inside", "cross", "pinball", "width")
COHORT_ALL = ("sd", "sd_subjects", "obs_mean", "l1")
MECH_GUARD, MECH_NG = 7.25, 64   # the mechanism outputs stand between MECH_NG guard words, which must stay
_band_same = functools.partial(_same, equal_nan=True)


def _quantiles(eng, flat, c, is_post, levels, eps="case", ns=None, tile=0, obs_d=None, labels=None):
    """Engine.recon_quantiles on the case's batch -> numpy [Lv, Q, B, C, T]."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q, Cn = (1 if c["ospec"].gauss else 3), c["obs"].shape[1]
    out = torch.full((len(levels), Q, c["B"], Cn, c["T"]), FILL, device=DEV)
    got = eng.recon_quantiles(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], is_post, ns, levels, out, tile)
    assert got is out
    res = out.cpu().numpy()
    assert not (res == FILL).any(), "an output element was not written"
    return res


def _band_outs(Q, B, Cn, T, Lv, ns):
    return [torch.full(shp, FILL, device=DEV) for shp in ((Q, B, Cn, T), (Q, B, Cn, T), (Q, B, Cn, Lv), (Q, B, Cn, Lv), (Q, B, Cn, 2), (Q, B, Cn, ns))]


def _band(eng, flat, c, is_post, levels=BAND_LEVELS, floor=0.0, eps="case", ns=None, obs_d=None, labels=None, null_obs=False):
    """Engine.joint_band on the case's batch -> dict of numpy arrays (crit / joint [Q, B, C, Lv], dev [Q, B, C, K], obs_dev / points
    [Q, B, C]); every output pre-filled with FILL and fully written."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q, Cn = (1 if c["ospec"].gauss else 3), c["obs"].shape[1]
    outs = _band_outs(Q, c["B"], Cn, c["T"], len(levels), ns)
    bt = eng.make_batch(obs_d, labels, e, particles=ns)
    if null_obs:
        bt.obs = None
    eng.joint_band(flat, bt, c["B"], is_post, ns, list(levels), floor, *outs)
    mean, sd, crit, joint, odev, dev = (t.cpu().numpy() for t in outs)
    assert not any((t == FILL).any() for t in (mean, sd, crit, joint, odev, dev)), "an output element was not written"
    return dict(mean=mean, sd=sd, crit=crit, joint=joint, obs_dev=odev[..., 0], points=odev[..., 1], dev=dev)


def _band_check_exact(r, curves, y, levels, floor, tag):
    """Every output of one call against the numpy restatement on the kernel's own curves, the call's own mean and sd: exactly."""
    dev, pts = BU.dev_f32(curves, r["mean"], r["sd"], floor)
    assert _band_same(r["dev"], np.ascontiguousarray(np.moveaxis(dev, 0, -1))), (tag, "dev", np.argwhere(r["dev"] != np.moveaxis(dev, 0, -1))[:4])
    crit, joint = BU.crit_joint(dev, levels)
    assert _band_same(r["crit"], crit), (tag, "crit")
    assert _band_same(r["joint"], joint), (tag, "joint")
    assert np.array_equal(r["points"], pts.astype(np.float32)), (tag, "points")
    if y is not None:
        odev, _ = BU.dev_f32(np.broadcast_to(RU._f32(y), r["mean"].shape)[None], r["mean"], r["sd"], floor)
        assert _band_same(r["obs_dev"], odev[0]), (tag, "obs_dev")
    ranks = BU.level_rule(levels, curves.shape[0])[0]
    for j, rk in enumerate(ranks):                                              # one of the stored deviations, by its rank
        assert np.array_equal(r["crit"][..., j], np.sort(r["dev"], -1)[..., rk - 1]), (tag, j)


def _band_check_oracle(r, v, y, levels, floor, tag, share_at=None):
    """One call's outputs against the oracle's draws v [Q, K, B, C, T] (BU.oracle_dev / BU.dev_bar per head curve).  Returns the worst
    error / bar of the deviations and of the critical values, and the largest near share at the levels of ``levels`` in BU.COUNT_LEVELS."""
    K = v.shape[1]
    ranks, z = BU.level_rule(levels, K)
    worst_dev = worst_crit = worst_obs = near_share = 0.0
    for q in range(v.shape[0]):
        o = BU.oracle_dev(v[q], y, floor)
        on = o["sd"] > floor
        bar = BU.dev_bar(o, on)                                                             # [K, B, C]
        assert np.array_equal(r["points"][q], o["points"].astype(np.float32)), (tag, q, "points")
        got = np.moveaxis(r["dev"][q].astype(np.float64), -1, 0)
        ok = bar > 0
        worst_dev = max(worst_dev, float((np.abs(got - o["dev"])[ok] / bar[ok]).max()) if ok.any() else 0.0)
        assert np.all(np.abs(got - o["dev"]) <= bar), (tag, q, "dev")
        scale = np.maximum(1.0, np.abs(o["mean"]))
        with np.errstate(divide="ignore", invalid="ignore"):                               # (y is exact: one MEAN_BAR, from the mean)
            obar = np.where(on, (RU.MEAN_BAR * scale + o["obs_dev"][..., None] * RU.SD_BAR * scale) / o["sd"], 0.0).max(-1)
        eo = np.abs(r["obs_dev"][q] - o["obs_dev"])
        worst_obs = max(worst_obs, float((eo[obar > 0] / obar[obar > 0]).max()) if (obar > 0).any() else 0.0)
        assert np.all(eo <= obar), (tag, q, "obs_dev")
        srt, cbar = np.sort(o["dev"], 0), bar.max(0)
        for j, (rk, zj) in enumerate(zip(ranks, z)):
            ec = np.abs(r["crit"][q, ..., j] - srt[rk - 1])
            worst_crit = max(worst_crit, float((ec[cbar > 0] / cbar[cbar > 0]).max()) if (cbar > 0).any() else 0.0)
            assert np.all(ec <= cbar), (tag, q, j, "crit")
            counts = np.rint(r["joint"][q, ..., j].astype(np.float64) * K)
            assert np.array_equal(RU._f32(counts) / np.float32(K), r["joint"][q, ..., j]), (tag, "joint is count / K")
            nr = np.abs(o["dev"] - zj) <= bar
            assert np.all(np.abs(counts - (o["dev"] <= zj).sum(0)) <= nr.sum(0)), (tag, q, j, "joint")
            if levels[j] in BU.COUNT_LEVELS:
                near_share = max(near_share, float(nr.mean()))
            if share_at is not None and levels[j] == share_at:
                assert float(nr.mean()) <= BU.NEAR_SHARE and np.all(counts == K), (tag, q, j, float(nr.mean()))
    return worst_dev, worst_crit, worst_obs, near_share


def _summary(eng, flat, c, is_post, thr, sense=1, eps="case", ns=None, sd=True, p=True, obs_d=None, labels=None):
    """Engine.curve_summary on the case's batch -> numpy (mean, sd, p_beyond), None where not asked."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q, Cn = (1 if c["ospec"].gauss else 3), c["obs"].shape[1]
    mean = torch.full((Q, c["B"], Cn, 8), FILL, device=DEV)
    sd_t = torch.full_like(mean, FILL) if sd else None
    pb = torch.full((Q, c["B"], Cn, c["T"]), FILL, device=DEV) if p else None
    eng.curve_summary(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], is_post, ns, None if thr is None else [float(x) for x in thr], sense,
                      mean, sd_t, pb)
    out = tuple(None if t is None else t.cpu().numpy() for t in (mean, sd_t, pb))
    assert all(t is None or not (t == FILL).any() for t in out), "an output element was not written"
    return out


def _cohort_lists(ids, G):
    members, offsets = KU.member_lists(ids, G)
    return torch.from_numpy(members).to(DEV), torch.from_numpy(offsets).to(DEV)


def _calib_invariants(got, ids, G, ns, gauss):
    """0 <= below <= count ns; inside <= count ns; Gauss: below[2] <= below[0] <= below[1] cell by cell, inside == below[1] - below[2],
    cross == 0."""
    below, inside, cross = got[:3]
    cap = torch.tensor([int((np.asarray(ids) == g).sum()) * ns for g in range(G)], dtype=torch.int32, device=DEV).view(G, 1, 1)
    assert bool((below >= 0).all()) and bool((below <= cap).all())
    if inside is not None:
        assert bool((inside >= 0).all()) and bool((inside <= cap).all()) and bool((inside <= below[1]).all())
    if cross is not None:
        assert bool((cross >= 0).all()) and bool((cross <= cap).all())
    if gauss:
        assert bool((below[2] <= below[0]).all()) and bool((below[0] <= below[1]).all())
        assert inside is None or torch.equal(inside, below[1] - below[2])
        assert cross is None or int(cross.abs().max()) == 0


def _calib(eng, flat, c, is_post, ids, G, chunk=3, eps="case", ns=None, outputs=CALIB_ALL, obs_d=None, labels=None, scratch=None, gauss=None):
    """(below, inside, cross, pinball, width); the outputs asked for pre-filled with -1 / NaN: every element must be written."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    C, T = c["obs"].shape[1], c["T"]
    out = dict(below=torch.full((3, G, C, T), -1, dtype=torch.int32, device=DEV))
    for name, shp, fill in (("inside", (G, C, T), -1), ("cross", (G, C, T), -1), ("pinball", (3, G, C), None), ("width", (G, C), None)):
        if name in outputs:
            out[name] = torch.full(shp, -1, dtype=torch.int32, device=DEV) if fill is not None else torch.full(shp, float("nan"), device=DEV)
    members, offsets = _cohort_lists(ids, G)
    got = eng.calibration(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], is_post, ns, members, offsets, G, chunk=chunk,
                          outputs=outputs, scratch=scratch, **out)
    _calib_invariants(got, ids, G, ns, c["ospec"].gauss if gauss is None else gauss)       # (gauss=False: NaN curves break the Gauss ordering)
    return got


def _calib_own_curves(eng, flat, c, is_post, eps, obs_d, labels):
    """[3, K, B, C, T] fp32: the kernels' own value of every curve of every draw -- K recon_moments calls with num_samples = 1 (mean = the
    draw); Gauss: mean + / - 2 s in fp32 with s the decode kernel's softplus(constant_std)."""
    heads = np.stack([_recon_moments(eng, flat, c, is_post, eps=eps[k].contiguous(), obs_d=obs_d, labels=labels, ns=1)[0].cpu().numpy() for k in range(eps.shape[0])], 1)
    if not c["ospec"].gauss:
        return heads                                                                       # [Q = 3, K, B, C, T]
    s = eng.decode_heads(flat, torch.zeros(1, c["T"], c["S"], device=DEV))[1].cpu().numpy()
    w = np.float32(2.0) * s
    return np.stack([heads[0], heads[0] + w, heads[0] - w]).astype(np.float32)


def _attr(eng, flat, c, is_post, masks, eps="case", obs_d=None, labels=None, ns=None):
    """Engine.latent_attribution on the case's batch; outputs pre-filled with NaN: every element must be written."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = c["eps2"].to(DEV).contiguous() if isinstance(eps, str) else eps
    Q, B, L = 1 if c["ospec"].gauss else 3, c["B"], c["ospec"].latent_dim
    mean = torch.full((Q, B, c["obs"].shape[1], c["T"]), float("nan"), device=DEV)
    sd = torch.full_like(mean, float("nan"))
    msd = torch.full((len(masks),) + tuple(mean.shape), float("nan"), device=DEV)
    bt = eng.make_batch(obs_d, labels, e, particles=ns, eps_shape=None if e is None else (2, ns, B, L))
    return eng.latent_attribution(flat, bt, B, is_post, ns, masks, mean, sd, msd)


def _mech(eng, flat, c, is_post, slots=MU.ALL, eps="case", ns=None, sd=True, obs_d=None, labels=None):
    """Engine.mechanism_moments on the case's batch -> numpy (mean, sd) [n_sel, B, S, T]; sd None where not asked.  The outputs lie in
    one buffer each, pre-filled, with MECH_NG guard words on either side."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    shp = (bin(slots).count("1"), c["B"], c["S"], c["T"])
    n = int(np.prod(shp))
    bufs = [torch.full((n + 2 * MECH_NG,), MECH_GUARD, device=DEV) for _ in range(2 if sd else 1)]
    outs = [b[MECH_NG:MECH_NG + n].view(shp) for b in bufs]
    for o in outs:
        o.fill_(FILL)
    got = eng.mechanism_moments(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], is_post, ns, slots, outs[0], outs[1] if sd else False)
    assert got[0] is outs[0] and (got[1] is outs[1] if sd else got[1] is None)
    for b in bufs:
        h = b.cpu().numpy()
        assert np.all(h[:MECH_NG] == MECH_GUARD) and np.all(h[MECH_NG + n:] == MECH_GUARD), "a guard word was written"
        assert not (h[MECH_NG:MECH_NG + n] == FILL).any(), "an output element was not written"
    return outs[0].cpu().numpy(), (outs[1].cpu().numpy() if sd else None)


def _label_split(c, u):
    """A [B, n_u] label matrix as the family's label tensors, one by one, on the device."""
    out, o = [], 0
    for w in WIDTHS[c["fam"]]:
        out.append(u[:, o:o + w].contiguous().to(DEV))
        o += w
    return out


def _iv(eng, flat, c, mask, u_cf, eps="case", obs_d=None, labels=None, ns=None):
    """Outputs pre-filled with NaN: every element must be written."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q = 1 if c["ospec"].gauss else 3
    outs = [torch.full((Q, c["B"], c["obs"].shape[1], c["T"]), float("nan"), device=DEV) for _ in range(4)]
    cf = None if u_cf is None else _label_split(c, u_cf)
    return eng.intervene_moments(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], cf, mask, ns, *outs)


def _cohort(eng, flat, c, is_post, ids, G, chunk=3, eps="case", ns=None, clip=None, outputs=COHORT_ALL, obs_d=None, labels=None, scratch=None):
    """(mean, sd, sd_subjects, obs_mean, l1); every output asked for is pre-filled with NaN: every element must be written."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q, C, T = 1 if c["ospec"].gauss else 3, c["obs"].shape[1], c["T"]
    nan = lambda *shp: torch.full(shp, float("nan"), device=DEV)
    out = dict(mean=nan(Q, G, C, T))
    for name, shp in (("sd", (Q, G, C, T)), ("sd_subjects", (Q, G, C, T)), ("obs_mean", (G, C, T)), ("l1", (G, C))):
        if name in outputs:
            out[name] = nan(*shp)
    members, offsets = _cohort_lists(ids, G)
    return eng.cohort_moments(flat, eng.make_batch(obs_d, labels, e, particles=ns), c["B"], is_post, ns, members, offsets, G, chunk=chunk,
                              clip_min=clip, outputs=outputs, scratch=scratch, **out)


def _cohort_ids(mode, B, seed=2):
    """(ids, G): "three": three cohorts and a tenth of the trajectories in none, interleaved; "one": G = 1; "singletons": G = B;
    "none": M = 0 with G = 2."""
    if mode == "one":
        return np.zeros(B, np.int64), 1
    if mode == "singletons":
        return np.arange(B), B
    if mode == "none":
        return np.full(B, -1), 2
    r = np.random.RandomState(seed)
    return r.choice([-1, 0, 1, 2], size=B, p=[0.1, 0.5, 0.3, 0.1]), 3


def _cohort_per_draw(eng, flat, c, is_post, eps, obs_d, labels):
    """[B, K, Q, C, T] fp32: the kernel's own value of every draw -- K calls with num_samples = 1 and singleton cohorts (mean = the draw)."""
    B = c["B"]
    ids, G = _cohort_ids("singletons", B)
    vals = [_cohort(eng, flat, c, is_post, ids, G, chunk=1, eps=eps[k].contiguous(), ns=1, outputs=(), obs_d=obs_d, labels=labels)[0].cpu().numpy()
            for k in range(eps.shape[0])]
    return np.stack(vals).transpose(2, 0, 1, 3, 4)                                        # [K, Q, B, C, T] -> [B, K, Q, C, T]


def _cohort_truth(vals, ids, G, R):
    """Per cohort: fp64 (mean, sd, sd_subjects) of the per-draw values, D of the chunking, stacked [Q, G, C, T] (NaN: empty)."""
    out = [np.full((vals.shape[2], G) + vals.shape[3:], np.nan) for _ in range(4)]
    for g in range(G):
        sel = np.flatnonzero(ids == g)
        if sel.size:
            v = vals[sel].astype(np.float64)
            for o, x in zip(out, CU.moments64(v) + (CU.chunk_spread(v, R),)):
                o[:, g] = x
    return out


def _forecast(eng, flat, c, is_post, window=0, eps="case", states=True, sd=True, x_mean=True, x_sd=True, times_out=None, ns=None, obs_d=None, labels=None):
    """(mean, sd, x_mean, x_sd), NaN-prefilled; an output switched off is passed as NULL and comes back as None."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    t_out = c["times_out"] if times_out is None else times_out
    Q, B, T_out = 1 if c["ospec"].gauss else 3, c["B"], t_out.numel()
    mean = torch.full((Q, B, c["obs"].shape[1], T_out), NAN, device=DEV)
    outs = [mean, torch.full_like(mean, NAN) if sd else None,
            torch.full((B, c["S"], T_out), NAN, device=DEV) if states and x_mean else None,
            torch.full((B, c["S"], T_out), NAN, device=DEV) if states and x_sd else None]
    tt, st = eng.forecast_grid(t_out)
    bt = eng.make_batch(obs_d, labels, e, particles=ns)
    ws = eng.workspace(B)
    eng._guard(flat, ws)
    from structured_latent_odes_amd.engine import _check
    _check(eng.lib, eng.handle, eng.lib.slode_forecast_moments(
        eng.handle, C.byref(eng.shape(B)), C.byref(eng.layout), eng._p(flat), eng._p(eng._times), eng._p(eng._stage_t), C.byref(bt), 1 if is_post else 0, ns, eng._p(tt), eng._p(st),
        T_out, int(window), *(eng._p(t) for t in outs), eng._p(ws), ws.numel() * 4, eng._stream()))
    return tuple(outs)
