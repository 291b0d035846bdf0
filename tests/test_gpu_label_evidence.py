"""GPU tests of the label evidence (slode_label_evidence / Engine.label_evidence / MechanisticBase.label_evidence / save_label_evidence /
--label-evidence): bitwise against Engine.traj_bounds on the substituted labels, against the per-row fp64 oracle, and against the fp64
recomputation from the kernel's own per-draw losses.  Bars: module docstrings of tests/label_evidence_util.py and tests/traj_bounds_util.py.
Outputs are pre-filled with NaN: every element must be written."""
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import label_evidence_util as LU
from tests import traj_bounds_util as TU
from tests.eval_gpu_util import ADAPTIVE, _captured, _device_batch, _engine, _model, _padded, _refused

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _eps(c, eps, K):
    e = c["eps"] if isinstance(eps, str) else eps
    if e is not None:
        e = (e[0] if K == 1 and e.dim() == 3 else e).to(DEV).contiguous()               # one draw: [B, L], as make_batch takes it
    return e


def _evidence(eng, flat, c, tabs, eps="case", K=None, log_prior=None, obs_d=None, labels=None):
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    K = c["K"] if K is None else K
    V = next(t for t in tabs if t is not None).shape[0]
    ev = torch.full((c["B"], V, 4), float("nan"), device=DEV)
    best = torch.full((c["B"],), -7, dtype=torch.int32, device=DEV)
    loss = torch.full((V, max(K, 0), c["B"]), float("nan"), device=DEV)
    hyp = [None if t is None else t.to(DEV).contiguous() for t in tabs]
    lp = None if log_prior is None else torch.as_tensor(log_prior, dtype=torch.float32).to(DEV)
    eng.label_evidence(flat, eng.make_batch(obs_d, labels, _eps(c, eps, K), particles=max(K, 1)), c["B"], K, hyp, V, lp, ev, best, loss)
    return ev, best, loss


def _bounds_of(eng, flat, c, tabs, v, eps="case", K=None):
    """Engine.traj_bounds on the batch with its labels replaced by hypothesis v."""
    c2 = dict(c, u=LU.substituted(c, tabs, v))
    obs_d, labels = _device_batch(c2)
    K = c["K"] if K is None else K
    bounds = torch.full((c["B"], 4), float("nan"), device=DEV)
    loss = torch.full((K, c["B"]), float("nan"), device=DEV)
    eng.traj_bounds(flat, eng.make_batch(obs_d, labels, _eps(c, eps, K), particles=K), c["B"], K, bounds, loss)
    return bounds, loss


def _check_own_reduction(ev, best, loss, tag, log_prior=None):
    """Slot 3 and best against the fp64 recomputation from the kernel's own loss_vkb; logsumexp_v(slot 3) = 0; best is an arg-max."""
    e, l = ev.double().cpu().numpy(), loss.double().cpu().numpy()
    _, _, _, post, _ = LU.reduce64(l, log_prior)
    r = np.abs(e[:, :, 3] - post) / LU.post_bar(post)
    m = e[:, :, 3].max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(e[:, :, 3] - m).sum(axis=1, keepdims=True)))[:, 0]
    print("%s: slot 3 error / bar %.3e, |logsumexp| max %.3e" % (tag, r.max(), np.abs(lse).max()))
    assert np.isfinite(e).all() and np.isfinite(l).all(), tag
    assert r.max() <= 1.0, (tag, "slot 3", r.max())
    assert np.all(np.abs(lse) <= LU.post_bar(m[:, 0])), (tag, "logsumexp", lse)
    b = best.cpu().numpy()
    assert np.all((b >= 0) & (b < e.shape[1])), (tag, b)
    assert np.array_equal(ev[:, :, 3].cpu().numpy()[np.arange(len(b)), b], ev[:, :, 3].max(dim=1).values.cpu().numpy()), (tag, "best")


@pytest.mark.parametrize("V,K", [(1, 1), (2, 7), (5, 3), (64, 2)])
@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald", "challenge_gauss"])
def test_columns_are_bitwise_the_bounds_of_the_substituted_labels(case, V, K):
    """L = 8, L = 50 with the label phase, T = 300; V = 5 is no multiple of the four waves, V = 64 the cap.  Explicit noise.  V = 1: the
    hypothesis is the labels of trajectory 0 as a shared row; slot 3 is exactly 0 and best is 0."""
    c = TU.build(case, "rk4", B=3, K=K)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    tabs = [c["u"][:1, lo:hi].contiguous().clone() for lo, hi in LU.offsets(c["fam"])] if V == 1 else LU.seeded(c, V)
    ev, best, loss = _evidence(eng, flat, c, tabs)
    assert torch.isfinite(ev).all() and torch.isfinite(loss).all()
    for v in range(V):
        bounds, loss_kb = _bounds_of(eng, flat, c, tabs, v)
        assert torch.equal(ev[:, v, :3], bounds[:, :3]), (case, V, K, v, "slots 0-2")
        assert torch.equal(loss[v], loss_kb), (case, V, K, v, "loss_vkb")
    _check_own_reduction(ev, best, loss, "%s V=%d K=%d" % (case, V, K))
    if V == 1:
        assert torch.equal(ev[:, 0, 3], torch.zeros(c["B"], device=DEV)) and torch.equal(best, torch.zeros_like(best))


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", ["cvs_ald", "challenge_ald", "proc_gauss"])
def test_losses_and_bounds_match_the_fp64_oracle(case, solver):
    """Independent of traj_bounds_kernel: loss_vkb and slots 0 / 1 against TU.oracle_rows with u replaced, one case per family x solver,
    V = 3, K = 4, at the bars of tests/traj_bounds_util.py."""
    c = TU.build(case, solver, B=4, K=4)
    eng = _engine(c)
    tabs = LU.seeded(c, 3)
    ev, best, loss = _evidence(eng, eng.pack(c["p"]), c, tabs)
    want = LU.oracle(c, tabs)
    e, l = ev.double().cpu().numpy(), loss.double().cpu().numpy()
    bar = TU.REL * want["mag"]
    elbo, iw, _, _, _ = LU.reduce64(want["loss"])
    rl = np.abs(l - want["loss"]) / bar
    r0 = np.abs(e[:, :, 0] - elbo) / bar.mean(1).T
    r1 = np.abs(e[:, :, 1] - iw) / bar.max(1).T
    print("%s/%s: error / bar: loss_vkb %.3f, slot 0 %.3f, slot 1 %.3f" % (case, solver, rl.max(), r0.max(), r1.max()))
    assert np.isfinite(e).all() and np.isfinite(l).all()
    assert rl.max() <= 1.0 and r0.max() <= 1.0 and r1.max() <= 1.0, (case, solver, rl.max(), r0.max(), r1.max())
    _check_own_reduction(ev, best, loss, "%s/%s" % (case, solver))


@pytest.mark.parametrize("prior", [None, "skewed"])
def test_posterior_on_non_degenerate_weights(prior):
    """cvs_ald, {0, 1}^2, B = 6, K = 8, noise x 1e-3 (tests/test_label_evidence_cpu.py: posteriors between 0.03 and 0.67): slot 3 against
    the fp64 recomputation, logsumexp_v(slot 3) = 0, best an arg-max -- with a uniform and with a non-uniform log_prior; 1 <= ESS <= K and
    slots 1 / 2 at the tight bars of the own reduction; at least two hypotheses per row above 0.03."""
    c = TU.build("cvs_ald", "rk4", B=6, K=8)
    eng = _engine(c)
    tabs = LU.binary_grid(c)
    lp = None if prior is None else np.log(np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32))
    ev, best, loss = _evidence(eng, eng.pack(c["p"]), c, tabs, eps=1e-3 * c["eps"], log_prior=lp)
    _check_own_reduction(ev, best, loss, "cvs_ald noise x 1e-3, prior %s" % prior, lp)
    for v in range(4):
        TU.check_reduction(torch.cat([ev[:, v, :3], ev[:, v, :1]], dim=1), loss[v], "column %d" % v)
    ess = ev[:, :, 2].cpu().numpy()
    assert np.all(ess >= 1.0) and np.all(ess <= 8.0) and np.sum((ess > 1.5) & (ess < 7.5)) >= 6, ess
    if prior is None:
        assert np.all((np.exp(ev[:, :, 3].double().cpu().numpy()) > 0.03).sum(axis=1) >= 2)


def test_one_hot_posterior_stays_finite():
    """proc_gauss, the first four label rows as hypotheses: bounds more than 1000 nat apart -- log_post finite, its maximum exactly 0."""
    c = TU.build("proc_gauss", "rk4", B=6, K=8)
    eng = _engine(c)
    ev, best, loss = _evidence(eng, eng.pack(c["p"]), c, LU.batch_rows(c), eps=1e-3 * c["eps"])
    _check_own_reduction(ev, best, loss, "proc_gauss one-hot")
    assert torch.equal(ev[:, :, 3].max(dim=1).values, torch.zeros(6, device=DEV)) and int(best[0]) == 0
    assert float((ev[:, :, 1].max(dim=1).values - ev[:, :, 1].min(dim=1).values).min()) > 1000.0


SIZES = [("cvs_gauss", 3, 2, 5, {}, None), ("cvs_gauss", 65, 2, 3, {}, None), ("proc_gauss", 9, 2, 5, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}, None),
         ("cvs_ald", 9, 3, 6, {"SLODE_ODE_GENERIC": "1"}, None),
         ("proc_ald", 9, 2, 5, {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}, None),
         ("proc_ald", 3, 2, 4, {}, (0,))]


@pytest.mark.parametrize("case,B,K,V,env,only", SIZES, ids=["%s-B%d-K%d-V%d%s%s" % (c, B, K, V, "-" + "-".join(k[10:].lower() for k in e) if e else "",
                                                                                      "-aR-alone" if o else "") for c, B, K, V, e, o in SIZES])
def test_sizes_and_instantiations(case, B, K, V, env, only, monkeypatch):
    """B in {3, 9, 65}, the persistent loop (9 trajectories on 2 workgroups), the run-time-S instantiation with and without the label phase,
    a partly-NULL hyp_labels (proc with aR alone hypothesised), NaN-poisoned workspace: against the oracle, bitwise against traj_bounds
    on two columns, and the own reduction."""
    c = TU.build(case, "rk4", B=B, K=K)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    tabs = LU.seeded(c, V, only)
    eng.workspace(B).fill_(float("nan"))
    ev, best, loss = _evidence(eng, flat, c, tabs)
    tag = "%s B=%d K=%d V=%d %s" % (case, B, K, V, env)
    rows = slice(0, min(B, 9))
    want = LU.oracle(c, tabs, rows=rows)
    rl = np.abs(loss.double().cpu().numpy()[:, :, rows] - want["loss"]) / (TU.REL * want["mag"])
    print("%s: loss_vkb error / bar %.3f" % (tag, rl.max()))
    assert rl.max() <= 1.0, (tag, rl.max())
    _check_own_reduction(ev, best, loss, tag)
    for v in (0, V - 1):
        bounds, loss_kb = _bounds_of(eng, flat, c, tabs, v)
        assert torch.equal(ev[:, v, :3], bounds[:, :3]) and torch.equal(loss[v], loss_kb), (tag, v)


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_bitwise_reproducible_and_independent_of_the_grid_and_of_where_the_noise_is_drawn(case, monkeypatch):
    """Two calls: bitwise equal.  One workgroup per trajectory against a 3-workgroup loop: bitwise equal.  In-kernel noise of drawing calls
    n .. n + 4 against the rows rng_normal(n + k, B) passed explicitly: bitwise equal; the counter goes n -> n + 5 and stays for explicit
    noise."""
    c = TU.build(case, "midpoint", B=7, K=5)
    tabs = LU.seeded(c, 6)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    a, b, l = _evidence(eng, flat, c, tabs), _evidence(eng, flat, c, tabs), _evidence(loop, flat, c, tabs)
    for x, y, z in zip(a, b, l):
        assert torch.equal(x, y) and torch.equal(x, z)
    for e in (eng, loop):
        e.rng_seed(77, first_trajectory=1000)
        e.rng_set_counter(5)
    drawn = _evidence(eng, flat, c, tabs, eps=None)
    assert eng.rng_state() == (77, 1000, 10)
    rows = torch.stack([eng.rng_normal(5 + k, c["B"]) for k in range(5)]).contiguous()
    given = _evidence(eng, flat, c, tabs, eps=rows)
    assert eng.rng_state() == (77, 1000, 10)                                             # explicit noise draws nothing
    drawn_loop = _evidence(loop, flat, c, tabs, eps=None)
    assert loop.rng_state() == (77, 1000, 10)
    for x, y, z in zip(drawn, given, drawn_loop):
        assert torch.isfinite(x.float()).all() and torch.equal(x, y) and torch.equal(x, z)


def test_refusals_by_name(monkeypatch):
    """Every refusal names its reason, draws nothing, launches nothing and writes nothing (rng_state, profile_read, outputs untouched)."""
    c = TU.build("cvs_ald", "rk4", B=4, K=2)
    obs_d, labels = _device_batch(c)
    grid = [t.to(DEV) for t in LU.binary_grid(c)]

    def refused(eng, match, obs=obs_d, K=2, V=4, hyp=grid, particles=1):
        flat = eng.pack(c["p"])
        ev = torch.full((c["B"], max(V, 1), 4), float("nan"), device=DEV)
        best = torch.full((c["B"],), -7, dtype=torch.int32, device=DEV)
        loss = torch.full((max(V, 1), K, c["B"]), float("nan"), device=DEV)
        bt = eng.make_batch(obs, labels, None)
        ws = eng.workspace(c["B"], particles)
        _refused(eng, lambda: eng._batch_call(eng.lib.slode_label_evidence, flat, bt, c["B"], particles, K, _ptrs(hyp), V, None, eng._p(ev),
                                              eng._p(best), eng._p(loss)), match)
        torch.cuda.synchronize(DEV)
        assert torch.isnan(ev).all() and torch.isnan(loss).all() and torch.equal(best, torch.full_like(best, -7)) and ws is not None

    def _ptrs(hyp):
        import ctypes as C
        from structured_latent_odes_amd import _lib as L
        if hyp is None:
            return None
        p = (C.c_void_p * L.MAX_LABELS)()
        for i, t in enumerate(hyp):
            if t is not None:
                p[i] = t.data_ptr()
        return p

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s" % solver)
    eng = _engine(c, monkeypatch)
    refused(eng, "particles = 2", particles=2)
    refused(eng, "num_draws = 0", K=0)
    refused(eng, "observation strides", obs=_padded(obs_d))
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    eng = _engine(c, monkeypatch)
    refused(eng, "V = 0 out of range", V=0)
    refused(eng, "V = 65 out of range", V=65)
    refused(eng, "hyp_labels is NULL", hyp=None)
    refused(eng, "every entry of hyp_labels is NULL", hyp=[None, None])
    refused(eng, "LDS tables.*num_draws = 2000, V = 64", K=2000, V=64)                    # 128,000 losses: 512 KB


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_call_and_its_files(fam, tmp_path):
    """label_evidence(num_draws=3, return_draws=True) on the family's default hypotheses: the dict's keys and shapes, bitwise equal to
    Engine.label_evidence from the same generator state; match against the labels; save_label_evidence's files."""
    m, batch = _model(fam)
    eng = m._bind().engine
    B = batch["observations"].shape[0]
    hyp = m.default_hypotheses(**{l: batch[l] for l in m.LABELS})
    V = next(iter(hyp.values())).shape[0]
    assert V == (12 if fam == "proc" else 4) and list(hyp) == list(m.LABELS[:2])
    eng.rng_seed(4321, first_trajectory=300)
    eng.rng_set_counter(9)
    res = m.label_evidence(num_draws=3, hypotheses=hyp, return_draws=True, **batch)
    assert eng.rng_state() == (4321, 300, 12)
    assert set(res) == {"elbo", "iw_bound", "ess", "log_post", "best", "match", "loss"}
    assert all(tuple(res[n].shape) == (B, V) for n in ("elbo", "iw_bound", "ess", "log_post"))
    assert tuple(res["best"].shape) == tuple(res["match"].shape) == (B,) and tuple(res["loss"].shape) == (V, 3, B)
    assert "loss" not in m.label_evidence(num_draws=2, hypotheses=hyp, **batch)
    eng.rng_set_counter(9)
    labs = [batch[l].reshape(B, -1).to(torch.float32).contiguous() for l in m.LABELS]
    tabs = [hyp[l].to(DEV) if l in hyp else None for l in m.LABELS]
    ev, best, loss = eng.label_evidence(m._bind().flat, eng.make_batch(batch["observations"], labs, None, particles=3), B, 3, tabs, V)
    assert torch.isfinite(ev).all() and torch.equal(loss, res["loss"]) and torch.equal(best, res["best"])
    for i, n in enumerate(("elbo", "iw_bound", "ess", "log_post")):
        assert torch.equal(ev[:, :, i], res[n])
    _check_own_reduction(ev, best, loss, fam + " model")
    match = res["match"].cpu().numpy()
    for b in range(B):                                                                   # the synthetic labels are binary / one-hot
        assert match[b] >= 0 and all(torch.equal(hyp[l][match[b]].to(DEV), labs[i][b]) for i, l in enumerate(m.LABELS) if l in hyp)
    eng.rng_set_counter(9)
    paths = m.save_label_evidence(str(tmp_path / "res"), [batch, batch], 3, hyp)
    assert [os.path.basename(p) for p in paths] == ["evidence_post.npy", "evidence_best.npy", "evidence_match.npy"] + [
        "evidence_hypotheses_%s.npy" % l for l in m.LABELS[:2]]
    table, tb, tm = (np.load(p) for p in paths[:3])
    assert table.shape == (2 * B, V, 4) and table.dtype == np.float32 and np.array_equal(table[:B], ev.cpu().numpy()) and np.isfinite(table).all()
    assert tb.shape == tm.shape == (2 * B,) and np.array_equal(tb[:B], best.cpu().numpy()) and np.array_equal(tm[:B], match)
    assert all(np.array_equal(np.load(p), hyp[l].numpy()) for p, l in zip(paths[3:], m.LABELS[:2]))


def test_training_entry_point_with_label_evidence(tmp_path, monkeypatch, capsys):
    """One --label-evidence 4 run of training.main on a synthetic loader, one epoch: the files beside the run's others, and the line."""
    import re
    from structured_latent_odes_amd import training as T
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.models.mechanistic_cvs_Gauss import MechanisticModelGauss

    def load_config():
        cfg = EU.model_config("cvs")
        cfg.update(mini_batch_size=16, seq_len=86)
        return cfg

    monkeypatch.chdir(tmp_path)
    T.main("cvs", load_config, MechanisticModel, MechanisticModelGauss, ["--epochs", "1", "--batches-per-epoch", "1", "--label-evidence", "4"])
    out = capsys.readouterr().out
    assert "FINAL TEST:" in out
    m = re.search(r"^label_evidence: V=4  matched=(\d+)/16  best==match=([0-9.]+)  mean_post_at_match=([0-9.]+)  median_ess_at_match=([0-9.]+)$", out, re.M)
    assert m and int(m.group(1)) == 16 and 0.0 <= float(m.group(2)) <= 1.0 and 0.0 <= float(m.group(3)) <= 1.0 and 1.0 <= float(m.group(4)) <= 4.0
    res = tmp_path / ("results_%s" % load_config().model)
    table = np.load(str(res / "evidence_post.npy"))
    assert table.shape == (16, 4, 4) and table.dtype == np.float32 and np.isfinite(table).all()
    assert np.all(table[:, :, 2] >= 1.0) and np.all(table[:, :, 2] <= 4.0)
    assert np.allclose(np.exp(table[:, :, 3].astype(np.float64)).sum(axis=1), 1.0, atol=1e-5)
    assert np.load(str(res / "evidence_best.npy")).shape == np.load(str(res / "evidence_match.npy")).shape == (16,)
    assert np.load(str(res / "evidence_hypotheses_iext.npy")).shape == np.load(str(res / "evidence_hypotheses_rtpr.npy")).shape == (4, 1)


def test_launches_and_graph_capture():
    """Three launches, "weff", "enc_fwd2", "label_evidence", on one stream (a linear graph: no parallel branches).  One capture and one
    replay of a call with explicit noise equal the stream-launched call bitwise."""
    c = TU.build("cvs_ald", "rk4", B=5, K=3)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    tabs = LU.binary_grid(c)
    eng.profile_enable(True)
    _evidence(eng, flat, c, tabs, obs_d=obs_d, labels=labels)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "label_evidence"]
    eng.profile_enable(False)
    ev = torch.zeros(c["B"], 4, 4, device=DEV)
    best = torch.zeros(c["B"], dtype=torch.int32, device=DEV)
    loss = torch.zeros(4, 3, c["B"], device=DEV)
    hyp = [t.to(DEV) for t in tabs]
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=3)
    want = _captured(lambda: eng.label_evidence(flat, bt, c["B"], 3, hyp, 4, None, ev, best, loss), (ev, loss))
    assert torch.equal(ev, want[0]) and torch.equal(loss, want[1]) and want[0].abs().sum().item() > 0.0
