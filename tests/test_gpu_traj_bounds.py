"""GPU tests of the per-trajectory bounds (slode_traj_bounds / Engine.traj_bounds / MechanisticBase.trajectory_bounds /
save_trajectory_bounds / --test-bounds) against the per-row fp64 oracle and against the fp64 reduction of the kernel's own per-draw losses.
Bars: module docstring of tests/traj_bounds_util.py.  Outputs are pre-filled with NaN: every element must be written."""
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import traj_bounds_util as TU
from tests.eval_gpu_util import ADAPTIVE, _captured, _device_batch, _engine, _model, _padded, _refused

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bounds(eng, flat, c, eps="case", K=None, obs_d=None, labels=None, particles=1):
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    K = c["K"] if K is None else K
    e = c["eps"] if isinstance(eps, str) else eps
    if e is not None:
        e = (e[0] if K == 1 and e.dim() == 3 else e).to(DEV).contiguous()               # one draw: [B, L], as make_batch takes it
    bounds = torch.full((c["B"], 4), float("nan"), device=DEV)
    loss = torch.full((max(K, 0), c["B"]), float("nan"), device=DEV)
    eng.traj_bounds(flat, eng.make_batch(obs_d, labels, e, particles=max(K, 1)), c["B"], K, bounds, loss, particles=particles)
    return bounds, loss


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_per_draw_losses_and_slots_match_the_fp64_oracle(case, solver):
    """Explicit noise, K = 4; six model classes x three fixed-grid solvers; cvs / challenge in the [B,T,C] layout, proc in [B,C,T]."""
    c = TU.build(case, solver, K=4)
    eng = _engine(c)
    bounds, loss = _bounds(eng, eng.pack(c["p"]), c)
    tag = "%s/%s" % (case, solver)
    TU.check_oracle(bounds, loss, TU.oracle_rows(c), tag)
    TU.check_reduction(bounds, loss, tag)


SIZES = [("cvs_gauss", 63, 2, {}), ("cvs_gauss", 65, 2, {}), ("cvs_gauss", 257, 2, {}), ("cvs_ald", 3, 200, {}), ("challenge_gauss", 2, 64, {}),
         ("proc_gauss", 65, 2, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}), ("cvs_ald", 9, 7, {"SLODE_ODE_GENERIC": "1"}),
         ("proc_ald", 9, 2, {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}), ("cvs_gauss", 5, 1, {})]


@pytest.mark.parametrize("case,B,K,env", SIZES, ids=["%s-B%d-K%d%s" % (c, B, K, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, K, e in SIZES])
def test_sizes_and_instantiations(case, B, K, env, monkeypatch):
    """B on both sides of the 64- and 256-thread edges, the persistent loop (65 and 9 trajectories on 5 and 2 workgroups), the run-time-S
    instantiation with and without the label phase, K in {1, 2, 7, 64, 200} (T = 200 and T = 300), rk4, NaN-poisoned workspace.  K = 1: the
    importance-weighted bound IS the -ELBO, bitwise, and the ESS is exactly 1."""
    c = TU.build(case, "rk4", B=B, K=K)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    bounds, loss = _bounds(eng, flat, c)
    tag = "%s B=%d K=%d %s" % (case, B, K, env)
    TU.check_oracle(bounds, loss, TU.oracle_rows(c), tag)
    TU.check_reduction(bounds, loss, tag)
    if K == 1:
        assert torch.equal(bounds[:, 1], bounds[:, 0]) and torch.equal(bounds[:, 0], loss[0])
        assert torch.equal(bounds[:, 2], torch.ones(B, device=DEV))


@pytest.mark.parametrize("case", ["cvs_ald", "challenge_gauss"])
def test_reduction_on_non_degenerate_weights(case):
    """Noise x 1e-3, K = 8 (tests/test_traj_bounds_cpu.py: ESS between 1.1 and 4.8 on the oracle): slots 1 and 2 against the fp64 reduction
    of the kernel's own loss_kb at the tight bars, 1 <= ESS <= K, slot 1 <= slot 0 + 2^-22 |slot 0|."""
    c = TU.build(case, "rk4", K=8)
    eng = _engine(c)
    bounds, loss = _bounds(eng, eng.pack(c["p"]), c, eps=1e-3 * c["eps"])
    TU.check_reduction(bounds, loss, case + " noise x 1e-3")
    ess = bounds[:, 2].cpu().numpy()
    assert np.sum((ess > 1.5) & (ess < 7.5)) >= 3, ess                                   # the case exercises the reduction


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_sum_of_the_elbo_slot_is_the_training_side_loss(case):
    """The in-order fp64 sum over b of slot 0 equals Engine.svi_step(SVI_MAIN, grads=None, particles=K) on the same [K, B, L] noise, to
    1e-5 relative (K = 3)."""
    from structured_latent_odes_amd import _lib as L
    c = TU.build(case, "rk4", K=3)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    bounds, _ = _bounds(eng, flat, c, obs_d=obs_d, labels=labels)
    out = torch.full((1,), float("nan"), device=DEV)
    eng.svi_step(L.SVI_MAIN, flat, eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=3), c["B"], out, None, particles=3)
    got = 0.0
    for v in bounds[:, 0].double().cpu().tolist():
        got += v
    want = float(out.item())
    print("%s: sum of slot 0 %.6f, svi_step %.6f, relative %.2e" % (case, got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_bitwise_reproducible_and_independent_of_the_grid_and_of_where_the_noise_is_drawn(case, monkeypatch):
    """Two calls: bitwise equal.  One workgroup per trajectory against a 3-workgroup loop: bitwise equal.  In-kernel noise of drawing calls
    n .. n + 6 against the rows rng_normal(n + k, B) passed explicitly: bitwise equal; the counter goes n -> n + 7 and stays for explicit
    noise."""
    c = TU.build(case, "midpoint", K=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    a, b, l = _bounds(eng, flat, c), _bounds(eng, flat, c), _bounds(loop, flat, c)
    for x, y, z in zip(a, b, l):
        assert torch.equal(x, y) and torch.equal(x, z)
    for e in (eng, loop):
        e.rng_seed(77, first_trajectory=1000)
        e.rng_set_counter(5)
    drawn = _bounds(eng, flat, c, eps=None)
    assert eng.rng_state() == (77, 1000, 12)
    rows = torch.stack([eng.rng_normal(5 + k, c["B"]) for k in range(7)]).contiguous()
    given = _bounds(eng, flat, c, eps=rows)
    assert eng.rng_state() == (77, 1000, 12)                                             # explicit noise draws nothing
    drawn_loop = _bounds(loop, flat, c, eps=None)
    assert loop.rng_state() == (77, 1000, 12)
    for x, y, z in zip(drawn, given, drawn_loop):
        assert torch.isfinite(x).all() and torch.equal(x, y) and torch.equal(x, z)


def test_refusals_by_name(monkeypatch):
    """Every refusal names its reason, draws nothing, launches nothing and writes nothing (rng_state, profile_read, outputs still NaN)."""
    c = TU.build("cvs_ald", "rk4", K=2)
    obs_d, labels = _device_batch(c)

    def refused(eng, match, obs=obs_d, K=2, particles=1):
        flat = eng.pack(c["p"])
        bounds = torch.full((c["B"], 4), float("nan"), device=DEV)
        loss = torch.full((K, c["B"]), float("nan"), device=DEV)
        _refused(eng, lambda: eng.traj_bounds(flat, eng.make_batch(obs, labels, None), c["B"], K, bounds, loss, particles=particles), match)
        torch.cuda.synchronize(DEV)
        assert torch.isnan(bounds).all() and torch.isnan(loss).all()

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s" % solver)
    eng = _engine(c, monkeypatch)
    refused(eng, "particles = 2", particles=2)
    refused(eng, "num_draws = 0", K=0)
    refused(eng, "observation strides", obs=_padded(obs_d))
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    refused(_engine(c, monkeypatch), "LDS tables", K=30000)                              # 2 x 30,000 floats of per-draw values: 240 KB


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_call_and_its_file(fam, tmp_path):
    """trajectory_bounds(num_draws=4, return_draws=True): the four [B] tensors and loss [4, B], bitwise equal to Engine.traj_bounds from the
    same generator state; save_trajectory_bounds writes the [n, 4] float32 table of the batches in order."""
    m, batch = _model(fam)
    eng = m._bind().engine
    B = batch["observations"].shape[0]
    eng.rng_seed(4321, first_trajectory=300)
    eng.rng_set_counter(9)
    res = m.trajectory_bounds(num_draws=4, return_draws=True, **batch)
    assert eng.rng_state() == (4321, 300, 13)
    assert set(res) == {"elbo", "iw_bound", "ess", "nll", "loss"}
    assert all(tuple(res[n].shape) == (B,) for n in ("elbo", "iw_bound", "ess", "nll")) and tuple(res["loss"].shape) == (4, B)
    assert set(m.trajectory_bounds(num_draws=2, **batch)) == {"elbo", "iw_bound", "ess", "nll"}
    eng.rng_set_counter(9)
    labs = [batch[l].reshape(B, -1).to(torch.float32).contiguous() for l in m.LABELS]
    bounds, loss = eng.traj_bounds(m._bind().flat, eng.make_batch(batch["observations"], labs, None, particles=4), B, 4)
    assert torch.isfinite(bounds).all() and torch.equal(loss, res["loss"])
    for i, n in enumerate(("elbo", "iw_bound", "ess", "nll")):
        assert torch.equal(bounds[:, i], res[n])
    TU.check_reduction(bounds, loss, fam + " model")
    eng.rng_set_counter(9)
    path = m.save_trajectory_bounds(str(tmp_path / "res"), [batch, batch], 4)
    table = np.load(path)
    assert os.path.basename(path) == "bounds_post.npy" and table.shape == (2 * B, 4) and table.dtype == np.float32
    assert np.array_equal(table[:B], bounds.cpu().numpy()) and np.isfinite(table).all()


def test_training_entry_point_with_test_bounds(tmp_path, monkeypatch, capsys):
    """One --test-bounds 4 run of training.main on a synthetic loader, one epoch: bounds_post.npy [n, 4] beside the run's other files."""
    from structured_latent_odes_amd import training as T
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.models.mechanistic_cvs_Gauss import MechanisticModelGauss

    def load_config():
        cfg = EU.model_config("cvs")
        cfg.update(mini_batch_size=16, seq_len=86)
        return cfg

    monkeypatch.chdir(tmp_path)
    T.main("cvs", load_config, MechanisticModel, MechanisticModelGauss, ["--epochs", "1", "--batches-per-epoch", "1", "--test-bounds", "4"])
    assert "FINAL TEST:" in capsys.readouterr().out
    table = np.load(str(tmp_path / ("results_%s" % load_config().model) / "bounds_post.npy"))
    assert table.shape == (16, 4) and table.dtype == np.float32 and np.isfinite(table).all()
    assert np.all(table[:, 2] >= 1.0) and np.all(table[:, 2] <= 4.0) and np.all(table[:, 1] <= table[:, 0] + 2.0 ** -22 * np.abs(table[:, 0]))


def test_launches_and_graph_capture():
    """Three launches, "weff", "enc_fwd2", "traj_bounds", on one stream (a linear graph: no parallel branches).  One capture and one replay
    of a call with explicit noise equal the stream-launched call bitwise."""
    c = TU.build("cvs_ald", "rk4", K=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eng.profile_enable(True)
    _bounds(eng, flat, c, obs_d=obs_d, labels=labels)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "traj_bounds"]
    eng.profile_enable(False)
    bounds = torch.zeros(c["B"], 4, device=DEV)
    loss = torch.zeros(7, c["B"], device=DEV)
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    want = _captured(lambda: eng.traj_bounds(flat, bt, c["B"], 7, bounds, loss), (bounds, loss))
    assert torch.equal(bounds, want[0]) and torch.equal(loss, want[1]) and want[0].abs().sum().item() > 0.0
