"""GPU tests of the fused statistics pass (slode_eval_stats / Engine.eval_stats / MechanisticBase.eval_stats /
training.input_pred_stats_fused) against the fp64 oracle and against the unfused pass.  Bars (tests/eval_stats_util.py):
  * slots 0, 1 (-ELBO main, auxiliary loss): 1e-5 relative, the bar of tests/test_gpu_parity.py;
  * slot 2 (sum |centre curve - observation|): 2e-5 * sum max(1, |oracle curve|) -- the per-element bar of decoded curves, summed;
  * hit counts: equal as integers (the seeds keep every decision 1e-4 away from its threshold: tests/test_eval_stats_cpu.py)."""
import importlib

import pytest
import torch

from tests import eval_stats_util as EU
from tests.eval_gpu_util import DEV, _captured, _device_batch, _engine, _model_batches, _padded

pytestmark = pytest.mark.gpu


def _row(eng, flat, obs_d, labels, eps4, is_post, B):
    from structured_latent_odes_amd import _lib as L
    out = torch.full((L.EVAL_SLOTS,), float("nan"), device=DEV)
    bt = eng.make_batch(obs_d, labels, eps4, particles=4 if eps4 is not None else 1)
    eng.eval_stats(flat, bt, B, is_post, out)
    return out


def _check_row(row, want, B, tag):
    row = row.double().cpu()
    n_aux = len(want["hits"])
    print("%s: main %.6f / %.6f  aux %.6f / %.6f  l1 %.6f / %.6f (bar %.3e)  hits %s / %s" % (
        tag, row[0], want["main"], row[1], want["aux"], row[2], want["l1_sum"], want["l1_bar"], row[3:3 + n_aux].tolist(), want["hits"]))
    assert torch.isfinite(row).all(), tag
    assert abs(row[0].item() - want["main"]) <= 1e-5 * abs(want["main"]), (tag, row[0].item(), want["main"])
    assert abs(row[1].item() - want["aux"]) <= 1e-5 * abs(want["aux"]), (tag, row[1].item(), want["aux"])
    assert abs(row[2].item() - want["l1_sum"]) <= want["l1_bar"], (tag, row[2].item(), want["l1_sum"], want["l1_bar"])
    assert [int(v) for v in row[3:3 + n_aux].tolist()] == want["hits"], (tag, row[3:3 + n_aux].tolist(), want["hits"])
    assert row[3 + n_aux:7].abs().sum().item() == 0.0 and row[7].item() == B, tag


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_row_matches_the_fp64_oracle(case, solver):
    """Explicit noise; six model classes x three fixed-grid solvers x {posterior, prior}."""
    c = EU.build(case, solver)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps4 = c["eps4"].to(DEV).contiguous()
    for is_post in (True, False):
        want = EU.oracle_row(c, is_post)
        assert EU.min_margin(want) >= EU.MARGIN            # the condition of the hit comparison: no trajectory is left out
        _check_row(_row(eng, flat, obs_d, labels, eps4, is_post, c["B"]), want, c["B"], "%s/%s/%s" % (case, solver, "post" if is_post else "prior"))


INSTANTIATIONS = {   # every compiled form of eval_stats_kernel: S = 5, S = 8, run-time S; each loop-free and in the persistent loop
    "s5": ("cvs_ald", {}), "s8": ("proc_ald", {}), "generic_s5": ("cvs_ald", {"SLODE_ODE_GENERIC": "1"}),
    "generic_s8": ("proc_gauss", {"SLODE_ODE_GENERIC": "1"}),
    "s5_loop": ("cvs_ald", {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}), "s8_loop": ("proc_ald", {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}),
    "generic_loop": ("challenge_ald", {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}),
}


@pytest.mark.parametrize("name", list(INSTANTIATIONS))
def test_every_instantiation_on_a_poisoned_workspace_twice(name, monkeypatch):
    """NaN-poisoned workspace, run twice: rows bitwise equal and equal to the oracle's; B = 37 / 16 / 9 trajectories on 5 / 2 workgroups
    in the looped forms (a B beyond the grid)."""
    case, env = INSTANTIATIONS[name]
    c = EU.build(case, "rk4")
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps4 = c["eps4"].to(DEV).contiguous()
    rows = []
    for _ in range(2):
        eng.workspace(c["B"]).fill_(float("nan"))
        rows.append(_row(eng, flat, obs_d, labels, eps4, True, c["B"]).clone())
    assert torch.equal(rows[0], rows[1])
    _check_row(rows[0], EU.oracle_row(c, True), c["B"], name)


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_in_kernel_noise_is_the_explicit_noise_bitwise(case):
    c = EU.build(case, "midpoint")
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eng.rng_seed(77)
    eng.rng_set_counter(5)
    for is_post in (True, False):
        n = eng.rng_state()[2]
        a = _row(eng, flat, obs_d, labels, None, is_post, c["B"]).clone()
        assert eng.rng_state()[2] == n + 4
        eps4 = torch.stack([eng.rng_normal(n + i, c["B"]) for i in range(4)]).contiguous()
        b = _row(eng, flat, obs_d, labels, eps4, is_post, c["B"])
        assert eng.rng_state()[2] == n + 4                 # explicit noise draws nothing
        assert torch.equal(a, b), (a, b)


def test_launch_count_and_graph_capture():
    """At most four kernels, the encoder among them once; the call is capturable and one replay is bitwise the stream-launched row."""
    from structured_latent_odes_amd import _lib as L
    c = EU.build("cvs_ald", "rk4")
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps4 = c["eps4"].to(DEV).contiguous()
    eng.profile_enable(True)
    _row(eng, flat, obs_d, labels, eps4, True, c["B"])
    prof = eng.profile_read()
    eng.profile_enable(False)
    names = [n for n, _ in prof]
    print("kernels:", prof)
    assert len(names) <= 4 and names.count("enc_fwd2") == 1 and names.count("eval_stats") == 1 and names[-1] == "eval_reduce", names

    out = torch.zeros(L.EVAL_SLOTS, device=DEV)
    bt = eng.make_batch(obs_d, labels, eps4, particles=4)
    want, = _captured(lambda: eng.eval_stats(flat, bt, c["B"], True, out), (out,))
    assert torch.equal(out, want), (out, want)


def test_refusals_by_name(monkeypatch):
    from structured_latent_odes_amd import _lib as L
    c = EU.build("cvs_ald", "rk4")
    obs_d, labels = _device_batch(c)
    eps4 = c["eps4"].to(DEV).contiguous()
    out = torch.zeros(L.EVAL_SLOTS, device=DEV)
    eng = _engine(c, solver="dopri5")
    flat = eng.pack(c["p"])
    n = eng.rng_state()[2]
    with pytest.raises(L.SlodeError, match="adaptive solver dopri5"):
        eng.eval_stats(flat, eng.make_batch(obs_d, labels, eps4, particles=4), c["B"], True, out)
    eng = _engine(c)
    with pytest.raises(L.SlodeError, match="particles = 2"):
        eng.eval_stats(flat, eng.make_batch(obs_d, labels, None), c["B"], True, out, particles=2)
    with pytest.raises(L.SlodeError, match="observation strides"):
        eng.eval_stats(flat, eng.make_batch(_padded(obs_d), labels, None), c["B"], True, out)
    assert eng.rng_state()[2] == n                          # a refused call draws nothing
    eng = _engine(c, monkeypatch, {"SLODE_ODE_ALG": "1"})
    with pytest.raises(L.SlodeError, match="measured arms"):
        eng.eval_stats(flat, eng.make_batch(obs_d, labels, None), c["B"], True, out)


def _model(fam, solver=None):
    m, batches = _model_batches(fam, solver)
    m._bind().engine.rng_seed(EU.MODEL_RNG_SEED)
    return m, batches


def _agree(f, u, n_batches, size, tag):
    print(tag, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in f.items()}, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in u.items()})
    for k in u:
        if k == "elbo":
            for a, b in zip(f[k].tolist(), u[k].tolist()):
                assert abs(a - b) <= 1e-5 * abs(b), (tag, k, a, b)
        elif k == "l1":
            # l1 = (sum of per-batch means) / trajectories; per element the curves agree to 2e-5 max(1, |curve|), taken at its floor 2e-5
            assert abs(f[k] - u[k]) <= 2e-5 * n_batches / size, (tag, f[k], u[k])
        else:
            assert f[k] == u[k], (tag, k, f[k], u[k])


@pytest.mark.parametrize("fam", list(EU.MODEL_CASES))
def test_fused_pass_equals_the_unfused_pass(fam):
    """Same generator state, same three batches (the last one ragged): the same dict, the same counter afterwards."""
    from structured_latent_odes_amd import training as TR
    from structured_latent_odes_amd.svi import SVI
    m, batches = _model(fam)
    eng = m._bind().engine
    losses = [SVI(m.model, m.guide, None), SVI(m.model_meta, m.guide_meta, None)]
    size = sum(b["observations"].shape[0] for b in batches)
    for is_post in (True, False):
        eng.rng_set_counter(0)
        unfused = TR.input_pred_stats(batches, m, losses, is_post, DEV, fam)
        n_unfused = eng.rng_state()[2]
        eng.rng_set_counter(0)
        fused = TR.input_pred_stats_fused(batches, m, is_post, DEV, fam)
        assert eng.rng_state()[2] == n_unfused == 4 * len(batches)
        _agree(fused, unfused, len(batches), size, "%s/%s" % (fam, "post" if is_post else "prior"))


def test_model_level_call_is_total_over_what_the_engine_refuses():
    """dopri5, two particles, a padded observation tensor: Engine.eval_stats refuses, MechanisticBase.eval_stats composes the row from the
    unfused calls -- equal to those calls made by hand from the same generator state."""
    from structured_latent_odes_amd.svi import SVI, Trace_ELBO
    for solver, K, pad in (("dopri5", 1, False), ("rk4", 2, False), ("rk4", 1, True)):
        m, batches = _model("cvs", solver)
        eng = m._bind().engine
        batch = {k: v.to(DEV) for k, v in batches[0].items()}
        batch = {k: (v.reshape(v.shape[0], -1) if k != "observations" else v) for k, v in batch.items()}
        if pad:
            batch["observations"] = _padded(batch["observations"])
        eng.rng_set_counter(0)
        row = m.eval_stats(is_post=True, num_particles=K, **batch).cpu()
        n_row = eng.rng_state()[2]
        eng.rng_set_counter(0)
        elbo = Trace_ELBO(num_particles=K)
        main = SVI(m.model, m.guide, None, loss=elbo).evaluate_loss(**batch)
        aux = SVI(m.model_meta, m.guide_meta, None, loss=elbo).evaluate_loss(**batch)
        l1 = float(m.recon(is_post=True, **batch)["l1"]) * batch["observations"].numel()
        pred = m._predict_labels(batch["observations"])
        hits = [float((pred[l] - batch[l]).abs().lt(0.5).all(dim=1).float().sum()) for l in ("iext", "rtpr")]
        assert eng.rng_state()[2] == n_row
        want = torch.tensor([main, aux, l1] + hits + [0.0, 0.0, float(batch["observations"].shape[0])])
        assert torch.allclose(row, want, rtol=1e-6, atol=0.0), (solver, K, pad, row, want)


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_training_entry_points_with_fused_statistics(fam, capsys):
    tr = importlib.import_module("training_" + fam)
    cfg = EU.model_config(fam)
    cfg.update(num_epochs=1, mini_batch_size=16, seq_len=86)
    var_model, best_model, best_epoch = tr.train(cfg, batches_per_epoch=2, fused_stats=True)
    out = capsys.readouterr().out
    assert "[Epoch 1/1] loss=" in out and "FINAL TEST:" in out and "l1=(" in out
    assert all(torch.isfinite(p).all() for p in var_model.parameters())
