"""CPU tests of the fused statistics pass: the C ABI of slode_eval_stats, the host logic of training.input_pred_stats_fused on a model
test double, and the margin condition of the GPU hit comparison (tests/test_gpu_eval_stats.py) on the fp64 oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_eval_stats_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    assert hasattr(lib, "slode_eval_stats") and "slode_eval_stats" in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_EVAL_SLOTS\s+(\d+)", hdr).group(1)) == L.EVAL_SLOTS == 8
    m = re.search(r"int\s+slode_eval_stats\s*\(([^;]*)\)\s*;", hdr)
    args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "s", "lay", "params", "times", "stage_t", "batch", "is_post", "out", "workspace",
                                                         "workspace_bytes", "stream"]
    assert len(lib.slode_eval_stats.argtypes) == len(args) and lib.slode_eval_stats.argtypes[7] is C.c_int
    assert lib.slode_eval_stats.argtypes[10] is C.c_size_t
    doc = hdr[hdr.index("one batch of the per-epoch statistics"):m.start()]
    for word in ("adaptive solver", "dopri5", "particles > 1", "observation strides", "SLODE_FOLD_NEXT", "SLODE_EINVAL", "n + 4"):
        assert word in doc, word
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 140
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_eval_stats(None, None, None, None, None, None, None, 1, None, None, 0, None) == -1


class _Double:
    """Stands for a model: eval_stats writes a prepared row into the caller's table row, on the 'device' the table lives on."""

    def __init__(self, rows, slots):
        self.rows, self.slots, self.calls = rows, slots, []

    def eval_stat_slots(self):
        return dict(self.slots)

    def eval_stats(self, observations, is_post, out=None, num_particles=1, **labels):
        i = len(self.calls)
        self.calls.append((tuple(observations.shape), bool(is_post), num_particles, sorted(labels)))
        out.copy_(torch.tensor(self.rows[i], dtype=torch.float32))
        return out


def _batches(sizes, C_=3, T=10):
    return [{"observations": torch.zeros(B, C_, T), "iext": torch.zeros(B, 1), "rtpr": torch.zeros(B, 1)} for B in sizes]


def test_fused_pass_host_logic(monkeypatch):
    from structured_latent_odes_amd import training as TR
    sizes = [4, 4, 3]                                        # ragged last batch
    C_, T = 3, 10
    rows = [[10.0 * B, 2.0 * B, 0.5 * B * C_ * T * (i + 1), B - 1, 1, 0, 0, B] for i, B in enumerate(sizes)]
    model = _Double(rows, {"iext": 3, "rtpr": 4})
    copies = []
    real = TR._to_host
    monkeypatch.setattr(TR, "_to_host", lambda t: (copies.append(tuple(t.shape)), real(t))[1])
    out = TR.input_pred_stats_fused(_batches(sizes), model, True, torch.device("cpu"), "cvs")
    assert copies == [(3, 8)]                                # ONE read-back, of the rows written
    assert [c[0] for c in model.calls] == [(4, 3, 10), (4, 3, 10), (3, 3, 10)] and all(c[1] for c in model.calls)
    assert all(c[3] == ["iext", "rtpr"] for c in model.calls)
    size = sum(sizes)
    assert out["iext"] == pytest.approx(sum(B - 1 for B in sizes) / size) and out["rtpr"] == pytest.approx(3 / size)
    # the reference's quirks: elbo = sum over batches of loss / B; l1 = (sum of per-batch means) / trajectories
    assert out["elbo"].tolist() == pytest.approx([30.0, 6.0])
    assert out["l1"] == pytest.approx((0.5 + 1.0 + 1.5) / size)
    assert set(out) == {"iext", "rtpr", "l1", "elbo"}


def test_fused_pass_grows_its_table_for_iterables_without_len(monkeypatch):
    from structured_latent_odes_amd import training as TR
    monkeypatch.setattr(TR, "STATS_CHUNK", 2)
    sizes = [2] * 5
    rows = [[1.0 * (i + 1), 0.0, 60.0, 2, 0, 0, 0, 2] for i in range(5)]
    model = _Double(rows, {"iext": 3, "rtpr": 4})
    copies = []
    real = TR._to_host
    monkeypatch.setattr(TR, "_to_host", lambda t: (copies.append(tuple(t.shape)), real(t))[1])
    out = TR.input_pred_stats_fused((b for b in _batches(sizes)), model, False, torch.device("cpu"), "cvs", num_particles=3)
    assert copies == [(5, 8)] and len(model.calls) == 5 and not any(c[1] for c in model.calls) and model.calls[0][2] == 3
    assert out["elbo"].tolist() == pytest.approx([sum(range(1, 6)) / 2.0, 0.0]) and out["iext"] == 1.0 and out["rtpr"] == 0.0
    empty = TR.input_pred_stats_fused([], model, True, torch.device("cpu"), "cvs")
    assert empty["l1"] == 0.0 and empty["iext"] == 0.0 and empty["elbo"].tolist() == [0.0, 0.0]


def test_model_level_call_falls_back_when_the_engine_refuses():
    """MechanisticBase.eval_stats on engine / binding doubles: an engine refusal (SlodeError) leads to the composed row; a particle count
    above one never reaches the engine's fused call."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class Eng:
        def __init__(self, refuse):
            self.refuse, self.fused = refuse, 0

        def make_batch(self, obs, labels, eps=None, particles=1):
            return object()

        def eval_stats(self, flat, bt, B, is_post, out):
            self.fused += 1
            if self.refuse:
                raise L.SlodeError("slode_eval_stats: adaptive solver dopri5 is not taken")
            out.fill_(1.0)
            return out

    class M(MechanisticBase):
        LABELS, AUX = ("iext",), [("q", "iext", "iext", "sigmoid")]

        def __init__(self, eng):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": eng, "flat": torch.zeros(1)})()
            self.composed = []

        def _bind(self):
            return self._b

        def _eval_stats_composed(self, observations, is_post, out, num_particles, labels):
            self.composed.append(num_particles)
            return out.fill_(2.0)

    obs, lab = torch.zeros(3, 3, 10), torch.zeros(3, 1)
    m = M(Eng(False))
    assert m.eval_stats(obs, True, iext=lab).tolist() == [1.0] * 8 and m.composed == []
    assert m.eval_stat_slots() == {"iext": 3}
    m = M(Eng(True))
    assert m.eval_stats(obs, True, iext=lab).tolist() == [2.0] * 8 and m.composed == [1] and m._b.engine.fused == 1
    m = M(Eng(False))
    assert m.eval_stats(obs, False, num_particles=2, iext=lab).tolist() == [2.0] * 8 and m.composed == [2] and m._b.engine.fused == 0


@pytest.mark.parametrize("case", list(EU.CASES))
def test_hit_decisions_of_the_gpu_cases_keep_their_margin(case):
    """A condition of the GPU comparison, not a measurement: on the fp64 oracle no trajectory of any case has a sigmoid output within 1e-4
    of 0.5, a softmax top-two gap under 1e-4 or an Exp/Exp value within 1e-4 of label +- 0.5 -- so ZERO trajectories are left out of the
    integer comparison of the hit counts.  (The label draw is a posterior draw and does not depend on the solver.)"""
    row = EU.oracle_row(EU.build(case, "euler"), True)
    assert len(row["margins"]) == len(row["hits"]) > 0
    for mg in row["margins"]:
        assert mg.shape[0] == EU.CASES[case][2] and float(mg.min()) >= EU.MARGIN, (case, float(mg.min()))


@pytest.mark.parametrize("fam", list(EU.MODEL_CASES))
def test_hit_decisions_of_the_model_level_pass_keep_their_margin(fam):
    """The same condition for the pass that compares the fused with the unfused statistics (in-kernel noise): batch i draws its label
    noise as drawing call 4 i + 3 of the Philox stream (tests/rng_math.py) keyed by the seed the GPU test sets."""
    from oracle import slode_oracle as O
    from tests import rng_math as RM
    twin, state, batches, times = EU.model_state(fam)
    cfg = EU.model_config(fam)
    ospec = {"cvs": lambda: O.cvs_spec(cfg.z_iext_dim, cfg.z_rtpr_dim, cfg.z_epsilon_dim, solver="rk4"),
             "challenge": lambda: O.challenge_spec(cfg.z_shedding_dim, cfg.z_symptoms_dim, cfg.z_epsilon_dim, solver="rk4"),
             "proc": lambda: O.proc_spec(cfg.z_aR_dim, cfg.z_epsilon_dim, solver="rk4")}[fam]()
    assert ospec.latent_dim == twin.latent_dim
    p64 = {k: v.double() for k, v in state.items()}
    for i, b in enumerate(batches):
        obs = b["observations"].double()
        u = torch.cat([b[l].reshape(obs.shape[0], -1) for l in twin.LABELS], 1).double()
        with torch.no_grad():
            loc, scale = O.encoder_conv(p64, obs, cfg.pool_size)
            eps = torch.from_numpy(RM.normals(EU.MODEL_RNG_SEED, 4 * i + 3, 0, obs.shape[0], ospec.latent_dim))
            hits, margins = EU.label_decisions(p64, ospec, loc + scale * eps, u)
        for mg in margins:
            assert float(mg.min()) >= EU.MARGIN, (fam, i, float(mg.min()))
