"""CPU tests of the sample moments of the reconstruction: the C ABI of slode_recon_moments, the numerics of the kernel's accumulation
(numpy restatement against fp64 np.mean / np.std on the case a plain sum of squares fails), the model-level fallback on an engine
double, and the --sample-moments flag of the three training entry points."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

from tests import recon_moments_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_recon_moments_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    assert hasattr(lib, "slode_recon_moments") and "slode_recon_moments" in L.EXPORTS
    m = re.search(r"int\s+slode_recon_moments\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]     # (the comments carry commas: [Q,B,C,T])
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "s", "lay", "params", "times", "stage_t", "batch", "is_post", "num_samples", "mean",
                                                         "sd", "workspace", "workspace_bytes", "stream"]
    at = lib.slode_recon_moments.argtypes
    assert len(at) == len(args) and at[7] is C.c_int and at[8] is C.c_int and at[12] is C.c_size_t
    doc = hdr[hdr.index("the Monte-Carlo summary of `multiple_samples`"):m.start()]
    for word in ("NULL handle", "num_samples < 1", "adaptive solver", "dopri5", "bosh3", "fehlberg2", "adaptive_heun", "particles > 1",
                 "observation strides", "SLODE_NO_FOLD", "SLODE_FOLD_NEXT", "SLODE_ODE_PACK", "SLODE_ODE_ALG", "LDS tables", "SLODE_EINVAL",
                 "n + 1", "mu_50", "mu_75", "mu_25", "POPULATION"):
        assert word in doc, word
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 150
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_recon_moments(None, None, None, None, None, None, None, 1, 200, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def _curves(ns=200, n=4096, ratio=1e-4, seed=5):
    """fp32 values of n curve points: level in [0.5, 20], sd = ratio x level over ns normal draws."""
    g = np.random.default_rng(seed)
    level = g.uniform(0.5, 20.0, size=n)
    return (level[None, :] * (1.0 + ratio * g.standard_normal((ns, n)))).astype(np.float32)


@pytest.mark.parametrize("ns", [2, 7, 200])
def test_shifted_accumulation_against_fp64_where_a_plain_sum_of_squares_fails(ns):
    """Curves with sd / mean = 1e-4 (a prior-pass curve), ns draws: the restatement of the kernel's accumulation (same operations, same
    order, fp32) against np.mean / np.std of the same fp32 values in fp64, within the rounding bounds of RU.accumulation_bars; the
    plain fp32 sum of v^2 misses the same sd bar -- by a factor printed here -- so the case tells the two apart."""
    vals = _curves(ns)
    v64 = vals.astype(np.float64)
    want_mean, want_sd = np.mean(v64, 0), np.std(v64, 0)
    assert np.all(np.abs(v64 - v64[0]).max(0) <= RU.SPREAD * want_sd)                 # the condition of the bars
    bar_mean, bar_sd = RU.accumulation_bars(want_mean, want_sd, ns)
    mean, sd = RU.shifted_moments_f32(vals)
    live = want_sd > 0                                                                # (two draws that round to the same fp32 value: sd = 0 = bar)
    assert np.array_equal(sd[~live], want_sd[~live])
    em, es = np.abs(mean - want_mean) / bar_mean, (np.abs(sd - want_sd)[live] / bar_sd[live])
    pm, ps = RU.plain_moments_f32(vals)
    plain = np.abs(ps - want_sd)[live] / bar_sd[live]
    sd, ps, want_sd = sd[live], ps[live], want_sd[live]
    print("ns = %d: shifted mean error / bar %.3f, sd error / bar %.3f (relative sd error %.2e); plain sum of squares: sd error / bar %.1f "
          "(relative %.2e)" % (ns, em.max(), es.max(), (np.abs(sd - want_sd) / want_sd).max(), plain.max(), (np.abs(ps - want_sd) / want_sd).max()))
    assert em.max() <= 1.0 and es.max() <= 1.0
    assert plain.max() > 1.0 and np.median(plain) > 1.0


def test_one_draw_gives_sd_zero_and_the_draw_itself():
    vals = _curves(1)
    mean, sd = RU.shifted_moments_f32(vals)
    assert np.array_equal(mean, vals[0]) and not sd.any()


def test_engine_signature():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.recon_moments).parameters)[:8] == ["self", "params", "batch", "B", "is_post", "num_samples", "mean", "sd"]


class _Eng:
    def __init__(self, refuse, Q):
        self.refuse, self.Q, self.fused, self.batches, self.draws = refuse, Q, 0, [], []      # refuse: a slode_status, or 0

    def draw_normal(self, rows):
        self.draws.append(rows)
        return torch.arange(rows * 4, dtype=torch.float32).view(rows, 4)                  # row r holds 4 r .. 4 r + 3

    def make_batch(self, obs, labels, eps=None, particles=1):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def recon_moments(self, flat, bt, B, is_post, num_samples):
        from structured_latent_odes_amd import _lib as L
        self.fused += 1
        if self.refuse:
            err = L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse                                                          # as engine._check raises it
            raise err
        q = torch.arange(self.Q, dtype=torch.float32).view(self.Q, 1, 1, 1)
        return q + torch.zeros(self.Q, B, 3, 10), -q + torch.zeros(self.Q, B, 3, 10)


def _double(gauss, refuse):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        LABELS, GAUSS = ("iext",), gauss

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3), "flat": torch.zeros(1)})()
            self.sample_calls = []

        def _bind(self):
            return self._b

        def recon_samples(self, observations, is_post, num_samples, eps=None, **labels):
            """[B, C, T, ns] curves = row index + draw index (+ 100 per curve name): their moments are known in closed form."""
            B = observations.shape[0]
            self.sample_calls.append((B, bool(is_post), num_samples, None if eps is None else tuple(eps.shape), labels["iext"].shape[0]))
            self.first_eps = getattr(self, "first_eps", []) + [None if eps is None else float(eps[0, 0, 0])]
            base = observations[:, :1, :1].reshape(B, 1, 1, 1) + torch.arange(num_samples, dtype=torch.float32).view(1, 1, 1, -1)
            names = ("mean",) if gauss else ("mu_75", "mu_50", "mu_25")
            return dict({n: (base + 100.0 * i).expand(B, 3, 10, num_samples) for i, n in enumerate(names)}, z=None)

    return M()


@pytest.mark.parametrize("gauss", [False, True])
def test_model_level_call_uses_the_engine_and_falls_back_when_it_refuses(gauss, monkeypatch):
    obs = torch.arange(7, dtype=torch.float32).view(7, 1, 1).expand(7, 3, 10).contiguous()
    lab = torch.zeros(7, 1)
    keys = {"mean"} if gauss else {"mu_50", "mu_75", "mu_25"}
    m = _double(gauss, refuse=0)
    res = m.recon_moments(obs, True, 5, iext=lab)
    assert set(res) == keys and m.sample_calls == [] and m._b.engine.fused == 1 and m._b.engine.batches == [((7, 3, 10), 1, None, 5)]
    for q, n in enumerate(("mean",) if gauss else ("mu_50", "mu_75", "mu_25")):      # the engine's head order
        mean, sd = res[n]
        assert tuple(mean.shape) == tuple(sd.shape) == (7, 3, 10) and float(mean[0, 0, 0]) == q and float(sd[0, 0, 0]) == -q
    # a refusal: the chunked composition from recon_samples, the same keys and shapes; explicit eps is sliced with the rows
    m = _double(gauss, refuse=-1)                                                    # SLODE_EINVAL
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)                           # 15 // 5 = 3 rows per chunk: 3 + 3 + 1
    eps = torch.zeros(5, 7, 4)
    res = m.recon_moments(obs, False, 5, eps=eps, iext=lab)
    assert m._b.engine.fused == 1 and m.sample_calls == [(3, False, 5, (5, 3, 4), 3), (3, False, 5, (5, 3, 4), 3), (1, False, 5, (5, 1, 4), 1)]
    assert set(res) == keys
    for i, n in enumerate(("mean",) if gauss else ("mu_75", "mu_50", "mu_25")):
        mean, sd = res[n]
        assert tuple(mean.shape) == tuple(sd.shape) == (7, 3, 10) and mean.dtype == torch.float32
        assert torch.allclose(mean[:, 0, 0], torch.arange(7.0) + 2.0 + 100.0 * i)    # mean of 0 .. 4 = 2
        assert torch.allclose(sd, torch.full_like(sd, float(np.std(np.arange(5.0)))))   # population sd
    with pytest.raises(ValueError, match="num_samples"):
        m.recon_moments(obs, True, 0, iext=lab)
    # no eps: ONE drawing call of ns * B rows for the whole batch, sliced per chunk (row k * B + b: chunk rows 0, 3, 6 of draw 0)
    m.sample_calls, m.first_eps = [], []
    m.recon_moments(obs, True, 5, iext=lab)
    assert m._b.engine.draws == [35] and [c[3] for c in m.sample_calls] == [(5, 3, 4), (5, 3, 4), (5, 1, 4)]
    assert m.first_eps == [0.0, 12.0, 24.0]


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    """SLODE_EHIP / SLODE_ENOSPC (a launch error, a workspace that is too small) are raised, not turned into the materialising path."""
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.recon_moments(torch.zeros(2, 3, 10), True, 5, iext=torch.zeros(2, 1))
    assert m.sample_calls == [] and m._b.engine.draws == []


def test_save_recon_moments_file_names(tmp_path):
    m = _double(False, refuse=0)
    obs = torch.zeros(2, 3, 10)
    files = m.save_recon_moments(str(tmp_path / "r"), obs, True, 4, iext=torch.zeros(2, 1))
    files += m.save_recon_moments(str(tmp_path / "r"), obs, False, 4, iext=torch.zeros(2, 1))
    want = sorted("%s_%s_sample_%s.npy" % (c, p, k) for c in ("mu_50", "mu_75", "mu_25") for p in ("post", "prior") for k in ("mean", "sd"))
    assert sorted(os.path.basename(f) for f in files) == want
    assert all(np.load(f).shape == (2, 3, 10) for f in files)


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_sample_moments_flag_of_the_training_entry_points(fam, monkeypatch, tmp_path):
    """--sample-moments reaches train() as sample_moments=True from each entry point; without it train() gets what it gets today."""
    from structured_latent_odes_amd import training as TR
    tr = importlib.import_module("training_" + fam)
    seen = []
    monkeypatch.setattr(TR, "train", lambda config, family, a, b, n, **kw: seen.append((family, kw)))
    monkeypatch.chdir(tmp_path)
    assert TR.build_parser().parse_args([]).sample_moments is False
    for argv in (["--epochs", "1"], ["--epochs", "1", "--sample-moments"]):
        TR.main(tr.FAMILY, tr.load_config, tr.MechanisticModel, tr.MechanisticModelGauss, argv=argv)
    assert seen == [(fam, {"fused_stats": False}), (fam, {"fused_stats": False, "sample_moments": True})]
