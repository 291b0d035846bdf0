"""CPU tests of the counterfactual curves: the C ABI of slode_intervene_moments, the oracle composition of tests/intervene_util.py (effect 0
under an empty mask; counterfactual labels that really differ), the numerics of the kernel's two shifted accumulations, and the model-level
call on an engine double (name validation before any engine call, engine route, composed route, file names)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import intervene_util as IU
from tests import recon_moments_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_intervene_moments_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    assert hasattr(lib, "slode_intervene_moments") and "slode_intervene_moments" in L.EXPORTS
    m = re.search(r"int\s+slode_intervene_moments\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "s", "lay", "params", "times", "stage_t", "batch", "cf_labels", "group_mask", "num_samples",
                                                         "cf_mean", "cf_sd", "eff_mean", "eff_sd", "workspace", "workspace_bytes", "stream"]
    at = lib.slode_intervene_moments.argtypes
    assert len(at) == len(args) and at[8] is C.c_uint and at[9] is C.c_int and at[15] is C.c_size_t
    doc = hdr[hdr.index("counterfactual curves as ONE call"):m.start()]
    for word in ("NULL handle", "num_samples < 1", "adaptive solver", "dopri5", "bosh3", "fehlberg2", "adaptive_heun", "particles > 1",
                 "observation strides", "SLODE_NO_FOLD", "SLODE_FOLD_NEXT", "SLODE_ODE_PACK", "SLODE_ODE_ALG", "LDS tables", "SLODE_EINVAL",
                 "n + 1", "mu_50", "POPULATION", "PAIRED", "group_mask == 0", "n_groups", "cf_labels NULL", "intervene_moments"):
        assert word in doc, word
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 170
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_intervene_moments(None, None, None, None, None, None, None, None, 1, 8, None, None, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_engine_signature():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.intervene_moments).parameters)[:7] == ["self", "params", "batch", "B", "cf_labels", "group_mask", "num_samples"]


@pytest.mark.parametrize("case", list(EU.CASES))
def test_oracle_effect_is_zero_under_an_empty_mask(case):
    """mask = 0: both arms are the posterior draw, whatever the counterfactual labels say; cf = the factual moments of RU.oracle_moments."""
    c = RU.build(case, "euler", B=3, ns=2)
    want = IU.oracle_moments(c, 0, IU.cf_labels(c["u"]))
    assert not want["eff_mean"].any() and not want["eff_sd"].any()
    mean, sd = RU.oracle_moments(c, True)
    assert np.array_equal(want["cf_mean"], mean) and np.array_equal(want["cf_sd"], sd)


@pytest.mark.parametrize("case", list(EU.CASES))
def test_rolled_labels_differ_in_every_intervened_group(case):
    """Otherwise the GPU oracle test could pass on an engine that ignores cf_labels: at the case's own B, for every mask of the family,
    every intervened group sees at least one row whose label columns changed -- and the columns no swap names stay as they were."""
    c = RU.build(case, "euler", ns=1)
    u, ospec = c["u"], c["ospec"]
    for tag, mask, cols in IU.MASKS[c["fam"]]:
        u_cf = IU.cf_labels(u, cols)
        for g, gr in enumerate(ospec.prior_groups):
            if (mask >> g) & 1:
                sl = slice(gr.u_off, gr.u_off + gr.u_dim)
                assert bool((u_cf[:, sl] != u[:, sl]).any(dim=1).any()), (case, tag, g)
        if cols is not None:
            keep = [q for q in range(u.shape[1]) if q not in cols]
            assert torch.equal(u_cf[:, keep], u[:, keep]) and set(cols) <= set(IU.group_columns(ospec, mask))
        if c["fam"] == "proc":                                          # one-hot columns stay one-hot
            assert torch.equal(u_cf[:, 0:3].sum(1), u[:, 0:3].sum(1)) and torch.equal(u_cf[:, 3:7].sum(1), u[:, 3:7].sum(1))


def test_oracle_effect_is_not_zero_when_a_group_is_intervened():
    c = RU.build("cvs_ald", "euler", B=4, ns=2)
    u_cf = torch.roll(c["u"], 1, 0)
    u_cf[:, 0] = 1.0 - c["u"][:, 0]                                     # iext flipped in every row
    want = IU.oracle_moments(c, 1, u_cf)
    assert float(np.abs(want["eff_mean"]).max()) > 1e-3
    assert np.allclose(want["eff_mean"], want["cf_mean"] - want["f_mean"], atol=1e-12)


def _pair(ns, n=4096, ratio=1e-4, seed=5):
    """fp32 values of n curve points of both arms: level in [0.5, 20]; the factual arm has sd = ratio x level over ns draws, the
    counterfactual arm = factual x (1 + shift) + its own small noise, so the paired difference has a spread of its own."""
    g = np.random.default_rng(seed)
    level = g.uniform(0.5, 20.0, size=n)
    vf = (level[None, :] * (1.0 + ratio * g.standard_normal((ns, n)))).astype(np.float32)
    vcf = (vf.astype(np.float64) * 1.05 + level[None, :] * ratio * g.standard_normal((ns, n))).astype(np.float32)
    return vf, vcf


@pytest.mark.parametrize("ns", [2, 7, 200])
def test_both_shifted_accumulations_stay_within_the_rounding_bars(ns):
    """The numpy restatement of the kernel's two accumulations (same operations, same order, fp32) against np.mean / np.std in fp64 of the
    same fp32 inputs -- v_cf, and e = fl(v_cf - v_f) -- within RU.accumulation_bars, on curves whose sd is 1e-4 of their level."""
    vf, vcf = _pair(ns)
    got = IU.paired_moments_f32(vf, vcf)
    for name, vals, (mean, sd) in (("cf", vcf, got[:2]), ("effect", (vcf - vf).astype(np.float32), got[2:])):
        v64 = vals.astype(np.float64)
        want_mean, want_sd = np.mean(v64, 0), np.std(v64, 0)
        assert np.all(np.abs(v64 - v64[0]).max(0) <= RU.SPREAD * want_sd)             # the condition of the bars
        bar_mean, bar_sd = RU.accumulation_bars(want_mean, want_sd, ns)
        live = want_sd > 0
        assert np.array_equal(sd[~live], want_sd[~live])
        em, es = np.abs(mean - want_mean) / bar_mean, np.abs(sd - want_sd)[live] / bar_sd[live]
        print("ns = %d %s: mean error / bar %.3f, sd error / bar %.3f" % (ns, name, em.max(), es.max()))
        assert em.max() <= 1.0 and es.max() <= 1.0


def test_one_draw_gives_both_sds_zero():
    vf, vcf = _pair(1)
    cm, cs, em, es = IU.paired_moments_f32(vf, vcf)
    assert np.array_equal(cm, vcf[0]) and np.array_equal(em, vcf[0] - vf[0]) and not cs.any() and not es.any()


class _Eng:
    def __init__(self, refuse, Q):
        self.refuse, self.Q, self.calls, self.batches, self.draws = refuse, Q, [], [], []

    def draw_normal(self, rows):
        self.draws.append(rows)
        return torch.arange(rows * 4, dtype=torch.float32).view(rows, 4)

    def make_batch(self, obs, labels, eps=None, particles=1):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def intervene_moments(self, flat, bt, B, cf_labels, group_mask, num_samples):
        from structured_latent_odes_amd import _lib as L
        self.calls.append((None if cf_labels is None else [None if t is None else tuple(t.shape) for t in cf_labels], group_mask, num_samples))
        self.cf_tensors = cf_labels
        if self.refuse:
            err = L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        q = torch.arange(self.Q, dtype=torch.float32).view(self.Q, 1, 1, 1) + torch.zeros(self.Q, B, 3, 10)
        return q, q + 10, q + 20, q + 30


FAMILIES = {     # FAMILY -> (LABELS, PRIORS) as the model classes carry them: cvs one prior group per label, proc ONE group over its four labels
    "cvs": (("iext", "rtpr"), [("p_z_iext_given_iext", ["iext"], ["iext"]), ("p_z_rtprs_given_rtprs", ["rtpr"], ["rtpr"])]),
    "proc": (("aR", "aS", "C12", "C6"), [("p_z_u_given_u", ["aR", "aS", "C12", "C6"], ["aR", "aS", "C12", "C6"])]),
}


def _double(gauss, refuse, fam="cvs"):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        FAMILY, GAUSS = fam, gauss
        LABELS, PRIORS = FAMILIES[fam]

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3), "flat": torch.zeros(1)})()
            self.sample_calls = []

        def _bind(self):
            return self._b

        def counterfactual_samples(self, observations, num_samples, intervene, eps=None, **labels):
            """factual = row index + draw index (+ 100 per curve name); counterfactual = factual + 2 x draw index + 1: closed-form moments."""
            B = observations.shape[0]
            self.sample_calls.append((B, num_samples, sorted(intervene), None if eps is None else tuple(eps.shape), intervene[sorted(intervene)[0]].shape[0]))
            k = torch.arange(num_samples, dtype=torch.float32).view(1, 1, 1, -1)
            base = observations[:, :1, :1].reshape(B, 1, 1, 1) + k
            names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
            return {n: ((base + 100.0 * i).expand(B, 3, 10, num_samples), (base + 100.0 * i + 2.0 * k + 1.0).expand(B, 3, 10, num_samples))
                    for i, n in enumerate(names)}

    return M()


@pytest.mark.parametrize("gauss", [False, True])
def test_model_level_call_validates_names_uses_the_engine_and_composes_on_a_refusal(gauss, monkeypatch):
    obs = torch.arange(7, dtype=torch.float32).view(7, 1, 1).expand(7, 3, 10).contiguous()
    labels = dict(iext=torch.zeros(7, 1), rtpr=torch.ones(7, 1))
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase
    m = _double(gauss, refuse=0)
    # a name that is no conditional-prior label of the family: ValueError before any engine call
    for bad in ({"symptoms": torch.zeros(7, 1)}, {"iext": torch.zeros(7, 1), "epsilon": torch.zeros(7, 1)}):
        with pytest.raises(ValueError, match="not a conditional-prior label"):
            m.intervention_moments(obs, 5, bad, **labels)
        with pytest.raises(ValueError, match="not a conditional-prior label"):
            MechanisticBase.counterfactual_samples(m, obs, 5, bad, **labels)                # (the base method: the double overrides it)
    assert m._b.engine.calls == [] and m._b.engine.batches == [] and m._b.engine.draws == []
    with pytest.raises(ValueError, match="num_samples"):
        m.intervention_moments(obs, 0, {"iext": torch.ones(7, 1)}, **labels)
    res = m.intervention_moments(obs, 5, {"rtpr": torch.zeros(7, 1)}, **labels)
    assert m._b.engine.calls == [([(7, 1), (7, 1)], 2, 5)] and m._b.engine.batches == [((7, 3, 10), 2, None, 5)] and m.sample_calls == []
    assert set(res) == set(names)
    for q, n in enumerate(names):                                        # the engine's head order
        assert set(res[n]) == {"cf", "effect"} and tuple(res[n]["cf"][0].shape) == (7, 3, 10)
        assert [float(t[0, 0, 0]) for t in res[n]["cf"] + res[n]["effect"]] == [q, q + 10, q + 20, q + 30]
    m.intervention_moments(obs, 5, {"rtpr": torch.zeros(7, 1), "iext": torch.ones(7, 1)}, **labels)
    assert m._b.engine.calls[-1] == ([(7, 1), (7, 1)], 3, 5)
    m.intervention_moments(obs, 5, {}, **labels)                         # nothing intervened: mask 0, no counterfactual labels
    assert m._b.engine.calls[-1] == (None, 0, 5)
    # a refusal: the chunked composition, ONE drawing call for the whole batch
    m = _double(gauss, refuse=-1)
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)               # 15 // 5 = 3 rows per chunk: 3 + 3 + 1
    res = m.intervention_moments(obs, 5, {"iext": torch.ones(7, 1)}, **labels)
    assert len(m._b.engine.calls) == 1 and m._b.engine.draws == [35]
    assert m.sample_calls == [(3, 5, ["iext"], (5, 3, 4), 3), (3, 5, ["iext"], (5, 3, 4), 3), (1, 5, ["iext"], (5, 1, 4), 1)]
    k = np.arange(5.0)
    for i, n in enumerate(names):
        (cm, cs), (em, es) = res[n]["cf"], res[n]["effect"]
        assert all(tuple(t.shape) == (7, 3, 10) and t.dtype == torch.float32 for t in (cm, cs, em, es))
        assert torch.allclose(cm[:, 0, 0], torch.arange(7.0) + 100.0 * i + float(np.mean(3 * k + 1)))
        assert torch.allclose(cs, torch.full_like(cs, float(np.std(3 * k + 1))))
        assert torch.allclose(em, torch.full_like(em, float(np.mean(2 * k + 1)))) and torch.allclose(es, torch.full_like(es, float(np.std(2 * k + 1))))


def test_partial_naming_in_a_group_over_several_labels_reaches_the_engine_with_every_tensor():
    """proc has ONE prior group over aR, aS, C12, C6: with C12 and C6 named, the engine call still gets all four tensors -- the named ones
    with the counterfactual values, the others as they were -- so the group can be redrawn in the one call (no composition)."""
    m = _double(False, refuse=0, fam="proc")
    obs = torch.zeros(7, 3, 10)
    g = torch.Generator().manual_seed(2)
    labels = dict(aR=torch.rand(7, 3, generator=g), aS=torch.rand(7, 4, generator=g), C12=torch.rand(7, 1, generator=g), C6=torch.rand(7, 1, generator=g))
    swap = dict(C12=torch.rand(7, 1, generator=g), C6=torch.rand(7, generator=g))                # [B] is taken as [B, 1]
    m.intervention_moments(obs, 5, swap, **labels)
    eng = m._b.engine
    assert eng.calls == [([(7, 3), (7, 4), (7, 1), (7, 1)], 1, 5)] and m.sample_calls == [] and eng.draws == []
    want = [labels["aR"], labels["aS"], swap["C12"], swap["C6"].reshape(7, 1)]
    assert all(t.dtype == torch.float32 and t.is_contiguous() and torch.equal(t, w) for t, w in zip(eng.cf_tensors, want))
    m.intervention_moments(obs, 5, {"aS": torch.roll(labels["aS"], 1, 0)}, **labels)
    assert eng.calls[-1] == ([(7, 3), (7, 4), (7, 1), (7, 1)], 1, 5)
    assert torch.equal(eng.cf_tensors[1], torch.roll(labels["aS"], 1, 0)) and torch.equal(eng.cf_tensors[0], labels["aR"])
    with pytest.raises(ValueError, match="not a conditional-prior label"):
        m.intervention_moments(obs, 5, {"iext": torch.zeros(7, 1)}, **labels)


def test_an_argument_error_of_the_engine_call_is_not_composed_around():
    """ValueError from Engine.intervene_moments (a label tensor missing, a wrong shape) is the caller's error: it propagates, nothing is
    drawn and counterfactual_samples is not called."""
    m = _double(False, refuse=0)

    def bad(*a, **k):
        raise ValueError("cf label 0 is None")
    m._b.engine.intervene_moments = bad
    with pytest.raises(ValueError, match="cf label 0"):
        m.intervention_moments(torch.zeros(2, 3, 10), 5, {"iext": torch.ones(2, 1)}, iext=torch.zeros(2, 1), rtpr=torch.zeros(2, 1))
    assert m.sample_calls == [] and m._b.engine.draws == []


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.intervention_moments(torch.zeros(2, 3, 10), 5, {"iext": torch.ones(2, 1)}, iext=torch.zeros(2, 1), rtpr=torch.zeros(2, 1))
    assert m.sample_calls == [] and m._b.engine.draws == []


def test_save_intervention_moments_file_names(tmp_path):
    m = _double(False, refuse=0)
    labels = dict(iext=torch.zeros(2, 1), rtpr=torch.zeros(2, 1))
    files = m.save_intervention_moments(str(tmp_path / "r"), torch.zeros(2, 3, 10), 4, {"iext": torch.ones(2, 1), "rtpr": torch.ones(2, 1)}, **labels)
    want = sorted("%s_%s_iext+rtpr_sample_%s.npy" % (c, a, k) for c in ("mu_50", "mu_75", "mu_25") for a in ("cf", "effect") for k in ("mean", "sd"))
    assert sorted(os.path.basename(f) for f in files) == want
    assert all(np.load(f).shape == (2, 3, 10) for f in files)
