"""CPU tests of the counterfactual summaries: the C ABI of slode_intervene_summary / slode_intervene_summary_plan, the plan against a hand count
of the kernel's tables (a V that fits and one that does not), the refusal ladder on a hand-filled handle
(tests/intervene_summary_refusals/intervene_summary_refusals.cpp), the split arithmetic, every condition the GPU tests ask shown to hold for
the fp64 oracle alone (near share of both thresholds in every arm, mixed crossing, cells without a draw that crosses in both arms), the numpy
restatement of the three accumulations against fp64, and the Python layer on an engine double (the dict, the ValueErrors, the split, the
composed route, the files, the training flag)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import draws_ladder_util as DL
from tests import eval_stats_util as EU
from tests import intervene_summary_util as ISU
from tests import lds_util as LU
from tests import recon_moments_util as RU
from tests import summary_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "hyp_labels", "V", "group_mask", "num_samples", "thr", "sense", "f_mean", "f_sd",
        "cf_mean", "cf_sd", "eff_mean", "eff_sd", "workspace", "workspace_bytes", "stream"]


def test_abi_exports_intervene_summary_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_intervene_summary", "slode_intervene_summary_plan"):
        assert hasattr(lib, name) and name in L.EXPORTS
    version = re.search(r"#define\s+SLODE_VERSION\s+(\d+)\s*/\*(.*?)\*/", hdr)
    assert int(version.group(1)) == lib.slode_version() >= 290 and "slode_intervene_summary, slode_intervene_summary_plan" in version.group(2)
    for earlier in ("0.2.5: slode_curve_summary", "0.1.7: slode_intervene_moments", "0.2.1: slode_label_evidence"):
        assert earlier in hdr                                                             # the earlier version lines are kept
    m = re.search(r"int\s+slode_intervene_summary\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_intervene_summary.argtypes
    assert len(at) == len(ARGS) and at[8] is C.c_int and at[9] is C.c_uint and at[10] is C.c_int and at[12] is C.c_int and at[20] is C.c_size_t
    assert re.search(r"int\s+slode_intervene_summary_plan\s*\(\s*const slode_shape\*\s*s,\s*int V,\s*size_t\*\s*lds_bytes\s*\)\s*;", hdr)
    assert int(re.search(r"#define\s+SLODE_INTERVENE_SUMMARY_MAX_ARMS\s+(\d+)", hdr).group(1)) == L.INTERVENE_SUMMARY_MAX_ARMS == 64
    doc = hdr[hdr.index("counterfactual summaries as ONE call"):m.start()]
    for word in ("NULL handle", "num_samples < 1", "adaptive solver", "dopri5", "particles > 1", "SLODE_NO_FOLD", "SLODE_ODE_ALG", "LDS tables",
                 "SLODE_EINVAL", "n + 1", "POPULATION", "cf_mean NULL", "group_mask", "hyp_labels", "P_cf - P_f", "share of draws whose crossing",
                 "BOTH arms", "NaN", '"intervene_summary"', "sense", "no atomics", "half mirror", "slode_intervene_summary_plan", "bit for bit",
                 "bitwise independent of V", "largest V that fits", "slode_label_evidence", "slode_intervene_moments"):
        assert word in doc, word
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_INTERVENE_SUMMARY_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_intervene_summary_lds_bytes" in common
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "intervene_summary_kernel.hip" in srcs
    assert "slode_intervene_summary" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    profile_doc = hdr[:hdr.index("int slode_profile_read(")]
    assert '"intervene_summary"' in profile_doc[profile_doc.rindex("/*"):]                  # the launch name is documented at slode_profile_read
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_intervene_summary(*([None] * 8), 1, 0, 8, None, 1, *([None] * 7), 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_engine_signature():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.intervene_summary).parameters)[:16] == [
        "self", "params", "batch", "B", "hyp_labels", "V", "group_mask", "num_samples", "thr", "sense", "f_mean", "f_sd", "cf_mean", "cf_sd",
        "eff_mean", "eff_sd"]
    assert list(inspect.signature(Engine.intervene_summary_plan).parameters) == ["self", "B", "V"]


def _hand_count(eng, V):
    """The shared forward pieces (LU.spec_shared_floats), the posterior loc | scale 2 L, the V counterfactual loc | scale rows 2 L V, the grid
    T and the node weights T, the value table Q C T, the factual functionals Q C 8, the moment triples 3 Q C 8 (1 + 2 V) and slot 6's two
    counts per arm Q C 2 V; every piece rounded up to 16 bytes."""
    sp, T = eng.spec, eng.T
    Ld, QC = sp.latent_dim, (1 if sp.gauss else 3) * sp.n_channels
    return 4 * (LU.spec_shared_floats(sp, T) + 2 * LU.r4(Ld) + LU.r4(2 * Ld * V) + 2 * LU.r4(T) + LU.r4(QC * T) + LU.r4(QC * 8)
                + LU.r4(3 * QC * 8 * (1 + 2 * V)) + LU.r4(QC * 2 * V))


@pytest.mark.parametrize("case", list(EU.CASES))
def test_plan_against_a_hand_count_of_the_tables(case):
    eng = LU.host_engine(case)
    sp = eng.spec
    QC, Ld = (1 if sp.gauss else 3) * sp.n_channels, sp.latent_dim
    for V in (1, 3, 16):
        assert eng.intervene_summary_plan(8, V) == _hand_count(eng, V)
    # one more arm costs its loc | scale row, two sets of triples and two counts per curve (V = 4 -> 6: every piece stays a multiple of 16 B)
    assert eng.intervene_summary_plan(8, 6) - eng.intervene_summary_plan(8, 4) == 4 * 2 * (2 * Ld + 2 * 3 * QC * 8 + 2 * QC)


def test_plan_of_a_v_that_fits_and_one_that_does_not():
    """proc ALD (S = 8, C = 4, three heads): every arm costs 2 L + 2 x 3 x 12 x 8 + 24 floats.  On its own grid 48 arms fit and 49 do not;
    at T = 1024 the step table alone is 64 KB and the value table 48 KB: 8 arms fit."""
    from structured_latent_odes_amd import _lib as L
    for T, fit in ((None, 48), (1024, 8)):
        eng = LU.host_engine("proc_ald", T=T)
        assert eng.intervene_summary_plan(8, fit) == _hand_count(eng, fit) <= 160 * 1024 < _hand_count(eng, fit + 1)
        with pytest.raises(L.SlodeError, match=r"T = %d, S = 8, C = 4, V = %d \(%d B\) exceed the budget of 163840 B; at most V = %d fits"
                           % (eng.T, fit + 1, _hand_count(eng, fit + 1), fit)):
            eng.intervene_summary_plan(8, fit + 1)
    for V in (0, 65):
        with pytest.raises(L.SlodeError, match=r"V = %d out of range \[1, 64\]" % V):
            eng.intervene_summary_plan(8, V)
    assert LU.host_engine("cvs_ald").intervene_summary_plan(8, 64) <= 160 * 1024          # the metric shape takes all 64 arms


# case -> call column, status and the words its message must carry, written from include/slode.h in rung order
_N = "slode_intervene_summary"
_ADVICE = "reduce counterfactual samples instead"
_POST, _PLAN = ("post",), ("plan",)
_BIG = "T 1024, S 8, C 4"
_WS = ["workspace 64 B < required"]


def _post_only(rungs):
    """The rungs of slode_recon_moments' ladder on the posterior side alone: the call has no prior side."""
    return [(name, _POST, status, words) for name, cols, status, words in rungs if "post" in cols]


_HEAD, _LABELS, _TWO = (_post_only(r) for r in DL.shared_rungs(_N, "batch / times / stage_t / workspace", _ADVICE))
_LDS = [_N, "LDS tables", "T = 1024, S = 8, C = 4, V = 16 (169120 B", "moment triples", "at most V = 13 fits", "slode_intervene_summary_plan"]
LADDER = _HEAD + [
    ("cf_mean NULL", _POST, -1, [_N, "cf_mean is NULL"]), ("V 0", _POST, -1, [_N, "V = 0 out of range [1, 64]"]),
    ("V 65", _POST, -1, [_N, "V = 65 out of range [1, 64]"]), ("sense 0", _POST, -1, [_N, "sense = 0"]),
    ("thr[1] NaN", _POST, -1, [_N, "thr[1] = nan is not finite"]), ("thr[3] NaN beyond C = 3: not read; workspace too small", _POST, -3, _WS),
    ("group_mask bit 2 of 2 groups", _POST, -1, [_N, "group_mask = 0x4 has bits at or beyond n_groups = 2"]),
    ("mask 3, hyp_labels NULL", _POST, -1, [_N, "group_mask = 0x3 needs the hypothesis tables", "hyp_labels is NULL"]),
    ("mask 3, every table NULL", _POST, -1, [_N, "every entry of hyp_labels is NULL"]),
    ("mask 3, no label tensors", _POST, -1, [_N, "n_labels is 0"]),
    ("mask 1, only the table of group 1", _POST, -1, [_N, "no group of group_mask = 0x1 reads a column of a hypothesised label tensor"]),
    ("mask 0, hyp_labels NULL: taken so far; workspace too small", _POST, -3, _WS),
    ("LDS: %s, V 16" % _BIG, _POST, -1, _LDS), ("%s, V 1: fits; workspace too small" % _BIG, _POST, -3, _WS),
] + _LABELS[:-1] + [
    ("workspace too small", _POST, -3, _WS), ("every optional output and thr NULL, sense -1; workspace too small", _POST, -3, _WS),
] + _TWO + [                                                                          # two conditions at once: the earlier rung speaks
    ("no_fold + cf_mean NULL", _POST, -1, ["observation strides"]), ("cf_mean NULL + V 0", _POST, -1, ["cf_mean is NULL"]),
    ("V 0 + sense 0", _POST, -1, ["V = 0"]), ("sense 0 + thr[0] NaN", _POST, -1, ["sense = 0"]),
    ("thr[0] NaN + mask bit 2", _POST, -1, ["thr[0] = nan"]), ("mask bit 2 + hyp_labels NULL", _POST, -1, ["group_mask = 0x7 has bits"]),
    ("every table NULL + LDS", _POST, -1, ["every entry of hyp_labels is NULL"]), ("LDS + label columns 3", _POST, -1, ["LDS tables"]),
    ("label columns 3 + workspace too small", _POST, -1, ["label tensors have 3 columns"]),
    # the plan
    ("shape NULL", _PLAN, -1, ["slode_intervene_summary_plan", "shape is NULL"]), ("bad shape", _PLAN, -1, ["slode_intervene_summary_plan", "T out of range"]),
    ("lds_bytes NULL", _PLAN, -1, ["slode_intervene_summary_plan", "lds_bytes is NULL"]),
    ("V 0", _PLAN, -1, ["slode_intervene_summary_plan", "V = 0 out of range"]), ("V 65", _PLAN, -1, ["slode_intervene_summary_plan", "V = 65 out of range"]),
    ("LDS: %s, V 16" % _BIG, _PLAN, -1, ["slode_intervene_summary_plan", "LDS tables", "V = 16 (169120 B)", "at most V = 13 fits"]),
]


def test_intervene_summary_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_intervene_summary and of slode_intervene_summary_plan without a device, in rung order: status,
    the words of the message and the untouched drawing-call counter against LADDER; line by line against
    tests/golden/intervene_summary_refusals.txt; the rungs shared with slode_recon_moments carry the texts tests/golden/eval_refusals.txt
    records for it on the posterior side, the call's name, its list of required pointers and its advice apart; the call's LDS figure is the
    plan's; and the memory that stands for the outputs untouched."""
    _, shared, figures = DL.check_ladder("intervene_summary_refusals", tmp_path, LADDER, _N, _ADVICE, not_shared=("V 0", "V 65"))
    assert set().union(*figures.values()) == {"169120"}                                # the call's figure is the plan's
    assert shared >= 28


def test_split_arithmetic():
    """_fewest_calls on the plan: as few calls as fit, as even as that number allows, every hypothesis once and in order."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase as M
    eng = LU.host_engine("proc_ald")                                                      # 48 arms fit
    plan = lambda n: eng.intervene_summary_plan(8, n)                                     # noqa: E731
    assert M._fewest_calls(48, L.INTERVENE_SUMMARY_MAX_ARMS, plan) == [(0, 48)]
    assert M._fewest_calls(49, L.INTERVENE_SUMMARY_MAX_ARMS, plan) == [(0, 25), (25, 49)]
    assert M._fewest_calls(64, L.INTERVENE_SUMMARY_MAX_ARMS, plan) == [(0, 32), (32, 64)]
    assert M._fewest_calls(100, L.INTERVENE_SUMMARY_MAX_ARMS, plan) == [(0, 34), (34, 68), (68, 100)]
    assert M._fewest_calls(6, 2, plan) == [(0, 2), (2, 4), (4, 6)] and M._fewest_calls(1, 64, plan) == [(0, 1)]
    small = LU.host_engine("cvs_ald")
    assert M._fewest_calls(130, L.INTERVENE_SUMMARY_MAX_ARMS, lambda n: small.intervene_summary_plan(8, n)) == [(0, 44), (44, 88), (88, 130)]


# ---- the numpy restatement on rows whose moments are known -----------------------------------------------------------------------------------
def test_effect_moments_take_t_hit_over_the_draws_that_cross_in_both_arms():
    ff, fv = np.zeros((4, 2, 8), np.float32), np.zeros((4, 2, 8), np.float32)
    ff[:, 0, 6], ff[:, 0, 7] = [1.0, 2.0, np.nan, 3.0], [1, 1, 0, 1]
    fv[:, 0, 6], fv[:, 0, 7] = [np.nan, 5.0, 4.0, 8.0], [0, 1, 1, 1]
    ff[:, 1, 6], ff[:, 1, 7] = [np.nan, 2.0, np.nan, np.nan], [0, 1, 0, 0]                 # cell 1: exactly one draw crosses in both arms
    fv[:, 1, 6], fv[:, 1, 7] = [1.0, 2.5, np.nan, 3.0], [1, 1, 0, 1]
    ff[:, :, 0], fv[:, :, 0] = [[1, 5], [2, 5], [3, 5], [6, 5]], [[2, 5], [2, 5], [5, 5], [5, 5]]
    mean, sd = ISU.effect_moments_f32(ff, fv)
    assert mean[0, 6] == 4.0 and sd[0, 6] == 1.0                                           # draws 1 and 3: 3 and 5
    assert mean[0, 7] == 0.0 and sd[0, 7] == np.float32(np.sqrt(0.5))                      # -1, 0, +1, 0: half of the draws change
    assert float(sd[0, 7]) ** 2 + float(mean[0, 7]) ** 2 == pytest.approx(0.5, abs=1e-7)   # the identity of slot 7
    assert mean[1, 6] == 0.5 and sd[1, 6] == 0.0 and mean[1, 7] == 0.5
    assert mean[0, 0] == 0.5 and mean[1, 0] == 0.0 and sd[1, 0] == 0.0
    none_m, none_s = ISU.effect_moments_f32(ff[[0, 2]], fv[[0, 2]])                         # no draw crosses in both arms: NaN
    assert np.isnan(none_m[:, 6]).all() and np.isnan(none_s[:, 6]).all() and none_m[0, 7] == 0.0 and none_s[0, 7] == 1.0
    one_m, one_s = ISU.effect_moments_f32(ff[1:2], fv[1:2])                                 # one draw: sd exactly 0, the mean is the difference
    assert one_m[0, 6] == 3.0 and np.all(one_s == 0.0)


# ---- every condition the GPU tests assert, on the oracle alone ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(case):
    c = RU.build(case, "rk4", B=13, ns=7)
    vf, vcf = ISU.oracle(c, ISU.hypothesis_rows(c), ISU.FAMILY_MASK[c["fam"]])
    return c, vf, vcf


@pytest.mark.parametrize("case", list(EU.CASES))
def test_oracle_thresholds_have_few_near_points_and_mixed_crossing(case):
    """Threshold (a), the pooled median: nearly every draw crosses; (b), the median of the pooled peaks: 20 - 65 % of the draws cross and the
    crossing differs from the factual arm's in at least a tenth of the (draw, row, channel) cells.  Both: the points within one bar of the
    level are under the cap NEAR_SHARE in EVERY arm.  The arms are distinguishable: the largest |cf - f| is above 5."""
    c, vf, vcf = _oracle(case)
    times = c["times"].numpy()
    assert np.abs(vcf - vf[None]).max() > 5.0
    for kind in ("median", "peaks"):
        thr = ISU.thresholds(vf, vcf, kind)
        ff, fv = ISU.functionals64(vf, vcf, times, thr, 1)
        share, cross, differs = ISU.near_share(vf, vcf, thr), float(fv[..., 7].mean()), float((fv[..., 7] != ff[None][..., 7]).mean())
        print("%s %s: thr %s, near share %.2e, draws that cross %.2f, crossing differs %.2f" % (case, kind, thr, share, cross, differs))
        assert share <= SU.NEAR_SHARE
        if kind == "median":
            assert cross >= 0.75
        else:
            assert 0.2 <= cross <= 0.65 and differs >= 0.1


def test_oracle_has_cells_without_a_draw_that_crosses_in_both_arms():
    """The NaN branch of the effect's slot 6 and the single-draw branch (sd exactly 0) are exercised by the cases of the GPU tests 2 and 3."""
    none = one = 0
    for case in ("cvs_ald", "proc_gauss", "challenge_gauss"):
        c, vf, vcf = _oracle(case)
        ff, fv = ISU.functionals64(vf, vcf, c["times"].numpy(), ISU.thresholds(vf, vcf, "peaks"), 1)
        both = ((fv[..., 7] == 1) & (ff[None][..., 7] == 1)).sum(1)
        none, one = none + int((both == 0).sum()), one + int((both == 1).sum())
    assert none >= 3 and one >= 3


@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss", "challenge_gauss"])
def test_restatement_against_fp64_within_the_accumulation_bars(case):
    """The fp32 restatement of the three accumulations on the oracle's functionals rounded to fp32, against np.mean / np.std of the same
    fp32 values in fp64: within RU.accumulation_bars (slot 6 with the count of the draws it runs over); NaN exactly where fp64 has NaN."""
    c, vf, vcf = _oracle(case)
    ff, fv = ISU.functionals64(vf, vcf, c["times"].numpy(), ISU.thresholds(vf, vcf, "peaks"), 1)
    ff32, fv32 = RU._f32(ff), RU._f32(fv)
    got = ISU.restatement_f32(ff32, fv32)
    e32 = [RU._f32(ISU.effect64(ff32, a)) for a in fv32]                                   # (the kernel rounds the difference: fl(f_v - f_f))
    want = dict(f=SU.oracle_moments(ff32.astype(np.float64)), cf=tuple(np.stack(x) for x in zip(*[SU.oracle_moments(a.astype(np.float64)) for a in fv32])),
                eff=tuple(np.stack(x) for x in zip(*[SU.oracle_moments(e.astype(np.float64)) for e in e32])))
    worst = 0.0
    for n in ("f", "cf", "eff"):
        (gm, gs), (wm, ws) = got[n], want[n]
        assert np.array_equal(np.isnan(gm), np.isnan(wm)) and np.array_equal(np.isnan(gs), np.isnan(ws)), n
        bm, bs = RU.accumulation_bars(np.nan_to_num(wm), np.nan_to_num(ws), 7)
        ok = ~np.isnan(wm)
        em, es = np.abs(gm.astype(np.float64) - wm)[ok], np.abs(gs.astype(np.float64) - ws)[ok]
        tiny = 2.0 ** -24 * np.maximum(1.0, np.abs(wm[ok]))                                # (an sd of exactly 0 has no bar: compared at one ulp of the mean)
        assert np.all(em <= bm[ok] + tiny) and np.all(es <= bs[ok] + 4e-4 * np.sqrt(tiny)), n
        worst = max(worst, float((em / (bm[ok] + tiny)).max()))
    print("%s: restatement against fp64, worst mean error / bar %.3f" % (case, worst))


# ---- the Python layer on an engine double ---------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self, refuse, Q, fit=64):
        from structured_latent_odes_amd import _lib as L
        self.L, self.refuse, self.Q, self.fit = L, refuse, Q, fit
        self.calls, self.batches, self.draws, self.counter, self.rewinds = [], [], [], 10, []

    def draw_normal(self, rows):
        self.draws.append(rows)
        self.counter += 1
        return torch.linspace(-1.0, 1.0, rows * 4).view(rows, 4)

    def rng_state(self):
        return (0, 0, self.counter)

    def rng_set_counter(self, n):
        self.rewinds.append(n)
        self.counter = n

    def make_batch(self, obs, labels, eps=None, particles=1, eps_shape=None):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def intervene_summary_plan(self, B, V):
        if V > self.fit:
            raise self.L.SlodeError("at most V = %d fits" % self.fit)
        return 1024

    def intervene_summary(self, flat, bt, B, hyp, V, mask, num_samples, thr, sense, f_mean=None, f_sd=None):
        self.calls.append(([None if t is None else t.clone() for t in hyp], V, mask, num_samples, thr, sense, f_mean, f_sd))
        if self.refuse:
            err = self.L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        self.counter += 1
        f = torch.arange(8, dtype=torch.float32).view(1, 1, 1, 8) + 10.0 * torch.arange(self.Q, dtype=torch.float32).view(self.Q, 1, 1, 1) + torch.zeros(self.Q, B, 3, 8)
        # column v carries the first hypothesised value of its row: the split must put every column where its hypothesis stands
        tag = next(t for t in hyp if t is not None)[:, 0].view(V, 1, 1, 1, 1)
        cf = f.unsqueeze(0) + 1000.0 * tag
        return (None if f_mean is False else f), (None if f_sd is False else f + 0.5), cf, cf + 0.5, cf - f, cf - f + 0.25


def _double(gauss, refuse, fit=64):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        FAMILY, GAUSS = "cvs", gauss
        LABELS = ("iext", "rtpr")
        PRIORS = [("p_z_iext_given_iext", ["iext"], ["iext"]), ("p_z_rtprs_given_rtprs", ["rtpr"], ["rtpr"])]

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3, fit), "flat": torch.zeros(1)})()
            self.times = torch.tensor([0.0, 1.0, 3.0, 4.0, 8.0, 9.0])
            self.label_dims = {"iext": 1, "rtpr": 1}
            self.sampled = []

        def _bind(self):
            return self._b

        def counterfactual_samples(self, observations, num_samples, intervene, eps=None, **labels):
            """factual = (t - 4)^2 / 4 - eps[., ., 0] on channel 0, its negative on channel 1, a constant 1 on channel 2 (+ 100 per head);
            counterfactual = factual scaled by (1 + the hypothesised iext) and lowered by the hypothesised rtpr (own labels where not named)."""
            self.sampled.append((observations.shape[0], num_samples, sorted(intervene)))
            e = eps[:, :, 0].permute(1, 0).reshape(-1, 1, 1, num_samples)
            base = ((self.times - 4.0) ** 2 / 4.0).view(1, 1, 6, 1) - e
            v = torch.cat([base, -base, torch.ones_like(base)], 1)
            u = {l: intervene.get(l, labels[l]).reshape(-1, 1, 1, 1) for l in ("iext", "rtpr")}
            heads = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
            return {n: (v + 100.0 * i, v * (1.0 + u["iext"]) - u["rtpr"] + 100.0 * i) for i, n in enumerate(heads)}

    return M()


LABELS = dict(iext=torch.zeros(7, 1), rtpr=torch.ones(7, 1))
HYP = {"iext": torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0]])}


@pytest.mark.parametrize("gauss", [False, True])
def test_model_level_call_uses_the_engine_once_and_splits_on_the_same_noise(gauss, monkeypatch):
    obs = torch.zeros(7, 3, 6)
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, 0)
    eng = m._b.engine
    res = m.intervention_summary(obs, 5, HYP, thresholds=torch.tensor([1.0, 2.0, 3.0]), sense="below", **LABELS)
    assert len(eng.calls) == 1 and eng.batches == [((7, 3, 6), 2, None, 5)] and eng.draws == [] and eng.counter == 11
    hyp, V, mask, ns, thr, sense, f_mean, f_sd = eng.calls[0]
    assert (V, mask, ns, thr, sense, f_mean, f_sd) == (5, 1, 5, [1.0, 2.0, 3.0], -1, None, None) and hyp[1] is None and torch.equal(hyp[0], HYP["iext"])
    assert set(res) == set(names) | {"hypotheses"} and torch.equal(res["hypotheses"]["iext"], HYP["iext"])
    for q, n in enumerate(names):
        assert set(res[n]) == {"factual", "cf", "effect"} and all(set(res[n][a]) == set(SU.NAMES) for a in res[n])
        for j, k in enumerate(SU.NAMES):
            fm, fs = res[n]["factual"][k]
            cm, cs = res[n]["cf"][k]
            em, es = res[n]["effect"][k]
            assert tuple(fm.shape) == tuple(fs.shape) == (7, 3) and tuple(cm.shape) == tuple(cs.shape) == tuple(em.shape) == tuple(es.shape) == (5, 7, 3)
            assert float(fm[0, 0]) == 10.0 * q + j and float(fs[0, 0]) == 10.0 * q + j + 0.5
            assert cm[:, 0, 0].tolist() == [10.0 * q + j + 1000.0 * (v + 1) for v in range(5)] and em[:, 0, 0].tolist() == [1000.0 * (v + 1) for v in range(5)]
            assert float(es[2, 0, 0]) == 3000.25
    # both groups named: mask 3; no thresholds: None reaches the engine
    m.intervention_summary(obs, 5, {"rtpr": [[0.0], [1.0]], "iext": [[1.0], [0.0]]}, eps=torch.zeros(5, 7, 4), **LABELS)
    assert eng.calls[-1][1:6] == (2, 3, 5, None, 1) and eng.batches[-1] == ((7, 3, 6), 2, (5, 7, 4), 5)
    # the split: a cap of 2 gives 2 + 2 + 1 on the same noise -- every call rewound to the first call's counter, the factual moments asked once
    monkeypatch.setattr(type(m), "INTERVENTION_SUMMARY_ARMS_PER_CALL", 2)
    eng.calls.clear()
    eng.counter = 20
    split = m.intervention_summary(obs, 5, HYP, thresholds=[1.0, 2.0, 3.0], sense="below", **LABELS)
    assert [(c[1], c[0][0][:, 0].tolist(), c[6]) for c in eng.calls] == [(2, [1.0, 2.0], None), (2, [3.0, 4.0], False), (1, [5.0], False)]
    assert eng.rewinds[-3:] == [20, 20, 20] and eng.counter == 21
    for n in names:
        for arm in ("factual", "cf", "effect"):
            assert all(torch.equal(a, b) for k in SU.NAMES for a, b in zip(split[n][arm][k], res[n][arm][k])), (n, arm)
    # what the LDS holds decides the same way: a plan that takes 3 arms splits 5 into 3 + 2
    monkeypatch.setattr(type(m), "INTERVENTION_SUMMARY_ARMS_PER_CALL", None)
    eng.fit = 3
    eng.calls.clear()
    m.intervention_summary(obs, 5, HYP, **LABELS)
    assert [c[1] for c in eng.calls] == [3, 2]


def test_value_errors_come_before_any_engine_call():
    m = _double(False, 0)
    obs = torch.zeros(7, 3, 6)
    for bad, match in ((dict(hypotheses={}), "must name at least one label"), (dict(hypotheses={"symptoms": [[0.0]]}), "not a label of the cvs family"),
                       (dict(hypotheses={"iext": [[0.0], [1.0]], "rtpr": [[0.0]]}), "every table needs the same V"),
                       (dict(hypotheses={"iext": [[0.0, 1.0]]}), r"must be \[V, 1\]"), (dict(sense="up"), "sense"),
                       (dict(thresholds=[1.0, 2.0]), "one per channel"), (dict(num_samples=0), "num_samples")):
        kw = dict(dict(num_samples=5, hypotheses=HYP), **bad)
        with pytest.raises(ValueError, match=match):
            m.intervention_summary(obs, **kw, **LABELS)
    # a label of the family that no conditional prior reads: _intervened's error text
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase
    type(m).LABELS = ("iext", "rtpr", "age")
    m.label_dims["age"] = 1
    with pytest.raises(ValueError, match="intervene: 'age' is not a conditional-prior label of the cvs family"):
        m.intervention_summary(obs, 5, {"age": [[1.0]]}, age=torch.zeros(7, 1), **LABELS)
    assert m._b.engine.calls == [] and m._b.engine.draws == [] and issubclass(type(m), MechanisticBase)


@pytest.mark.parametrize("gauss", [False, True])
def test_composed_route_on_a_refusal(gauss, monkeypatch):
    """The engine refuses (status -1): one drawing call for the whole batch, counterfactual_samples per hypothesis and chunk, the functionals
    and the paired rules in torch -- equal to the numpy restatement on the same curves (t_hit of an effect over the draws that cross in both
    arms), independent of the chunking."""
    obs = torch.zeros(7, 3, 6)
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, -1)
    eng = m._b.engine
    thr, hyp = [0.5, -0.5, 1.0], {"iext": [[0.0], [1.0]], "rtpr": [[1.0], [3.0]]}
    res = m.intervention_summary(obs, 5, hyp, thresholds=thr, sense="above", **LABELS)
    assert len(eng.calls) == 1 and eng.draws == [35] and m.sampled == [(7, 5, ["iext", "rtpr"])] * 2 and eng.counter == 11
    eps = torch.linspace(-1.0, 1.0, 35 * 4).view(5, 7, 4)
    times = m.times.numpy()
    for v in range(2):
        swap = {l: torch.tensor(t[v:v + 1]).expand(7, -1) for l, t in hyp.items()}
        curves = m.counterfactual_samples(obs, 5, swap, eps=eps, **LABELS)
        for n in names:
            f_f, f_v = (SU.functionals(curves[n][a].permute(3, 0, 1, 2).numpy(), times, np.array(thr, np.float32), 1) for a in (0, 1))
            for arm, f, col in (("factual", f_f, None), ("cf", f_v, v), ("effect", f_v - f_f, v)):
                wm, ws = SU.oracle_moments(f)
                for j, k in enumerate(SU.NAMES):
                    gm, gs = (t.double().numpy() if col is None else t[col].double().numpy() for t in res[n][arm][k])
                    assert np.allclose(gm, wm[..., j], rtol=1e-5, atol=1e-5, equal_nan=True), (n, arm, k)
                    assert np.allclose(gs, ws[..., j], rtol=1e-4, atol=1e-4, equal_nan=True), (n, arm, k)
    r = res[names[0]]
    # hypothesis 0 (iext 0, rtpr 1 = every subject's own labels... but for rtpr lowering the curve by 1): channel 2 is the constant 1 - 1 = 0
    assert float(r["cf"]["peak"][0][0, 0, 2]) == 0.0 and float(r["effect"]["peak"][0][0, 0, 2]) == -1.0 and float(r["effect"]["peak"][1][0, 0, 2]) == 0.0
    assert torch.isnan(r["effect"]["t_hit"][0][:, :, 2]).all() and float(r["effect"]["crossed"][0][0, 0, 2]) == 0.0    # 1 > 1 is false in both arms
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)                                  # 15 // 5 = 3 rows per chunk: 3 + 3 + 1
    m.sampled.clear()
    chunked = m.intervention_summary(obs, 5, hyp, thresholds=thr, sense="above", **LABELS)
    assert [s[0] for s in m.sampled] == [3, 3, 3, 3, 1, 1] and eng.draws == [35, 35]
    for n in names:
        for arm in ("factual", "cf", "effect"):
            for k in SU.NAMES:
                assert all(torch.equal(a.nan_to_num(nan=7e33), b.nan_to_num(nan=7e33)) for a, b in zip(chunked[n][arm][k], res[n][arm][k])), (n, arm, k)
    none = m.intervention_summary(obs, 5, hyp, **LABELS)
    assert all(torch.isnan(none[n][arm][k][0]).all() for n in names for arm in ("factual", "cf", "effect") for k in ("time_beyond", "t_hit", "crossed"))


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.intervention_summary(torch.zeros(7, 3, 6), 5, HYP, **LABELS)
    assert m.sampled == [] and m._b.engine.draws == []


def test_save_intervention_summary_files_and_lines(tmp_path):
    m = _double(False, 0)
    batches = [dict(observations=torch.zeros(B, 3, 6), iext=torch.zeros(B, 1), rtpr=torch.zeros(B, 1)) for B in (2, 3)]
    files = m.save_intervention_summary(str(tmp_path / "r"), batches, 4, HYP, thresholds=[1.0, 2.0, 3.0], sense="below")
    want = ["summary_%s_%s_%s.npy" % (n, a, k) for n in ("mu_50", "mu_75", "mu_25") for a in ("factual", "cf", "effect") for k in ("mean", "sd")]
    want += ["summary_hypotheses_iext.npy"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "r"))) == sorted(want)
    assert np.array_equal(np.load(files[-1]), HYP["iext"].numpy())
    f_mean, f_sd, cf_mean, _, eff_mean, eff_sd = (np.load(f) for f in files[:6])
    assert f_mean.shape == f_sd.shape == (5, 3, 8) and cf_mean.shape == eff_mean.shape == eff_sd.shape == (5, 5, 3, 8) and f_mean.dtype == np.float32
    assert f_mean[0, 0].tolist() == list(range(8)) and f_sd[0, 0, 0] == 0.5 and cf_mean[4, 2, 0, 1] == 3001.0 and eff_mean[4, 2, 0].tolist() == [3000.0] * 8
    lines = m.intervention_summary_lines(eff_mean, HYP, True)
    assert len(lines) == 5 and lines[1].startswith("intervention_summary: iext=[2.0]  n=5  c0 d_peak=2000 d_auc=2000 d_p_cross=2000.000") and " c2 d_peak=" in lines[1]
    assert "d_p_cross" not in m.intervention_summary_lines(eff_mean, HYP, False)[0]


def test_training_entry_points_take_the_flag():
    import inspect
    from structured_latent_odes_amd import training as TR
    assert inspect.signature(TR.train).parameters["intervention_summary"].default == 0
    a = TR.build_parser().parse_args(["--intervention-summary", "64", "--summary-thresholds", "0.5,1,2.5", "--summary-sense", "below"])
    assert (a.intervention_summary, a.summary_thresholds, a.summary_sense) == (64, [0.5, 1.0, 2.5], "below")
    assert TR.build_parser().parse_args([]).intervention_summary == 0
    for script in ("training_cvs.py", "training_challenge.py", "training_proc.py"):
        assert "main(" in open(os.path.join(ROOT, script)).read()                           # the three entry points run training.main: its parser
