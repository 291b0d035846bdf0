"""GPU tests of the counterfactual summaries (slode_intervene_summary; Engine.intervene_summary; MechanisticModel.intervention_summary).

What is exact and what has a bar (tests/intervene_summary_util.py): the factual set is held to slode_curve_summary(is_post = 1) on the same
noise with torch.equal; per draw (num_samples = 1) an arm's slots 0 - 3, 6, 7 are held to numpy on the curve slode_intervene_moments returns
for that hypothesis EXACTLY, its two sums to the summation bar, and the effect to the fp32 difference of the two per-draw rows exactly; the
three sets of moments over K = 7 draws are held to the numpy restatement of the shifted accumulations bitwise; column v of a V-arm call to
the V = 1 call with that row with torch.equal.  Against the fp64 oracle the factual and cf sets have the rules of the curve summaries and
the effects the sum of the two arms' bars, nothing excluded.  Outputs are pre-filled with a sentinel: every element must be written."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import intervene_summary_util as ISU
from tests import recon_moments_util as RU
from tests import summary_util as SU
from tests.eval_gpu_util import (ADAPTIVE, DEV, ENV_KEYS, FILL, SIZES, WIDTHS, _captured, _count_calls, _device_batch, _engine, _eps_dev, _iv, _label_split, _model,
                                 _padded, _peak, _refused, _same as _same_arrays, _summary)

pytestmark = pytest.mark.gpu
_same = functools.partial(_same_arrays, equal_nan=True)
NAMES = ("f_mean", "f_sd", "cf_mean", "cf_sd", "eff_mean", "eff_sd")


def _ivs(eng, flat, c, hyp_u, mask, thr, sense=1, eps="case", ns=None, want=NAMES, obs_d=None, labels=None):
    """Engine.intervene_summary on the case's batch with the hypothesis rows hyp_u [V, n_u] (None: no tables) -> dict of numpy arrays; the
    outputs in ``want`` pre-filled with FILL and fully written, the others passed as NULL."""
    if obs_d is None:
        obs_d, labels = _device_batch(c)
    ns = ns or c["ns"]
    e = _eps_dev(c["eps"]) if isinstance(eps, str) else eps
    Q, Cn, B = (1 if c["ospec"].gauss else 3), c["obs"].shape[1], c["B"]
    V = 1 if hyp_u is None else hyp_u.shape[0]
    outs = {n: (torch.full(((Q, B, Cn, 8) if n[0] == "f" else (V, Q, B, Cn, 8)), FILL, device=DEV) if n in want else False) for n in NAMES}
    hyp = None if hyp_u is None else _label_split(c, hyp_u)
    got = eng.intervene_summary(flat, eng.make_batch(obs_d, labels, e, particles=ns), B, hyp, V, mask, ns, None if thr is None else [float(x) for x in thr],
                                sense, **outs)
    res = {n: (None if t is None else t.cpu().numpy()) for n, t in zip(NAMES, got)}
    assert all((res[n] is None) == (n not in want) for n in NAMES)
    assert all(t is None or not (t == FILL).any() for t in res.values()), "an output element was not written"
    return res


@functools.lru_cache(maxsize=None)
def _case(case):
    """Computed once per case, shared by tests 1 - 5: B = 13, K = 7, explicit eps, V = 3 hypothesis rows over every prior group; the
    oracle's arms and the two thresholds; per draw (num_samples = 1) the three sets at threshold (b), sense +1."""
    c = RU.build(case, "rk4", B=13, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    hyp, mask = ISU.hypothesis_rows(c), ISU.FAMILY_MASK[c["fam"]]
    vf, vcf = ISU.oracle(c, hyp, mask)
    thr = {kind: ISU.thresholds(vf, vcf, kind) for kind in ("median", "peaks")}
    eps = c["eps"].to(DEV)
    rows = [_ivs(eng, flat, c, hyp, mask, thr["peaks"], 1, eps=eps[k].contiguous(), ns=1, obs_d=obs_d, labels=labels) for k in range(7)]
    return dict(c=c, eng=eng, flat=flat, obs_d=obs_d, labels=labels, hyp=hyp, mask=mask, thr=thr, rows=rows, vf=vf, vcf=vcf)


CASES3 = ["cvs_ald", "proc_gauss", "challenge_gauss"]


@pytest.mark.parametrize("case", CASES3)
def test_factual_arm_is_curve_summary_bit_for_bit(case):
    """(1) f_mean / f_sd equal slode_curve_summary(is_post = 1) on the same explicit noise: both thresholds, both senses, and without one."""
    s = _case(case)
    c, eng, flat = s["c"], s["eng"], s["flat"]
    for thr in (s["thr"]["median"], s["thr"]["peaks"], None):
        for sense in (1, -1):
            got = _ivs(eng, flat, c, s["hyp"], s["mask"], thr, sense)
            mean, sd, _ = _summary(eng, flat, c, True, thr, sense, p=False)
            assert torch.equal(torch.from_numpy(got["f_mean"]).nan_to_num(nan=7e33), torch.from_numpy(mean).nan_to_num(nan=7e33)), (case, sense)
            assert _same(got["f_mean"], mean) and _same(got["f_sd"], sd), (case, sense)
            if thr is None:
                assert all(np.isnan(got[n][..., 5:]).all() for n in NAMES)


@pytest.mark.parametrize("case", CASES3)
def test_per_draw_exactness_against_the_counterfactual_curves(case):
    """(2) num_samples = 1, every arm: cf_mean slots 0 - 3, 6, 7 equal numpy's on the curve slode_intervene_moments(ns = 1) returns as
    cf_mean for that hypothesis row given to every trajectory; slots 4 and 5 within SU.sum_bars; eff_mean is the fp32 difference of the two
    per-draw rows exactly (slot 6 NaN unless both cross) and every sd that is not NaN is exactly 0."""
    s = _case(case)
    c, eng, flat = s["c"], s["eng"], s["flat"]
    times, thr = c["times"].numpy(), s["thr"]["peaks"]
    eps = c["eps"].to(DEV)
    for k in range(7):
        row = s["rows"][k]
        for v in range(ISU.V):
            u_cf = s["hyp"][v:v + 1].expand(c["B"], -1).contiguous()
            curve = _iv(eng, flat, c, s["mask"], u_cf, eps=eps[k].contiguous(), obs_d=s["obs_d"], labels=s["labels"], ns=1)[0].cpu().numpy()
            want = SU.functionals(curve, times, thr, 1)
            got = row["cf_mean"][v]
            for slot in (0, 1, 2, 3, 6, 7):
                assert np.array_equal(got[..., slot].astype(np.float64), want[..., slot], equal_nan=True), (case, k, v, SU.NAMES[slot])
            bar_auc, bar_tb = SU.sum_bars(curve, times)
            assert (np.abs(got[..., 4] - want[..., 4]) / bar_auc).max() <= 1.0 and (np.abs(got[..., 5] - want[..., 5]) / bar_tb).max() <= 1.0
            f = row["f_mean"]
            e = RU._f32(got - f)
            e[..., 6] = np.where(np.isnan(got[..., 6]) | np.isnan(f[..., 6]), np.float32("nan"), e[..., 6])
            assert _same(row["eff_mean"][v], e), (case, k, v)
        for n in ("f", "cf", "eff"):
            sd, mean = row[n + "_sd"], row[n + "_mean"]
            assert np.array_equal(np.isnan(sd), np.isnan(mean)) and np.all(sd[~np.isnan(sd)] == 0.0), (case, k, n)


def test_moments_over_draws_bitwise():
    """(3) One call with num_samples = 7 equals the numpy restatement of the three accumulations on the per-draw rows bitwise (slot 6 of an
    arm over its crossing draws, of an effect over the draws that cross in both arms).  Over the three cases there is a cell where no
    draw crosses in both arms (NaN) and one where exactly one does (sd exactly 0)."""
    none = one = 0
    for case in CASES3:
        s = _case(case)
        got = _ivs(s["eng"], s["flat"], s["c"], s["hyp"], s["mask"], s["thr"]["peaks"], 1)
        ff = np.stack([r["f_mean"] for r in s["rows"]])                                      # [ns, Q, B, C, 8]
        fv = np.stack([np.stack([r["cf_mean"][v] for r in s["rows"]]) for v in range(ISU.V)])   # [V, ns, Q, B, C, 8]
        want = ISU.restatement_f32(ff, fv)
        for n in ("f", "cf", "eff"):
            for j, kind in enumerate(("mean", "sd")):
                g, w = got["%s_%s" % (n, kind)], want[n][j]
                assert _same(g, w), (case, n, kind, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
        both = ((fv[..., 7] == 1) & (ff[None][..., 7] == 1)).sum(1)                           # [V, Q, B, C]
        assert np.array_equal(np.isnan(got["eff_mean"][..., 6]), both == 0) and np.all(got["eff_sd"][..., 6][both == 1] == 0.0)
        # the identity of slot 7: sd^2 + mean^2 is the share of draws whose crossing changes
        changed = (fv[..., 7] != ff[None][..., 7]).mean(1)
        assert np.abs(got["eff_sd"][..., 7].astype(np.float64) ** 2 + got["eff_mean"][..., 7].astype(np.float64) ** 2 - changed).max() <= 1e-6
        none, one = none + int((both == 0).sum()), one + int((both == 1).sum())
        print("%s: cells with no draw crossing in both arms %d, with exactly one %d, crossing differs in %.2f of the (draw, cell)s"
              % (case, int((both == 0).sum()), int((both == 1).sum()), float((fv[..., 7] != ff[None][..., 7]).mean())))
    assert none > 0 and one > 0


@pytest.mark.parametrize("case", CASES3)
def test_no_group_intervened(case):
    """(4) group_mask = 0: cf == f bitwise in every column, every effect is exactly 0, and slot 6's NaN pattern is the factual one."""
    s = _case(case)
    for hyp in (s["hyp"], None):
        got = _ivs(s["eng"], s["flat"], s["c"], hyp, 0, s["thr"]["peaks"], 1)
        for v in range(got["cf_mean"].shape[0]):
            assert _same(got["cf_mean"][v], got["f_mean"]) and _same(got["cf_sd"][v], got["f_sd"])
            nan6 = np.isnan(got["f_mean"][..., 6])
            assert np.array_equal(np.isnan(got["eff_mean"][v][..., 6]), nan6) and np.array_equal(np.isnan(got["eff_sd"][v][..., 6]), nan6)
            for n in ("eff_mean", "eff_sd"):
                e = got[n][v].copy()
                e[..., 6] = np.where(nan6, 0.0, e[..., 6])
                assert np.all(e == 0.0), (case, n)


def test_column_independence_and_the_model_level_split(monkeypatch):
    """(5) V = 5 against five V = 1 calls with torch.equal; permuted hypotheses give permuted columns; the model-level split (cap forced to
    2) equals the single call."""
    s = _case("cvs_ald")
    c, eng, flat = s["c"], s["eng"], s["flat"]
    thr = s["thr"]["peaks"]
    hyp5 = ISU.hypothesis_rows(c, rows=[0, 4, 2, 9, 12])
    all5 = _ivs(eng, flat, c, hyp5, s["mask"], thr, 1)
    for v in range(5):
        one = _ivs(eng, flat, c, hyp5[v:v + 1], s["mask"], thr, 1)
        for n in NAMES:
            a, b = (one[n], all5[n]) if n[0] == "f" else (one[n][0], all5[n][v])
            assert torch.equal(torch.from_numpy(a).nan_to_num(nan=7e33), torch.from_numpy(b).nan_to_num(nan=7e33)) and _same(a, b), (v, n)
    perm = [3, 0, 4, 1, 2]
    shuffled = _ivs(eng, flat, c, hyp5[perm], s["mask"], thr, 1)
    for n in NAMES[2:]:
        assert _same(shuffled[n], all5[n][perm]), n
    m, batch = _model("cvs")
    meng = m._bind().engine
    B = batch["observations"].shape[0]
    hyp = m.label_grid(iext=[0.0, 1.0, 0.5], rtpr=[0.0, 1.0])                                  # V = 6
    eps = torch.randn(5, B, meng.spec.latent_dim, generator=torch.Generator().manual_seed(3)).to(DEV)
    calls = _count_calls(monkeypatch, meng, "intervene_summary", note=lambda a: a[4])
    whole = m.intervention_summary(num_samples=5, hypotheses=hyp, thresholds=[0.4, 0.4, 0.4], eps=eps, **batch)
    assert calls == [6]
    monkeypatch.setattr(type(m), "INTERVENTION_SUMMARY_ARMS_PER_CALL", 2)
    calls.clear()
    split = m.intervention_summary(num_samples=5, hypotheses=hyp, thresholds=[0.4, 0.4, 0.4], eps=eps, **batch)
    assert calls == [2, 2, 2]
    for n in m.MOMENT_HEADS[bool(m.GAUSS)]:
        for arm in ("factual", "cf", "effect"):
            for k in SU.NAMES:
                for a, b in zip(whole[n][arm][k], split[n][arm][k]):
                    assert a.shape == b.shape and torch.equal(a.nan_to_num(nan=7e33), b.nan_to_num(nan=7e33)), (n, arm, k)
    # drawn noise: the split leaves the counter where one call does, and draws the same rows
    meng.rng_seed(9)
    meng.rng_set_counter(3)
    drawn = m.intervention_summary(num_samples=5, hypotheses=hyp, thresholds=[0.4, 0.4, 0.4], **batch)
    assert meng.rng_state() == (9, 0, 4)
    rows = meng.rng_normal(3, 5 * B).view(5, B, -1)
    given = m.intervention_summary(num_samples=5, hypotheses=hyp, thresholds=[0.4, 0.4, 0.4], eps=rows, **batch)
    n0 = m.MOMENT_HEADS[bool(m.GAUSS)][0]
    assert all(torch.equal(a.nan_to_num(nan=7e33), b.nan_to_num(nan=7e33)) for k in SU.NAMES for a, b in zip(drawn[n0]["effect"][k], given[n0]["effect"][k]))


def _against_the_oracle(eng, flat, c, tag, V=ISU.V, kinds=("median", "peaks")):
    """(6) factual and cf by SU.check_continuous and, per draw, SU.tolerant_violations (unchanged); the effects by ISU.check_effect."""
    times = c["times"].numpy()
    span = float(times[-1] - times[0])
    ns = c["ns"]
    obs_d, labels = _device_batch(c)
    hyp, mask = ISU.hypothesis_rows(c, V), ISU.FAMILY_MASK[c["fam"]]
    vf, vcf = ISU.oracle(c, hyp, mask)
    for kind in kinds:
        thr = ISU.thresholds(vf, vcf, kind)
        share = ISU.near_share(vf, vcf, thr)
        assert share <= SU.NEAR_SHARE, (tag, kind, share)
        for sense in (1, -1):
            t = "%s %s sense %d" % (tag, kind, sense)
            got = {k: x.astype(np.float64) for k, x in _ivs(eng, flat, c, hyp, mask, thr, sense, obs_d=obs_d, labels=labels).items()}
            ff, fv = ISU.functionals64(vf, vcf, times, thr, sense)
            want = ISU.oracle_moments(ff, fv)
            SU.check_continuous(got["f_mean"], got["f_sd"], want["f"][0], want["f"][1], np.abs(vf).max(-1).max(1), span, t + " factual")
            for v in range(V):
                SU.check_continuous(got["cf_mean"][v], got["cf_sd"][v], want["cf"][0][v], want["cf"][1][v], np.abs(vcf[v]).max(-1).max(1), span, t + " cf %d" % v)
                near = SU.near(np.moveaxis(vcf[v], 1, 0), thr).any(-1).sum(0) / ns
                assert np.all(np.abs(got["cf_mean"][v][..., 7] - want["cf"][0][v][..., 7]) <= near + 1e-6), t
            ISU.check_effect(got["eff_mean"], got["eff_sd"], want["eff"], ff, fv, vf, vcf, times, thr, ns, t)
    return hyp, mask, vf, vcf, thr


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_against_the_fp64_oracle(case, solver):
    c = RU.build(case, solver, B=13, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    hyp, mask, vf, vcf, thr = _against_the_oracle(eng, flat, c, "%s/%s" % (case, solver))
    # the discontinuous slots of every arm, per draw, by the tolerant rules: nothing excluded
    times = c["times"].numpy()
    obs_d, labels = _device_batch(c)
    eps = c["eps"].to(DEV)
    rows = [_ivs(eng, flat, c, hyp, mask, thr, 1, eps=eps[k].contiguous(), ns=1, want=("f_mean", "cf_mean"), obs_d=obs_d, labels=labels) for k in range(7)]
    for arm, v64 in [("factual", vf)] + [("cf %d" % v, vcf[v]) for v in range(ISU.V)]:
        got = np.stack([r["f_mean"] if arm == "factual" else r["cf_mean"][int(arm[3:])] for r in rows]).astype(np.float64)
        bad = SU.tolerant_violations(got, np.moveaxis(v64, 1, 0), times, thr, 1)
        assert all(n == 0 for _, n in bad), (case, solver, arm, bad)


@pytest.mark.parametrize("case,B,ns,env", SIZES, ids=["%s-B%d-ns%d%s" % (c, B, ns, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, ns, e in SIZES])
def test_sizes_and_instantiations(case, B, ns, env, monkeypatch):
    """(7) B on both sides of the 64- and 256-thread edges, the persistent loop, the run-time-S build, ns in {1, 2, 7, 200}; V = 2;
    NaN-poisoned workspace, pre-filled outputs."""
    c = RU.build(case, "rk4", B=B, ns=ns)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    _against_the_oracle(eng, flat, c, "%s B=%d ns=%d %s" % (case, B, ns, env), V=2, kinds=("median",))


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_noise_and_independence(case, monkeypatch):
    """(8) In-kernel noise equals the same rows passed explicitly, bitwise, and the counter ends at n + 1; two grids are bitwise equal; a
    repeat is bitwise equal; every subset of the optional outputs leaves the others bitwise unchanged (cf alone: the factual arm is not run)."""
    c = RU.build(case, "midpoint", B=13, ns=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    hyp, mask = ISU.hypothesis_rows(c), ISU.FAMILY_MASK[c["fam"]]
    thr = ISU.thresholds(*ISU.oracle(c, hyp, mask), "peaks")
    a = _ivs(eng, flat, c, hyp, mask, thr)
    for other in (_ivs(eng, flat, c, hyp, mask, thr), _ivs(loop, flat, c, hyp, mask, thr)):
        assert all(_same(a[n], other[n]) for n in NAMES)
    for want in (("cf_mean",), ("cf_mean", "cf_sd"), ("cf_mean", "eff_sd"), ("f_sd", "cf_mean"), ("f_mean", "cf_mean", "eff_mean")):
        lean = _ivs(eng, flat, c, hyp, mask, thr, want=want)
        assert all(_same(lean[n], a[n]) for n in want), want
    for e in (eng, loop):
        e.rng_seed(77, first_trajectory=1000)
        e.rng_set_counter(5)
    drawn = _ivs(eng, flat, c, hyp, mask, thr, eps=None)
    assert eng.rng_state() == (77, 1000, 6)
    rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
    given = _ivs(eng, flat, c, hyp, mask, thr, eps=rows)
    assert eng.rng_state() == (77, 1000, 6)                                       # explicit noise draws nothing
    drawn_loop = _ivs(loop, flat, c, hyp, mask, thr, eps=None)
    assert all(_same(drawn[n], given[n]) and _same(drawn[n], drawn_loop[n]) for n in NAMES)


def test_launches_and_graph_capture():
    """(9) "weff", "enc_fwd2", "intervene_summary" on one stream; one capture and one replay equal the stream-launched call bitwise;
    capturing executes nothing (threshold and tables travel by value / by device pointer: nothing is read from the host at replay)."""
    s = _case("cvs_ald")
    c, eng, flat = s["c"], s["eng"], s["flat"]
    thr = [float(x) for x in s["thr"]["peaks"]]
    eng.profile_enable(True)
    _ivs(eng, flat, c, s["hyp"], s["mask"], thr)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "intervene_summary"]
    eng.profile_enable(False)
    B = c["B"]
    outs = [torch.zeros(3, B, 3, 8, device=DEV) for _ in range(2)] + [torch.zeros(ISU.V, 3, B, 3, 8, device=DEV) for _ in range(4)]
    bt = eng.make_batch(s["obs_d"], s["labels"], c["eps"].to(DEV).contiguous(), particles=7)
    hyp = _label_split(c, s["hyp"])
    want = _captured(lambda: eng.intervene_summary(flat, bt, B, hyp, ISU.V, s["mask"], 7, thr, 1, *outs), outs)
    assert all(_same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(outs, want)) and float(outs[2].nan_to_num().abs().max()) > 0.0


def test_refusals_by_name(monkeypatch):
    """(10) Every refusal names its reason, draws nothing and launches nothing (rng_state, profile_read)."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd import engine as E
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)
    rows = ISU.hypothesis_rows(c)

    def refused(eng, match, obs=obs_d, ns=2, particles=1, null_obs=False, thr=(0.1, 0.2, 0.3), sense=1, V=3, mask=3, hyp="rows", error=None):
        flat = eng.pack(c["p"])
        bt = eng.make_batch(obs, labels, None)
        if null_obs:
            bt.obs = None
        h = _label_split(c, rows[:max(V, 1)]) if hyp == "rows" else hyp
        err = _refused(eng, lambda: eng.intervene_summary(flat, bt, c["B"], h, V, mask, ns, thr, sense, particles=particles), match, error=error)
        assert error is not None or (err.status == -1 and "slode_intervene_summary" in str(err))

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s .*reduce counterfactual samples instead" % solver)
    eng = _engine(c, monkeypatch)
    refused(eng, "particles = 2", particles=2)
    refused(eng, "num_samples = 0", ns=0)
    refused(eng, "V = 0 out of range \\[1, 64\\]", V=0, hyp=None, mask=0)
    refused(eng, "V = 65 out of range \\[1, 64\\]", V=65, hyp=None, mask=0)
    refused(eng, "sense = 0", sense=0)
    refused(eng, "thr\\[1\\] = nan is not finite", thr=(0.1, float("nan"), 0.3))
    refused(eng, "group_mask = 0x4 has bits at or beyond n_groups = 2", mask=4)
    refused(eng, "group_mask = 0x1 needs the hypothesis tables \\(hyp_labels is NULL\\)", mask=1, hyp=None)
    refused(eng, "every entry of hyp_labels is NULL", mask=1, hyp=[None, None])
    refused(eng, "no group of group_mask = 0x1 reads a column of a hypothesised label tensor", mask=1, hyp=[None, _label_split(c, rows)[1]])
    refused(eng, "one per channel", thr=(0.1, 0.2), error=ValueError)
    refused(eng, "batch->obs is NULL", null_obs=True)
    refused(eng, "observation strides", obs=_padded(obs_d))
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    # the LDS rung names V and the largest V that fits, and the plan says the same: T = 1024 with S = 8, C = 4, three heads holds 8 arms
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    big = E.Engine(E.proc_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    big.profile_enable(True)
    flat0 = torch.zeros(big.n_params, device=DEV)
    bt = big.make_batch(torch.zeros(2, 4, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["proc"]], None)
    tables = lambda V: [torch.zeros(V, w, device=DEV) for w in WIDTHS["proc"]]            # noqa: E731
    with pytest.raises(L.SlodeError, match="LDS tables of T = 1024, S = 8, C = 4, V = 9 .*at most V = 8 fits"):
        big.intervene_summary(flat0, bt, 2, tables(9), 9, 1, 2, [0.5] * 4, 1)
    assert big.rng_state()[2] == 0
    with pytest.raises(L.SlodeError, match="no profiled step"):
        big.profile_read()
    with pytest.raises(L.SlodeError, match="V = 9 .*at most V = 8 fits"):
        big.intervene_summary_plan(2, 9)
    assert big.intervene_summary_plan(2, 8) <= 160 * 1024
    got = big.intervene_summary(flat0, bt, 2, tables(8), 8, 1, 2, [0.5] * 4, 1)             # eight arms of the same shape are taken
    assert [n for n, _ in big.profile_read()] == ["weff", "enc_fwd2", "intervene_summary"] and bool(torch.isfinite(got[2][..., :6]).all())


# ---- the model layer ---------------------------------------------------------------------------------------------------------------------
def _stack(res, m, arm, kind):
    """[Q, (V,) B, C, 8] fp64 of the dict's ``arm``: kind 0 the means, 1 the sds."""
    return np.stack([np.stack([res[n][arm][k][kind].double().cpu().numpy() for k in SU.NAMES], -1) for n in m.MOMENT_HEADS[bool(m.GAUSS)]])


@pytest.mark.parametrize("why", ["dopri5", "strided"])
def test_composed_route_where_the_engine_refuses(why, monkeypatch):
    """(11) dopri5, a padded observation tensor: the engine refuses, intervention_summary composes the dict from counterfactual_samples --
    one drawing call, the counter at n + 1 -- and agrees with the definitions: the composed effect is the paired rule on the composed arms'
    own per-draw functionals.  On the fixed-grid model the fused call (dense observations, same noise) agrees with the composed route
    within the bars of the continuous slots (both are fp32 evaluations of the same curves: twice the per-arm bar)."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch)
    eng = m._bind().engine
    B, ns = batch["observations"].shape[0], 6
    dense = dict(batch)
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    hyp = m.label_grid(iext=[0.0, 1.0], rtpr=[1.0])
    thr = [0.45, 0.45, 0.45]
    calls = _count_calls(monkeypatch, eng, "intervene_summary")
    eng.rng_seed(11)
    eng.rng_set_counter(2)
    eps = eng.rng_normal(2, ns * B).view(ns, B, -1)
    drawn = m.intervention_summary(num_samples=ns, hypotheses=hyp, thresholds=thr, sense="below", **batch)
    assert eng.rng_state() == (11, 0, 3) and len(calls) == 1                        # refused once, then composed
    given = m.intervention_summary(num_samples=ns, hypotheses=hyp, thresholds=thr, sense="below", eps=eps, **batch)
    for arm in ("factual", "cf", "effect"):
        assert np.array_equal(_stack(given, m, arm, 0), _stack(drawn, m, arm, 0), equal_nan=True), arm
    assert set(given) == {"hypotheses"} | set(m.MOMENT_HEADS[bool(m.GAUSS)]) and tuple(_stack(given, m, "cf", 0).shape[1:]) == (2, B, 3, 8)
    # the definitions, from counterfactual_samples on hypothesis 1 directly
    labels = {l: batch[l] for l in m.LABELS}
    swap = {l: t[1:2].to(DEV).expand(B, -1).contiguous() for l, t in hyp.items()}
    res = m.counterfactual_samples(batch["observations"], ns, swap, eps=eps, **labels)
    times = torch.as_tensor(m.times).float().cpu().numpy()
    for q, n in enumerate(m.MOMENT_HEADS[bool(m.GAUSS)]):
        f_f, f_v = (SU.functionals(res[n][a].permute(3, 0, 1, 2).cpu().numpy(), times, np.array(thr, np.float32), -1) for a in (0, 1))
        wm, ws = SU.oracle_moments(f_v - f_f)
        assert np.allclose(_stack(given, m, "effect", 0)[q, 1], wm, rtol=1e-4, atol=1e-5, equal_nan=True), n
        assert np.allclose(_stack(given, m, "effect", 1)[q, 1], ws, rtol=1e-3, atol=1e-4, equal_nan=True), n
    if why == "strided":
        calls.clear()
        fused = m.intervention_summary(num_samples=ns, hypotheses=hyp, thresholds=thr, sense="below", eps=eps, **dense)
        assert len(calls) == 1
        span = float(times[-1] - times[0])
        for arm in ("factual", "cf", "effect"):
            a, b = _stack(fused, m, arm, 0), _stack(given, m, arm, 0)
            for slot, scale in ((0, 1.0), (2, 1.0), (4, span)):
                bar = 2 * (2 if arm == "effect" else 1) * scale * RU.MEAN_BAR * np.maximum(1.0, np.abs(b[..., slot]))
                assert np.all(np.abs(a[..., slot] - b[..., slot]) <= bar), (arm, slot)


def test_memory_stays_below_one_materialised_tensor():
    """(12) After a warm-up call, the peak of torch.cuda.max_memory_allocated of the fused call at B = 64, K = 64, V = 4 over the
    allocation before it stays below ONE materialised [B, C, T, K] tensor."""
    m, batch = _model("cvs")
    batch = {k: torch.cat([v] * 4)[:64].contiguous() for k, v in batch.items()}
    batch["observations"] = batch["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    hyp = m.default_hypotheses(**{l: batch[l] for l in m.LABELS})
    thr = [0.5] * Cn
    m.intervention_summary(num_samples=8, hypotheses=hyp, thresholds=thr, **batch)
    eng.profile_enable(True)
    peak = _peak(lambda: m.intervention_summary(num_samples=64, hypotheses=hyp, thresholds=thr, **batch))
    assert [n for n, _ in eng.profile_read()][-1] == "intervene_summary"       # the fused route, not the composition
    eng.profile_enable(False)
    one = B * Cn * T * 64 * 4
    print("peak over the allocation before the call: fused B=64 K=64 V=4 %d B; one materialised [B, C, T, K] tensor %d B" % (peak, one))
    assert B == 64 and next(iter(hyp.values())).shape[0] == 4 and peak < one


def test_output_files(tmp_path):
    """(13) save_intervention_summary over two batches: the arrays and the hypothesis tables, equal to intervention_summary from the same
    generator state, the trajectories in loader order."""
    m, batch = _model("challenge")
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    halves = [{k: v[:9] for k, v in batch.items()}, {k: v[9:] for k, v in batch.items()}]
    halves = [dict(h, observations=h["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)) for h in halves]
    hyp = m.default_hypotheses(**{l: batch[l] for l in m.LABELS})
    V = next(iter(hyp.values())).shape[0]
    thr = [0.3] * Cn
    eng.rng_seed(8)
    files = m.save_intervention_summary(str(tmp_path / "is"), halves, 5, hyp, thresholds=thr, sense="above")
    assert eng.rng_state()[2] == 2
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    want = ["summary_%s_%s_%s.npy" % (n, arm, k) for n in names for arm in ("factual", "cf", "effect") for k in ("mean", "sd")]
    want += ["summary_hypotheses_%s.npy" % l for l in m.LABELS if l in hyp]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "is"))) == sorted(want)
    f_mean, cf_mean, eff_mean = np.load(files[0]), np.load(files[2]), np.load(files[4])
    assert f_mean.shape == (B, Cn, 8) and cf_mean.shape == eff_mean.shape == (B, V, Cn, 8) and f_mean.dtype == np.float32
    assert np.isfinite(f_mean[..., :6]).all() and np.isfinite(eff_mean[..., :6]).all()
    eng.rng_set_counter(1)
    res = m.intervention_summary(num_samples=5, hypotheses=hyp, thresholds=thr, **halves[1])
    assert np.array_equal(eff_mean[9:, :, :, 0], res[names[0]]["effect"]["peak"][0].transpose(0, 1).cpu().numpy())
    assert np.array_equal(f_mean[9:, :, 4], res[names[0]]["factual"]["auc"][0].cpu().numpy())
    for line in m.intervention_summary_lines(eff_mean, hyp, True):
        print(line)
