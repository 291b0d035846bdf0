"""GPU tests of the counterfactual curves (slode_intervene_moments / Engine.intervene_moments / MechanisticBase.intervention_moments /
counterfactual_samples / save_intervention_moments) against the fp64 oracle composed in tests/intervene_util.py, against
recon_moments(is_post=True) and against the materialising composition.  Bars: module docstring of tests/intervene_util.py (the project's
per-value bar for cf; the sum of the two arms' bars for the effect)."""
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import intervene_util as IU
from tests import recon_moments_util as RU
from tests.eval_gpu_util import (ADAPTIVE, DEV, ENV_KEYS, SIZES, WIDTHS, _captured, _device_batch, _engine, _eps_dev, _model, _padded, _peak,
                                 _recon_moments, _refused)
from tests.eval_gpu_util import _iv, _label_split as _split

pytestmark = pytest.mark.gpu


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_against_the_fp64_oracle(case, solver):
    """Explicit noise, ns = 7; six model classes x three fixed-grid solvers x the masks of the family (each single prior group, all groups;
    proc also with the pair {C12, C6} alone swapped)."""
    c = RU.build(case, solver, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    for tag, mask, cols in IU.MASKS[c["fam"]]:
        u_cf = IU.cf_labels(c["u"], cols)
        got = _iv(eng, flat, c, mask, u_cf, obs_d=obs_d, labels=labels)
        IU.check(got, IU.oracle_moments(c, mask, u_cf), "%s/%s/%s" % (case, solver, tag))


@pytest.mark.parametrize("case,B,ns,env", SIZES, ids=["%s-B%d-ns%d%s" % (c, B, ns, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, ns, e in SIZES])
def test_sizes_and_instantiations(case, B, ns, env, monkeypatch):
    """The grid of tests/test_gpu_recon_moments.py: B on both sides of the 64- and 256-thread edges, the persistent loop on 5 and 2
    workgroups, the run-time-S instantiation, ns in {1, 2, 7, 200} (200 at B <= 3), rk4, the last mask of the family, NaN-poisoned
    workspace.  ns = 1: both sds are exactly 0."""
    c = RU.build(case, "rk4", B=B, ns=ns)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    tag, mask, cols = IU.MASKS[c["fam"]][-1]
    u_cf = IU.cf_labels(c["u"], cols)
    got = _iv(eng, flat, c, mask, u_cf)
    IU.check(got, IU.oracle_moments(c, mask, u_cf), "%s B=%d ns=%d %s %s" % (case, B, ns, env, tag))
    if ns == 1:
        assert float(got[1].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0


@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_empty_mask_gives_effect_zero_and_the_factual_moments(case):
    """group_mask = 0 (with and without counterfactual labels): the effect is exactly 0; cf agrees with recon_moments(is_post=True) on the
    same noise within the RU bars (printed: whether bitwise)."""
    c = RU.build(case, "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    mean, sd = _recon_moments(eng, flat, c, True)
    for u_cf in (None, IU.cf_labels(c["u"])):
        cm, cs, em, es = _iv(eng, flat, c, 0, u_cf)
        assert float(em.abs().max()) == 0.0 and float(es.abs().max()) == 0.0
        print("%s mask 0: cf bitwise equal to recon_moments(is_post=True): mean %s, sd %s" % (case, torch.equal(cm, mean), torch.equal(cs, sd)))
        RU.check(cm, cs, mean.double().cpu().numpy(), sd.double().cpu().numpy(), "%s mask 0 against recon_moments" % case)


@pytest.mark.parametrize("case", ["cvs_ald", "challenge_gauss"])
def test_effect_mean_is_cf_mean_minus_the_factual_mean(case):
    """One generator state: eff_mean = cf_mean - recon_moments(is_post=True).mean within the effect-mean bar."""
    c = RU.build(case, "midpoint", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    tag, mask, cols = IU.MASKS[c["fam"]][-1]
    eng.rng_seed(19)
    eng.rng_set_counter(3)
    cm, cs, em, es = _iv(eng, flat, c, mask, IU.cf_labels(c["u"], cols), eps=None)
    assert eng.rng_state() == (19, 0, 4)
    eng.rng_set_counter(3)
    fm, _ = _recon_moments(eng, flat, c, True, eps=None)
    bar = RU.MEAN_BAR * (fm.abs().clamp_min(1.0) + cm.abs().clamp_min(1.0))
    r = float(((em - (cm - fm)).abs() / bar).max())
    print("%s: |eff_mean - (cf_mean - f_mean)| / bar %.3e (largest |eff_mean| %.3e)" % (case, r, float(em.abs().max())))
    assert r <= 1.0 and float(em.abs().max()) > 0.0


INTERVENE = {"cvs": ("iext",), "challenge": ("shedding",), "proc": ("C12", "C6")}


def _swap(fam, batch):
    return {n: torch.roll(batch[n], 1, 0) for n in INTERVENE[fam]}


def _hand(res, names):
    """fp32 mean / population std of the materialised arms, as the composed route reduces them."""
    out = {}
    for n in names:
        f, c = res[n]
        d = c - f
        out[n] = (c.mean(-1), c.std(-1, unbiased=False), d.mean(-1), d.std(-1, unbiased=False))
    return out


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_paired_sd_against_counterfactual_samples(fam):
    """eff_sd (and the other three) of the ONE engine call (asserted from profile_read, for all three families) against the fp64 moments of
    the paired differences taken from counterfactual_samples on the same noise.  Printed, not asserted: the ratio of eff_sd to the unpaired sqrt(cf_sd^2 + f_sd^2)."""
    m, batch = _model(fam)
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    B, ns = batch["observations"].shape[0], 12
    eps = torch.randn(ns, B, m.latent_dim, generator=torch.Generator().manual_seed(5)).to(DEV)
    swap = _swap(fam, batch)
    eng = m._bind().engine
    eng.profile_enable(True)
    got = m.intervention_moments(num_samples=ns, intervene=swap, eps=eps, **batch)
    # the fused route, not the composition: challenge and proc name only some labels of their one prior group
    assert [k for k, _ in eng.profile_read()] == ["weff", "enc_fwd2", "intervene_moments"]
    eng.profile_enable(False)
    res = m.counterfactual_samples(num_samples=ns, intervene=swap, eps=eps, **batch)
    assert set(got) == set(names) and tuple(res["z"][0].shape) == (ns, B, m.latent_dim)
    for n in names:
        f, c = (t.double().cpu().numpy() for t in res[n])
        assert f.shape == c.shape == (B, batch["observations"].shape[1], batch["observations"].shape[2], ns)
        d = c - f
        want = dict(cf_mean=c.mean(-1), cf_sd=c.std(-1), eff_mean=d.mean(-1), eff_sd=d.std(-1), f_mean=f.mean(-1))
        IU.check(got[n]["cf"] + got[n]["effect"], want, "%s %s against counterfactual_samples" % (fam, n))
        unpaired = np.sqrt(want["cf_sd"] ** 2 + f.std(-1) ** 2)
        live = unpaired > 0
        print("%s %s: eff_sd / sqrt(cf_sd^2 + f_sd^2): median %.3f, max %.3f" % (fam, n, float(np.median(want["eff_sd"][live] / unpaired[live])),
                                                                              float((want["eff_sd"][live] / unpaired[live]).max())))


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_bitwise_reproducible_and_independent_of_the_grid(case, monkeypatch):
    """Two calls: bitwise equal.  One workgroup per trajectory against a 3-workgroup loop: bitwise equal.  In-kernel noise against the same
    rows passed explicitly: bitwise equal; the counter moves by one and explicit noise draws nothing."""
    c = RU.build(case, "midpoint", ns=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    tag, mask, cols = IU.MASKS[c["fam"]][-1]
    u_cf = IU.cf_labels(c["u"], cols)
    a = _iv(eng, flat, c, mask, u_cf)
    assert _equal(a, _iv(eng, flat, c, mask, u_cf)) and _equal(a, _iv(loop, flat, c, mask, u_cf))
    for e in (eng, loop):
        e.rng_seed(77, first_trajectory=1000)
        e.rng_set_counter(5)
    drawn = _iv(eng, flat, c, mask, u_cf, eps=None)
    assert eng.rng_state() == (77, 1000, 6)
    rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
    given = _iv(eng, flat, c, mask, u_cf, eps=rows)
    assert eng.rng_state() == (77, 1000, 6)                                       # explicit noise draws nothing
    assert _equal(drawn, given) and _equal(drawn, _iv(loop, flat, c, mask, u_cf, eps=None))
    # outputs the caller does not want: the others are unchanged, with and without the factual arm
    bt = eng.make_batch(*_device_batch(c), _eps_dev(c["eps"]), particles=7)
    only_cf = eng.intervene_moments(flat, bt, c["B"], _split(c, u_cf), mask, 7, None, None, False, False)
    only_sd = eng.intervene_moments(flat, bt, c["B"], _split(c, u_cf), mask, 7, False, None, False, None)
    assert only_cf[2] is None and only_cf[3] is None and torch.equal(only_cf[0], a[0]) and torch.equal(only_cf[1], a[1])
    assert only_sd[0] is None and only_sd[2] is None and torch.equal(only_sd[1], a[1]) and torch.equal(only_sd[3], a[3])


def test_refusals_by_name(monkeypatch):
    """Every refusal names its reason, draws nothing and launches nothing (rng_state, profile_read)."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd import engine as E
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)
    cf = _split(c, IU.cf_labels(c["u"]))

    def refused(eng, match, obs=obs_d, ns=2, particles=1, mask=1, cf_labels=cf, null_obs=False, error=None):
        flat = eng.pack(c["p"])
        bt = eng.make_batch(obs, labels, None)
        if null_obs:
            bt.obs = None
        err = _refused(eng, lambda: eng.intervene_moments(flat, bt, c["B"], cf_labels, mask, ns, particles=particles), match, error)
        if error is None:
            assert err.status == -1 and "slode_intervene_moments" in str(err)

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s" % solver)
    eng = _engine(c, monkeypatch)
    refused(eng, "particles = 2", particles=2)
    refused(eng, "num_samples = 0", ns=0)
    refused(eng, "exceeds 2\\^30 - 1 noise rows", ns=2 ** 30)                      # refused on the host: nothing sized by it is touched
    refused(eng, "batch->obs is NULL", null_obs=True)
    refused(eng, "observation strides", obs=_padded(obs_d))
    refused(eng, "bits at or beyond n_groups = 2", mask=4)
    refused(eng, "bits at or beyond n_groups = 2", mask=1 << 31)
    refused(eng, "cf_labels is NULL", cf_labels=None)
    # a missing tensor that an intervened group reads is the caller's argument error: ValueError from the engine, not a refusal to compose from
    refused(eng, "cf label 1 is None", mask=3, cf_labels=[cf[0], None], error=ValueError)
    refused(eng, "cf label 0 is None", mask=1, cf_labels=[None, cf[1]], error=ValueError)
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    # tables beyond the LDS of one CU: T = 1024 with S = 8, C = 4, three heads (the environment of the previous engines cleared first)
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    big = E.Engine(E.proc_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    big.profile_enable(True)
    with pytest.raises(L.SlodeError, match="LDS tables"):
        big.intervene_moments(torch.zeros(big.n_params, device=DEV), big.make_batch(torch.zeros(2, 4, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["proc"]], None),
                              2, None, 0, 2)
    assert big.rng_state()[2] == 0
    with pytest.raises(L.SlodeError, match="no profiled step"):
        big.profile_read()
    # a counterfactual tensor that no intervened group reads may be missing: mask = iext alone
    flat = eng.pack(c["p"])
    u_cf = IU.cf_labels(c["u"])
    got = eng.intervene_moments(flat, eng.make_batch(obs_d, labels, _eps_dev(c["eps"]), particles=2), c["B"], [cf[0], None], 1, 2)
    IU.check(got, IU.oracle_moments(c, 1, u_cf), "rtpr tensor missing, iext intervened")


@pytest.mark.parametrize("why", ["dopri5", "strided", "SLODE_ODE_ALG"])
def test_model_level_call_is_total_over_what_the_engine_refuses(why, monkeypatch):
    """dopri5, a padded observation tensor, a measured arm: the engine refuses, intervention_moments composes the dict -- equal to the hand
    reduction of counterfactual_samples from the same generator state (fp32 mean / population std); ONE drawing call, whatever the chunking."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch, {why: "1"} if why.startswith("SLODE") else None)
    eng = m._bind().engine
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    names, ns = ("mu_50", "mu_75", "mu_25"), 6
    swap = _swap("cvs", batch)
    eng.rng_seed(11)
    got = m.intervention_moments(num_samples=ns, intervene=swap, **batch)
    assert eng.rng_state()[2] == 1
    eng.rng_set_counter(0)
    want = _hand(m.counterfactual_samples(num_samples=ns, intervene=swap, **batch), names)
    assert eng.rng_state()[2] == 1
    for n in names:
        assert tuple(got[n]["cf"][0].shape) == (batch["observations"].shape[0], 3, 86)
        assert _equal(got[n]["cf"] + got[n]["effect"], want[n]), n
        assert float(got[n]["effect"][0].abs().max()) > 0.0
    if why != "dopri5":                                                           # four chunks of 5 rows: the same rows, the same bits
        monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 5 * ns)
        eng.rng_set_counter(0)
        chunked = m.intervention_moments(num_samples=ns, intervene=swap, **batch)
        assert eng.rng_state()[2] == 1
        assert all(_equal(chunked[n]["cf"] + chunked[n]["effect"], want[n]) for n in names)


def test_launches_and_graph_capture():
    """Three launches, "weff", "enc_fwd2", "intervene_moments", on one stream (a linear graph).  One capture and one replay equal the
    stream-launched call bitwise; capturing executes nothing."""
    c = RU.build("cvs_ald", "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    u_cf = IU.cf_labels(c["u"])
    eng.profile_enable(True)
    _iv(eng, flat, c, 3, u_cf)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "intervene_moments"]
    eng.profile_enable(False)
    outs = [torch.zeros(3, c["B"], 3, c["T"], device=DEV) for _ in range(4)]
    cf = _split(c, u_cf)
    bt = eng.make_batch(obs_d, labels, c["eps"].to(DEV).contiguous(), particles=7)
    want = _captured(lambda: eng.intervene_moments(flat, bt, c["B"], cf, 3, 7, *outs), outs)
    assert _equal(outs, want)


def test_memory_does_not_scale_with_the_number_of_draws():
    """After a warm-up call, the peak of torch.cuda.max_memory_allocated over the allocation before the call is the same at ns = 8 and at
    ns = 200 (the four [Q, B, C, T] outputs); counterfactual_samples at ns = 8 already needs more."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    swap = _swap("cvs", batch)
    m.intervention_moments(num_samples=8, intervene=swap, **batch)
    eng.profile_enable(True)
    fused = []
    for ns in (8, 200):
        fused.append(_peak(lambda: m.intervention_moments(num_samples=ns, intervene=swap, **batch)))
        assert [n for n, _ in eng.profile_read()][-1] == "intervene_moments"       # the fused route, not the composition
    eng.profile_enable(False)
    samples = _peak(lambda: m.counterfactual_samples(num_samples=8, intervene=swap, **batch))
    print("peak over the allocation before the call: fused ns=8 %d B, ns=200 %d B; counterfactual_samples ns=8 %d B" % (fused[0], fused[1], samples))
    assert fused[0] == fused[1]
    assert fused[1] < samples


def test_output_files(tmp_path):
    """save_intervention_moments: <curve>_{cf,effect}_<names joined by '+'>_sample_{mean,sd}.npy, [B, C, T] fp32 each, equal to
    intervention_moments from the same generator state."""
    m, batch = _model("proc")
    eng = m._bind().engine
    B = batch["observations"].shape[0]
    swap = _swap("proc", batch)
    eng.rng_seed(8)
    eng.profile_enable(True)
    files = m.save_intervention_moments(str(tmp_path / "iv"), num_samples=5, intervene=swap, **batch)
    assert [k for k, _ in eng.profile_read()][-1] == "intervene_moments"           # the fused route: C12 and C6 named, aR and aS as they were
    eng.profile_enable(False)
    want = sorted("%s_%s_C12+C6_sample_%s.npy" % (cv, a, k) for cv in ("mu_50", "mu_75", "mu_25") for a in ("cf", "effect") for k in ("mean", "sd"))
    assert sorted(os.path.basename(f) for f in files) == want == sorted(os.listdir(str(tmp_path / "iv")))
    eng.rng_set_counter(0)
    res = m.intervention_moments(num_samples=5, intervene=swap, **batch)
    assert float(res["mu_50"]["effect"][0].abs().max()) > 0.0
    for f in files:
        a = np.load(f)
        assert a.shape == (B,) + tuple(batch["observations"].shape[1:]) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(np.load(str(tmp_path / "iv" / "mu_75_effect_C12+C6_sample_sd.npy")), res["mu_75"]["effect"][1].cpu().numpy())
    assert np.array_equal(np.load(str(tmp_path / "iv" / "mu_50_cf_C12+C6_sample_mean.npy")), res["mu_50"]["cf"][0].cpu().numpy())
