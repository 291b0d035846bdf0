"""GPU tests of the cohort moments (slode_cohort_moments / Engine.cohort_moments / MechanisticBase.cohort_moments / save_cohort_moments /
--cohort-curves) against the fp64 oracle composed by cohort, against slode_recon_moments, and against the kernel's own per-draw fp32
values reduced in fp64.  Every bar lives in tests/cohort_util.py, with its derivation.  No test here feeds member indices or offsets
that are out of range: that guard is code plus its restatement in tests/test_cohort_cpu.py."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import cohort_util as CU
from tests import eval_stats_util as EU
from tests import recon_moments_util as RU
from tests.eval_gpu_util import (ADAPTIVE, DEV, WIDTHS, _captured, _device_batch, _engine, _eps_dev, _model, _model_batches, _on_device, _padded,
                                 _peak, _refused)
from tests.eval_gpu_util import _recon_moments as _moments
from tests.eval_gpu_util import _cohort, _cohort_ids as _ids, _cohort_lists as _lists, _cohort_per_draw as _per_draw, _cohort_truth as _truth

pytestmark = pytest.mark.gpu
ALL = ("sd", "sd_subjects", "obs_mean", "l1")


def _same(x, y):
    """Bitwise equal, the NaN of an empty cohort equal to itself."""
    return torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0))


# ---- the fp64 oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_cohorts_match_the_fp64_oracle(case, solver):
    """Six model classes x three fixed-grid solvers x {posterior, prior}; B = 23, K = 7, explicit noise; G = 5 with cohort sizes
    (7, 0, 11, 1, 2), two trajectories in no cohort, members interleaved in batch order; chunk = 3: ragged chunk ends and a one-member
    chunk.  All five outputs pre-filled with NaN: the empty cohort all NaN, the rest finite and within the bars."""
    c = RU.build(case, solver, B=23, ns=7)
    ids, G = CU.parity_ids()
    eng = _engine(c)
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        got = _cohort(eng, flat, c, is_post, ids, G, chunk=3)
        CU.check(got, CU.oracle_cohorts(c, is_post, ids, G), c["obs"], 3, "%s/%s/%s" % (case, solver, "post" if is_post else "prior"))
        assert torch.isnan(got[0][:, 1]).all() and torch.isnan(got[4][1]).all()


def test_clip_acts_on_the_samples():
    """clip_min at the median of the oracle's head values: every moment against the oracle's per-draw curves clipped by comparison."""
    c = RU.build("proc_ald", "rk4", B=9, ns=7)
    ids, G = _ids("three", 9)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    clip = float(np.median(CU.oracle_draws(c, True)))
    for is_post in (True, False):
        got = _cohort(eng, flat, c, is_post, ids, G, chunk=2, clip=clip)
        CU.check(got, CU.oracle_cohorts(c, is_post, ids, G, clip=clip), c["obs"], 2, "clip %s" % is_post)
        assert float(got[0][torch.isfinite(got[0])].min()) >= np.float32(clip)


SIZES = [("cvs_gauss", 65, 2, 0, "three", {}, ALL), ("cvs_gauss", 65, 2, 1, "three", {}, ALL), ("cvs_gauss", 65, 2, 2, "three", {}, ALL),
         ("cvs_gauss", 65, 2, 64, "three", {}, ALL), ("cvs_gauss", 65, 1, 0, "three", {}, ALL), ("challenge_gauss", 12, 2, 5, "three", {}, ALL),
         ("cvs_ald", 3, 200, 2, "one", {}, ALL), ("proc_gauss", 65, 2, 4, "three", {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"}, ALL),
         ("cvs_ald", 9, 7, 2, "three", {"SLODE_ODE_GENERIC": "1"}, ALL),
         ("proc_ald", 9, 2, 0, "three", {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}, ALL),
         ("cvs_gauss", 65, 2, 0, "one", {}, ALL), ("cvs_gauss", 65, 2, 3, "singletons", {}, ALL), ("cvs_gauss", 16, 2, 0, "none", {}, ALL),
         ("cvs_ald", 9, 2, 2, "three", {}, ())]


@pytest.mark.parametrize("case,B,ns,chunk,mode,env,outputs", SIZES,
                         ids=["%s-B%d-ns%d-R%d-%s%s%s" % (c, B, ns, R, m, "-" + "-".join(k[10:].lower() for k in e) if e else "", "" if o else "-mean_only")
                              for c, B, ns, R, m, e, o in SIZES])
def test_sizes_and_instantiations(case, B, ns, chunk, mode, env, outputs, monkeypatch):
    """chunk in {0, 1, 2, 64} at B = 65; T = 300 (challenge_gauss) against the metric T = 200 (cvs_ald); K in {1, 2, 200} (200 at B = 3);
    the persistent loop; the run-time-S build; G = 1, G = B singletons, M = 0 (every output NaN), every output NULL except mean; rk4,
    posterior and prior, NaN-poisoned workspace."""
    c = RU.build(case, "rk4", B=B, ns=ns)
    ids, G = _ids(mode, B)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    R = chunk or eng.cohort_plan(B, int((ids >= 0).sum()), G, ns)[0]
    for is_post in (True, False):
        got = _cohort(eng, flat, c, is_post, ids, G, chunk=chunk, outputs=outputs)
        assert all((x is None) == (n not in outputs) for n, x in zip(ALL, got[1:]))
        CU.check(got, CU.oracle_cohorts(c, is_post, ids, G), c["obs"], R, "%s B=%d ns=%d R=%d %s %s %s" % (case, B, ns, chunk, mode, env, is_post))
        if mode == "none":
            assert all(torch.isnan(x).all() for x in got)
        if mode == "singletons":
            assert float(got[2].abs().max()) == 0.0
        if ns == 1 and outputs:
            assert _same(got[1], got[2])


# ---- against the kernel's own per-draw values, and against slode_recon_moments ------------------------------------------------------------
@pytest.mark.parametrize("is_post", [False, True])
def test_kernel_accumulation_on_curves_whose_sd_is_1e4_of_their_level(is_post):
    """As test_gpu_recon_moments' case of the same name: noise scaled by 3e-5, the kernel's own fp32 value of every draw from K calls with
    num_samples = 1 and singleton cohorts, reduced in fp64 by cohort; the cohort call at chunk = 3 and at chunk = 64 against it at
    CU.accumulation_bars -- bounds without a term in |mean| for the sds, which a plain sum of squares misses -- and the two chunk sizes
    against each other within the two bounds added."""
    K, B = 6, 14
    c = RU.build("cvs_ald", "rk4", B=B, ns=K)
    c["obs"], c["u"] = c["obs"][:1].repeat(B, 1, 1), c["u"][:1].repeat(B, 1)                # every member the same subject: one thin band per cohort
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps = (3e-5 * c["eps"]).to(DEV).contiguous()
    ids, G = np.array([0, 1, 0, 0, 1, -1, 0, 2, 0, 1, 0, 0, 1, 0]), 3
    vals = _per_draw(eng, flat, c, is_post, eps, obs_d, labels)
    got = {}
    for R in (3, 64):
        mean, sd, sdb = (x.cpu().numpy() for x in _cohort(eng, flat, c, is_post, ids, G, chunk=R, eps=eps, obs_d=obs_d, labels=labels)[:3])
        want_mean, want_sd, want_sdb, D = _truth(vals, ids, G, R)
        bm, bs, bb = CU.accumulation_bars(want_mean, want_sd, want_sdb, D, min(R, 8), K)  # (a chunk holds at most the cohort's 8 members)
        live = want_sd > 0                                                                # (cohort 2 has one member: K values)
        assert live.mean() > 0.9 and np.all(D[live] <= CU.SPREAD * want_sd[live])         # the condition of the bars
        assert float(np.median(want_sd[live] / np.abs(want_mean[live]))) < 1e-3
        em, es = np.abs(mean - want_mean) / bm, np.abs(sd - want_sd)[live] / bs[live]
        liveb = want_sdb > 0
        eb = np.abs(sdb - want_sdb)[liveb] / bb[liveb]
        print("post=%s R=%d: median sd / |mean| %.2e; error / bound: mean %.3f, sd %.3f, sd_subjects %.3f"
              % (is_post, R, float(np.median(want_sd[live] / np.abs(want_mean[live]))), em.max(), es.max(), eb.max()))
        assert em.max() <= 1.0 and es.max() <= 1.0 and eb.max() <= 1.0
        assert np.array_equal(sdb[:, 2], np.zeros_like(sdb[:, 2]))                        # cohort 2: one member
        got[R] = (mean, sd, sdb, bm, bs, bb, live, liveb)
    a, b = got[3], got[64]
    assert np.all(np.abs(a[0] - b[0]) <= a[3] + b[3]) and np.all(np.abs(a[1] - b[1])[a[6]] <= (a[4] + b[4])[a[6]])
    assert np.all(np.abs(a[2] - b[2])[a[7]] <= (a[5] + b[5])[a[7]])


def test_identities_against_recon_moments():
    """G = B singletons: sd_subjects == 0 exactly, mean and sd match slode_recon_moments of the same noise within the accumulation bounds
    of both kernels.  K = 1: sd equals sd_subjects.  Any cohort: sd^2 = sd_subjects^2 + mean over members of recon_moments' sd_b^2 (law
    of total variance), within the bounds added.  Excluding a trajectory leaves every other cohort bitwise unchanged."""
    K, B = 7, 13
    c = RU.build("cvs_ald", "midpoint", B=B, ns=K)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps = c["eps"].to(DEV).contiguous()
    vals = _per_draw(eng, flat, c, True, eps, obs_d, labels)
    rmean, rsd = (x.cpu().numpy() for x in _moments(eng, flat, c, True))
    # singletons
    ids, G = _ids("singletons", B)
    mean, sd, sdb = (x.cpu().numpy() for x in _cohort(eng, flat, c, True, ids, G, chunk=4)[:3])
    want_mean, want_sd, want_sdb, D = _truth(vals, ids, G, 1)
    assert float(np.abs(sdb).max()) == 0.0
    assert np.all(D <= RU.SPREAD * want_sd)
    bm, bs, _ = CU.accumulation_bars(want_mean, want_sd, want_sdb, D, 1, K)
    rbm, rbs = RU.accumulation_bars(want_mean, want_sd, K)
    print("singletons against recon_moments: |mean diff| / bound %.3f, |sd diff| / bound %.3f" % ((np.abs(mean - rmean) / (bm + rbm)).max(), (np.abs(sd - rsd) / (bs + rbs)).max()))
    assert np.all(np.abs(mean - rmean) <= bm + rbm) and np.all(np.abs(sd - rsd) <= bs + rbs)
    # the law of total variance, three cohorts at chunk = 2
    ids, G = _ids("three", B)
    full = _cohort(eng, flat, c, True, ids, G, chunk=2)
    mean, sd, sdb = (x.double().cpu().numpy() for x in full[:3])
    want_mean, want_sd, want_sdb, D = _truth(vals, ids, G, 2)
    _, bs, bb = CU.accumulation_bars(want_mean, want_sd, want_sdb, D, 2, K)
    for g in range(G):
        sel = np.flatnonzero(ids == g)
        if not sel.size:
            continue
        within = (rsd[:, sel].astype(np.float64) ** 2).mean(1)
        tol = 2 * sd[:, g] * bs[:, g] + (2 * sdb[:, g] * bb[:, g] if sel.size > 1 else 0.0) + (2 * rsd[:, sel] * rbs[:, sel]).mean(1)
        assert np.all(np.abs(sd[:, g] ** 2 - (sdb[:, g] ** 2 + within)) <= tol), g
    # K = 1: the two sds are the same number
    one = _cohort(eng, flat, c, True, ids, G, chunk=2, eps=eps[0].contiguous(), ns=1)
    assert _same(one[1], one[2])
    # excluding one trajectory of cohort 0: the other cohorts do not move by a bit
    less = ids.copy()
    less[np.flatnonzero(ids == 0)[1]] = -1
    other = _cohort(eng, flat, c, True, less, G, chunk=2)
    for x, y in zip(full, other):
        assert _same(x[..., 1:, :, :] if x.dim() == 4 else x[1:], y[..., 1:, :, :] if y.dim() == 4 else y[1:])
    assert not torch.equal(full[0][:, 0], other[0][:, 0])


# ---- reproducibility and noise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_bitwise_reproducible_and_independent_of_the_grid(case, monkeypatch):
    """Two calls: bitwise equal.  One workgroup per chunk against the 3-workgroup loop: bitwise equal.  In-kernel noise against the same
    rows passed explicitly: bitwise equal; the counter moves by one, and not at all with explicit noise."""
    c = RU.build(case, "midpoint", ns=7)
    ids, G = _ids("three", c["B"])
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    same = lambda x, y: all(_same(a, b) for a, b in zip(x, y))
    for is_post in (True, False):
        a = _cohort(eng, flat, c, is_post, ids, G)
        assert same(a, _cohort(eng, flat, c, is_post, ids, G)) and same(a, _cohort(loop, flat, c, is_post, ids, G))
        for e in (eng, loop):
            e.rng_seed(77, first_trajectory=1000)
            e.rng_set_counter(5)
        drawn = _cohort(eng, flat, c, is_post, ids, G, eps=None)
        assert eng.rng_state() == (77, 1000, 6)
        rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
        given = _cohort(eng, flat, c, is_post, ids, G, eps=rows)
        assert eng.rng_state() == (77, 1000, 6)                                           # explicit noise draws nothing
        assert same(drawn, given) and same(drawn, _cohort(loop, flat, c, is_post, ids, G, eps=None))
        assert not same(a, drawn)


# ---- launches, capture, refusals, memory -----------------------------------------------------------------------------------------------------
def test_launches_and_graph_capture():
    """Posterior: "weff", "enc_fwd2", "cohort_plan", "cohort_moments", "cohort_merge" on one stream (a linear graph); prior: the last
    three.  One capture and one replay of a posterior call equal the stream-launched call bitwise."""
    c = RU.build("cvs_ald", "rk4", ns=7)
    ids, G = _ids("three", c["B"])
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps = c["eps"].to(DEV).contiguous()
    eng.profile_enable(True)
    _cohort(eng, flat, c, True, ids, G)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "cohort_plan", "cohort_moments", "cohort_merge"]
    _cohort(eng, flat, c, False, ids, G)
    assert [n for n, _ in eng.profile_read()] == ["cohort_plan", "cohort_moments", "cohort_merge"]
    eng.profile_enable(False)
    members, offsets = _lists(ids, G)
    out = [torch.zeros(3, G, 3, c["T"], device=DEV) for _ in range(3)] + [torch.zeros(G, 3, c["T"], device=DEV), torch.zeros(G, 3, device=DEV)]
    scratch = torch.zeros(eng.cohort_plan(c["B"], members.numel(), G, 7, 3)[3] // 4, device=DEV)
    bt = eng.make_batch(obs_d, labels, eps, particles=7)
    call = lambda: eng.cohort_moments(flat, bt, c["B"], True, 7, members, offsets, G, 3, None, *out, scratch=scratch)
    want = _captured(call, out)
    assert all(_same(x, y) for x, y in zip(out, want)) and bool(torch.isfinite(out[0][:, :2]).all())     # (cohort 2 of these ids is empty: NaN)


def test_refusals_write_nothing_and_draw_nothing(monkeypatch):
    """Every refusal names its reason, draws nothing, launches nothing (rng_state, profile_read) and leaves the outputs as they were."""
    from structured_latent_odes_amd import _lib as L
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)
    ids, G = _ids("three", c["B"])
    members, offsets = _lists(ids, G)

    def refused(eng, match, obs=obs_d, ns=2, is_post=True, G=G, chunk=0, offsets=offsets, scratch=None, outputs=ALL):
        flat = eng.pack(c["p"])
        mean = torch.full((3, max(G, 1), 3, c["T"]), 7.0, device=DEV)
        _refused(eng, lambda: eng.cohort_moments(flat, eng.make_batch(obs, labels, None), c["B"], is_post, ns, members, offsets, G, chunk=chunk,
                                                 mean=mean, outputs=outputs, scratch=scratch), match)
        torch.cuda.synchronize(DEV)
        assert bool((mean == 7.0).all())

    eng = _engine(c, monkeypatch)
    some = torch.zeros(1 << 16, device=DEV)
    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s" % solver, scratch=some)
    refused(eng, "num_samples = 0", ns=0)
    refused(eng, "chunk = 65", chunk=65)
    refused(eng, "G = 1025", G=1025, offsets=torch.zeros(1026, dtype=torch.int32, device=DEV))
    refused(eng, "scratch_bytes", scratch=torch.zeros(64, device=DEV))
    padded = _padded(obs_d)
    refused(eng, "observation strides", obs=padded, scratch=some)
    refused(eng, "obs_mean / l1 need dense", obs=padded, is_post=False, scratch=some)
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms", scratch=some)
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD", scratch=some)
    # the prior without obs_mean / l1 reads no observations: their strides do not matter
    eng = _engine(c, monkeypatch)
    flat = eng.pack(c["p"])
    got = _cohort(eng, flat, c, False, ids, G, outputs=("sd", "sd_subjects"), obs_d=padded, labels=labels)
    want = CU.oracle_cohorts(c, False, ids, G)
    CU.check(got[:3] + (None, None), want, c["obs"], 3, "prior with padded observations")
    # tables beyond the LDS of one CU: T = 1024 with three heads
    from structured_latent_odes_amd import engine as E
    big = E.Engine(E.proc_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    with pytest.raises(L.SlodeError, match="LDS tables"):
        big.cohort_moments(torch.zeros(big.n_params, device=DEV), big.make_batch(torch.zeros(2, 4, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["proc"]], None),
                           2, False, 2, torch.zeros(2, dtype=torch.int32, device=DEV), torch.tensor([0, 2], dtype=torch.int32, device=DEV), 1, scratch=some)
    assert big.rng_state()[2] == 0


@pytest.mark.parametrize("is_post", [True, False])
def test_memory_is_the_outputs_and_the_scratch(is_post):
    """After a warm-up call, the peak of torch.cuda.max_memory_allocated over the allocation before the call is the outputs plus the
    plan's scratch_bytes (and the member lists): the same at K = 8 and K = 200, and at chunk = 8 below slode_recon_moments' outputs for
    the same B."""
    m, batches = _model_batches("cvs")
    batch = _on_device(batches[0], "cvs")                                                   # 24 trajectories
    eng = m._bind().engine
    B = batch["observations"].shape[0]
    ids = torch.arange(B, device=DEV) % 2
    m.cohort_moments(is_post=is_post, num_samples=8, cohorts=ids, chunk=8, **batch)
    eng.profile_enable(True)
    fused = []
    for ns in (8, 200):
        fused.append(_peak(lambda: m.cohort_moments(is_post=is_post, num_samples=ns, cohorts=ids, chunk=8, **batch)))
        assert [n for n, _ in eng.profile_read()][-1] == "cohort_merge"                   # the fused route, not the composition
    eng.profile_enable(False)
    G, Q, C, T = 2, 3, 3, 86
    outputs = 4 * (3 * Q * G * C * T + G * C * T + G * C)
    scratch = eng.cohort_plan(B, B, G, 8, 8)[3]
    recon_out = 2 * Q * B * C * T * 4
    print("peak over the allocation before the call: K=8 %d B, K=200 %d B (outputs %d B + scratch %d B); recon_moments' outputs %d B" % (fused[0], fused[1], outputs, scratch, recon_out))
    assert fused[0] == fused[1]
    slack = 32 * 512                                                                      # member lists, counts, keys and the allocator's rounding: 512 B blocks
    assert outputs + scratch <= fused[1] <= outputs + scratch + slack
    assert fused[1] < recon_out


# ---- the model route -------------------------------------------------------------------------------------------------------------------------
def _agree(got, want, names, tag):
    """The fused dict against the composed one at the oracle bars (scale from the composed mean)."""
    live = (want["count"] > 0).cpu().numpy()
    assert torch.equal(got["count"], want["count"]) and torch.equal(got["keys"], want["keys"])
    for n in names:
        scale = want[n][0].double().abs().clamp_min(1.0).cpu().numpy()[live]
        for i, bar in enumerate((CU.MEAN_BAR, CU.SD_BAR, CU.SD_BAR)):
            g, w = got[n][i].double().cpu().numpy(), want[n][i].double().cpu().numpy()
            assert np.isnan(g[~live]).all() and np.isnan(w[~live]).all()
            r = float((np.abs(g[live] - w[live]) / (bar * scale)).max())
            assert r <= 1.0, (tag, n, i, r)
    T = want["observations"].shape[-1]
    ob = CU.obs_bar(want["observations"].cpu().numpy()[live], 64)
    assert np.all(np.abs((got["observations"] - want["observations"]).cpu().numpy()[live]) <= ob)
    l1_bar = (CU.MEAN_BAR * want[names[0]][0].double().abs().clamp_min(1.0)).sum(-1).cpu().numpy()[live] + T * ob
    assert np.all(np.abs((got["l1"].double() - want["l1"].double()).cpu().numpy()[live]) <= l1_bar), tag


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_fused_route_agrees_with_the_composed_one(fam):
    """cohorts from all of the family's labels (cohort_index) and from an id tensor with an empty cohort and an excluded trajectory;
    in-kernel noise from the same generator state on both routes; both leave the counter at n + 1."""
    m, batch = _model(fam)
    eng = m._bind().engine
    names = ("mu_50", "mu_75", "mu_25")
    B = batch["observations"].shape[0]
    labels = {k: v for k, v in batch.items() if k != "observations"}
    ids_t = torch.tensor([(i * 7) % 3 for i in range(B)], device=DEV) * 2                   # cohorts 0, 2, 4: 1 and 3 empty
    ids_t[5] = -1
    for cohorts, kw in ((tuple(m.LABELS), {}), (ids_t, dict(num_cohorts=6))):
        for is_post in (True, False):
            eng.rng_seed(4321, first_trajectory=300)
            eng.rng_set_counter(9)
            eng.profile_enable(True)
            got = m.cohort_moments(is_post=is_post, num_samples=12, cohorts=cohorts, clip_min=0.0, **kw, **batch)
            assert [n for n, _ in eng.profile_read()][-1] == "cohort_merge" and eng.rng_state() == (4321, 300, 10)
            eng.profile_enable(False)
            eng.rng_set_counter(9)
            ids, keys, G, _, _, count = m._cohort_lists(batch["observations"], cohorts, kw.get("num_cohorts"), labels)
            want = dict(m._cohort_composed(batch["observations"], is_post, 12, ids, G, count, None, 0.0, labels), count=count, keys=keys)
            assert eng.rng_state() == (4321, 300, 10)
            _agree(got, want, names, "%s/%s" % (fam, is_post))
    assert got["count"].tolist() == [int((ids_t == g).sum()) for g in range(6)] and got["count"][1] == 0 and int(got["count"].sum()) == B - 1


@pytest.mark.parametrize("why", ["dopri5", "strided", "SLODE_ODE_ALG"])
def test_model_level_call_is_total_over_what_the_engine_refuses(why, monkeypatch):
    """dopri5, a padded observation tensor, a measured arm: the engine refuses, MechanisticBase.cohort_moments composes the dict from
    recon_samples -- equal to the notebooks' arithmetic done in numpy on recon_samples of the same generator state; one drawing call."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch, {why: "1"} if why.startswith("SLODE") else None)
    eng = m._bind().engine
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    ns = 6
    eng.rng_seed(11)
    got = m.cohort_moments(is_post=True, num_samples=ns, cohorts=("iext", "rtpr"), **batch)
    assert eng.rng_state()[2] == 1
    eng.rng_set_counter(0)
    res = m.recon_samples(is_post=True, num_samples=ns, **batch)
    ids, keys = m.cohort_index(by=("iext", "rtpr"), **{k: v for k, v in batch.items() if k != "observations"})
    ids = ids.cpu().numpy()
    y = batch["observations"].double().cpu().numpy()
    assert torch.equal(got["keys"], keys) and got["count"].tolist() == [int((ids == g).sum()) for g in range(keys.shape[0])]
    for g in range(keys.shape[0]):
        loc = np.flatnonzero(ids == g)
        for n in ("mu_50", "mu_75", "mu_25"):
            data = res[n].double().cpu().numpy()[loc]                                     # [n, C, T, ns]
            for x, w in zip(got[n], (data.mean((0, 3)), np.std(np.moveaxis(data, 3, 1).reshape(-1, 3, 86), 0), np.std(data.mean(3), 0))):
                assert np.allclose(x[g].double().cpu().numpy(), w, rtol=1e-5, atol=1e-6), (g, n)
        mean_mu = res["mu_50"].double().cpu().numpy()[loc].mean((0, 3))
        assert np.allclose(got["l1"][g].cpu().numpy(), np.abs(y[loc].mean(0) - mean_mu).sum(-1), rtol=1e-5)


def test_output_files(tmp_path):
    """save_cohort_moments: the file names of the issue, [G, C, T] each, equal to cohort_moments from the same generator state."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    eng.rng_seed(8)
    files = m.save_cohort_moments(str(tmp_path / "c"), is_post=True, num_samples=5, cohorts=("iext", "rtpr"), **batch)
    files += m.save_cohort_moments(str(tmp_path / "c"), is_post=False, num_samples=5, cohorts=("iext", "rtpr"), **batch)
    want = sorted(["%s_%s_cohort_%s.npy" % (cv, p, k) for cv in ("mu_50", "mu_75", "mu_25") for p in ("post", "prior") for k in ("mean", "sd", "sd_subjects")]
                  + ["observations_cohort_mean.npy", "cohort_keys.npy", "cohort_count.npy", "l1_post_cohort.npy", "l1_prior_cohort.npy"])
    assert sorted(set(os.path.basename(f) for f in files)) == want == sorted(os.listdir(str(tmp_path / "c")))
    eng.rng_set_counter(0)
    res = m.cohort_moments(is_post=True, num_samples=5, cohorts=("iext", "rtpr"), **batch)
    G = res["keys"].shape[0]
    assert np.load(str(tmp_path / "c" / "cohort_keys.npy")).shape == (G, 2) and int(np.load(str(tmp_path / "c" / "cohort_count.npy")).sum()) == batch["observations"].shape[0]
    assert np.array_equal(np.load(str(tmp_path / "c" / "mu_75_post_cohort_sd_subjects.npy")), res["mu_75"][2].cpu().numpy())
    assert np.array_equal(np.load(str(tmp_path / "c" / "l1_post_cohort.npy")), res["l1"].cpu().numpy()) and np.load(str(tmp_path / "c" / "l1_post_cohort.npy")).shape == (G, 3)


def test_l1_error_is_the_notebook_arithmetic():
    """l1_error = mean over non-empty cohorts and channels of l1, against the notebooks' arithmetic in numpy on recon_samples of the same
    generator state: mean_y = np.mean(y[loc], 0); mean_mu = np.mean(mu_50_sample[loc], (0, sample axis)); sum_t |mean_y - mean_mu|."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    eng.rng_seed(5)
    res = m.cohort_moments(is_post=True, num_samples=9, cohorts=("iext", "rtpr"), **batch)
    got = float(res["l1"][res["count"] > 0].mean())
    eng.rng_set_counter(0)
    mu = m.recon_samples(is_post=True, num_samples=9, **batch)["mu_50"].double().cpu().numpy()
    y = batch["observations"].double().cpu().numpy()
    ids = m.cohort_index(by=("iext", "rtpr"), **{k: v for k, v in batch.items() if k != "observations"})[0].cpu().numpy()
    l1 = [np.abs(y[ids == g].mean(0) - mu[ids == g].mean((0, 3))).sum(-1) for g in range(int(ids.max()) + 1)]
    want = float(np.mean(l1))
    bar = CU.MEAN_BAR * 86 * max(1.0, float(np.abs(mu).max())) + 86 * CU.obs_bar(y, 64)
    print("l1_error: fused %.6f, notebook arithmetic %.6f (bar %.2e)" % (got, want, bar))
    assert abs(got - want) <= bar


def test_training_entry_point_with_cohort_curves(tmp_path, capsys):
    tr = importlib.import_module("training_cvs")
    cfg = EU.model_config("cvs")
    cfg.update(num_epochs=0, mini_batch_size=16, seq_len=86, num_samples=5)
    tr.train(cfg, batches_per_epoch=1, cohort_curves=True, results_dir=str(tmp_path / "res"))
    out = capsys.readouterr().out
    assert "FINAL TEST:" in out and "l1_error_post: " in out and "l1_error_prior: " in out
    assert np.isfinite(float(out.split("l1_error_post: ")[1].split()[0]))
    got = sorted(os.listdir(str(tmp_path / "res")))
    assert len(got) == 18 + 5 and "mu_50_post_cohort_mean.npy" in got and "l1_prior_cohort.npy" in got
    G = np.load(str(tmp_path / "res" / "cohort_keys.npy")).shape[0]
    assert np.load(str(tmp_path / "res" / "mu_50_post_cohort_sd_subjects.npy")).shape == (G, 3, 86)
