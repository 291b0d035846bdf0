"""GPU tests of the calibration pass (slode_calibration / Engine.calibration / MechanisticBase.calibration / save_calibration /
--calibration) against the fp64 oracle by the comparison rule of tests/calibration_util.py, against the kernels' own per-draw fp32
curves compared in numpy, and against recon_samples reduced by hand.  The rule, every bar and the accumulation bound live in
tests/calibration_util.py, with their derivations.  Every call made through _calib also checks the invariants of the outputs.  No test
here feeds member indices or offsets that are out of range: that guard is code plus its restatement in tests/test_calibration_cpu.py."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import calibration_util as KU
from tests import eval_stats_util as EU
from tests import recon_moments_util as RU
from tests.eval_gpu_util import (ADAPTIVE, DEV, SIZES, WIDTHS, _captured, _device_batch, _engine, _eps_dev, _model, _model_batches, _on_device,
                                 _padded, _peak, _refused)
from tests.eval_gpu_util import _recon_moments as _moments
from tests.eval_gpu_util import _calib, _calib_invariants as _invariants, _calib_own_curves as _own_curves, _cohort_lists as _lists

pytestmark = pytest.mark.gpu
ALL = ("inside", "cross", "pinball", "width")


def _same(x, y):
    """Bitwise equal, the NaN of an empty cohort equal to itself."""
    if x is None or y is None:
        return x is None and y is None
    return torch.equal(x, y) if x.dtype == torch.int32 else torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0))


def _all_same(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _ids(mode, B, seed=2):
    """(ids, G): "three": three cohorts and a tenth of the trajectories in none, interleaved; "one": G = 1; "parts": three cohorts that
    partition the batch; "edges": cohort sizes 1, 2, 3 (B = 6)."""
    if mode == "one":
        return np.zeros(B, np.int64), 1
    if mode == "parts":
        return np.arange(B) % 3, 3
    if mode == "edges":
        return np.array([2, 0, 1, 2, 1, 2]), 3
    r = np.random.RandomState(seed)
    return r.choice([-1, 0, 1, 2], size=B, p=[0.1, 0.5, 0.3, 0.1]), 3


# ---- 1. the fp64 oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_counts_match_the_fp64_oracle(case, solver):
    """Six model classes x three fixed-grid solvers x {posterior, prior}, the case's own observations; B = 23, ns = 7, explicit noise;
    G = 5 with cohort sizes (7, 0, 11, 1, 2), two trajectories in no cohort; chunk = 3.  Outputs pre-filled with -1 / NaN.  Counts by the
    comparison rule, pinball and width within their bars, the empty cohort 0 / NaN."""
    c = RU.build(case, solver, B=23, ns=7)
    ids, G = KU.parity_ids()
    eng = _engine(c)
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        got = _calib(eng, flat, c, is_post, ids, G, chunk=3)
        KU.check(got, KU.oracle_calibration(c, is_post, ids, G), "%s/%s/%s" % (case, solver, "post" if is_post else "prior"), 7)
        assert int(got[0][:, 1].abs().max()) == 0 and torch.isnan(got[3][:, 1]).all() and torch.isnan(got[4][1]).all()


@pytest.mark.parametrize("case", list(EU.CASES))
def test_constructed_observations_match_the_fp64_oracle(case):
    """Observations built around one extra prior draw (KU.constructed_case: B = 9, ns = 7, rk4, the prior side): the oracle's head-0
    fractions lie in [0.2, 0.8] in every channel -- asserted before anything is compared -- so the counts are interior; three cohorts
    and the whole batch as one."""
    c, y = KU.constructed_case(case)
    one = KU.oracle_calibration(c, False, np.zeros(9, np.int64), 1, obs=y)
    frac = one["counts"][0, 0].sum(-1) / (9 * 7 * c["T"])
    assert np.all((frac >= 0.2) & (frac <= 0.8)), frac
    c = dict(c, obs=y)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    for mode in ("one", "three"):
        ids, G = _ids(mode, 9)
        got = _calib(eng, flat, c, False, ids, G, chunk=2)
        want = KU.oracle_calibration(c, False, ids, G)
        KU.check(got, want, "%s constructed %s" % (case, mode), 7)
    print("%s: head-0 fraction below %s, crossing share %s" % (case, frac, one["counts"][4, 0].sum(-1) / (9 * 7 * c["T"])))


# ---- 2. the kernels' own per-draw values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_counts_are_those_of_the_kernels_own_curves(case):
    """The per-draw fp32 curves of ns = 1 recon_moments calls compared in numpy with the observations, against the counts of ONE ns = 7
    call, by the comparison rule (near points on the kernels' own values).  Prints how many cells differ at all: zero is expected where the
    shared routines give the same bits."""
    K, B = 7, 13
    c = RU.build(case, "rk4", B=B, ns=K)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps = c["eps"].to(DEV).contiguous()
    ids, G = _ids("three", B)
    y = c["obs"].numpy()
    for is_post in (True, False):
        v = _own_curves(eng, flat, c, is_post, eps, obs_d, labels)
        want = KU.reduce_by_cohort(y, v, KU.nominal(c["ospec"]), ids, G)
        got = _calib(eng, flat, c, is_post, ids, G, chunk=2, eps=eps, obs_d=obs_d, labels=labels)
        cells = KU.check(got, want, "%s own curves post=%s" % (case, is_post), K)
        print("%s post=%s: cells that differ from the kernels' own curves: %s" % (case, is_post, cells))


# ---- 3. sizes and instantiations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B,ns,env", SIZES, ids=["%s-B%d-ns%d%s" % (c, B, ns, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, ns, e in SIZES])
def test_sizes_and_instantiations(case, B, ns, env, monkeypatch):
    """B = 63 / 65 / 255 / 257, ns in {1, 2, 7, 200}, T = 300 (challenge_gauss: two rounds of the thread <-> t phase), the persistent loop,
    the run-time-S build; three cohorts at the library's chunk, rk4, posterior and prior, NaN-poisoned workspace.  ns = 1 on a Gauss case:
    cross all zero and inside <= count (the invariants of every call)."""
    c = RU.build(case, "rk4", B=B, ns=ns)
    ids, G = _ids("three", B)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    for is_post in (True, False):
        got = _calib(eng, flat, c, is_post, ids, G, chunk=0)
        KU.check(got, KU.oracle_calibration(c, is_post, ids, G), "%s B=%d ns=%d %s %s" % (case, B, ns, env, is_post), ns)


@pytest.mark.parametrize("case", ["cvs_gauss", "cvs_ald"])
def test_chunk_edges_and_optional_outputs(case):
    """Cohort sizes 1, 2 and 3 with chunk = 2: a one-member chunk, a full one, a full one followed by a ragged one; every optional output
    NULL leaves below as it is with them."""
    c = RU.build(case, "rk4", B=6, ns=2)
    ids, G = _ids("edges", 6)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        got = _calib(eng, flat, c, is_post, ids, G, chunk=2)
        KU.check(got, KU.oracle_calibration(c, is_post, ids, G), "%s edges %s" % (case, is_post), 2)
        only = _calib(eng, flat, c, is_post, ids, G, chunk=2, outputs=())
        assert only[1:] == (None, None, None, None) and torch.equal(only[0], got[0])


def test_nan_curves_compare_false_everywhere():
    """A NaN in constant_std at one (c, t) of a Gaussian model makes v_1 and v_2 NaN there, for every member and draw (the forward pass
    itself swallows a NaN latent: its ReLU is an fmaxf): below[1], below[2] and inside are 0 in that cell, below[0] and every other cell
    are those of the clean call bit for bit, and the float outputs of every cohort with a member are NaN."""
    c = RU.build("cvs_gauss", "rk4", B=9, ns=3)
    ids, G = KU.parity_ids()[0][:9] % 3, 4                                                # cohort 3 stays empty
    eng = _engine(c)
    clean = _calib(eng, eng.pack(c["p"]), c, False, ids, G, chunk=2)
    p = {k: v.clone() for k, v in c["p"].items()}
    p["decoder.constant_std"][1, 5] = float("nan")
    got = _calib(eng, eng.pack(p), c, False, ids, G, chunk=2, gauss=False)
    cell = torch.zeros_like(clean[1], dtype=torch.bool)
    cell[:, 1, 5] = True
    assert torch.equal(got[0][0], clean[0][0]) and torch.equal(got[2], clean[2])
    for x, y in ((got[0][1], clean[0][1]), (got[0][2], clean[0][2]), (got[1], clean[1])):
        assert int(x[cell].abs().max()) == 0 and torch.equal(x[~cell], y[~cell])
    assert int(clean[0][1][cell].max()) > 0                                               # (the clean call counts something there)
    live = torch.tensor([(ids == g).any() for g in range(G)], device=DEV)
    assert torch.isnan(got[3][:, live]).all() and torch.isnan(got[4][live]).all() and bool(torch.isfinite(clean[3][:, live]).all())
    assert torch.isnan(got[3][:, ~live]).all() and int(got[0][:, ~live].abs().max()) == 0


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_bitwise_reproducible_and_independent_of_the_grid(case, monkeypatch):
    """Two calls: equal.  One workgroup per chunk against the 3-workgroup loop: equal.  In-kernel noise against the same rows passed
    explicitly: equal; the counter moves by one, and not at all with explicit noise.  torch.equal on every output."""
    c = RU.build(case, "midpoint", ns=7)
    ids, G = _ids("three", c["B"])
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        a = _calib(eng, flat, c, is_post, ids, G)
        assert _all_same(a, _calib(eng, flat, c, is_post, ids, G)) and _all_same(a, _calib(loop, flat, c, is_post, ids, G))
        for e in (eng, loop):
            e.rng_seed(77, first_trajectory=1000)
            e.rng_set_counter(5)
        drawn = _calib(eng, flat, c, is_post, ids, G, eps=None)
        assert eng.rng_state() == (77, 1000, 6)
        rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
        given = _calib(eng, flat, c, is_post, ids, G, eps=rows)
        assert eng.rng_state() == (77, 1000, 6)                                           # explicit noise draws nothing
        assert _all_same(drawn, given) and _all_same(drawn, _calib(loop, flat, c, is_post, ids, G, eps=None))
        assert not _all_same(a, drawn)


@pytest.mark.parametrize("case", ["cvs_ald", "challenge_gauss"])
def test_integer_outputs_do_not_depend_on_the_chunk(case):
    """chunk 1 against 4 against 64: torch.equal on the integer outputs; the float outputs within twice KU.accumulation_bar (pinball terms
    are non-negative: their mean absolute value is the output itself; the width's is at most the oracle's mean |v_1| + |v_2|).  And the
    sum over the cohorts of a partition equals the one-cohort call exactly, for the integer outputs."""
    c = RU.build(case, "rk4", B=11, ns=3)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    ids, G = _ids("parts", 11)
    for is_post in (True, False):
        got = {R: _calib(eng, flat, c, is_post, ids, G, chunk=R) for R in (1, 4, 64)}
        scale = KU.oracle_calibration(c, is_post, ids, G)["scale"]
        for R in (4, 64):
            assert all(torch.equal(x, y) for x, y in zip(got[R][:3], got[1][:3]))
            pin, pin1 = got[R][3].double().cpu().numpy(), got[1][3].double().cpu().numpy()
            assert np.all(np.abs(pin - pin1) <= 2 * KU.accumulation_bar(np.maximum(pin, pin1)))
            wid, wid1 = got[R][4].double().cpu().numpy(), got[1][4].double().cpu().numpy()
            assert np.all(np.abs(wid - wid1) <= 2 * KU.accumulation_bar(scale[1] + scale[2]))
            print("%s post=%s chunk %d vs 1: pinball equal %s, width equal %s" % (case, is_post, R, np.array_equal(pin, pin1), np.array_equal(wid, wid1)))
        whole = _calib(eng, flat, c, is_post, np.zeros(11, np.int64), 1, chunk=4)
        for x, y in zip(got[4][:3], whole[:3]):
            assert torch.equal(x.sum(dim=-3, keepdim=True), y)


# ---- 6. launches, capture, refusals, memory --------------------------------------------------------------------------------------------------
def test_launches_and_graph_capture():
    """Posterior: "weff", "enc_fwd2", "cohort_plan", "calibration", "calibration_merge" on one stream (a linear graph); prior: the last
    three.  One capture and one replay of a posterior call equal the stream-launched call."""
    c = RU.build("cvs_ald", "rk4", ns=7)
    ids, G = _ids("three", c["B"])
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps = c["eps"].to(DEV).contiguous()
    eng.profile_enable(True)
    _calib(eng, flat, c, True, ids, G)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "cohort_plan", "calibration", "calibration_merge"]
    _calib(eng, flat, c, False, ids, G)
    assert [n for n, _ in eng.profile_read()] == ["cohort_plan", "calibration", "calibration_merge"]
    eng.profile_enable(False)
    members, offsets = _lists(ids, G)
    T = c["T"]
    out = [torch.zeros(3, G, 3, T, dtype=torch.int32, device=DEV), torch.zeros(G, 3, T, dtype=torch.int32, device=DEV),
           torch.zeros(G, 3, T, dtype=torch.int32, device=DEV), torch.zeros(3, G, 3, device=DEV), torch.zeros(G, 3, device=DEV)]
    scratch = torch.zeros(eng.calibration_plan(c["B"], members.numel(), G, 7, 3)[3] // 4, device=DEV)
    bt = eng.make_batch(obs_d, labels, eps, particles=7)
    call = lambda: eng.calibration(flat, bt, c["B"], True, 7, members, offsets, G, 3, *out, scratch=scratch)
    want = _captured(call, out)
    assert _all_same(out, want) and bool(torch.isfinite(out[3][:, :2]).all()) and int(out[0].sum()) > 0   # (cohort 2 of these ids is empty)


def test_refusals_write_nothing_and_draw_nothing(monkeypatch):
    """Every refusal names its reason, draws nothing, launches nothing (rng_state, profile_read) and leaves the outputs as they were."""
    from structured_latent_odes_amd import _lib as L
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)
    ids, G = _ids("three", c["B"])
    members, offsets = _lists(ids, G)

    def refused(eng, match, obs=obs_d, ns=2, is_post=True, G=G, chunk=0, offsets=offsets, scratch=None):
        flat = eng.pack(c["p"])
        below = torch.full((3, max(G, 1), 3, c["T"]), 7, dtype=torch.int32, device=DEV)
        pinball = torch.full((3, max(G, 1), 3), 7.0, device=DEV)
        _refused(eng, lambda: eng.calibration(flat, eng.make_batch(obs, labels, None), c["B"], is_post, ns, members, offsets, G, chunk=chunk,
                                              below=below, pinball=pinball, outputs=(), scratch=scratch), match)
        torch.cuda.synchronize(DEV)
        assert bool((below == 7).all()) and bool((pinball == 7.0).all())

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
    refused(eng, "comparisons need dense", obs=padded, is_post=False, scratch=some)
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms", scratch=some)
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD", scratch=some)
    # tables beyond the LDS of one CU: T = 1024
    from structured_latent_odes_amd import engine as E
    big = E.Engine(E.proc_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    with pytest.raises(L.SlodeError, match="LDS tables"):
        big.calibration(torch.zeros(big.n_params, device=DEV), big.make_batch(torch.zeros(2, 4, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["proc"]], None),
                        2, False, 2, torch.zeros(2, dtype=torch.int32, device=DEV), torch.tensor([0, 2], dtype=torch.int32, device=DEV), 1, scratch=some)
    assert big.rng_state()[2] == 0


@pytest.mark.parametrize("is_post", [True, False])
def test_memory_does_not_grow_with_the_draws(is_post):
    """After a warm-up call, the peak of torch.cuda.max_memory_allocated over the allocation before the call is identical at ns = 8 and
    ns = 200, and at ns = 8 below that of the composed route (recon_samples plus comparisons)."""
    m, batches = _model_batches("cvs")
    batch = _on_device(batches[0], "cvs")                                                   # 24 trajectories
    eng = m._bind().engine
    B = batch["observations"].shape[0]
    ids = torch.arange(B, device=DEV) % 2
    labels = {k: v for k, v in batch.items() if k != "observations"}
    m.calibration(is_post=is_post, num_samples=8, cohorts=ids, chunk=8, **batch)
    eng.profile_enable(True)
    fused = []
    for ns in (8, 200):
        fused.append(_peak(lambda: m.calibration(is_post=is_post, num_samples=ns, cohorts=ids, chunk=8, **batch)))
        assert [n for n, _ in eng.profile_read()][-1] == "calibration_merge"              # the fused route, not the composition
    eng.profile_enable(False)
    _, _, G, _, _, count = m._cohort_lists(batch["observations"], ids, None, labels)
    composed = _peak(lambda: m._calibration_composed(batch["observations"], is_post, 8, ids, G, count, None, labels))
    print("peak over the allocation before the call: ns=8 %d B, ns=200 %d B; composed at ns=8 %d B" % (fused[0], fused[1], composed))
    assert fused[0] == fused[1] and fused[0] < composed


# ---- 6. the model route ------------------------------------------------------------------------------------------------------------------------
def _hand_made(m, batch, is_post, ns, ids, G, eps=None):
    """KU.reduce_by_cohort of recon_samples (drawn from the engine's current generator state, or from ``eps``) in numpy, the near points
    at twice the bar: the decoder's fp32 curves and the fused kernel's are two evaluations, each within the bar of the truth."""
    res = m.recon_samples(is_post=is_post, num_samples=ns, eps=eps, **batch)
    v = np.stack([x.cpu().numpy() for x in m._calibration_curves(res)])                   # [3, B, C, T, ns] fp32
    return KU.reduce_by_cohort(batch["observations"].cpu().numpy(), np.moveaxis(v, 4, 1), m.calibration_nominal().numpy(), ids, G, factor=2.0)


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_result(fam):
    """Default cohort, an id tensor with an empty cohort and an excluded trajectory, a label-name tuple (keys): the fused route (its last
    launch is calibration_merge), one drawing call; the fractions equal counts over count x ns; against the hand-made reduction of
    recon_samples from the same generator state by the comparison rule on the model's own curves."""
    m, batch = _model(fam)
    eng = m._bind().engine
    B, T = batch["observations"].shape[0], batch["observations"].shape[2]
    ids_t = torch.tensor([(i * 7) % 3 for i in range(B)], device=DEV) * 2                   # cohorts 0, 2, 4: 1 and 3 empty
    ids_t[5] = -1
    labels = {k: v for k, v in batch.items() if k != "observations"}
    ns = 12
    for cohorts, kw in ((None, {}), (ids_t, dict(num_cohorts=6)), (tuple(m.LABELS), {})):
        for is_post in (True, False):
            eng.rng_seed(4321, first_trajectory=300)
            eng.rng_set_counter(9)
            eng.profile_enable(True)
            got = m.calibration(is_post=is_post, num_samples=ns, cohorts=cohorts, **kw, **batch)
            assert [n for n, _ in eng.profile_read()][-1] == "calibration_merge" and eng.rng_state() == (4321, 300, 10)
            eng.profile_enable(False)
            G = got["count"].numel()
            if cohorts is None:
                ids = np.zeros(B, np.int64)
                assert G == 1 and got["count"].tolist() == [B]
            elif torch.is_tensor(cohorts):
                ids = ids_t.cpu().numpy()
                assert got["count"].tolist() == [int((ids == g).sum()) for g in range(6)] and got["count"][1] == 0
            else:
                ids_l, keys = m.cohort_index(by=cohorts, **labels)
                ids = ids_l.cpu().numpy()
                assert torch.equal(got["keys"], keys)
            den = (got["count"].double() * ns).view(G, 1, 1)
            for n in ("below", "inside", "cross"):
                assert got["counts"][n].dtype == torch.int32 and got[n + "_t"].dtype == torch.float64
                assert torch.equal(torch.nan_to_num(got[n + "_t"], nan=-1.0), torch.nan_to_num(got["counts"][n].double() / den, nan=-1.0))
                assert torch.equal(torch.nan_to_num(got[n], nan=-1.0), torch.nan_to_num(got["counts"][n].long().sum(-1).double() / (den[..., 0] * T), nan=-1.0))
            assert torch.equal(got["nominal"], m.calibration_nominal()) and tuple(got["below"].shape) == (3, G, batch["observations"].shape[1])
            eng.rng_set_counter(9)
            want = _hand_made(m, batch, is_post, ns, ids, G)
            KU.check((got["counts"]["below"], got["counts"]["inside"], got["counts"]["cross"], got["pinball"], got["width"]), want,
                     "%s cohorts=%s post=%s against the decoder's curves" % (fam, type(cohorts).__name__, is_post), ns)


@pytest.mark.parametrize("why", ["dopri5", "strided", "SLODE_ODE_ALG"])
def test_model_level_call_is_total_over_what_the_engine_refuses(why, monkeypatch):
    """dopri5, a padded observation tensor, a measured arm: the engine refuses, MechanisticBase.calibration composes the dict from
    recon_samples -- equal to the hand-made reduction of recon_samples of the same generator state, the integer outputs exactly; one
    drawing call."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch, {why: "1"} if why.startswith("SLODE") else None)
    eng = m._bind().engine
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    ns = 6
    labels = {k: v for k, v in batch.items() if k != "observations"}
    eng.rng_seed(11)
    got = m.calibration(is_post=True, num_samples=ns, cohorts=("iext", "rtpr"), **batch)
    assert eng.rng_state()[2] == 1
    eng.rng_set_counter(0)
    ids = m.cohort_index(by=("iext", "rtpr"), **labels)[0].cpu().numpy()
    G = got["count"].numel()
    want = _hand_made(m, batch, True, ns, ids, G)
    cnt = want["counts"]
    assert eng.rng_state()[2] == 1 and got["count"].tolist() == [int((ids == g).sum()) for g in range(G)]
    assert np.array_equal(got["counts"]["below"].cpu().numpy(), cnt[:3]) and np.array_equal(got["counts"]["inside"].cpu().numpy(), cnt[3])
    assert np.array_equal(got["counts"]["cross"].cpu().numpy(), cnt[4]) and got["counts"]["below"].dtype == torch.int32
    assert np.allclose(got["pinball"].cpu().numpy(), want["pinball"], rtol=1e-5) and np.allclose(got["width"].cpu().numpy(), want["width"], rtol=1e-5)



def test_more_than_1024_cohorts_are_composed():
    m, batches = _model_batches("cvs")
    batch = _on_device(batches[0], "cvs")
    B = batch["observations"].shape[0]
    got = m.calibration(is_post=False, num_samples=2, cohorts=torch.arange(B, device=DEV) * 50, num_cohorts=1200, **batch)
    assert got["count"].numel() == 1200 and int(got["count"].sum()) == B and tuple(got["counts"]["below"].shape) == (3, 1200, 3, 86)
    assert int(got["counts"]["below"][:, 1].abs().max()) == 0 and torch.isnan(got["pinball"][:, 1]).all() and bool(torch.isfinite(got["pinball"][:, 50]).all())


# ---- 7. files and the entry point ----------------------------------------------------------------------------------------------------------
def test_save_calibration_over_two_batches_equals_their_concatenation(tmp_path):
    """The same 48 trajectories as two batches of 24 and as one batch, every batch carrying its cohort ids and its rows of ONE noise tensor
    (the keys ``cohorts`` and ``eps`` of a batch dict): integer files exactly, float files to rounding -- each fused mean within
    KU.accumulation_bar of the exact mean of its fp32 summands, one more rounding for the pooled fp32 inputs.  Names and shapes."""
    m, batches = _model_batches("cvs")
    two = [_on_device(b, "cvs") for b in batches[:2]]
    cat = {k: torch.cat([b[k] for b in two], 0) for k in two[0]}
    cat["observations"] = cat["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    ns, L = 5, m._bind().engine.spec.latent_dim
    eps = torch.randn(ns, 48, L, generator=torch.Generator().manual_seed(5)).to(DEV)
    ids = torch.arange(48, device=DEV) % 3
    loader = [dict(b, cohorts=ids[lo:lo + 24], eps=eps[:, lo:lo + 24].contiguous()) for lo, b in ((0, two[0]), (24, two[1]))]
    files, pooled = m.save_calibration(str(tmp_path / "two"), loader, False, ns)
    files1, one = m.save_calibration(str(tmp_path / "one"), [dict(cat, cohorts=ids, eps=eps)], False, ns)
    names = ["calibration_%s_prior.npy" % n for n in ("below", "below_t", "inside", "cross", "pinball", "width")] + ["calibration_nominal.npy", "calibration_count.npy"]
    assert [os.path.basename(f) for f in files] == names and sorted(os.listdir(str(tmp_path / "two"))) == sorted(names)
    shapes = dict(zip(names, [(3, 3, 3), (3, 3, 3, 86), (3, 3), (3, 3), (3, 3, 3), (3, 3), (3,), (3,)]))
    v = m._calibration_curves(m.recon_samples(is_post=False, num_samples=ns, eps=eps, **cat))
    mabs = {"pinball": np.load(files1[4]), "width": float((v[1] - v[2]).abs().max())}   # pinball terms are >= 0; |width term| <= its maximum
    for f, f1 in zip(files, files1):
        n, a, b = os.path.basename(f), np.load(f), np.load(f1)
        assert a.shape == shapes[n] == b.shape, n
        kind = "pinball" if "pinball" in n else ("width" if "width" in n else None)
        if kind:
            assert np.all(np.abs(a - b) <= 3 * KU.accumulation_bar(mabs[kind])), n
        else:
            assert np.array_equal(a, b), n
    for n in ("below", "inside", "cross"):
        assert pooled["counts"][n].dtype == np.int64 and np.array_equal(pooled["counts"][n], one["counts"][n])
    assert np.load(files[7]).tolist() == [16, 16, 16] and np.load(files[6]).tolist() == m.calibration_nominal().tolist()
    below_t = np.load(files[1])
    assert np.array_equal(below_t, pooled["counts"]["below"] / (16 * ns)) and 0.0 < below_t.mean() < 1.0


def test_training_entry_point_with_calibration(tmp_path, capsys):
    tr = importlib.import_module("training_cvs")
    cfg = EU.model_config("cvs")
    cfg.update(num_epochs=0, mini_batch_size=16, seq_len=86, num_samples=5)
    tr.train(cfg, batches_per_epoch=1, calibration=True, results_dir=str(tmp_path / "res"))
    out = capsys.readouterr().out
    assert "FINAL TEST:" in out and "calibration_post: tau=0.5000:" in out and "calibration_prior: tau=0.5000:" in out
    line = out.split("calibration_post: ")[1].splitlines()[0]
    assert "band=" in line and "crossing=" in line and "pinball=(" in line and np.isfinite(float(line.split("band=")[1].split()[0]))
    got = sorted(os.listdir(str(tmp_path / "res")))
    want = sorted(["calibration_%s_%s.npy" % (n, s) for n in ("below", "below_t", "inside", "cross", "pinball", "width") for s in ("post", "prior")]
                  + ["calibration_nominal.npy", "calibration_count.npy"])
    assert got == want
    assert np.load(str(tmp_path / "res" / "calibration_below_t_prior.npy")).shape == (3, 1, 3, 86)
    assert np.load(str(tmp_path / "res" / "calibration_count.npy")).tolist() == [16]
