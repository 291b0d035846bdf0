"""GPU tests of the latent attribution (slode_latent_attribution / Engine.latent_attribution / MechanisticBase.latent_attribution /
save_latent_attribution) against the fp64 oracle composed in tests/attribution_util.py, against recon_moments on the same base noise and
against the materialising composition.  Bars: module docstring of tests/attribution_util.py (the project's per-value bar for the base mean
and sd; for msd the two arms' bars carried through the squared difference, plus the fp32 accumulation term)."""
import os

import numpy as np
import pytest
import torch

from tests import attribution_util as AU
from tests import eval_stats_util as EU
from tests import recon_moments_util as RU
from tests.eval_gpu_util import (ADAPTIVE, DEV, ENV_KEYS, SIZES, WIDTHS, _captured, _count_calls, _device_batch, _engine, _eps_dev, _model, _padded,
                                 _peak, _recon_moments, _refused)
from tests.eval_gpu_util import _attr

pytestmark = pytest.mark.gpu


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_against_the_fp64_oracle(case, solver):
    """Explicit noise, ns = 7; six model classes x three fixed-grid solvers x posterior / prior; the arms of the family: every single block
    and every complement (cvs: six arms, challenge and proc: two)."""
    c = AU.build(case, solver, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    masks, _, _ = AU.arm_masks(c["ospec"])
    for is_post in (True, False):
        got = _attr(eng, flat, c, is_post, masks, obs_d=obs_d, labels=labels)
        AU.check(got, AU.oracle_moments(c, is_post, masks), "%s/%s/%s" % (case, solver, "post" if is_post else "prior"))


@pytest.mark.parametrize("case,B,ns,env", SIZES, ids=["%s-B%d-ns%d%s" % (c, B, ns, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, ns, e in SIZES])
def test_sizes_and_instantiations(case, B, ns, env, monkeypatch):
    """The grid of tests/test_gpu_recon_moments.py: B on both sides of the 64- and 256-thread edges, the persistent loop on 5 and 2
    workgroups, the run-time-S instantiation, ns in {1, 2, 7, 200} (200 at B <= 3), rk4, every arm of the family, posterior and prior,
    NaN-poisoned workspace.  ns = 1: sd is exactly 0."""
    c = AU.build(case, "rk4", B=B, ns=ns)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    masks, _, _ = AU.arm_masks(c["ospec"])
    for is_post in (True, False):
        got = _attr(eng, flat, c, is_post, masks)
        AU.check(got, AU.oracle_moments(c, is_post, masks), "%s B=%d ns=%d %s %s" % (case, B, ns, env, "post" if is_post else "prior"))
        if ns == 1:
            assert float(got[1].abs().max()) == 0.0


@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_exact_zeros_and_the_base_against_recon_moments(case):
    """An arm with mask 0 is exactly 0, whatever the other arms; with the fresh rows equal to the base rows every arm is exactly 0.  The
    base mean / sd agree with recon_moments on the same base noise within the RU bars (printed: whether bitwise), posterior and prior."""
    c = AU.build(case, "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    masks, _, _ = AU.arm_masks(c["ospec"])
    same = torch.stack([c["eps"], c["eps"]]).to(DEV).contiguous()
    for is_post in (True, False):
        mean, sd, msd = _attr(eng, flat, c, is_post, [masks[0], 0, masks[-1]])
        assert float(msd[1].abs().max()) == 0.0 and float(msd[0].abs().max()) > 0.0 and float(msd[2].abs().max()) > 0.0
        _, _, zero = _attr(eng, flat, c, is_post, masks, eps=same)
        assert float(zero.abs().max()) == 0.0
        rm, rs = _recon_moments(eng, flat, c, is_post)
        print("%s %s: base bitwise equal to recon_moments: mean %s, sd %s" % (case, "post" if is_post else "prior", torch.equal(mean, rm), torch.equal(sd, rs)))
        RU.check(mean, sd, rm.double().cpu().numpy(), rs.double().cpu().numpy(), "%s base against recon_moments" % case)


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_noise_and_independence(case, monkeypatch):
    """In-kernel noise at seed 19, counter 3: the counter is afterwards at 5 and every output equals, bit for bit, the call on the explicit
    tensor read back with rng_normal(3), rng_normal(4) (which draws nothing).  Arm a alone equals column a of the all-arms call; one
    workgroup per trajectory equals a 3-workgroup loop; two runs are equal; outputs the caller does not want leave the others unchanged."""
    c = AU.build(case, "midpoint", ns=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    masks, _, _ = AU.arm_masks(c["ospec"])
    B = c["B"]
    for is_post in (True, False):
        a = _attr(eng, flat, c, is_post, masks)
        assert _equal(a, _attr(eng, flat, c, is_post, masks)) and _equal(a, _attr(loop, flat, c, is_post, masks))
        for i, m in enumerate(masks):
            mean, sd, msd = _attr(eng, flat, c, is_post, [m])
            assert torch.equal(msd[0], a[2][i]) and torch.equal(mean, a[0]) and torch.equal(sd, a[1]), (case, is_post, hex(m))
        for e in (eng, loop):
            e.rng_seed(19)
            e.rng_set_counter(3)
        drawn = _attr(eng, flat, c, is_post, masks, eps=None)
        assert eng.rng_state() == (19, 0, 5)
        rows = torch.stack([eng.rng_normal(3, 7 * B).view(7, B, -1), eng.rng_normal(4, 7 * B).view(7, B, -1)]).contiguous()
        given = _attr(eng, flat, c, is_post, masks, eps=rows)
        assert eng.rng_state() == (19, 0, 5)                                          # explicit noise draws nothing
        assert _equal(drawn, given) and _equal(drawn, _attr(loop, flat, c, is_post, masks, eps=None))
        assert float(drawn[2].abs().max()) > 0.0 and not _equal(drawn[2:], a[2:])
        bt = eng.make_batch(*_device_batch(c), c["eps2"].to(DEV).contiguous(), particles=7, eps_shape=tuple(c["eps2"].shape))
        only = eng.latent_attribution(flat, bt, B, is_post, 7, masks, False, False)
        assert only[0] is None and only[1] is None and torch.equal(only[2], a[2])


def test_launches_and_graph_capture():
    """Posterior: three launches, "weff", "enc_fwd2", "latent_attribution", on one stream; prior: "latent_attribution" alone.  One capture and
    one replay equal the stream-launched call bitwise; capturing executes nothing."""
    c = AU.build("cvs_ald", "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    masks, _, _ = AU.arm_masks(c["ospec"])
    eng.profile_enable(True)
    _attr(eng, flat, c, True, masks)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "latent_attribution"]
    _attr(eng, flat, c, False, masks)
    assert [n for n, _ in eng.profile_read()] == ["latent_attribution"]
    eng.profile_enable(False)
    outs = [torch.zeros(3, c["B"], 3, c["T"], device=DEV), torch.zeros(3, c["B"], 3, c["T"], device=DEV), torch.zeros(len(masks), 3, c["B"], 3, c["T"], device=DEV)]
    bt = eng.make_batch(obs_d, labels, c["eps2"].to(DEV).contiguous(), particles=7, eps_shape=tuple(c["eps2"].shape))
    want = _captured(lambda: eng.latent_attribution(flat, bt, c["B"], True, 7, masks, *outs), outs)
    assert _equal(outs, want) and float(outs[2].abs().max()) > 0.0


def test_refusals_by_name(monkeypatch):
    """Every refusal names its reason, draws nothing and launches nothing (rng_state, profile_read)."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd import engine as E
    c = AU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)

    def refused(eng, match, obs=obs_d, ns=2, particles=1, masks=(1, 6), is_post=True, null_obs=False):
        flat = eng.pack(c["p"])
        bt = eng.make_batch(obs, labels, None)
        if null_obs:
            bt.obs = None
        err = _refused(eng, lambda: eng.latent_attribution(flat, bt, c["B"], is_post, ns, list(masks), particles=particles), match)
        assert err.status == -1 and "slode_latent_attribution" in str(err)

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s" % solver, is_post=solver != "bosh3")
    eng = _engine(c, monkeypatch)
    for is_post in (True, False):
        refused(eng, "particles = 2", particles=2, is_post=is_post)
        refused(eng, "num_samples = 0", ns=0, is_post=is_post)
        refused(eng, "exceeds 2\\^30 - 1 noise rows", ns=2 ** 30, is_post=is_post)   # refused on the host: nothing sized by it is touched
        refused(eng, "n_arms = 0 out of range \\[1, 16\\]", masks=(), is_post=is_post)
        refused(eng, "n_arms = 17 out of range \\[1, 16\\]", masks=(1,) * 17, is_post=is_post)
        refused(eng, "arm_masks\\[1\\] = 0x8 has bits beyond n_groups = 2", masks=(1, 8), is_post=is_post)
        refused(eng, "arm_masks\\[0\\] = 0x80000000 has bits beyond", masks=(1 << 31,), is_post=is_post)
    refused(eng, "batch->obs is NULL", null_obs=True)
    refused(eng, "observation strides", obs=_padded(obs_d))
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    # tables beyond the LDS of one CU: T = 1024 with S = 8, C = 4, three heads (the environment of the previous engines cleared first)
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    big = E.Engine(E.proc_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    big.profile_enable(True)
    with pytest.raises(L.SlodeError, match="LDS tables of T = 1024, S = 8, C = 4, n_arms = 2"):
        big.latent_attribution(torch.zeros(big.n_params, device=DEV), big.make_batch(torch.zeros(2, 4, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["proc"]], None),
                               2, True, 2, [1, 2])
    assert big.rng_state()[2] == 0
    with pytest.raises(L.SlodeError, match="no profiled step"):
        big.profile_read()
    with pytest.raises(L.SlodeError, match="n_arms = 2"):
        big.attribution_plan(2, 2)


# ---- the model layer ---------------------------------------------------------------------------------------------------------------------
KEYS = ("mean", "var", "total", "first", "total_index", "first_index")


def _materialised(m, batch, is_post, eps, masks):
    """The per-draw curves of the base and of every arm from the model's own decoder on the same two noise tensors, as fp64 numpy
    [Q, ns, B, C, T]: what the composed route reduces, kept whole here for the bars (the d_k of tests/attribution_util.py)."""
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    labels = {k: v for k, v in batch.items() if k != "observations"}
    with torch.no_grad():
        loc, scale = m._loc_scale(batch["observations"], is_post, labels)

        def curves(e):
            d = m._decoded_draws(loc.unsqueeze(0) + scale.unsqueeze(0) * e)
            return np.stack([d[n].double().permute(3, 0, 1, 2).cpu().numpy() for n in names])
        return curves(eps[0]), [curves(torch.where(m._block_dims(k).to(DEV), eps[1], eps[0])) for k in masks]


def _check_model(res, m, v, arms, single, comp, tag):
    """The dict of latent_attribution against the materialised curves: mean within RU.MEAN_BAR x max(1, |mean|); var = sd^2, so within
    2 sd b + b^2 with b = RU.SD_BAR x max(1, |mean|); total within AU.msd_bar; first = var - msd within the sum of the two."""
    worst = 0.0
    for q, n in enumerate(m.MOMENT_HEADS[bool(m.GAUSS)]):
        r = {k: res[n][k].double().cpu().numpy() for k in KEYS}
        mean, sd = np.mean(v[q], 0), np.std(v[q], 0)
        scale = np.maximum(1.0, np.abs(mean))
        b = RU.SD_BAR * scale
        var_bar = 2.0 * sd * b + b * b
        ratios = [np.abs(r["mean"] - mean) / (RU.MEAN_BAR * scale), np.abs(r["var"] - sd * sd) / var_bar]
        for p in range(len(single)):
            vs, vc = arms[single[p]], arms[comp[p]]
            ratios.append(np.abs(r["total"][p] - AU.msd64(v, vs)[q]) / AU.msd_bar(v, vs)[q])
            ratios.append(np.abs(r["first"][p] - (sd * sd - AU.msd64(v, vc)[q])) / (var_bar + AU.msd_bar(v, vc)[q]))
        assert all(np.isfinite(x).all() for x in r.values()), (tag, n)
        worst = max(worst, max(float(x.max()) for x in ratios))
    print("%s: largest error / bar over mean, var, total, first: %.3e" % (tag, worst))
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_model_level_dict_routes_split_and_identity(fam, monkeypatch):
    """Names and shapes of the dict for all three families; the fused route seen in profile_read (three launches for the posterior, one
    for the prior); values against the model's own materialised curves on the same noise; splitting the arms one per call changes no bit;
    for the two-block families first_index[0] = 1 - total_index[1] within the rounding of first = fl(var - msd):
    2^-24 (sum_t var + sum_t msd) / sum_t var."""
    m, batch = _model(fam)
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    blocks, masks, single, comp = m._attribution_arms(None)
    B, Cn, T = batch["observations"].shape
    ns = 12
    eps = torch.randn(2, ns, B, m.latent_dim, generator=torch.Generator().manual_seed(5)).to(DEV)
    eng = m._bind().engine
    assert blocks == {"cvs": ["iext", "rtpr", "epsilon"], "challenge": ["shedding+symptoms", "epsilon"], "proc": ["aR+aS+C12+C6", "epsilon"]}[fam]
    assert len(masks) == (6 if fam == "cvs" else 2) and eng.attribution_blocks() == len(blocks)
    for is_post in (True, False):
        tag = "%s %s" % (fam, "post" if is_post else "prior")
        eng.profile_enable(True)
        res = m.latent_attribution(is_post=is_post, num_samples=ns, eps=eps, **batch)
        assert [k for k, _ in eng.profile_read()] == (["weff", "enc_fwd2", "latent_attribution"] if is_post else ["latent_attribution"])
        eng.profile_enable(False)
        assert res["blocks"] == blocks and set(res) == {"blocks"} | set(names)
        P = len(blocks)
        for n in names:
            r = res[n]
            assert set(r) == set(KEYS) and tuple(r["mean"].shape) == tuple(r["var"].shape) == (B, Cn, T)
            assert tuple(r["total"].shape) == tuple(r["first"].shape) == (P, B, Cn, T)
            assert tuple(r["total_index"].shape) == tuple(r["first_index"].shape) == (P, B, Cn) and r["first_index"].dtype == torch.float64
            assert float(r["total"].min()) >= 0.0 and float(r["total_index"].min()) > 0.0
            if P == 2:
                den = r["var"].double().sum(-1)
                bar = AU.U24 * (den + r["total"][1].double().sum(-1)) / den + 1e-15
                gap = (r["first_index"][0] - (1.0 - r["total_index"][1])).abs() / bar
                print("%s %s: |first_index[0] - (1 - total_index[1])| / bar %.3e" % (tag, n, float(gap.max())))
                assert float(gap.max()) <= 1.0
        v, arms = _materialised(m, batch, is_post, eps, masks)
        _check_model(res, m, v, arms, single, comp, tag + " fused")
        monkeypatch.setattr(type(m), "ATTRIBUTION_ARMS_PER_CALL", 1)
        eng.profile_enable(True)
        split = m.latent_attribution(is_post=is_post, num_samples=ns, eps=eps, **batch)
        assert [k for k, _ in eng.profile_read()] == (["weff", "enc_fwd2", "latent_attribution"] if is_post else ["latent_attribution"])   # (the last call's)
        eng.profile_enable(False)
        monkeypatch.setattr(type(m), "ATTRIBUTION_ARMS_PER_CALL", None)
        assert all(torch.equal(split[n][k], res[n][k]) for n in names for k in KEYS), tag
    # in-kernel noise: one call and the split leave the counter at n + 2 and agree bit for bit
    eng.rng_seed(23)
    eng.rng_set_counter(6)
    one = m.latent_attribution(is_post=True, num_samples=ns, **batch)
    assert eng.rng_state() == (23, 0, 8)
    eng.rng_set_counter(6)
    monkeypatch.setattr(type(m), "ATTRIBUTION_ARMS_PER_CALL", 1)
    split = m.latent_attribution(is_post=True, num_samples=ns, **batch)
    assert eng.rng_state() == (23, 0, 8)
    assert all(torch.equal(split[n][k], one[n][k]) for n in names for k in KEYS)


@pytest.mark.parametrize("why", ["dopri5", "strided"])
def test_composed_route_where_the_engine_refuses(why, monkeypatch):
    """dopri5, a padded observation tensor: the engine refuses, latent_attribution composes the dict from the decoder's per-draw curves --
    two drawing calls, the counter at n + 2 -- and agrees with those curves reduced here within the bars; on the fixed-grid model the
    composed route (padded observations) also agrees with the fused call (dense observations, same noise) within the same bars."""
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch)
    eng = m._bind().engine
    blocks, masks, single, comp = m._attribution_arms(None)
    B, ns = batch["observations"].shape[0], 6
    dense = dict(batch)
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    calls = _count_calls(monkeypatch, eng, "latent_attribution")
    eng.rng_seed(11)
    eng.rng_set_counter(2)
    drawn = m.latent_attribution(is_post=True, num_samples=ns, **batch)
    assert eng.rng_state() == (11, 0, 4) and len(calls) == 1                        # refused once, then composed
    eps = torch.stack([eng.rng_normal(2, ns * B).view(ns, B, -1), eng.rng_normal(3, ns * B).view(ns, B, -1)])
    given = m.latent_attribution(is_post=True, num_samples=ns, eps=eps, **batch)
    names = m.MOMENT_HEADS[bool(m.GAUSS)]
    assert all(torch.equal(given[n][k], drawn[n][k]) for n in names for k in KEYS)
    v, arms = _materialised(m, batch, True, eps, masks)
    _check_model(given, m, v, arms, single, comp, "%s composed" % why)
    assert float(given["mu_50"]["total"].max()) > 0.0 and given["mu_50"]["total"].dtype == torch.float32
    if why == "strided":
        calls.clear()
        fused = m.latent_attribution(is_post=True, num_samples=ns, eps=eps, **dense)
        assert len(calls) == 1
        _check_model(fused, m, v, arms, single, comp, "fused against the composed route's curves")


def test_memory_stays_below_one_materialised_arm():
    """After a warm-up call, the peak of torch.cuda.max_memory_allocated of the fused call at ns = 200 over the allocation before it stays
    below the size of ONE materialised arm (Q x ns x B x C x T floats); the composed route needs 1 + A of them."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    m.latent_attribution(is_post=True, num_samples=8, **batch)
    eng.profile_enable(True)
    peak = _peak(lambda: m.latent_attribution(is_post=True, num_samples=200, **batch))
    assert [n for n, _ in eng.profile_read()][-1] == "latent_attribution"           # the fused route, not the composition
    eng.profile_enable(False)
    one_arm = 3 * 200 * B * Cn * T * 4
    print("peak over the allocation before the call: fused ns=200 %d B; one materialised arm %d B" % (peak, one_arm))
    assert peak < one_arm


def test_output_files(tmp_path):
    """save_latent_attribution over two batches: the four arrays and the block names, equal to latent_attribution from the same generator
    state, the trajectories in loader order."""
    m, batch = _model("challenge")
    eng = m._bind().engine
    B, Cn, T = batch["observations"].shape
    halves = [{k: v[:9] for k, v in batch.items()}, {k: v[9:] for k, v in batch.items()}]
    halves = [dict(h, observations=h["observations"].permute(0, 2, 1).contiguous().permute(0, 2, 1)) for h in halves]
    eng.rng_seed(8)
    files = m.save_latent_attribution(str(tmp_path / "at"), halves, True, 5)
    assert eng.rng_state()[2] == 4
    want = ["attribution_%s_post.npy" % k for k in ("total", "first", "total_index", "first_index")] + ["attribution_blocks.txt"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "at"))) == sorted(want)
    assert open(files[-1]).read().split() == ["shedding+symptoms", "epsilon"]
    total, first, ti, fi = (np.load(f) for f in files[:4])
    Q = len(m.MOMENT_HEADS[bool(m.GAUSS)])
    assert total.shape == first.shape == (Q, 2, B, Cn, T) and total.dtype == np.float32 and ti.shape == fi.shape == (Q, 2, B, Cn) and ti.dtype == np.float64
    assert np.isfinite(total).all() and np.isfinite(fi).all()
    eng.rng_set_counter(2)
    res = m.latent_attribution(is_post=True, num_samples=5, **halves[1])
    n0 = m.MOMENT_HEADS[bool(m.GAUSS)][0]
    assert np.array_equal(total[0][:, 9:], res[n0]["total"].cpu().numpy()) and np.array_equal(fi[0][:, 9:], res[n0]["first_index"].cpu().numpy())
    print(m.attribution_line(ti, fi, "post"))
