"""GPU tests of the sample moments of the reconstruction (slode_recon_moments / Engine.recon_moments / MechanisticBase.recon_moments /
save_recon_moments / --sample-moments) against the fp64 oracle and against the materialising path (recon_samples reduced in fp64).
Bars (tests/recon_moments_util.py), derived from the suite's own bar for one head value, 1e-4 * max(1, |mu|)
(test_recon_samples_is_one_batched_launch_of_recon): a mean of values within that bar is within it; the sd is a scaled 2-norm of the
centred values, so by the triangle inequality its error is at most the same bar, and 2e-4 * max(1, |mu|) covers the accumulation.
|mu| is taken as the oracle's mean curve (max(1, |mean of mu_k|) <= mean of max(1, |mu_k|): not wider than the derivation)."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import eval_stats_util as EU
from tests import recon_moments_util as RU
from tests.eval_gpu_util import ADAPTIVE, DEV, SIZES, WIDTHS, _captured, _device_batch, _engine, _model, _padded, _peak, _refused
from tests.eval_gpu_util import _recon_moments as _moments

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("solver", EU.SOLVERS)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_moments_match_the_fp64_oracle(case, solver):
    """Explicit noise, ns = 7; six model classes x three fixed-grid solvers x {posterior, prior}; cvs / challenge in the [B,T,C] layout,
    proc in [B,C,T]."""
    c = RU.build(case, solver, ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        mean, sd = _moments(eng, flat, c, is_post)
        RU.check(mean, sd, *RU.oracle_moments(c, is_post), "%s/%s/%s" % (case, solver, "post" if is_post else "prior"))


@pytest.mark.parametrize("case,B,ns,env", SIZES, ids=["%s-B%d-ns%d%s" % (c, B, ns, "-" + "-".join(k[10:].lower() for k in e) if e else "") for c, B, ns, e in SIZES])
def test_sizes_and_instantiations(case, B, ns, env, monkeypatch):
    """B on both sides of the 64- and 256-thread edges, the persistent loop (65 and 9 trajectories on 5 and 2 workgroups), the run-time-S
    instantiation, ns in {1, 2, 7, 200} (200 at B = 3 and B = 2: the oracle stays cheap; T = 200 and T = 300), rk4, posterior and prior,
    NaN-poisoned workspace.  ns = 1: sd is exactly 0."""
    c = RU.build(case, "rk4", B=B, ns=ns)
    eng = _engine(c, monkeypatch, env)
    flat = eng.pack(c["p"])
    eng.workspace(B).fill_(float("nan"))
    for is_post in (True, False):
        mean, sd = _moments(eng, flat, c, is_post)
        RU.check(mean, sd, *RU.oracle_moments(c, is_post), "%s B=%d ns=%d %s %s" % (case, B, ns, env, "post" if is_post else "prior"))
        if ns == 1:
            assert float(sd.abs().max()) == 0.0


@pytest.mark.parametrize("case", ["cvs_ald", "proc_ald"])
def test_bitwise_reproducible_and_independent_of_the_grid(case, monkeypatch):
    """Two calls: bitwise equal.  One workgroup per trajectory against the persistent loop (3 workgroups for 37 / 16 trajectories):
    bitwise equal.  In-kernel noise against the same rows passed explicitly: bitwise equal; the counter moves by one."""
    c = RU.build(case, "midpoint", ns=7)
    eng = _engine(c, monkeypatch)
    loop = _engine(c, monkeypatch, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "3"})
    flat = eng.pack(c["p"])
    for is_post in (True, False):
        a = _moments(eng, flat, c, is_post)
        b = _moments(eng, flat, c, is_post)
        l = _moments(loop, flat, c, is_post)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0], l[0]) and torch.equal(a[1], l[1])
        for e in (eng, loop):
            e.rng_seed(77, first_trajectory=1000)
            e.rng_set_counter(5)
        drawn = _moments(eng, flat, c, is_post, eps=None)
        assert eng.rng_state() == (77, 1000, 6)
        rows = eng.rng_normal(5, 7 * c["B"]).view(7, c["B"], -1).contiguous()
        given = _moments(eng, flat, c, is_post, eps=rows)
        assert eng.rng_state() == (77, 1000, 6)                                   # explicit noise draws nothing
        drawn_loop = _moments(loop, flat, c, is_post, eps=None)
        for x, y, z in zip(drawn, given, drawn_loop):
            assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("is_post", [False, True])
def test_kernel_accumulation_on_curves_whose_sd_is_1e4_of_their_level(is_post):
    """Ties the kernel's moments (phases M6 / M7) to the numerics test of tests/test_recon_moments_cpu.py.  Noise scaled by 3e-5: the curves
    of the 20 draws differ by about 1e-4 of their level.  The kernel's own fp32 value of every draw comes from 20 calls with ns = 1
    (mean = the draw, sd = 0); the ns = 20 call is then compared with np.mean / np.std of those fp32 values in fp64 at the rounding bounds
    of RU.accumulation_bars (no term in |mean| for the sd) -- bars a plain fp32 sum of squares misses by orders of magnitude, which
    the oracle bar 2e-4 max(1, |mu|) cannot see -- and with the numpy restatement of the accumulation, to within the two bounds added."""
    ns = 20
    c = RU.build("cvs_ald", "rk4", B=5, ns=ns)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps = (3e-5 * c["eps"]).to(DEV).contiguous()
    vals = np.stack([_moments(eng, flat, c, is_post, eps=eps[k].contiguous(), obs_d=obs_d, labels=labels, ns=1)[0].cpu().numpy() for k in range(ns)])
    mean, sd = (t.cpu().numpy() for t in _moments(eng, flat, c, is_post, eps=eps, obs_d=obs_d, labels=labels))
    v64 = vals.astype(np.float64)
    want_mean, want_sd = np.mean(v64, 0), np.std(v64, 0)
    live = want_sd > 0
    assert live.mean() > 0.9 and np.all(np.abs(v64 - v64[0]).max(0) <= RU.SPREAD * want_sd)          # the condition of the bars
    ratio = float(np.median(want_sd[live] / np.abs(want_mean[live])))
    bar_mean, bar_sd = RU.accumulation_bars(want_mean, want_sd, ns)
    em, es = np.abs(mean - want_mean) / bar_mean, np.abs(sd - want_sd)[live] / bar_sd[live]
    plain = np.abs(RU.plain_moments_f32(vals)[1] - want_sd)[live] / bar_sd[live]
    print("post=%s: median sd / |mean| %.2e; kernel mean error / bar %.3f, sd error / bar %.3f; a plain sum of squares: sd error / bar %.1f (median %.1f)"
          % (is_post, ratio, em.max(), es.max(), plain.max(), np.median(plain)))
    assert ratio < 1e-3
    assert np.array_equal(sd[~live], want_sd[~live])
    assert em.max() <= 1.0 and es.max() <= 1.0
    assert np.median(plain) > 1.0                                                                    # the case tells the two forms apart
    rm, rs = RU.shifted_moments_f32(vals)
    assert np.all(np.abs(mean - rm) <= 2 * bar_mean) and np.all(np.abs(sd - rs) <= 2 * bar_sd)


def _reduce64(res, names):
    return {n: (res[n].double().mean(-1), res[n].double().std(-1, unbiased=False)) for n in names}


def _agree(got, want, tag):
    for n in want:
        RU.check(got[n][0], got[n][1], want[n][0].cpu().numpy(), want[n][1].cpu().numpy(), "%s %s" % (tag, n))


@pytest.mark.parametrize("fam", ["cvs", "proc", "challenge"])
def test_same_draw_as_recon_samples(fam):
    """From the same (seed, first_trajectory, n): recon_moments(eps=None) against recon_samples(eps=None) reduced in fp64, to the bars
    above; both leave the counter at n + 1.  ns = 1: sd exactly 0 and the mean is recon's curve of the same draw, to the per-value bar."""
    m, batch = _model(fam)
    eng = m._bind().engine
    names = ("mu_50", "mu_75", "mu_25")
    for is_post in (True, False):
        eng.rng_seed(4321, first_trajectory=300)
        eng.rng_set_counter(9)
        got = m.recon_moments(is_post=is_post, num_samples=12, **batch)
        assert eng.rng_state() == (4321, 300, 10) and set(got) == set(names)
        eng.rng_set_counter(9)
        want = _reduce64(m.recon_samples(is_post=is_post, num_samples=12, **batch), names)
        assert eng.rng_state() == (4321, 300, 10)
        _agree(got, want, "%s/%s" % (fam, "post" if is_post else "prior"))
        eng.rng_set_counter(9)
        one = m.recon_moments(is_post=is_post, num_samples=1, **batch)
        eng.rng_set_counter(9)
        rec = m.recon(is_post=is_post, **batch)
        assert eng.rng_state()[2] == 10
        for n in names:
            assert float(one[n][1].abs().max()) == 0.0
            err = ((one[n][0] - rec[n]).abs() / rec[n].abs().clamp_min(1.0)).max().item()
            assert err <= RU.MEAN_BAR, (fam, is_post, n, err)


@pytest.mark.parametrize("is_post", [True, False])
def test_memory_does_not_scale_with_the_number_of_draws(is_post):
    """The property the call exists for: after a warm-up call, the peak of torch.cuda.max_memory_allocated over the allocation before the
    call is the same at ns = 8 and at ns = 200 (the two [Q, B, C, T] outputs); the materialising path at ns = 8 already needs more."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    B = batch["observations"].shape[0]
    m.recon_moments(is_post=is_post, num_samples=8, **batch)
    fused = []
    eng.profile_enable(True)
    for ns in (8, 200):
        fused.append(_peak(lambda: m.recon_moments(is_post=is_post, num_samples=ns, **batch)))
        assert [n for n, _ in eng.profile_read()][-1] == "recon_moments"           # the fused route, not the composition
    eng.profile_enable(False)
    samples = _peak(lambda: m.recon_samples(is_post=is_post, num_samples=8, **batch))
    out_bytes = 2 * 3 * B * 3 * 86 * 4
    print("peak over the allocation before the call: fused ns=8 %d B, ns=200 %d B (outputs %d B); recon_samples ns=8 %d B" % (fused[0], fused[1], out_bytes, samples))
    assert fused[0] == fused[1]
    assert fused[1] < samples


def test_refusals_by_name(monkeypatch):
    """Every refusal names its reason, draws nothing and launches nothing (rng_state, profile_read)."""
    from structured_latent_odes_amd import _lib as L
    c = RU.build("cvs_ald", "rk4", ns=2)
    obs_d, labels = _device_batch(c)

    def refused(eng, match, obs=obs_d, ns=2, particles=1, is_post=True):
        flat = eng.pack(c["p"])
        _refused(eng, lambda: eng.recon_moments(flat, eng.make_batch(obs, labels, None), c["B"], is_post, ns, particles=particles), match)

    for solver in ADAPTIVE:
        refused(_engine(c, monkeypatch, solver=solver), "adaptive solver %s" % solver)
    eng = _engine(c, monkeypatch)
    refused(eng, "particles = 2", particles=2)
    refused(eng, "num_samples = 0", ns=0)
    padded = _padded(obs_d)
    refused(eng, "observation strides", obs=padded)
    for env in ({"SLODE_ODE_ALG": "1"}, {"SLODE_ODE_PACK": "4"}, {"SLODE_FOLD_NEXT": "1"}):
        refused(_engine(c, monkeypatch, env), "measured arms")
        refused(_engine(c, monkeypatch, env), "measured arms", is_post=False)
    refused(_engine(c, monkeypatch, {"SLODE_NO_FOLD": "1"}), "SLODE_NO_FOLD")
    # tables beyond the LDS of one CU: T = 1024 with S = 8, C = 4, three heads (230 KB)
    from structured_latent_odes_amd import engine as E
    big = E.Engine(E.proc_spec(), 1024, DEV)
    big.set_times(torch.linspace(0.0, 1.0, 1024))
    big.profile_enable(True)
    with pytest.raises(L.SlodeError, match="LDS tables"):
        big.recon_moments(torch.zeros(big.n_params, device=DEV), big.make_batch(torch.zeros(2, 4, 1024, device=DEV), [torch.zeros(2, w, device=DEV) for w in WIDTHS["proc"]], None),
                          2, False, 2)
    assert big.rng_state()[2] == 0
    with pytest.raises(L.SlodeError, match="no profiled step"):
        big.profile_read()
    # the prior reads no observations: their strides do not matter
    eng = _engine(c, monkeypatch)
    flat = eng.pack(c["p"])
    mean, sd = _moments(eng, flat, c, False, obs_d=padded, labels=labels)
    RU.check(mean, sd, *RU.oracle_moments(c, False), "prior with padded observations")


@pytest.mark.parametrize("why", ["dopri5", "strided", "SLODE_ODE_ALG"])
def test_model_level_call_is_total_over_what_the_engine_refuses(why, monkeypatch):
    """dopri5, a padded observation tensor, a measured arm: the engine refuses, MechanisticBase.recon_moments composes the dict from
    recon_samples -- equal to that reduction made by hand from the same generator state (fp32 mean / population std).  dopri5: also
    against the fp64 oracle at the existing dopri5 eval bar (test_recon_samples_at_200_samples): error against the tight fp64 solve
    (rtol 1e-10) < 3 x that of the fp64 restatement at the engine's tolerances + 1e-5, and within 1e-3; for the mean and for the sd."""
    from oracle import slode_oracle as O
    from tests.eval_side_util import DP5_TOL, _heads64, _p64
    m, batch = _model("cvs", "dopri5" if why == "dopri5" else None, monkeypatch, {why: "1"} if why.startswith("SLODE") else None)
    eng = m._bind().engine
    if why == "strided":
        batch["observations"] = _padded(batch["observations"])
    names, ns = ("mu_50", "mu_75", "mu_25"), 6
    B, L = batch["observations"].shape[0], m.latent_dim
    eng.rng_seed(11)
    got = m.recon_moments(is_post=True, num_samples=ns, **batch)
    assert eng.rng_state()[2] == 1
    eng.rng_set_counter(0)
    res = m.recon_samples(is_post=True, num_samples=ns, **batch)
    for n in names:
        assert tuple(got[n][0].shape) == tuple(got[n][1].shape) == (B, 3, 86)
        assert torch.equal(got[n][0], res[n].mean(-1)) and torch.equal(got[n][1], res[n].std(-1, unbiased=False))
    if why != "dopri5":                                                           # four chunks of 5 rows: ONE drawing call, the same rows, the same bits
        monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 5 * ns)
        eng.rng_set_counter(0)
        chunked = m.recon_moments(is_post=True, num_samples=ns, **batch)
        assert eng.rng_state()[2] == 1
        assert all(torch.equal(chunked[n][0], got[n][0]) and torch.equal(chunked[n][1], got[n][1]) for n in names)
    eps = torch.randn(ns, B, L, generator=torch.Generator().manual_seed(2)).to(DEV)
    given = m.recon_moments(is_post=True, num_samples=ns, eps=eps, **batch)       # explicit noise on the composed route
    assert eng.rng_state()[2] == 1
    res = m.recon_samples(is_post=True, num_samples=ns, eps=eps, **batch)
    assert all(torch.equal(given[n][0], res[n].mean(-1)) for n in names)
    if why == "dopri5":
        p = _p64(m)
        ospec = O.cvs_spec(m.z_dims["iext"], m.z_dims["rtpr"], m.z_dims["epsilon"], solver="dopri5")
        nb = 4                                                                    # the first four trajectories: 24 fp64 solves
        z = res["z"][:, :nb].reshape(ns * nb, L).cpu().double()
        times = m.times.cpu().double()
        tight = _heads64(p, ospec, O.solve_ode(p, z, times, "dopri5", rtol=1e-10, atol=1e-12, per_trajectory=True))
        ref = _heads64(p, ospec, O.solve_ode(p, z, times, "dopri5", **DP5_TOL))
        for n in names:
            t = tight[n].reshape(ns, nb, 3, 86)
            r = ref[n].reshape(ns, nb, 3, 86)
            for i, f in enumerate((lambda v: v.mean(0), lambda v: v.std(0, unbiased=False))):
                scale = f(t).abs().clamp_min(1.0) if i == 0 else t.mean(0).abs().clamp_min(1.0)
                e_gpu = ((given[n][i][:nb].cpu().double() - f(t)).abs() / scale).max().item()
                e_ref = ((f(r) - f(t)).abs() / scale).max().item()
                print("dopri5 %s %s: error %.2e (fp64 restatement %.2e)" % (n, ("mean", "sd")[i], e_gpu, e_ref))
                assert e_gpu < 3.0 * e_ref + 1e-5 and e_gpu < 1e-3, (n, i, e_gpu, e_ref)


def test_launches_and_graph_capture():
    """Posterior: three launches, "weff", "enc_fwd2", "recon_moments", on one stream (a linear graph: no parallel branches); prior: one.
    One capture and one replay of a posterior call equal the stream-launched call bitwise."""
    c = RU.build("cvs_ald", "rk4", ns=7)
    eng = _engine(c)
    flat = eng.pack(c["p"])
    obs_d, labels = _device_batch(c)
    eps = c["eps"].to(DEV).contiguous()
    eng.profile_enable(True)
    _moments(eng, flat, c, True)
    assert [n for n, _ in eng.profile_read()] == ["weff", "enc_fwd2", "recon_moments"]
    _moments(eng, flat, c, False)
    assert [n for n, _ in eng.profile_read()] == ["recon_moments"]
    eng.profile_enable(False)
    Q = 3
    mean = torch.zeros(Q, c["B"], 3, c["T"], device=DEV)
    sd = torch.zeros_like(mean)
    bt = eng.make_batch(obs_d, labels, eps, particles=7)
    want = _captured(lambda: eng.recon_moments(flat, bt, c["B"], True, 7, mean, sd), (mean, sd))
    assert torch.equal(mean, want[0]) and torch.equal(sd, want[1])


def test_output_files(tmp_path):
    """save_recon_moments: <curve>_<post|prior>_sample_{mean,sd}.npy, [B, C, T] each, equal to recon_moments from the same generator
    state; save_recon_samples keeps writing the reference's names and shapes."""
    m, batch = _model("cvs")
    eng = m._bind().engine
    B = batch["observations"].shape[0]
    eng.rng_seed(8)
    files = m.save_recon_moments(str(tmp_path / "mom"), is_post=True, num_samples=5, **batch)
    files += m.save_recon_moments(str(tmp_path / "mom"), is_post=False, num_samples=5, **batch)
    want = sorted("%s_%s_sample_%s.npy" % (cv, p, k) for cv in ("mu_50", "mu_75", "mu_25") for p in ("post", "prior") for k in ("mean", "sd"))
    assert sorted(os.path.basename(f) for f in files) == want == sorted(os.listdir(str(tmp_path / "mom")))
    eng.rng_set_counter(0)
    res = m.recon_moments(is_post=True, num_samples=5, **batch)
    for f in files:
        a = np.load(f)
        assert a.shape == (B, 3, 86) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(np.load(str(tmp_path / "mom" / "mu_75_post_sample_sd.npy")), res["mu_75"][1].cpu().numpy())
    old = m.save_recon_samples(str(tmp_path / "smp"), is_post=True, num_samples=5, **batch)
    assert sorted(os.path.basename(f) for f in old) == ["mu_25_post_sample.npy", "mu_50_post_sample.npy", "mu_75_post_sample.npy"]
    assert np.load(old[0]).shape == (B, 3, 86, 5)


def test_training_entry_point_with_sample_moments(tmp_path, capsys):
    tr = importlib.import_module("training_cvs")
    cfg = EU.model_config("cvs")
    cfg.update(num_epochs=0, mini_batch_size=16, seq_len=86, num_samples=5)
    tr.train(cfg, batches_per_epoch=1, sample_moments=True, results_dir=str(tmp_path / "res"))
    assert "FINAL TEST:" in capsys.readouterr().out
    got = sorted(os.listdir(str(tmp_path / "res")))
    assert len(got) == 12 and "mu_50_post_sample_mean.npy" in got and "mu_50_prior_sample_sd.npy" in got
    assert np.load(str(tmp_path / "res" / "mu_50_post_sample_mean.npy")).shape == (16, 3, 86)
