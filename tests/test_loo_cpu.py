"""CPU tests of PSIS leave-one-out: the C ABI of slode_pointwise_loo / slode_loo_plan, the plan rule restated in Python, the refusal ladder on
a hand-filled handle (tests/loo_refusals/loo_refusals.cpp), the numpy restatement of tests/loo_util.py against closed forms, and the Python
layer on an engine double (the fused dict, the composed route against the restatement, the files of save_pointwise_loo, the --loo line)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import loo_util as LU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "num_draws", "mask", "loc", "scale", "tile", "point", "summary", "tail_out",
        "workspace", "workspace_bytes", "stream"]


def test_abi_exports_pointwise_loo_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_pointwise_loo", "slode_loo_plan"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() == 290
    assert "0.2.9: slode_pointwise_loo, slode_loo_plan" in hdr
    for earlier in ("0.2.8: slode_joint_band", "0.2.3: slode_pointwise_density", "0.1.6: slode_traj_bounds"):
        assert earlier in hdr                                                             # the earlier version lines are kept
    m = re.search(r"int\s+slode_pointwise_loo\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_pointwise_loo.argtypes
    assert len(at) == len(ARGS) and at[7] is C.c_int and at[11] is C.c_int and at[16] is C.c_size_t
    assert re.search(r"int\s+slode_loo_plan\s*\(\s*const slode_shape\*\s*s,\s*int num_draws,\s*int tile,\s*int\*\s*tile_out,\s*int\*\s*sweeps,"
                     r"\s*int\*\s*depth,\s*size_t\*\s*lds_bytes\s*\)\s*;", hdr)
    assert int(re.search(r"#define\s+SLODE_LOO_SLOTS\s+(\d+)", hdr).group(1)) == 8 == L.LOO_SLOTS and L.LOO_LDS_MAX == 160 * 1024 == LU.LOO_LDS_MAX
    doc = hdr[:hdr.index("int slode_profile_read(")]
    assert '"pointwise_loo"' in doc[doc.rindex("/*"):]                                    # the launch name is documented at slode_profile_read
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_LOO_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_pointwise_loo_lds_bytes" in common
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "pointwise_loo_kernel.hip" in srcs
    assert lib.slode_pointwise_loo(None, None, None, None, None, None, None, 0, None, None, None, 0, None, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_tail_length_table():
    assert [LU.tail_len(K) for K in (1, 2, 20, 21, 64, 200, 1024)] == [0, 1, 4, 5, 13, 40, 96]
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase
    assert all(MechanisticBase.loo_tail_length(K) == LU.tail_len(K) for K in range(1, 1200))


def _engine(fam, T):
    from structured_latent_odes_amd import _lib as L, engine as E

    class _E(E.Engine):
        def __init__(self, spec, T):
            self.spec, self.T, self._shapes = spec, T, {}
            self.lib = L.load()

    spec = {"cvs": lambda: E.cvs_spec(3, 3, 2, solver="rk4"), "challenge": lambda: E.challenge_spec(solver="rk4", gauss=True),
            "proc": lambda: E.proc_spec(z_g=3, z_eps=2, solver="rk4", gauss=True)}[fam]()
    return _E(spec, T)


@pytest.mark.parametrize("fam,T", [("cvs", 200), ("challenge", 300), ("proc", 86)])
def test_plan_is_the_rule_restated(fam, T):
    """slode_loo_plan against tests/loo_util.plan (the tail length, the LDS carve, the fewest sweeps that fit) for K in {1, 2, 20, 21, 64,
    200, 1024} and tile in {0, 1, T}: the same figures, and a refusal exactly where the restatement has none."""
    from structured_latent_odes_amd import _lib as L
    eng = _engine(fam, T)
    s = eng.shape(4)
    Q = 1 if s.likelihood == L.GAUSS else 3
    seen_sweeps = set()
    for K in (1, 2, 20, 21, 64, 200, 1024):
        for tile in (0, 1, T):
            want = LU.plan(T, s.S, s.C, s.L, s.H, s.n_u, Q, K, tile)
            if want is None:
                with pytest.raises(L.SlodeError, match="num_draws = %d" % K):
                    eng.loo_plan(4, K, tile)
                continue
            got = eng.loo_plan(4, K, tile)
            assert got == want, (fam, K, tile, got, want)
            assert got[2] == LU.tail_len(K) + 1 and got[3] <= LU.LOO_LDS_MAX and got[1] == -(-T // got[0])
            if tile == 0 and got[1] > 1:                                                  # the fewest sweeps: one fewer does not fit
                assert LU.lds_bytes(T, s.S, s.C, s.L, s.H, s.n_u, Q, got[2], -(-T // (got[1] - 1))) > LU.LOO_LDS_MAX
            seen_sweeps.add(got[1])
    assert len(seen_sweeps) > 1                                                           # K = 1024 needs more than one sweep at these T
    for tile, match in ((-1, "tile = -1"), (T + 1, "tile = %d" % (T + 1))):
        with pytest.raises(L.SlodeError, match=match):
            eng.loo_plan(4, 8, tile)
    with pytest.raises(L.SlodeError, match="num_draws = 0 < 1"):
        eng.loo_plan(4, 0, 0)


def test_loo_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_pointwise_loo and slode_loo_plan without a device: line by line against
    tests/golden/loo_refusals.txt; refused (status -1, or -3 for the workspace) with the counter untouched; the rungs shared with
    slode_pointwise_density carry its texts (tests/golden/pointwise_refusals.txt), the call's name apart; outputs untouched."""
    from tests.refusals_util import refusal_lines
    lines = refusal_lines("loo_refusals", tmp_path)
    assert lines[-1] == "memory that stands for the outputs | untouched"
    want = open(os.path.join(ROOT, "tests", "golden", "loo_refusals.txt")).read().splitlines()
    for i, (g, w) in enumerate(zip(lines, want)):
        assert g == w, "line %d:\n  got  %s\n  want %s" % (i + 1, g, w)
    assert len(lines) == len(want) >= 55
    density = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "pointwise_refusals.txt")).read().splitlines()[:-1]:
        name, _, _, msg = line.split(" | ", 3)
        density[name] = msg
    shared = 0
    for line in lines[:-1]:
        name, which, status, counter, msg = line.split(" | ", 4)
        assert int(status) == (-3 if "workspace too small" in name and "+" not in name else -1) and counter == "7" and msg, line
        assert ("slode_loo_plan" in msg) == (which == "plan") or "slode_" not in msg, line
        if which == "loo" and name in density and "LDS" not in name and "workspace too small" not in name:
            shared += 1
            assert msg == density[name].replace("slode_pointwise_density", "slode_pointwise_loo"), (name, msg)
    assert shared >= 28
    by = {(l.split(" | ")[0], l.split(" | ")[1]): l.split(" | ", 4)[4] for l in lines[:-1]}
    assert "num_draws = 33554432" in by[("num_draws 2^25", "loo")] and "num_draws = 33554432" in by[("num_draws 2^25", "plan")]
    assert "tile = 86 does not fit" in by[("tile T does not fit at num_draws 4000", "loo")] and "num_draws = 4000" in by[("tile T does not fit at num_draws 4000", "plan")]


# ---- the numpy restatement against closed forms ---------------------------------------------------------------------------------------------
def test_all_draws_equal_and_one_draw():
    for K in (1, 4, 20, 21, 64, 200):
        e, k, n = LU.psis_point(np.full(K, -3.25))
        assert abs(e + 3.25) < 1e-14 and k == np.inf and n == 0                           # every draw ties with the cutoff: no tail
    e, k, n = LU.psis_point(np.array([-7.5]))
    assert e == -7.5 == LU.lppd(np.array([[-7.5]]))[0] and k == np.inf


def test_elpd_loo_is_at_most_lppd_and_small_k_is_plain_importance_sampling():
    g = np.random.default_rng(5)
    for K in (4, 20, 21, 64, 200):
        l = g.normal(-2.0, 1.5, size=(K, 40))
        e, k = LU.psis(l)
        assert np.all(e <= LU.lppd(l) + 1e-12 * (1 + np.abs(e)))
        if K <= 20:                                                                       # M < 5: no smoothing; the harmonic-mean estimate
            assert np.all(np.isinf(k))
            assert np.allclose(e, -np.log(np.exp(-l).mean(0)), rtol=1e-12, atol=1e-12)
        else:
            assert np.all(np.isfinite(k))


def test_ties_with_the_cutoff_shorten_the_tail():
    l = np.sort(np.random.default_rng(2).normal(size=64))
    l[10:14] = l[13]                                                                      # ranks 10 .. 12 tie with rank M = 13
    e, k, n = LU.psis_point(l)
    assert n == 10 and np.isfinite(k)
    l[3:14] = l[13]
    assert LU.psis_point(l)[1:] == (np.inf, 3)


@pytest.mark.parametrize("k_true", [0.2, 0.7])
def test_fit_recovers_the_shape_of_an_exact_pareto_tail(k_true):
    """Tails drawn from an exact generalised Pareto distribution, n = 1000: the estimator's spread measured over 200 seeds; every estimate
    within 4 sd of the prior-shrunk truth (n k + 5) / (n + 10), and their mean within 4 standard errors of it plus the estimator's known
    O(1 / n) bias."""
    n = 1000
    est = np.array([LU.gpd_fit(LU.gpd_sample(k_true, 1.0, n, np.random.default_rng(seed)))[0] for seed in range(200)])
    target = (n * k_true + 5.0) / (n + 10.0)
    sd = est.std()
    assert 0.5 * (1 + k_true) / math.sqrt(n) < sd < 2.0 * (1 + k_true) / math.sqrt(n)   # the asymptotic sd of the shape estimate is (1 + k) / sqrt n
    assert np.all(np.abs(est - target) <= 4.0 * sd), np.abs(est - target).max() / sd
    assert abs(est.mean() - target) <= 4.0 * sd / math.sqrt(200) + 5.0 / n


def _harmonic(l):
    """The plain importance-sampling estimate -log mean_k exp(-l_k), shifted by the smallest l."""
    l = np.asarray(l, np.float64)
    return l.min() - math.log(np.exp(-(l - l.min())).mean())


def test_a_tail_that_spans_300_decades_is_left_unsmoothed():
    """x = [9.09e-309, 4.44e-304, 2.14e-293, 2.99e-264, 1.0] (a challenge_gauss point under the `fitted` regime): x_[n/4] is denormal,
    1 / (3 x) overflows and b* is 0 / 0.  gpd_fit returns a non-finite pair and raises nothing; psis_point follows the kernel's rule --
    isfinite(khat) && isfinite(sigma), otherwise unsmoothed with khat = +inf -- so elpd_loo is the plain importance-sampling estimate."""
    x = np.array([9.09e-309, 4.44e-304, 2.14e-293, 2.99e-264, 1.0])
    kh, sigma = LU.gpd_fit(x)
    assert not (np.isfinite(kh) and np.isfinite(sigma))
    tiny = np.finfo(np.float64).tiny
    K = 21                                                                                # M = 5: the shortest tail that is fitted at all
    a = np.concatenate([[0.0], np.log(x[:4] + tiny)[::-1], np.linspace(-800.0, -5000.0, K - 5)])   # rank order; ranks 5 .. under the clamp
    assert np.all(np.diff(a) < 0) and a[5] < LU.LOG_DBL_MIN < a[4]
    l = -3.0 - a
    tail = (np.exp(a[:5]) - tiny)[::-1]
    assert np.allclose(tail[:4], x[:4], rtol=1e-2) and tail[4] == 1.0                     # the quoted tail, to its three digits
    for order in (np.arange(K), np.random.default_rng(1).permutation(K)):
        e, k, n = LU.psis_point(l[order])
        assert n == 5 and k == np.inf
        assert abs(e - _harmonic(l)) <= 1e-12 * abs(e)


def test_the_clamp_decides_the_tail_where_the_ratios_span_more_than_708_nat():
    """K = 64 (M = 13): a generalised Pareto tail whose log-ratios are rescaled to span 1100 nat.  The cutoff a_M lies under log DBL_MIN, so
    cut = log DBL_MIN and n = #{a > log DBL_MIN} < M; the fit runs on exp(a) - DBL_MIN of those ranks alone; draws under the clamp can move
    further down without changing n, khat or elpd_loo (exp(a) of such a draw is below one fp64 ulp of the largest ratio)."""
    K, M = 64, 13
    g = np.random.default_rng(9)
    r = np.log1p(LU.gpd_sample(0.7, 1.0, K, g))                                           # ascending log-ratios, rank 0 last
    a = (r - r[-1])[::-1]                                                                 # rank order: a_0 = 0 >= a_1 >= ...
    a = a * (1100.0 / -a[M])
    n_want = int((a[:M] > LU.LOG_DBL_MIN).sum())
    assert a[M] < LU.LOG_DBL_MIN and 5 <= n_want < M
    l = 2.5 - a
    e, k, n = LU.psis_point(l[g.permutation(K)])
    assert n == n_want and np.isfinite(k) and np.isfinite(e)
    kh, _ = LU.gpd_fit((np.exp(a[:n]) - np.finfo(np.float64).tiny)[::-1])
    assert k == kh
    assert e <= LU.lppd(l[:, None])[0] + 1e-12 * abs(e)
    lower = l.copy()
    lower[n:] += np.linspace(50.0, 5000.0, K - n)                                         # every draw under the clamp, further down
    e2, k2, n2 = LU.psis_point(lower)
    assert (n2, k2) == (n, k) and abs(e2 - e) <= 1e-13 * abs(e)


# ---- the Python layer, on an engine double --------------------------------------------------------------------------------------------------
class _Eng:
    spec = type("S", (), {"latent_dim": 4, "labels_in_main": False})()

    def __init__(self, refuse, sweeps=1):
        self.refuse, self.sweeps, self.calls, self.draws, self.counter = refuse, sweeps, [], [], 11

    def draw_normal(self, rows):
        self.draws.append(rows)
        self.counter += 1
        return torch.randn(rows, 4, generator=torch.Generator().manual_seed(rows))

    def rng_state(self):
        return (3, 0, self.counter)

    def rng_set_counter(self, n):
        self.counter = n

    def make_batch(self, obs, labels, eps=None, particles=1):
        return object()

    def loo_plan(self, B, K, tile=0):
        return (tile or 10, self.sweeps, LU.tail_len(K) + 1, 1024)

    def pointwise_loo(self, flat, bt, B, K, mask=None, loc=None, scale=None, tile=0, tail=None):
        from structured_latent_odes_amd import _lib as L
        self.calls.append((B, K, None if mask is None else tuple(mask.stride()), loc is not None, tile, tail))
        if self.refuse:
            err = L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        point = torch.arange(3 * B * 3 * 10, dtype=torch.float32).view(3, B, 3, 10)
        return point, torch.arange(B * 8, dtype=torch.float32).view(B, 8), torch.zeros(LU.tail_len(K) + 1, B, 3, 10) if tail else None


def _double(gauss, refuse, sweeps=1):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        LABELS, GAUSS, AUX, FAMILY = ("iext",), gauss, (), "cvs"

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, sweeps), "flat": torch.zeros(1)})()
            self.config = type("Cfg", (), {"quantile_diff": 0.3})()
            self.decoder = type("D", (), {"constant_std": torch.linspace(-1.0, 1.0, 30).view(3, 10)})()
            self.encoder = type("Enc", (), {"forward": staticmethod(lambda obs: (obs[:, 0, :4] * 0.1, 0.5 + obs[:, 1, :4] * 0.1))})()
            self.times = torch.arange(10.0)
            self.sample_calls = []

        def _bind(self):
            return self._b

        def recon_samples(self, observations, is_post, num_samples, eps=None, posterior=None, **labels):
            B = observations.shape[0]
            self.sample_calls.append((B, num_samples, posterior is not None))
            loc, scale = self.encoder.forward(observations) if posterior is None else posterior
            z = loc.unsqueeze(0) + scale.unsqueeze(0) * eps                                  # [K, B, 4]
            base = observations[:, :, :, None] + 0.6 * z[:, :, 0].t().reshape(B, 1, 1, num_samples) * torch.arange(1.0, 4.0).view(1, 3, 1, 1) \
                + 0.3 * z[:, :, 1].t().reshape(B, 1, 1, num_samples) * torch.arange(10.0).view(1, 1, 10, 1)
            names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
            shift = (0.0,) if gauss else (0.0, 0.12, -0.12)
            return dict({n: base + s for n, s in zip(names, shift)}, z=z)

    return M()


def test_fused_dict_and_arguments():
    m = _double(False, 0)
    obs = torch.rand(5, 10, 3).permute(0, 2, 1)                                           # the [B,C,T] view of a [B,T,C] tensor
    res = m.pointwise_loo(obs, 24, iext=torch.zeros(5, 1))
    planes = {"elpd_loo", "khat", "lppd", "p_loo"}
    assert set(res) == planes | set(m.LOO_NAMES) and m.LOO_NAMES == ("elpd_loo_in", "lppd_in", "n_in", "n_bad_in", "khat_max_in", "elpd_loo_out", "lppd_out", "n_out")
    assert all(tuple(res[n].shape) == (5, 3, 10) for n in planes) and all(tuple(res[n].shape) == (5,) for n in m.LOO_NAMES)
    assert torch.equal(res["p_loo"], res["lppd"] - res["elpd_loo"])
    assert m._b.engine.calls == [(5, 24, None, False, 0, None)]
    mask = torch.zeros(5, 3, 10, dtype=torch.bool)
    res = m.pointwise_loo(obs, 21, mask=mask, posterior=(torch.zeros(5, 4), torch.ones(5, 4)), tile=7, return_tail=True, iext=torch.zeros(5, 1))
    assert m._b.engine.calls[-1] == (5, 21, tuple(obs.stride()), True, 7, True) and tuple(res["tail"].shape) == (6, 5, 3, 10)
    for bad, match in ((dict(num_draws=0), "num_draws"), (dict(num_draws=4, tile=11), "tile must lie"), (dict(num_draws=4, tile=-1), "tile must lie"),
                       (dict(num_draws=4, posterior=(torch.zeros(5, 3), torch.ones(5, 3))), "posterior must be")):
        with pytest.raises(ValueError, match=match):
            m.pointwise_loo(obs, iext=torch.zeros(5, 1), **bad)


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.pointwise_loo(torch.zeros(2, 3, 10), 5, iext=torch.zeros(2, 1))
    assert m.sample_calls == [] and m._b.engine.draws == []


def test_more_sweeps_than_max_sweeps_compose_without_an_engine_call():
    m = _double(True, 0, sweeps=3)
    res = m.pointwise_loo(torch.rand(2, 3, 10), 8, eps=torch.randn(8, 2, 4), iext=torch.zeros(2, 1))
    assert m._b.engine.calls == [] and len(m.sample_calls) == 1 and torch.isfinite(res["elpd_loo"]).all()
    m.pointwise_loo(torch.rand(2, 3, 10), 8, eps=torch.randn(8, 2, 4), max_sweeps=3, iext=torch.zeros(2, 1))
    assert len(m._b.engine.calls) == 1


@pytest.mark.parametrize("gauss", [False, True])
@pytest.mark.parametrize("K", [1, 20, 21, 64])
def test_composed_route_equals_the_restatement_on_hand_made_terms(gauss, K, monkeypatch):
    """A refusal: the dict comes from recon_samples in chunks of rows; against tests/loo_util.psis on point terms written out here, with
    a prefix mask and a given posterior; the chunking changes nothing; the counter ends at n + K."""
    g = torch.Generator().manual_seed(4)
    B = 5
    obs = torch.rand(B, 3, 10, generator=g) + 1.0
    eps = torch.randn(K, B, 4, generator=g)
    lab = torch.rand(B, 1, generator=g)
    mask = torch.ones(B, 3, 10)
    mask[:, :, 6:] = 0.0
    post = (torch.randn(B, 4, generator=g) * 0.1, torch.rand(B, 4, generator=g) + 0.5)
    results = []
    for chunk_rows, fit_elements in ((2 * K, 1 << 24), (1 << 16, 4096)):
        m = _double(gauss, refuse=-1)
        monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", chunk_rows)
        monkeypatch.setattr(type(m), "LOO_FIT_ELEMENTS", fit_elements)
        results.append(m.pointwise_loo(obs, K, mask=mask, posterior=post, eps=eps, return_tail=True, iext=lab))
        rows = max(1, chunk_rows // K)
        assert [c[0] for c in m.sample_calls] == [min(rows, B - lo) for lo in range(0, B, rows)] and all(c[2] for c in m.sample_calls)
        assert m._b.engine.counter == 11 and m._b.engine.draws == []                      # eps given: the generator is not used
    for n in results[0]:
        assert torch.allclose(results[0][n], results[1][n], rtol=1e-6, atol=1e-6), n
    res = results[0]
    s = m.recon_samples(obs, True, K, eps=eps, posterior=post, iext=lab)
    sd = torch.nn.functional.softplus(m.decoder.constant_std).double().numpy()[None, :, :, None]
    y = obs.double().numpy()[..., None]
    if gauss:
        ell = -np.log(sd) - 0.5 * np.log(2 * np.pi) - 0.5 * ((y - s["mean"].double().numpy()) / sd) ** 2
    else:
        ell = 0.0
        for name, tau in (("mu_50", 0.5), ("mu_75", 0.8), ("mu_25", 0.2)):
            mu = s[name].double().numpy()
            ell = ell + np.where(y >= mu, tau, 1 - tau) * (-np.log(2 * sd) - np.abs(y - mu) / sd)
    ell = np.moveaxis(ell, -1, 0)                                                         # [K, B, C, T]
    elpd, khat = LU.psis(ell)
    M = LU.tail_len(K)
    assert np.allclose(res["elpd_loo"].numpy(), elpd, rtol=2e-6, atol=2e-6)
    assert np.array_equal(np.isinf(res["khat"].numpy()), np.isinf(khat)) and np.all(np.isinf(khat)) == (K <= 20)
    fin = np.isfinite(khat)
    assert np.allclose(res["khat"].numpy()[fin], khat[fin], rtol=1e-5, atol=1e-5)
    assert np.allclose(res["lppd"].numpy(), LU.lppd(ell), rtol=2e-6, atol=2e-6)
    assert np.array_equal(res["tail"].numpy(), np.sort(ell, 0)[:M + 1].astype(np.float32))
    assert torch.equal(res["p_loo"], res["lppd"] - res["elpd_loo"])
    inn = mask.numpy() > 0
    e32, l32, k32 = (res[n].double().numpy() for n in ("elpd_loo", "lppd", "khat"))
    assert np.allclose(res["elpd_loo_in"].numpy(), (e32 * inn).sum((1, 2)), rtol=1e-6) and np.allclose(res["elpd_loo_out"].numpy(), (e32 * ~inn).sum((1, 2)), rtol=1e-6)
    assert np.allclose(res["lppd_in"].numpy(), (l32 * inn).sum((1, 2)), rtol=1e-6) and np.allclose(res["lppd_out"].numpy(), (l32 * ~inn).sum((1, 2)), rtol=1e-6)
    assert res["n_in"].tolist() == [18.0] * B and res["n_out"].tolist() == [12.0] * B
    assert np.array_equal(res["n_bad_in"].numpy(), ((k32 > 0.7) & inn).sum((1, 2)).astype(np.float32))
    assert np.array_equal(res["khat_max_in"].numpy(), np.where(inn, k32, -np.inf).max((1, 2)).astype(np.float32))
    # no eps: ONE drawing call of K * B rows for the whole batch, and the counter where the engine call leaves it
    m = _double(gauss, refuse=-1)
    m.pointwise_loo(obs, K, iext=lab)
    assert m._b.engine.draws == [K * B] and m._b.engine.counter == 11 + K


def test_save_pointwise_loo_files_and_the_loo_line(tmp_path):
    m = _double(False, 0)
    obs = torch.rand(4, 3, 10)
    files = m.save_pointwise_loo(str(tmp_path / "r"), [{"observations": obs, "iext": torch.zeros(4, 1)}, {"observations": obs[:2], "iext": torch.zeros(2, 1)}], 24)
    names = ["pointwise_elpd_loo_post.npy", "pointwise_khat_post.npy", "loo_post.npy"]
    assert [os.path.basename(f) for f in files] == names and sorted(os.listdir(str(tmp_path / "r"))) == sorted(names)
    arrays = [np.load(f) for f in files]
    assert [a.shape for a in arrays] == [(6, 3, 10)] * 2 + [(6, 8)] and all(a.dtype == np.float32 for a in arrays)
    with pytest.raises(ValueError, match="no batches"):
        m.save_pointwise_loo(str(tmp_path / "e"), [], 5)
    table = np.zeros((3, 8)); table[:, 0] = [-11.0, -14.0, -20.0]; table[:, 1] = [-10.0, -12.0, -17.0]
    k = np.zeros((3, 1, 4)); k[0, 0, 0] = 0.6; k[1, 0, 1] = np.inf
    line = m.loo_line(table, k, 24)
    assert line == "loo: K=24  n=3  elpd_loo=%.4f  se=%.4f  p_loo=%.4f  share(khat>0.7)=%.4f  share(khat>0.5)=%.4f" % (
        -45.0, np.sqrt(3 * table[:, 0].var()), 6.0, 1 / 12, 2 / 12)


def test_loo_flag_is_off_by_default_on_the_three_entry_points():
    from structured_latent_odes_amd import training
    ap = training.build_parser()
    assert ap.parse_args([]).loo == 0 and ap.parse_args(["--loo", "64"]).loo == 64
    import inspect
    assert inspect.signature(training.train).parameters["loo"].default == 0
