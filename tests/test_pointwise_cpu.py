"""CPU tests of the pointwise predictive density: the C ABI of slode_pointwise_density / slode_pointwise_plan, the refusal ladder on a
hand-filled handle (tests/pointwise_refusals/pointwise_refusals.cpp), the fp64 fold of tests/pointwise_util.py against direct computations,
every condition the GPU tests ask shown to hold for the reference alone (the exclusion cap per configuration, the fp32 oracle inside the
bars, non-degenerate importance weights), and the Python layer on an engine double (the composed route, the files of
save_pointwise_density, the WAIC line)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import pointwise_util as PU
from tests import traj_bounds_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "num_draws", "weights", "mask", "loc", "scale", "point", "summary", "loss_kb",
        "workspace", "workspace_bytes", "stream"]


def test_abi_exports_pointwise_density_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_pointwise_density", "slode_pointwise_plan"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 230 and "0.2.3" in hdr
    for earlier in ("0.2.2: slode_posterior_refine", "0.2.1: slode_label_evidence", "0.1.6: slode_traj_bounds"):
        assert earlier in hdr                                                             # the earlier version lines are kept
    m = re.search(r"int\s+slode_pointwise_density\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_pointwise_density.argtypes
    assert len(at) == len(ARGS) and at[7] is C.c_int and at[8] is C.c_int and at[16] is C.c_size_t
    assert re.search(r"int\s+slode_pointwise_plan\s*\(\s*const slode_shape\*\s*s,\s*int num_draws,\s*int weights,\s*size_t\*\s*lds_bytes\s*\)\s*;", hdr)
    for name, val in (("SLODE_POINTWISE_SLOTS", 8), ("SLODE_PW_POSTERIOR", 0), ("SLODE_PW_IMPORTANCE", 1)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == val
    assert (L.POINTWISE_SLOTS, L.PW_POSTERIOR, L.PW_IMPORTANCE, L.POINTWISE_LDS_MAX) == (8, 0, 1, 160 * 1024)
    doc = hdr[:hdr.index("int slode_profile_read(")]
    assert '"pointwise_density"' in doc[doc.rindex("/*"):]                                # the launch name is documented at slode_profile_read
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_POINTWISE_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_pointwise_lds_bytes" in common
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "pointwise_kernel.hip" in srcs
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_pointwise_density(None, None, None, None, None, None, None, 0, 0, None, None, None, None, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_plan_is_host_arithmetic():
    """slode_pointwise_plan on the cvs shape (T = 200, C = 3, S = 5): posterior mode does not depend on K; importance mode adds 5 K
    floats (each table rounded up to 16 bytes); both refuse by name what cannot fit."""
    from structured_latent_odes_amd import _lib as L, engine as E

    class _E(E.Engine):
        def __init__(self, spec, T):
            self.spec, self.T, self._shapes = spec, T, {}
            self.lib = L.load()

    eng = _E(E.cvs_spec(3, 3, 2, solver="rk4"), 200)
    post = [eng.pointwise_plan(8, K, L.PW_POSTERIOR) for K in (1, 8, 200, 100000)]
    assert len(set(post)) == 1 and post[0] < 64 * 1024
    imp = [eng.pointwise_plan(8, K, L.PW_IMPORTANCE) for K in (4, 8, 200)]
    assert [v - post[0] for v in imp] == [4 * 5 * K for K in (4, 8, 200)]
    with pytest.raises(L.SlodeError, match="num_draws = 100000"):
        eng.pointwise_plan(8, 100000, L.PW_IMPORTANCE)
    with pytest.raises(L.SlodeError, match="weights = 2"):
        eng.pointwise_plan(8, 4, 2)
    with pytest.raises(L.SlodeError, match="num_draws = 0 < 1"):
        eng.pointwise_plan(8, 0, 0)


# case -> status and the words its message must carry, written from include/slode.h in rung order
_N = "slode_pointwise_density"
LADDER = [
    ("handle NULL", -1, ["handle is NULL"]), ("shape NULL", -1, ["shape is NULL"]), ("layout NULL", -1, ["layout is NULL"]),
    ("params NULL", -1, ["params is NULL"]), ("batch NULL", -1, [_N, "batch", "is NULL"]), ("times NULL", -1, [_N, "times", "is NULL"]),
    ("stage_t NULL", -1, [_N, "stage_t", "is NULL"]), ("workspace NULL", -1, [_N, "workspace", "is NULL"]), ("bad shape", -1, ["T out of range"]),
    ("draws 0", -1, [_N, "num_draws = 0 < 1"]), ("draws 2^30", -1, [_N, "B x num_draws", "2^30 - 1"]), ("posterior: draws 0", -1, [_N, "num_draws = 0 < 1"]),
    ("adaptive method 3", -1, [_N, "adaptive solver dopri5"]), ("adaptive method 4", -1, [_N, "adaptive solver bosh3"]),
    ("adaptive method 5", -1, [_N, "adaptive solver fehlberg2"]), ("adaptive method 6", -1, [_N, "adaptive solver adaptive_heun"]),
    ("particles 2", -1, [_N, "particles = 2"]), ("fold_on", -1, [_N, "measured arms"]), ("ode_pack", -1, [_N, "measured arms"]),
    ("ode_alg", -1, [_N, "measured arms"]), ("obs NULL", -1, [_N, "batch->obs is NULL"]), ("padded strides", -1, [_N, "observation strides (266, 1, 3)"]),
    ("channel-major strides of another T", -1, [_N, "observation strides (258, 87, 1)"]), ("no_fold", -1, [_N, "SLODE_NO_FOLD"]),
    ("weights 2", -1, [_N, "weights = 2", "SLODE_PW_POSTERIOR", "SLODE_PW_IMPORTANCE"]), ("weights -1", -1, [_N, "weights = -1"]),
    ("point NULL", -1, [_N, "point", "is NULL"]), ("summary NULL", -1, [_N, "summary", "is NULL"]),
    ("summary 4 bytes off", -1, [_N, "summary", "16-byte aligned"]), ("loc alone", -1, [_N, "loc and scale", "scale is NULL"]),
    ("scale alone", -1, [_N, "loc and scale", "loc is NULL"]), ("posterior: loss_kb", -1, [_N, "loss_kb", "importance mode alone"]),
    ("LDS: T 1000", -1, [_N, "LDS tables", "T = 1000", "num_draws = 2", "163840"]),
    ("posterior: LDS: T 1000", -1, [_N, "LDS tables", "T = 1000, S = 5, C = 3 (", "163840"]),       # posterior mode: the figure does not name the draws
    ("LDS: num_draws 100000", -1, [_N, "LDS tables", "num_draws = 100000"]), ("LDS: num_draws 2^24", -1, [_N, "LDS tables", "num_draws = 16777216"]),
    ("label columns 3, n_u 2", -1, ["label tensors have 3 columns"]), ("n_labels 5", -1, ["n_labels out of range"]),
    ("label tensor 1 NULL", -1, ["label tensor 1 is NULL"]), ("workspace too small", -3, ["workspace 64 B < required"]),
    ("posterior, mask NULL, loc and scale, num_draws 100000; workspace too small", -3, ["workspace 64 B < required"]),
    # two conditions at once: the earlier rung speaks
    ("params NULL + batch NULL", -1, ["params is NULL"]), ("times NULL + draws 0", -1, ["is NULL"]), ("draws 0 + adaptive", -1, ["num_draws = 0"]),
    ("adaptive + particles 2", -1, ["adaptive solver bosh3"]), ("ode_alg + obs NULL", -1, ["measured arms"]),
    ("no_fold + weights 2", -1, ["observation strides"]), ("weights 2 + point NULL", -1, ["weights = 2"]),
    ("summary NULL + loc alone", -1, ["point / summary"]), ("scale alone + posterior: loss_kb", -1, ["loc and scale"]),
    ("posterior: loss_kb + LDS", -1, ["loss_kb"]), ("LDS + label columns 3", -1, ["LDS tables"]),
    ("label columns 3 + workspace too small", -1, ["label tensors have 3 columns"]),
]


def test_pointwise_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_pointwise_density without a device, in rung order: status, the words of the message and the
    untouched drawing-call counter against LADDER; line by line against tests/golden/pointwise_refusals.txt; the shared rungs carry the
    texts tests/golden/eval_refusals.txt records for slode_traj_bounds, the call's name and its list of required pointers apart; and the
    memory that stands for the outputs untouched."""
    from tests.refusals_util import refusal_lines
    lines = refusal_lines("pointwise_refusals", tmp_path)
    assert lines[-1] == "memory that stands for the outputs | untouched"
    want = open(os.path.join(ROOT, "tests", "golden", "pointwise_refusals.txt")).read().splitlines()
    for i, (g, w) in enumerate(zip(lines, want)):
        assert g == w, "line %d:\n  got  %s\n  want %s" % (i + 1, g, w)
    assert len(lines) == len(want) == len(LADDER) + 1
    bounds = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "eval_refusals.txt")).read().splitlines():
        parts = line.split(" | ", 4)
        if len(parts) == 5 and parts[1] == "traj_bounds":
            bounds[parts[0]] = parts[4]
    shared = 0
    for line, (name, status, words) in zip(lines[:-1], LADDER):
        got_name, got_status, counter, msg = line.split(" | ", 3)
        assert got_name == name and int(got_status) == status and counter == "7", line      # refused, and nothing drawn
        for w in words:
            assert w in msg, (name, w, msg)
        if name in bounds and "LDS" not in name and "workspace too small" not in name:
            shared += 1
            assert msg == bounds[name].replace("slode_traj_bounds", _N).replace("batch / bounds / ", "batch / "), (name, msg, bounds[name])
    assert shared >= 22


# ---- the fp64 fold of tests/pointwise_util.py ------------------------------------------------------------------------------------------
def _toy(K=5, B=3, Cn=2, T=7, seed=0):
    g = np.random.default_rng(seed)
    return g.normal(-3.0, 2.0, size=(K, B, Cn, T)), g.normal(50.0, 1.5, size=(K, B))


def test_fold_against_direct_logsumexp_and_weighted_moments():
    ell, loss = _toy()
    for lw in (PU.log_weights(5, 3), PU.log_weights(5, 3, loss)):
        assert np.allclose(np.exp(lw).sum(0), 1.0, rtol=0, atol=1e-14)
        planes, slots = PU.fold64(ell, lw)
        a = torch.from_numpy(lw)[:, :, None, None] + torch.from_numpy(ell)
        w = torch.from_numpy(np.exp(lw))[:, :, None, None]
        mean = (w * torch.from_numpy(ell)).sum(0)
        assert np.allclose(planes[0], torch.logsumexp(a, 0).numpy(), rtol=1e-13, atol=1e-13)
        assert np.allclose(planes[1], mean.numpy(), rtol=1e-13, atol=1e-13)
        assert np.allclose(planes[2], (w * torch.from_numpy(ell) ** 2).sum(0).numpy() - mean.numpy() ** 2, rtol=1e-9, atol=1e-11)
        assert np.all(planes[0] >= planes[1]) and np.all(planes[2] >= 0)                  # Jensen
        assert np.allclose(slots[:, 0], planes[0].sum((1, 2))) and np.allclose(slots[:, 1], planes[2].sum((1, 2)))
        assert np.array_equal(slots[:, 3], np.full(3, 14.0)) and np.array_equal(slots[:, 4:7], np.zeros((3, 3)))
        assert np.allclose(slots[:, 7], TU.reduce64(-lw)[2])                              # the ESS of traj_bounds' reduction
    assert np.allclose(PU.fold64(ell, PU.log_weights(5, 3))[1][:, 7], 5.0)
    # a mask repartitions the sums and nothing else
    mask = np.ones((3, 2, 7)); mask[:, :, 4:] = 0.0; mask[1] = 0.0
    p2, s2 = PU.fold64(ell, lw, mask)
    assert np.array_equal(p2, planes) and np.array_equal(s2[:, 3], [8.0, 0.0, 8.0]) and np.array_equal(s2[:, 6], [6.0, 14.0, 6.0])
    assert np.allclose(s2[:, 0] + s2[:, 4], slots[:, 0]) and np.allclose(s2[:, 2] + s2[:, 5], slots[:, 2])


def test_fold_at_one_draw():
    ell, loss = _toy(K=1)
    for lw in (PU.log_weights(1, 3), PU.log_weights(1, 3, loss)):
        assert np.array_equal(lw, np.zeros((1, 3)))                                       # lw_0 is exactly 0 in both modes
        planes, slots = PU.fold64(ell, lw)
        assert np.array_equal(planes[0], ell[0]) and np.array_equal(planes[1], ell[0]) and np.array_equal(planes[2], np.zeros_like(ell[0]))
        assert np.array_equal(slots[:, 7], np.ones(3))


def test_importance_fold_is_the_self_normalised_estimator():
    """All-zero KL: loss_k = -sum_i ell_k[i], so w_k ~ prod_i p_k[i] and lppd[i] = log(sum_k p_k[i] prod_j p_k[j] / sum_k prod_j p_k[j])."""
    ell, _ = _toy(K=4, B=2, Cn=1, T=3)
    lw = PU.log_weights(4, 2, -ell.sum((2, 3)))
    planes, _ = PU.fold64(ell, lw)
    p = np.exp(ell)
    joint = p.prod((2, 3))                                                                # [K, B]
    want = np.log((p * joint[:, :, None, None]).sum(0) / joint.sum(0)[:, None, None])
    assert np.allclose(planes[0], want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss"])
def test_uniform_weights_sum_of_mean_ll_is_minus_the_mean_nll(case):
    """sum_i mean_ll[i] under w_k = 1 / K = -(mean over k of the negative log-likelihood of TU.oracle_rows): the point terms are the
    addends of the trajectory's log-likelihood, nothing else."""
    c = PU.build(case, "midpoint", B=3, K=3)
    want = PU.oracle_points(c)
    _, slots = PU.fold64(want["ell"], PU.log_weights(3, 3))
    nll = TU.oracle_rows(c)["nll"].mean(0)
    assert np.allclose(slots[:, 2], -nll, rtol=1e-12)
    # the masked loss of the importance mode: all-ones mask = the loss, zero mask = the KL-and-label part
    rows = TU.oracle_rows(c)
    assert np.allclose(PU.masked_loss(rows, want, np.ones(c["obs"].shape)), rows["loss"], rtol=1e-13)
    assert np.allclose(PU.masked_loss(rows, want, np.zeros(c["obs"].shape)), rows["loss"] - rows["nll"], rtol=1e-12)


# ---- every condition the GPU tests ask, on the reference alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", PU.CONFIGS, ids=["%s-%s-B%s-K%d-x%g" % c for c in PU.CONFIGS])
def test_exclusion_cap_and_clean_trajectories_per_gpu_configuration(cfg):
    """PU.conditions on the oracle alone: at most 0.1 % of the configuration's points excluded and at least half of its trajectories without
    an excluded point (K = 200: of its (draw, point) pairs; PU.conditions says why).  The Gauss likelihood has no jump: nothing to run."""
    if "gauss" in cfg[0]:
        return
    want = PU.oracle_points(PU.config(cfg))
    pts, share, clean = PU.excluded(want)
    print("%s: %d of %d (draw, point) pairs, %d of %d points (%.4f %%), %d of %d trajectories clean"
          % (cfg, int(want["excl"].sum()), want["excl"].size, int(pts.sum()), pts.size, 100 * share, int(clean.sum()), clean.size))
    PU.conditions(want, str(cfg))
    assert cfg[3] > PU.MANY_DRAWS or (share <= PU.CAP and clean.sum() * 2 >= clean.size)


@pytest.mark.parametrize("case", list(PU.EU.CASES))
def test_fp32_oracle_stays_inside_the_bars(case):
    """The oracle in fp32 against itself in fp64 at the case's own B, K = 4, rk4: every (draw, point) term outside the exclusion within
    bar_k[i]; the folded planes of both weightings within their bars (importance weights from the fp64 losses, as the GPU test takes the
    kernel's own)."""
    c = PU.build(case, "rk4", K=4)
    w64, w32 = PU.oracle_points(c), PU.oracle_points(c, dtype=torch.float32)
    r = np.where(w64["excl"], 0.0, np.abs(w32["ell"] - w64["ell"]) / w64["bar"])
    worst = [r.max()]
    pts = w64["excl"].any(0)
    for lw in (PU.log_weights(4, c["B"]), PU.log_weights(4, c["B"], TU.oracle_rows(c)["loss"])):
        p64, _ = PU.fold64(w64["ell"], lw)
        p32, _ = PU.fold64(w32["ell"], lw)
        pb, _ = PU.bars(w64["bar"], lw, p64)
        worst += [float(np.where(pts, 0.0, np.abs(p32[j] - p64[j]) / pb[j]).max()) for j in range(3)]
    print("%s: fp32 oracle, worst error / bar: terms %.3f; posterior lppd %.3f mean %.3f var %.3f; importance lppd %.3f mean %.3f var %.3f"
          % ((case,) + tuple(worst)))
    assert max(worst) <= 1.0


@pytest.mark.parametrize("cfg", PU.SPREAD, ids=[c[0] for c in PU.SPREAD])
def test_spread_configurations_have_non_degenerate_weights(cfg):
    """Noise x 1e-3, K = 8: 1.5 < ESS < 7.5 on at least 3 trajectories of the oracle's own losses (the importance fold is exercised with
    weights that neither collapse nor are uniform)."""
    ess = TU.reduce64(TU.oracle_rows(PU.config(cfg))["loss"])[2]
    assert np.sum((ess > 1.5) & (ess < 7.5)) >= 3, ess


# ---- the Python layer, on an engine double --------------------------------------------------------------------------------------------------
class _Eng:
    spec = type("S", (), {"latent_dim": 4, "labels_in_main": False})()

    def __init__(self, refuse):
        self.refuse, self.calls, self.draws = refuse, [], []

    def draw_normal(self, rows):
        self.draws.append(rows)
        return torch.arange(rows * 4, dtype=torch.float32).view(rows, 4) % 7 - 3.0

    def make_batch(self, obs, labels, eps=None, particles=1):
        return object()

    def pointwise_density(self, flat, bt, B, K, weights, mask=None, loc=None, scale=None, loss_kb=None):
        from structured_latent_odes_amd import _lib as L
        self.calls.append((B, K, weights, None if mask is None else tuple(mask.stride()), loc is not None, loss_kb))
        if self.refuse:
            err = L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        point = torch.arange(3 * B * 3 * 10, dtype=torch.float32).view(3, B, 3, 10)
        return point, torch.arange(B * 8, dtype=torch.float32).view(B, 8), None if loss_kb is False else torch.zeros(K, B)


def _double(gauss, refuse, aux=()):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        LABELS, GAUSS, AUX, FAMILY = ("iext",), gauss, aux, "cvs"

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse), "flat": torch.zeros(1)})()
            self.config = type("Cfg", (), {"quantile_diff": 0.3})()
            self.decoder = type("D", (), {"constant_std": torch.linspace(-1.0, 1.0, 30).view(3, 10)})()
            self.encoder = type("Enc", (), {"forward": staticmethod(lambda obs: (obs[:, 0, :4] * 0.1, 0.5 + obs[:, 1, :4] * 0.1))})()
            self.sample_calls = []

        def _bind(self):
            return self._b

        def _prior_loc_scale(self, labels):
            B = labels["iext"].shape[0]
            return torch.zeros(B, 4) + labels["iext"], torch.ones(B, 4)

        def recon_samples(self, observations, is_post, num_samples, eps=None, posterior=None, **labels):
            B = observations.shape[0]
            self.sample_calls.append((B, num_samples, posterior is not None))
            loc, scale = self.encoder.forward(observations) if posterior is None else posterior
            z = loc.unsqueeze(0) + scale.unsqueeze(0) * eps                                  # [K, B, 4]
            base = observations[:, :, :, None] + 0.2 * z[:, :, 0].t().reshape(B, 1, 1, num_samples) * torch.arange(1.0, 4.0).view(1, 3, 1, 1)
            names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
            shift = (0.0,) if gauss else (0.0, 0.12, -0.12)
            return dict({n: base + s for n, s in zip(names, shift)}, z=z)

    return M()


def test_fused_dict_and_arguments():
    m = _double(False, 0)
    obs = torch.rand(5, 10, 3).permute(0, 2, 1)                                           # the [B,C,T] view of a [B,T,C] tensor
    res = m.pointwise_density(obs, 4, iext=torch.zeros(5, 1))
    assert set(res) == {"lppd", "mean_ll", "p_waic", "elpd_waic"} | set(m.POINTWISE_NAMES)
    assert all(tuple(res[n].shape) == (5, 3, 10) for n in ("lppd", "mean_ll", "p_waic", "elpd_waic")) and all(tuple(res[n].shape) == (5,) for n in m.POINTWISE_NAMES)
    assert torch.equal(res["elpd_waic"], res["lppd"] - res["p_waic"])
    assert m._b.engine.calls == [(5, 4, 0, None, False, False)]
    mask = torch.zeros(5, 3, 10, dtype=torch.bool)
    res = m.pointwise_density(obs, 2, weights="importance", mask=mask, posterior=(torch.zeros(5, 4), torch.ones(5, 4)), return_draws=True, iext=torch.zeros(5, 1))
    assert m._b.engine.calls[-1] == (5, 2, 1, tuple(obs.stride()), True, None) and tuple(res["loss"].shape) == (2, 5)
    with pytest.raises(ValueError, match="weights must be"):
        m.pointwise_density(obs, 2, weights="prior", iext=torch.zeros(5, 1))
    with pytest.raises(ValueError, match="return_draws"):
        m.pointwise_density(obs, 2, return_draws=True, iext=torch.zeros(5, 1))
    with pytest.raises(ValueError, match="num_draws"):
        m.pointwise_density(obs, 0, iext=torch.zeros(5, 1))
    with pytest.raises(ValueError, match="posterior must be"):
        m.pointwise_density(obs, 2, posterior=(torch.zeros(5, 3), torch.ones(5, 3)), iext=torch.zeros(5, 1))


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.pointwise_density(torch.zeros(2, 3, 10), 5, iext=torch.zeros(2, 1))
    assert m.sample_calls == [] and m._b.engine.draws == []


@pytest.mark.parametrize("gauss", [False, True])
@pytest.mark.parametrize("weights", ["posterior", "importance"])
def test_composed_route_equals_the_fold_of_hand_made_terms(gauss, weights, monkeypatch):
    """A refusal: the dict is folded from recon_samples in chunks of rows; against PU.fold64 on point terms written out here, with a
    prefix mask and a given posterior; the chunking does not change the result."""
    g = torch.Generator().manual_seed(4)
    B, K = 7, 3
    obs = torch.rand(B, 3, 10, generator=g) + 1.0
    eps = torch.randn(K, B, 4, generator=g)
    lab = torch.rand(B, 1, generator=g)
    mask = torch.ones(B, 3, 10)
    mask[:, :, 6:] = 0.0
    post = (torch.randn(B, 4, generator=g) * 0.1, torch.rand(B, 4, generator=g) + 0.5)
    results = []
    for chunk_rows in (2 * K, 1 << 16):
        m = _double(gauss, refuse=-1)
        monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", chunk_rows)
        results.append(m.pointwise_density(obs, K, weights=weights, mask=mask, posterior=post, eps=eps, return_draws=weights == "importance", iext=lab))
        rows = max(1, chunk_rows // K)
        assert [c[0] for c in m.sample_calls] == [min(rows, B - lo) for lo in range(0, B, rows)] and all(c[2] for c in m.sample_calls)
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
    loss = None
    if weights == "importance":
        z = s["z"].double()
        log_q = torch.distributions.Normal(post[0].double(), post[1].double()).log_prob(z).sum(-1).numpy()
        log_p = torch.distributions.Normal(lab.double().expand(B, 4), torch.ones(B, 4).double()).log_prob(z).sum(-1).numpy()
        loss = -((mask.double().numpy()[None] * ell).sum((2, 3)) + log_p - log_q)
        assert np.allclose(res["loss"].numpy(), loss, rtol=1e-5)
    planes, slots = PU.fold64(ell, PU.log_weights(K, B, loss), mask.numpy())
    for j, n in enumerate(("lppd", "mean_ll", "p_waic")):
        assert np.allclose(res[n].numpy(), planes[j], rtol=1e-5, atol=1e-6), n
    for j, n in enumerate(m.POINTWISE_NAMES):
        assert np.allclose(res[n].numpy(), slots[:, j], rtol=1e-5, atol=1e-5), n
    assert res["n_in"].tolist() == [18.0] * B and res["n_out"].tolist() == [12.0] * B
    if weights == "posterior":
        assert res["ess"].tolist() == [float(K)] * B
    # no eps: ONE drawing call of K * B rows for the whole batch
    m = _double(gauss, refuse=-1)
    m.pointwise_density(obs, K, weights=weights, iext=lab)
    assert m._b.engine.draws == [K * B]


def test_importance_weights_of_a_family_that_scores_labels_are_refused_by_name():
    m = _double(False, refuse=-1, aux=(("q", "z", "iext", "sigmoid"),))
    m._b.engine.spec = type("S", (), {"latent_dim": 4, "labels_in_main": True})()
    with pytest.raises(ValueError, match="importance weights of the cvs family cannot be composed"):
        m.pointwise_density(torch.zeros(2, 3, 10), 3, weights="importance", eps=torch.zeros(3, 2, 4), iext=torch.zeros(2, 1))
    res = m.pointwise_density(torch.ones(2, 3, 10), 3, eps=torch.zeros(3, 2, 4), iext=torch.zeros(2, 1))   # posterior weights compose
    assert torch.isfinite(res["lppd"]).all() and float(res["p_waic"].abs().max()) < 1e-6


def test_save_pointwise_density_files_and_the_waic_line(tmp_path):
    m = _double(False, 0)
    obs = torch.rand(4, 3, 10)
    files = m.save_pointwise_density(str(tmp_path / "r"), [{"observations": obs, "iext": torch.zeros(4, 1)}, {"observations": obs[:2], "iext": torch.zeros(2, 1)}], 5)
    names = ["pointwise_lppd_post.npy", "pointwise_p_waic_post.npy", "pointwise_mean_ll_post.npy", "waic_post.npy"]
    assert [os.path.basename(f) for f in files] == names and sorted(os.listdir(str(tmp_path / "r"))) == sorted(names)
    arrays = [np.load(f) for f in files]
    assert [a.shape for a in arrays] == [(6, 3, 10)] * 3 + [(6, 8)] and all(a.dtype == np.float32 for a in arrays)
    with pytest.raises(ValueError, match="no batches"):
        m.save_pointwise_density(str(tmp_path / "e"), [], 5)
    table = np.zeros((3, 8)); table[:, 0] = [-10.0, -12.0, -17.0]; table[:, 1] = [1.0, 2.0, 3.0]
    p = np.zeros((3, 1, 4)); p[0, 0, 0] = 0.5
    line = m.waic_line(table, p, 5)
    elpd = np.array([-11.0, -14.0, -20.0])
    assert line == "waic: K=5  n=3  elpd_waic=%.4f  se=%.4f  p_waic=%.4f  share(p_waic>0.4)=%.4f" % (-45.0, np.sqrt(3 * elpd.var()), 6.0, 1 / 12)
