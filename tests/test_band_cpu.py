"""CPU tests of the simultaneous bands: the C ABI of slode_joint_band / slode_joint_band_plan / slode_joint_band_levels, the plan against a
hand count of the kernel's tables (every case; the smallest draw count it refuses at T = 200 and at T = 1024), the level rule with hand
values, the refusal ladder on a hand-filled handle (tests/band_refusals/band_refusals.cpp), the numpy restatement, the conditions the GPU
tests rest on shown for the fp64 oracle alone, and the Python layer on an engine double (the dict, the composed route on the oracle's draws,
the files, the flags)."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import band_util as BU
from tests import draws_ladder_util as DL
from tests import eval_stats_util as EU
from tests import lds_util as LU
from tests import recon_moments_util as RU
from tests import summary_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "is_post", "num_samples", "n_levels", "levels", "sd_floor", "mean", "sd", "crit",
        "joint", "obs_dev", "dev_out", "workspace", "workspace_bytes", "stream"]
BUDGET = 160 * 1024


def test_abi_exports_joint_band_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_joint_band", "slode_joint_band_plan", "slode_joint_band_levels"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 280 and "0.2.8: slode_joint_band" in hdr
    for earlier in ("0.2.7: slode_mechanism_moments", "0.2.6: slode_recon_quantiles", "0.2.5: slode_curve_summary", "0.2.4: slode_latent_attribution",
                    "0.2.3: slode_pointwise_density", "0.2.2: slode_posterior_refine", "0.1.5: slode_recon_moments", "0.1.1: slode_svi_step"):
        assert earlier in hdr                                                             # the earlier version lines are kept
    m = re.search(r"int\s+slode_joint_band\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_joint_band.argtypes
    assert len(at) == len(ARGS) and at[7] is C.c_int and at[8] is C.c_int and at[9] is C.c_int and at[11] is C.c_float and at[19] is C.c_size_t
    assert re.search(r"int\s+slode_joint_band_plan\s*\(\s*const slode_shape\*\s*s,\s*int num_samples,\s*size_t\*\s*lds_bytes\s*\)\s*;", hdr)
    assert int(re.search(r"#define\s+SLODE_JOINT_BAND_MAX_LEVELS\s+(\d+)", hdr).group(1)) == L.JOINT_BAND_MAX_LEVELS == 8
    doc = hdr[hdr.index("credible bands as ONE call"):m.start()]
    for word in ("NULL handle", "num_samples < 2", "adaptive solver", "particles > 1", "SLODE_NO_FOLD", "SLODE_ODE_ALG", "LDS tables", "SLODE_EINVAL",
                 "sd_floor", "(0, 1]", "mean / sd / crit NULL", "n_levels", "sqrt(K - 1)", "ceil(p_j K - 1e-9)", "Phi^-1((1 + p_j) / 2)", '"weff"',
                 '"enc_fwd2"', '"joint_band"', "no atomics", "[Q,B,C,n_levels]", "[Q,B,C,2]", "[Q,B,C,num_samples]", "slode_joint_band_plan",
                 "first_trajectory", "capturable", "same noise", "slode_recon_moments"):
        assert word in doc, word
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_JOINT_BAND_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_joint_band_lds_bytes" in common
    assert L.JOINT_BAND_LDS_MAX == BUDGET
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "joint_band_kernel.hip" in srcs
    assert "slode_joint_band" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert '"calibration_merge", "joint_band", ...' in hdr                                  # appended to the names slode_profile_read documents
    assert '"recon_quantiles", "mechanism_moments", "intervene_moments"' in hdr              # ... and nothing inserted inside them
    # host-side refusals need no device: a NULL handle is refused before anything else
    lv = (C.c_double * 1)(0.95)
    assert lib.slode_joint_band(None, None, None, None, None, None, None, 1, 8, 1, lv, 0.0, None, None, None, None, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_engine_and_model_signatures():
    from structured_latent_odes_amd.engine import Engine
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase
    assert list(inspect.signature(Engine.joint_band).parameters) == ["self", "params", "batch", "B", "is_post", "num_samples", "levels", "sd_floor",
                                                                    "mean", "sd", "crit", "joint", "obs_dev", "dev"]
    assert inspect.signature(Engine.joint_band).parameters["dev"].default is None
    assert list(inspect.signature(Engine.joint_band_plan).parameters) == ["self", "B", "num_samples"]
    sig = inspect.signature(MechanisticBase.simultaneous_band).parameters
    assert list(sig)[:8] == ["self", "observations", "is_post", "num_samples", "levels", "sd_floor", "eps", "return_draws"]
    assert sig["levels"].default == (0.95,) and sig["sd_floor"].default == 0.0 and sig["eps"].default is None and sig["return_draws"].default is False
    sig = inspect.signature(MechanisticBase.save_simultaneous_band).parameters
    assert list(sig) == ["self", "results_dir", "batches", "is_post", "num_samples", "levels"] and sig["levels"].default == (0.95,)
    assert "sqrt(K - 1)" in MechanisticBase.simultaneous_band.__doc__ and "K = 20" in MechanisticBase.simultaneous_band.__doc__


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def _hand_count(eng, K):
    sp = eng.spec
    return BU.plan_bytes(eng.T, sp.ode_state_dim, sp.n_channels, sp.latent_dim, sp.ode_hidden_dim, sp.n_u, sp.gauss, K)


@pytest.mark.parametrize("case", list(EU.CASES))
def test_plan_against_a_hand_count_of_the_tables(case):
    """Every case: the plan is the hand count (BU.plan_bytes); one more draw costs 4 Q C bytes up to the rounding of the table to 16 B; B
    does not enter."""
    eng = LU.host_engine(case)
    QC = (1 if eng.spec.gauss else 3) * eng.spec.n_channels
    got = {K: eng.joint_band_plan(8, K) for K in (2, 4, 7, 8, 33, 200)}
    for K, b in got.items():
        assert b == _hand_count(eng, K) <= BUDGET, (case, K)
    assert got[8] - got[4] == 4 * QC * 4 and got[200] - got[8] == 4 * QC * 192                # multiples of four draws: no rounding
    assert eng.joint_band_plan(1, 33) == eng.joint_band_plan(1024, 33)                       # one workgroup per trajectory


@pytest.mark.parametrize("T", [200, 1024])
def test_smallest_draw_count_the_plan_refuses(T):
    """cvs (S = 5, C = 3, three heads) at T = 200 and T = 1024: the smallest K whose hand count exceeds the budget is refused by name with
    that figure, one fewer is taken, and a refusal still writes the bytes."""
    from structured_latent_odes_amd import _lib as L
    eng = LU.host_engine("cvs_ald", T=T)
    K = 2
    while _hand_count(eng, K) <= BUDGET:
        K += 1
    print("T = %d: the plan takes K <= %d (%d B) and refuses K = %d (%d B)" % (T, K - 1, _hand_count(eng, K - 1), K, _hand_count(eng, K)))
    # by hand: the other tables take 33600 B at T = 200 and 155552 B at T = 1024 (2 r4(5 (T - 1)) + 3 r4(9 T) floats grow with T), the
    # deviations 4 r4(9 K): 33600 + 4 r4(9 x 3617) = 163824 fits, 3618 gives 163856; 155552 + 4 r4(9 x 230) = 163840 fits exactly, 231 does not
    assert _hand_count(eng, 0) == {200: 33600, 1024: 155552}[T] and K == {200: 3618, 1024: 231}[T]
    assert eng.joint_band_plan(8, K - 1) == _hand_count(eng, K - 1) <= BUDGET
    with pytest.raises(L.SlodeError, match=r"T = %d, S = 5, C = 3, num_samples = %d \(%d B.*exceed the budget of 163840 B" % (T, K, _hand_count(eng, K))):
        eng.joint_band_plan(8, K)
    lib, r = L.load(), C.c_size_t(0)
    assert lib.slode_joint_band_plan(C.byref(eng.shape(8)), K, C.byref(r)) == -1 and r.value == _hand_count(eng, K)
    with pytest.raises(L.SlodeError, match="num_samples = 1 < 2"):
        eng.joint_band_plan(8, 1)


# ---- the level rule -------------------------------------------------------------------------------------------------------------------------
def test_rank_rule_and_z_with_hand_values():
    """r = min(K, max(1, ceil(level K - 1e-9))) and z = Phi^-1((1 + level) / 2): the library's, the model layer's and BU's restatement agree
    at K in {2, 7, 20, 200} x levels {0.5, 0.9, 0.95, 1.0}; hand values; the fp32 half-widths the kernel compares with are the same bits."""
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase
    eng = LU.host_engine("cvs_ald")
    levels = (0.5, 0.9, 0.95, 1.0)
    hand = {2: [1, 2, 2, 2], 7: [4, 7, 7, 7], 20: [10, 18, 19, 20], 200: [100, 180, 190, 200]}
    z_hand = [0.6744897501960817, 1.6448536269514722, 1.959963984540054, math.inf]
    for K, want in hand.items():
        ranks, z = eng.joint_band_levels(K, levels)
        r2, z2 = BU.level_rule(levels, K)
        r3, z3 = zip(*MechanisticBase._band_levels(levels, K))
        assert ranks == want == r2 == list(r3), K
        for a, b, c, h in zip(z, z2, z3, z_hand):
            assert (a == b == c == h) if math.isinf(h) else (abs(a - h) <= 1e-14 * h and b == c and abs(b - h) <= 1e-14 * h), (K, a, b, h)
            assert np.float32(a) == np.float32(b)
    # 0.7 x 10 = 7.000000000000001 in double: the 1e-9 keeps the rank at 7; a level below 1 / K still selects the minimum
    assert eng.joint_band_levels(10, (0.7, 0.05, 0.3))[0] == [7, 1, 3] == BU.level_rule((0.7, 0.05, 0.3), 10)[0]
    # (towards level 1 the result is as well conditioned as 1 - level is known: both forms lose digits there, each in its own way)
    for p in (0.001, 0.3, 0.8, 0.99, 0.999):
        a, b = eng.joint_band_levels(5, (p,))[1][0], BU.level_rule((p,), 5)[1][0]
        assert abs(a - b) <= 1e-12 * b and np.float32(a) == np.float32(b), (p, a, b)


# ---- the refusal ladder ---------------------------------------------------------------------------------------------------------------------
_N = "slode_joint_band"
NAMED = {                       # the reasons the issue lists, by the case that shows them: the words of the message
    "handle NULL": ["handle is NULL"], "num_samples 1": [_N, "num_samples = 1 < 2", "the sd of one draw is 0"], "n_levels 0": [_N, "n_levels = 0 out of range [1, 8]"],
    "n_levels 9": [_N, "n_levels = 9"], "level 0": [_N, "levels[1] = 0 is not in (0, 1]"], "level 1.5": [_N, "levels[0] = 1.5"], "level NaN": [_N, "nan"],
    "sd_floor -1": [_N, "sd_floor = -1 is negative or not finite"], "sd_floor NaN": [_N, "sd_floor = nan"], "sd_floor inf": [_N, "sd_floor = inf"],
    "mean NULL": [_N, "mean / sd / crit is NULL"], "sd NULL": [_N, "mean / sd / crit is NULL"], "crit NULL": [_N, "mean / sd / crit is NULL"],
    "adaptive method 3": [_N, "adaptive solver dopri5", "reduce recon_samples instead"], "adaptive method 6": [_N, "adaptive solver adaptive_heun"],
    "padded strides": [_N, "observation strides (266, 1, 3)"], "particles 2": [_N, "particles = 2"], "no_fold": [_N, "SLODE_NO_FOLD"],
    "fold_on": [_N, "measured arms"], "ode_pack": [_N, "measured arms"], "ode_alg": [_N, "measured arms"],
    "LDS: T 1024, 400 draws": [_N, "T = 1024, S = 5, C = 3, num_samples = 400 (169952 B", "exceed the budget of 163840 B"],
    "LDS: T 86, 4100 draws": [_N, "num_samples = 4100 (164352 B"],
}


def test_band_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_joint_band (posterior and prior), of its plan and of its level rule without a device, in rung
    order, line by line against tests/golden/band_refusals.txt; every refusal of the call is SLODE_EINVAL (or SLODE_ENOSPC for the
    workspace) with the generator's counter untouched; the reasons the issue names carry their words; the rungs shared with
    slode_recon_moments carry its texts, the name and the pointer list apart; the LDS figures are the hand count's; the memory that stands
    for the outputs is untouched."""
    lines = DL.golden_lines("band_refusals", tmp_path)
    assert len(lines) >= 120
    recon = DL.recon_texts(_N)
    seen, shared = set(), 0
    for line in lines[:-1]:
        name, col, status, counter, msg = line.split(" | ", 4)
        if col in ("plan", "levels"):
            assert int(status) == -1 and (int(counter) == 0 or "LDS" in name), line
            continue
        assert int(status) == (-3 if msg.startswith("workspace ") else -1) and counter == "7", line          # refused, and nothing drawn
        for w in NAMED.get(name, []):
            assert w in msg, (name, w, msg)
        seen.add(name)
        key = name.replace("num_samples", "draws")
        if key in recon and "LDS" not in name and "workspace too small" not in name and "NULL" not in name.replace("handle NULL", "") \
                and name not in ("num_samples 0", "num_samples 1") and not (col == "prior" and "strides" in name):
            shared += 1
            assert msg == recon[key], (name, msg, recon[key])
    assert set(NAMED) <= seen
    big, small = LU.host_engine("cvs_ald", T=1024), LU.host_engine("cvs_ald", T=86)
    sp = small.spec
    assert _hand_count(big, 400) == 169952
    assert BU.plan_bytes(86, 5, 3, 8, 25, 2, False, 4100) == 164352                       # the shape of tests/refusals_common.h
    print("%d lines, %d of them word for word slode_recon_moments' texts (cvs latent dim %d)" % (len(lines), shared, sp.latent_dim))
    assert shared >= 25


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------------
def test_restatement_on_hand_values():
    """Two roundings per point, a floor that excludes, -1 never selected, the rank rule on ties, counts at equality."""
    v = RU._f32([[[1.0, 2.0, 7.0]], [[3.0, 2.5, 7.0]], [[2.0, 0.0, 7.0]]])                 # [K = 3, 1, T = 3]
    m, s = RU._f32([[2.0, 1.5, 7.0]]), RU._f32([[0.5, 3.0, 0.0]])
    dev, pts = BU.dev_f32(v, m, s)
    assert pts.tolist() == [2] and dev.dtype == np.float32
    assert dev[:, 0].tolist() == [2.0, 2.0, 0.5]                                             # |1 - 2| / 0.5; |3 - 2| / 0.5; 1.5 / 3: s = 0 takes no part
    third = BU.dev_f32(RU._f32([[[1.0]]]), RU._f32([[0.0]]), RU._f32([[3.0]]))[0]
    assert third[0, 0] == np.float32(1.0) / np.float32(3.0)
    dev2, pts2 = BU.dev_f32(v, m, s, floor=0.5)                                              # s = 0.5 is not above the floor
    assert pts2.tolist() == [1] and np.allclose(dev2[:, 0], [1.0 / 6.0, 1.0 / 3.0, 0.5])
    none, pts0 = BU.dev_f32(v, m, s, floor=5.0)
    assert pts0.tolist() == [0] and np.all(none == 0.0)
    crit, joint = BU.crit_joint(dev, (1.0, 0.3, 0.5, 0.95))                                  # ranks 3, 1, 2, 3 of (0.5, 2, 2)
    assert crit[0].tolist() == [2.0, 0.5, 2.0, 2.0]
    assert joint[0].tolist() == [1.0, 0.0, float(np.float32(1.0) / np.float32(3.0)), float(np.float32(1.0) / np.float32(3.0))]
    # the deviation of any draw from the sample mean is at most sqrt(K - 1) sample sds: attained by one outlier among equal draws
    for K in (2, 7, 20):
        w = np.zeros((K, 1, 1)); w[0] = 1.0
        o = BU.oracle_dev(w)
        assert o["dev"].max() == pytest.approx(math.sqrt(K - 1), rel=1e-12)


# ---- the conditions the GPU tests rest on, for the oracle alone -------------------------------------------------------------------------------
GPU_CASES = ("cvs_ald", "proc_gauss", "challenge_gauss", "proc_ald")


def test_oracle_conditions_of_the_gpu_cases():
    """What the GPU tests rest on, shown on the fp64 oracle alone for the cases they use (B = 13, K = 7 and 33, both sides).  The smallest
    sd is above 5e-3: sd_floor = 0 excludes nothing.  The deviations span 0.04 .. 4.9 (at most sqrt(K - 1)) and the worst bar is 0.12 in
    that unit (cvs_ald, prior, K = 7: an sd of 5e-3 under a curve of size 1.4).  A bar that wide puts 0.5 .. 5 % of the draws within their bar
    of an informative z (printed: it cannot stay under NEAR_SHARE = 1e-3 there, whatever the case), so the GPU test asserts the share at
    BU.CLEAR_LEVEL, whose z clears sqrt(K - 1) by more than the worst bar -- no draw is near, every count must be K -- and applies the
    rule that only near draws may differ at the informative levels too."""
    lo, hi, worst, smallest, near, clear = np.inf, 0.0, 0.0, np.inf, {}, 0.0
    for case in GPU_CASES:
        for ns in (7, 33):
            c = RU.build(case, "rk4", B=13, ns=ns)
            for is_post in (True, False):
                v = SU.oracle_draws(c, is_post)
                for q in range(v.shape[0]):
                    o = BU.oracle_dev(v[q])
                    bar = BU.dev_bar(o)
                    lo, hi, worst, smallest = min(lo, o["dev"].min()), max(hi, o["dev"].max()), max(worst, bar.max()), min(smallest, o["sd"].min())
                    assert o["dev"].max() <= math.sqrt(ns - 1) * (1 + 1e-12)
                    for p, z in zip(BU.COUNT_LEVELS, BU.level_rule(BU.COUNT_LEVELS, ns)[1]):
                        near[p] = max(near.get(p, 0.0), float((np.abs(o["dev"] - z) <= bar).mean()))
                    clear = max(clear, float((np.abs(o["dev"] - BU.level_rule((BU.CLEAR_LEVEL[ns],), ns)[1][0]) <= bar).mean()))
    print("oracle: smallest sd %.3e, deviations %.3f .. %.3f, worst bar %.3e, largest near share per level %s, at the clear level %.1e"
          % (smallest, lo, hi, worst, {p: round(s, 4) for p, s in near.items()}, clear))
    assert smallest >= 5e-3 and 0.04 <= lo and hi <= 4.9 and worst <= 0.12
    assert clear == 0.0 <= BU.NEAR_SHARE
    for ns in (7, 33):
        assert BU.level_rule((BU.CLEAR_LEVEL[ns],), ns)[1][0] > math.sqrt(ns - 1) + 0.12


# ---- the Python layer on an engine double ---------------------------------------------------------------------------------------------
class _Eng:
    """mean = q + 0.01 b + 0.001 c (constant in t), sd = 2, crit = 10 + level index + 0.01 b, joint = 0.5, obs_dev = 10.5 + 0.01 b | points T,
    dev = k: a value names its curve, trajectory, channel, level and draw."""
    Q, Cn, T = 3, 3, 6

    def __init__(self, refuse=0):
        from structured_latent_odes_amd import _lib as L
        self.L, self.refuse = L, refuse
        self.calls, self.batches, self.draws, self.counter = [], [], [], 9

    def draw_normal(self, rows):
        self.draws.append(rows)
        self.counter += 1
        return torch.linspace(-1.0, 1.0, rows * 4).view(rows, 4)

    def make_batch(self, obs, labels, eps=None, particles=1, eps_shape=None):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles))
        return object()

    def rng_state(self):
        return (0, 0, self.counter)

    def rng_set_counter(self, n):
        self.counter = n

    def joint_band(self, flat, bt, B, is_post, num_samples, levels, sd_floor=0.0, mean=None, sd=None, crit=None, joint=None, obs_dev=None, dev=None):
        self.calls.append((bool(is_post), num_samples, tuple(levels), sd_floor, dev))
        if self.refuse:
            err = self.L.SlodeError("libslode call failed (%d)" % self.refuse)
            err.status = self.refuse
            raise err
        self.counter += 1
        Q, Cn, T, Lv = self.Q, self.Cn, self.T, len(levels)
        b = 0.01 * torch.arange(B, dtype=torch.float32)
        mean = (torch.arange(Q, dtype=torch.float32).view(Q, 1, 1, 1) + b.view(1, B, 1, 1) + 0.001 * torch.arange(Cn, dtype=torch.float32).view(1, 1, Cn, 1)
                + torch.zeros(Q, B, Cn, T))
        crit = 10.0 + torch.arange(Lv, dtype=torch.float32).view(1, 1, 1, Lv) + b.view(1, B, 1, 1) + torch.zeros(Q, B, Cn, Lv)
        odev = torch.stack([10.5 + b.view(1, B, 1) + torch.zeros(Q, B, Cn), torch.full((Q, B, Cn), float(T))], -1)
        d = None if dev is None else torch.arange(num_samples, dtype=torch.float32).view(1, 1, 1, -1) + torch.zeros(Q, B, Cn, num_samples)
        return mean, torch.full_like(mean, 2.0), crit, torch.full_like(crit, 0.5), odev, d


def _double(refuse=0, draws=None):
    """A model whose engine is ``_Eng`` and whose ``recon_samples`` returns the rows of ``draws`` ({curve: [B, C, T, ns]}) named by the label
    ``iext`` (the row index): what the composed route reduces."""
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        FAMILY, GAUSS = "cvs", False
        LABELS = ("iext", "rtpr")

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse), "flat": torch.zeros(1)})()
            self.times = torch.arange(6.0)
            self.sampled = []

        def _bind(self):
            return self._b

        def recon_samples(self, observations, is_post, num_samples, eps=None, posterior=None, **labels):
            rows = labels["iext"].reshape(-1).long()
            self.sampled.append((len(rows), tuple(eps.shape)))
            return dict({n: v[rows] for n, v in draws.items()}, z=eps)

    return M()


def _labels(B):
    return dict(iext=torch.arange(float(B)).view(B, 1), rtpr=torch.ones(B, 1))


def test_model_level_call_uses_the_engine_once():
    m = _double()
    eng = m._b.engine
    B = 7
    res = m.simultaneous_band(torch.zeros(B, 3, 6), True, 5, **_labels(B))
    assert eng.calls == [(True, 5, (0.95,), 0.0, None)] and eng.batches == [((B, 3, 6), 2, None, 5)] and eng.draws == [] and eng.counter == 10
    assert set(res) == {"levels", "mu_50", "mu_75", "mu_25"} and res["levels"].dtype == torch.float64 and res["levels"].tolist() == [0.95]
    keys = {"mean", "sd", "crit", "lower", "upper", "pointwise_joint", "obs_dev", "obs_inside", "points"}
    for q, n in enumerate(("mu_50", "mu_75", "mu_25")):
        r = res[n]
        assert set(r) == keys
        assert tuple(r["mean"].shape) == tuple(r["sd"].shape) == (B, 3, 6) and tuple(r["crit"].shape) == tuple(r["pointwise_joint"].shape) == (1, B, 3)
        assert tuple(r["lower"].shape) == tuple(r["upper"].shape) == (1, B, 3, 6) and tuple(r["obs_dev"].shape) == tuple(r["points"].shape) == (B, 3)
        assert r["obs_inside"].dtype == torch.bool and tuple(r["obs_inside"].shape) == (1, B, 3)
        assert float(r["mean"][3, 1, 0]) == pytest.approx(q + 0.031) and float(r["crit"][0, 3, 1]) == pytest.approx(10.03)
        assert torch.equal(r["lower"], r["mean"].unsqueeze(0) - r["crit"].unsqueeze(-1) * r["sd"].unsqueeze(0))
        assert torch.equal(r["upper"], r["mean"].unsqueeze(0) + r["crit"].unsqueeze(-1) * r["sd"].unsqueeze(0))
        assert float(r["upper"][0, 3, 1, 2]) == pytest.approx(q + 0.031 + 2 * 10.03)
        assert not bool(r["obs_inside"].any()) and float(r["points"][0, 0]) == 6.0           # 10.5 + 0.01 b > 10 + 0.01 b
    many = m.simultaneous_band(torch.zeros(B, 3, 6), False, 5, levels=torch.tensor([0.5, 1.0, 0.9], dtype=torch.float64), sd_floor=0.25, eps=torch.zeros(5, B, 4),
                               return_draws=True, **_labels(B))
    assert eng.calls[-1] == (False, 5, (0.5, 1.0, 0.9), 0.25, True) and eng.batches[-1] == ((B, 3, 6), 2, (5, B, 4), 5)
    r = many["mu_75"]
    assert tuple(r["crit"].shape) == (3, B, 3) and tuple(r["dev"].shape) == (5, B, 3) and float(r["dev"][4, 0, 0]) == 4.0
    assert r["obs_inside"][:, 0, 0].tolist() == [False, True, True]                          # 10.5 against 10, 11, 12
    for bad, exc in (((), "levels"), ((0.0,), "levels"), ((1.5,), "levels"), (tuple([0.5] * 9), "levels")):
        with pytest.raises(ValueError, match=exc):
            m.simultaneous_band(torch.zeros(B, 3, 6), True, 5, levels=bad, **_labels(B))
    with pytest.raises(ValueError, match="num_samples"):
        m.simultaneous_band(torch.zeros(B, 3, 6), True, 1, **_labels(B))
    for floor in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sd_floor"):
            m.simultaneous_band(torch.zeros(B, 3, 6), True, 5, sd_floor=floor, **_labels(B))
    assert len(eng.calls) == 2


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
def test_composed_route_against_numpy_on_the_oracle_draws(is_post, monkeypatch):
    """The engine refuses (status -1): one drawing call for the whole batch (the counter at n + 1, as the engine call leaves it),
    recon_samples in chunks, and the dict equals a plain numpy restatement in fp64 of the same draws -- the fp64 oracle's (SU.oracle_draws)
    rounded to fp32.  torch's fp32 mean / std of K = 7 values carry at most K 2^-24 relative error, under a tenth of RU's bars: mean, sd and
    the deviations are held to a tenth of BU.dev_bar, crit to the largest such bar of its curve, and a count may differ only by the draws
    within that bar of z; a floor between the sds excludes the same points."""
    c = RU.build("cvs_ald", "rk4", B=13, ns=7)
    v = RU._f32(SU.oracle_draws(c, is_post))                                                 # [Q, ns, B, C, T]
    names = ("mu_50", "mu_75", "mu_25")
    draws = {n: torch.from_numpy(np.ascontiguousarray(np.moveaxis(v[q], 0, -1))) for q, n in enumerate(names)}      # [B, C, T, ns]
    y = c["obs"].float()
    levels = (0.9, 0.5, 1.0, 0.1)
    gap_floor, ratio = BU.floor_in_gap(v.astype(np.float64).std(1), 0.1, 0.9)              # inside the middle of the sds: it excludes some points
    assert ratio >= 1.0 + 1e-3                                                              # no sd at the floor: the same points on both sides
    for floor in (0.0, gap_floor):
        m = _double(refuse=-1, draws=draws)
        monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 7 * 5)                            # 5 rows per chunk: 5 + 5 + 3
        eng = m._b.engine
        res = m.simultaneous_band(y, is_post, 7, levels=levels, sd_floor=floor, return_draws=True, **_labels(13))
        assert len(eng.calls) == 1 and eng.draws == [91] and eng.counter == 10 and [r for r, _ in m.sampled] == [5, 5, 3]
        ranks, z = BU.level_rule(levels, 7)
        for q, n in enumerate(names):
            o = BU.oracle_dev(v[q].astype(np.float64), y.double().numpy(), floor)
            on = o["sd"] > floor
            assert floor == 0.0 or 0 < on.sum() < on.size
            bar = 0.1 * BU.dev_bar(o, on)                                                    # [ns, B, C]
            r = {k: t.double().numpy() for k, t in res[n].items()}
            scale = np.maximum(1.0, np.abs(o["mean"]))
            assert np.all(np.abs(r["mean"] - o["mean"]) <= 0.1 * RU.MEAN_BAR * scale) and np.all(np.abs(r["sd"] - o["sd"]) <= 0.1 * RU.SD_BAR * scale)
            assert np.array_equal(r["points"], o["points"]) and np.all(np.abs(r["dev"] - o["dev"]) <= bar + 1e-12)
            obar = 0.1 * np.where(on, (2 * RU.MEAN_BAR * scale + o["obs_dev"][..., None] * RU.SD_BAR * scale) / o["sd"], 0.0).max(-1)
            assert np.all(np.abs(r["obs_dev"] - o["obs_dev"]) <= obar + 1e-12)
            srt = np.sort(o["dev"], 0)
            for j, (rk, zj) in enumerate(zip(ranks, z)):
                assert np.all(np.abs(r["crit"][j] - srt[rk - 1]) <= bar.max(0) + 1e-12), (n, j)
                want = (o["dev"] <= zj).sum(0)
                assert np.all(np.abs(np.rint(r["pointwise_joint"][j] * 7) - want) <= (np.abs(o["dev"] - zj) <= bar).sum(0)), (n, j)
            assert np.array_equal(res[n]["obs_inside"].numpy(), res[n]["obs_dev"].unsqueeze(0).numpy() <= res[n]["crit"].numpy())
            assert np.array_equal(r["crit"][2], r["dev"].max(0)) and np.array_equal(r["crit"][3], r["dev"].min(0))      # level 1: the maximum; r = 1: the minimum
        given = m.simultaneous_band(y, is_post, 7, levels=levels, sd_floor=floor, return_draws=True, eps=torch.zeros(7, 13, 4), **_labels(13))
        assert eng.draws == [91] and eng.counter == 10                                       # explicit noise draws nothing
        assert all(torch.equal(given[n][k], res[n][k]) for n in names for k in res[n])


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(refuse=status, draws={})
    with pytest.raises(L.SlodeError):
        m.simultaneous_band(torch.zeros(7, 3, 6), True, 5, **_labels(7))
    assert m.sampled == [] and m._b.engine.draws == []


def test_save_simultaneous_band_files_and_line(tmp_path):
    m = _double()
    batches = [dict(observations=torch.zeros(B, 3, 6), **_labels(B)) for B in (2, 3)]
    files = m.save_simultaneous_band(str(tmp_path / "r"), batches, False, 4, levels=(0.5, 0.95))
    names = ("mu_50", "mu_75", "mu_25")
    want = ["%s_prior_band_%s.npy" % (n, k) for n in names for k in ("mean", "sd", "crit", "pointwise_joint", "obs_dev")] + ["band_levels.npy"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "r"))) == sorted(want)
    arrays = {os.path.basename(f): np.load(f) for f in files}
    assert arrays["band_levels.npy"].tolist() == [0.5, 0.95] and arrays["band_levels.npy"].dtype == np.float64
    for q, n in enumerate(names):
        mean, sd = arrays["%s_prior_band_mean.npy" % n], arrays["%s_prior_band_sd.npy" % n]
        crit, joint, odev = (arrays["%s_prior_band_%s.npy" % (n, k)] for k in ("crit", "pointwise_joint", "obs_dev"))
        assert mean.shape == sd.shape == (5, 3, 6) and crit.shape == joint.shape == (5, 2, 3) and odev.shape == (5, 3)      # the trajectories in loader order
        assert all(a.dtype == np.float32 for a in (mean, sd, crit, joint, odev))
        assert mean[2, 0, 0] == np.float32(q) and mean[4, 1, 0] == pytest.approx(q + 0.021, abs=1e-6) and crit[3, 1, 0] == pytest.approx(11.01)
    line = m.band_line(arrays["mu_50_prior_band_crit.npy"], arrays["mu_50_prior_band_pointwise_joint.npy"], arrays["mu_50_prior_band_obs_dev.npy"],
                       arrays["band_levels.npy"], "prior")
    assert line.startswith("joint_band_prior: n=5  levels=[0.5, 0.95]  0.5: crit=10.008 (z=0.674) pointwise_joint=0.500 obs_inside=0.000  "
                           "0.95: crit=11.008 (z=1.960) pointwise_joint=0.500 obs_inside=1.000"), line


def test_training_entry_points_take_the_flags():
    from structured_latent_odes_amd import training as TR
    sig = inspect.signature(TR.train).parameters
    assert sig["joint_band"].default == 0 and tuple(sig["band_levels"].default) == (0.95,)
    a = TR.build_parser().parse_args(["--joint-band", "64", "--band-levels", "0.5,0.9,1"])
    assert a.joint_band == 64 and a.band_levels == [0.5, 0.9, 1.0]
    d = TR.build_parser().parse_args([])
    assert d.joint_band == 0 and d.band_levels == [0.95]
    src = inspect.getsource(TR.main)
    assert 'kw["joint_band"], kw["band_levels"] = a.joint_band, a.band_levels' in src
    assert "save_simultaneous_band" in inspect.getsource(TR.train) and "band_line" in inspect.getsource(TR.train)
