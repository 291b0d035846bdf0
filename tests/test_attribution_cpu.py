"""CPU tests of the latent attribution: the C ABI of slode_latent_attribution / slode_attribution_plan, the plan against a hand count of the
kernel's tables, the refusal ladder on a hand-filled handle (tests/attribution_refusals/attribution_refusals.cpp), the fp32 restatement of
the kernel's accumulation against fp64, every condition the GPU tests ask shown to hold for the fp64 oracle alone (the all-blocks arm
reproduces the variance, the two-block identity, the msd bar discriminates), and the Python layer on an engine double (arm lists, the split
over calls, the composed route, the files of save_latent_attribution)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import attribution_util as AU
from tests import draws_ladder_util as DL
from tests import eval_stats_util as EU
from tests import lds_util as LU
from tests import recon_moments_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "is_post", "num_samples", "arm_masks", "n_arms", "mean", "sd", "msd", "workspace",
        "workspace_bytes", "stream"]


def test_abi_exports_latent_attribution_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_latent_attribution", "slode_attribution_plan"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 240 and "0.2.4" in hdr
    for earlier in ("0.2.3: slode_pointwise_density", "0.2.2: slode_posterior_refine", "0.1.7: slode_intervene_moments"):
        assert earlier in hdr                                                             # the earlier version lines are kept
    m = re.search(r"int\s+slode_latent_attribution\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_latent_attribution.argtypes
    assert len(at) == len(ARGS) and at[7] is C.c_int and at[8] is C.c_int and at[10] is C.c_int and at[15] is C.c_size_t
    assert re.search(r"int\s+slode_attribution_plan\s*\(\s*const slode_shape\*\s*s,\s*int n_arms,\s*size_t\*\s*lds_bytes\s*\)\s*;", hdr)
    assert int(re.search(r"#define\s+SLODE_ATTRIBUTION_MAX_ARMS\s+(\d+)", hdr).group(1)) == L.ATTRIBUTION_MAX_ARMS == 16
    doc = hdr[hdr.index("latent attribution as ONE call"):m.start()]
    for word in ("NULL handle", "num_samples < 1", "adaptive solver", "dopri5", "particles > 1", "SLODE_NO_FOLD", "SLODE_ODE_ALG", "LDS tables",
                 "SLODE_EINVAL", "n + 2", "n + 1", "POPULATION", "Jansen", "TOTAL-EFFECT", "FIRST-ORDER", "arm_masks[a] == 0", "REST", "HOST array",
                 "[2, num_samples, B, L]", '"latent_attribution"', "SLODE_ATTRIBUTION_MAX_ARMS", "slode_attribution_plan"):
        assert word in doc, word
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_ATTRIBUTION_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_attribution_lds_bytes" in common
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "attribution_kernel.hip" in srcs
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_latent_attribution(None, None, None, None, None, None, None, 1, 8, None, 1, None, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_engine_signature():
    import inspect
    from structured_latent_odes_amd.engine import Engine
    assert list(inspect.signature(Engine.latent_attribution).parameters)[:7] == ["self", "params", "batch", "B", "is_post", "num_samples", "arm_masks"]
    assert list(inspect.signature(Engine.attribution_plan).parameters) == ["self", "B", "n_arms"]
    assert "eps_shape" in inspect.signature(Engine.make_batch).parameters


@pytest.mark.parametrize("case", list(EU.CASES))
def test_plan_against_a_hand_count_of_the_tables(case):
    """slode_attribution_plan for the six model shapes: the shared forward pieces (step table 2 (T - 1) S, one row of 2 + 2 S floats rounded
    up to four per hidden unit, the transposed first layers L x 2 H, their biases 2 H, the init net's output layer H S + S, the head
    weights Q C S, the dynamics biases 2 S, z, the labels, the init net's hidden layer, x0), then base moments 3 Q C T, base values Q C T, arm
    sums A Q C T and loc | scale; every piece rounded up to 16 bytes.  One more arm costs exactly Q C T floats."""
    from structured_latent_odes_amd import _lib as L
    eng = LU.host_engine(case)
    sp, T = eng.spec, eng.T
    Ld, Cn, Q = sp.latent_dim, sp.n_channels, 1 if sp.gauss else 3
    shared = LU.spec_shared_floats(sp, T)
    for A in (1, 2, 6, 16):
        want = 4 * (shared + LU.r4(3 * Q * Cn * T) + LU.r4(Q * Cn * T) + LU.r4(A * Q * Cn * T) + 2 * LU.r4(Ld))
        if want <= 160 * 1024:
            assert eng.attribution_plan(8, A) == want, (case, A)
        else:
            with pytest.raises(L.SlodeError, match="n_arms = %d \\(%d B\\)" % (A, want)):
                eng.attribution_plan(8, A)
    for bad in (0, -1, 17):
        with pytest.raises(L.SlodeError, match="n_arms = %d out of range \\[1, 16\\]" % bad):
            eng.attribution_plan(8, bad)
    assert eng.attribution_blocks() == len(sp.prior_groups) + 1


# case -> call column, status and the words its message must carry, written from include/slode.h in rung order
_N = "slode_latent_attribution"
_BOTH, _POST, _PRIOR, _PLAN = ("post", "prior"), ("post",), ("prior",), ("plan",)
_HEAD, _LABELS, _TWO = DL.shared_rungs(_N, "batch / times / stage_t / workspace", "reduce the attribution samples instead")
LADDER = _HEAD + [
    ("n_arms 0", _BOTH, -1, [_N, "n_arms = 0", "[1, 16]"]), ("n_arms -3", _BOTH, -1, [_N, "n_arms = -3"]), ("n_arms 17", _BOTH, -1, [_N, "n_arms = 17"]),
    ("arm_masks NULL", _BOTH, -1, [_N, "arm_masks", "is NULL"]), ("msd NULL", _BOTH, -1, [_N, "msd", "is NULL"]),
    ("mask bit 3, n_groups 2", _BOTH, -1, [_N, "arm_masks[2] = 0x8", "beyond n_groups = 2"]),
    ("mask bit 31", _BOTH, -1, [_N, "arm_masks[5] = 0x80000001", "beyond n_groups = 2"]),
    ("rest bit, groups cover all of L", _BOTH, -1, [_N, "arm_masks[1] = 0x6", "rest block", "cover all L = 6"]),
    ("no groups: the rest block is bit 0, bits beyond it", _BOTH, -1, [_N, "beyond n_groups = 0"]),
    ("LDS: T 1024", _BOTH, -1, [_N, "LDS tables", "T = 1024", "n_arms = 6", "163840", "fewer arms per call"]),
    ("LDS: T 500, n_arms 16", _BOTH, -1, [_N, "LDS tables", "T = 500", "n_arms = 16 (384000 B"]),
] + _LABELS + [
    ("mean and sd NULL, mask 0 among the arms; workspace too small", _BOTH, -3, ["workspace 64 B < required"]),
] + _TWO + [                                                                          # two conditions at once: the earlier rung speaks
    ("no_fold + n_arms 0", _POST, -1, ["observation strides"]),
    ("n_arms 17 + arm_masks NULL", _BOTH, -1, ["n_arms = 17"]), ("msd NULL + mask bit 3", _BOTH, -1, ["arm_masks / msd is NULL"]),
    ("mask bit 3 + LDS", _BOTH, -1, ["arm_masks[1] = 0x9"]), ("LDS + label columns 3", _BOTH, -1, ["LDS tables"]),
    ("label columns 3 + workspace too small", _BOTH, -1, ["label tensors have 3 columns"]),
    # the plan
    ("shape NULL", _PLAN, -1, ["slode_attribution_plan", "shape is NULL"]), ("bad shape", _PLAN, -1, ["slode_attribution_plan", "T out of range"]),
    ("lds_bytes NULL", _PLAN, -1, ["slode_attribution_plan", "lds_bytes is NULL"]), ("n_arms 0", _PLAN, -1, ["slode_attribution_plan", "n_arms = 0"]),
    ("n_arms 17", _PLAN, -1, ["slode_attribution_plan", "n_arms = 17"]),
    ("LDS: T 1024", _PLAN, -1, ["slode_attribution_plan", "LDS tables", "n_arms = 6 (413600 B)"]),
    ("LDS: T 500, n_arms 16", _PLAN, -1, ["slode_attribution_plan", "n_arms = 16 (384000 B)"]),
]


def test_attribution_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_latent_attribution (posterior and prior) and of slode_attribution_plan without a device, in rung
    order: status, the words of the message and the untouched drawing-call counter against LADDER; line by line against
    tests/golden/attribution_refusals.txt; the rungs shared with slode_recon_moments carry the texts tests/golden/eval_refusals.txt records
    for it on that side, the call's name, its list of required pointers and its advice apart; the call's LDS figure is the plan's; and the
    memory that stands for the outputs untouched."""
    _, shared, figures = DL.check_ladder("attribution_refusals", tmp_path, LADDER, _N, "reduce the attribution samples instead")
    assert all(len(v) == 1 for v in figures.values()) and len(figures) == 2                # the call names the plan's figure
    assert shared >= 50


# ---- the fp32 restatement of the kernel's accumulation against fp64 ----------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 2, 7, 200])
def test_fma_accumulation_stays_within_the_accumulation_term(ns):
    """AU.msd_f32 (the kernel's operations in its order, fp32) against 1 / (2 ns) sum d^2 in fp64 of the same fp32 inputs, within
    ns 2^-24 msd: the arms lie within a factor of two of each other, so every difference is exact (Sterbenz, asserted) and what is left is
    the chain of ns fma roundings, each at most 2^-24 of a running sum that does not exceed the final one."""
    g = np.random.default_rng(9)
    level = g.uniform(0.5, 20.0, size=4096)
    v = (level[None, :] * (1.0 + 1e-2 * g.standard_normal((ns, 4096)))).astype(np.float32)
    va = (level[None, :] * (1.0 + 1e-2 * g.standard_normal((ns, 4096)))).astype(np.float32)
    assert np.array_equal((va - v).astype(np.float64), va.astype(np.float64) - v.astype(np.float64))
    want = 0.5 * np.mean((va.astype(np.float64) - v.astype(np.float64)) ** 2, 0)
    got = AU.msd_f32(v, va).astype(np.float64)
    r = np.abs(got - want) / (ns * AU.U24 * want)
    print("ns = %d: fp32 accumulation error / (ns 2^-24 msd): %.3f" % (ns, r.max()))
    assert want.min() > 0 and r.max() <= 1.0
    assert not AU.msd_f32(v, v).any()                                                     # an arm equal to the base: exactly 0


# ---- every condition the GPU tests assert, on the fp64 oracle alone ------------------------------------------------------------------------
ORACLE_CASES = ("cvs_ald", "challenge_gauss", "proc_ald")       # one per family
NS_ORACLE = 1500


@functools.lru_cache(maxsize=None)
def _oracle(case, is_post):
    """The oracle's curves of the base, of every arm of the family and of the all-blocks arm: B = 2, rk4, 1500 draws, computed once."""
    c = AU.build(case, "rk4", B=2, ns=NS_ORACLE)
    masks, single, comp = AU.arm_masks(c["ospec"])
    every = (1 << AU.n_blocks(c["ospec"])) - 1
    v, arms = AU.oracle_arms(c, is_post, masks + [every])
    return c, masks, single, comp, v, arms[:-1], arms[-1]


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_oracle_all_blocks_arm_reproduces_the_variance(case, is_post):
    """With every block redrawn the two arms are independent: msd estimates the plain variance.  Pointwise within 5 standard errors, the
    standard error taken from the same sample (the per-draw terms (v' - v)^2 / 2 - (v - mean)^2)."""
    c, masks, single, comp, v, arms, v_all = _oracle(case, is_post)
    var = np.var(v, 1)
    terms = 0.5 * (v_all - v) ** 2 - (v - np.mean(v, 1, keepdims=True)) ** 2
    se = np.std(terms, 1) / np.sqrt(NS_ORACLE)
    live = se > 0
    r = np.abs(AU.msd64(v, v_all) - var)[live] / se[live]
    print("%s %s: |msd(all blocks) - var| / standard error: max %.2f over %d values" % (case, "post" if is_post else "prior", r.max(), r.size))
    assert live.any() and r.max() <= 5.0


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_oracle_indices_and_the_two_block_identity(case, is_post):
    """The time-summed indices are finite, the totals positive; for the two-block families first_index[0] == 1 - total_index[1] (the
    complement of block 0 IS block 1: one arm serves both) to fp64 rounding."""
    c, masks, single, comp, v, arms, _ = _oracle(case, is_post)
    var = np.var(v, 1)
    msd = [AU.msd64(v, a) for a in arms]
    total = np.stack([msd[a] for a in single])
    first = np.stack([var - msd[a] for a in comp])
    ti, fi = AU.indices(var[None], total, first)
    print("%s %s: total index per block %s, first-order %s" % (case, "post" if is_post else "prior",
                                                             np.round(ti.mean(axis=(1, 2, 3)), 3), np.round(fi.mean(axis=(1, 2, 3)), 3)))
    assert np.isfinite(ti).all() and np.isfinite(fi).all() and (ti > 0).all()
    if AU.n_blocks(c["ospec"]) == 2:
        assert len(masks) == 2 and np.abs(fi[0] - (1.0 - ti[1])).max() <= 1e-12 and np.abs(fi[1] - (1.0 - ti[0])).max() <= 1e-12
    else:
        assert len(masks) == 6


@pytest.mark.parametrize("is_post", [True, False], ids=["post", "prior"])
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_oracle_msd_bar_discriminates(case, is_post):
    """An engine that dropped the 1/2, or gave an arm its neighbour's mask, would move msd by more than the bar, for every arm."""
    c, masks, single, comp, v, arms, _ = _oracle(case, is_post)
    for a, va in enumerate(arms):
        msd, bar = AU.msd64(v, va), AU.msd_bar(v, va)
        no_half = float((np.abs(2.0 * msd - msd) / bar).max())
        neighbour = float((np.abs(AU.msd64(v, arms[(a + 1) % len(arms)]) - msd) / bar).max())
        print("%s %s arm 0x%x: without the 1/2: %.1f bars; with the neighbour's mask 0x%x: %.1f bars"
              % (case, "post" if is_post else "prior", masks[a], no_half, masks[(a + 1) % len(arms)], neighbour))
        assert no_half > 1.0 and neighbour > 1.0


# ---- the Python layer on an engine double ---------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self, refuse, Q, fit=16):
        from structured_latent_odes_amd import _lib as L
        self.L, self.refuse, self.Q, self.fit = L, refuse, Q, fit
        self.calls, self.batches, self.draws, self.counter, self.set_to = [], [], [], 9, []
        self.spec = type("S", (), {"latent_dim": 4})()

    def draw_normal(self, rows):
        self.draws.append(rows)
        self.counter += 1
        return torch.arange(rows * 4, dtype=torch.float32).view(rows, 4) + 1000.0 * len(self.draws)

    def rng_state(self):
        return (0, 0, self.counter)

    def rng_set_counter(self, n):
        self.set_to.append(n)
        self.counter = n

    def make_batch(self, obs, labels, eps=None, particles=1, eps_shape=None):
        self.batches.append((tuple(obs.shape), len(labels), None if eps is None else tuple(eps.shape), particles, eps_shape))
        return object()

    def _err(self, status):
        err = self.L.SlodeError("libslode call failed (%d)" % status)
        err.status = status
        return err

    def attribution_plan(self, B, n_arms):
        if n_arms > self.fit:
            raise self._err(-1)
        return 1024 * n_arms

    def latent_attribution(self, flat, bt, B, is_post, num_samples, arm_masks, mean=None, sd=None):
        self.calls.append((bool(is_post), num_samples, list(arm_masks), mean, sd))
        if self.refuse:
            raise self._err(self.refuse)
        self.counter += 2
        q = torch.arange(self.Q, dtype=torch.float32).view(self.Q, 1, 1, 1) + torch.zeros(self.Q, B, 3, 10)
        msd = torch.stack([q + 0.125 * m for m in arm_masks], 0)
        return (None if mean is False else q + 10), (None if sd is False else q + 2), msd


FAMILIES = {"cvs": (("iext", "rtpr"), [("p_z_iext_given_iext", ["iext"], ["iext"]), ("p_z_rtprs_given_rtprs", ["rtpr"], ["rtpr"])], ("iext", "rtpr", "epsilon"),
                    {"iext": 1, "rtpr": 1, "epsilon": 2}),
            "proc": (("aR", "aS"), [("p_z_u_given_u", ["aR", "aS"], ["aR", "aS"])], ("aR", "aS", "epsilon"), {"aR": 1, "aS": 1, "epsilon": 2})}


def _double(gauss, refuse, fam="cvs", fit=16):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class M(MechanisticBase):
        FAMILY, GAUSS = fam, gauss
        LABELS, PRIORS, Z_GROUPS, _DIMS = FAMILIES[fam]

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, 1 if gauss else 3, fit), "flat": torch.zeros(1)})()
            self.z_dims, self.z_off, off = dict(self._DIMS), {}, 0
            for g in self.Z_GROUPS:
                self.z_off[g] = off
                off += self.z_dims[g]
            self.latent_dim = off
            self.decoded = []

        def _bind(self):
            return self._b

        def _loc_scale(self, observations, is_post, labels):
            B = observations.shape[0]
            return observations[:, 0, :1].expand(B, 4).clone(), torch.ones(B, 4)

        def _decoded_draws(self, z):
            """every head curve = the sum over the latent dims weighted 1, 2, 4, 8 (+ 100 per curve): linear, so the indices are known."""
            ns, B = z.shape[:2]
            self.decoded.append((ns, B))
            f = (z * torch.tensor([1.0, 2.0, 4.0, 8.0])).sum(-1).permute(1, 0).reshape(B, 1, 1, ns)
            names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
            return {n: (f + 100.0 * i).expand(B, 3, 10, ns) for i, n in enumerate(names)}

    return M()


def test_blocks_and_arm_lists():
    m = _double(False, 0)
    assert m.attribution_blocks() == ["iext", "rtpr", "epsilon"]
    assert m._attribution_arms(None) == (["iext", "rtpr", "epsilon"], [1, 6, 2, 5, 4, 3], [0, 2, 4], [1, 3, 5])
    assert m._attribution_arms(["epsilon"]) == (["epsilon"], [4, 3], [0], [1])
    p = _double(False, 0, "proc")
    assert p.attribution_blocks() == ["aR+aS", "epsilon"]
    assert p._attribution_arms(None) == (["aR+aS", "epsilon"], [1, 2], [0, 1], [1, 0])      # equal masks once: two arms serve four uses
    assert [m._block_dims(k).tolist() for k in (1, 2, 4, 6)] == [[True, False, False, False], [False, True, False, False],
                                                                   [False, False, True, True], [False, True, True, True]]
    for bad in (["symptoms"], ["iext", "z_epsilon"], []):
        with pytest.raises(ValueError, match="latent block"):
            m.latent_attribution(torch.zeros(2, 3, 10), True, 5, blocks=bad, iext=torch.zeros(2, 1), rtpr=torch.zeros(2, 1))
    with pytest.raises(ValueError, match="num_samples"):
        m.latent_attribution(torch.zeros(2, 3, 10), True, 0, iext=torch.zeros(2, 1), rtpr=torch.zeros(2, 1))
    assert m._b.engine.calls == [] and m._b.engine.batches == [] and m._b.engine.draws == []


def test_fewest_calls_that_fit():
    """The split of latent_attribution's arms and mechanism_moments' slots on its own: for 1 to 6 items, a cap of 1 to 6 per call and a plan
    that takes up to 1 to 6 (one item is never planned: the call itself refuses it), the slices cover every item once and in order, none
    is larger than the cap or than what the plan takes, no smaller number of calls would do, and the sizes differ by at most one."""
    from structured_latent_odes_amd import _lib as L
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    for n in range(1, 7):
        for cap in range(1, 7):
            for takes in range(1, 7):
                asked = []

                def plan(k):
                    asked.append(k)
                    if k > takes:
                        raise L.SlodeError("libslode call failed (-1)")
                slices = MechanisticBase._fewest_calls(n, cap, plan)
                most = min(n, cap, takes)
                assert [i for lo, hi in slices for i in range(lo, hi)] == list(range(n)), (n, cap, takes, slices)
                sizes = [hi - lo for lo, hi in slices]
                assert min(sizes) >= 1 and max(sizes) <= most and max(sizes) - min(sizes) <= 1, (n, cap, takes, slices)
                assert len(slices) == -(-n // most), (n, cap, takes, slices)                # fewer calls would need a larger one
                assert 1 not in asked and all(k <= min(n, cap) for k in asked)


@pytest.mark.parametrize("gauss", [False, True])
def test_model_level_call_uses_the_engine_once_and_splits_on_the_same_noise(gauss):
    obs = torch.arange(7, dtype=torch.float32).view(7, 1, 1).expand(7, 3, 10).contiguous()
    labels = dict(iext=torch.zeros(7, 1), rtpr=torch.ones(7, 1))
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, 0)
    eng = m._b.engine
    res = m.latent_attribution(obs, True, 5, **labels)
    assert eng.calls == [(True, 5, [1, 6, 2, 5, 4, 3], None, None)] and eng.batches == [((7, 3, 10), 2, None, 5, None)]
    assert eng.set_to == [9] and eng.counter == 11 and eng.draws == []                     # drawing calls n, n + 1: the counter ends at n + 2
    assert res["blocks"] == ["iext", "rtpr", "epsilon"] and set(res) == {"blocks"} | set(names)
    for q, n in enumerate(names):
        r = res[n]
        assert set(r) == {"mean", "var", "total", "first", "total_index", "first_index"}
        assert tuple(r["mean"].shape) == tuple(r["var"].shape) == (7, 3, 10) and tuple(r["total"].shape) == tuple(r["first"].shape) == (3, 7, 3, 10)
        assert tuple(r["total_index"].shape) == tuple(r["first_index"].shape) == (3, 7, 3) and r["total_index"].dtype == torch.float64
        var = (q + 2.0) ** 2
        assert float(r["mean"][0, 0, 0]) == q + 10 and float(r["var"][0, 0, 0]) == var
        assert [float(t[0, 0, 0]) for t in r["total"]] == [q + 0.125 * k for k in (1, 2, 4)]
        assert [float(t[0, 0, 0]) for t in r["first"]] == [var - (q + 0.125 * k) for k in (6, 5, 3)]
        assert torch.allclose(r["total_index"][:, 0, 0], torch.tensor([(q + 0.125 * k) / var for k in (1, 2, 4)], dtype=torch.float64), rtol=1e-12, atol=0)
    # explicit noise: one [2, ns, B, L] tensor, nothing drawn, the counter untouched
    m.latent_attribution(obs, False, 5, blocks=["rtpr"], eps=torch.zeros(2, 5, 7, 4), **labels)
    assert eng.calls[-1] == (False, 5, [2, 5], None, None) and eng.batches[-1] == ((7, 3, 10), 2, (2, 5, 7, 4), 5, (2, 5, 7, 4)) and eng.set_to == [9]
    # the plan lets four arms into one call: six arms over the fewest calls (two, three arms each), every call on the counter rewound; the
    # base moments come from the first call alone
    m2 = _double(gauss, 0, fit=4)
    e2 = m2._b.engine
    split = m2.latent_attribution(obs, True, 5, **labels)
    assert e2.calls == [(True, 5, [1, 6, 2], None, None), (True, 5, [5, 4, 3], False, False)] and e2.set_to == [9, 9] and e2.counter == 11
    for n in names:
        assert all(torch.equal(split[n][k], res[n][k]) for k in ("mean", "var", "total", "first", "total_index", "first_index"))
    type(m2).ATTRIBUTION_ARMS_PER_CALL = 1
    one = m2.latent_attribution(obs, True, 5, **labels)
    assert [c[2] for c in e2.calls[2:]] == [[1], [6], [2], [5], [4], [3]] and e2.counter == 13
    assert all(torch.equal(one[n]["first"], res[n]["first"]) for n in names)


def test_index_is_nan_where_the_curve_has_no_variance():
    m = _double(True, 0)
    mean, var = torch.zeros(1, 2, 3, 10), torch.zeros(1, 2, 3, 10)
    var[0, 1] = 1.0
    r = m._attribution_result(["iext"], [0], [1], mean, var, torch.full((2, 1, 2, 3, 10), 0.25))["mean"]
    assert torch.isnan(r["total_index"][0, 0]).all() and torch.isnan(r["first_index"][0, 0]).all()
    assert torch.equal(r["total_index"][0, 1], torch.full((3,), 0.25, dtype=torch.float64)) and float(r["first_index"][0, 1, 0]) == 0.75


@pytest.mark.parametrize("gauss", [False, True])
def test_composed_route_on_a_refusal(gauss, monkeypatch):
    """The engine refuses (status -1): two drawing calls for the whole batch, every arm's latents from the same two noise tensors, the
    chunked composition reduced in fp64.  The double's curves are linear in z with weights 1, 2, 4, 8 and unit scales, so as ns grows the
    total and first-order variance of a block both tend to the sum of its squared weights; at ns = 5 the exact identities are checked: a
    mask-0-free arm list, first = var - msd of the complement, the result independent of the chunking."""
    obs = torch.arange(7, dtype=torch.float32).view(7, 1, 1).expand(7, 3, 10).contiguous()
    labels = dict(iext=torch.zeros(7, 1), rtpr=torch.ones(7, 1))
    names = ("mean",) if gauss else ("mu_50", "mu_75", "mu_25")
    m = _double(gauss, -1)
    eng = m._b.engine
    res = m.latent_attribution(obs, True, 5, **labels)
    assert len(eng.calls) == 1 and eng.draws == [35, 35] and m.decoded == [(5, 7)] * 7
    e0 = (torch.arange(35 * 4, dtype=torch.float64).view(5, 7, 4) + 1000.0)
    e1 = e0 + 1000.0
    w = torch.tensor([1.0, 2.0, 4.0, 8.0], dtype=torch.float64)
    base = (e0 * w).sum(-1)                                                                  # (+ loc: cancels in every quantity below)
    var = base.var(0, unbiased=False)
    for n in names:
        r = res[n]
        assert r["var"].dtype == torch.float32 and torch.allclose(r["var"][:, 0, 0].double(), var, rtol=1e-6)
        for p, (bit, dims) in enumerate(((1, [0]), (2, [1]), (4, [2, 3]))):
            d = ((e1 - e0)[..., dims] * w[dims]).sum(-1)
            assert torch.allclose(r["total"][p, :, 0, 0].double(), 0.5 * (d ** 2).mean(0), rtol=1e-6)
            rest = [l for l in range(4) if l not in dims]
            dc = ((e1 - e0)[..., rest] * w[rest]).sum(-1)
            assert torch.allclose(r["first"][p, :, 0, 0].double(), var - 0.5 * (dc ** 2).mean(0), rtol=1e-5, atol=1e-2)
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)                                  # 15 // 5 = 3 rows per chunk: 3 + 3 + 1
    eng.draws.clear()
    m.decoded.clear()
    eng.counter = 9
    chunked = m.latent_attribution(obs, True, 5, **labels)
    assert eng.draws == [35, 35] and m.decoded == [(5, 3)] * 7 + [(5, 3)] * 7 + [(5, 1)] * 7
    given = m.latent_attribution(obs, True, 5, eps=torch.stack([e0, e1]).float(), **labels)
    assert eng.draws == [35, 35]                                                            # explicit noise draws nothing
    for n in names:
        for k in ("mean", "var", "total", "first", "total_index", "first_index"):
            assert torch.equal(chunked[n][k], res[n][k]) and torch.equal(given[n][k], res[n][k]), (n, k)


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(False, refuse=status)
    with pytest.raises(L.SlodeError):
        m.latent_attribution(torch.zeros(2, 3, 10), True, 5, iext=torch.zeros(2, 1), rtpr=torch.zeros(2, 1))
    assert m.decoded == [] and m._b.engine.draws == []


def test_save_latent_attribution_files_and_line(tmp_path):
    m = _double(False, 0, "proc")
    batches = [dict(observations=torch.zeros(B, 3, 10), aR=torch.zeros(B, 1), aS=torch.zeros(B, 1)) for B in (2, 3)]
    files = m.save_latent_attribution(str(tmp_path / "r"), batches, False, 4)
    want = ["attribution_%s_prior.npy" % k for k in ("total", "first", "total_index", "first_index")] + ["attribution_blocks.txt"]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "r"))) == sorted(want)
    assert open(files[-1]).read().split() == ["aR+aS", "epsilon"]
    total, first, ti, fi = (np.load(f) for f in files[:4])
    assert total.shape == first.shape == (3, 2, 5, 3, 10) and total.dtype == np.float32 and ti.shape == fi.shape == (3, 2, 5, 3) and ti.dtype == np.float64
    line = m.attribution_line(ti, fi, "prior")
    assert line.startswith("attribution_prior: n=5  aR+aS total=") and "epsilon total=" in line and line.count("first=") == 2


def test_training_entry_points_take_the_flag():
    import inspect
    from structured_latent_odes_amd import training as TR
    assert inspect.signature(TR.train).parameters["attribution"].default == 0
    assert TR.build_parser().parse_args(["--attribution", "64"]).attribution == 64 and TR.build_parser().parse_args([]).attribution == 0
