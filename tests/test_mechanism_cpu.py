"""CPU tests of the mechanism curves: the C ABI of slode_mechanism_moments / slode_mechanism_plan, the plan against a hand count of the
kernel's tables (every case, several slot masks, a shape that fits one slot and not five), the refusal ladder on a hand-filled handle
(tests/mechanism_refusals/mechanism_refusals.cpp), the conditions the GPU tests rest on shown for the fp64 oracle alone (the bars against
the fp32 oracle's distance, the smallest degradation of the cases), and the Python layer on an engine double (the dict, the slot split,
the composed route, the files, the flag)."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import draws_ladder_util as DL
from tests import eval_stats_util as EU
from tests import lds_util as LU
from tests import mechanism_util as MU
from tests import recon_moments_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "is_post", "num_samples", "slots", "mean", "sd", "workspace", "workspace_bytes",
        "stream"]


def test_abi_exports_mechanism_moments_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    for name in ("slode_mechanism_moments", "slode_mechanism_plan"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 270 and "0.2.7: slode_mechanism_moments" in hdr
    for earlier in ("0.2.6: slode_recon_quantiles", "0.2.5: slode_curve_summary", "0.2.4: slode_latent_attribution", "0.2.3: slode_pointwise_density",
                    "0.2.2: slode_posterior_refine", "0.1.5: slode_recon_moments", "0.1.1: slode_svi_step"):
        assert earlier in hdr                                                             # the earlier version lines are kept
    m = re.search(r"int\s+slode_mechanism_moments\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_mechanism_moments.argtypes
    assert len(at) == len(ARGS) and at[7] is C.c_int and at[8] is C.c_int and at[9] is C.c_uint and at[13] is C.c_size_t
    assert re.search(r"int\s+slode_mechanism_plan\s*\(\s*const slode_shape\*\s*s,\s*unsigned int slots,\s*size_t\*\s*lds_bytes\s*\)\s*;", hdr)
    assert int(re.search(r"#define\s+SLODE_MECHANISM_SLOTS\s+(\d+)", hdr).group(1)) == L.MECHANISM_SLOTS == len(L.MECHANISM_NAMES) == 5
    assert L.MECHANISM_NAMES == MU.NAMES == ("state", "production", "degradation", "set_point", "net_rate")
    doc = hdr[hdr.index("mechanism curves as ONE call"):m.start()]
    for word in ("NULL handle", "num_samples < 1", "adaptive solver", "dopri5", "particles > 1", "SLODE_NO_FOLD", "SLODE_ODE_ALG", "LDS tables",
                 "SLODE_EINVAL", "n + 1", "POPULATION", "state", "production", "degradation", "set_point", "net_rate", "fmaf(-d, x_i[s], a)",
                 "stage_t[i R]", "stage_t[R (T - 1)]", '"weff"', '"enc_fwd2"', '"mechanism_moments"', "mean NULL", "slots == 0", "no atomics",
                 "[n_sel, B, S, T]", "capture table", "slode_mechanism_plan", "first_trajectory", "capturable"):
        assert word in doc, word
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_MECHANISM_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_mechanism_lds_bytes" in common
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "mechanism_moments_kernel.hip" in srcs
    assert "slode_mechanism_moments" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert '"recon_quantiles", "mechanism_moments", "intervene_moments"' in hdr              # the names slode_profile_read documents
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_mechanism_moments(None, None, None, None, None, None, None, 1, 8, 31, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


def test_engine_and_model_signatures():
    from structured_latent_odes_amd.engine import Engine
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase
    assert list(inspect.signature(Engine.mechanism_moments).parameters) == ["self", "params", "batch", "B", "is_post", "num_samples", "slots", "mean",
                                                                           "sd"]
    assert list(inspect.signature(Engine.mechanism_plan).parameters) == ["self", "B", "slots"]
    sig = inspect.signature(MechanisticBase.mechanism_moments).parameters
    assert list(sig)[:6] == ["self", "observations", "is_post", "num_samples", "quantities", "eps"] and sig["quantities"].default is None
    assert list(inspect.signature(MechanisticBase.save_mechanism_moments).parameters) == ["self", "results_dir", "batches", "is_post", "num_samples"]
    assert MechanisticBase.MECHANISM_NAMES == MU.NAMES


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def _hand_count(eng, n_sel):
    sp = eng.spec
    return MU.plan_bytes(eng.T, sp.ode_state_dim, sp.n_channels, sp.latent_dim, sp.ode_hidden_dim, sp.n_u, sp.gauss, n_sel)


MASKS = (0x01, 0x08, 0x0a, 0x15, 0x1e, 0x1f)


@pytest.mark.parametrize("case", list(EU.CASES))
def test_plan_against_a_hand_count_of_the_tables(case):
    """Every case, several masks: the plan is the hand count (MU.plan_bytes) for the mask's population count, depends on the count alone, and
    one slot costs exactly 4 r4(3 S T) bytes."""
    eng = LU.host_engine(case)
    S, T = eng.spec.ode_state_dim, eng.T
    got = {m: eng.mechanism_plan(8, m) for m in MASKS}
    for m, b in got.items():
        n = bin(m).count("1")
        assert b == _hand_count(eng, n) <= 160 * 1024, (case, hex(m))
        assert b - got[0x01] == (n - 1) * 4 * LU.r4(3 * S * T), (case, hex(m))                 # the cost of one slot, exactly
    assert got[0x15] == eng.mechanism_plan(8, 0x07)
    assert eng.mechanism_plan(1, 0x1f) == eng.mechanism_plan(1024, 0x1f)                   # one workgroup per trajectory: B does not enter


def test_one_slot_costs_one_moment_table():
    """3 S T is a multiple of four on cvs at T = 200 (S = 5): every further slot adds exactly 4 r4(3 S T) = 12 S T bytes."""
    eng = LU.host_engine("cvs_ald")
    assert (eng.spec.ode_state_dim, eng.T) == (5, 200)
    sizes = [eng.mechanism_plan(8, (1 << n) - 1) for n in range(1, 6)]
    assert [b - a for a, b in zip(sizes, sizes[1:])] == [4 * LU.r4(3 * 5 * 200)] * 4 == [12000] * 4


def test_plan_of_a_shape_that_fits_one_slot_and_not_five():
    """cvs at T = 1024: the step table and the capture table are 2 x 5 x 1024 x 4 B = 40 KB each, one slot's triples 60 KB: one slot fits,
    five do not -- both figures computed here -- and a refusal still writes the bytes."""
    from structured_latent_odes_amd import _lib as L
    eng = LU.host_engine("cvs_ald", T=1024)
    assert (eng.spec.ode_state_dim, eng.spec.gauss) == (5, False)
    one, five = _hand_count(eng, 1), _hand_count(eng, 5)
    assert five - one == 4 * 4 * LU.r4(3 * 5 * 1024) and one <= 160 * 1024 < five
    assert eng.mechanism_plan(8, 0x10) == one
    with pytest.raises(L.SlodeError, match=r"T = 1024, S = 5, slots = 5 \(%d B\) exceed the budget of 163840 B" % five):
        eng.mechanism_plan(8, 0x1f)
    lib, r = L.load(), C.c_size_t(0)
    assert lib.slode_mechanism_plan(C.byref(eng.shape(8)), 0x1f, C.byref(r)) == -1 and r.value == five
    r.value = 0
    assert lib.slode_mechanism_plan(C.byref(eng.shape(8)), 0x3f, C.byref(r)) == -1 and r.value == five     # a bad mask: the bytes of its valid bits
    assert b"bits at or beyond SLODE_MECHANISM_SLOTS" in lib.slode_last_error(None)
    with pytest.raises(L.SlodeError, match="selects nothing"):
        eng.mechanism_plan(8, 0)


# ---- the refusal ladder ---------------------------------------------------------------------------------------------------------------------
_N = "slode_mechanism_moments"
_P = "slode_mechanism_plan"
_BOTH, _POST, _PRIOR, _PLAN = ("post", "prior"), ("post",), ("prior",), ("plan",)
_ADVICE = "compose slode_ode_solve_fwd and the dynamics net instead"
_HEAD, _LABELS, _TWO = DL.shared_rungs(_N, "batch / times / stage_t / workspace", _ADVICE)
LADDER = _HEAD + [
    ("mean NULL", _BOTH, -1, [_N + ": mean is NULL"]), ("slots 0", _BOTH, -1, [_N + ": slots = 0x0 selects nothing"]),
    ("slots bit 5", _BOTH, -1, [_N + ": slots = 0x20", "bits at or beyond SLODE_MECHANISM_SLOTS = 5"]),
    ("slots all + bit 31", _BOTH, -1, [_N + ": slots = 0x8000001f"]),
    ("LDS: T 1024, five slots", _BOTH, -1, [_N + ": the LDS tables of T = 1024, S = 5, C = 3, slots = 5 (393120 B: step table, moment triples, "
                                             "capture table, staged weights) exceed the budget of 163840 B", "slode_mechanism_plan"]),
    ("LDS: T 1024, two slots", _BOTH, -1, [_N, "slots = 2 (208800 B"]),
    ("T 1024, one slot, run-time S build: fits; workspace too small", _BOTH, -3, ["workspace 64 B < required"]),
    ("T 1024, one slot: fits; workspace too small", _BOTH, -3, ["workspace 64 B < required"]),
] + _LABELS + [
    ("sd NULL, one slot; workspace too small", _BOTH, -3, ["workspace 64 B < required"]),
] + _TWO + [                                                                          # two conditions at once: the earlier rung speaks
    ("no_fold + mean NULL", _POST, -1, ["observation strides"]),
    ("mean NULL + slots 0", _BOTH, -1, ["mean is NULL"]), ("slots bit 7 + LDS", _BOTH, -1, ["slots = 0x9f"]),
    ("LDS + label columns 3", _BOTH, -1, ["LDS tables"]), ("label columns 3 + workspace too small", _BOTH, -1, ["label tensors have 3 columns"]),
    # the plan (its counter column: the bytes it wrote)
    ("shape NULL", _PLAN, -1, [_P, "shape is NULL"]), ("bad shape", _PLAN, -1, [_P, "T out of range"]), ("lds_bytes NULL", _PLAN, -1, [_P, "lds_bytes is NULL"]),
    ("slots 0", _PLAN, -1, [_P, "slots = 0x0 selects nothing"]), ("slots bit 5", _PLAN, -1, [_P, "slots = 0x21"]),
    ("LDS: T 1024, five slots", _PLAN, -1, [_P, "T = 1024, S = 5, slots = 5 (393120 B) exceed the budget of 163840 B"]),
    ("LDS: T 1024, two slots", _PLAN, -1, [_P, "slots = 2 (208800 B)"]),
]
PLAN_BYTES = {"shape NULL": 0, "bad shape": 0, "lds_bytes NULL": 0, "LDS: T 1024, five slots": 393120, "LDS: T 1024, two slots": 208800}


def test_mechanism_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_mechanism_moments (posterior and prior) and of slode_mechanism_plan without a device, in rung
    order: status, the words of the message and the untouched drawing-call counter against LADDER; line by line against
    tests/golden/mechanism_refusals.txt; the rungs shared with slode_recon_moments carry the texts tests/golden/eval_refusals.txt records
    for it on that side, the call's name, its list of required pointers and its advice apart; the call's LDS figures are the plan's and
    the hand count's; a refused plan has written its bytes; and the memory that stands for the outputs is untouched."""
    def plan_line(name, counter, line):      # (the plan's counter column: the bytes it wrote, refused or not)
        assert counter == PLAN_BYTES.get(name, counter) and (name not in ("slots 0", "slots bit 5") or counter > 0), line
    _, shared, figures = DL.check_ladder("mechanism_refusals", tmp_path, LADDER, _N, _ADVICE, plan_line=plan_line, not_shared=("mean NULL",))
    figures = {k: int(*v) for k, v in figures.items()}
    eng = LU.host_engine("cvs_ald", T=1024)
    assert figures == {"LDS: T 1024, five slots": PLAN_BYTES["LDS: T 1024, five slots"] == _hand_count(eng, 5) and _hand_count(eng, 5),
                       "LDS: T 1024, two slots": _hand_count(eng, 2)}
    assert shared >= 40


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------------
def test_restatement_of_the_two_derived_slots():
    a, d, x = RU._f32([0.75, 0.1, 1.0]), RU._f32([0.5, 0.3, 3.0]), RU._f32([2.0, 1.0 / 3.0, 1.0 / 3.0])
    assert MU.set_point_f32(a, d).tolist() == [1.5, float(np.float32(0.1) / np.float32(0.3)), float(np.float32(1.0) / np.float32(3.0))]
    nr = MU.net_rate_f32(a, d, x)
    assert nr[0] == -0.25 and nr.dtype == np.float32
    # one rounding, not two: 1 - 3 * fl(1/3) is -2^-25 * ... exactly in the fma, and 0 with a rounded product
    assert nr[2] != 0.0 and RU._f32(a[2] - RU._f32(d[2] * x[2])) == 0.0
    m, s = RU.shifted_moments_f32(np.stack([nr]))
    assert np.array_equal(m, nr) and np.all(s == 0.0)                                      # one draw: the mean is the draw, sd exactly 0


# ---- the conditions the GPU tests rest on, for the oracle alone ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _distances():
    return MU.fp32_distances()


def test_bars_follow_the_rule_and_the_fp32_oracle_stays_within_a_quarter():
    """Every slot's bar is RU's, or 4 x the fp32 CPU oracle's worst distance from the fp64 oracle where that is larger (within the rounding
    of the figure written down: 3 digits, upwards); the fp32 oracle stays within a quarter of every bar."""
    worst, _ = _distances()
    for n in MU.NAMES:
        (wm, ws), (bm, bs) = worst[n], MU.BARS[n]
        print("%-12s fp32-vs-fp64 worst mean %.3e sd %.3e   4 x %.3e %.3e   bar %.3e %.3e" % (n, wm, ws, 4 * wm, 4 * ws, bm, bs))
        assert wm <= bm / 4 and ws <= bs / 4, n
        for w, b, ru in ((wm, bm, RU.MEAN_BAR), (ws, bs, RU.SD_BAR)):
            assert b == ru if 4 * w <= ru else 4 * w <= b <= 4 * w * 1.005, (n, w, b)


def test_oracle_smallest_degradation_of_the_cases():
    """The condition on the cases: the fp64 oracle's smallest d over all draws, times and states is at least MU.MIN_D = 1e-3 on every case
    a set point is compared on -- MU.build of every case of EU.CASES, of MU.SIZES, MU.grid_case at T in MU.GRID_T, both sides (a and d at
    the grid times do not depend on the solver).  RU.build's cases as they are do not meet it (the right column of MU's table, printed
    here too): that is why the set point is compared on their conditioned form."""
    table = MU.condition_table()
    for tag, smallest in table.items():
        print("%-40s the oracle's smallest d %.3e" % (tag, smallest))
    _, cond = _distances()
    for (case, side), (now, as_built) in cond.items():
        print("%s %s: conditioned %.3e, as built %.3e" % (case, side, now, as_built))
    assert len(table) >= 40 and min(table.values()) >= MU.MIN_D, {k: v for k, v in table.items() if v < MU.MIN_D}
    assert sum(as_built < MU.MIN_D for _, as_built in cond.values()) == 11           # what the conditioning is for


def test_conditioned_cases_keep_everything_but_the_grid_and_two_label_columns():
    for case in ("cvs_ald", "proc_gauss"):
        a, b = RU.build(case, "midpoint", B=3, ns=2), MU.build(case, "midpoint", B=3, ns=2)
        assert set(a) == set(b) and all(torch.equal(a["p"][k], b["p"][k]) for k in a["p"])
        assert all(torch.equal(a[k], b[k]) for k in ("obs", "eps")) and all(a[k] == b[k] for k in ("B", "T", "S", "ns", "fam", "kw"))
        assert float(b["times"][0]) == 0.0 and float(b["times"][-1]) == MU.SPAN and torch.allclose(b["times"] * float(a["times"][-1]), a["times"])
        if case == "proc_gauss":
            assert torch.equal(a["u"][:, :7], b["u"][:, :7]) and torch.allclose(b["u"][:, 7:], a["u"][:, 7:] * MU.PROC_CONC)
        else:
            assert torch.equal(a["u"], b["u"])


def test_oracle_production_and_degradation_are_those_of_the_vector_field():
    """MU.production_degradation reads the parameters O.dynamics reads: a - d x equals O.dynamics at every grid time."""
    from oracle import slode_oracle as O
    c = RU.build("cvs_ald", "rk4", B=3, ns=2)
    p = EU.f64(c["p"])
    z = torch.randn(5, c["ospec"].latent_dim, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    x = torch.rand(5, c["S"], dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    a, d = MU.production_degradation(p, z, c["times"].double())
    for i in (0, 7, c["T"] - 1):
        assert torch.allclose(a[:, i] - d[:, i] * x, O.dynamics(p, c["times"][i].double().reshape(1, 1), x, z), rtol=0, atol=1e-15)


# ---- the Python layer on an engine double ---------------------------------------------------------------------------------------------
class _Eng:
    """mean of slot q = q + 0.01 b + 0.001 s (constant in t), sd = mean + 0.5: a value names its slot, trajectory and state."""
    S, T = 2, 6

    def __init__(self, refuse=0, fit=5):
        from structured_latent_odes_amd import _lib as L
        self.L, self.refuse, self.fit = L, refuse, fit
        self.calls, self.batches, self.draws, self.plans, self.counter, self.counters = [], [], [], [], 9, []

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

    def _raise(self, status):
        err = self.L.SlodeError("libslode call failed (%d)" % status)
        err.status = status
        raise err

    def mechanism_plan(self, B, slots):
        self.plans.append(slots)
        if bin(slots).count("1") > self.fit:
            self._raise(-1)
        return 1000

    def mechanism_moments(self, flat, bt, B, is_post, num_samples, slots, mean=None, sd=None):
        self.calls.append((bool(is_post), num_samples, slots))
        self.counters.append(self.counter)
        if self.refuse:
            self._raise(self.refuse)
        self.counter += 1
        sel = [q for q in range(5) if (slots >> q) & 1]
        m = (torch.tensor(sel, dtype=torch.float32).view(-1, 1, 1, 1) + 0.01 * torch.arange(B, dtype=torch.float32).view(1, B, 1, 1)
             + 0.001 * torch.arange(self.S, dtype=torch.float32).view(1, 1, self.S, 1) + torch.zeros(len(sel), B, self.S, self.T))
        return m, m + 0.5


def _double(refuse=0, fit=5):
    from structured_latent_odes_amd.models._mechanistic import MechanisticBase

    class _Dyn:
        @staticmethod
        def prod(tz):                        # a = sigmoid(0.1 t + z_0), one value per state
            return torch.sigmoid(0.1 * tz[..., 0:1] + tz[..., 1:2]).expand(*tz.shape[:-1], 2)

        @staticmethod
        def degr(tz):                        # d = sigmoid(z_1 - 0.05 t)
            return torch.sigmoid(tz[..., 2:3] - 0.05 * tz[..., 0:1]).expand(*tz.shape[:-1], 2)

    class _Ode:
        dynamics = _Dyn()

        def __init__(self, owner):
            self.owner = owner

        def solve_ODE(self, z):              # x[n, t, s] = z_2 + s + 0.1 t
            self.owner.solved.append(z.shape[0])
            t = self.owner.times
            return z[:, 2].reshape(-1, 1, 1) + torch.arange(2.0).reshape(1, 1, 2) + 0.1 * t.reshape(1, -1, 1)

    class M(MechanisticBase):
        FAMILY, GAUSS = "cvs", False
        LABELS = ("iext", "rtpr")

        def __init__(self):
            torch.nn.Module.__init__(self)
            self._b = type("B", (), {"engine": _Eng(refuse, fit), "flat": torch.zeros(1)})()
            self.times = torch.tensor([0.0, 1.0, 3.0, 4.0, 8.0, 9.0])
            self.solved = []
            object.__setattr__(self, "decoder", type("D", (), {"ode_model": _Ode(self)})())

        def _bind(self):
            return self._b

        def _loc_scale(self, observations, is_post, labels):
            B = observations.shape[0]                                                      # loc from the labels: rows keep theirs in a chunk
            return labels["iext"].to(torch.float32).view(B, 1).expand(B, 4), torch.full((B, 4), 0.5 if is_post else 2.0)

    return M()


LABELS = dict(iext=0.1 * torch.arange(7.0).view(7, 1), rtpr=torch.ones(7, 1))
OBS = torch.zeros(7, 3, 6)


def test_model_level_call_uses_the_engine_once():
    m = _double()
    eng = m._b.engine
    res = m.mechanism_moments(OBS, True, 5, **LABELS)
    assert eng.calls == [(True, 5, 0x1f)] and eng.batches == [((7, 3, 6), 2, None, 5)] and eng.draws == [] and eng.counter == 10
    assert res["quantities"] == MU.NAMES and set(res) == set(MU.NAMES) | {"quantities"}
    for q, n in enumerate(MU.NAMES):
        mean, sd = res[n]
        assert tuple(mean.shape) == tuple(sd.shape) == (7, 6, 2)                          # [B, T, S]: a permuted view of the engine's [B, S, T]
        assert float(mean[3, 0, 1]) == pytest.approx(q + 0.03 + 0.001) and float(sd[3, 5, 1]) == pytest.approx(q + 0.531)
    some = m.mechanism_moments(OBS, False, 5, quantities=("net_rate", "production"), eps=torch.zeros(5, 7, 4), **LABELS)
    assert eng.calls[-1] == (False, 5, 0x12) and eng.batches[-1] == ((7, 3, 6), 2, (5, 7, 4), 5)
    assert some["quantities"] == ("net_rate", "production") and set(some) == {"quantities", "net_rate", "production"}
    assert float(some["net_rate"][0][0, 0, 0]) == 4.0 and float(some["production"][0][0, 0, 0]) == 1.0     # stored in increasing slot order
    for bad in (("state", "rate"), ("set point",), ()):
        with pytest.raises(ValueError, match="quantities"):
            m.mechanism_moments(OBS, True, 5, quantities=bad, **LABELS)
    with pytest.raises(ValueError, match="num_samples"):
        m.mechanism_moments(OBS, True, 0, **LABELS)
    assert len(eng.calls) == 2


@pytest.mark.parametrize("fit,want", [(5, [0x1f]), (4, [0x07, 0x18]), (3, [0x07, 0x18]), (2, [0x03, 0x0c, 0x10]), (1, [1, 2, 4, 8, 16])])
def test_slot_split_runs_every_call_on_the_same_noise(fit, want):
    """The plan refuses more than ``fit`` slots: the fewest calls that fit, evenly filled, in slot order; the generator's counter is rewound
    to n0 before each and ends at n0 + 1; the dict is that of the single call."""
    m = _double(fit=fit)
    eng = m._b.engine
    res = m.mechanism_moments(OBS, True, 5, **LABELS)
    assert [c[2] for c in eng.calls] == want and eng.counters == [9] * len(want) and eng.counter == 10
    single = _double().mechanism_moments(OBS, True, 5, **LABELS)
    for n in MU.NAMES:
        assert torch.equal(res[n][0], single[n][0]) and torch.equal(res[n][1], single[n][1])
    eng.calls.clear(); eng.counters.clear()
    m.mechanism_moments(OBS, True, 5, eps=torch.zeros(5, 7, 4), **LABELS)                  # explicit noise: nothing to rewind
    assert [c[2] for c in eng.calls] == want and eng.counter == 10 + len(want)


def test_forced_split():
    m = _double()
    type(m).MECHANISM_SLOTS_PER_CALL = 2
    m.mechanism_moments(OBS, True, 5, quantities=("state", "set_point", "net_rate"), **LABELS)
    assert [c[2] for c in m._b.engine.calls] == [0x09, 0x10]


def test_composed_route_on_a_refusal(monkeypatch):
    """The engine refuses (status -1): one drawing call for the whole batch (the counter at n + 1, as the engine call leaves it), the states
    from decoder.ode_model.solve_ODE, a and d from dynamics.prod / dynamics.degr on cat([t_i, z]) for all grid times at once, the five
    quantities reduced in fp32 -- equal to numpy on the same definitions; the means do not depend on the chunking, the sds to 1e-6."""
    m = _double(refuse=-1)
    eng = m._b.engine
    res = m.mechanism_moments(OBS, False, 5, **LABELS)
    assert len(eng.calls) == 1 and eng.draws == [35] and m.solved == [35] and eng.counter == 10
    eps = torch.linspace(-1.0, 1.0, 35 * 4).view(5, 7, 4).double()
    loc, scale = m._loc_scale(OBS, False, LABELS)
    z = loc.double().unsqueeze(0) + scale.double().unsqueeze(0) * eps                    # [ns, B, L]
    t = m.times.double().view(1, 1, 6, 1)
    x = z[..., 2].view(5, 7, 1, 1) + torch.arange(2.0).double().view(1, 1, 1, 2) + 0.1 * t
    a = torch.sigmoid(0.1 * t + z[..., 0].view(5, 7, 1, 1)).expand(5, 7, 6, 2)
    d = torch.sigmoid(z[..., 1].view(5, 7, 1, 1) - 0.05 * t).expand(5, 7, 6, 2)
    want = dict(state=x, production=a, degradation=d, set_point=a / d, net_rate=a - d * x)
    for n in MU.NAMES:
        mean, sd = res[n]
        assert tuple(mean.shape) == (7, 6, 2) and mean.dtype == torch.float32
        assert np.allclose(mean.numpy(), want[n].mean(0).numpy(), rtol=1e-5, atol=1e-6), n
        assert np.allclose(sd.numpy(), want[n].std(0, unbiased=False).numpy(), rtol=1e-4, atol=1e-5), n
    given = m.mechanism_moments(OBS, False, 5, eps=eps.float(), **LABELS)                  # explicit noise draws nothing
    assert eng.draws == [35] and eng.counter == 10 and all(torch.equal(given[n][k], res[n][k]) for n in MU.NAMES for k in (0, 1))
    m.solved.clear()
    monkeypatch.setattr(type(m), "MOMENTS_CHUNK_ROWS", 15)                                  # 15 // 5 = 3 rows per chunk: 3 + 3 + 1
    m.solved.clear()
    chunked = m.mechanism_moments(OBS, False, 5, quantities=("set_point", "state"), **LABELS)
    assert m.solved == [15, 15, 5] and eng.draws == [35, 35] and chunked["quantities"] == ("set_point", "state")
    for n in ("set_point", "state"):
        assert torch.equal(chunked[n][0], res[n][0])
        # torch.std's summation tree depends on the tensor's size: the sd of values of size 1 .. 3 moves by roundings of 2^-24 of them
        assert float((chunked[n][1] - res[n][1]).abs().max()) <= 1e-6


@pytest.mark.parametrize("status", [-2, -3])
def test_only_a_refusal_leads_to_the_composition(status):
    from structured_latent_odes_amd import _lib as L
    m = _double(refuse=status)
    with pytest.raises(L.SlodeError):
        m.mechanism_moments(OBS, True, 5, **LABELS)
    assert m.solved == [] and m._b.engine.draws == []


def test_save_mechanism_moments_files_and_line(tmp_path):
    m = _double()
    batches = [dict(observations=torch.zeros(B, 3, 6), iext=torch.zeros(B, 1), rtpr=torch.zeros(B, 1)) for B in (2, 3)]
    files = m.save_mechanism_moments(str(tmp_path / "r"), batches, False, 4)
    want = ["mechanism_%s_prior_%s.npy" % (n, k) for n in MU.NAMES for k in ("mean", "sd")]
    assert [os.path.basename(f) for f in files] == want and sorted(os.listdir(str(tmp_path / "r"))) == sorted(want)
    arrays = {os.path.basename(f): np.load(f) for f in files}
    for q, n in enumerate(MU.NAMES):
        mean, sd = arrays["mechanism_%s_prior_mean.npy" % n], arrays["mechanism_%s_prior_sd.npy" % n]
        assert mean.shape == sd.shape == (5, 6, 2) and mean.dtype == np.float32            # [n, T, S], the trajectories in loader order
        assert mean[2, 0, 0] == np.float32(q) and mean[4, 0, 1] == pytest.approx(q + 0.021, abs=1e-6) and sd[0, 0, 0] == np.float32(q + 0.5)
    line = m.mechanism_line({k: arrays["mechanism_%s_prior_mean.npy" % k] for k in ("production", "degradation", "set_point")}, "prior")
    assert line.startswith("mechanism_prior: n=5  x0 a=1.008 d=2.008 a/d=3.008  x1 a=1.009 d=2.009 a/d=3.009"), line


def test_training_entry_points_take_the_flag():
    from structured_latent_odes_amd import training as TR
    assert inspect.signature(TR.train).parameters["mechanism"].default == 0
    assert TR.build_parser().parse_args(["--mechanism", "64"]).mechanism == 64
    assert TR.build_parser().parse_args([]).mechanism == 0
    src = inspect.getsource(TR.main)
    assert 'kw["mechanism"] = a.mechanism' in src
