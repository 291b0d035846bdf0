"""CPU tests of the posterior refinement: the C ABI of slode_posterior_refine, its refusal ladder on a hand-filled handle
(tests/refine_refusals/refine_refusals.cpp), and the test infrastructure the GPU tests rest on (tests/refine_util.py): the weighted likelihood, the
reference gradient against finite differences, the transcription of the kernel's backward formulas against autograd, and every condition the
GPU tests ask of the kernel shown to hold for the reference alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import slode_oracle as O
from tests import refine_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "num_draws", "num_steps", "lr", "mask", "loc_out", "scale_out", "elbo_out",
        "grad0_out", "trace_out", "best_step", "workspace", "workspace_bytes", "stream"]
CONFIGS = [(case, solver, masked) for case in RU.CASES for solver in RU.SOLVERS for masked in (False, True)]


def test_abi_exports_posterior_refine_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    assert hasattr(lib, "slode_posterior_refine") and "slode_posterior_refine" in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 220 and "0.2.2" in hdr
    m = re.search(r"int\s+slode_posterior_refine\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_posterior_refine.argtypes
    assert len(at) == len(ARGS) and at[7] is C.c_int and at[8] is C.c_int and at[9] is C.c_float and at[18] is C.c_size_t
    doc = hdr[:hdr.index("int slode_profile_read(")]
    assert '"posterior_refine"' in doc[doc.rindex("/*"):]                                 # the launch name is documented at slode_profile_read
    common = open(os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "slode_common.h")).read()
    assert re.search(r"#define\s+SLODE_REFINE_LDS_MAX\s+\(160 \* 1024\)", common) and "slode_refine_lds_bytes" in common
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_posterior_refine(None, None, None, None, None, None, None, 0, 0, 0.0, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


# case -> status and the words its message must carry, written from include/slode.h in rung order
_N = "slode_posterior_refine"
LADDER = [
    ("handle NULL", -1, ["handle is NULL"]), ("shape NULL", -1, ["shape is NULL"]), ("layout NULL", -1, ["layout is NULL"]),
    ("params NULL", -1, ["params is NULL"]), ("batch NULL", -1, [_N, "batch", "is NULL"]), ("loc_out NULL", -1, [_N, "loc_out", "is NULL"]),
    ("scale_out NULL", -1, [_N, "scale_out", "is NULL"]), ("elbo_out NULL", -1, [_N, "elbo_out", "is NULL"]),
    ("times NULL", -1, [_N, "times", "is NULL"]), ("stage_t NULL", -1, [_N, "stage_t", "is NULL"]), ("workspace NULL", -1, [_N, "workspace", "is NULL"]),
    ("bad shape", -1, ["T out of range"]), ("draws 0", -1, [_N, "num_draws = 0 < 1"]), ("draws 2^30", -1, [_N, "B x num_draws", "2^30 - 1"]),
    ("adaptive method 3", -1, [_N, "adaptive solver dopri5"]), ("adaptive method 4", -1, [_N, "adaptive solver bosh3"]),
    ("adaptive method 5", -1, [_N, "adaptive solver fehlberg2"]), ("adaptive method 6", -1, [_N, "adaptive solver adaptive_heun"]),
    ("particles 2", -1, [_N, "particles = 2"]), ("fold_on", -1, [_N, "measured arms"]), ("ode_pack", -1, [_N, "measured arms"]),
    ("ode_alg", -1, [_N, "measured arms"]), ("obs NULL", -1, [_N, "batch->obs is NULL"]), ("padded strides", -1, [_N, "observation strides (266, 1, 3)"]),
    ("channel-major strides of another T", -1, [_N, "observation strides (258, 87, 1)"]), ("no_fold", -1, [_N, "SLODE_NO_FOLD"]),
    ("steps -1", -1, [_N, "num_steps = -1 < 0"]), ("lr 0", -1, [_N, "lr = 0", "finite positive"]), ("lr -0.05", -1, [_N, "lr = -0.05"]),
    ("lr inf", -1, [_N, "lr = inf"]), ("lr nan", -1, [_N, "lr = ", "nan"]),
    ("labels in the main loss", -1, [_N, "scores the labels", "proc", "label heads", "out of scope"]),
    ("LDS: T 1000", -1, [_N, "LDS tables", "T = 1000", "163840"]), ("LDS: num_draws 100000", -1, [_N, "LDS tables", "num_draws = 100000"]),
    ("LDS: num_draws 2^24", -1, [_N, "LDS tables", "num_draws = 16777216"]),
    ("label columns 3, n_u 2", -1, ["label tensors have 3 columns"]), ("n_labels 5", -1, ["n_labels out of range"]),
    ("label tensor 1 NULL", -1, ["label tensor 1 is NULL"]), ("workspace too small", -3, ["workspace 64 B < required"]),
    ("mask NULL, steps 0; workspace too small", -3, ["workspace 64 B < required"]),
    # two conditions at once: the earlier rung speaks
    ("params NULL + batch NULL", -1, ["params is NULL"]), ("times NULL + draws 0", -1, ["is NULL"]), ("draws 0 + adaptive", -1, ["num_draws = 0"]),
    ("adaptive + particles 2", -1, ["adaptive solver bosh3"]), ("particles 2 + fold_on", -1, ["particles = 2"]),
    ("ode_alg + obs NULL", -1, ["measured arms"]), ("no_fold + steps -1", -1, ["observation strides"]), ("steps -1 + lr nan", -1, ["num_steps = -1"]),
    ("lr 0 + labels in the main loss", -1, ["lr = 0"]), ("labels in the main loss + LDS", -1, ["scores the labels"]),
    ("LDS + label columns 3", -1, ["LDS tables"]), ("label columns 3 + workspace too small", -1, ["label tensors have 3 columns"]),
]


def test_refine_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_posterior_refine without a device, in rung order: status, the words of the message and the
    untouched drawing-call counter against LADDER; line by line against tests/golden/refine_refusals.txt; the shared rungs carry the texts
    tests/golden/eval_refusals.txt records for slode_traj_bounds, the call's name and its list of required pointers apart; and the memory
    that stands for the outputs untouched."""
    from tests.refusals_util import refusal_lines
    lines = refusal_lines("refine_refusals", tmp_path)
    assert lines[-1] == "memory that stands for the outputs | untouched"
    want = open(os.path.join(ROOT, "tests", "golden", "refine_refusals.txt")).read().splitlines()
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
            assert msg == bounds[name].replace("slode_traj_bounds", _N).replace("batch / bounds / ", "batch / loc_out / scale_out / elbo_out / "), \
                (name, msg, bounds[name])
    assert shared >= 25


@pytest.mark.parametrize("case", RU.CASES)
def test_weighted_loglik_at_unit_weights_is_the_oracle_loglik(case):
    c = RU.build(case, "midpoint")
    ospec, p = c["ospec"], {k: v.double() for k, v in c["p"].items()}
    obs, times = c["obs"].double(), c["times"].double()
    with torch.no_grad():
        loc, _ = O.encoder_conv(p, obs, ospec.pool_size)
        dec = (O.decoder_gauss if ospec.gauss else O.decoder_ald)(p, loc, times, ospec.solver)
        got = RU.weighted_loglik(ospec, dec, obs, torch.ones_like(obs))
        for b in range(c["B"]):
            row = tuple(t[b:b + 1] for t in dec[1:])
            want = O.gauss_loglik(obs[b:b + 1], *row) if ospec.gauss else O.ald_loglik_3q(obs[b:b + 1], *row, ospec.quantile_diff)
            assert abs(got[b].item() - want.item()) <= 1e-12 * abs(want.item()), (case, b)
        half = RU.weighted_loglik(ospec, dec, obs, RU.prefix_mask(c).double())
        assert torch.all(half != got)                                                     # the weights are not ignored


@pytest.mark.parametrize("case,solver,masked", [("cvs_ald", "rk4", False), ("cvs_gauss", "midpoint", True), ("challenge_ald", "euler", True),
                                                ("challenge_gauss", "rk4", False)])
def test_reference_gradient_against_finite_differences(case, solver, masked):
    """Central differences of the fp64 objective along a random direction per trajectory (step 1e-6; ALD is piecewise smooth: a kink
    crossed inside the step moves the quotient by the slope change times the step) against autograd: 1e-6 of |g| |d|."""
    c, w, r = RU.reference(case, solver, masked)
    loc, rho = RU.encoder(c)
    d = torch.randn(c["B"], 2 * loc.shape[1], generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    L, h = loc.shape[1], 1e-6
    with torch.no_grad():
        fp, _ = RU.objective(c, loc + h * d[:, :L], rho + h * d[:, L:], w=w)
        fm, _ = RU.objective(c, loc - h * d[:, :L], rho - h * d[:, L:], w=w)
    fd = ((fp - fm) / (2 * h)).numpy()
    gd = (r["grad0"] * d.numpy()).sum(1)
    err = np.abs(fd - gd) / (np.linalg.norm(r["grad0"], axis=1) * np.linalg.norm(d.numpy(), axis=1))
    print("%s/%s masked=%s: finite differences against autograd %.2e" % (case, solver, masked, err.max()))
    assert err.max() <= 1e-6


@pytest.mark.parametrize("case,solver,masked", CONFIGS)
def test_kernel_backward_formulas_equal_autograd(case, solver, masked):
    """The transcription of the formulas refine_kernel.hip executes (weighted likelihood gradient on the states, reverse scan,
    step_coeffs_bwd, a / d, hidden layer, init net, KL terms, the mean over the draws) against autograd through the oracle, fp64: 1e-10
    norm-wise per trajectory."""
    c, w, r = RU.reference(case, solver, masked)
    loc, rho = RU.encoder(c)
    err = RU.norm_err(RU.kernel_grad(c, loc.numpy(), rho.numpy(), w=w), r["grad0"])
    assert err.max() <= 1e-10, (case, solver, masked, err.max())


def test_every_condition_of_the_gpu_tests_holds_for_the_reference_alone():
    """Over CASES x SOLVERS x {no mask, prefix mask}, B = 5, K = 3, J = 4, lr = 0.05: the fp64 loop improves every trajectory strictly, by
    at least 2 % and by far more than the bar; the objective falls at every step (the best iterate is the last); the gradient norm has a floor
    (the norm-wise bar is meaningful); the fp32 loop stays within RHO bars of the fp64 loop (the measured figure is printed); Adam without
    bias correction -- a first step 3.16 x too long -- moves the trace by more than 600 bars."""
    rho_max, nobias_min = 0.0, np.inf
    for case, solver, masked in CONFIGS:
        c, w, r = RU.reference(case, solver, masked)
        bar = RU.REL * r["mag"]
        assert np.all(r["elbo"] < r["elbo0"] - bar) and np.all(r["elbo0"] - r["elbo"] >= 0.02 * np.abs(r["elbo0"])), (case, solver, masked)
        assert np.all(np.diff(r["trace"], axis=0) < 0) and np.all(r["best_step"] == RU.J)
        assert np.linalg.norm(r["grad0"], axis=1).min() >= 50.0
        r32 = RU.refine(c, w=w, dtype=torch.float32)
        rho_max = max(rho_max, (np.abs(r32["trace"] - r["trace"]) / bar).max())
        if solver == "rk4":
            wrong = RU.refine(c, w=w, bias_correction=False)
            nobias_min = min(nobias_min, (np.abs(wrong["trace"] - r["trace"]) / bar).max())
    print("fp32 loop against fp64 loop: largest trace deviation %.4f bar (RHO = %.2f); without bias correction: at least %.0f bars"
          % (rho_max, RU.RHO, nobias_min))
    assert rho_max <= RU.RHO and nobias_min > 600.0


def test_a_fully_masked_row_follows_the_kl_terms_alone():
    """Row 1 with every weight 0 (cvs_ald / midpoint): the reference gradient is the KL terms' alone -- g_loc = mean_k (z_k - pl) ips^2,
    g_rho = mean_k (z_k - pl) ips^2 scale eps_k - 1 -- and after the four steps its loc lies closer to the prior loc."""
    c = RU.build("cvs_ald", "midpoint")
    w = torch.ones_like(c["obs"])
    w[1] = 0.0
    r = RU.refine(c, w=w)
    loc, rho = RU.encoder(c)
    with torch.no_grad():
        ploc, pscale = O.prior_loc_scale({k: v.double() for k, v in c["p"].items()}, c["ospec"], c["u"].double())
    e = c["eps"].double()[:, 1]
    gz = ((loc[1] + rho[1].exp() * e - ploc[1]) / pscale[1] ** 2)
    want = torch.cat([gz.mean(0), (gz * rho[1].exp() * e).mean(0) - 1.0]).numpy()
    assert np.linalg.norm(r["grad0"][1] - want) <= 1e-12 * np.linalg.norm(want)
    assert np.linalg.norm(r["loc"][1] - ploc[1].numpy()) < np.linalg.norm(loc[1].numpy() - ploc[1].numpy())
