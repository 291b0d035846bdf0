"""CPU tests of csrc/fixed_step.h, the one definition of a fixed-grid step's arithmetic that the training kernel (ode_kernel.hip), the
refinement kernel (refine_kernel.hip) and the eval-side forward (slode_forward.h) execute: every routine compiled for the host
(tests/fixed_step/fixed_step.cpp) and run on the same 60 random steps per method in fp32 -- h in (0.05, 0.5), stage values a, d in (0, 1),
incoming gradients ~ N(0, 1) -- against tests/kernel_math.py and the oracle in fp64.  Every bound is 1e-5 of the largest value the step
yields (fp32 rounding of a few dozen operations); the two shapes of the forward coefficients are held equal bit for bit."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import slode_oracle as O
from tests import kernel_math as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("euler", "midpoint", "rk4")
NST = {"euler": 1, "midpoint": 2, "rk4": 4}                                                # evaluations of one step
BOUND = 1e-5


def _steps():
    """(method, [h, a0 .. a3, d0 .. d3, g0, g1]) of the 180 steps, as float32 values held in fp64"""
    rng = np.random.default_rng(5)
    rows = []
    for method in METHODS:
        for _ in range(60):
            v = np.concatenate([[rng.uniform(0.05, 0.5)], rng.uniform(0.02, 0.98, 8), rng.normal(size=2)]).astype(np.float32)
            rows.append((method, v.astype(np.float64)))
    return rows


ROWS = _steps()


def _f(v):
    return " ".join("%.9g" % x for x in v)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the host program, built once: request lines in, one list of words per output line out"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present: the host program is not built")
    exe = str(tmp_path_factory.mktemp("fixed_step") / "fixed_step")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-O1", os.path.join(ROOT, "tests", "fixed_step", "fixed_step.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]

    def go(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return go


def test_stage_counts_of_the_header(run):
    got = run(["counts %d" % mi for mi in range(3)])
    assert [[int(x) for x in g] for g in got] == [[KM.stage_layout(m), NST[m]] for m in METHODS]


def test_reverse_step_routine_of_the_kernel_matches_step_coeffs_bwd(run):
    """step_bwd, the one reverse step routine of the training and the refinement kernel, against tests/kernel_math.py::step_coeffs_bwd in
    fp64: within 1e-5 of the largest stage gradient of the step, and exactly 0 in the stages the method does not have."""
    got = np.array(run(["bwd %d %s" % (METHODS.index(m), _f(v)) for m, v in ROWS]), dtype=np.float64)
    assert got.shape == (180, 8)
    worst = 0.0
    for (method, v), g in zip(ROWS, got):
        h, a, d, gA, gb = v[0], v[1:5].reshape(4, 1), v[5:9].reshape(4, 1), v[9:10], v[10:11]
        _, _, cache = KM.step_coeffs(method, h, a, d)
        ga, gd = KM.step_coeffs_bwd(method, h, a, d, cache, gA, gb)
        want = np.concatenate([ga[:, 0], gd[:, 0]])
        nst = NST[method]
        assert np.all(g[nst:4] == 0.0) and np.all(g[4 + nst:] == 0.0) and np.all(want[nst:4] == 0.0)
        worst = max(worst, np.abs(g - want).max() / np.abs(want).max())
    print("step_bwd against step_coeffs_bwd: worst error / largest stage gradient %.2e" % worst)
    assert worst <= BOUND


def test_step_fwd_matches_step_coeffs(run):
    """step_fwd against tests/kernel_math.py::step_coeffs in fp64: A and b within 1e-5 of the larger of the two."""
    got = np.array(run(["fwd %d %s" % (METHODS.index(m), _f(v[:9])) for m, v in ROWS]), dtype=np.float64)
    assert got.shape == (180, 2)
    worst = 0.0
    for (method, v), g in zip(ROWS, got):
        A, b, _ = KM.step_coeffs(method, v[0], v[1:5].reshape(4, 1), v[5:9].reshape(4, 1))
        want = np.array([A[0], b[0]])
        worst = max(worst, np.abs(g - want).max() / np.abs(want).max())
    print("step_fwd against step_coeffs: worst error / largest coefficient %.2e" % worst)
    assert worst <= BOUND


@pytest.mark.parametrize("sm", [5, 8])
def test_fwd_step_coeffs_equals_step_fwd_bit_for_bit(run, sm):
    """fwd_step_coeffs<SM> (all components, stage by stage, around an evaluator: the eval-side shape) and step_fwd (one component from its
    four stage values: the training kernel's shape) are the same arithmetic: step i with the stage values of the steps i .. i + SM - 1 of
    its method as its SM components, every coefficient of every component the same bits."""
    lines = []
    for mi in range(3):
        rows = [v for _, v in ROWS[60 * mi:60 * mi + 60]]
        for i in range(60):
            lines.append("coeffs %d %d %s " % (sm, mi, _f(rows[i][:1])) + " ".join(_f(rows[(i + s) % 60][1:9]) for s in range(sm)))
    got = run(lines)
    for i, g in enumerate(got):
        assert len(g) == 4 * sm and all(len(w) == 8 for w in g)
        assert g[:2 * sm] == g[2 * sm:], (METHODS[i // 60], i % 60, g)
    assert len({w for g in got for w in g}) > 180 * sm                                    # (the coefficients are not all one value)


def test_radj_M_is_the_step_coefficient_of_the_adjoint_equation(run):
    """The adjoint obeys lam' = +d lam: radj_M(method, hb, D) is A of step_coeffs(method, hb, a = 0, d = -D), fp64, within 1e-5 of it."""
    got = np.array(run(["radj %d %s" % (METHODS.index(m), _f(np.concatenate([[-v[0]], v[1:]]))) for m, v in ROWS]), dtype=np.float64)
    assert got.shape == (180, 9)
    worst = 0.0
    for (method, v), g in zip(ROWS, got):
        A, _, _ = KM.step_coeffs(method, -v[0], np.zeros((4, 1)), -v[5:9].reshape(4, 1))
        worst = max(worst, abs(g[0] - A[0]) / abs(A[0]))
    print("radj_M against step_coeffs: worst relative error %.2e" % worst)
    assert worst <= BOUND


def test_radj_routines_match_the_oracle_adjoint(run):
    """radj_M and radj_stage_grads against oracle/slode_oracle.py::_OdeintAdjoint in fp64 on one step t0 -> t1 = t0 + h of a scalar state
    under f(t, y) = a_j - d_j y, j the stage whose time t hits: the backward step evaluates f at t1 and at the forward stage times in reverse
    order (the stage times of these methods coincide in both directions), so a table of the backward stages j = 0 .. 3 is a valid f; the
    forward pass of euler and midpoint also reads f at t0, an entry of its own that the backward pass never reads.  The oracle's gradient
    to a_j, d_j is gaq[j], gdq[j] (no sigmoid stands between), its gradient to y0 over the incoming lam is radj_M; y is the oracle's
    y[1].  Within 1e-5 of the largest stage gradient of the step, resp. of M; exactly 0 in the stages the method lacks."""
    reqs, wants = [], []
    for method, v in ROWS:
        h, a, d, y0, lam = v[0], v[1:5], v[5:9], v[9], v[10]
        t0 = 0.25
        back = {"euler": [t0 + h], "midpoint": [t0 + h, t0 + 0.5 * h], "rk4": [t0 + h, t0 + h * 2.0 / 3.0, t0 + h / 3.0, t0]}[method]
        nb = len(back)
        tab_t = torch.tensor(back + ([] if method == "rk4" else [t0]), dtype=torch.float64)
        pa = torch.tensor(a[:len(tab_t)], dtype=torch.float64, requires_grad=True)
        pd = torch.tensor(d[:len(tab_t)], dtype=torch.float64, requires_grad=True)

        def fb(params):
            def f(t, y):
                j = int(torch.argmin((tab_t - t).abs()))
                assert abs(float(tab_t[j] - t)) <= 1e-12
                return params[0][j] - params[1][j] * y
            return f
        y_init = torch.tensor([y0], dtype=torch.float64, requires_grad=True)
        y = O._OdeintAdjoint.apply(fb, y_init, torch.tensor([t0, t0 + h], dtype=torch.float64), method, pa, pd)
        (lam * y[1]).sum().backward()
        gaq, gdq = np.zeros(4), np.zeros(4)
        gaq[:nb], gdq[:nb] = pa.grad.numpy()[:nb], pd.grad.numpy()[:nb]
        assert np.all(pa.grad.numpy()[nb:] == 0.0) and np.all(pd.grad.numpy()[nb:] == 0.0)
        A4, D4 = np.zeros(4), np.zeros(4)
        A4[:nb], D4[:nb] = a[:nb], d[:nb]
        reqs.append("radj %d %s" % (METHODS.index(method), _f(np.concatenate([[-h], A4, D4, [lam, y[1].item()]]))))
        wants.append((nb, y_init.grad.item() / lam, np.concatenate([gaq, gdq])))
    got = np.array(run(reqs), dtype=np.float64)
    assert got.shape == (180, 9)
    worst_m, worst_g = 0.0, 0.0
    for g, (nb, M, want) in zip(got, wants):
        assert np.all(g[1 + nb:5] == 0.0) and np.all(g[5 + nb:] == 0.0)
        worst_m = max(worst_m, abs(g[0] - M) / abs(M))
        worst_g = max(worst_g, np.abs(g[1:] - want).max() / np.abs(want).max())
    print("against _OdeintAdjoint: radj_M worst relative error %.2e; radj_stage_grads worst error / largest stage gradient %.2e" % (worst_m, worst_g))
    assert worst_m <= BOUND and worst_g <= BOUND
