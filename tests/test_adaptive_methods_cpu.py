"""CPU checks of the adaptive Runge-Kutta tableaus (tests/adaptive_rk_ref.py) and of the method strings of the Python layer.  No GPU."""
import math

import pytest
import torch

from oracle import slode_oracle as O
from tests import adaptive_rk_ref as R

ALL = [R.DOPRI5, R.BOSH3, R.FEHLBERG2, R.ADAPTIVE_HEUN]


def test_dopri5_restatement_equals_the_oracle_bitwise():
    """With the DOPRI5 tableau the generic restatement is the committed oracle's per-trajectory solve, bit for bit in fp64 (cvs shape)."""
    ospec = O.cvs_spec(3, 3, 2, solver="dopri5")
    T, B = 60, 12
    p = O.init_params(ospec, T=T, S=5)
    g = torch.Generator().manual_seed(4)
    p = {k: (v + 0.05 * torch.randn(v.shape, generator=g)).double() for k, v in p.items()}
    _, _, _, times = O.synthetic_batch(ospec, 4, T)
    times = (times * 0.25).double()
    z = torch.randn(B, ospec.latent_dim, generator=g).double()
    want = O.solve_ode(p, z, times, "dopri5", rtol=1e-7, atol=1e-9, per_trajectory=True)
    with R.patched(R.DOPRI5):
        got = O.solve_ode(p, z, times, "dopri5", rtol=1e-7, atol=1e-9, per_trajectory=True)
    assert torch.equal(got, want)
    assert O.odeint_dopri5 is not None and O.odeint_dopri5.__name__ == "odeint_dopri5"   # restored


@pytest.mark.parametrize("tab", ALL, ids=lambda t: t.name)
def test_tableau_identities(tab):
    """Each beta row sums to its alpha, c_sol sums to 1, c_error to 0, c_mid's weights sum to 1/2 (y_mid = y(t + dt/2)), and the last
    stage is FSAL: time t + dt, beta row = c_sol (so k_last = f(t + dt, y1) is the next step's first stage)."""
    ns = len(tab.c_sol)
    assert len(tab.alpha) == len(tab.beta) == ns - 1 and len(tab.c_error) == len(tab.c_mid) == ns
    for a, row in zip(tab.alpha, tab.beta):
        assert math.isclose(sum(row), a, rel_tol=1e-12, abs_tol=1e-12), (tab.name, a, row)
    assert math.isclose(sum(tab.c_sol), 1.0, rel_tol=1e-12)
    assert abs(sum(tab.c_error)) < 1e-12
    assert math.isclose(sum(tab.c_mid), 0.5, rel_tol=1e-9)
    assert tab.alpha[-1] == 1.0
    last = list(tab.beta[-1]) + [0.0] * (ns - len(tab.beta[-1]))
    assert all(math.isclose(a, b, abs_tol=1e-15) for a, b in zip(last, tab.c_sol)), tab.name
    assert tab.c_sol[-1] == 0.0


# dx/dt = a(t) - d(t) x with a = 1 + sin t, d = 1 + 0.5 cos t: x(t) = exp(-D(t)) (x0 + int_0^t exp(D(s)) a(s) ds), D = t + 0.5 sin t; the
# integral in closed form is not needed -- a reference by the fixed-step dopri5 solution at a very small step is exact to 1e-15.
def _f(t, x):
    return (1.0 + torch.sin(t)) - (1.0 + 0.5 * torch.cos(t)) * x


def _fixed_step(tab, h, t_end=1.0, x0=0.3):
    t = torch.tensor(0.0, dtype=torch.float64)
    x = torch.tensor([x0], dtype=torch.float64)
    n = int(round(t_end / h))
    for _ in range(n):
        ks = [_f(t, x)]
        for a, row in zip(tab.alpha, tab.beta):
            ks.append(_f(t + a * h, x + h * sum(b * k for b, k in zip(row, ks))))
        x = x + h * sum(c * k for c, k in zip(tab.c_sol, ks))
        t = t + h
    return x


def _one_step_error(tab, h, t0=0.2, x0=0.3):
    """(embedded estimate h sum c_error k, true local error of the solution y1)"""
    t = torch.tensor(t0, dtype=torch.float64)
    x = torch.tensor([x0], dtype=torch.float64)
    ks = [_f(t, x)]
    for a, row in zip(tab.alpha, tab.beta):
        ks.append(_f(t + a * h, x + h * sum(b * k for b, k in zip(row, ks))))
    est = h * sum(c * k for c, k in zip(tab.c_error, ks))
    return est.abs().item()


def _slope(hs, errs):
    lh = [math.log(h) for h in hs]
    le = [math.log(e) for e in errs]
    n = len(hs)
    mh, me = sum(lh) / n, sum(le) / n
    return sum((a - mh) * (b - me) for a, b in zip(lh, le)) / sum((a - mh) ** 2 for a in lh)


@pytest.mark.parametrize("tab", ALL, ids=lambda t: t.name)
def test_orders(tab):
    """The fixed-step solution converges with the tableau's order p (global error ~ h^p), and the embedded error estimate of one step
    scales as h^p (the lower-order member's local error, h^(p_low + 1) = h^p): slopes within +-0.25 of p."""
    ref = _fixed_step(R.DOPRI5, 1.0 / 4096)
    hs = [1 / 8, 1 / 16, 1 / 32, 1 / 64] if tab.order >= 4 else [1 / 16, 1 / 32, 1 / 64, 1 / 128]
    errs = [(_fixed_step(tab, h) - ref).abs().item() for h in hs]
    s = _slope(hs, errs)
    assert abs(s - tab.order) <= 0.25, (tab.name, s, errs)
    hs = [0.2, 0.1, 0.05, 0.025]
    ests = [_one_step_error(tab, h) for h in hs]
    s = _slope(hs, ests)
    assert abs(s - tab.order) <= 0.25, (tab.name, "embedded estimate", s, ests)


def test_method_strings():
    """The Python layer maps torchdiffeq's method strings to slode_method (include/slode.h) and treats the four adaptive ones alike."""
    from structured_latent_odes_amd import _lib as L
    assert L.METHODS["bosh3"] == 4 and L.METHODS["fehlberg2"] == 5 and L.METHODS["adaptive_heun"] == 6
    assert L.METHODS["dopri5"] == 3
    assert set(L.ADAPTIVE) == {"dopri5", "bosh3", "fehlberg2", "adaptive_heun"}
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/slode.h").read()
    for name, v in (("SLODE_BOSH3", 4), ("SLODE_FEHLBERG2", 5), ("SLODE_ADAPTIVE_HEUN", 6)):
        assert "%s = %d" % (name, v) in hdr
