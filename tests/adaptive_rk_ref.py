"""fp64 restatement of the per-trajectory adaptive Runge-Kutta solver for any of torchdiffeq's RKAdaptiveStepsizeODESolver tableaus
(test infrastructure).  Same structure and arithmetic as oracle.slode_oracle.odeint_dopri5(per_trajectory=True) -- FSAL, error ratio
rms(err / (atol + rtol max(|y0|, |y1|))), factor clamp [0.2, 10] with safety 0.9, Hairer initial step, quartic dense output through
(y0, y_mid, y1, f0, f1) -- with the tableau and the order p (exponent 1/p in the controller and the initial step) as parameters.

The tableaus restate torchdiffeq/_impl/dopri5.py, bosh3.py, fehlberg2.py and adaptive_heun.py (0.2.x); no fixture pins them, the
CPU tests check their identities and orders instead.  GPU tests reach the oracle's ELBO with one of these by patching
slode_oracle.odeint_dopri5 (see `patched`)."""
import contextlib
from dataclasses import dataclass
from typing import List

import torch

from oracle import slode_oracle as O


@dataclass(frozen=True)
class Tableau:
    name: str
    order: int
    alpha: List[float]        # stage times of stages 2 .. NS (fractions of dt)
    beta: List[List[float]]   # rows of stages 2 .. NS
    c_sol: List[float]
    c_error: List[float]
    c_mid: List[float]


DOPRI5 = Tableau("dopri5", 5, O._DP_ALPHA, O._DP_BETA, O._DP_CSOL, O._DP_CERR, O._DP_CMID)
BOSH3 = Tableau("bosh3", 3, [1 / 2, 3 / 4, 1.0], [[1 / 2], [0.0, 3 / 4], [2 / 9, 1 / 3, 4 / 9]],
                [2 / 9, 1 / 3, 4 / 9, 0.0], [2 / 9 - 7 / 24, 1 / 3 - 1 / 4, 4 / 9 - 1 / 3, -1 / 8], [0.0, 0.5, 0.0, 0.0])
FEHLBERG2 = Tableau("fehlberg2", 2, [1 / 2, 1.0, 1.0], [[1 / 2], [1 / 256, 255 / 256], [1 / 512, 255 / 256, 1 / 512]],
                    [1 / 512, 255 / 256, 1 / 512, 0.0], [-1 / 512, 0.0, 1 / 512, 0.0], [0.0, 0.5, 0.0, 0.0])
ADAPTIVE_HEUN = Tableau("adaptive_heun", 2, [1.0, 1.0], [[1.0], [1 / 2, 1 / 2]],
                        [1 / 2, 1 / 2, 0.0], [1 / 2, -1 / 2, 0.0], [1 / 2, 0.0, 0.0])
TABLEAUS = {t.name: t for t in (DOPRI5, BOSH3, FEHLBERG2, ADAPTIVE_HEUN)}


def odeint_rk(f, y0, times, tab: Tableau, rtol=1e-7, atol=1e-9, max_steps=100000, counts=None):
    """Per-trajectory adaptive solve of dy/dt = f(t, y) with tableau `tab`; f takes a [B,1] time column.  -> [T, B, S].  counts (a
    list, optional) receives the accepted steps per trajectory ([B] int tensor)."""
    dtype = y0.dtype

    def norm(x):
        return x.pow(2).mean(dim=1).sqrt()

    def bc(v):
        return v.reshape(-1, 1)

    def fr(t, y):
        return f(t.reshape(-1, 1), y)

    rp = 1.0 / tab.order
    t0 = times[0].to(dtype)
    f0 = f(t0, y0)
    scale = atol + y0.abs() * rtol
    d0, d1 = norm(y0 / scale), norm(f0 / scale)
    h0 = torch.where((d0 < 1e-5) | (d1 < 1e-5), torch.full_like(d0, 1e-6), 0.01 * d0 / d1)
    y1 = y0 + bc(h0) * f0
    f1 = fr(t0 + h0, y1)
    d2 = norm((f1 - f0) / scale) / h0
    h1 = torch.where((d1 <= 1e-15) & (d2 <= 1e-15), torch.maximum(torch.full_like(h0, 1e-6), h0 * 1e-3),
                     (0.01 / torch.maximum(d1, d2)) ** rp)
    dt = torch.minimum(100 * h0, h1).detach()
    t = t0.expand(dt.shape[0]).clone()
    y, fy = y0.clone(), f0.clone()
    out = [y0]
    t_prev = t.clone()
    y_prev, y_mid, f_prev = y.clone(), y.clone(), fy.clone()
    nacc = torch.zeros(dt.shape[0], dtype=torch.int64)
    for j in range(1, times.shape[0]):
        tj = times[j].to(dtype)
        steps = 0
        while bool((t < tj).any()):
            steps += 1
            if steps > max_steps:
                raise RuntimeError("%s: max_steps exceeded" % tab.name)
            active = t < tj
            ks = [fy]
            for a, brow in zip(tab.alpha, tab.beta):
                yi = y + bc(dt) * sum(b * k for b, k in zip(brow, ks))
                ti = t + a * dt if a != 1.0 else t + dt
                ks.append(fr(ti, yi))
            y_new = y + bc(dt) * sum(c * k for c, k in zip(tab.c_sol, ks))
            err = bc(dt) * sum(c * k for c, k in zip(tab.c_error, ks))
            tol = atol + rtol * torch.maximum(y.abs(), y_new.abs())
            ratio = norm(err / tol)
            accept = (ratio <= 1) & active
            ymid_new = y + bc(dt) * sum(c * k for c, k in zip(tab.c_mid, ks))
            acc = bc(accept)
            nacc += accept.long()
            t_prev = torch.where(accept, t, t_prev)
            y_prev = torch.where(acc, y, y_prev)
            y_mid = torch.where(acc, ymid_new, y_mid)
            f_prev = torch.where(acc, fy, f_prev)
            t = torch.where(accept, t + dt, t)
            y = torch.where(acc, y_new, y)
            fy = torch.where(acc, ks[-1], fy)
            safe = torch.where(ratio == 0, torch.full_like(ratio, 10.0), 0.9 * ratio.clamp_min(1e-300) ** (-rp))
            factor = torch.where(ratio < 1, safe.clamp(1.0, 10.0), safe.clamp(0.2, 10.0))
            factor = torch.where(ratio == 0, torch.full_like(ratio, 10.0), factor)
            dt = torch.where(active, dt * factor, dt).detach()
        out.append(O._dopri5_interp(bc(t_prev), bc(t), y_prev, y_mid, y, f_prev, fy, tj))
    if counts is not None:
        counts.append(nacc)
    return torch.stack(out, dim=0)


def solver_for(tab: Tableau, counts=None):
    """A stand-in for slode_oracle.odeint_dopri5 (same signature; per_trajectory must be True) that runs `tab`."""
    def odeint(f, y0, times, rtol=1e-7, atol=1e-9, per_trajectory=False, max_steps=100000):
        assert per_trajectory, "the restatement is per trajectory"
        return odeint_rk(f, y0, times, tab, rtol=rtol, atol=atol, max_steps=max_steps, counts=counts)
    return odeint


@contextlib.contextmanager
def patched(tab: Tableau, counts=None):
    """Within the block the oracle's adaptive solve (solve_ode with method "dopri5") runs `tab`."""
    orig = O.odeint_dopri5
    O.odeint_dopri5 = solver_for(tab, counts)
    try:
        yield
    finally:
        O.odeint_dopri5 = orig
