"""Test infrastructure of the mechanism curves (slode_mechanism_moments): the fp64 oracle's five quantities per draw -- composed from
oracle/slode_oracle.py: encoder_conv / prior_loc_scale for the source of the draws, solve_ode for the states, the growth and degradation
sigmoids read from the same parameters as O.dynamics for a and d -- their np.mean / np.std over the draws, the per-slot bars and the check
against them.  Not imported by the product.

Slots: 0 state x_i[s], 1 production a_s(t_i, z), 2 degradation d_s(t_i, z), 3 set_point a / d, 4 net_rate a - d x; arrays [5, B, S, T].

The cases, and the condition on them.  The set point a / d is finite and its bar meaningful only where d stays away from 0: the oracle's
smallest d over all draws, times and states must be at least MIN_D = 1e-3 (`min_degradation`; tests/test_mechanism_cpu.py asserts it on the
oracle alone for every case a set point is compared on, `condition_table`).  The cases of tests/recon_moments_util.build do not meet it as
they are built, and none of the seeds behind them can make them: their grids run to t = 19 .. 299 at parameters drawn for t of order 1,
and the untrained prior nets of proc turn log-concentration labels of 7 .. 10 into prior scales of up to 517, so the degradation sigmoid
saturates whatever the noise (table below, right column).  The set point is therefore compared on `build`: RU.build's case -- the same
parameters, observations, noise, B, T, S, solver -- with two inputs changed, `conditioned`: the time grid compressed to [0, SPAN = 1] and,
for proc, the two log-concentration label columns multiplied by PROC_CONC = 0.1.  The four bounded slots are ALSO compared on RU.build's
cases as they are, so nothing the unconditioned cases can check is lost.  The oracle's smallest d at rk4, ns = 7:

    case              conditioned, posterior / prior     as built, posterior / prior
    cvs_ald           3.2e-2 / 4.8e-3                    5.7e-9  / 2.1e-9
    cvs_gauss         1.5e-2 / 2.2e-2                    4.5e-8  / 5.0e-8
    challenge_ald     1.1e-2 / 4.4e-3                    1.6e-23 / 3.1e-24
    challenge_gauss   7.6e-2 / 4.2e-2                    1.7e-18 / 3.9e-19
    proc_ald          3.2e-3 / 9.8e-3                    1.6e-5  / 7.5e-140
    proc_gauss        7.3e-3 / 8.3e-3                    1.4e-3  / 6.2e-14

and 1.5e-3 at the least over all 40 conditioned cases of the tests (those six, `SIZES`, `grid_case` at T in GRID_T; both sides).

Bars, x max(1, |oracle mean|).  By the project's rule (tests/test_gpu_eval_side.py, the table above BAR) a slot's bar is the suite's bar of
the same kind of value -- RU.MEAN_BAR for a mean and RU.SD_BAR for an sd of bounded curve inputs -- unless 4 x the worst distance of the fp32
CPU oracle (this module's composition on fp32 tensors) from the fp64 oracle, scaled the same way, exceeds it; the slot then takes the larger
figure.  Measured on every case of EU.CASES x EU.SOLVERS, ns = 7, both sides, conditioned (all five slots) and as built (the bounded four)
(`fp32_distances`; tests/test_mechanism_cpu.py runs it and asserts that the fp32 oracle stays within a quarter of every bar):

    slot          fp32-vs-fp64 worst, mean / sd    4 x                     bar (mean, sd)
    state         3.73e-6 / 9.06e-6                1.49e-5 / 3.63e-5       1e-4, 2e-4 (RU's)
    production    3.86e-7 / 4.18e-7                1.54e-6 / 1.67e-6       1e-4, 2e-4 (RU's)
    degradation   1.20e-6 / 1.45e-6                4.82e-6 / 5.81e-6       1e-4, 2e-4 (RU's)
    set_point     2.07e-6 / 4.80e-6                8.27e-6 / 1.92e-5       1e-4, 2e-4 (RU's)
    net_rate      1.28e-6 / 2.06e-6                5.12e-6 / 8.23e-6       1e-4, 2e-4 (RU's)

No bar comes from the kernel's output."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import slode_oracle as O
from tests import eval_stats_util as EU
from tests import lds_util as LU
from tests import recon_moments_util as RU

NAMES = ("state", "production", "degradation", "set_point", "net_rate")
SLOTS = len(NAMES)
ALL = (1 << SLOTS) - 1
MIN_D = 1e-3
_ODE = "decoder.ode_model."
# (mean bar, sd bar) per slot: RU's, or 4 x the fp32 oracle's measured distance where that is larger (module docstring)
BARS = {n: (RU.MEAN_BAR, RU.SD_BAR) for n in NAMES}


def production_degradation(p, z, times):
    """a, d [N, T, S] at every grid time: the hidden layer on cat([t, z]), ReLU, the growth and the degradation sigmoid -- the parameters
    and the arithmetic of O.dynamics, all grid times at once."""
    N, T = z.shape[0], times.numel()
    x = torch.cat([times.reshape(1, T, 1).expand(N, T, 1), z.unsqueeze(1).expand(N, T, z.shape[1])], dim=2)
    h = torch.relu(F.linear(x, p[_ODE + "dynamics.dynamics_hidden.weight"], p[_ODE + "dynamics.dynamics_hidden.bias"]))
    a = torch.sigmoid(F.linear(h, p[_ODE + "dynamics.dyanamics_growth.weight"], p[_ODE + "dynamics.dyanamics_growth.bias"]))
    d = torch.sigmoid(F.linear(h, p[_ODE + "dynamics.dyanmics_degradation.weight"], p[_ODE + "dynamics.dyanmics_degradation.bias"]))
    return a, d


def oracle_draws(c, is_post, eps=None, dtype=torch.float64):
    """The five quantities of every draw, [5, ns, B, S, T] (numpy, ``dtype``): z = loc + scale * eps_k, the oracle's solve and a, d."""
    ospec = c["ospec"]
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    obs, u, times = c["obs"].to(dtype), c["u"].to(dtype), c["times"].to(dtype)
    e = (c["eps"] if eps is None else eps).to(dtype)
    ns, B, L = e.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p, obs, ospec.pool_size) if is_post else O.prior_loc_scale(p, ospec, u)
        z = (loc.unsqueeze(0) + scale.unsqueeze(0) * e).reshape(ns * B, L)
        x = O.solve_ode(p, z, times, ospec.solver)                       # [N, T, S]
        a, d = production_degradation(p, z, times)
        v = torch.stack([x, a, d, a / d, a - d * x])                     # [5, N, T, S]
    return v.reshape(SLOTS, ns, B, v.shape[2], v.shape[3]).permute(0, 1, 2, 4, 3).contiguous().numpy()


def moments(draws):
    """(mean, sd) [5, B, S, T]: np.mean / np.std (population) over the draw axis of ``oracle_draws``' array."""
    return np.mean(draws, 1), np.std(draws, 1)


SPAN = 1.0          # the conditioned cases' grids end here: times x SPAN / times[-1]
PROC_CONC = 0.1     # and the two log-concentration labels of proc (columns 7, 8, about 7 .. 10) are multiplied by this
# (case, B, ns, environment) of the GPU test "sizes and instantiations": B in {1, 3, 65}, 2 and 5 workgroups, T in {86, 100, 200, 300},
# S = 5, 8 and the run-time-S build, ns in {1, 2, 7} and one ns = 200
SIZES = [("cvs_gauss", 1, 2, {}), ("cvs_gauss", 65, 7, {}), ("cvs_ald", 3, 200, {}), ("cvs_ald", 3, 7, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"}),
         ("proc_gauss", 65, 2, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}), ("challenge_gauss", 65, 1, {"SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "5"}),
         ("challenge_gauss", 3, 7, {}), ("cvs_ald", 3, 7, {"SLODE_ODE_GENERIC": "1"}),
         ("proc_ald", 3, 2, {"SLODE_ODE_GENERIC": "1", "SLODE_ODE_LOOP": "1", "SLODE_ODE_GRID": "2"})]
GRID_T = (2, 3, 257)


def conditioned(c):
    """The case ``c`` with the two inputs changed that keep its degradation away from 0 (module docstring): the time grid compressed to
    [0, SPAN] and, for proc, the two log-concentration label columns multiplied by PROC_CONC.  Parameters, observations, the other labels,
    noise, B, T, S and the solver are those of ``c``."""
    u = c["u"].clone()
    if c["fam"] == "proc":
        u[:, 7:] *= PROC_CONC
    return dict(c, times=(c["times"] * (SPAN / float(c["times"][-1]))).contiguous(), u=u)


def build(case, solver="rk4", B=None, ns=7):
    """RU.build's case, conditioned."""
    return conditioned(RU.build(case, solver, B=B, ns=ns))


def grid_case(fam, T, B=3, ns=2, solver="rk4"):
    """A conditioned Gaussian case of any grid length T >= 2: EU.build_case's recipe (reference initialisers, every tensor moved by 0.05
    randn of seed 11, the synthetic batch of seed 7, RU's noise seed) with filter_size = pool_size = 1, which no T is too short for."""
    kw = EU.CASES[fam + "_gauss"][1]
    ospec = {"cvs": O.cvs_spec, "proc": O.proc_spec}[fam](solver=solver, pool_size=1, **kw)
    S = 8 if fam == "proc" else 5
    g = torch.Generator().manual_seed(11)
    p = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in O.init_params(ospec, T=T, S=S, K=1).items()}
    obs, u, _, times = O.synthetic_batch(ospec, B, T, seed=7)
    eps = torch.randn(ns, B, ospec.latent_dim, generator=torch.Generator().manual_seed(RU.NOISE_SEED + ns))
    return conditioned(dict(fam=fam, kw=dict(kw, solver=solver), ospec=ospec, p=p, obs=obs, u=u, times=times, B=B, T=T, S=S, eps=eps, ns=ns))


@functools.lru_cache(maxsize=None)
def reference(case, solver="rk4", B=None, ns=7, is_post=True, as_built=False):
    """The fp64 oracle's (mean, sd, smallest d) of build(case, solver, B, ns) -- ``as_built``: of RU.build's case as it is -- on its own
    noise: computed once, shared, not to be changed."""
    dr = oracle_draws((RU.build if as_built else build)(case, solver, B, ns), is_post)
    mean, sd = moments(dr)
    for a in (mean, sd):
        a.setflags(write=False)
    return mean, sd, float(dr[2].min())


def min_degradation(draws):
    return float(draws[2].min())


def ratios(mean, sd, want_mean, want_sd, slots=ALL):
    """{name: (mean error / bar, sd error / bar)} of the selected slots: ``mean`` / ``sd`` [n_sel, B, S, T] in increasing slot order
    against the matching rows of the oracle's [5, B, S, T]."""
    out = {}
    sel = [q for q in range(SLOTS) if (slots >> q) & 1]
    for j, q in enumerate(sel):
        scale = np.maximum(1.0, np.abs(want_mean[q]))
        mb, sb = BARS[NAMES[q]]
        out[NAMES[q]] = (float((np.abs(mean[j] - want_mean[q]) / (mb * scale)).max()), float((np.abs(sd[j] - want_sd[q]) / (sb * scale)).max()))
    return out


def check(mean, sd, want_mean, want_sd, tag, slots=ALL, factor=1.0):
    """Prints the worst ratios error / bar per slot, then asserts finiteness and every bar (``factor`` x the bar)."""
    m = mean.detach().double().cpu().numpy() if torch.is_tensor(mean) else np.asarray(mean, dtype=np.float64)
    s = sd.detach().double().cpu().numpy() if torch.is_tensor(sd) else np.asarray(sd, dtype=np.float64)
    r = ratios(m, s, want_mean, want_sd, slots)
    print("%s: error / bar  %s" % (tag, "  ".join("%s mean %.3e sd %.3e" % ((n,) + r[n]) for n in r)))
    assert np.isfinite(m).all() and np.isfinite(s).all(), tag
    for n, (rm, rs) in r.items():
        assert rm <= factor, (tag, n, "mean", rm)
        assert rs <= factor, (tag, n, "sd", rs)


def fp32_distances(cases=None, solvers=None, ns=7):
    """({name: (worst scaled mean distance, worst scaled sd distance)} of the fp32 CPU oracle from the fp64 oracle, both sides, every case x
    solver: all five slots on the conditioned cases and the four bounded slots on RU.build's cases as they are; {(case, side): smallest d
    of the conditioned case, of the case as built} at rk4): what the bars and the tables of the module docstring come from."""
    worst = {n: [0.0, 0.0] for n in NAMES}
    cond = {}
    for case in (cases or EU.CASES):
        for solver in (solvers or EU.SOLVERS):
            for as_built in (False, True):
                c = (RU.build if as_built else build)(case, solver, ns=ns)
                for is_post in (True, False):
                    d64 = oracle_draws(c, is_post)
                    if solver == "rk4":
                        cond.setdefault((case, "post" if is_post else "prior"), []).append(min_degradation(d64))
                    m64, s64 = moments(d64)
                    with np.errstate(all="ignore"):
                        m32, s32 = moments(oracle_draws(c, is_post, dtype=torch.float32).astype(np.float64))
                    for q, n in enumerate(NAMES):
                        if as_built and n == "set_point":
                            continue
                        scale = np.maximum(1.0, np.abs(m64[q]))
                        worst[n][0] = max(worst[n][0], float((np.abs(m32[q] - m64[q]) / scale).max()))
                        worst[n][1] = max(worst[n][1], float((np.abs(s32[q] - s64[q]) / scale).max()))
    return {n: tuple(v) for n, v in worst.items()}, {k: tuple(v) for k, v in cond.items()}


def condition_table():
    """{tag: the oracle's smallest d} of every conditioned case the tests compare a set point on: EU.CASES at ns = 7, SIZES, the grid cases;
    both sides (a, d at the grid times do not depend on the solver)."""
    out = {}
    for is_post in (True, False):
        side = "post" if is_post else "prior"
        for case in EU.CASES:
            out["%s %s" % (case, side)] = min_degradation(oracle_draws(build(case, "rk4"), is_post))
        for case, B, ns, _ in SIZES:
            out["%s B=%d ns=%d %s" % (case, B, ns, side)] = min_degradation(oracle_draws(build(case, "rk4", B, ns), is_post))
        for fam in ("cvs", "proc"):
            for T in GRID_T:
                out["%s T=%d %s" % (fam, T, side)] = min_degradation(oracle_draws(grid_case(fam, T), is_post))
    return out


# ---- the numpy restatement of the kernel's per-draw slots on given fp32 state, a, d ---------------------------------------------------
def set_point_f32(a, d):
    return RU._f32(RU._f32(a) / RU._f32(d))


def net_rate_f32(a, d, x):
    return RU._fma32(-RU._f32(d), RU._f32(x), RU._f32(a))


def plan_bytes(T, S, C, L, H, n_u, gauss, n_sel):
    """The hand count of the kernel's LDS tables in bytes, every piece rounded to 16 B: the shared pieces (step table 2 (T - 1) S, the
    H rows of 2 + 2 S floats rounded to four, w1 2 H L, b1 2 H, w2 H S + S, head weights Q C S, biases 2 S, z L, labels max(n_u, 1), h0 H,
    x0 S), the moment table n_sel r4(3 S T), loc | scale, the capture table 2 T S."""
    r4 = LU.r4
    return 4 * (LU.fwd_shared_floats(T, S, C, L, H, n_u, gauss) + n_sel * r4(3 * S * T) + 2 * r4(L) + r4(2 * T * S))
