"""The regimes of tests/regime_util.py do what they claim, on the oracle alone: every case the GPU tests of tests/test_gpu_regimes.py run is
finite in fp64 and in fp32, reaches the range its regime is for, keeps clear_of_kinks under 1 % of its elements, and leaves the fp32 CPU
oracle within a quarter of every bar the GPU tests hold the kernels to.  The rows these tests print are the table of regime_util's docstring;
a library update that moves it fails here, before it moves a GPU bar.  No GPU."""
import math

import pytest
import torch

from tests import eval_stats_util as EU
from tests import regime_util as G
from tests import traj_bounds_util as TU
from tests.test_gpu_instantiations import SHAPES

B, EB, EK = 12, 4, 3
# (shape, regime, loss) whose bars the rule raises above the suite's, with a ceiling of about 3 x the largest bar measured (the table of
# tests/regime_util.py).  c0, auxiliary loss: the gradients of encoder.z_loc.* at posterior scales of 1e-3, where d/d loc of
# log N(loc + scale eps; loc, scale) cancels to zero between terms of size 1 / scale (bars 1.7e-3, 2.6e-3).  c4 fitted: a Gauss likelihood
# with scales down to 1e-3 fitted to curves that reach 300 -- one fp32 ulp of the curve is 3e-5, a thirtieth of the scale (bar 1.8e-2,
# decoder.ode_model.latent_to_ode_net.2.bias; the loss stays 1.7e-6 from fp64).
RAISED = {("c0_cvs_T100_L4_rk4", "posterior_scales", "aux"): 5e-3, ("c0_cvs_T100_L4_rk4", "all", "aux"): 8e-3,
          ("c4_challenge_gauss_T300_L15_rk4", "fitted", "main"): 5e-2}
LOSS_CEILING = 2e-5         # the largest fp32 loss distance is 1.7e-6 (c4 fitted): a raised loss bar would have to stay under this
# the fp32 oracle's worst per-row distance / the suite's per-row bar 1e-5 x mag over the bounds cases: at most 1.31 (challenge_gauss at
# trained_weights and all), except the fitted Gauss rows (cvs_gauss 7.7, challenge_gauss 34: the conditioning of c4 fitted above, per row)
BOUNDS_CEILING = {"fitted": 100.0}
_cache = {}


def _shape(shape, regime):
    if (shape, regime) not in _cache:
        fam, kw, T = SHAPES[shape]
        c = G.apply(regime, G.shape_case(fam, kw, T, B))
        _cache[shape, regime] = (c, G.Oracles(c, "main"), G.Oracles(c, "aux"))
    return _cache[shape, regime]


def _quarter(o):
    """The fp32 oracle within a quarter of every bar of ``o``; a tensor that is zero in fp64 is zero in fp32."""
    assert o.loss32 <= o.loss_bar / 4.0
    for k, e in o.grad32.items():
        assert (e == 0.0) if k in o.zero else (e <= o.grad_bar[k] / 4.0), (k, e, o.grad_bar[k])


def _reaches(regime, c):
    """The regime is not vacuous on this case (fp64 oracle)."""
    r = G.reach(c)
    print("    reach: %s" % r)
    assert c["moved"] <= G.KINK_SHARE * c["obs"].numel(), c["moved"]
    if regime in ("tight_noise", "fitted", "all"):
        assert r["lik_scale"][0] < 2e-3 and r["lik_scale"][1] > 20.0
        cs = c["p"]["decoder.constant_std"]
        assert bool(((cs > 19.0) & (cs < 20.0)).any()) and bool((cs > 20.0).any())          # both sides of softplus's branch
    if regime in ("posterior_scales", "all"):
        assert r["post_ratio"] >= 1e3
    if regime in ("prior_scales", "all"):
        # a prior group of ONE latent dimension (c0: z_iext = z_rtpr = 1) gets linspace(-4, 3, 1) = -4: no spread to ask for, the scale
        # itself moves to e^-4 of its own
        if all(g.z_dim == 1 for g in c["ospec"].prior_groups):
            _, ps = G.O.prior_loc_scale(c["p"], c["ospec"], c["u"])
            assert float(ps[:, :c["ospec"].latent_dim - c["ospec"].z_eps_dim].min()) < math.exp(-3.0)
        else:
            assert r["prior_ratio"] >= 1e3
    if regime in ("trained_weights", "all"):
        assert r["tanh_share"] >= 0.1 and r["state_max"] > 1.0                               # measured: 0.45 .. 0.73, 0.89 .. 0.97 at `all`
    if regime == "ties":
        assert r["ties"] > 0 and r["ties"] == G.reach(c, torch.float32)["ties"]
        assert r["ties"] >= c["obs"].shape[0] * ((c["obs"].shape[2] + 2) // 3)                # every constructed tie is one
    if regime == "fitted":
        assert r["fit_median"] <= 2.0


@pytest.mark.parametrize("regime", list(G.REGIMES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_compiled_shapes(shape, regime):
    c, main, aux = _shape(shape, regime)
    print(G.fp32_row(shape, regime, main, aux))
    assert c["obs"].dtype == torch.float32 and bool(torch.isfinite(c["obs"]).all())
    assert main.finite() and aux.finite()
    _quarter(main)
    _quarter(aux)
    for o in (main, aux):
        raised = o.loss_bar > G.LOSS_BAR or any(b > G.GRAD_BAR for b in o.grad_bar.values())
        assert raised == ((shape, regime, o.which) in RAISED), (shape, regime, o.which, "the table of tests/regime_util.py moved")
        assert o.loss_bar <= LOSS_CEILING and max(o.grad_bar.values()) <= RAISED.get((shape, regime, o.which), G.GRAD_BAR)
    if regime in ("tight_noise", "fitted"):
        d, b = main.block("decoder.constant_std", G.small_std_block(c))
        assert int(G.small_std_block(c).sum()) > 0 and d <= b / 4.0 and (b == G.GRAD_BAR or (shape, regime, "main") in RAISED)
    _reaches(regime, c)


@pytest.mark.parametrize("regime", G.BOUNDS_REGIMES)
@pytest.mark.parametrize("case", list(EU.CASES))
def test_bounds_cases(case, regime):
    c = G.apply(regime, TU.build(case, "rk4", B=EB, K=EK))
    one = dict(c, eps=c["eps"][0])
    main, aux = G.Oracles(one, "main"), G.Oracles(one, "aux")
    assert main.finite() and aux.finite()
    want, r32 = G.bounds_oracles(c)
    factor = float((want["mag"] / TU.oracle_rows(c)["mag"]).max())
    print("%-16s %-16s fp32 oracle / per-row bar %.2f -> bar x %.2f; moved %d" % (case, regime, r32, factor, c["moved"]))
    assert r32 <= BOUNDS_CEILING.get(regime, 2.0) and math.isclose(factor, max(1.0, 4.0 * r32), rel_tol=1e-12) and r32 <= 1.000001 * factor / 4.0
    _reaches(regime, one)
