"""The fold launch (weff_kernel: a quad produces a window of consecutive time points of one (hidden unit, channel) from registers,
csrc/fold_math.h) through an existing entry point, at the shapes where the windows can go wrong: T = K + P - 1 (n_pool = 1: every tap index
is clamped), T = 23 (no window width divides it; n_pool = 10), T = 100 (several blocks), three and four channels, both dense layouts
(kappa = t C + c and kappa = c T + t), B = 2 and B = 5, and the long-tap instantiation (J = 17 > 14).

Engine.posterior_refine with num_steps = 0 returns the posterior the folded encoder (launches weff, enc_fwd2) left in the workspace, bit for
bit (tests/test_gpu_refine.py); it is held to the oracle's layer-by-layer encoder at the bound of tests/test_gpu_parity.py::
test_encoder_forward (2e-5 norm-wise: the fold differs from it by fp32 summation order alone), and a repeat of the call to itself bit for
bit.  Weights away from the initialisation (+ 0.05 N(0, 1)): an orthogonal lin.weight would hide little, but costs nothing to leave."""
import dataclasses

import pytest
import torch

from oracle import slode_oracle as O
from tests.eval_gpu_util import DEV, WIDTHS

pytestmark = pytest.mark.gpu

# (family, T, n_filters, filter_size, pool_size)
SHAPES = {
    "cvs_T14": ("cvs", 14, 10, 10, 5),
    "cvs_T23": ("cvs", 23, 10, 10, 5),
    "cvs_T100": ("cvs", 100, 10, 10, 5),
    "challenge_T14": ("challenge", 14, 10, 10, 5),
    "challenge_T23": ("challenge", 23, 10, 10, 5),
    "challenge_T100": ("challenge", 100, 10, 10, 5),
    "cvs_long_tap_T90_K12_P6": ("cvs", 90, 4, 12, 6),
}


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("t_major", [True, False], ids=["t_major", "c_major"])
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_folded_encoder_forward_against_the_oracle_and_repeatable(name, B, t_major):
    from structured_latent_odes_amd import engine as E
    fam, T, F_, K, P = SHAPES[name]
    ospec = {"cvs": O.cvs_spec, "challenge": O.challenge_spec}[fam](solver="rk4", pool_size=P)
    p = O.init_params(ospec, T=T, S=5, F_=F_, K=K)
    g = torch.Generator().manual_seed(31)
    p = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in p.items()}
    obs, u, eps, times = O.synthetic_batch(ospec, B, T)
    espec = {"cvs": E.cvs_spec, "challenge": E.challenge_spec}[fam](solver="rk4")
    espec = dataclasses.replace(espec, n_filters=F_, filter_size=K, pool_size=P)
    eng = E.Engine(espec, T, DEV)
    eng.set_times(times)
    flat = eng.pack(p)
    obs_d = obs.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1) if t_major else obs.to(DEV).contiguous()
    labels, o = [], 0
    for w in WIDTHS[fam]:
        labels.append(u[:, o:o + w].contiguous().to(DEV))
        o += w
    L = ospec.latent_dim
    outs, names = [], []
    for rep in range(2):
        eng.workspace(B).fill_(float("nan"))
        loc, scale = torch.full((B, L), float("nan"), device=DEV), torch.full((B, L), float("nan"), device=DEV)
        eng.profile_enable(True)
        eng.posterior_refine(flat, eng.make_batch(obs_d, labels, eps.to(DEV).contiguous()), B, 1, 0, loc=loc, scale=scale, grad0=False, trace=False,
                             best_step=False)
        names.append([n for n, _ in eng.profile_read()])
        eng.profile_enable(False)
        outs.append((loc.clone(), scale.clone()))
    assert names[0][:2] == ["weff", "enc_fwd2"], names[0]                                  # the fold launch ran, and the folded forward read it
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    loc, scale = outs[0]
    assert torch.isfinite(loc).all() and torch.isfinite(scale).all()
    want_loc, want_scale = O.encoder_conv(p, obs, ospec.pool_size)
    el, es = _rel(loc, want_loc), _rel(scale, want_scale)
    print("%s B = %d %s: loc %.2e scale %.2e (bound 2e-5)" % (name, B, "t-major" if t_major else "c-major", el, es))
    assert el < 2e-5 and es < 2e-5
