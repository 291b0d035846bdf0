"""Test infrastructure of the fused statistics pass (slode_eval_stats): the seeded cases shared by the CPU margin check and the GPU
parity tests, and the fp64 oracle's statistics row -- main loss, auxiliary loss, reconstruction L1 sum, label hits with their decision
margins -- by the rule of training.input_pred_stats.  Not imported by the product."""
import numpy as np
import torch

from oracle import slode_oracle as O

# the six model classes; T and B from the parity cases of tests/test_gpu_parity.py (a ragged B among them)
CASES = {
    "cvs_ald": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2), 37, 200),
    "cvs_gauss": ("cvs", dict(gauss=True), 16, 86),
    "challenge_ald": ("challenge", dict(), 9, 142),
    "challenge_gauss": ("challenge", dict(gauss=True), 12, 300),
    "proc_ald": ("proc", dict(z_g=10, z_eps=10), 16, 100),
    "proc_gauss": ("proc", dict(z_g=3, z_eps=2, gauss=True), 7, 86),
}
SOLVERS = ("euler", "midpoint", "rk4")
NOISE_SEED = 21      # the four explicit noise rows [4, B, L] of a case: main, auxiliary, recon, labels
MARGIN = 1e-4        # no decision of the hit test may be closer than this to its threshold (on the fp64 oracle)
_OSPEC = {"cvs": O.cvs_spec, "challenge": O.challenge_spec, "proc": O.proc_spec}


def build_case(case, noise, solver="rk4", B=None, jitter_heads=True):
    """One seeded case at any B (None: the case's own): parameters (reference initialisers, every tensor moved by 0.05 randn and, with
    ``jitter_heads``, the label heads by another 0.3 randn: at their N(0, 1e-3) initialisation every sigmoid sits within 1e-3 of 0.5),
    one synthetic batch (seed 7) and the noise ``noise`` = (key, rows, seed): [rows, B, L] under ``key`` -- CPU generators only."""
    fam, kw, B0, T = CASES[case]
    B = B or B0
    ospec = _OSPEC[fam](solver=solver, **kw)
    S = 8 if fam == "proc" else 5
    p = O.init_params(ospec, T=T, S=S)
    g = torch.Generator().manual_seed(11)
    p = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in p.items()}
    g3 = torch.Generator().manual_seed(3)
    for k in sorted(p):
        if jitter_heads and k.startswith("q_"):
            p[k] = p[k] + 0.3 * torch.randn(p[k].shape, generator=g3)
    obs, u, _, times = O.synthetic_batch(ospec, B, T, seed=7)
    key, rows, seed = noise
    c = dict(fam=fam, kw=dict(kw, solver=solver), ospec=ospec, p=p, obs=obs, u=u, times=times, B=B, T=T, S=S)
    c[key] = torch.randn(rows, B, ospec.latent_dim, generator=torch.Generator().manual_seed(seed))
    return c


def build(case, solver="rk4"):
    """The case of the statistics row: the four noise rows [4, B, L] (main, auxiliary, recon, labels) under ``eps4``."""
    return build_case(case, ("eps4", 4, NOISE_SEED), solver)


def f64(p):
    return {k: v.double() for k, v in p.items()}


def label_decisions(p64, ospec, z4, u):
    """Per head: hits [B] (bool) and the decision margins [B] -- sigmoid: |p - 0.5|; softmax: gap between the two largest class
    probabilities; Exp/Exp: distance of the value from label +- 0.5 -- by the rule of training.input_pred_stats (prediction within 0.5
    of the label in every column)."""
    hits, margins = [], []
    for kind, prefix, zo, zd, uo, ud in ospec.aux_heads:
        zg, lab = z4[:, zo:zo + zd], u[:, uo:uo + ud]
        if kind == "bernoulli":
            pr = O.classifier_sigmoid(p64, prefix, zg)
            pred = (pr > 0.5).double()
            mg = (pr - 0.5).abs().min(dim=1).values
        elif kind == "onehot":
            pr = O.classifier_softmax(p64, prefix, zg)
            pred = torch.zeros_like(pr).scatter_(1, pr.argmax(1, keepdim=True), 1.0)
            top = pr.topk(2, dim=1).values
            mg = top[:, 0] - top[:, 1]
        else:
            pred = O.regressor_exp_exp(p64, prefix, zg)[0]
            mg = ((pred - lab).abs() - 0.5).abs().min(dim=1).values
        hits.append((pred - lab).abs().lt(0.5).all(dim=1))
        margins.append(mg)
    return hits, margins


def oracle_row(c, is_post, eps4=None):
    """The statistics row on the fp64 oracle: dict(main, aux, l1_sum, l1_bar, hits [per head], margins [per head, B])."""
    ospec, p64 = c["ospec"], f64(c["p"])
    obs, u, times = c["obs"].double(), c["u"].double(), c["times"].double()
    e = (c["eps4"] if eps4 is None else eps4).double()
    with torch.no_grad():
        main = O.main_loss(p64, ospec, obs, u, e[0], times).item()
        aux = O.aux_loss(p64, ospec, obs, u, e[1]).item()
        loc, scale = O.encoder_conv(p64, obs, ospec.pool_size)
        if is_post:
            z3 = loc + scale * e[2]
        else:
            ploc, pscale = O.prior_loc_scale(p64, ospec, u)
            z3 = ploc + pscale * e[2]
        dec = (O.decoder_gauss if ospec.gauss else O.decoder_ald)(p64, z3, times, ospec.solver)
        centre = dec[1] if ospec.gauss else dec[2]          # mean | mu_50, [B, C, T]
        l1_sum = (centre - obs).abs().sum().item()
        # |sum|a - x| - sum|b - x|| <= sum|a - b|: the per-element bar of decoded curves (2e-5 max(1, |curve|)), summed over the elements
        l1_bar = 2e-5 * centre.abs().clamp_min(1.0).sum().item()
        hits, margins = label_decisions(p64, ospec, loc + scale * e[3], u)
    return dict(main=main, aux=aux, l1_sum=l1_sum, l1_bar=l1_bar, hits=[int(h.sum()) for h in hits],
                margins=[m.numpy() for m in margins])


def min_margin(row):
    return min(float(np.min(m)) for m in row["margins"])


# ---- the model-level pass of the GPU test "fused == unfused" (in-kernel noise): three batches per family ---------------------------
MODEL_CASES = {"cvs": 86, "challenge": 86, "proc": 86}    # family -> T
MODEL_BATCH_SIZES = (24, 24, 17)
MODEL_RNG_SEED = 1234


def model_config(fam):
    from structured_latent_odes_amd import configs as CF
    cfg = getattr(CF, "load_config_" + fam)()
    cfg.update(seq_len=MODEL_CASES[fam], solver="rk4", num_particles=1)
    return cfg


def model_state(fam):
    """A CPU twin of the model (torch.manual_seed(3)), its label heads moved by 0.3 randn (generator seed 3): the state_dict the GPU
    test loads, and the batches of the pass."""
    import importlib
    from structured_latent_odes_amd.synthetic import synthetic_batch
    cfg = model_config(fam)
    T = MODEL_CASES[fam]
    _, _, times = synthetic_batch(fam, 1, T, cfg.obs_dim, seed=0)
    st = torch.random.get_rng_state()
    torch.manual_seed(3)
    try:
        m = importlib.import_module("structured_latent_odes_amd.models.mechanistic_" + fam).MechanisticModel(cfg, torch.device("cpu"), times)
    finally:
        torch.random.set_rng_state(st)
    g3 = torch.Generator().manual_seed(3)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k in sorted(state):
        if k.startswith("q_"):
            state[k] = state[k] + 0.3 * torch.randn(state[k].shape, generator=g3)
    batches = []
    for i, B in enumerate(MODEL_BATCH_SIZES):
        obs, labels, _ = synthetic_batch(fam, B, T, cfg.obs_dim, seed=7 + i)
        d = {"observations": obs}
        d.update(labels)
        batches.append(d)
    return m, state, batches, times
