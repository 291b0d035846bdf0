"""Helpers of the eval-side tests (tests/test_gpu_eval_side.py, tests/test_gpu_models_eval.py): the shapes, seeded inputs, the fp64
references, per-row error measures, and guarded output buffers for calls made through the raw C ABI.

A guarded buffer is one allocation [256 sentinel floats | the logical output, filled with NaN | 256 sentinel floats]; the kernel gets
the address of the middle part.  After the call the middle must hold no NaN (every element has an owner) and both sentinel runs must be
untouched (nothing was written outside): an out-of-bounds write is detected by reading memory the test owns, never by a fault."""
import ctypes as C

import torch
import torch.nn.functional as F

from oracle import slode_oracle as O

GUARD = 256
SENTINEL = -123456.0          # exact in fp32; no kernel output takes this value

# name: (family, spec kwargs, T, S)
SHAPES = {
    "cvs": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2), 200, 5),                    # the metric shape: L = 8, C = 3, ALD
    "proc": ("proc", dict(z_g=10, z_eps=10), 100, 8),                             # BASELINE config[2]'s dims: L = 50, C = 4, four label heads
    "challenge_gauss": ("challenge", dict(gauss=True), 300, 5),                   # BASELINE config[4]: L = 15, C = 4, one head
    "wide_head": ("cvs", dict(z_iext=17, z_rtpr=3, z_eps=2), 64, 5),              # a label head that reads 17 latent dims
}
BLOCK_EDGES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097]
DP5_TOL = dict(rtol=1e-7, atol=1e-9, per_trajectory=True)        # the engine's (torchdiffeq's) default tolerances


def _p64(m):
    return {k: v.detach().cpu().double().clone() for k, v in m.state_dict().items()}


def _heads64(p, ospec, sol):
    names = {"mean": "output_mean"} if ospec.gauss else {"mu_50": "output_q50", "mu_75": "output_q75", "mu_25": "output_q25"}
    return {k: F.linear(sol, p["decoder.%s.0.weight" % n]).permute(0, 2, 1) for k, n in names.items()}


def case_cpu(name, solver="rk4", seed=11):
    """Oracle spec, perturbed parameters (fp32 and fp64) and time grid of a shape: no GPU needed."""
    fam, kw, T, S = SHAPES[name]
    ospec = {"cvs": O.cvs_spec, "challenge": O.challenge_spec, "proc": O.proc_spec}[fam](solver=solver, **kw)
    p = O.init_params(ospec, T=T, S=S)
    g = torch.Generator().manual_seed(seed)
    p = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in p.items()}     # off the near-zero initialisation, as _mk does
    _, _, _, times = O.synthetic_batch(ospec, 4, T)
    return dict(name=name, fam=fam, kw=kw, ospec=ospec, p=p, p64={k: v.double() for k, v in p.items()}, times=times, T=T, S=S,
                L=ospec.latent_dim, C=ospec.n_channels, Q=1 if ospec.gauss else 3)


def case_gpu(name, solver="rk4", rtol=None, atol=None, times_scale=1.0):
    """case_cpu + an engine with the parameters packed."""
    from structured_latent_odes_amd import engine as E
    c = case_cpu(name, solver)
    espec = {"cvs": E.cvs_spec, "challenge": E.challenge_spec, "proc": E.proc_spec}[c["fam"]](solver=solver, **c["kw"])
    if rtol is not None:
        espec.rtol, espec.atol = rtol, atol
    c["times"] = c["times"] * times_scale
    c["dev"] = torch.device("cuda:0")
    c["eng"] = E.Engine(espec, c["T"], c["dev"])
    c["eng"].set_times(c["times"])
    c["flat"] = c["eng"].pack(c["p"])
    return c


def inputs(c, B, seed=6):
    """Seeded inputs of every standalone op at batch size B (CPU, fp32)."""
    g = torch.Generator().manual_seed(seed + 1000 * B)
    obs, u, _, _ = O.synthetic_batch(c["ospec"], B, c["T"], seed=seed + B)
    d = dict(z=torch.randn(B, c["L"], generator=g), state=torch.rand(B, c["S"], generator=g), u=u, obs=obs,
             x=torch.rand(B, c["T"], c["S"], generator=g), g_mu=torch.randn(c["Q"], B, c["C"], c["T"], generator=g),
             g_std=torch.randn(c["C"], c["T"], generator=g))
    d["state_wide"] = 3.0 * torch.rand(B, c["S"], generator=g) - 1.0      # [-1, 2): outside [0, 1] on both sides
    return d


def head_names(c):
    return ["output_mean"] if c["ospec"].gauss else ["output_q50", "output_q75", "output_q25"]


def references(c, d, dtype=torch.float64):
    """Every standalone op of the eval side on the inputs `d`, by the oracle (einsums for the head backward), in `dtype`."""
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    sp = c["ospec"]
    z, u, obs, x, g_mu, g_std = (d[k].to(dtype) for k in ("z", "u", "obs", "x", "g_mu", "g_std"))
    r = {"x0": O.initialize_state(p, z)}
    r["ploc"], r["pscale"] = O.prior_loc_scale(p, sp, u)
    lab = torch.zeros(z.shape[0], u.shape[1], dtype=dtype)
    for kind, prefix, zo, zd, uo, ud in sp.aux_heads:
        zg = z[:, zo:zo + zd]
        fn = {"bernoulli": O.classifier_sigmoid, "onehot": O.classifier_softmax}.get(kind)
        lab[:, uo:uo + ud] = fn(p, prefix, zg) if fn is not None else O.regressor_exp_exp(p, prefix, zg)[0]
    r["labels"] = lab
    W = [p["decoder.%s.0.weight" % n] for n in head_names(c)]
    r["mu"] = torch.stack([F.linear(x, w).permute(0, 2, 1) for w in W])                       # [Q, B, C, T]
    r["std"] = F.softplus(p["decoder.constant_std"])
    r["g_x"] = sum(torch.einsum("bct,cs->bts", g_mu[q], W[q]) for q in range(len(W)))
    r["g_heads"] = torch.stack([torch.einsum("bct,bts->cs", g_mu[q], x) for q in range(len(W))])
    r["g_cstd"] = g_std * torch.sigmoid(p["decoder.constant_std"])
    r["loc"], r["scale"] = O.encoder_conv(p, obs, sp.pool_size)
    return r


def dynamics_ref(c, t, state, z, dtype=torch.float64):
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    return O.dynamics(p, torch.tensor(float(t), dtype=dtype), state.to(dtype), z.to(dtype))


def row_err(got, want, row_dim=0):
    """max over rows b of |got_b - want_b| / max(|want_b|, 1) (2-norms over the row; the clamp of test_gpu_parity._close), against an
    fp64 reference: one wrong trajectory among thousands shows at full size, where a norm over the whole batch would bury it."""
    g, w = got.detach().double().cpu().movedim(row_dim, 0), want.double().cpu().movedim(row_dim, 0)
    g, w = g.reshape(g.shape[0], -1), w.reshape(w.shape[0], -1)
    return ((g - w).norm(dim=1) / w.norm(dim=1).clamp_min(1.0)).max().item()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def elem_err(a, b):
    """max |a - b| / max(1, |b|) element-wise: the trajectory measure of the suite (test_gpu_parity._close)."""
    a, b = a.detach().double().cpu(), b.double().cpu()
    return ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()


class Guarded:
    """A caller-allocated output with NaN inside and sentinel runs on both sides (module docstring)."""

    def __init__(self, shape, dev):
        n = 1
        for s in shape:
            n *= int(s)
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(float("nan"))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def check(self, what):
        torch.cuda.synchronize()
        assert not bool(torch.isnan(self.t).any()), "%s: output elements left unwritten (or NaN)" % what
        assert bool((self.buf[:GUARD] == SENTINEL).all()), "%s: write in front of the output buffer" % what
        assert bool((self.buf[GUARD + self.n:] == SENTINEL).all()), "%s: write behind the output buffer" % what
        return self.t


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _call(eng, name, *args):
    from structured_latent_odes_amd.engine import _check
    _check(eng.lib, eng.handle, getattr(eng.lib, name)(eng.handle, *args, eng._stream()))


def _sl(eng, B):
    return C.byref(eng.shape(B)), C.byref(eng.layout)


# ---- the raw entry points, outputs guarded (inputs: contiguous fp32 device tensors) ---------------------------------------------------
def raw_initialize_state(eng, flat, z):
    out = Guarded((z.shape[0], eng.spec.ode_state_dim), z.device)
    _call(eng, "slode_initialize_state", *_sl(eng, z.shape[0]), _ptr(flat), _ptr(z), out.ptr)
    return out.check("initialize_state B=%d" % z.shape[0])


def raw_dynamics_eval(eng, flat, t, state, z):
    out = Guarded(tuple(state.shape), z.device)
    _call(eng, "slode_dynamics_eval", *_sl(eng, z.shape[0]), _ptr(flat), float(t), _ptr(state), _ptr(z), out.ptr)
    return out.check("dynamics_eval B=%d t=%g" % (z.shape[0], t))


def raw_prior_nets(eng, flat, u):
    B = u.shape[0]
    loc, scale = Guarded((B, eng.spec.latent_dim), u.device), Guarded((B, eng.spec.latent_dim), u.device)
    _call(eng, "slode_prior_nets", *_sl(eng, B), _ptr(flat), _ptr(u), loc.ptr, scale.ptr)
    return loc.check("prior_nets loc B=%d" % B), scale.check("prior_nets scale B=%d" % B)


def raw_label_heads(eng, flat, z):
    out = Guarded((z.shape[0], eng.spec.n_u), z.device)          # every label column of these families is scored by a head
    _call(eng, "slode_label_heads", *_sl(eng, z.shape[0]), _ptr(flat), _ptr(z), out.ptr)
    return out.check("label_heads B=%d" % z.shape[0])


def raw_decode_heads(eng, flat, x):
    B, sp = x.shape[0], eng.spec
    mu = Guarded((1 if sp.gauss else 3, B, sp.n_channels, eng.T), x.device)
    std = Guarded((sp.n_channels, eng.T), x.device)
    _call(eng, "slode_decode_heads", *_sl(eng, B), _ptr(flat), _ptr(x), mu.ptr, std.ptr)
    return mu.check("decode_heads mu B=%d" % B), std.check("decode_heads std B=%d" % B)


def raw_decode_heads_bwd(eng, flat, x, g_mu, g_std=None, snapshot=None):
    B, sp = x.shape[0], eng.spec
    Q = 1 if sp.gauss else 3
    g_x = Guarded((B, eng.T, sp.ode_state_dim), x.device)
    g_heads = Guarded((Q, sp.n_channels, sp.ode_state_dim), x.device)
    g_cstd = Guarded((sp.n_channels, eng.T), x.device)
    if snapshot is not None:
        snap, lo = snapshot
        p_ptr = C.c_void_p(snap.data_ptr() - 4 * lo)           # the kernels read nothing below the first decoder head
    else:
        p_ptr = _ptr(flat)
    _call(eng, "slode_decode_heads_bwd", *_sl(eng, B), p_ptr, _ptr(x), _ptr(g_mu), _ptr(g_std), g_x.ptr, g_heads.ptr, g_cstd.ptr)
    w = "decode_heads_bwd B=%d" % B
    return g_x.check(w + " g_x"), g_heads.check(w + " g_heads"), g_cstd.check(w + " g_cstd")


def raw_rng_normal(eng, n, B):
    out = Guarded((B, eng.spec.latent_dim), eng.device)
    from structured_latent_odes_amd.engine import _check
    _check(eng.lib, eng.handle, eng.lib.slode_rng_normal(eng.handle, int(n), B, eng.spec.latent_dim, out.ptr, None, eng._stream()))
    return out.check("rng_normal B=%d" % B)


def raw_sample_normal(eng, loc, scale):
    out = Guarded(tuple(loc.shape), loc.device)
    from structured_latent_odes_amd.engine import _check
    _check(eng.lib, eng.handle, eng.lib.slode_sample_normal(eng.handle, loc.shape[0], loc.shape[1], _ptr(loc), _ptr(scale), out.ptr, eng._stream()))
    return out.check("sample_normal B=%d" % loc.shape[0])


def raw_encoder_fwd(eng, flat, obs):
    """The inference form: pooled / hid NULL."""
    B = obs.shape[0]
    loc, scale = Guarded((B, eng.spec.latent_dim), obs.device), Guarded((B, eng.spec.latent_dim), obs.device)
    _call(eng, "slode_encoder_conv_fwd", *_sl(eng, B), _ptr(flat), _ptr(obs), eng._obs_strides(obs), loc.ptr, scale.ptr, None, None)
    return loc.check("encoder_fwd loc B=%d" % B), scale.check("encoder_fwd scale B=%d" % B)


def raw_ode_solve(eng, flat, z):
    B = z.shape[0]
    x = Guarded((B, eng.T, eng.spec.ode_state_dim), z.device)
    _call(eng, "slode_ode_solve_fwd", *_sl(eng, B), _ptr(flat), _ptr(eng._times), _ptr(eng._stage_t), _ptr(z), x.ptr)
    return x.check("ode_solve B=%d" % B)


def obs_to_device(c, obs):
    """The family's native layout: [B, C, T] view of a dense [B, T, C] tensor (cvs / challenge), dense [B, C, T] (proc)."""
    if c["fam"] == "proc":
        return obs.contiguous().to(c["dev"])
    return obs.permute(0, 2, 1).contiguous().to(c["dev"]).permute(0, 2, 1)


def oracle_rows(B, ns=None):
    """The fixed selection of at most 96 trajectories checked against the fp64 oracle at a large size: the first 16, the 32 around the
    65,536 switch of the launch policy, the last 32 (what a resident workgroup reaches last) and 16 scattered."""
    rows = list(range(16)) + [r for r in range(65520, 65552) if r < B] + list(range(B - 32, B))
    g = torch.Generator().manual_seed(B)
    rows += torch.randint(0, B, (16,), generator=g).tolist()
    return sorted(set(r for r in rows if 0 <= r < B))
