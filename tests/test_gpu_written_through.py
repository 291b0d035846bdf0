"""What the ODE / ELBO launch (shape-specialised forms with a short latent) and the GEMM launch hand to the next launch leaves as
write-through stores (st_out, csrc/slode_common.h): slab rows, g_pre / glat, the saved tanh, the split-K slabs and the stage-1
partial rows.  The stored VALUES are what they were; what this file checks is that no launch reads a predecessor's output before it has
landed -- at the smallest grids, where one late workgroup is the whole launch: three consecutive svi_step calls with Adam (main, and
main + auxiliary) from a NaN-filled workspace are finite, sit inside the parity bars of the fp64 oracle on the first step (-ELBO 1e-5
relative on a fixed grid as in test_gpu_parity.py, 2e-5 for dopri5 at its default tolerances), repeat bit for bit from the same state,
and equal ONE replay of a hipGraph capture of the same three steps bit for bit."""
import pytest
import torch

from oracle import slode_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 3

CASES = {
    # (family, spec kwargs, B, T, S, relative bar of the first step's loss)
    "cvs_metric_B1": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2, solver="rk4"), 1, 200, 5, 1e-5),
    "cvs_metric_B5": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2, solver="rk4"), 5, 200, 5, 1e-5),
    "cvs_metric_B257": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2, solver="rk4"), 257, 200, 5, 1e-5),
    "cvs_midpoint_B13_T86": ("cvs", dict(solver="midpoint"), 13, 86, 5, 1e-5),
    "proc_c_major_B7_T86": ("proc", dict(z_g=3, z_eps=2, solver="midpoint"), 7, 86, 8, 1e-5),      # [B,C,T]-contiguous rows
    "cvs_dopri5_B20_T40": ("cvs", dict(z_iext=3, z_rtpr=3, z_eps=2, solver="dopri5"), 20, 40, 5, 2e-5),
}
_cache = {}


def _case(case):
    """Inputs, engine and the fp64 oracle's first-step losses, once per case."""
    if case not in _cache:
        from structured_latent_odes_amd import engine as E
        fam, kw, B, T, S, bar = CASES[case]
        ospec = {"cvs": O.cvs_spec, "proc": O.proc_spec}[fam](**kw)
        espec = {"cvs": E.cvs_spec, "proc": E.proc_spec}[fam](**kw)
        p = O.init_params(ospec, T=T, S=S)
        g = torch.Generator().manual_seed(5)
        p = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in p.items()}
        obs, u, eps, times = O.synthetic_batch(ospec, B, T)
        eng = E.Engine(espec, T, torch.device(DEV))
        eng.set_times(times)
        obs_d = obs.contiguous().to(DEV) if fam == "proc" else obs.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
        with torch.no_grad():
            want_main = O.main_loss({k: v.double() for k, v in p.items()}, ospec, obs.double(), u.double(), eps.double(), times.double()).item()
        _cache[case] = dict(eng=eng, flat0=eng.pack(p), obs_d=obs_d, u_d=u.to(DEV).contiguous(), eps_d=eps.to(DEV).contiguous(), B=B, bar=bar,
                            ospec=ospec, cpu=(obs.double(), u.double(), eps.double()), want_main=want_main)
    return _cache[case]


class _Run:
    """STEPS minibatches of svi_step calls on buffers allocated up front (nothing is allocated between the calls: capturable)."""

    def __init__(self, c, with_aux):
        from structured_latent_odes_amd import _lib as L
        self.c, self.kinds = c, [L.SVI_MAIN, L.SVI_AUX] if with_aux else [L.SVI_MAIN]
        eng, n = c["eng"], STEPS * len(self.kinds)
        self.flat = c["flat0"].clone()
        self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.loss = torch.zeros(n, device=DEV)
        self.grads = torch.zeros(n, eng.n_params, device=DEV)
        self.after_first = torch.zeros_like(self.flat)       # the weights the first auxiliary call scores

    def reset(self, poison):
        c = self.c
        self.flat.copy_(c["flat0"]); self.m.zero_(); self.v.zero_()
        self.loss.fill_(float("nan")); self.grads.fill_(float("nan"))
        if poison:
            c["eng"].workspace(c["B"]).fill_(float("nan"))    # nothing may survive from an earlier launch
        torch.cuda.synchronize()

    def steps(self, keep_first=False):
        c, eng, t = self.c, self.c["eng"], 0
        for _ in range(STEPS):
            for kind in self.kinds:
                eng.svi_step(kind, self.flat, eng.make_batch(c["obs_d"], [c["u_d"]], c["eps_d"]), c["B"], self.loss[t:t + 1], self.grads[t],
                             adam=(self.m, self.v, 1e-3, t + 1, (0.9, 0.999), 1e-8))
                if keep_first and t == 0:
                    self.after_first.copy_(self.flat)
                t += 1

    def result(self):
        torch.cuda.synchronize()
        return [x.clone() for x in (self.loss, self.grads, self.flat, self.m, self.v)]


NAMES = ("losses", "gradients", "weights", "exp_avg", "exp_avg_sq")


@pytest.mark.parametrize("with_aux", [False, True], ids=["main", "main_aux"])
@pytest.mark.parametrize("case", list(CASES))
def test_three_steps_from_a_poisoned_workspace(case, with_aux):
    c = _case(case)
    r = _Run(c, with_aux)
    r.reset(poison=True)
    r.steps(keep_first=True)
    first = r.result()
    for name, a in zip(NAMES, first):
        assert torch.isfinite(a).all(), name
    got = first[0][0].item()
    assert abs(got - c["want_main"]) / abs(c["want_main"]) < c["bar"], (got, c["want_main"])
    if with_aux:
        q = {k: v.double().cpu() for k, v in c["eng"].unpack(r.after_first[:c["eng"].n_params]).items()}
        with torch.no_grad():
            want_aux = O.aux_loss(q, c["ospec"], *c["cpu"]).item()
        got_aux = first[0][1].item()
        assert abs(got_aux - want_aux) / abs(want_aux) < 1e-5, (got_aux, want_aux)

    # the whole run again from the same state: bit for bit
    r.reset(poison=True)
    r.steps()
    for name, a, b in zip(NAMES, r.result(), first):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())

    # ONE replay of a capture of the same three steps: bit for bit the stream-launched run
    r.reset(poison=False)                                      # (per-shape set-up and the workspace exist by now: nothing of it is captured)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r.steps()
    torch.cuda.synchronize()
    assert torch.equal(r.flat, c["flat0"]), "capturing must not execute anything"
    g.replay()
    for name, a, b in zip(NAMES, r.result(), first):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
