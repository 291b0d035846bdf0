"""Host-side engine: owns the libslode handle, the parameter layout and the workspaces; every method is one call
through the C ABI (include/slode.h) on the caller's current HIP stream.  PyTorch tensors are storage only."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L


@dataclass
class PriorGroup:
    """p(z_g | u_g): latent dims [z_off, z_off+z_dim), label columns [u_off, u_off+u_dim) of u.
    `prefix` is the reference attribute name of the EncoderMLP (e.g. 'p_z_iext_given_iext')."""
    prefix: str
    z_off: int
    z_dim: int
    u_off: int
    u_dim: int


@dataclass
class AuxHead:
    """A label head q(label | z_g) (auxiliary loss; also the main loss for the proc family): `prefix` = reference attribute
    (e.g. 'q_aR_given_z_aR'), kind in sigmoid | softmax | expexp; `std_key` = the scalar std parameter of an expexp head."""
    prefix: str
    kind: str
    z_off: int
    z_dim: int
    u_off: int
    u_dim: int
    std_key: str = ""


@dataclass
class ModelSpec:
    """Shape of one of the reference's three model families (models/mechanistic_{cvs,proc,challenge}[_Gauss].py)."""
    name: str
    gauss: bool
    n_channels: int
    latent_dim: int
    z_eps_dim: int
    n_u: int
    prior_groups: List[PriorGroup]
    ode_state_dim: int = 5
    ode_hidden_dim: int = 25
    n_filters: int = 10
    filter_size: int = 10
    pool_size: int = 5
    cnn_hidden_dim: int = 50
    solver: str = "midpoint"   # _lib.METHODS: euler / midpoint / rk4 (fixed grid), dopri5 / bosh3 / fehlberg2 / adaptive_heun (adaptive)
    quantile_diff: float = 0.475
    aux_heads: List[AuxHead] = field(default_factory=list)
    labels_in_main: bool = False   # proc: the main model also scores the label heads (mechanistic_proc.py:145-146)
    u_hidden_dim: int = 25
    aux_mult: float = 46.0
    rtol: float = 1e-7      # adaptive methods only (torchdiffeq defaults)
    atol: float = 1e-9
    # "exact": gradient of the discrete scheme (== adjoint_solver=False); "reference_adjoint": torchdiffeq.odeint_adjoint's backward,
    # the reference default (config.adjoint_solver = True; models/blackbox_ode.py:40-42) -- no gradient to z through the dynamics
    grad_mode: str = "exact"

    @property
    def head_names(self) -> List[str]:
        return ["output_mean"] if self.gauss else ["output_q50", "output_q75", "output_q25"]


def _check(lib, handle, rc):
    if rc != 0:
        msg = lib.slode_last_error(handle)
        err = L.SlodeError("libslode call failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        err.status = int(rc)   # slode_status: -1 = SLODE_EINVAL (a refusal: nothing was launched), -2 = SLODE_EHIP, -3 = SLODE_ENOSPC
        raise err


PROFILE_MAX_KERNELS = 16   # include/slode.h, SLODE_PROFILE_MAX_KERNELS


class Engine:
    def __init__(self, spec: ModelSpec, n_time: int, device: Optional[torch.device] = None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.SlodeError("no HIP device visible: the slode engine has no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        if self.device.type != "cuda":
            raise L.SlodeError("the slode engine runs on a HIP device only, got %s" % self.device)
        self.spec, self.T = spec, int(n_time)
        self.handle = C.c_void_p()
        _check(self.lib, None, self.lib.slode_create(C.byref(self.handle), self.device.index or 0))
        self._shapes: Dict[Tuple[int, int], L.Shape] = {}
        self.layout = L.Layout()
        _check(self.lib, None, self.lib.slode_layout_init(C.byref(self.shape(1)), C.byref(self.layout)))
        self.n_params = int(self.layout.n_params)
        self._ws: Dict[Tuple[int, int], torch.Tensor] = {}
        self._stage_t: Optional[torch.Tensor] = None
        self._times: Optional[torch.Tensor] = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.slode_destroy(self.handle)
        except Exception:
            pass

    # ---- shapes / layout ---------------------------------------------------------------------------------
    def shape(self, B: int, particles: int = 1) -> L.Shape:
        """slode_shape for B data rows and `particles` ELBO particles (Trace_ELBO(num_particles=...): include/slode.h)."""
        particles = int(particles)
        if particles < 1 or particles > L.MAX_PARTICLES:
            raise ValueError("particles must be in [1, %d], got %d" % (L.MAX_PARTICLES, particles))
        s = self._shapes.get((B, particles))
        if s is None:
            sp = self.spec
            if sp.solver not in L.METHODS:
                raise ValueError("unknown solver %r" % sp.solver)
            s = L.Shape(B=B, T=self.T, C=sp.n_channels, L=sp.latent_dim, S=sp.ode_state_dim, H=sp.ode_hidden_dim,
                        F=sp.n_filters, K=sp.filter_size, P=sp.pool_size, Hc=sp.cnn_hidden_dim, n_u=sp.n_u,
                        n_groups=len(sp.prior_groups), method=L.METHODS[sp.solver],
                        likelihood=L.GAUSS if sp.gauss else L.ALD, quantile_diff=sp.quantile_diff, rtol=sp.rtol, atol=sp.atol,
                        n_aux=len(sp.aux_heads), U=sp.u_hidden_dim, aux_mult=sp.aux_mult, aux_in_main=int(sp.labels_in_main),
                        grad_mode=L.GRAD_MODES[sp.grad_mode], particles=particles)
            for i, a in enumerate(sp.aux_heads):
                s.aux[i] = L.Aux(L.AUX_KINDS[a.kind], a.z_off, a.z_dim, a.u_off, a.u_dim)
            for i, g in enumerate(sp.prior_groups):
                s.groups[i] = L.Group(g.z_off, g.z_dim, g.u_off, g.u_dim)
            self._shapes[(B, particles)] = s
        return s

    def param_table(self) -> List[Tuple[str, int, Tuple[int, ...]]]:
        """(reference state_dict key, offset, shape) of every tensor of the flat layout, in layout order."""
        sp, lay, T = self.spec, self.layout, self.T
        C_, Ld, S, H, F, K, Hc = sp.n_channels, sp.latent_dim, sp.ode_state_dim, sp.ode_hidden_dim, sp.n_filters, sp.filter_size, sp.cnn_hidden_dim
        FQ = F * (T - K + 1 - sp.pool_size + 1)
        t = [("encoder.conv.weight", lay.conv_w, (F, C_, K)), ("encoder.conv.bias", lay.conv_b, (F,)),
             ("encoder.lin.weight", lay.lin_w, (Hc, FQ)), ("encoder.lin.bias", lay.lin_b, (Hc,)),
             ("encoder.z_loc.weight", lay.zloc_w, (Ld, Hc)), ("encoder.z_loc.bias", lay.zloc_b, (Ld,)),
             ("encoder.z_scale.0.weight", lay.zls_w, (Ld, Hc)), ("encoder.z_scale.0.bias", lay.zls_b, (Ld,))]
        for i, g in enumerate(sp.prior_groups):
            t += [(g.prefix + ".sequential_mlp.1.0.0.weight", lay.ploc_w[i], (g.z_dim, g.u_dim)),
                  (g.prefix + ".sequential_mlp.1.0.0.bias", lay.ploc_b[i], (g.z_dim,)),
                  (g.prefix + ".sequential_mlp.1.1.0.weight", lay.pls_w[i], (g.z_dim, g.u_dim)),
                  (g.prefix + ".sequential_mlp.1.1.0.bias", lay.pls_b[i], (g.z_dim,))]
        o = "decoder.ode_model."
        t += [(o + "latent_to_ode_net.0.weight", lay.init_w1, (H, Ld)), (o + "latent_to_ode_net.0.bias", lay.init_b1, (H,)),
              (o + "latent_to_ode_net.2.weight", lay.init_w2, (S, H)), (o + "latent_to_ode_net.2.bias", lay.init_b2, (S,)),
              (o + "dynamics.dynamics_hidden.weight", lay.dyn_wh, (H, 1 + Ld)), (o + "dynamics.dynamics_hidden.bias", lay.dyn_bh, (H,)),
              (o + "dynamics.dyanamics_growth.weight", lay.dyn_wg, (S, H)), (o + "dynamics.dyanamics_growth.bias", lay.dyn_bg, (S,)),
              (o + "dynamics.dyanmics_degradation.weight", lay.dyn_wd, (S, H)), (o + "dynamics.dyanmics_degradation.bias", lay.dyn_bd, (S,))]
        for i, hn in enumerate(sp.head_names):
            t.append(("decoder.%s.0.weight" % hn, lay.head_w[i], (C_, S)))
        U = sp.u_hidden_dim
        for i, a in enumerate(sp.aux_heads):
            t += [(a.prefix + ".sequential_mlp.1.module.weight", lay.aux_w1[i], (U, a.z_dim)),
                  (a.prefix + ".sequential_mlp.1.module.bias", lay.aux_b1[i], (U,))]
            if a.kind == "expexp":
                t += [(a.prefix + ".sequential_mlp.3.0.0.weight", lay.aux_w2[i], (a.u_dim, U)), (a.prefix + ".sequential_mlp.3.0.0.bias", lay.aux_b2[i], (a.u_dim,)),
                      (a.prefix + ".sequential_mlp.3.1.0.weight", lay.aux_w3[i], (a.u_dim, U)), (a.prefix + ".sequential_mlp.3.1.0.bias", lay.aux_b3[i], (a.u_dim,)),
                      (a.std_key, lay.aux_c[i], (1,))]
            else:
                t += [(a.prefix + ".sequential_mlp.3.weight", lay.aux_w2[i], (a.u_dim, U)), (a.prefix + ".sequential_mlp.3.bias", lay.aux_b2[i], (a.u_dim,))]
        t.append(("decoder.constant_std", lay.cstd, (C_, T)))
        return t

    def pack(self, params: Dict[str, torch.Tensor], flat: Optional[torch.Tensor] = None, extra: int = 0) -> torch.Tensor:
        """Copy a reference-keyed parameter dict into a flat device vector (n_params + extra floats)."""
        if flat is None:
            flat = torch.zeros(self.n_params + extra, dtype=torch.float32, device=self.device)
        for key, off, shp in self.param_table():
            n = 1
            for d in shp:
                n *= d
            flat[off:off + n].copy_(params[key].reshape(-1).to(torch.float32))
        return flat

    def unpack(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        for key, off, shp in self.param_table():
            n = 1
            for d in shp:
                n *= d
            out[key] = flat[off:off + n].view(*shp)
        return out

    # ---- plumbing ----------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _p(t: Optional[torch.Tensor]):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def _f32(self, t: torch.Tensor, name: str, contiguous: bool = True) -> torch.Tensor:
        if t.device != self.device or t.dtype != torch.float32:
            raise ValueError("%s must be a float32 tensor on %s (got %s on %s)" % (name, self.device, t.dtype, t.device))
        if contiguous and not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        return t

    def _eps_shape(self, B: int, particles: int):
        """Explicit noise: [B, L] for one particle, one dense particle-major [K, B, L] tensor for K > 1."""
        return (B, self.spec.latent_dim) if particles == 1 else (particles, B, self.spec.latent_dim)

    def _check_batch(self, obs, u, eps, particles: int = 1):
        """The kernels read raw device pointers: a CPU / float64 / strided label or noise tensor must not get that far."""
        B = obs.shape[0]
        self._f32(obs, "observations", contiguous=False)
        if u is not None:
            self._f32(u, "u")
            if tuple(u.shape) != (B, self.spec.n_u):
                raise ValueError("u must be [%d, %d], got %s" % (B, self.spec.n_u, tuple(u.shape)))
        self._f32(eps, "eps")
        if tuple(eps.shape) != self._eps_shape(B, particles):
            raise ValueError("eps must be %s, got %s" % (list(self._eps_shape(B, particles)), tuple(eps.shape)))

    def workspace(self, B: int, particles: int = 1) -> torch.Tensor:
        w = self._ws.get((B, particles))
        if w is None:
            nbytes = int(self.lib.slode_workspace_bytes(self.handle, C.byref(self.shape(B, particles))))
            if nbytes == 0:
                _check(self.lib, None, -1)
            w = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
            self._ws[(B, particles)] = w
        return w

    def _check_grid(self, t: torch.Tensor):
        """ValueError unless the grid ``t`` is one the solver takes (``set_times`` and ``forecast_grid``)."""
        d = t[1:] - t[:-1]
        if not (bool((d > 0).all()) or bool((d < 0).all())):    # torchdiffeq odeint's own precondition (misc._check_timelike)
            raise ValueError("t must be strictly increasing or decreasing")
        if self.spec.solver in L.ADAPTIVE and not bool((d > 0).all()):
            # torchdiffeq integrates a decreasing grid in s = -t; the adaptive kernels here only walk forward in time
            # (dopri5_kernel.hip: dt > 0, outputs emitted while tj <= t1) and answer such a grid with NaN trajectories
            raise ValueError("solver=%r needs a strictly increasing time grid (decreasing grids: fixed-grid solvers only)" % self.spec.solver)

    def _head_shape(self, rows: int, T: int = None):
        """``(Q, rows, C, T)`` of a head-curve output: Q = 3 quantile heads, 1 for the Gaussian family; T: the bound grid's by default."""
        return (1 if self.spec.gauss else 3, rows, self.spec.n_channels, self.T if T is None else T)

    def set_times(self, times: torch.Tensor) -> torch.Tensor:
        """Bind the time grid (len T) and build the stage-time table on device."""
        times = self._f32(times.to(self.device, torch.float32).contiguous(), "times")
        if times.numel() != self.T:
            raise ValueError("times has %d points, engine built for T=%d" % (times.numel(), self.T))
        self._check_grid(times)
        n = int(self.lib.slode_num_stage_times(C.byref(self.shape(1))))
        st = torch.empty(n, dtype=torch.float32, device=self.device)
        _check(self.lib, self.handle, self.lib.slode_stage_times(self.handle, C.byref(self.shape(1)), self._p(times), self._p(st), self._stream()))
        self._times, self._stage_t = times, st
        return st

    def _obs_strides(self, obs: torch.Tensor):
        if obs.dim() != 3 or obs.shape[1] != self.spec.n_channels or obs.shape[2] != self.T:
            raise ValueError("observations must be [B, %d, %d], got %s" % (self.spec.n_channels, self.T, tuple(obs.shape)))
        return (C.c_int64 * 3)(*obs.stride())

    # ---- ops (one C-ABI call each) ---------------------------------------------------------------------------
    def encoder_fwd(self, params, obs, save: bool = True):
        B = obs.shape[0]
        sp = self.spec
        self._f32(obs, "observations", contiguous=False)
        FQ = sp.n_filters * (self.T - sp.filter_size + 1 - sp.pool_size + 1)
        loc = torch.empty(B, sp.latent_dim, dtype=torch.float32, device=self.device)
        scale = torch.empty_like(loc)
        pooled = torch.empty(B, FQ, dtype=torch.float32, device=self.device) if save else None
        hid = torch.empty(B, sp.cnn_hidden_dim, dtype=torch.float32, device=self.device) if save else None
        _check(self.lib, self.handle, self.lib.slode_encoder_conv_fwd(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(obs), self._obs_strides(obs),
            self._p(loc), self._p(scale), self._p(pooled), self._p(hid), self._stream()))
        return loc, scale, pooled, hid

    def encoder_bwd(self, params, obs, scale, pooled, hid, g_loc, g_scale, grads):
        B = obs.shape[0]
        ws = self.workspace(B)
        _check(self.lib, self.handle, self.lib.slode_encoder_conv_bwd(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(obs), self._obs_strides(obs),
            self._p(scale), self._p(pooled), self._p(hid), self._p(self._f32(g_loc, "g_loc")), self._p(self._f32(g_scale, "g_scale")),
            self._p(grads), self._p(ws), ws.numel() * 4, self._stream()))
        return grads

    def ode_solve(self, params, z, times=None):
        """z [B, L] -> x [B, T, S] on the bound grid, or, with ``times`` (a tensor ``forecast_grid`` takes), on that grid: x [B, len(times), S].
        The solve kernels read the init net and the dynamics alone -- no parameter whose size depends on T (the encoder's lin.weight and
        constant_std are not theirs) -- so a shape copy with T = len(times) on the same flat vector is the same model on another grid.
        That shape goes through the library's own check: at most 1024 points."""
        B = z.shape[0]
        if times is None:
            shp, T, tt, st = self.shape(B), self.T, self._times, self._stage_t
        else:
            tt, st = self.forecast_grid(times)
            T = tt.numel()
            shp = L.Shape.from_buffer_copy(self.shape(B))
            shp.T = T
        x = torch.empty(B, T, self.spec.ode_state_dim, dtype=torch.float32, device=self.device)
        _check(self.lib, self.handle, self.lib.slode_ode_solve_fwd(
            self.handle, C.byref(shp), C.byref(self.layout), self._p(params), self._p(tt), self._p(st),
            self._p(self._f32(z, "z")), self._p(x), self._stream()))
        return x

    def ode_snapshot(self, params):
        """Copy of the flat range [layout.ode_begin, n_params) -- everything ode_solve_bwd reads of the parameters -- and its start:
        the weights of a forward solve, frozen for its backward (the fused Adam kernels update the flat vector in place)."""
        lo = int(self.layout.ode_begin)
        return params[lo:self.n_params].clone(), lo

    def ode_solve_bwd(self, params, z, g_x, grads, snapshot=None):
        """Backward of ode_solve.  `snapshot` = ode_snapshot(...) of the forward: the kernel then differentiates at those weights (it
        reads no parameter below layout.ode_begin, so the base pointer is the snapshot's, moved back by its start)."""
        B = z.shape[0]
        ws = self.workspace(B)
        g_z = torch.empty_like(z)
        if snapshot is not None:
            snap, lo = snapshot
            if snap.numel() != self.n_params - lo or lo != int(self.layout.ode_begin):
                raise ValueError("snapshot does not match this engine's layout")
            p_ptr = C.c_void_p(self._f32(snap, "snapshot").data_ptr() - 4 * lo)
        else:
            p_ptr = self._p(params)
        _check(self.lib, self.handle, self.lib.slode_ode_solve_bwd(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), p_ptr, self._p(self._times), self._p(self._stage_t),
            self._p(self._f32(z, "z")), self._p(self._f32(g_x, "g_x")), self._p(g_z), self._p(grads), self._p(ws), ws.numel() * 4, self._stream()))
        return g_z

    def dynamics_eval(self, params, t: float, state, z):
        B = z.shape[0]
        out = torch.empty_like(state)
        _check(self.lib, self.handle, self.lib.slode_dynamics_eval(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), float(t), self._p(self._f32(state, "state")),
            self._p(self._f32(z, "z")), self._p(out), self._stream()))
        return out

    def initialize_state(self, params, z):
        """OdeModel.initialize_state: z [B, L] -> x0 [B, S] (one small HIP kernel, no solve)."""
        B = z.shape[0]
        x0 = torch.empty(B, self.spec.ode_state_dim, dtype=torch.float32, device=self.device)
        _check(self.lib, self.handle, self.lib.slode_initialize_state(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(self._f32(z, "z")), self._p(x0), self._stream()))
        return x0

    def prior_nets(self, params, u):
        """Conditional priors: u [B, n_u] -> (loc, scale) [B, L]; dims outside every conditional group: (0, 1)."""
        B = u.shape[0]
        loc = torch.empty(B, self.spec.latent_dim, dtype=torch.float32, device=self.device)
        scale = torch.empty_like(loc)
        _check(self.lib, self.handle, self.lib.slode_prior_nets(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(self._f32(u, "u")), self._p(loc), self._p(scale),
            self._stream()))
        return loc, scale

    def label_heads(self, params, z):
        """Label heads q(label | z_g): z [B, L] -> [B, n_u] probabilities / Laplace locations in the label columns they score."""
        B = z.shape[0]
        out = torch.zeros(B, self.spec.n_u, dtype=torch.float32, device=self.device)
        _check(self.lib, self.handle, self.lib.slode_label_heads(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(self._f32(z, "z")), self._p(out), self._stream()))
        return out

    def dopri5_step_counts(self, B: int, particles: int = 1) -> torch.Tensor:
        """Accepted steps per trajectory of the last adaptive-method (dopri5, bosh3, fehlberg2, adaptive_heun) training step at batch
        size B (diagnostic; int32 [B], [particles * B] particle-major with particles; -1: 20,000 attempts exhausted, > slode_dopri5_kmax:
        record overflow)."""
        out = torch.empty(B * particles, dtype=torch.int32, device=self.device)
        w = self.workspace(B, particles)
        _check(self.lib, self.handle, self.lib.slode_dopri5_step_counts(
            self.handle, C.byref(self.shape(B, particles)), C.byref(self.layout), self._p(w), w.numel() * 4, self._p(out), self._stream()))
        return out

    def decode_heads(self, params, x):
        B = x.shape[0]
        sp = self.spec
        mu = torch.empty(self._head_shape(B), dtype=torch.float32, device=self.device)
        std = torch.empty(sp.n_channels, self.T, dtype=torch.float32, device=self.device)
        _check(self.lib, self.handle, self.lib.slode_decode_heads(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(self._f32(x, "x")), self._p(mu), self._p(std), self._stream()))
        return mu, std

    def heads_snapshot(self, params):
        """Copy of the flat range [first decoder head, n_params) -- the decoder heads and constant_std (with the label heads, if any,
        between them) -- and its start: what decode_heads_bwd reads of the parameters, frozen at forward time."""
        lo = int(self.layout.head_w[0])
        return params[lo:self.n_params].clone(), lo

    def decode_heads_bwd(self, params, x, g_mu, g_std=None, snapshot=None):
        """Backward of decode_heads: g_mu [Q, B, C, T] (+ g_std [C, T]) -> (g_x [B, T, S], g_heads [Q, C, S], g_cstd [C, T]).
        `snapshot` = heads_snapshot(...) of the forward: the kernel then reads the head weights / constant_std from it (it touches no
        parameter below the first decoder head, so the base pointer is the snapshot's, moved back by its start)."""
        B = x.shape[0]
        sp = self.spec
        Q = 1 if sp.gauss else 3
        g_x = torch.empty(B, self.T, sp.ode_state_dim, dtype=torch.float32, device=self.device)
        g_heads = torch.empty(Q, sp.n_channels, sp.ode_state_dim, dtype=torch.float32, device=self.device)
        g_cstd = torch.empty(sp.n_channels, self.T, dtype=torch.float32, device=self.device)
        if snapshot is not None:
            snap, lo = snapshot
            if snap.numel() != self.n_params - lo or lo != int(self.layout.head_w[0]):
                raise ValueError("snapshot does not match this engine's layout")
            p_ptr = C.c_void_p(self._f32(snap, "snapshot").data_ptr() - 4 * lo)
        else:
            p_ptr = self._p(params)
        _check(self.lib, self.handle, self.lib.slode_decode_heads_bwd(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), p_ptr, self._p(self._f32(x, "x")), self._p(self._f32(g_mu, "g_mu")),
            self._p(self._f32(g_std, "g_std") if g_std is not None else None), self._p(g_x), self._p(g_heads), self._p(g_cstd), self._stream()))
        return g_x, g_heads, g_cstd

    def elbo_step(self, params, obs, u, eps, loss_out, grads=None, x_out=None, z_out=None):
        """-ELBO (summed over the batch) into loss_out[0]; exact gradient into grads (flat) unless grads is None."""
        B = obs.shape[0]
        self._check_batch(obs, u, eps)
        ws = self.workspace(B)
        self._guard(params, ws)
        _check(self.lib, self.handle, self.lib.slode_elbo_step(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(self._times), self._p(self._stage_t),
            self._p(obs), self._obs_strides(obs), self._p(u), self._p(eps), self._p(loss_out), self._p(grads), self._p(x_out), self._p(z_out),
            self._p(ws), ws.numel() * 4, self._stream()))
        return loss_out

    def elbo_adam_step(self, params, obs, u, eps, loss_out, grads, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), adam_eps=1e-8):
        """elbo_step + Adam with the update fused into the gradient reduction (single-process training)."""
        B = obs.shape[0]
        self._check_batch(obs, u, eps)
        ws = self.workspace(B)
        self._guard(params, ws)
        _check(self.lib, self.handle, self.lib.slode_elbo_adam_step(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(self._times), self._p(self._stage_t),
            self._p(obs), self._obs_strides(obs), self._p(u), self._p(eps), self._p(loss_out), self._p(grads), self._p(ws), ws.numel() * 4,
            params.numel(), self._p(exp_avg), self._p(exp_avg_sq), float(lr), float(betas[0]), float(betas[1]), float(adam_eps), int(step),
            self._stream()))
        return loss_out

    def aux_step(self, params, obs, u, eps, loss_out, grads=None, adam=None):
        """-ELBO of the auxiliary loss (model_meta) and its gradient; `adam` = (exp_avg, exp_avg_sq, lr, step, betas, eps) fuses
        the Adam update into the final reduction."""
        B = obs.shape[0]
        self._check_batch(obs, u, eps)
        ws = self.workspace(B)
        self._guard(params, ws)
        m, v, lr, step, betas, aeps = adam if adam is not None else (None, None, 0.0, 1, (0.9, 0.999), 1e-8)
        _check(self.lib, self.handle, self.lib.slode_aux_step(
            self.handle, C.byref(self.shape(B)), C.byref(self.layout), self._p(params), self._p(obs), self._obs_strides(obs), self._p(u),
            self._p(eps), self._p(loss_out), self._p(grads), self._p(ws), ws.numel() * 4, params.numel(), self._p(m), self._p(v), float(lr),
            float(betas[0]), float(betas[1]), float(aeps), int(step), self._stream()))
        return loss_out

    # ---- SVI.step(**batch) as one call: labels as the loader yields them, noise drawn in the kernels -----------------------------
    def make_batch(self, obs, labels, eps=None, particles: int = 1, eps_shape=None) -> L.Batch:
        """slode_batch for `obs` [B, C, T] (any strides) and the label tensors in the model's concatenation order (each [B, width] or [B],
        float32, contiguous, on the device).  eps [B, L] ([particles, B, L] for particles > 1) or None (None: drawn in-kernel from the
        handle's Philox stream, rng_seed: particle k is drawing call n + k).  ``eps_shape``: the shape a call with a noise tensor of its own
        form expects instead (``latent_attribution``: [2, num_samples, B, L]); None: the shapes above.
        The batch carries raw device pointers; it also holds the tensors they point at (``tensors``), so a label tensor converted just
        for this batch lives until the batch does -- until the step that reads it is enqueued."""
        B = obs.shape[0]
        self._f32(obs, "observations", contiguous=False)
        bt = L.Batch()
        bt.obs = obs.data_ptr()
        st = self._obs_strides(obs)
        for i in range(3):
            bt.obs_strides[i] = st[i]
        if len(labels) > L.MAX_LABELS:
            raise ValueError("at most %d label tensors, got %d" % (L.MAX_LABELS, len(labels)))
        cols = 0
        for i, t in enumerate(labels):
            self._f32(t, "label %d" % i)
            if t.shape[0] != B:
                raise ValueError("label %d has %d rows, the batch %d" % (i, t.shape[0], B))
            w = t.numel() // B
            bt.labels[i], bt.label_width[i] = t.data_ptr(), w
            cols += w
        if labels and cols != self.spec.n_u:
            raise ValueError("the label tensors have %d columns in all, the model's u has %d" % (cols, self.spec.n_u))
        bt.n_labels = len(labels)
        if eps is not None:
            self._f32(eps, "eps")
            want = self._eps_shape(B, int(particles)) if eps_shape is None else tuple(int(n) for n in eps_shape)
            if tuple(eps.shape) != want:
                raise ValueError("eps must be %s, got %s" % (list(want), tuple(eps.shape)))
            bt.eps = eps.data_ptr()
        bt.tensors = (obs, *labels, eps)
        return bt

    def _batch_call(self, fn, params, batch: L.Batch, B: int, particles: int, *args, kind=None, last=()):
        """The call every entry point that takes a slode_batch makes: the workspace of (B, particles), the fold guard, then
        ``fn(handle, shape, layout, [kind,] params, times, stage_t, batch, *args, workspace, bytes, *last, stream)``, checked."""
        ws = self.workspace(B, particles)
        self._guard(params, ws)
        _check(self.lib, self.handle, fn(
            self.handle, C.byref(self.shape(B, particles)), C.byref(self.layout), *(() if kind is None else (int(kind),)), self._p(params),
            self._p(self._times), self._p(self._stage_t), C.byref(batch), *args, self._p(ws), ws.numel() * 4, *last, self._stream()))

    def _out(self, t, name: str, shp):
        """The output tensor ``t`` of an eval-side call: a float32 device tensor of shape ``shp``, allocated when None."""
        if t is None:
            return torch.empty(shp, dtype=torch.float32, device=self.device)
        if tuple(self._f32(t, name).shape) != tuple(shp):
            raise ValueError("%s must be %s, got %s" % (name, list(shp), tuple(t.shape)))
        return t

    def _adam_args(self, params, adam):
        """slode_adam of ``adam`` = (exp_avg, exp_avg_sq, lr, step, betas, eps), by reference; None: no fused update."""
        if adam is None:
            return None
        m, v, lr, step, betas, aeps = adam
        return C.byref(L.AdamArgs(params.numel(), m.data_ptr(), v.data_ptr(), float(lr), float(betas[0]), float(betas[1]), float(aeps), int(step)))

    def svi_step(self, kind: int, params, batch: L.Batch, B: int, loss_out, grads=None, adam=None, particles: int = 1):
        """slode_svi_step: kind L.SVI_MAIN | L.SVI_AUX; adam = (exp_avg, exp_avg_sq, lr, step, betas, eps) or None; particles = K: the mean
        loss and mean gradient of K particles in the same one call (the batch's eps, if given, is [K, B, L])."""
        self._batch_call(self.lib.slode_svi_step, params, batch, B, particles, self._p(loss_out), self._p(grads), kind=kind,
                         last=(self._adam_args(params, adam),))
        return loss_out

    def eval_stats(self, params, batch: L.Batch, B: int, is_post: bool, out, particles: int = 1):
        """slode_eval_stats: the statistics row of one batch -- [-ELBO main, auxiliary loss, sum |centre curve - observation|, hits of label
        head 0..3 (spec.aux_heads order), B] -- into ``out`` (float32 [L.EVAL_SLOTS], device), enqueued on the current stream: no
        synchronisation, no read-back.  Four latent draws per trajectory (main, auxiliary, recon, labels): the batch's eps is [4, B, L] or
        None (drawing calls n .. n + 3 of the generator).  Raises SlodeError naming the reason for what the fused kernel does not take
        (adaptive solver, ``particles`` > 1, strided observations, measured arms): nothing is launched and no draw is consumed then."""
        if out.numel() != L.EVAL_SLOTS:
            raise ValueError("out must hold %d floats, got %d" % (L.EVAL_SLOTS, out.numel()))
        self._batch_call(self.lib.slode_eval_stats, params, batch, B, particles, 1 if is_post else 0, self._p(self._f32(out, "out")))
        return out

    def recon_moments(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, mean=None, sd=None, particles: int = 1):
        """slode_recon_moments: per trajectory, the mean and the population sd (np.std) over ``num_samples`` latent draws of every decoder
        head curve -- ``(mean, sd)``, each float32 [Q, B, C, T] with q in the layout's head order (ALD: mu_50, mu_75, mu_25; Gauss: mean)
        -- enqueued on the current stream; nothing sized num_samples x B x C x T exists anywhere.  The batch's eps is
        [num_samples, B, L] or None (ONE drawing call of the generator: row k * B + b is draw k of trajectory b, what
        ``draw_normal(num_samples * B).view(num_samples, B, L)`` yields).  Raises SlodeError naming the reason for what the kernel does not
        take (adaptive solver, ``particles`` > 1, strided posterior observations, measured arms, num_samples < 1, LDS budget): nothing is
        launched and no draw is consumed then."""
        shp = self._head_shape(B)
        mean, sd = self._out(mean, "mean", shp), self._out(sd, "sd", shp)
        self._batch_call(self.lib.slode_recon_moments, params, batch, B, particles, 1 if is_post else 0, int(num_samples), self._p(mean), self._p(sd))
        return mean, sd

    # ---- forecast: the output grid is the call's own argument -------------------------------------------------------------------
    def forecast_grid(self, times_out: torch.Tensor):
        """``(times, stage table)`` on the device for an output grid of any length in [2, L.FORECAST_MAX_T]: monotonicity checked as
        ``set_times`` checks it, the stage table built by ``slode_stage_times_n``; cached per tensor (identity and version)."""
        cache = self.__dict__.setdefault("_fgrids", {})
        key = (id(times_out), times_out._version)
        hit = cache.get(key)
        if hit is not None and hit[0] is times_out:
            return hit[1], hit[2]
        tt = self._f32(times_out.detach().to(self.device, torch.float32).contiguous().reshape(-1), "times_out")
        n = tt.numel()
        if n < 2 or n > L.FORECAST_MAX_T:
            raise ValueError("times_out has %d points, outside [2, %d]" % (n, L.FORECAST_MAX_T))
        self._check_grid(tt)
        ns = int(self.lib.slode_num_stage_times_n(C.byref(self.shape(1)), n))
        if ns < 1:
            _check(self.lib, None, -1)
        st = torch.empty(ns, dtype=torch.float32, device=self.device)
        _check(self.lib, self.handle, self.lib.slode_stage_times_n(self.handle, C.byref(self.shape(1)), n, self._p(tt), self._p(st), self._stream()))
        if len(cache) >= 8:
            cache.clear()
        cache[key] = (times_out, tt, st)
        return tt, st

    def forecast_plan(self, B: int, T_out: int, num_samples: int, states: bool = False, window: int = 0):
        """``slode_forecast_plan``: (steps per window, dynamic LDS bytes) of ``forecast_moments`` for these sizes; host arithmetic only."""
        w, nbytes = C.c_int(0), C.c_size_t(0)
        _check(self.lib, None, self.lib.slode_forecast_plan(C.byref(self.shape(B)), int(T_out), int(num_samples), 1 if states else 0, int(window),
                                                            C.byref(w), C.byref(nbytes)))
        return int(w.value), int(nbytes.value)

    def forecast_moments(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, times_out, mean=None, sd=None, x_mean=None,
                         x_sd=None, states: bool = False, window: int = 0):
        """slode_forecast_moments: the draws of ``recon_moments``, solved on ``times_out`` (any length in [2, L.FORECAST_MAX_T], beginning at
        the bound grid's first time) instead of the bound grid: ``(mean, sd, x_mean, x_sd)`` -- mean / population sd over ``num_samples``
        draws of every head curve, float32 [Q, B, C, T_out], and of the ODE state, float32 [B, S, T_out] (None, None unless ``states`` or
        a state tensor is given).  ``window``: grid steps solved per pass, 0 = the library's choice (``forecast_plan``).  Enqueued on the
        current stream; nothing sized num_samples x B x C x T_out exists anywhere.  The batch's eps is [num_samples, B, L] or None (ONE
        drawing call, as ``recon_moments``).  Raises SlodeError naming the reason for what the kernel does not take (everything
        ``recon_moments`` refuses but its LDS budget; a bad T_out; a window that does not fit): nothing is launched or drawn then."""
        tt, st = self.forecast_grid(times_out)
        T_out = tt.numel()
        shp = self._head_shape(B, T_out)
        mean, sd = self._out(mean, "mean", shp), self._out(sd, "sd", shp)
        if states or x_mean is not None or x_sd is not None:
            xs = (B, self.spec.ode_state_dim, T_out)
            x_mean, x_sd = self._out(x_mean, "x_mean", xs), self._out(x_sd, "x_sd", xs)
        self._batch_call(self.lib.slode_forecast_moments, params, batch, B, 1, 1 if is_post else 0, int(num_samples), self._p(tt), self._p(st),
                         T_out, int(window), self._p(mean), self._p(sd), self._p(x_mean), self._p(x_sd))
        return mean, sd, x_mean, x_sd

    def forecast_summary_plan(self, T_out: int, window: int = 0):
        """``slode_forecast_summary_plan``: (steps per window, dynamic LDS bytes) of ``forecast_summary`` for an output grid of ``T_out``
        points; host arithmetic only.  Neither the batch size nor the draw count enters."""
        w, nbytes = C.c_int(0), C.c_size_t(0)
        _check(self.lib, None, self.lib.slode_forecast_summary_plan(C.byref(self.shape(1)), int(T_out), int(window), C.byref(w), C.byref(nbytes)))
        return int(w.value), int(nbytes.value)

    def forecast_summary(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, times_out, first_point: int = 0, thr=None,
                         sense: int = 1, mean=None, sd=None, window: int = 0):
        """slode_forecast_summary: the ``L.SUMMARY_SLOTS`` functionals ``L.SUMMARY_NAMES`` of ``curve_summary``, taken on
        ``times_out[first_point:]`` of every draw's curve as ``forecast_moments`` solves it (the draws of ``recon_moments`` on the same side
        and noise; ``times_out`` of any length in [2, L.FORECAST_MAX_T], beginning at the bound grid's first time).  Returns ``(mean, sd)``:
        ``mean`` float32 [Q, B, C, 8] (None: allocated) and ``sd`` likewise (None = not computed, True = allocated, or the tensor to write).
        ``thr``: None (slots 5 - 7 are NaN) or C floats read on the host now; ``sense``: +1 (beyond: above ``thr``) or -1 (below).  ``t_hit``
        takes the crossing draws only -- a draw already beyond at ``first_point`` hits there -- and is NaN where none crosses.  ``window``:
        grid steps solved per pass, 0 = the library's choice (``forecast_summary_plan``).  Enqueued on the current stream; nothing sized by
        num_samples or by T_out exists anywhere.  The batch's eps is [num_samples, B, L] or None (ONE drawing call).  Raises SlodeError naming
        the reason for what the kernel does not take (everything ``forecast_moments`` refuses up to its grid; ``first_point`` outside
        [0, T_out - 1]; ``sense``; a non-finite threshold; a window that does not fit): nothing is launched or drawn then."""
        tt, st = self.forecast_grid(times_out)
        T_out = tt.numel()
        Q, _, Cn, _ = self._head_shape(B)
        mean = self._out(mean, "mean", (Q, B, Cn, L.SUMMARY_SLOTS))
        sd = None if sd is None else self._out(None if sd is True else sd, "sd", (Q, B, Cn, L.SUMMARY_SLOTS))
        arr = None
        if thr is not None:
            vals = [float(v) for v in (thr.detach().cpu().reshape(-1).tolist() if isinstance(thr, torch.Tensor) else thr)]
            if len(vals) != Cn:
                raise ValueError("thr must hold %d values (one per channel), got %d" % (Cn, len(vals)))
            arr = (C.c_float * Cn)(*vals)
        self._batch_call(self.lib.slode_forecast_summary, params, batch, B, 1, 1 if is_post else 0, int(num_samples), self._p(tt), self._p(st),
                         T_out, int(first_point), int(window), arr, int(sense), self._p(mean), self._p(sd))
        return mean, sd

    # ---- cohort curves: the draws of recon_moments reduced by cohort -------------------------------------------------------------
    COHORT_OUTPUTS = ("sd", "sd_subjects", "obs_mean", "l1")

    def _plan_bytes(self, fn, B: int, *args) -> int:
        """A plan entry point whose one figure is the dynamic LDS bytes (host arithmetic only; SlodeError where it refuses)."""
        r = C.c_size_t(0)
        _check(self.lib, None, fn(C.byref(self.shape(B)), *[int(a) for a in args], C.byref(r)))
        return int(r.value)

    def _plan4(self, fn, B: int, M: int, G: int, num_samples: int, chunk: int):
        """A plan entry point of the cohort calls: (members per partial, bound on the partials, dynamic LDS bytes, scratch bytes)."""
        r, n, lds, scr = C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)
        _check(self.lib, None, fn(C.byref(self.shape(B)), int(M), int(G), int(num_samples), int(chunk), C.byref(r), C.byref(n), C.byref(lds),
                                  C.byref(scr)))
        return int(r.value), int(n.value), int(lds.value), int(scr.value)

    def _cohort_index(self, members, offsets, G):
        """The checks of the cohort index of ``cohort_moments`` / ``calibration``: (M, G)."""
        for name, t in (("members", members), ("offsets", offsets)):
            if t.device != self.device or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1:
                raise ValueError("%s must be a contiguous 1-d int32 tensor on %s" % (name, self.device))
        M, G = members.numel(), int(G)
        if offsets.numel() != G + 1:
            raise ValueError("offsets must have G + 1 = %d entries, got %d" % (G + 1, offsets.numel()))
        return M, G

    def _mask_like_obs(self, mask, batch: L.Batch, B: int):
        """The mask of ``posterior_refine`` / ``pointwise_density``: None, or float32 with the shape and the strides of the observations."""
        if mask is not None:
            self._f32(mask, "mask", contiguous=False)
            if tuple(mask.shape) != (B, self.spec.n_channels, self.T) or tuple(mask.stride()) != tuple(batch.obs_strides[i] for i in range(3)):
                raise ValueError("mask must have the shape and the strides of the observations")

    def cohort_plan(self, B: int, M: int, G: int, num_samples: int, chunk: int = 0):
        """``slode_cohort_plan``: (members per partial, bound on the partials, dynamic LDS bytes, scratch bytes) of ``cohort_moments`` for
        these sizes; host arithmetic only."""
        return self._plan4(self.lib.slode_cohort_plan, B, M, G, num_samples, chunk)

    def cohort_moments(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, members, offsets, G: int, chunk: int = 0,
                       clip_min=None, mean=None, sd=None, sd_subjects=None, obs_mean=None, l1=None, outputs=COHORT_OUTPUTS, scratch=None):
        """slode_cohort_moments: the draws of ``recon_moments`` reduced by cohort -- ``(mean, sd, sd_subjects, obs_mean, l1)``: mean,
        population sd over members x draws and population sd over the members' draw means of every head curve, float32 [Q, G, C, T]; the
        members' mean observation [G, C, T]; sum_t |obs_mean - mean[0]|, [G, C].  ``members`` int32 [M] on the device: the member
        trajectories sorted by cohort; ``offsets`` int32 [G + 1]: cohort g is members[offsets[g]:offsets[g + 1]].  ``outputs`` names the
        optional outputs to produce (the others come back None, unless a tensor is given); ``chunk``: members folded per partial, 0 = the
        library's choice (``cohort_plan``); ``clip_min``: values below it are replaced by it (None: off).  ``scratch``: a float32 device
        tensor of at least the plan's scratch bytes (allocated when None).  Enqueued on the current stream.  Raises SlodeError naming the
        reason for what the kernel does not take (everything ``recon_moments`` refuses; sizes out of range; obs_mean / l1 without dense
        observations; LDS budget): nothing is launched and no draw is consumed then."""
        M, G = self._cohort_index(members, offsets, G)
        shp = self._head_shape(G)
        mean = self._out(mean, "mean", shp)
        if sd is not None or "sd" in outputs:
            sd = self._out(sd, "sd", shp)
        if sd_subjects is not None or "sd_subjects" in outputs:
            sd_subjects = self._out(sd_subjects, "sd_subjects", shp)
        if obs_mean is not None or "obs_mean" in outputs:
            obs_mean = self._out(obs_mean, "obs_mean", shp[1:])
        if l1 is not None or "l1" in outputs:
            l1 = self._out(l1, "l1", shp[1:3])
        if scratch is None:    # (sized by the library's own arithmetic; a refusal there is raised as the call's would be)
            scratch = torch.empty((self.cohort_plan(B, M, G, max(int(num_samples), 1), chunk)[3] + 3) // 4, dtype=torch.float32, device=self.device)
        self._batch_call(self.lib.slode_cohort_moments, params, batch, B, 1, 1 if is_post else 0, int(num_samples), self._p(members),
                         self._p(offsets), M, G, int(chunk), float("-inf") if clip_min is None else float(clip_min), self._p(mean), self._p(sd),
                         self._p(sd_subjects), self._p(obs_mean), self._p(l1), self._p(self._f32(scratch, "scratch")), scratch.numel() * 4)
        return mean, sd, sd_subjects, obs_mean, l1

    # ---- calibration: the draws of recon_moments compared with the observations, counted by cohort -----------------------------------
    CALIBRATION_OUTPUTS = ("inside", "cross", "pinball", "width")

    def calibration_plan(self, B: int, M: int, G: int, num_samples: int, chunk: int = 0):
        """``slode_calibration_plan``: (members per partial, bound on the partials, dynamic LDS bytes, scratch bytes) of ``calibration`` for
        these sizes; host arithmetic only, the chunk rule of ``cohort_plan``."""
        return self._plan4(self.lib.slode_calibration_plan, B, M, G, num_samples, chunk)

    def _out_i32(self, t, name: str, shp):
        """An int32 output tensor of an eval-side call, allocated when None."""
        if t is None:
            return torch.empty(shp, dtype=torch.int32, device=self.device)
        if t.device != self.device or t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != tuple(shp):
            raise ValueError("%s must be a contiguous int32 tensor %s on %s" % (name, list(shp), self.device))
        return t

    def calibration(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, members, offsets, G: int, chunk: int = 0,
                    below=None, inside=None, cross=None, pinball=None, width=None, outputs=CALIBRATION_OUTPUTS, scratch=None):
        """slode_calibration: the three curves of every draw of ``recon_moments`` (ALD: mu_50, mu_75, mu_25; Gauss: mean, mean +- 2 s)
        against the observations, by cohort -- ``(below, inside, cross, pinball, width)``: int32 counts of (member, draw) pairs with y < v_j
        [3, G, C, T], with v_2 <= y < v_1 and with crossing curves [G, C, T]; the mean pinball loss [3, G, C] and the mean band width
        [G, C], float32.  ``members`` / ``offsets`` / ``chunk`` / ``scratch`` as ``cohort_moments``; ``outputs`` names the optional outputs
        to produce.  Enqueued on the current stream.  Raises SlodeError naming the reason for what the kernel does not take (everything
        ``cohort_moments`` refuses; no observations; LDS budget): nothing is launched and no draw is consumed then."""
        M, G = self._cohort_index(members, offsets, G)
        Cn, T = self._head_shape(G)[2:]
        below = self._out_i32(below, "below", (3, G, Cn, T))
        if inside is not None or "inside" in outputs:
            inside = self._out_i32(inside, "inside", (G, Cn, T))
        if cross is not None or "cross" in outputs:
            cross = self._out_i32(cross, "cross", (G, Cn, T))
        if pinball is not None or "pinball" in outputs:
            pinball = self._out(pinball, "pinball", (3, G, Cn))
        if width is not None or "width" in outputs:
            width = self._out(width, "width", (G, Cn))
        if scratch is None:    # (sized by the library's own arithmetic; a refusal there is raised as the call's would be)
            scratch = torch.empty((self.calibration_plan(B, M, G, max(int(num_samples), 1), chunk)[3] + 3) // 4, dtype=torch.float32, device=self.device)
        self._batch_call(self.lib.slode_calibration, params, batch, B, 1, 1 if is_post else 0, int(num_samples), self._p(members),
                         self._p(offsets), M, G, int(chunk), self._p(below), self._p(inside), self._p(cross), self._p(pinball), self._p(width),
                         self._p(self._f32(scratch, "scratch")), scratch.numel() * 4)
        return below, inside, cross, pinball, width

    def traj_bounds(self, params, batch: L.Batch, B: int, num_draws: int, bounds=None, loss_kb=None, particles: int = 1):
        """slode_traj_bounds: per trajectory, from ``num_draws`` posterior draws, ``bounds`` float32 [B, L.BOUND_SLOTS] = [-ELBO (mean of
        the per-draw losses), importance-weighted bound -log(1/K sum exp(-loss)), effective sample size of the weights, mean negative
        log-likelihood] and ``loss_kb`` float32 [num_draws, B], the per-draw losses themselves (the main loss of the single row b on draw
        k) -- ``(bounds, loss_kb)``, enqueued on the current stream: no synchronisation, no read-back.  The batch's eps is
        [num_draws, B, L] (``make_batch(..., particles=num_draws)``) or None (drawing calls n .. n + num_draws - 1 of the generator: draw
        k of trajectory b is row b of call n + k, as ``svi_step(particles=num_draws)`` draws).  Raises SlodeError naming the reason for
        what the kernel does not take (adaptive solver, ``particles`` > 1 in the shape, strided observations, SLODE_NO_FOLD, measured arms, num_draws < 1, LDS budget):
        nothing is launched and no draw is consumed then; there is no composed fallback."""
        K = int(num_draws)
        bounds = self._out(bounds, "bounds", (B, L.BOUND_SLOTS))
        loss_kb = self._out(loss_kb, "loss_kb", (max(K, 0), B))
        self._batch_call(self.lib.slode_traj_bounds, params, batch, B, particles, K, self._p(bounds), self._p(loss_kb))
        return bounds, loss_kb

    def label_evidence(self, params, batch: L.Batch, B: int, num_draws: int, hyp_labels, V: int, log_prior=None, evidence=None, best=None,
                       loss_vkb=None, particles: int = 1):
        """slode_label_evidence: ``V`` label hypotheses scored on the ``num_draws`` posterior draws of every trajectory in one call --
        ``(evidence, best, loss_vkb)``: ``evidence`` float32 [B, V, L.EVIDENCE_SLOTS] = [-ELBO under hypothesis v, importance-weighted bound
        on -log p(x_b | u_v), effective sample size of its weights, log posterior over v], ``best`` int32 [B], the arg-max of the log
        posterior (lowest index on a tie), ``loss_vkb`` float32 [V, num_draws, B], the per-draw losses; enqueued on the current stream.
        ``hyp_labels``: one entry per label tensor of ``make_batch``: a float32 [V, width] table shared by all trajectories, or None (the
        label is not hypothesised: every hypothesis keeps the trajectory's own).  ``log_prior``: float32 [V] on the device, or None
        (uniform).  Slots 0-2 of column v and ``loss_vkb[v]`` are bitwise what ``traj_bounds`` returns on the batch with those labels and
        the same noise (the batch's eps: as ``traj_bounds``).  Raises SlodeError naming the reason for what the kernel does not take
        (everything ``traj_bounds`` refuses; V outside [1, L.EVIDENCE_MAX_V]; no hypothesised label; LDS budget): nothing is launched and no
        draw is consumed then; there is no composed fallback."""
        K, V = int(num_draws), int(V)
        if hyp_labels is None or len(hyp_labels) != int(batch.n_labels):
            raise ValueError("hyp_labels needs one entry per label tensor of the batch (%d), got %s"
                             % (int(batch.n_labels), "None" if hyp_labels is None else len(hyp_labels)))
        ptrs = (C.c_void_p * L.MAX_LABELS)()
        for i, t in enumerate(hyp_labels):
            if t is None:
                continue
            if self._f32(t, "hyp label %d" % i).numel() != V * int(batch.label_width[i]):
                raise ValueError("hyp label %d must be [%d, %d], got %s" % (i, V, int(batch.label_width[i]), tuple(t.shape)))
            ptrs[i] = t.data_ptr()
        if log_prior is not None and self._f32(log_prior, "log_prior").numel() != V:
            raise ValueError("log_prior must hold V = %d values, got %s" % (V, tuple(log_prior.shape)))
        evidence = self._out(evidence, "evidence", (B, max(V, 0), L.EVIDENCE_SLOTS))
        best = self._out_i32(best, "best", (B,))
        loss_vkb = self._out(loss_vkb, "loss_vkb", (max(V, 0), max(K, 0), B))
        self._batch_call(self.lib.slode_label_evidence, params, batch, B, particles, K, ptrs, V, self._p(log_prior), self._p(evidence),
                         self._p(best), self._p(loss_vkb))
        return evidence, best, loss_vkb

    def posterior_refine(self, params, batch: L.Batch, B: int, num_draws: int, num_steps: int, lr: float = 0.05, mask=None, loc=None, scale=None,
                         elbo=None, grad0=None, trace=None, best_step=None, particles: int = 1):
        """slode_posterior_refine: every trajectory takes ``num_steps`` Adam steps (``lr``, beta = (0.9, 0.999), eps 1e-8, bias correction)
        on its own (loc, log scale), starting from the encoder's, against its own -ELBO over ``num_draws`` noise rows that stay fixed for
        the whole call, all inside one kernel -- ``(loc, scale, elbo, grad0, trace, best_step)``: the best iterate float32 [B, L] twice,
        ``elbo`` [B, 2] = (the -ELBO at the encoder's posterior, the best one: never larger), ``grad0`` [B, 2 L] = the gradient at the
        encoder's posterior with respect to (loc, log scale), ``trace`` [num_steps + 1, B] = the -ELBO of every iterate, ``best_step`` int32
        [B] (``grad0`` / ``trace`` / ``best_step`` passed as False are not computed: None in their place).  ``mask``: float32 weights >= 0
        of the likelihood terms, a tensor with the shape AND strides of the observations, or None (all 1; bitwise what an all-ones mask
        gives); the encoder still reads every observation.  The batch's eps is [num_draws, B, L] (``make_batch(..., particles=num_draws)``)
        or None (drawing calls n .. n + num_draws - 1, as ``traj_bounds``: the counter advances by num_draws, not by num_draws x num_steps).
        Enqueued on the current stream.  Raises SlodeError naming the reason for what the kernel does not take (everything ``traj_bounds``
        refuses; num_steps < 0; lr not finite and positive; a family whose main loss scores the labels: proc; LDS budget): nothing is
        launched and no draw is consumed then; there is no composed fallback."""
        K, J, Ld = int(num_draws), int(num_steps), self.spec.latent_dim
        self._mask_like_obs(mask, batch, B)
        loc, scale = self._out(loc, "loc", (B, Ld)), self._out(scale, "scale", (B, Ld))
        elbo = self._out(elbo, "elbo", (B, 2))
        grad0 = None if grad0 is False else self._out(grad0, "grad0", (B, 2 * Ld))
        trace = None if trace is False else self._out(trace, "trace", (max(J, 0) + 1, B))
        best_step = None if best_step is False else self._out_i32(best_step, "best_step", (B,))
        self._batch_call(self.lib.slode_posterior_refine, params, batch, B, particles, K, J, float(lr), self._p(mask), self._p(loc),
                         self._p(scale), self._p(elbo), self._p(grad0), self._p(trace), self._p(best_step))
        return loc, scale, elbo, grad0, trace, best_step

    def pointwise_plan(self, B: int, num_draws: int, weights: int) -> int:
        """``slode_pointwise_plan``: the dynamic LDS bytes of ``pointwise_density`` for this shape (host arithmetic only; raises SlodeError
        where the call would refuse them at its LDS rung)."""
        return self._plan_bytes(self.lib.slode_pointwise_plan, B, num_draws, weights)

    def pointwise_density(self, params, batch: L.Batch, B: int, num_draws: int, weights: int, mask=None, loc=None, scale=None, point=None,
                          summary=None, loss_kb=None, particles: int = 1):
        """slode_pointwise_density: per observation point (c, t), over ``num_draws`` posterior draws with normalised weights w_k, the log of
        the mean density, the mean and the variance of the log density -- ``(point, summary, loss_kb)``: ``point`` float32 [3, B, C, T] =
        lppd | mean_ll | var_ll (the WAIC penalty), ``summary`` float32 [B, L.POINTWISE_SLOTS] = [sum_in lppd, sum_in var_ll, sum_in
        mean_ll, n_in, sum_out lppd, sum_out mean_ll, n_out, ESS of the weights], ``loss_kb`` float32 [num_draws, B] in importance mode
        (None in posterior mode, or when passed as False).  ``weights``: L.PW_POSTERIOR (w_k = 1 / K) or L.PW_IMPORTANCE (w_k ~
        exp(-loss_k), the per-draw losses of ``traj_bounds`` with the mask on their likelihood terms).  ``mask``: float32 weights >= 0, a
        tensor with the shape AND strides of the observations, or None (all 1): which points count as observed -- the in / out partition
        of the sums, and in importance mode the weights of the likelihood terms of loss_k; the planes are written for every point.
        ``loc`` / ``scale``: float32 [B, L] each, both or neither -- the posterior the draws come from (``posterior_refine``'s output);
        None: the encoder's.  The batch's eps: as ``traj_bounds`` ([num_draws, B, L], or None: the counter advances by num_draws).
        Enqueued on the current stream.  Raises SlodeError naming the reason for what the kernel does not take (everything ``traj_bounds``
        refuses; weights outside {0, 1}; one of loc / scale alone; loss_kb in posterior mode; LDS budget): nothing is launched and no draw
        is consumed then; there is no composed fallback."""
        K, Ld, Cn = int(num_draws), self.spec.latent_dim, self.spec.n_channels
        self._mask_like_obs(mask, batch, B)
        for name, t in (("loc", loc), ("scale", scale)):
            if t is not None and tuple(self._f32(t, name).shape) != (B, Ld):
                raise ValueError("%s must be [%d, %d], got %s" % (name, B, Ld, tuple(t.shape)))
        point = self._out(point, "point", (3, B, Cn, self.T))
        summary = self._out(summary, "summary", (B, L.POINTWISE_SLOTS))
        if loss_kb is False or (loss_kb is None and int(weights) != L.PW_IMPORTANCE):
            loss_kb = None
        else:
            loss_kb = self._out(loss_kb, "loss_kb", (max(K, 0), B))
        self._batch_call(self.lib.slode_pointwise_density, params, batch, B, particles, K, int(weights), self._p(mask), self._p(loc),
                         self._p(scale), self._p(point), self._p(summary), self._p(loss_kb))
        return point, summary, loss_kb

    def loo_plan(self, B: int, num_draws: int, tile: int = 0):
        """``slode_loo_plan``: ``(tile, sweeps, depth, lds_bytes)`` of ``pointwise_loo`` for this shape and draw count -- time points per
        sweep over the draws, the number of sweeps, the depth M + 1 of the kept sorted tail (M = min(ceil(min(0.2 K, 3 sqrt K)), K - 1))
        and the dynamic LDS bytes; host arithmetic only.  ``tile`` = 0: the fewest sweeps that fit.  Raises SlodeError where the call
        would refuse them at its own rungs."""
        t, sw, d, lds = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
        _check(self.lib, None, self.lib.slode_loo_plan(C.byref(self.shape(B)), int(num_draws), int(tile), C.byref(t), C.byref(sw), C.byref(d),
                                                       C.byref(lds)))
        return int(t.value), int(sw.value), int(d.value), int(lds.value)

    def pointwise_loo(self, params, batch: L.Batch, B: int, num_draws: int, mask=None, loc=None, scale=None, tile: int = 0, point=None,
                      summary=None, tail=None, particles: int = 1):
        """slode_pointwise_loo: Pareto-smoothed importance-sampling leave-one-out from the ``num_draws`` posterior draws of
        ``pointwise_density`` (posterior weights) -- ``(point, summary, tail)``: ``point`` float32 [3, B, C, T] = elpd_loo | khat | lppd
        (``lppd`` bit for bit ``pointwise_density``'s plane 0; ``khat`` = +inf where no smoothing was possible), ``summary`` float32 [B,
        L.LOO_SLOTS] = [sum_in elpd_loo, sum_in lppd, n_in, the number of points in with khat > 0.7, their largest khat, sum_out
        elpd_loo, sum_out lppd, n_out], ``tail`` float32 [M + 1, B, C, T], the kept smallest per-draw log-densities of every point,
        ascending (``tail=True``: allocated; a tensor: written; None: not produced).  ``mask`` / ``loc`` / ``scale`` / the batch's eps:
        as ``pointwise_density``; the counter advances by num_draws whatever the number of sweeps.  ``tile``: time points per sweep (0:
        the library's choice, ``loo_plan``); no output bit depends on it.  Enqueued on the current stream.  Raises SlodeError naming the
        reason for what the kernel does not take (everything ``pointwise_density`` refuses in posterior mode; one of loc / scale alone;
        tile outside [0, T]; a draw count whose tables do not fit the LDS): nothing is launched and no draw is consumed then."""
        K, Ld, Cn = int(num_draws), self.spec.latent_dim, self.spec.n_channels
        self._mask_like_obs(mask, batch, B)
        for name, t in (("loc", loc), ("scale", scale)):
            if t is not None and tuple(self._f32(t, name).shape) != (B, Ld):
                raise ValueError("%s must be [%d, %d], got %s" % (name, B, Ld, tuple(t.shape)))
        point = self._out(point, "point", (3, B, Cn, self.T))
        summary = self._out(summary, "summary", (B, L.LOO_SLOTS))
        if tail is not None and tail is not False:
            tail = self._out(None if tail is True else tail, "tail", (self.loo_plan(B, K, tile)[2], B, Cn, self.T))
        else:
            tail = None
        self._batch_call(self.lib.slode_pointwise_loo, params, batch, B, particles, K, self._p(mask), self._p(loc), self._p(scale), int(tile),
                         self._p(point), self._p(summary), self._p(tail))
        return point, summary, tail

    def intervene_moments(self, params, batch: L.Batch, B: int, cf_labels, group_mask: int, num_samples: int, cf_mean=None, cf_sd=None,
                          eff_mean=None, eff_sd=None, particles: int = 1):
        """slode_intervene_moments: counterfactual curves from ``num_samples`` paired posterior draws per trajectory.  Both arms of a draw
        share one noise row: the factual latent is the posterior draw of ``recon_moments(is_post=True)``; the counterfactual latent replaces
        the dims of every prior group g with bit g of ``group_mask`` set by that group's conditional prior on ``cf_labels``, driven by the
        same noise.  Returns ``(cf_mean, cf_sd, eff_mean, eff_sd)``, each float32 [Q, B, C, T] in the head order of ``recon_moments``: mean /
        population sd of the counterfactual curve and of the paired difference counterfactual - factual (an output passed as False is not computed: None in its place); enqueued on the current
        stream, nothing sized num_samples x B x C x T exists anywhere.  ``cf_labels``: the label tensors of ``make_batch`` once more, with the
        counterfactual values (an entry no intervened group reads may be None, one that an intervened group reads raises ValueError; None
        altogether with ``group_mask`` = 0).  The batch's eps is
        [num_samples, B, L] or None (ONE drawing call: row k * B + b is draw k of trajectory b).  Raises SlodeError naming the reason for what
        the kernel does not take (everything ``recon_moments(is_post=True)`` refuses; mask bits beyond the prior groups; a non-zero mask
        without counterfactual labels): nothing is launched and no draw is consumed then."""
        sp = self.spec
        shp = self._head_shape(B)
        # (an output passed as False is not wanted: NULL in the C call, None in the result)
        outs = [None if t is False else self._out(t, name, shp)
                for t, name in ((cf_mean, "cf_mean"), (cf_sd, "cf_sd"), (eff_mean, "eff_mean"), (eff_sd, "eff_sd"))]
        ptrs = None
        if cf_labels is not None:
            if len(cf_labels) != int(batch.n_labels):
                raise ValueError("cf_labels has %d entries, the batch %d label tensors" % (len(cf_labels), int(batch.n_labels)))
            ptrs = (C.c_void_p * L.MAX_LABELS)()
            groups = [g for i, g in enumerate(sp.prior_groups) if (int(group_mask) >> i) & 1]
            col = 0
            for i, t in enumerate(cf_labels):
                lo, col = col, col + int(batch.label_width[i])
                if t is None:                   # an argument error of the caller, not a configuration the kernel does not take
                    reader = [g.prefix for g in groups if lo < g.u_off + g.u_dim and col > g.u_off]
                    if reader:
                        raise ValueError("cf label %d is None, but the intervened prior group %s (group_mask = 0x%x) reads its label columns "
                                         "[%d, %d): pass every label tensor of an intervened group" % (i, reader[0], int(group_mask), lo, col))
                    continue
                if self._f32(t, "cf label %d" % i).numel() != B * int(batch.label_width[i]):
                    raise ValueError("cf label %d must be [%d, %d], got %s" % (i, B, int(batch.label_width[i]), tuple(t.shape)))
                ptrs[i] = t.data_ptr()
        self._batch_call(self.lib.slode_intervene_moments, params, batch, B, particles, ptrs, int(group_mask), int(num_samples),
                         *(self._p(t) for t in outs))
        return tuple(outs)

    # ---- latent attribution: per-block variance shares of the curves from pick-freeze draws -------------------------------------------
    def attribution_blocks(self) -> int:
        """The number of latent blocks of the spec: its prior groups, plus the rest block (bit ``len(prior_groups)`` of a mask) when some
        latent dim lies in no group."""
        sp = self.spec
        covered = sum(g.z_dim for g in sp.prior_groups)
        return len(sp.prior_groups) + (1 if covered < sp.latent_dim else 0)

    def attribution_plan(self, B: int, n_arms: int) -> int:
        """``slode_attribution_plan``: the dynamic LDS bytes of ``latent_attribution`` for this shape and ``n_arms`` arms (host arithmetic
        only; raises SlodeError where the call would refuse them at its LDS rung, or for n_arms outside [1, L.ATTRIBUTION_MAX_ARMS])."""
        return self._plan_bytes(self.lib.slode_attribution_plan, B, n_arms)

    def latent_attribution(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, arm_masks, mean=None, sd=None, msd=None,
                           particles: int = 1):
        """slode_latent_attribution: pick-freeze draws per trajectory -- the base draw of ``recon_moments`` on the same side, and per arm a
        the same draw with the latent blocks of ``arm_masks[a]`` redrawn on a second noise row (bit g: prior group g of the spec; bit
        ``len(prior_groups)``: the rest dims no group covers).  Returns ``(mean, sd, msd)``: mean / population sd of the base curve, float32
        [Q, B, C, T] each in the head order of ``recon_moments`` (either passed as False is not computed: None in its place), and ``msd``
        float32 [n_arms, Q, B, C, T] = 1 / (2 num_samples) sum_k (v_a,k - v_k)^2 (a mask of 0 gives exactly 0); enqueued on the current
        stream, nothing sized num_samples x B x C x T exists anywhere.  The batch's eps is [2, num_samples, B, L] (base, then fresh:
        ``make_batch(..., eps_shape=...)``) or None (drawing calls n and n + 1 of the generator, row k * B + b each; the counter moves by
        two).  Raises SlodeError naming the reason for what the kernel does not take (everything ``recon_moments`` refuses on that side;
        n_arms outside [1, L.ATTRIBUTION_MAX_ARMS]; mask bits beyond the blocks; LDS budget): nothing is launched and no draw is consumed
        then."""
        masks = [int(m) for m in arm_masks]
        A = len(masks)
        shp = self._head_shape(B)
        mean, sd = (None if t is False else self._out(t, name, shp) for t, name in ((mean, "mean"), (sd, "sd")))
        msd = self._out(msd, "msd", (max(A, 0),) + tuple(shp))
        arr = (C.c_uint * max(A, 1))(*[m & 0xFFFFFFFF for m in masks])
        self._batch_call(self.lib.slode_latent_attribution, params, batch, B, particles, 1 if is_post else 0, int(num_samples), arr, A,
                         self._p(mean), self._p(sd), self._p(msd))
        return mean, sd, msd

    # ---- curve summaries: peak, time to peak, area and threshold crossing of every draw's curve -----------------------------------------
    def curve_summary_plan(self, B: int, want_p_beyond: bool) -> int:
        """``slode_curve_summary_plan``: the dynamic LDS bytes of ``curve_summary`` for this shape, with or without the counters of
        ``p_beyond`` (host arithmetic only; raises SlodeError where the call would refuse them at its LDS rung)."""
        return self._plan_bytes(self.lib.slode_curve_summary_plan, B, bool(want_p_beyond))

    def curve_summary(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, thr, sense: int, mean, sd=None, p_beyond=None,
                      particles: int = 1):
        """slode_curve_summary: per trajectory, head curve and channel, the mean and the population sd over ``num_samples`` latent draws (those
        of ``recon_moments`` on the same side and noise) of the ``L.SUMMARY_SLOTS`` functionals ``L.SUMMARY_NAMES`` of every draw's whole curve.
        Returns ``(mean, sd, p_beyond)``: ``mean`` float32 [Q, B, C, 8] (None: allocated), ``sd`` likewise and ``p_beyond`` float32
        [Q, B, C, T], the share of draws beyond the threshold at every point (each: None = not computed, True = allocated, or the tensor to
        write).  ``thr``: None (slots 5 - 7 are NaN; ``p_beyond`` is refused) or C floats read on the host now; ``sense``: +1 (beyond: above
        ``thr``) or -1 (below).  ``t_hit`` (slot 6) takes the crossing draws only and is NaN where none crosses.  Enqueued on the current
        stream; nothing sized num_samples x B x C x T exists anywhere.  Raises SlodeError naming the reason for what the kernel does not take
        (everything ``recon_moments`` refuses on that side; ``sense``; a non-finite threshold; ``p_beyond`` without one; LDS budget): nothing
        is launched and no draw is consumed then."""
        Q, _, Cn, T = self._head_shape(B)
        mean = self._out(mean, "mean", (Q, B, Cn, L.SUMMARY_SLOTS))
        sd = None if sd is None else self._out(None if sd is True else sd, "sd", (Q, B, Cn, L.SUMMARY_SLOTS))
        p_beyond = None if p_beyond is None else self._out(None if p_beyond is True else p_beyond, "p_beyond", (Q, B, Cn, T))
        arr = None
        if thr is not None:
            vals = [float(v) for v in (thr.detach().cpu().reshape(-1).tolist() if isinstance(thr, torch.Tensor) else thr)]
            if len(vals) != Cn:
                raise ValueError("thr must hold %d values (one per channel), got %d" % (Cn, len(vals)))
            arr = (C.c_float * Cn)(*vals)
        self._batch_call(self.lib.slode_curve_summary, params, batch, B, particles, 1 if is_post else 0, int(num_samples), arr, int(sense),
                         self._p(mean), self._p(sd), self._p(p_beyond))
        return mean, sd, p_beyond

    # ---- counterfactual summaries: the curve functionals of every subject under V hypothesised inputs, with the paired effects ------------
    def intervene_summary_plan(self, B: int, V: int) -> int:
        """``slode_intervene_summary_plan``: the dynamic LDS bytes of ``intervene_summary`` for this shape and ``V`` arms (host arithmetic
        only; raises SlodeError, naming the largest V that fits, where the call would refuse them at its V or LDS rung)."""
        return self._plan_bytes(self.lib.slode_intervene_summary_plan, B, V)

    def intervene_summary(self, params, batch: L.Batch, B: int, hyp_labels, V: int, group_mask: int, num_samples: int, thr, sense: int,
                          f_mean=None, f_sd=None, cf_mean=None, cf_sd=None, eff_mean=None, eff_sd=None, particles: int = 1):
        """slode_intervene_summary: the ``L.SUMMARY_SLOTS`` curve functionals ``L.SUMMARY_NAMES`` of ``curve_summary`` on ``num_samples``
        PAIRED posterior draws per trajectory, for the subject's own curve and for its curve under each of ``V`` hypothesised inputs.  All
        V + 1 arms of a draw share one noise row: the factual latent is the posterior draw of ``curve_summary(is_post=True)``; arm v
        replaces the dims of every prior group g with bit g of ``group_mask`` set by that group's conditional prior on the trajectory's
        own labels with the columns of every hypothesised tensor replaced by row v of its table, as ``intervene_moments`` forms it.
        ``hyp_labels``: one entry per label tensor of ``make_batch``: a float32 [V, width] table shared by all trajectories, or None (not
        hypothesised); None altogether with ``group_mask`` = 0.  Returns ``(f_mean, f_sd, cf_mean, cf_sd, eff_mean, eff_sd)``: the
        factual moments float32 [Q, B, C, 8] (bitwise ``curve_summary``'s on the same noise), those of every arm and of the paired
        difference arm - factual float32 [V, Q, B, C, 8] (an output passed as False is not computed: None in its place; with both factual
        and both effect outputs False the factual arm is not run).  Slot 6 of an arm takes its crossing draws, of an effect the draws
        that cross in both arms (NaN where there is none); slot 7 of an effect is the change of P(cross).  ``thr``: None (slots 5 - 7 are
        NaN) or C floats read on the host now; ``sense``: +1 / -1.  The batch's eps is [num_samples, B, L] or None (ONE drawing call).
        Column v does not depend on V or on the other rows.  Raises SlodeError naming the reason for what the kernel does not take
        (everything ``recon_moments(is_post=True)`` refuses; V outside [1, L.INTERVENE_SUMMARY_MAX_ARMS]; ``sense``; a non-finite
        threshold; mask bits beyond the prior groups; a non-zero mask without a hypothesised column one of its groups reads; LDS budget,
        naming the largest V that fits): nothing is launched and no draw is consumed then."""
        V = int(V)
        Q, _, Cn, _ = self._head_shape(B)
        shp_f, shp_v = (Q, B, Cn, L.SUMMARY_SLOTS), (max(V, 1), Q, B, Cn, L.SUMMARY_SLOTS)     # (V < 1 is refused by name: the pointers must not be NULL for it)
        if cf_mean is False:
            raise ValueError("cf_mean is always computed")
        outs = [None if t is False else self._out(t, name, shp)
                for t, name, shp in ((f_mean, "f_mean", shp_f), (f_sd, "f_sd", shp_f), (cf_mean, "cf_mean", shp_v), (cf_sd, "cf_sd", shp_v),
                                     (eff_mean, "eff_mean", shp_v), (eff_sd, "eff_sd", shp_v))]
        ptrs = None
        if hyp_labels is not None:
            if len(hyp_labels) != int(batch.n_labels):
                raise ValueError("hyp_labels needs one entry per label tensor of the batch (%d), got %d" % (int(batch.n_labels), len(hyp_labels)))
            ptrs = (C.c_void_p * L.MAX_LABELS)()
            for i, t in enumerate(hyp_labels):
                if t is None:
                    continue
                if self._f32(t, "hyp label %d" % i).numel() != V * int(batch.label_width[i]):
                    raise ValueError("hyp label %d must be [%d, %d], got %s" % (i, V, int(batch.label_width[i]), tuple(t.shape)))
                ptrs[i] = t.data_ptr()
        arr = None
        if thr is not None:
            vals = [float(v) for v in (thr.detach().cpu().reshape(-1).tolist() if isinstance(thr, torch.Tensor) else thr)]
            if len(vals) != Cn:
                raise ValueError("thr must hold %d values (one per channel), got %d" % (Cn, len(vals)))
            arr = (C.c_float * Cn)(*vals)
        self._batch_call(self.lib.slode_intervene_summary, params, batch, B, particles, ptrs, V, int(group_mask), int(num_samples), arr, int(sense),
                         *(self._p(t) for t in outs))
        return tuple(outs)

    # ---- sample quantiles: order statistics of every curve value over the draws ------------------------------------------------------------
    @staticmethod
    def _levels(levels):
        """``levels`` (a sequence or tensor of floats) as a C array of doubles and its length."""
        vals = [float(v) for v in (levels.detach().cpu().reshape(-1).tolist() if isinstance(levels, torch.Tensor) else levels)]
        return (C.c_double * max(1, len(vals)))(*vals), len(vals)

    def quantile_plan(self, B: int, num_samples: int, levels, tile: int = 0):
        """``slode_quantile_plan``: ``(tile, sweeps, depth_lo, depth_hi, lds_bytes)`` of ``recon_quantiles`` for this shape, draw count and
        level set -- the time points per sweep, the passes over the draws, the depths of the two sorted buffers and the kernel's dynamic
        LDS bytes (host arithmetic only; raises SlodeError where the call would refuse them at its own rungs)."""
        arr, n = self._levels(levels)
        t, sw, lo, hi, nbytes = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
        _check(self.lib, None, self.lib.slode_quantile_plan(C.byref(self.shape(B)), int(num_samples), n, arr, int(tile), C.byref(t), C.byref(sw),
                                                            C.byref(lo), C.byref(hi), C.byref(nbytes)))
        return int(t.value), int(sw.value), int(lo.value), int(hi.value), int(nbytes.value)

    def recon_quantiles(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, levels, out=None, tile: int = 0, particles: int = 1):
        """slode_recon_quantiles: per trajectory, head curve, channel and time point, the sample quantiles (numpy's "linear" definition) at
        ``levels`` (at most ``L.QUANTILE_MAX_LEVELS`` values in [0, 1], any order) of the ``num_samples`` latent draws ``recon_moments``
        walks on the same side and noise: ``out`` float32 [n_levels, Q, B, C, T] (None: allocated), returned.  A level whose rank is an
        integer (0, 1, ...) is one of the draw values exactly.  ``tile``: time points per sweep over the draws, 0 = the library's choice
        (``quantile_plan``).  Enqueued on the current stream; nothing sized num_samples x B x C x T exists anywhere.  The batch's eps is
        [num_samples, B, L] or None (rows k * B + b of drawing call n; the counter moves to n + num_samples).  Raises SlodeError naming the
        reason for what the kernel does not take (everything ``recon_moments`` refuses on that side; the level count; a level outside
        [0, 1]; the tile; LDS budget): nothing is launched and no draw is consumed then."""
        arr, n = self._levels(levels)
        Q, _, Cn, T = self._head_shape(B)
        out = self._out(out, "out", (max(n, 1), Q, B, Cn, T))
        self._batch_call(self.lib.slode_recon_quantiles, params, batch, B, particles, 1 if is_post else 0, int(num_samples), n, arr, int(tile),
                         self._p(out))
        return out

    # ---- mechanism curves: moments of the state, production, degradation, set point and net rate at every grid point ---------------------
    def mechanism_plan(self, B: int, slots: int) -> int:
        """``slode_mechanism_plan``: the dynamic LDS bytes of ``mechanism_moments`` for this shape and the slot mask ``slots`` (host arithmetic
        only; raises SlodeError where the call would refuse them at its mask or LDS rung)."""
        return self._plan_bytes(self.lib.slode_mechanism_plan, B, slots)

    def mechanism_moments(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, slots: int, mean=None, sd=None):
        """slode_mechanism_moments: per trajectory, state component and grid point, the mean and the population sd over ``num_samples`` latent
        draws (those of ``recon_moments`` on the same side and noise) of the slots selected by the bit mask ``slots`` (bit i:
        ``L.MECHANISM_NAMES[i]`` -- the state x, the production a and the degradation d of dx/dt = a - d x at the grid time, the set point
        a / d, the net rate a - d x).  Returns ``(mean, sd)``: float32 [n_sel, B, S, T] each, the selected slots in increasing slot order
        (``mean``, ``sd``: None = allocated, or the tensor to write; ``sd=False``: not computed, returned as None).  Enqueued on the current
        stream; nothing sized num_samples x B x T x S exists anywhere.  Raises SlodeError naming the reason for what the kernel does not take
        (everything ``recon_moments`` refuses on that side; an empty mask or bits beyond ``L.MECHANISM_SLOTS``; LDS budget): nothing is
        launched and no draw is consumed then."""
        slots = int(slots)
        n_sel = max(1, bin(slots & ((1 << L.MECHANISM_SLOTS) - 1)).count("1"))
        shp = (n_sel, B, self.spec.ode_state_dim, self.T)
        mean = self._out(mean, "mean", shp)
        sd = None if sd is False else self._out(sd, "sd", shp)
        self._batch_call(self.lib.slode_mechanism_moments, params, batch, B, 1, 1 if is_post else 0, int(num_samples), slots & 0xffffffff,
                         self._p(mean), self._p(sd))
        return mean, sd

    # ---- simultaneous bands: the quantiles over the draws of the largest standardised deviation of a whole curve -------------------------
    def joint_band_plan(self, B: int, num_samples: int) -> int:
        """``slode_joint_band_plan``: the dynamic LDS bytes of ``joint_band`` for this shape and draw count (host arithmetic only; raises
        SlodeError where the call would refuse them at its draw-count or LDS rung)."""
        return self._plan_bytes(self.lib.slode_joint_band_plan, B, num_samples)

    def joint_band_levels(self, num_samples: int, levels):
        """``slode_joint_band_levels``: ``(ranks, z)`` of ``joint_band`` for ``num_samples`` draws as the call forms them on the host in
        fp64 -- per level p the rank r = min(K, max(1, ceil(p K - 1e-9))), counted from 1, and z = Phi^-1((1 + p) / 2) (inf at p = 1)."""
        arr, n = self._levels(levels)
        ranks, z = (C.c_int * max(1, n))(), (C.c_double * max(1, n))()
        _check(self.lib, None, self.lib.slode_joint_band_levels(int(num_samples), n, arr, ranks, z))
        return [int(v) for v in ranks[:n]], [float(v) for v in z[:n]]

    def joint_band(self, params, batch: L.Batch, B: int, is_post: bool, num_samples: int, levels, sd_floor: float = 0.0, mean=None, sd=None,
                   crit=None, joint=None, obs_dev=None, dev=None):
        """slode_joint_band: per trajectory, head curve and channel, over the ``num_samples`` = K latent draws ``recon_moments`` walks on the
        same side and noise: ``mean``, ``sd`` float32 [Q, B, C, T] (its bits), the deviations dev_k = max_t |v_k(t) - mean(t)| / sd(t) over
        the points with sd > ``sd_floor``, and per level (1 to ``L.JOINT_BAND_MAX_LEVELS`` values in (0, 1], any order) ``crit`` [Q, B, C,
        Lv], the r-th smallest deviation (``joint_band_levels``), and ``joint`` [Q, B, C, Lv], the share of draws with dev_k <= z: wholly
        inside the pointwise band.  ``obs_dev`` [Q, B, C, 2]: the observed curve's deviation and the number of participating points.
        ``dev``: None = not returned, True = allocated, or the tensor [Q, B, C, K] to write.  Returns ``(mean, sd, crit, joint, obs_dev,
        dev)``.  Enqueued on the current stream; nothing sized K x B x C x T exists anywhere.  The batch's eps is [K, B, L] or None (one
        drawing call, as ``recon_moments``).  Raises SlodeError naming the reason for what the kernel does not take (everything
        ``recon_moments`` refuses on that side; K < 2; the level count; a level outside (0, 1]; a negative or non-finite floor; LDS budget):
        nothing is launched and no draw is consumed then."""
        arr, n = self._levels(levels)
        Q, _, Cn, T = self._head_shape(B)
        mean, sd = self._out(mean, "mean", (Q, B, Cn, T)), self._out(sd, "sd", (Q, B, Cn, T))
        crit, joint = self._out(crit, "crit", (Q, B, Cn, max(n, 1))), self._out(joint, "joint", (Q, B, Cn, max(n, 1)))
        obs_dev = self._out(obs_dev, "obs_dev", (Q, B, Cn, 2))
        dev = None if dev is None else self._out(None if dev is True else dev, "dev", (Q, B, Cn, max(int(num_samples), 1)))
        self._batch_call(self.lib.slode_joint_band, params, batch, B, 1, 1 if is_post else 0, int(num_samples), n, arr, float(sd_floor),
                         self._p(mean), self._p(sd), self._p(crit), self._p(joint), self._p(obs_dev), self._p(dev))
        return mean, sd, crit, joint, obs_dev, dev

    # ---- data parallel with the small payload: grad_partial -> all-reduce(payload) -> grad_apply (include/slode.h) ------------------
    def payload_floats(self, kind: int) -> int:
        return int(self.lib.slode_grad_payload_floats(C.byref(self.shape(1)), C.byref(self.layout), int(kind)))

    def grad_partial(self, kind: int, params, batch: L.Batch, B: int, payload, particles: int = 1):
        self._batch_call(self.lib.slode_grad_partial, params, batch, B, particles, self._p(self._f32(payload, "payload")), kind=kind)

    def grad_apply(self, kind: int, params, batch: L.Batch, B: int, payload, loss_out, grads, adam=None, particles: int = 1):
        ws = self.workspace(B, particles)
        _check(self.lib, self.handle, self.lib.slode_grad_apply(
            self.handle, C.byref(self.shape(B, particles)), C.byref(self.layout), int(kind), self._p(params), batch.obs_strides, self._p(payload),
            self._p(loss_out), self._p(grads), self._p(ws), ws.numel() * 4, self._adam_args(params, adam), self._stream()))
        return loss_out

    def fold_invalidate(self):
        """Tell the engine that the parameter vector was written outside its own steps (checkpoint load, another optimizer): the next step
        folds the encoder weights again instead of trusting the fold the previous step left in the workspace (slode_fold_invalidate)."""
        _check(self.lib, self.handle, self.lib.slode_fold_invalidate(self.handle))

    def _guard(self, params, ws):
        """torch-side writes to the flat vector itself, or to the workspace of this call (it carries the kept fold), bump the tensor's
        version counter: such a write between two steps invalidates the kept fold.  (Writes through re-pointed nn.Parameters do not show
        here: models call fold_invalidate from load_state_dict.)"""
        pk = (params.data_ptr(), params._version)
        wk = ws.data_ptr()
        if (getattr(self, "_pk", None) not in (None, pk)) or getattr(self, "_wv", {}).get(wk, ws._version) != ws._version:
            self.fold_invalidate()
        self._pk = pk
        if not hasattr(self, "_wv"):
            self._wv = {}
        self._wv[wk] = ws._version

    def rng_seed(self, seed: int, first_trajectory: int = 0):
        """Key of the in-kernel noise generator (Philox-4x32-10); resets its call counter.  Data parallel: every rank passes the global
        index of its shard's first trajectory, so the draws do not depend on the sharding."""
        _check(self.lib, self.handle, self.lib.slode_rng_seed(self.handle, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_trajectory)))

    def rng_state(self):
        """(seed, first_trajectory, calls drawn so far)."""
        a, b, c = C.c_uint64(), C.c_int64(), C.c_uint64()
        _check(self.lib, self.handle, self.lib.slode_rng_get(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def rng_set_counter(self, n: int):
        _check(self.lib, self.handle, self.lib.slode_rng_set_counter(self.handle, int(n)))

    def rng_normal(self, n: int, B: int, raw: bool = False):
        """The noise drawing call `n` uses for B trajectories: eps [B, L] (and the raw Philox words [B, ceil(L/4), 4] as int64 if raw)."""
        Ld = self.spec.latent_dim
        eps = torch.empty(B, Ld, dtype=torch.float32, device=self.device)
        words = torch.empty(B, (Ld + 3) // 4, 4, dtype=torch.int32, device=self.device) if raw else None
        _check(self.lib, self.handle, self.lib.slode_rng_normal(self.handle, int(n), B, Ld, self._p(eps), self._p(words), self._stream()))
        return (eps, words.to(torch.int64) & 0xFFFFFFFF) if raw else eps

    def draw_normal(self, B: int):
        """eps [B, L] of the next drawing call of the engine's generator (the call counter moves on)."""
        _, _, n = self.rng_state()
        eps = self.rng_normal(n, B)
        self.rng_set_counter(n + 1)
        return eps

    def sample_normal(self, loc, scale):
        """torch.normal(loc, scale) on the engine's generator: z = loc + scale * eps, one HIP kernel, one drawing call."""
        z = torch.empty_like(self._f32(loc, "loc"))
        _check(self.lib, self.handle, self.lib.slode_sample_normal(self.handle, loc.shape[0], loc.shape[1], self._p(loc),
                                                                   self._p(self._f32(scale, "scale")), self._p(z), self._stream()))
        return z

    def adam_step(self, params, grads, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-8):
        _check(self.lib, self.handle, self.lib.slode_adam_step(
            self.handle, params.numel(), self._p(params), self._p(grads), self._p(exp_avg), self._p(exp_avg_sq),
            float(lr), float(betas[0]), float(betas[1]), float(eps), int(step), self._stream()))


    def adam_region(self, lo: int, hi: int, step_delta: int):
        """Flat-vector elements [lo, hi) use Adam step count `step + step_delta` (skipped while < 1): include/slode.h, slode_adam_region."""
        _check(self.lib, self.handle, self.lib.slode_adam_region(self.handle, int(lo), int(hi), int(step_delta)))

    def aux_only_region(self):
        """[lo, hi) of the label-head parameters when only the auxiliary loss uses them (cvs / challenge), else (0, 0)."""
        lay, sp = self.layout, self.spec
        if not sp.aux_heads or sp.labels_in_main:
            return 0, 0
        return int(lay.aux_w1[0]), int(lay.cstd)

    def profile_enable(self, on: bool):
        """Per-kernel device timestamps for the step entry points (include/slode.h, slode_profile_enable)."""
        _check(self.lib, self.handle, self.lib.slode_profile_enable(self.handle, 1 if on else 0))

    def profile_read(self) -> List[Tuple[str, float]]:
        """[(kernel name, microseconds)] of the last profiled step call on this engine, in launch order."""
        names = (C.c_char_p * PROFILE_MAX_KERNELS)()
        us = (C.c_float * PROFILE_MAX_KERNELS)()
        n = self.lib.slode_profile_read(self.handle, PROFILE_MAX_KERNELS, names, us)
        if n < 0:
            _check(self.lib, self.handle, n)
        return [(names[i].decode(), float(us[i])) for i in range(n)]


def cvs_spec(z_iext=5, z_rtpr=5, z_eps=5, gauss=False, solver="midpoint", quantile_diff=0.475) -> ModelSpec:
    """data/cvs/config_cvs.py:6-52; u = [iext, rtpr] columns (models/mechanistic_cvs.py:131-135)."""
    return ModelSpec("cvs", gauss, 3, z_iext + z_rtpr + z_eps, z_eps, 2,
                     [PriorGroup("p_z_iext_given_iext", 0, z_iext, 0, 1), PriorGroup("p_z_rtprs_given_rtprs", z_iext, z_rtpr, 1, 1)],
                     solver=solver, quantile_diff=quantile_diff,
                     aux_heads=[AuxHead("q_iext_given_z_iext", "sigmoid", 0, z_iext, 0, 1),
                                AuxHead("q_rtpr_given_z_rtpr", "sigmoid", z_iext, z_rtpr, 1, 1)])


def challenge_spec(z_shed=5, z_symp=5, z_eps=5, gauss=False, solver="midpoint", quantile_diff=0.475) -> ModelSpec:
    """data/challenge/config_challenge.py; u = cat(symptoms, shedding) (models/mechanistic_challenge.py:167)."""
    return ModelSpec("challenge", gauss, 4, z_shed + z_symp + z_eps, z_eps, 2, [PriorGroup("p_z_u_given_u", 0, z_shed + z_symp, 0, 2)],
                     solver=solver, quantile_diff=quantile_diff,
                     aux_heads=[AuxHead("q_shedding_given_z_shedding", "sigmoid", 0, z_shed, 1, 1),
                                AuxHead("q_symptom_given_z_symptom", "sigmoid", z_shed, z_symp, 0, 1)])


def proc_spec(z_g=10, z_eps=10, gauss=False, solver="midpoint", quantile_diff=0.475) -> ModelSpec:
    """data/proc/config_proc.py; u = cat(aR[3], aS[4], C12, C6) (models/mechanistic_proc.py:196-198)."""
    aux = [AuxHead("q_aR_given_z_aR", "softmax", 0, z_g, 0, 3), AuxHead("q_aS_given_z_aS", "softmax", z_g, z_g, 3, 4),
           AuxHead("q_C12_given_z_C12", "expexp", 2 * z_g, z_g, 7, 1, "constant_std_C_12"),
           AuxHead("q_C6_given_z_C6", "expexp", 3 * z_g, z_g, 8, 1, "constant_std_C_6")]
    return ModelSpec("proc", gauss, 4, 4 * z_g + z_eps, z_eps, 9, [PriorGroup("p_z_u_given_u", 0, 4 * z_g, 0, 9)],
                     ode_state_dim=8, solver=solver, quantile_diff=quantile_diff, aux_heads=aux, labels_in_main=True)
