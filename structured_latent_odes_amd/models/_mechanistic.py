"""Shared implementation of the reference's six ``MechanisticModel[Gauss]`` classes (models/mechanistic_{cvs,proc,challenge}
[_Gauss].py).  The per-dataset modules only declare their label schema and attribute names."""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Tuple

import torch
import torch.nn as nn

from ..engine import AuxHead, ModelSpec, PriorGroup
from ..utils.exp import Exp
from .decoders import Decoder, GaussianDecoder
from .encoder_conv import EncoderCONV
from .encoder_mlp import EncoderMLP


class MechanisticBase(nn.Module):
    """Subclasses set:
      FAMILY        'cvs' | 'challenge' | 'proc'
      GAUSS         bool
      LABELS        ordered label names as the prior nets see them (columns of u), with their dims from config
      PRIORS        [(attr, [label names], [z group names])]            conditional prior nets p(z_g | u_g)
      AUX           [(attr, z group name, label name, kind)]            auxiliary heads q(label | z_g); kind in sigmoid|softmax|expexp
      Z_GROUPS      ordered latent group names (config attr = 'z_<name>_dim'); the last one is 'epsilon'
    """
    FAMILY, GAUSS = "", False
    LABELS: Tuple[str, ...] = ()
    PRIORS: List = []
    AUX: List = []
    Z_GROUPS: Tuple[str, ...] = ()
    LABELS_IN_MAIN = False   # proc: the main model also scores the labels on the replayed z (mechanistic_proc.py:145-146)

    def __init__(self, config, device, times):
        super().__init__()
        self.config, self.times, self.device = config, times, device
        self.obs_dim = config.obs_dim
        self.n_time = len(times)
        self.aux_loss_multiplier = float(config.aux_loss_multiplier)
        self.u_hidden_dim = config.u_hidden_dim
        self.use_cuda = True            # SURVEY note A: always truthy in the reference => hidden layers carry '.module.'
        self.allow_broadcast = False
        self.z_dims = {g: int(getattr(config, "z_%s_dim" % g)) for g in self.Z_GROUPS}
        self.z_off, off = {}, 0
        for g in self.Z_GROUPS:
            self.z_off[g] = off
            off += self.z_dims[g]
        self.latent_dim = off
        self.z_epsilon_dim = self.z_dims["epsilon"]
        self.label_dims = {l: int(getattr(config, "%s_dim" % l)) for l in self.LABELS}
        self.u_off, off = {}, 0
        for l in self.LABELS:
            self.u_off[l] = off
            off += self.label_dims[l]
        self.n_u = off
        self.setup_networks()
        self.l1_func = nn.L1Loss()
        self._binding = None
        self.to(device)

    # ---- construction -------------------------------------------------------------------------------------
    def setup_networks(self):
        cfg = self.config
        for attr, group, label, kind in self.AUX:
            zd, ld = self.z_dims[group], self.label_dims[label]
            if kind == "sigmoid":
                net = EncoderMLP([zd, self.u_hidden_dim, ld], activation=nn.Softplus, output_activation=nn.Sigmoid,
                                 allow_broadcast=False, use_cuda=self.use_cuda)
            elif kind == "softmax":
                net = EncoderMLP([zd, self.u_hidden_dim, ld], activation=nn.Softplus, output_activation=nn.Softmax,
                                 allow_broadcast=False, use_cuda=self.use_cuda)
            else:
                net = EncoderMLP([zd, self.u_hidden_dim, [ld, ld]], activation=nn.Softplus, output_activation=[Exp, Exp],
                                 allow_broadcast=False, use_cuda=self.use_cuda)
            setattr(self, attr, net)
        self.encoder = EncoderCONV(n_channels=self.obs_dim, n_time=self.n_time, n_filters=cfg.n_filters,
                                   filter_size=cfg.filter_size, pool_size=cfg.pool_size, latent_dim=self.latent_dim,
                                   hidden_dim=cfg.cnn_hidden_dim)
        for attr, labels, groups in self.PRIORS:
            n_in = sum(self.label_dims[l] for l in labels)
            n_out = sum(self.z_dims[g] for g in groups)
            setattr(self, attr, EncoderMLP([n_in, [n_out, n_out]], activation=nn.Softplus, output_activation=[None, Exp],
                                           allow_broadcast=False, use_cuda=self.use_cuda))
        dec = GaussianDecoder if self.GAUSS else Decoder
        self.decoder = dec(config=cfg, times=self.times, latent_dim=self.latent_dim, device=self.device)
        if self.FAMILY == "proc":
            self.constant_std_C_12 = nn.Parameter(torch.ones(1) * cfg.constant_std, requires_grad=True)
            self.constant_std_C_6 = nn.Parameter(torch.ones(1) * cfg.constant_std, requires_grad=True)
            self.softplus = nn.Softplus()

    def model_spec(self) -> ModelSpec:
        cfg = self.config
        groups = []
        for attr, labels, zgroups in self.PRIORS:
            groups.append(PriorGroup(attr, self.z_off[zgroups[0]], sum(self.z_dims[g] for g in zgroups),
                                     self.u_off[labels[0]], sum(self.label_dims[l] for l in labels)))
        aux = []
        for attr, group, label, kind in self.AUX:
            aux.append(AuxHead(attr, kind, self.z_off[group], self.z_dims[group], self.u_off[label], self.label_dims[label],
                               "constant_std_C_12" if label == "C12" else ("constant_std_C_6" if label == "C6" else "")))
        return ModelSpec(self.FAMILY, self.GAUSS, self.obs_dim, self.latent_dim, self.z_epsilon_dim, self.n_u, groups,
                         aux_heads=aux, labels_in_main=self.LABELS_IN_MAIN, u_hidden_dim=self.u_hidden_dim, aux_mult=self.aux_loss_multiplier,
                         ode_state_dim=cfg.ode_state_dim, ode_hidden_dim=cfg.ode_hidden_dim, n_filters=cfg.n_filters,
                         filter_size=cfg.filter_size, pool_size=cfg.pool_size, cnn_hidden_dim=cfg.cnn_hidden_dim,
                         solver=cfg.solver, quantile_diff=cfg.quantile_diff,
                         # config.adjoint_solver (True in all three reference configs) selects torchdiffeq.odeint_adjoint
                         # (models/blackbox_ode.py:40-42): its gradients are reproduced by grad_mode "reference_adjoint"
                         grad_mode="reference_adjoint" if getattr(cfg, "adjoint_solver", False) else "exact")

    def _bind(self):
        """Create the engine and move every parameter into the flat vector (first hot-path use; needs a HIP device)."""
        if self._binding is None:
            from ._binding import Binding
            named = self.encoder._named_for_binding()
            named.update(self.decoder._named_for_binding())
            for attr, _, _ in self.PRIORS:
                net = getattr(self, attr)
                for k, p in net.named_parameters():
                    named["%s.%s" % (attr, k)] = p
            for attr, _, _, _ in self.AUX:   # label heads: auxiliary-loss kernel (and the main loss for proc) => in the layout
                for k, p in getattr(self, attr).named_parameters():
                    named["%s.%s" % (attr, k)] = p
            if self.FAMILY == "proc":
                named["constant_std_C_12"], named["constant_std_C_6"] = self.constant_std_C_12, self.constant_std_C_6
            hot = set(id(p) for p in named.values())
            extra = [p for p in self.parameters() if id(p) not in hot]
            dev = next(self.parameters()).device
            self._binding = Binding(self.model_spec(), self.times.to(torch.float32), dev, named, extra)
            self.encoder._binding = self._binding
            self.decoder.ode_model._binding = self._binding
        return self._binding

    def load_state_dict(self, *args, **kwargs):
        """nn.Module.load_state_dict + a note to the engine: the weights were written behind its back, so the next step must fold the
        encoder again (the kept fold belongs to the old weights; include/slode.h, slode_fold_invalidate)."""
        res = super().load_state_dict(*args, **kwargs)
        if self._binding is not None:
            self._binding.engine.fold_invalidate()
        return res

    def parameters_changed(self):
        """Call after writing parameters by any other route (own optimizer, manual edits) between two SVI steps."""
        if self._binding is not None:
            self._binding.engine.fold_invalidate()

    # ---- helpers ------------------------------------------------------------------------------------------
    def labels_to_u(self, **labels) -> torch.Tensor:
        return torch.cat([labels[l].reshape(labels[l].shape[0], -1).to(torch.float32) for l in self.LABELS], dim=1).contiguous()

    def draw_eps(self, batch_size: int, device) -> torch.Tensor:
        """Reparameterisation noise in the guide's site order (one ``randn`` per ``pyro.sample`` site)."""
        parts = [torch.randn(batch_size, n, device=device) for n in self._site_dims()]
        return torch.cat(parts, dim=1)

    def _site_dims(self) -> List[int]:
        if self.FAMILY == "cvs":
            return [self.z_dims[g] for g in self.Z_GROUPS]                       # z_iext, z_rtpr, z_epsilon
        return [self.latent_dim - self.z_epsilon_dim, self.z_epsilon_dim]        # z_u, z_epsilon

    def _prior_loc_scale(self, labels: Dict[str, torch.Tensor]):
        """(loc, scale) [B, L] of p(z | labels): the conditional prior nets on the label columns, N(0, 1) for the z_epsilon dims -- one
        HIP kernel (``slode_prior_nets``), the same nets the fused ELBO kernel evaluates in its P0 phase."""
        b = self._bind()
        return b.engine.prior_nets(b.flat, self.labels_to_u(**labels))

    def _z_group(self, t: torch.Tensor, g: str) -> torch.Tensor:
        return t[:, self.z_off[g]:self.z_off[g] + self.z_dims[g]]

    # ---- the four callables the training scripts hand to SVI (training_cvs.py:236-249) -----------------------
    def model(self, observations, **labels):
        """Stands for the Pyro model (mechanistic_cvs.py:105-178); together with ``guide`` it defines the main loss, whose
        arithmetic is ``slode_elbo_step``.  Called directly it returns -ELBO (summed over the batch) for fresh noise."""
        from ..svi import SVI
        return SVI(self.model, self.guide, None).evaluate_loss(observations=observations, **labels)

    def guide(self, observations, **labels):
        """q(z | x): encoder + one reparameterised Normal per latent group (mechanistic_cvs.py:213-238).  The sites are reparameterised,
        so z carries the encoder's graph: the noise is one drawing call of the engine's generator (the call ``sample_normal`` would
        make: same draw, the counter moves by one) and z = loc + scale * eps is formed in torch.  Without gradients the one-kernel
        ``sample_normal`` is used (the same draw; the multiply-add may be fused, so z can differ in the last bit)."""
        b = self._bind()
        loc, scale = self.encoder.forward(observations)
        if torch.is_grad_enabled() and (loc.requires_grad or scale.requires_grad):
            z = loc + scale * b.engine.draw_normal(loc.shape[0])
        else:
            z = b.engine.sample_normal(loc.contiguous(), scale.contiguous())
        return tuple(self._z_group(z, g) for g in self.Z_GROUPS)

    def model_meta(self, observations, **labels):
        """Auxiliary supervised loss (mechanistic_cvs.py:240-270); arithmetic in :class:`svi.AuxStep`."""
        from ..svi import SVI
        return SVI(self.model_meta, self.guide_meta, None).evaluate_loss(observations=observations, **labels)

    def guide_meta(self, observations, **labels):
        """Empty guide accompanying ``model_meta`` (mechanistic_cvs.py:272-276)."""
        return None

    # ---- eval-side API -------------------------------------------------------------------
    def _predict_labels(self, observations):
        """classifier / pred_inputs of the reference (mechanistic_cvs.py:278-296): encoder -> one posterior draw -> label heads
        (``slode_label_heads``: every head writes the label columns it scores) -> hard decisions."""
        b = self._bind()
        with torch.no_grad():
            loc, scale = self.encoder.forward(observations)
            z = b.engine.sample_normal(loc.contiguous(), scale.contiguous())
            probs = b.engine.label_heads(b.flat, z)
            res = {}
            heads = {h.prefix: h for h in b.engine.spec.aux_heads}
            for attr, group, label, kind in self.AUX:
                head = heads[attr]
                val = probs[:, head.u_off:head.u_off + head.u_dim]
                if kind == "sigmoid":
                    res[label] = (val > 0.5).float()
                elif kind == "softmax":
                    res[label] = torch.zeros_like(val).scatter_(1, val.argmax(1, keepdim=True), 1.0)
                else:
                    res[label] = val.clone()
            return res

    def recon(self, observations, is_post, **labels):
        """Posterior (is_post) or prior reconstruction (mechanistic_cvs.py:298-323): returns the reference's dict."""
        b = self._bind()
        with torch.no_grad():
            loc, scale = self._loc_scale(observations, is_post, labels)
            z = b.engine.sample_normal(loc.contiguous(), scale.contiguous())
            if self.GAUSS:
                solution_xt, mean, std = self.decoder.forward(z=z)
                return {"l1": self.l1_func(mean, observations), "solution_xt": solution_xt, "mean": mean, "std": std, "z": z}
            solution_xt, mu_75, mu_50, mu_25, std = self.decoder.forward(z=z)
            return {"l1": self.l1_func(mu_50, observations), "solution_xt": solution_xt, "mu_75": mu_75, "mu_50": mu_50,
                    "mu_25": mu_25, "std": std, "z": z}

    # ---- what the fused eval-side calls below share ----------------------------------------------------------------------------
    def _label_tensors(self, labels, B):
        """The label tensors in ``LABELS`` order as ``make_batch`` takes them: ``[B, width]``, float32, contiguous."""
        return [labels[l].reshape(B, -1).to(torch.float32).contiguous() for l in self.LABELS]

    def _draws_batch(self, observations, labels, eps, draws):
        """The engine batch of a call with ``draws`` draws per trajectory: ``eps`` ``[draws, B, L]`` (``[B, L]`` for one draw) or None."""
        B = observations.shape[0]
        e = eps if eps is None or draws > 1 else eps.reshape(B, -1)
        return self._bind().engine.make_batch(observations, self._label_tensors(labels, B),
                                              None if e is None else e.to(torch.float32).contiguous(), particles=draws)

    @staticmethod
    def _count(n, name="num_samples") -> int:
        """The draw count of a call as an int; ValueError below 1."""
        if int(n) < 1:
            raise ValueError("%s must be >= 1, got %d" % (name, int(n)))
        return int(n)

    def _loc_scale(self, observations, is_post, labels):
        """(loc, scale) [B, L] of the posterior q(z | x) (``is_post``: the encoder) or of the conditional prior p(z | labels)."""
        return self.encoder.forward(observations) if is_post else self._prior_loc_scale(labels)

    def _noise(self, ns, B, eps, device=None):
        """``eps`` as ``[ns, B, L]``; None: ONE drawing call of the engine's generator (counter n -> n + 1, row k * B + b = draw k of
        trajectory b, as the fused engine calls make it).  The one place of the eval-side API that draws ``ns`` rows per trajectory."""
        if eps is None:
            eps = self._bind().engine.draw_normal(ns * B)
        return (eps if device is None else eps.to(device)).reshape(ns, B, -1)

    def _draws(self, loc, scale, ns, eps):
        """``(eps, z)``, ``[ns, B, L]`` each: z = loc + scale * eps, with ``eps`` as ``_noise`` yields it."""
        eps = self._noise(ns, loc.shape[0], eps, loc.device)
        return eps, loc.unsqueeze(0) + scale.unsqueeze(0) * eps

    def _decoded_draws(self, z):
        """``decoder.forward`` on the draws ``z`` ``[ns, B, L]`` in one pass: ``{curve: [B, C, T, ns]}`` of every head curve."""
        ns, B = z.shape[:2]
        names = ("solution_xt", "mean", "std") if self.GAUSS else ("solution_xt", "mu_75", "mu_50", "mu_25", "std")
        return {n: v.reshape(ns, B, v.shape[1], v.shape[2]).permute(1, 2, 3, 0).contiguous()
                for n, v in zip(names, self.decoder.forward(z=z.reshape(ns * B, -1).contiguous())) if n not in ("solution_xt", "std")}

    @staticmethod
    def _fused_or_composed(fused, composed):
        """``fused()``; where the engine refuses it (SlodeError with SLODE_EINVAL, status -1: nothing launched, nothing drawn), ``composed()``.
        Any other engine error is raised."""
        from .. import _lib as L
        try:
            return fused()
        except L.SlodeError as err:
            if getattr(err, "status", None) != -1:
                raise
        return composed()

    def _chunks(self, observations, labels, ns, eps):
        """The chunk walk of a composed route: ``(lo, hi, eps[:, lo:hi], rows [lo, hi) of the batch as keyword arguments)`` for
        ``MOMENTS_CHUNK_ROWS // ns`` rows at a time.  The noise is drawn once for the whole batch, before chunking, and sliced per chunk,
        so the result does not depend on the chunking."""
        B = observations.shape[0]
        eps = self._noise(ns, B, eps)
        rows = max(1, self.MOMENTS_CHUNK_ROWS // ns)
        for lo in range(0, B, rows):
            hi = min(B, lo + rows)
            yield lo, hi, eps[:, lo:hi], dict({k: v[lo:hi] for k, v in labels.items()}, observations=observations[lo:hi])

    def _composed_moments(self, observations, labels, ns, eps, materialise, reduce, names=None):
        """A composed fallback over ``_chunks``: ``materialise(lo, hi, eps chunk, batch chunk)`` yields the per-draw curves of rows [lo, hi)
        (``{curve: ...}``) and ``reduce`` turns one curve's into a tuple of ``[rows, C, T]`` tensors; returns ``{curve: tuple of [B, C, T]}``."""
        names = names or self.MOMENT_HEADS[bool(self.GAUSS)]      # (names: the curves to reduce, where they are not the head curves alone)
        parts = {n: [] for n in names}
        for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
            res = materialise(lo, hi, e, d)
            for n in names:
                parts[n].append(reduce(res[n]))
            del res
        return {n: tuple(torch.cat(col, 0) for col in zip(*chunks)) for n, chunks in parts.items()}

    @staticmethod
    def _mean_sd(v):
        """fp32 ``mean`` / ``std(unbiased=False)`` over the sample axis of ``[rows, C, T, ns]``."""
        v = v.to(torch.float32)
        return v.mean(dim=-1), v.std(dim=-1, unbiased=False)

    @staticmethod
    def _save_arrays(results_dir, named):
        """``np.save`` of every ``(file name, tensor)`` of ``named`` under ``results_dir`` (created if missing): the paths written, in order."""
        import os
        import numpy as np
        os.makedirs(results_dir, exist_ok=True)
        written = []
        for fname, val in named:
            path = os.path.join(results_dir, fname)
            np.save(path, val.cpu().numpy())
            written.append(path)
        return written

    # ---- what the whole-curve calls share (latent_attribution, curve_summary, recon_quantiles, mechanism_moments, simultaneous_band) ----
    @staticmethod
    def _levels_list(levels, most: int, open_at_zero: bool):
        """``levels`` (a sequence, or a tensor read on the host once) as a list of floats: 1 to ``most`` values in [0, 1] -- in (0, 1] with
        ``open_at_zero`` -- or ValueError."""
        lv = [float(x) for x in (levels.detach().cpu().reshape(-1).tolist() if isinstance(levels, torch.Tensor) else levels)]
        if not 1 <= len(lv) <= most:
            raise ValueError("levels must hold 1 to %d values, got %d" % (most, len(lv)))
        if any(not ((0.0 < x if open_at_zero else 0.0 <= x) and x <= 1.0) for x in lv):
            raise ValueError("levels must lie in %s, got %r" % ("(0, 1]" if open_at_zero else "[0, 1]", lv))
        return lv

    @staticmethod
    def _fewest_calls(n_items: int, cap: int, plan):
        """``n_items`` items (arms, slots) in the fewest engine calls that fit the LDS, as even as that number allows: ``[(lo, hi)]``.
        ``plan(n)`` raises SlodeError where a call of n items does not fit (one item is not asked: the call itself refuses it); ``cap``:
        the most items of one call."""
        from .. import _lib as L
        fit = min(n_items, cap)
        while fit > 1:
            try:
                plan(fit)
                break
            except L.SlodeError:
                fit -= 1
        n_calls = -(-n_items // fit)
        per = -(-n_items // n_calls)
        return [(lo, min(lo + per, n_items)) for lo in range(0, n_items, per)]

    @staticmethod
    def _on_the_same_noise(eng, eps, slices, call):
        """``[call(lo, hi)]`` over ``slices``, every call rewound to the drawing call the first begins at (``eps`` given: nothing to rewind),
        so the counter ends where ONE call leaves it and the split changes no bit."""
        n0 = None if eps is not None else eng.rng_state()[2]
        out = []
        for lo, hi in slices:
            if n0 is not None:
                eng.rng_set_counter(n0)
            out.append(call(lo, hi))
        return out

    @contextlib.contextmanager
    def _counter_moves_by(self, moved: int, eps):
        """Around a composed route that stands in for an engine call which moves the generator's counter by ``moved``: whatever the route
        draws, the counter ends at n + ``moved`` (``eps`` given: the generator is not used)."""
        eng = self._bind().engine
        n0 = eng.rng_state()[2] if eps is None else None
        yield
        if n0 is not None:
            eng.rng_set_counter(n0 + moved)

    def _save_over_batches(self, results_dir, batches, call, rows, dim: int = 0, side=None):
        """``call(**batch)`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors); ``rows(result)``
        yields the batch's ``(file name, tensor)`` pairs, which are concatenated along ``dim`` (the trajectories, in loader order) and
        written with ONE read-back, at the end; then the side file ``side`` = ``(file name, write(path, last result or None))``.  Returns
        the paths."""
        import os
        parts, r = {}, None
        for d in batches:
            r = call(**d)
            for fname, t in rows(r):
                parts.setdefault(fname, []).append(t)
        written = self._save_arrays(results_dir, ((fname, torch.cat(v, dim)) for fname, v in parts.items()))
        if side is not None:
            os.makedirs(results_dir, exist_ok=True)
            path = os.path.join(results_dir, side[0])
            side[1](path, r)
            written.append(path)
        return written

    @staticmethod
    def _save_levels(path, r):
        """The side file of a call with levels: the float64 ``"levels"`` of its last result (no batch: an empty array)."""
        import numpy as np
        np.save(path, np.asarray([] if r is None else r["levels"].tolist(), dtype=np.float64))

    # ---- the statistics row of one batch (training.input_pred_stats_fused) -------------------------------------------------
    def eval_stat_slots(self) -> Dict[str, int]:
        """{label name: its hit-count slot in the eval_stats row}: 3 + index of the label's head in ``AUX`` (include/slode.h)."""
        return {label: 3 + a for a, (_, _, label, _) in enumerate(self.AUX)}

    def eval_stats(self, observations, is_post, out=None, eps=None, num_particles: int = 1, **labels):
        """What one batch of ``input_pred_stats`` (training_cvs.py:43-144) needs, as one device row of ``EVAL_SLOTS`` floats --
        [-ELBO of the main loss, auxiliary loss, sum over [B, C, T] of |mu_50 or mean - observations| of one reconstruction (posterior if
        ``is_post`` else prior), hits per label head (``eval_stat_slots``), B] -- from ONE engine call (``slode_eval_stats``): nothing is
        read back and the stream is not synchronised.  ``out``: a float32 [EVAL_SLOTS] device tensor (a row of the caller's table).
        ``eps`` [4, B, L] (main, auxiliary, recon, labels) makes it reproducible; None draws four calls of the engine's generator, the
        ones the unfused sequence evaluate_loss, evaluate_loss, recon, classifier would draw.  Where the engine refuses (adaptive solver,
        ``num_particles`` > 1, strided observations, measured arms) the row is composed from those unfused calls instead."""
        from .. import _lib as L
        b = self._bind()
        B = observations.shape[0]
        if out is None:
            out = torch.empty(L.EVAL_SLOTS, dtype=torch.float32, device=b.flat.device)
        if int(num_particles) == 1:
            bt = b.engine.make_batch(observations, self._label_tensors(labels, B), eps, particles=4 if eps is not None else 1)
            try:
                return b.engine.eval_stats(b.flat, bt, B, is_post, out)
            except L.SlodeError:      # ANY engine error leads to the unfused calls here, not a refusal (_fused_or_composed) alone:
                pass                  # they name the same fault themselves, and the row is wanted wherever they can make it
        if eps is not None:
            raise ValueError("explicit eps is taken by the fused statistics call only; this configuration runs the unfused calls")
        return self._eval_stats_composed(observations, is_post, out, int(num_particles), labels)

    def _eval_stats_composed(self, observations, is_post, out, num_particles, labels):
        """The same row from the existing calls, in their order (each draws its own noise and reads its own result back)."""
        from ..svi import SVI, Trace_ELBO
        cache = self.__dict__.setdefault("_stat_svi", {})
        if num_particles not in cache:
            elbo = Trace_ELBO(num_particles=num_particles)
            cache[num_particles] = (SVI(self.model, self.guide, None, loss=elbo), SVI(self.model_meta, self.guide_meta, None, loss=elbo))
        main, aux = cache[num_particles]
        row = [0.0] * out.numel()
        row[0] = main.evaluate_loss(observations=observations, **labels)
        row[1] = aux.evaluate_loss(observations=observations, **labels) if self.AUX else 0.0
        row[2] = float(self.recon(observations=observations, is_post=is_post, **labels)["l1"]) * observations.numel()
        pred = self._predict_labels(observations)
        for label, slot in self.eval_stat_slots().items():
            want = labels[label].reshape(observations.shape[0], -1)
            row[slot] = float((pred[label] - want).abs().lt(0.5).all(dim=1).float().sum())
        row[-1] = float(observations.shape[0])
        out.copy_(torch.tensor(row, dtype=torch.float32))
        return out

    def recon_samples(self, observations, is_post, num_samples: int, eps=None, posterior=None, **labels):
        """``multiple_samples`` of the reference (training_proc.py:205-223, training_cvs.py / training_challenge.py alike): it calls
        ``recon`` ``num_samples`` times (config.num_samples = 200) and concatenates the quantile curves along a new last axis.
        Here the ``num_samples`` latent draws of the whole batch go through ONE ODE solve + ONE head launch
        (``num_samples * B`` trajectories).  Returns a dict of tensors shaped ``[B, C, T, num_samples]`` (``mu_25/mu_50/mu_75``, or
        ``mean`` for the Gaussian family) plus ``z`` ``[num_samples, B, L]``.  ``eps`` (``[num_samples, B, L]`` standard normal
        draws, optional) makes the result reproducible.  ``posterior`` = ``(loc, scale)`` ``[B, L]`` replaces the encoder's / the prior
        nets' distribution (a refined posterior of ``refine_posterior``: its curves decoded); None (the default): unchanged."""
        self._bind()
        with torch.no_grad():
            loc, scale = self._loc_scale(observations, is_post, labels) if posterior is None else self._given_posterior(observations, posterior)
            _, z = self._draws(loc, scale, int(num_samples), eps)      # [ns, B, L]
            return {"z": z, **self._decoded_draws(z)}

    def save_recon_samples(self, results_dir: str, observations, is_post, num_samples: int, **labels):
        """Writes the arrays ``multiple_samples`` saves, under the reference's file names (``mu_50_post_sample.npy`` ...)."""
        res = self.recon_samples(observations, is_post, num_samples, **labels)
        tag = "post_sample" if is_post else "prior_sample"
        return self._save_arrays(results_dir, (("%s_%s.npy" % (name, tag), res[name]) for name in ("mu_50", "mu_75", "mu_25", "mean") if name in res))

    # ---- the Monte-Carlo summary of multiple_samples: mean and sd over the draws, nothing per draw kept -------------------------------
    MOMENT_HEADS = {False: ("mu_50", "mu_75", "mu_25"), True: ("mean",)}   # GAUSS -> curve names in the engine's head order q = 0, 1, 2
    MOMENTS_CHUNK_ROWS = 65536                                             # composed route: trajectories (num_samples x rows) per chunk

    def recon_moments(self, observations, is_post, num_samples: int, eps=None, **labels):
        """What the reference's evaluation takes from ``multiple_samples``: per trajectory, the mean and the population standard
        deviation (``np.mean(..., -1)`` / ``np.std(..., -1)``) over ``num_samples`` latent draws of every decoder head curve, as
        ``{"mu_50": (mean, sd), "mu_75": ..., "mu_25": ...}`` (``{"mean": (mean, sd)}`` for the Gaussian family), each tensor
        ``[B, C, T]`` -- from ONE engine call (``slode_recon_moments``) that keeps the running moments on chip: no
        ``[B, C, T, num_samples]`` tensor exists.  ``eps`` ``[num_samples, B, L]`` makes it reproducible; None draws one call of the
        engine's generator, the draw ``recon_samples`` makes.  Where the engine refuses (adaptive solver, strided observations,
        measured arms, LDS budget) the same dict is composed from ``recon_samples`` in chunks over B."""
        b = self._bind()
        B, ns = observations.shape[0], self._count(num_samples)

        def fused():
            mean, sd = b.engine.recon_moments(b.flat, self._draws_batch(observations, labels, eps, ns), B, is_post, ns)
            return {n: (mean[q], sd[q]) for q, n in enumerate(self.MOMENT_HEADS[bool(self.GAUSS)])}
        return self._fused_or_composed(fused, lambda: self._composed_moments(
            observations, labels, ns, eps, lambda lo, hi, e, d: self.recon_samples(is_post=is_post, num_samples=ns, eps=e, **d), self._mean_sd))

    def save_recon_moments(self, results_dir: str, observations, is_post, num_samples: int, **labels):
        """Writes ``<curve>_<post|prior>_sample_mean.npy`` and ``..._sample_sd.npy`` (``[B, C, T]`` each) for every head curve: new names
        beside the reference's ``mu_50_post_sample.npy`` & co., which ``save_recon_samples`` keeps writing."""
        res = self.recon_moments(observations, is_post, num_samples, **labels)
        tag = "post_sample" if is_post else "prior_sample"
        return self._save_arrays(results_dir, (("%s_%s_%s.npy" % (name, tag, kind), val)
                                               for name, moments in res.items() for kind, val in zip(("mean", "sd"), moments)))

    # ---- cohort curves: the draws of recon_moments reduced by condition, as the reference's evaluation notebooks report them ----------
    def cohort_index(self, by=None, **labels):
        """``(ids [B] int64, keys [G, width])``: the cohort of every trajectory under the label columns named in ``by`` (default: all of
        the family's labels, ``LABELS`` order) -- ``torch.unique(dim=0, return_inverse=True)`` over the concatenated columns, so cohort g
        is the set of trajectories whose labels equal ``keys[g]``, keys in sorted order.  This step synchronises with the device (the
        number of distinct rows decides a shape)."""
        names = tuple(by) if by else tuple(self.LABELS)
        missing = [n for n in names if n not in labels]
        if missing or not names:
            raise ValueError("cohort_index needs the label tensors %s (missing: %s)" % (list(names), missing))
        B = labels[names[0]].shape[0]
        cols = torch.cat([labels[n].reshape(B, -1).to(torch.float32) for n in names], dim=1)
        keys, ids = torch.unique(cols, dim=0, return_inverse=True)
        return ids.reshape(B).to(torch.int64), keys

    def _cohort_lists(self, observations, cohorts, num_cohorts, labels):
        """``(ids, keys, G, members int32 [M], offsets int32 [G + 1], count int64 [G])`` of ``cohorts``: a ``[B]`` integer tensor (negative: no
        cohort) or a tuple of label names for ``cohort_index``; members sorted by cohort with a stable sort (batch order inside a cohort)."""
        B, dev = observations.shape[0], observations.device
        if torch.is_tensor(cohorts):
            ids = cohorts.reshape(-1).to(dev, torch.int64)
            if ids.numel() != B:
                raise ValueError("cohorts must have B = %d entries, got %d" % (B, ids.numel()))
            G = int(num_cohorts) if num_cohorts is not None else (int(ids.max()) + 1 if B else 0)
            if G < 1:
                raise ValueError("no cohort: every id is negative (pass num_cohorts to keep empty cohorts)")
            if B and int(ids.max()) >= G:
                raise ValueError("cohort id %d beyond num_cohorts = %d" % (int(ids.max()), G))
            keys = torch.arange(G, device=dev).reshape(G, 1)
        else:
            ids, keys = self.cohort_index(by=cohorts, **labels)
            G = keys.shape[0]
        key = torch.where(ids < 0, torch.full_like(ids, G), ids)
        order = torch.sort(key, stable=True).indices
        count = torch.bincount(key, minlength=G + 1)[:G]
        offsets = torch.cat([count.new_zeros(1), count.cumsum(0)]).to(torch.int32)
        members = order[:int(count.sum())].to(torch.int32).contiguous()
        return ids, keys, G, members, offsets, count

    def cohort_moments(self, observations, is_post, num_samples: int, cohorts, eps=None, chunk: int = 0, clip_min=None, num_cohorts=None,
                       **labels):
        """Per-condition curves, as the reference's evaluation notebooks report them: for every cohort g (a set of trajectories of this
        batch) and head curve, ``(mean, sd, sd_subjects)``, ``[G, C, T]`` each -- the mean over members x draws, the population sd over
        members x draws, and the population sd over the members of their draw means (at ``num_samples`` = 1 the notebooks'
        ``np.std(data[loc], 0)``) -- with ``"observations"`` ``[G, C, T]`` (the members' mean observation), ``"l1"`` ``[G, C]`` (``sum_t
        |mean observation - mean mu_50|``, the notebooks' ``l1_error`` summand), ``"count"`` ``[G]`` and ``"keys"``.  ``cohorts``: a
        ``[B]`` integer tensor, negative = no cohort (``num_cohorts`` keeps trailing empty cohorts), or a tuple of label names for
        ``cohort_index`` (which synchronises).  An empty cohort is NaN throughout.  The draws are those of ``recon_moments`` (``eps``
        ``[num_samples, B, L]`` or one drawing call); ``clip_min`` replaces head values below it (the sbio notebooks' ``mu_50[mu_50 < 0] =
        0``).  ONE engine call (``slode_cohort_moments``); ``chunk``: members folded per partial, 0 = the library's choice.  Where the engine
        refuses (adaptive solver, strided observations, measured arms, LDS budget, more than 1024 cohorts) the same dict is reduced from
        ``recon_samples`` in chunks of rows in fp64."""
        b = self._bind()
        B, ns = observations.shape[0], self._count(num_samples)
        ids, keys, G, members, offsets, count = self._cohort_lists(observations, cohorts, num_cohorts, labels)

        def fused():
            mean, sd, sdb, om, l1 = b.engine.cohort_moments(b.flat, self._draws_batch(observations, labels, eps, ns), B, is_post, ns, members,
                                                            offsets, G, chunk=chunk, clip_min=clip_min)
            return dict({n: (mean[q], sd[q], sdb[q]) for q, n in enumerate(self.MOMENT_HEADS[bool(self.GAUSS)])}, observations=om, l1=l1)
        return dict({"count": count, "keys": keys}, **self._fused_or_composed(
            fused, lambda: self._cohort_composed(observations, is_post, ns, ids, G, count, eps, clip_min, labels)))

    def _cohort_composed(self, observations, is_post, ns, ids, G, count, eps, clip_min, labels):
        """The composed route: ``recon_samples`` of ``MOMENTS_CHUNK_ROWS // ns`` rows at a time (ONE drawing call for the whole batch, sliced
        per chunk), every row's draw mean and sum of squares added to its cohort's fp64 sums."""
        B, dev = observations.shape[0], observations.device
        names = self.MOMENT_HEADS[bool(self.GAUSS)]
        Cn, T = observations.shape[1], observations.shape[2]
        slot = torch.where(ids < 0, torch.full_like(ids, G), ids)           # (bucket G: the trajectories of no cohort)
        s1 = {n: torch.zeros(G + 1, Cn, T, dtype=torch.float64, device=dev) for n in names}
        sb2 = {n: torch.zeros_like(s1[n]) for n in names}
        sv2 = {n: torch.zeros_like(s1[n]) for n in names}
        so = torch.zeros(G + 1, Cn, T, dtype=torch.float64, device=dev).index_add_(0, slot, observations.to(torch.float64))
        for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
            got = self.recon_samples(is_post=is_post, num_samples=ns, eps=e, **d)
            for n in names:
                v = got[n].to(torch.float64)                                # [rows, C, T, ns]
                if clip_min is not None:
                    v = torch.where(v < clip_min, torch.full_like(v, float(clip_min)), v)
                mb = v.mean(dim=-1)
                s1[n].index_add_(0, slot[lo:hi], mb)
                sb2[n].index_add_(0, slot[lo:hi], mb * mb)
                sv2[n].index_add_(0, slot[lo:hi], (v * v).sum(dim=-1))
            del got
        cnt = count.to(torch.float64).reshape(G, 1, 1)
        nan = torch.full((G, Cn, T), float("nan"), dtype=torch.float64, device=dev)
        live = (cnt > 0).expand(G, Cn, T)
        res = {}
        for n in names:
            mean = s1[n][:G] / cnt
            sd = (sv2[n][:G] / (cnt * ns) - mean * mean).clamp_min(0).sqrt()
            sdb = (sb2[n][:G] / cnt - mean * mean).clamp_min(0).sqrt()
            res[n] = tuple(torch.where(live, x, nan).to(torch.float32) for x in (mean, sd, sdb))
        res["observations"] = torch.where(live, so[:G] / cnt, nan).to(torch.float32)
        res["l1"] = (res["observations"].to(torch.float64) - res[names[0]][0].to(torch.float64)).abs().sum(dim=-1).to(torch.float32)
        return res

    def save_cohort_moments(self, results_dir: str, observations, is_post, num_samples: int, cohorts, **labels):
        """Writes ``<curve>_<post|prior>_cohort_{mean,sd,sd_subjects}.npy`` (``[G, C, T]`` each) for every head curve,
        ``observations_cohort_mean.npy``, ``cohort_keys.npy``, ``cohort_count.npy`` and ``l1_<post|prior>_cohort.npy``; returns the paths."""
        return self._save_arrays(results_dir, self._cohort_named(self.cohort_moments(observations, is_post, num_samples, cohorts, **labels), is_post))

    def _cohort_named(self, res, is_post):
        """``(file name, tensor)`` of every array of a ``cohort_moments`` result, under ``save_cohort_moments``' names."""
        tag = "post" if is_post else "prior"
        named = [("%s_%s_cohort_%s.npy" % (name, tag, kind), val) for name in self.MOMENT_HEADS[bool(self.GAUSS)]
                 for kind, val in zip(("mean", "sd", "sd_subjects"), res[name])]
        return named + [("observations_cohort_mean.npy", res["observations"]), ("cohort_keys.npy", res["keys"]),
                        ("cohort_count.npy", res["count"]), ("l1_%s_cohort.npy" % tag, res["l1"])]

    # ---- calibration: are the quantile curves quantiles?  Coverage, pinball loss, band width and crossings, by cohort -------------------
    CALIBRATION_FILES = ("below", "below_t", "inside", "cross", "pinball", "width")

    def calibration_nominal(self) -> torch.Tensor:
        """``[3]`` float64: the nominal levels of the three curves -- ALD: 0.5, 0.5 + quantile_diff, 0.5 - quantile_diff (the heads mu_50,
        mu_75, mu_25 are trained so that P(actual < pred) = tau); Gauss: 0.5, Phi(2), Phi(-2) (mean, mean + 2 s, mean - 2 s)."""
        from .. import _lib as L
        if self.GAUSS:
            return torch.tensor([0.5, L.CALIBRATION_PHI2, L.CALIBRATION_PHIM2], dtype=torch.float64)
        d = float(self.config.quantile_diff)
        return torch.tensor([0.5, 0.5 + d, 0.5 - d], dtype=torch.float64)

    def calibration(self, observations, is_post, num_samples: int, cohorts=None, eps=None, chunk: int = 0, num_cohorts=None, **labels):
        """How the three curves of the family lie against the observations, per cohort (default: ONE cohort, the whole batch; else as
        ``cohort_moments``: a ``[B]`` id tensor or a tuple of label names).  Curves v_0, v_1, v_2: ``mu_50, mu_75, mu_25``, or ``mean,
        mean + 2 s, mean - 2 s`` (s = softplus(constant_std)) for the Gaussian family; their nominal levels under ``"nominal"`` ``[3]``.
        Over the members of a cohort x ``num_samples`` draws (those of ``recon_moments``): ``"below"`` ``[3, G, C]`` / ``"below_t"``
        ``[3, G, C, T]`` the fraction with ``y < v_j`` (calibrated: equal to nominal); ``"inside"`` / ``"inside_t"`` the fraction with
        ``v_2 <= y < v_1``; ``"cross"`` / ``"cross_t"`` the fraction whose curves cross (``v_2 > v_0`` or ``v_0 > v_1``); ``"pinball"``
        ``[3, G, C]`` the mean of ``(y - v_j)(tau_j - [y < v_j])``; ``"width"`` ``[G, C]`` the mean of ``v_1 - v_2``; ``"count"`` ``[G]``,
        ``"keys"``; the raw int32 tensors under ``"counts"`` (``below`` ``[3, G, C, T]``, ``inside``, ``cross`` ``[G, C, T]``).  An empty
        cohort has counts 0 and NaN elsewhere.  ONE engine call (``slode_calibration``): no ``[B, C, T, num_samples]`` tensor exists, and
        the counts are exact whatever the launch grid or ``chunk``.  Where the engine refuses (adaptive solver, strided observations,
        measured arms, more than 1024 cohorts) the same dict is composed from ``recon_samples`` in chunks of rows."""
        b = self._bind()
        B, ns = observations.shape[0], self._count(num_samples)
        if cohorts is None:
            cohorts, num_cohorts = torch.zeros(B, dtype=torch.int64, device=observations.device), 1
        ids, keys, G, members, offsets, count = self._cohort_lists(observations, cohorts, num_cohorts, labels)

        def fused():
            return b.engine.calibration(b.flat, self._draws_batch(observations, labels, eps, ns), B, is_post, ns, members, offsets, G, chunk=chunk)
        below, inside, cross, pinball, width = self._fused_or_composed(
            fused, lambda: self._calibration_composed(observations, is_post, ns, ids, G, count, eps, labels))
        T = observations.shape[2]
        den = (count.to(torch.float64) * ns).reshape(G, 1, 1)                  # (0 for an empty cohort: its fractions are NaN)
        res = {"nominal": self.calibration_nominal(), "pinball": pinball, "width": width, "count": count, "keys": keys,
               "counts": {"below": below, "inside": inside, "cross": cross}}
        for n, v in res["counts"].items():
            res[n + "_t"] = v.to(torch.float64) / den
            res[n] = v.to(torch.int64).sum(dim=-1).to(torch.float64) / (den[..., 0] * T)
        return res

    def _calibration_curves(self, got):
        """The three curves ``[rows, C, T, ns]`` (fp32, as the decoder gives them) of one ``recon_samples`` result."""
        if self.GAUSS:
            w = 2.0 * torch.nn.functional.softplus(self.decoder.constant_std.detach()).to(got["mean"].dtype)[None, :, :, None]
            return got["mean"], got["mean"] + w, got["mean"] - w
        return got["mu_50"], got["mu_75"], got["mu_25"]

    def _calibration_composed(self, observations, is_post, ns, ids, G, count, eps, labels):
        """The composed route: ``recon_samples`` of ``MOMENTS_CHUNK_ROWS // ns`` rows at a time (ONE drawing call for the whole batch, sliced
        per chunk); comparisons in torch, integer sums per cohort, the float summands (fp32, as the kernel forms them) added in fp64."""
        dev = observations.device
        Cn, T = observations.shape[1], observations.shape[2]
        slot = torch.where(ids < 0, torch.full_like(ids, G), ids)           # (bucket G: the trajectories of no cohort)
        tau = self.calibration_nominal().to(dev, torch.float32)
        n_int = torch.zeros(5, G + 1, Cn, T, dtype=torch.int64, device=dev)
        s_flt = torch.zeros(4, G + 1, Cn, dtype=torch.float64, device=dev)
        bad = torch.zeros(G + 1, dtype=torch.int64, device=dev)
        for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
            v = self._calibration_curves(self.recon_samples(is_post=is_post, num_samples=ns, eps=e, **d))
            y = d["observations"].to(torch.float32)[..., None]
            lt = [y < vj for vj in v]
            ind = lt + [(v[2] <= y) & lt[1], (v[2] > v[0]) | (v[0] > v[1])]
            for j, m in enumerate(ind):
                n_int[j].index_add_(0, slot[lo:hi], m.sum(dim=-1))
            terms = [(y - v[j]) * torch.where(lt[j], tau[j] - 1.0, tau[j]) for j in range(3)] + [v[1] - v[2]]
            for j, t in enumerate(terms):
                s_flt[j].index_add_(0, slot[lo:hi], t.to(torch.float64).sum(dim=(-1, -2)))
            bad.index_add_(0, slot[lo:hi], (torch.isnan(v[0]) | torch.isnan(v[1]) | torch.isnan(v[2])).flatten(1).any(dim=1).to(torch.int64))
            del v, lt, ind, terms
        den = (count.to(torch.float64) * ns * T).reshape(1, G, 1)
        flt = s_flt[:, :G] / den
        flt = torch.where(((count > 0) & (bad[:G] == 0)).reshape(1, G, 1), flt, torch.full_like(flt, float("nan"))).to(torch.float32)
        n32 = n_int[:, :G].to(torch.int32)
        return n32[:3].contiguous(), n32[3].contiguous(), n32[4].contiguous(), flt[:3].contiguous(), flt[3].contiguous()

    def save_calibration(self, results_dir: str, batches, is_post, num_samples: int, cohorts=None):
        """``calibration`` over a loader (an iterable of batch dicts: ``observations`` and the label tensors; a batch may carry its own
        ``cohorts`` ids and ``eps``), the cohorts -- ids or label names, merged across batches by their keys -- pooled: the integer counts
        added exactly (int64 on the host), the float means weighted by their point counts in fp64.  Writes ``calibration_{below,below_t,inside,cross,pinball,width}_
        <post|prior>.npy`` (fractions ``[3, G, C]``, ``[3, G, C, T]``, ``[G, C]``, ``[G, C]``; means ``[3, G, C]``, ``[G, C]``),
        ``calibration_nominal.npy`` and ``calibration_count.npy``; returns ``(paths, pooled result)``."""
        import numpy as np
        ns = self._count(num_samples)
        pool = {}                                                              # key row (tuple) -> sums
        for d in batches:
            d = dict(d)
            obs = d.pop("observations")
            res = self.calibration(obs, is_post, ns, cohorts=d.pop("cohorts", cohorts), **d)
            keys = res["keys"].cpu().numpy()
            cnt = res["count"].cpu().numpy().astype(np.int64)
            ints = {n: v.cpu().numpy().astype(np.int64) for n, v in res["counts"].items()}
            pin, wid = res["pinball"].cpu().numpy().astype(np.float64), res["width"].cpu().numpy().astype(np.float64)
            T = obs.shape[2]
            for g in range(len(cnt)):
                k = tuple(np.atleast_1d(keys[g]).tolist())
                p = pool.setdefault(k, {"count": 0, "below": 0, "inside": 0, "cross": 0, "pin": np.zeros(pin.shape[::2]),
                                        "wid": np.zeros(wid.shape[1:]), "pts": 0})
                p["count"] += int(cnt[g])
                for n in ("below", "inside", "cross"):
                    p[n] = p[n] + (ints[n][:, g] if n == "below" else ints[n][g])
                if cnt[g]:                                                     # (an empty cohort's NaN means carry no weight)
                    w = int(cnt[g]) * ns * T
                    p["pin"], p["wid"], p["pts"] = p["pin"] + w * pin[:, g], p["wid"] + w * wid[g], p["pts"] + w
        if not pool:
            raise ValueError("save_calibration: no batch")
        order = sorted(pool)
        cnt = np.array([pool[k]["count"] for k in order], dtype=np.int64)
        below = np.stack([pool[k]["below"] for k in order], axis=1)           # [3, G, C, T]
        inside, cross = (np.stack([pool[k][n] for k in order], axis=0) for n in ("inside", "cross"))
        T = below.shape[-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            den = (cnt * ns).astype(np.float64).reshape(-1, 1, 1)
            pts = np.array([pool[k]["pts"] for k in order], dtype=np.float64)
            out = {"below_t": below / den, "below": below.sum(-1) / (den[..., 0] * T), "inside": inside.sum(-1) / (den[..., 0] * T),
                   "cross": cross.sum(-1) / (den[..., 0] * T),
                   "pinball": np.stack([pool[k]["pin"] for k in order], axis=1) / pts.reshape(1, -1, 1),
                   "width": np.stack([pool[k]["wid"] for k in order], axis=0) / pts.reshape(-1, 1)}
        tag = "post" if is_post else "prior"
        named = [("calibration_%s_%s.npy" % (n, tag), torch.from_numpy(np.ascontiguousarray(out[n]))) for n in self.CALIBRATION_FILES]
        named += [("calibration_nominal.npy", self.calibration_nominal()), ("calibration_count.npy", torch.from_numpy(cnt))]
        out.update(count=cnt, keys=np.array(order), nominal=self.calibration_nominal().numpy(),
                   counts={"below": below, "inside": inside, "cross": cross})
        return self._save_arrays(results_dir, named), out

    @staticmethod
    def calibration_line(res, tag: str) -> str:
        """One line: nominal against empirical level per curve, band coverage, crossing share and pinball loss, pooled over the cohorts
        (weighted by their counts) and averaged over the channels."""
        import numpy as np
        cnt = np.asarray(res["count"], dtype=np.float64)
        w = cnt / max(cnt.sum(), 1.0)

        def pooled(a, axis):
            a = np.where(np.isnan(np.asarray(a, dtype=np.float64)), 0.0, np.asarray(a, dtype=np.float64))
            return np.tensordot(a, w, axes=([axis], [0]))
        below, pin = pooled(res["below"], 1).mean(-1), pooled(res["pinball"], 1).mean(-1)
        nom = np.asarray(res["nominal"], dtype=np.float64)
        levels = "  ".join("tau=%.4f:%.4f" % (nom[j], below[j]) for j in range(3))
        return "calibration_%s: %s  band=%.4f (nominal %.4f)  crossing=%.4f  pinball=(%.6f,%.6f,%.6f)  width=%.6f" % (
            tag, levels, pooled(res["inside"], 0).mean(), nom[1] - nom[2], pooled(res["cross"], 0).mean(), pin[0], pin[1], pin[2],
            pooled(res["width"], 0).mean())

    # ---- forecast: the same draws, solved on an output grid of the caller's -- past the observed window, or finer than the training grid ----
    def horizon_times(self, extra_steps: int, refine: int = 1) -> torch.Tensor:
        """The training grid with each interval split in ``refine`` equal parts, followed by ``extra_steps`` steps of the (refined) last
        spacing: ``[(T - 1) * refine + 1 + extra_steps]``, float32, on the model's device; it begins at the model's first time."""
        extra, refine = int(extra_steps), int(refine)
        if extra < 0 or refine < 1:
            raise ValueError("horizon_times needs extra_steps >= 0 and refine >= 1, got %d, %d" % (extra, refine))
        t = torch.as_tensor(self.times, dtype=torch.float32).reshape(-1).cpu()
        if refine > 1:
            frac = torch.arange(refine, dtype=torch.float32) / refine
            fine = (t[:-1, None] + (t[1:] - t[:-1])[:, None] * frac[None, :]).reshape(-1)
            t = torch.cat([fine, t[-1:]])
        if extra:
            h = t[-1] - t[-2]
            t = torch.cat([t, t[-1] + h * torch.arange(1, extra + 1, dtype=torch.float32)])
        return t.to(self.device)

    def _forecast_times(self, times_out) -> torch.Tensor:
        """``times_out`` as a float32 vector; ValueError unless it begins at the model's first time (x0 = initialize_state(z) is the state
        there, as ``odeint(f, x0, times)`` places it)."""
        t = times_out if torch.is_tensor(times_out) else torch.as_tensor(times_out, dtype=torch.float32)
        t0 = float(torch.as_tensor(self.times, dtype=torch.float32).reshape(-1)[0])
        if t.numel() < 2:
            raise ValueError("times_out needs at least two points, got %d" % t.numel())
        if float(t.reshape(-1)[0].to(torch.float32)) != t0:
            raise ValueError("times_out must begin at the model's first time %r (the initial state belongs there), got %r" % (t0, float(t.reshape(-1)[0])))
        return t

    def forecast_samples(self, observations, is_post, num_samples: int, times_out, eps=None, states: bool = False, posterior=None, **labels):
        """The materialising form of ``forecast_moments``: the head curves of ``num_samples`` latent draws on ``times_out``, ``[B, C, T_out,
        num_samples]`` each (``mu_50 / mu_75 / mu_25``, or ``mean``), ``"solution_xt"`` ``[B, T_out, S, num_samples]`` with ``states``, plus
        ``z`` ``[num_samples, B, L]``.  Composed from the encoder or the prior nets, ONE ODE solve of ``num_samples * B`` trajectories on
        ``times_out`` (``Engine.ode_solve(times=...)``: any solver, T_out within what ``slode_ode_solve_fwd`` takes) and the head weights
        as a torch matmul -- not ``slode_decode_heads``, whose std table is ``constant_std[C, T]`` of the training grid.  ``posterior`` =
        ``(loc, scale)`` ``[B, L]`` replaces the encoder's / the prior nets' distribution (``refine_posterior``: a refined posterior
        forecast); None (the default): unchanged."""
        b = self._bind()
        t = self._forecast_times(times_out)
        with torch.no_grad():
            B, ns = observations.shape[0], int(num_samples)
            loc, scale = self._loc_scale(observations, is_post, labels) if posterior is None else self._given_posterior(observations, posterior)
            _, z = self._draws(loc, scale, ns, eps)             # [ns, B, L]
            x = b.engine.ode_solve(b.flat, z.reshape(ns * B, -1).contiguous(), times=t)              # [ns * B, T_out, S]
            heads = b.engine.unpack(b.flat)
            res = {"z": z}
            for name, hn in zip(self.MOMENT_HEADS[bool(self.GAUSS)], b.engine.spec.head_names):
                mu = torch.matmul(x, heads["decoder.%s.0.weight" % hn].t())                         # [ns * B, T_out, C]
                res[name] = mu.reshape(ns, B, mu.shape[1], mu.shape[2]).permute(1, 3, 2, 0).contiguous()
            if states:
                res["solution_xt"] = x.reshape(ns, B, x.shape[1], x.shape[2]).permute(1, 2, 3, 0).contiguous()
            return res

    def forecast_moments(self, observations, is_post, num_samples: int, times_out, eps=None, states: bool = False, window: int = 0, **labels):
        """The posterior (``is_post``) or conditional-prior curves of these subjects on ``times_out`` -- any grid that begins at the model's
        first time: past the observed window (``horizon_times(n)``), finer than the training grid (``horizon_times(0, refine)``), longer
        than 1024 points -- as ``{"mu_50": (mean, sd), "mu_75": ..., "mu_25": ...}`` (``{"mean": (mean, sd)}`` for the Gaussian family),
        mean and population sd over ``num_samples`` latent draws, ``[B, C, T_out]`` each; ``states`` adds ``"solution_xt": (mean, sd)``,
        ``[B, T_out, S]``, the same moments of the ODE state.  The draws are those of ``recon_moments`` (same noise convention: ``eps``
        ``[num_samples, B, L]`` or one drawing call); no observation noise is added (``constant_std`` exists on the training grid only).
        ONE engine call (``slode_forecast_moments``), which walks the grid in windows of ``window`` steps (0: the library's choice).  Where
        the engine refuses (adaptive solver, strided observations, measured arms, the plan) the same dict is composed from
        ``forecast_samples`` in chunks over B."""
        b = self._bind()
        B, ns = observations.shape[0], self._count(num_samples)
        t = self._forecast_times(times_out)
        names = self.MOMENT_HEADS[bool(self.GAUSS)]

        def fused():
            mean, sd, xm, xs = b.engine.forecast_moments(b.flat, self._draws_batch(observations, labels, eps, ns), B, is_post, ns, t,
                                                         states=states, window=window)
            res = {n: (mean[q], sd[q]) for q, n in enumerate(names)}
            if states:
                res["solution_xt"] = (xm.permute(0, 2, 1), xs.permute(0, 2, 1))
            return res
        return self._fused_or_composed(fused, lambda: self._composed_moments(
            observations, labels, ns, eps,
            lambda lo, hi, e, d: self.forecast_samples(is_post=is_post, num_samples=ns, times_out=t, eps=e, states=states, **d),
            self._mean_sd, names=names + (("solution_xt",) if states else ())))

    def save_forecast_moments(self, results_dir: str, observations, is_post, num_samples: int, times_out, **labels):
        """Writes ``<curve>_<post|prior>_forecast_mean.npy`` / ``..._forecast_sd.npy`` (``[B, C, T_out]`` each) for every head curve and
        ``forecast_times.npy`` (``[T_out]``); returns the paths."""
        res = self.forecast_moments(observations, is_post, num_samples, times_out, **labels)
        tag = "post" if is_post else "prior"
        named = [("%s_%s_forecast_%s.npy" % (name, tag, kind), val) for name, moments in res.items() for kind, val in zip(("mean", "sd"), moments)]
        t = times_out if torch.is_tensor(times_out) else torch.as_tensor(times_out, dtype=torch.float32)
        return self._save_arrays(results_dir, named + [("forecast_times.npy", t.detach().to(torch.float32).reshape(-1))])

    # ---- counterfactual curves: the subject's own latent groups kept, the intervened groups redrawn from p(z_g | u'_g) on the same noise ----
    def _intervened(self, intervene, labels):
        """(group_mask, labels with the counterfactual tensors swapped in) of ``intervene`` = {label name: tensor [B, u_dim]}: bit g of the
        mask is set when a label of prior group g (``PRIORS`` order = the engine's) is named.  A name that is no conditional-prior label of the
        family raises ValueError."""
        known = [l for _, ls, _ in self.PRIORS for l in ls]
        mask, swapped = 0, dict(labels)
        for name, val in intervene.items():
            if name not in known:
                raise ValueError("intervene: %r is not a conditional-prior label of the %s family (labels: %s)" % (name, self.FAMILY, ", ".join(known)))
            if val.numel() != labels[name].numel():
                raise ValueError("intervene[%r] must hold %d values, got %s" % (name, labels[name].numel(), tuple(val.shape)))
            swapped[name] = val.reshape(labels[name].shape).to(labels[name].device)
            mask |= 1 << next(g for g, (_, ls, _) in enumerate(self.PRIORS) if name in ls)
        return mask, swapped

    def counterfactual_samples(self, observations, num_samples: int, intervene, eps=None, **labels):
        """The materialising form of ``intervention_moments``: ``{"mu_50": (factual, counterfactual), ...}`` (``{"mean": ...}`` for the Gaussian
        family), each tensor ``[B, C, T, num_samples]``, plus ``"z"``: the two latents ``[num_samples, B, L]``.  Draw k of trajectory b uses
        ONE noise row for both arms: z_f = loc(x) + scale(x) eps; z_cf = z_f outside the intervened prior groups and
        ploc_g(u') + pscale_g(u') eps inside them (``_prior_loc_scale`` on the swapped labels).  Composed from the encoder, the prior nets and
        ``decoder.forward`` on both latents; ``eps`` ``[num_samples, B, L]`` or None (one drawing call of the engine's generator)."""
        mask, swapped = self._intervened(intervene, labels)
        self._bind()
        with torch.no_grad():
            loc, scale = self.encoder.forward(observations)
            cloc, cscale = loc.clone(), scale.clone()
            if mask:
                ploc, pscale = self._prior_loc_scale(swapped)
                for g, (_, _, zgroups) in enumerate(self.PRIORS):
                    if (mask >> g) & 1:
                        lo = self.z_off[zgroups[0]]
                        hi = lo + sum(self.z_dims[z] for z in zgroups)
                        cloc[:, lo:hi], cscale[:, lo:hi] = ploc[:, lo:hi], pscale[:, lo:hi]
            e, z_f = self._draws(loc, scale, int(num_samples), eps)
            z_cf = cloc.unsqueeze(0) + cscale.unsqueeze(0) * e
            arms = [self._decoded_draws(z) for z in (z_f, z_cf)]
            res = {n: (arms[0][n], arms[1][n]) for n in self.MOMENT_HEADS[bool(self.GAUSS)]}
            res["z"] = (z_f, z_cf)
            return res

    def intervention_moments(self, observations, num_samples: int, intervene, eps=None, **labels):
        """"What would THIS subject's curves have looked like under THAT input?": per head curve
        ``{"mu_50": {"cf": (mean, sd), "effect": (mean, sd)}, ...}`` (``{"mean": ...}`` for the Gaussian family), each tensor ``[B, C, T]`` --
        the mean and the population sd over ``num_samples`` draws of the counterfactual curve, and of the PAIRED difference counterfactual -
        factual (both arms of a draw share their noise, so ``z_epsilon`` and the groups left alone cancel in the effect).  ``intervene`` maps
        label names of the family's conditional priors to counterfactual tensors ``[B, u_dim]``; every prior group with a named label is
        redrawn from p(z_g | u'_g), the other latent dims keep the subject's posterior draw.  ONE engine call (``slode_intervene_moments``):
        no ``[B, C, T, num_samples]`` tensor exists.  ``eps`` ``[num_samples, B, L]`` makes it reproducible; None draws one call of the
        engine's generator.  Where the engine refuses (adaptive solver, strided observations, measured arms, LDS budget) the same dict is
        composed from ``counterfactual_samples`` in chunks over B."""
        B, ns = observations.shape[0], self._count(num_samples)
        mask, swapped = self._intervened(intervene, labels)
        b = self._bind()
        # every label tensor goes to the engine, the named ones with their counterfactual values: a prior group over several labels
        # (challenge, proc) reads all of its columns, whichever of them were named
        cf = self._label_tensors(swapped, B)

        def fused():
            cm, cs, em, es = b.engine.intervene_moments(b.flat, self._draws_batch(observations, labels, eps, ns), B, cf if mask else None, mask, ns)
            return {n: {"cf": (cm[q], cs[q]), "effect": (em[q], es[q])} for q, n in enumerate(self.MOMENT_HEADS[bool(self.GAUSS)])}

        def paired(arms):      # (factual, counterfactual) [rows, C, T, ns] -> moments of the counterfactual and of the paired difference
            f, c = (v.to(torch.float32) for v in arms)
            d = c - f
            return c.mean(dim=-1), c.std(dim=-1, unbiased=False), d.mean(dim=-1), d.std(dim=-1, unbiased=False)

        def composed():
            res = self._composed_moments(observations, labels, ns, eps, lambda lo, hi, e, d: self.counterfactual_samples(
                num_samples=ns, intervene={k: swapped[k][lo:hi] for k in intervene}, eps=e, **d), paired)
            return {n: {"cf": (v[0], v[1]), "effect": (v[2], v[3])} for n, v in res.items()}
        return self._fused_or_composed(fused, composed)

    def save_intervention_moments(self, results_dir: str, observations, num_samples: int, intervene, **labels):
        """Writes ``<curve>_cf_<names>_sample_mean.npy`` / ``..._sample_sd.npy`` and ``<curve>_effect_<names>_sample_mean.npy`` /
        ``..._sample_sd.npy`` (``[B, C, T]`` each) for every head curve, ``<names>`` the intervened label names joined by '+' in the order
        given."""
        res = self.intervention_moments(observations, num_samples, intervene, **labels)
        tag = "+".join(intervene)
        return self._save_arrays(results_dir, (("%s_%s_%s_sample_%s.npy" % (name, arm, tag, kind), val) for name, arms in res.items()
                                               for arm in ("cf", "effect") for kind, val in zip(("mean", "sd"), arms[arm])))

    # ---- latent attribution: how much of the variance of the curves comes from which latent block (pick-freeze / Jansen) ----------------
    ATTRIBUTION_ARMS_PER_CALL = None      # most arms of one engine call; None: what the engine's plan says fits the LDS (at most 16)

    def attribution_blocks(self):
        """The latent blocks of the family by name, in bit order: every conditional-prior group (its latent groups joined by '+': ``iext``,
        ``rtpr``; ``shedding+symptoms``; ``aR+aS+C12+C6``), then ``epsilon`` -- the dims no prior group covers -- when there are any."""
        names = ["+".join(zg) for _, _, zg in self.PRIORS]
        if sum(self.z_dims[z] for _, _, zg in self.PRIORS for z in zg) < self.latent_dim:
            names.append("epsilon")
        return names

    def _block_dims(self, mask):
        """bool ``[L]``: the latent dims of the blocks in ``mask`` (bit order of ``attribution_blocks``)."""
        sel = torch.zeros(self.latent_dim, dtype=torch.bool)
        rest = torch.ones(self.latent_dim, dtype=torch.bool)
        for g, (_, _, zg) in enumerate(self.PRIORS):
            lo = self.z_off[zg[0]]
            hi = lo + sum(self.z_dims[z] for z in zg)
            rest[lo:hi] = False
            if (mask >> g) & 1:
                sel[lo:hi] = True
        return sel | rest if (mask >> len(self.PRIORS)) & 1 else sel

    def _attribution_arms(self, blocks):
        """``(blocks, masks, single, complement)``: the deduplicated arm masks of ``blocks`` (None: all of them) -- each single block, and
        every block of the family but that one -- and per block the index of its two arms in ``masks``."""
        known = self.attribution_blocks()
        blocks = list(known) if blocks is None else list(blocks)
        for name in blocks:
            if name not in known:
                raise ValueError("blocks: %r is not a latent block of the %s family (blocks: %s)" % (name, self.FAMILY, ", ".join(known)))
        if not blocks:
            raise ValueError("blocks names no latent block (blocks: %s)" % ", ".join(known))
        every = (1 << len(known)) - 1
        masks, single, comp = [], [], []
        for name in blocks:
            bit = 1 << known.index(name)
            for m, idx in ((bit, single), (every ^ bit, comp)):
                if m not in masks:
                    masks.append(m)
                idx.append(masks.index(m))
        return blocks, masks, single, comp

    def _attribution_result(self, blocks, single, comp, mean, var, msd):
        """The dict of ``latent_attribution`` from mean / var ``[Q, B, C, T]`` and msd ``[A, Q, B, C, T]``."""
        res = {"blocks": list(blocks)}
        for q, n in enumerate(self.MOMENT_HEADS[bool(self.GAUSS)]):
            total = torch.stack([msd[a][q] for a in single], 0)
            first = torch.stack([var[q] - msd[a][q] for a in comp], 0)
            den = var[q].double().sum(-1)
            den = torch.where(den == 0, torch.full_like(den, float("nan")), den)
            res[n] = {"mean": mean[q].to(torch.float32), "var": var[q].to(torch.float32), "total": total.to(torch.float32),
                      "first": first.to(torch.float32), "total_index": total.double().sum(-1) / den, "first_index": first.double().sum(-1) / den}
        return res

    def latent_attribution(self, observations, is_post, num_samples: int, blocks=None, eps=None, **labels):
        """How much of the variation of a subject's curves comes from which latent block, at which channel and time: the variance
        (Sobol / ANOVA) decomposition of every head curve over the independent blocks of the latent -- the conditional-prior groups and
        ``epsilon`` (``attribution_blocks``) -- under the posterior q(z | x) (``is_post``) or the conditional prior p(z | labels), estimated
        by pick-freeze over ``num_samples`` draws: a base draw z = loc + scale e and, per arm, the same draw with some blocks redrawn on a
        second noise row e'; msd = 1 / (2 ns) sum_k (v_arm,k - v_k)^2 (Jansen).  Returns ``{"blocks": [P names], "mu_50": {...}, "mu_75":
        ..., "mu_25": ...}`` (``"mean"`` alone for the Gaussian family), per head curve

        * ``"mean"``, ``"var"`` ``[B, C, T]``: mean and population variance of the base curve (the square of ``recon_moments``' sd);
        * ``"total"`` ``[P, B, C, T]``: the block's total-effect variance E[Var(f | z_~g)] = msd of the arm that redraws the block alone;
        * ``"first"`` ``[P, B, C, T]``: the block's first-order variance Var(E[f | z_g]) = var - msd of the arm that redraws every other
          block.  NOT clipped: estimator noise can make it negative, or larger than ``total``;
        * ``"total_index"``, ``"first_index"`` ``[P, B, C]`` float64: sum_t total / sum_t var (and first), NaN where sum_t var == 0.

        ``blocks`` names the P blocks wanted (default: all).  Arms with equal masks are shared, so a two-block family needs two arms, and
        there ``first_index[0] == 1 - total_index[1]``.  ONE engine call (``slode_latent_attribution``) where the arms fit the LDS, else the
        fewest calls that do, all on the same noise: no ``[B, C, T, num_samples]`` tensor exists, and the split changes no bit.  ``eps``
        ``[2, num_samples, B, L]`` (base, fresh) makes it reproducible; None takes drawing calls n and n + 1 of the engine's generator (the
        counter ends at n + 2).  Where the engine refuses (adaptive solver, strided observations, measured arms, LDS budget) the same dict
        is composed from ``_decoded_draws`` on every arm's latents in chunks over B, reduced in fp64."""
        from .. import _lib as L
        b = self._bind()
        B, ns = observations.shape[0], self._count(num_samples)
        blocks, masks, single, comp = self._attribution_arms(blocks)
        if eps is not None:
            eps = eps.to(torch.float32).reshape(2, ns, B, -1).contiguous()

        def fused():
            eng = b.engine
            slices = self._fewest_calls(len(masks), min(L.ATTRIBUTION_MAX_ARMS, self.ATTRIBUTION_ARMS_PER_CALL or L.ATTRIBUTION_MAX_ARMS),
                                        lambda n: eng.attribution_plan(B, n))
            bt = eng.make_batch(observations, self._label_tensors(labels, B), eps, particles=ns,
                                eps_shape=None if eps is None else (2, ns, B, eng.spec.latent_dim))
            got = self._on_the_same_noise(eng, eps, slices, lambda lo, hi: eng.latent_attribution(      # (drawing calls n0, n0 + 1 every time)
                b.flat, bt, B, is_post, ns, masks[lo:hi], mean=None if lo == 0 else False, sd=None if lo == 0 else False))
            (mean, sd, _), parts = got[0], [g[2] for g in got]
            return self._attribution_result(blocks, single, comp, mean, sd * sd, parts[0] if len(parts) == 1 else torch.cat(parts, 0))

        def composed():
            with torch.no_grad():
                e0, e1 = (eps[0], eps[1]) if eps is not None else (self._noise(ns, B, None), self._noise(ns, B, None))
                names = self.MOMENT_HEADS[bool(self.GAUSS)]
                rows = max(1, self.MOMENTS_CHUNK_ROWS // ns)
                cols = []
                for lo in range(0, B, rows):
                    hi = min(B, lo + rows)
                    d = {k: v[lo:hi] for k, v in labels.items()}
                    loc, scale = self._loc_scale(observations[lo:hi], is_post, d)
                    a0, a1 = e0[:, lo:hi].to(loc.device), e1[:, lo:hi].to(loc.device)
                    base = {n: v.double() for n, v in self._decoded_draws(loc.unsqueeze(0) + scale.unsqueeze(0) * a0).items()}
                    mean = torch.stack([base[n].mean(-1) for n in names], 0)
                    var = torch.stack([base[n].var(-1, unbiased=False) for n in names], 0)
                    msd = []
                    for m in masks:
                        e = torch.where(self._block_dims(m).to(loc.device), a1, a0)
                        arm = self._decoded_draws(loc.unsqueeze(0) + scale.unsqueeze(0) * e)
                        msd.append(torch.stack([0.5 * ((arm[n].double() - base[n]) ** 2).mean(-1) for n in names], 0))
                        del arm
                    cols.append((mean, var, torch.stack(msd, 0)))
                    del base
                mean, var, msd = torch.cat([c[0] for c in cols], 1), torch.cat([c[1] for c in cols], 1), torch.cat([c[2] for c in cols], 2)
                return self._attribution_result(blocks, single, comp, mean, var, msd)
        return self._fused_or_composed(fused, composed)

    def save_latent_attribution(self, results_dir: str, batches, is_post, num_samples: int):
        """Runs ``latent_attribution`` (all blocks) over ``batches`` (an iterable of device batch dicts: ``observations`` + the label
        tensors) and writes ``attribution_total_<post|prior>.npy`` / ``attribution_first_<post|prior>.npy``, float32 ``[Q, P, n, C, T]`` (head
        curves in the engine's order, blocks, the trajectories in loader order), ``attribution_total_index_<post|prior>.npy`` /
        ``attribution_first_index_<post|prior>.npy``, float64 ``[Q, P, n, C]``, and ``attribution_blocks.txt``, one block name per line.  One
        read-back, at the end.  Returns the paths."""
        names = self.MOMENT_HEADS[bool(self.GAUSS)]
        tag = "post" if is_post else "prior"

        def blocks(path, _):
            with open(path, "w") as f:
                f.write("\n".join(self.attribution_blocks()) + "\n")
        return self._save_over_batches(
            results_dir, batches, lambda **d: self.latent_attribution(is_post=is_post, num_samples=num_samples, **d),
            lambda r: (("attribution_%s_%s.npy" % (k, tag), torch.stack([r[n][k] for n in names], 0))
                       for k in ("total", "first", "total_index", "first_index")), dim=2, side=("attribution_blocks.txt", blocks))

    def attribution_line(self, total_index, first_index, tag):
        """One printed line of a ``save_latent_attribution`` pass: per block, the mean over head curves, trajectories and channels of the
        total and the first-order index (NaN entries -- curves without variance -- left out)."""
        import numpy as np
        t, f = (np.asarray(a, dtype=np.float64) for a in (total_index, first_index))
        cells = ["%s total=%.3f first=%.3f" % (n, float(np.nanmean(t[:, p])), float(np.nanmean(f[:, p])))
                 for p, n in enumerate(self.attribution_blocks())]
        return "attribution_%s: n=%d  %s" % (tag, t.shape[2], "  ".join(cells))

    # ---- curve summaries: peak, time to peak, area and threshold crossing of every draw's curve ------------------------------------------
    SUMMARY_NAMES = ("peak", "t_peak", "trough", "t_trough", "auc", "time_beyond", "t_hit", "crossed")   # the slots of slode_curve_summary

    @staticmethod
    def _summary_sense(sense) -> int:
        """``"above"`` / ``"below"`` (or +1 / -1) as the engine's +1 / -1; ValueError otherwise."""
        if sense in ("above", 1):
            return 1
        if sense in ("below", -1):
            return -1
        raise ValueError("sense must be 'above' or 'below', got %r" % (sense,))

    def _summary_weights(self, device, grid=None):
        """``(times, w)`` float32 [T] on ``device``: the grid and the trapezoid node weights w_0 = 0.5 (t_1 - t_0), w_i = 0.5 (t_{i+1} -
        t_{i-1}), w_{T-1} = 0.5 (t_{T-1} - t_{T-2}), formed in fp32 as the kernel forms them.  ``grid``: the grid to take them on (None:
        the model's own)."""
        t = torch.as_tensor(self.times if grid is None else grid, dtype=torch.float32).reshape(-1).to(device)
        i = torch.arange(t.numel(), device=device)
        return t, 0.5 * (t[(i + 1).clamp(max=t.numel() - 1)] - t[(i - 1).clamp(min=0)])

    def _summary_functionals(self, v, thr, sense, grid=None):
        """The eight functionals of the curves ``v`` ``[rows, C, T, ns]`` in torch, on the definitions of ``slode_curve_summary``:
        ``(f [rows, C, ns, 8] float32, beyond [rows, C, T, ns] bool or None)``.  First indices are a masked ``min`` over the index (torch's
        argmax tie rule is not relied on); ``t_hit`` of a draw that does not cross is NaN; ``thr`` None: slots 5 - 7 are NaN.  ``grid``:
        the T times the curves live on (None: the model's own grid)."""
        v = v.to(torch.float32)
        T = v.shape[2]
        t, w = self._summary_weights(v.device, grid)
        idx = torch.arange(T, device=v.device).reshape(1, 1, T, 1)

        def first(mask):
            return torch.where(mask, idx, torch.full_like(idx, T)).amin(dim=2)
        peak, trough = v.amax(dim=2), v.amin(dim=2)
        t_peak, t_trough = t[first(v == peak.unsqueeze(2))], t[first(v == trough.unsqueeze(2))]
        auc = (w.reshape(1, 1, T, 1) * v).sum(dim=2)
        nan = torch.full_like(auc, float("nan"))
        beyond = None
        if thr is None:
            tb, t_hit, crossed = nan, nan, nan
        else:
            th = torch.as_tensor(thr, dtype=torch.float32, device=v.device).reshape(1, -1, 1, 1)
            beyond = v > th if sense > 0 else v < th
            tb = (w.reshape(1, 1, T, 1) * beyond.to(torch.float32)).sum(dim=2)
            ih = first(beyond)
            crossed = (ih < T).to(torch.float32)
            t_hit = torch.where(ih < T, t[ih.clamp(max=T - 1)], nan)
        return torch.stack([peak, t_peak, trough, t_trough, auc, tb, t_hit, crossed], dim=-1), beyond

    @staticmethod
    def _summary_moments(f):
        """``(mean, sd)`` ``[rows, C, 8]`` over the draw axis of ``f`` ``[rows, C, ns, 8]``: population sd; NaN entries (``t_hit`` of the
        draws that do not cross) are left out, a slot with none left is NaN."""
        ok = ~torch.isnan(f)
        n = ok.sum(dim=2).to(f.dtype)
        f0 = torch.where(ok, f, torch.zeros_like(f))
        mean = f0.sum(dim=2) / n                                           # n = 0: 0 / 0 = NaN
        dev = torch.where(ok, f - mean.unsqueeze(2), torch.zeros_like(f))
        return mean, ((dev * dev).sum(dim=2) / n).sqrt()

    def curve_summary(self, observations, is_post, num_samples: int, thresholds=None, sense="above", eps=None, pointwise: bool = False, **labels):
        """What one asks of a curve -- how high does it get and when, how much is there in total, does it cross a level, when first and for
        how long -- over ``num_samples`` latent draws: per head curve name (``mu_50``, ``mu_75``, ``mu_25``; ``mean`` for the Gaussian
        family) a dict of ``(mean, sd)`` pairs, ``[B, C]`` each, under ``"peak"``, ``"t_peak"``, ``"trough"``, ``"t_trough"``, ``"auc"``
        (trapezoid rule on the model's grid), ``"time_beyond"``, ``"t_hit"`` (over the draws that cross; NaN where none does) and
        ``"crossed"`` (``P(cross)``, ``sqrt(p (1 - p))``); ``pointwise=True`` adds ``"p_beyond"`` ``[B, C, T]``, the share of draws beyond
        the threshold at every point.  These are functionals of every draw's whole curve: the moments of ``recon_moments`` do not yield
        them.  ``thresholds``: a length-C sequence or tensor, read on the host once (None: the three threshold entries are NaN and
        ``pointwise`` is refused); ``sense``: ``"above"`` or ``"below"``.  ONE engine call (``slode_curve_summary``) on the draws of
        ``recon_moments`` (same ``eps`` / generator use); where the engine refuses (adaptive solver, strided observations, measured arms,
        LDS budget) the same dict is composed from ``recon_samples`` in chunks over B, the functionals in torch on the same definitions."""
        b = self._bind()
        B, ns, sn = observations.shape[0], self._count(num_samples), self._summary_sense(sense)
        thr = None if thresholds is None else [float(x) for x in torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1).tolist()]
        if thr is not None and len(thr) != observations.shape[1]:
            raise ValueError("thresholds must hold %d values (one per channel), got %d" % (observations.shape[1], len(thr)))
        if pointwise and thr is None:
            raise ValueError("pointwise=True needs thresholds")
        names = self.MOMENT_HEADS[bool(self.GAUSS)]

        def pack(mean, sd, p):
            return {n: dict({k: (mean[q][..., j], sd[q][..., j]) for j, k in enumerate(self.SUMMARY_NAMES)}, **({"p_beyond": p[q]} if pointwise else {}))
                    for q, n in enumerate(names)}

        def fused():
            return pack(*b.engine.curve_summary(b.flat, self._draws_batch(observations, labels, eps, ns), B, is_post, ns, thr, sn, None, True,
                                                True if pointwise else None))

        def composed():
            cols = {n: ([], [], []) for n in names}
            for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
                res = self.recon_samples(is_post=is_post, num_samples=ns, eps=e, **d)
                for n in names:
                    f, beyond = self._summary_functionals(res[n], thr, sn)
                    m, s = self._summary_moments(f)
                    cols[n][0].append(m); cols[n][1].append(s)
                    if pointwise:
                        count = beyond.to(torch.float32).sum(dim=-1)                 # exact; count / ns as the kernel divides it (a tensor
                        cols[n][2].append(count / torch.full_like(count, float(ns)))     # divisor: a true division, not a reciprocal multiply)
                del res
            return pack([torch.cat(cols[n][0], 0) for n in names], [torch.cat(cols[n][1], 0) for n in names],
                        [torch.cat(cols[n][2], 0) if pointwise else None for n in names])
        return self._fused_or_composed(fused, composed)

    def save_curve_summary(self, results_dir: str, batches, is_post, num_samples: int, thresholds=None, sense="above"):
        """Runs ``curve_summary`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors) and writes
        ``summary_<curve>_<post|prior>_mean.npy`` / ``..._sd.npy``, float32 ``[n, C, 8]`` (the trajectories in loader order, the slots in
        ``SUMMARY_NAMES`` order), and ``summary_slots.npy``, the slot names.  One read-back, at the end.  Returns the paths."""
        import numpy as np
        names = self.MOMENT_HEADS[bool(self.GAUSS)]
        tag = "post" if is_post else "prior"
        return self._save_over_batches(
            results_dir, batches, lambda **d: self.curve_summary(is_post=is_post, num_samples=num_samples, thresholds=thresholds, sense=sense, **d),
            lambda r: (("summary_%s_%s_%s.npy" % (n, tag, ("mean", "sd")[k]), torch.stack([r[n][slot][k] for slot in self.SUMMARY_NAMES], -1))
                       for n in names for k in (0, 1)),
            side=("summary_slots.npy", lambda path, _: np.save(path, np.array(self.SUMMARY_NAMES))))

    def summary_line(self, mean, tag, with_threshold: bool, name: str = "curve_summary"):
        """One printed line of a ``save_curve_summary`` pass from the central curve's ``mean`` array ``[n, C, 8]``: per channel, the mean over
        trajectories of the mean peak, time to peak and AUC and, with thresholds, of ``P(cross)`` and ``t_hit`` (NaN entries left out).
        ``name``: the line's prefix (``save_forecast_summary``'s pass: ``"forecast_summary"``)."""
        import numpy as np
        m = np.asarray(mean, dtype=np.float64)
        cells = []
        for c in range(m.shape[1]):
            cell = "c%d peak=%.4g t_peak=%.4g auc=%.4g" % (c, m[:, c, 0].mean(), m[:, c, 1].mean(), m[:, c, 4].mean())
            if with_threshold:
                hit = m[:, c, 6]
                cell += " p_cross=%.3f t_hit=%.4g" % (m[:, c, 7].mean(), float(np.nanmean(hit)) if np.isfinite(hit).any() else float("nan"))
            cells.append(cell)
        return "%s_%s: n=%d  %s" % (name, tag, m.shape[0], "  ".join(cells))

    # ---- forecast summaries: the same functionals from a time on, on any output grid -------------------------------------------------------
    @staticmethod
    def _first_point(times_out, since) -> int:
        """The first index of ``times_out`` whose time has reached ``since``, in the grid's own direction (an increasing grid: t >= since; a
        decreasing one: t <= since); None: 0.  Found on the host.  ValueError where no point of the grid has reached it."""
        if since is None:
            return 0
        t = torch.as_tensor(times_out).detach().to("cpu", torch.float32).reshape(-1)
        s = torch.tensor(float(since), dtype=torch.float32)
        reached = (t >= s) if bool(t[-1] >= t[0]) else (t <= s)
        idx = torch.nonzero(reached)
        if idx.numel() == 0:
            raise ValueError("since = %r lies beyond the output grid [%r, %r]" % (float(since), float(t[0]), float(t[-1])))
        return int(idx[0])

    def forecast_summary(self, observations, is_post, num_samples: int, times_out, since=None, thresholds=None, sense="above", eps=None,
                         window: int = 0, **labels):
        """Will the curve cross the level after the observed window, when, how high will it still get and how much is still to come: the
        functionals of ``curve_summary`` over ``num_samples`` latent draws, taken on the part of ``times_out`` from the time ``since`` on
        (None: the whole grid).  ``times_out`` is any grid ``forecast_moments`` takes (``horizon_times(n)``, finer, longer than 1024 points).
        Returns per head curve name a dict of ``(mean, sd)`` pairs, ``[B, C]`` each, under the eight names of ``curve_summary`` -- the area
        and ``time_beyond`` by the trapezoid rule on the sub-grid, ``t_hit`` over the draws that cross at or after ``since`` (a draw already
        beyond the level there hits there; NaN where none crosses) -- plus ``"first_point"``, the index of the first grid point used: the
        first whose time has reached ``since``, in the grid's own direction.  That index is found on the host: a device-resident
        ``times_out`` synchronises there, as ``cohort_index`` does; a ``since`` beyond the grid is a ValueError.  The moments of
        ``forecast_moments`` do not yield these: the peak of the mean forecast is not the mean of the peaks.  ``thresholds`` / ``sense`` /
        ``eps``: as ``curve_summary``.  ONE engine call (``slode_forecast_summary``), which walks the grid in windows of ``window`` steps (0:
        the library's choice) and keeps nothing sized by ``num_samples`` or by the grid.  Where the engine refuses (adaptive solver, strided
        observations, measured arms) the same dict is composed from ``forecast_samples`` in chunks over B (T_out <= 1024), the functionals
        in torch on ``times_out[first_point:]``."""
        b = self._bind()
        B, ns, sn = observations.shape[0], self._count(num_samples), self._summary_sense(sense)
        thr = None if thresholds is None else [float(x) for x in torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1).tolist()]
        if thr is not None and len(thr) != observations.shape[1]:
            raise ValueError("thresholds must hold %d values (one per channel), got %d" % (observations.shape[1], len(thr)))
        t = self._forecast_times(times_out)
        i0 = self._first_point(t, since)
        names = self.MOMENT_HEADS[bool(self.GAUSS)]

        def pack(mean, sd):
            return {n: dict({k: (mean[q][..., j], sd[q][..., j]) for j, k in enumerate(self.SUMMARY_NAMES)}, first_point=i0)
                    for q, n in enumerate(names)}

        def fused():
            return pack(*b.engine.forecast_summary(b.flat, self._draws_batch(observations, labels, eps, ns), B, is_post, ns, t, first_point=i0,
                                                   thr=thr, sense=sn, mean=None, sd=True, window=window))

        def composed():
            sub = torch.as_tensor(t, dtype=torch.float32).reshape(-1)[i0:]
            cols = {n: ([], []) for n in names}
            for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
                res = self.forecast_samples(is_post=is_post, num_samples=ns, times_out=t, eps=e, **d)
                for n in names:
                    f, _ = self._summary_functionals(res[n][:, :, i0:], thr, sn, grid=sub)
                    m, s = self._summary_moments(f)
                    cols[n][0].append(m); cols[n][1].append(s)
                del res
            return pack([torch.cat(cols[n][0], 0) for n in names], [torch.cat(cols[n][1], 0) for n in names])
        return self._fused_or_composed(fused, composed)

    def save_forecast_summary(self, results_dir: str, batches, is_post, num_samples: int, times_out, since=None, thresholds=None, sense="above"):
        """Runs ``forecast_summary`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors) and writes
        ``summary_<curve>_<post|prior>_forecast_mean.npy`` / ``..._forecast_sd.npy``, float32 ``[n, C, 8]`` (the trajectories in loader
        order, the slots in ``SUMMARY_NAMES`` order), and ``forecast_times.npy`` (``[T_out]``).  One read-back, at the end.  Returns the
        paths."""
        import numpy as np
        names = self.MOMENT_HEADS[bool(self.GAUSS)]
        tag = "post" if is_post else "prior"
        tt = (times_out if torch.is_tensor(times_out) else torch.as_tensor(times_out, dtype=torch.float32)).detach().to(torch.float32).reshape(-1)
        return self._save_over_batches(
            results_dir, batches,
            lambda **d: self.forecast_summary(is_post=is_post, num_samples=num_samples, times_out=times_out, since=since, thresholds=thresholds,
                                              sense=sense, **d),
            lambda r: (("summary_%s_%s_forecast_%s.npy" % (n, tag, ("mean", "sd")[k]), torch.stack([r[n][slot][k] for slot in self.SUMMARY_NAMES], -1))
                       for n in names for k in (0, 1)),
            side=("forecast_times.npy", lambda path, _: np.save(path, tt.cpu().numpy())))

    # ---- counterfactual summaries: peak, AUC and crossing of THIS subject's curves under V hypothesised inputs, with the paired effects ----
    INTERVENTION_SUMMARY_ARMS_PER_CALL = None     # most hypotheses of one engine call; None: what the engine's plan says fits the LDS (at most 64)
    SUMMARY_ARMS = ("factual", "cf", "effect")

    def _summary_hypotheses(self, hypotheses):
        """``(V, tables, group_mask)`` of ``hypotheses`` = {label name: [V, width]} (``_hypothesis_tables``): every named label must be a
        conditional-prior label of the family (``_intervened``'s error); bit g of the mask is set when a label of prior group g is named."""
        V, tabs = self._hypothesis_tables(hypotheses)
        known = [l for _, ls, _ in self.PRIORS for l in ls]
        mask = 0
        for name, t in tabs.items():
            if name not in known:
                raise ValueError("intervene: %r is not a conditional-prior label of the %s family (labels: %s)" % (name, self.FAMILY, ", ".join(known)))
            if t.shape[1] != self.label_dims[name]:
                raise ValueError("hypotheses[%r] must be [V, %d], got %s" % (name, self.label_dims[name], tuple(t.shape)))
            mask |= 1 << next(g for g, (_, ls, _) in enumerate(self.PRIORS) if name in ls)
        return V, tabs, mask

    def intervention_summary(self, observations, num_samples: int, hypotheses, thresholds=None, sense="above", eps=None, **labels):
        """"By how much does input u' change THIS subject's peak, its total, and does the curve still cross the level?": the functionals of
        ``curve_summary`` on the paired draws of ``intervention_moments``, for V hypothesised inputs shared by all trajectories at once.
        ``hypotheses`` = {label name: [V, width]} as ``label_evidence`` takes them (``label_grid`` builds the Cartesian product), every
        name a conditional-prior label of the family; every prior group with a named label is redrawn from p(z_g | u'_g) on the subject's
        own noise, a label that is not named keeps each trajectory's own value.  Returns ``{"hypotheses": tables, curve: {"factual":
        {name: (mean, sd) [B, C]}, "cf": {name: (mean, sd) [V, B, C]}, "effect": {name: (mean, sd) [V, B, C]}}}`` per head curve
        (``mu_50``, ``mu_75``, ``mu_25``; ``mean`` for the Gaussian family) over the eight names of ``SUMMARY_NAMES``: mean and population sd
        over ``num_samples`` draws of the functional on the subject's own curve, on its curve under hypothesis v, and of the PAIRED
        difference (both arms of a draw share their noise).  ``"t_hit"`` of an arm runs over its crossing draws, of an effect over the draws
        that cross in both arms (NaN where none does); the effect on ``"crossed"`` is the change of P(cross), and its sd^2 + mean^2 is the
        share of draws whose crossing changes.  ``thresholds`` / ``sense``: as ``curve_summary`` (None: the three threshold entries are
        NaN).  ONE engine call (``slode_intervene_summary``) where the V arms fit the LDS, else the fewest calls that do, all on the same
        noise -- column v does not depend on the others, so the split changes no bit; no ``[B, C, T, num_samples]`` tensor exists and
        the encoder and the factual arm run once per call, not once per hypothesis.  ``eps`` ``[num_samples, B, L]`` makes it reproducible;
        None draws one call of the engine's generator.  Where the engine refuses (adaptive solver, strided observations, measured arms)
        the same dict is composed from ``counterfactual_samples`` per hypothesis in chunks over B, the functionals and the paired rules
        in torch on the same definitions."""
        from .. import _lib as L
        b = self._bind()
        B, ns, sn = observations.shape[0], self._count(num_samples), self._summary_sense(sense)
        V, tabs, mask = self._summary_hypotheses(hypotheses)
        thr = None if thresholds is None else [float(x) for x in torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1).tolist()]
        if thr is not None and len(thr) != observations.shape[1]:
            raise ValueError("thresholds must hold %d values (one per channel), got %d" % (observations.shape[1], len(thr)))
        names = self.MOMENT_HEADS[bool(self.GAUSS)]
        dev = observations.device

        def pack(f, cf, eff):      # each (mean, sd): f [Q, B, C, 8], cf / eff [V, Q, B, C, 8]
            res = {"hypotheses": tabs}
            for q, n in enumerate(names):
                res[n] = {"factual": {k: (f[0][q][..., j], f[1][q][..., j]) for j, k in enumerate(self.SUMMARY_NAMES)},
                          "cf": {k: (cf[0][:, q][..., j], cf[1][:, q][..., j]) for j, k in enumerate(self.SUMMARY_NAMES)},
                          "effect": {k: (eff[0][:, q][..., j], eff[1][:, q][..., j]) for j, k in enumerate(self.SUMMARY_NAMES)}}
            return res

        def fused():
            eng = b.engine
            cap = min(L.INTERVENE_SUMMARY_MAX_ARMS, self.INTERVENTION_SUMMARY_ARMS_PER_CALL or L.INTERVENE_SUMMARY_MAX_ARMS)
            slices = self._fewest_calls(V, cap, lambda n: eng.intervene_summary_plan(B, n))
            bt = self._draws_batch(observations, labels, eps, ns)

            def call(lo, hi):
                hyp = [tabs[l][lo:hi].contiguous().to(dev) if l in tabs else None for l in self.LABELS]
                first = None if lo == 0 else False            # the factual moments are the same in every call: asked for once
                return eng.intervene_summary(b.flat, bt, B, hyp, hi - lo, mask, ns, thr, sn, f_mean=first, f_sd=first)
            got = self._on_the_same_noise(eng, eps, slices, call)
            cat = lambda i: got[0][i] if len(got) == 1 else torch.cat([g[i] for g in got], 0)      # noqa: E731
            return pack((got[0][0], got[0][1]), (cat(2), cat(3)), (cat(4), cat(5)))

        def composed():
            cols = {n: [] for n in names}      # per chunk: (f mean, f sd [rows, C, 8], cf mean, cf sd, eff mean, eff sd [V, rows, C, 8])
            for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
                part = {n: [None, None, [], [], [], []] for n in names}
                for v in range(V):
                    swap = {l: t[v:v + 1].to(dev).expand(hi - lo, -1).contiguous() for l, t in tabs.items()}
                    res = self.counterfactual_samples(num_samples=ns, intervene=swap, eps=e, **d)
                    for n in names:
                        ff, _ = self._summary_functionals(res[n][0], thr, sn)
                        fv, _ = self._summary_functionals(res[n][1], thr, sn)
                        if v == 0:
                            part[n][0], part[n][1] = self._summary_moments(ff)
                        for i, t in zip((2, 3, 4, 5), self._summary_moments(fv) + self._summary_moments(fv - ff)):      # (NaN - x = NaN: slot 6 of
                            part[n][i].append(t)                                                                       # an effect keeps the draws that cross in both arms)
                    del res
                for n in names:
                    cols[n].append(part[n][:2] + [torch.stack(p, 0) for p in part[n][2:]])
            st = lambda i, dim: torch.stack([torch.cat([c[i] for c in cols[n]], dim) for n in names], 0 if dim == 0 else 1)      # noqa: E731
            return pack((st(0, 0), st(1, 0)), (st(2, 1), st(3, 1)), (st(4, 1), st(5, 1)))
        return self._fused_or_composed(fused, composed)

    def save_intervention_summary(self, results_dir: str, batches, num_samples: int, hypotheses, thresholds=None, sense="above"):
        """Runs ``intervention_summary`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors) and writes
        ``summary_<curve>_factual_mean.npy`` / ``..._sd.npy``, float32 ``[n, C, 8]``, ``summary_<curve>_cf_{mean,sd}.npy`` and
        ``summary_<curve>_effect_{mean,sd}.npy``, float32 ``[n, V, C, 8]`` (the trajectories in loader order, the slots in ``SUMMARY_NAMES``
        order), and ``summary_hypotheses_<label>.npy`` (``[V, width]``) per hypothesised label.  One read-back, at the end.  Returns the
        paths."""
        V, tabs, _ = self._summary_hypotheses(hypotheses)
        names = self.MOMENT_HEADS[bool(self.GAUSS)]

        def rows(r):
            for n in names:
                for arm in self.SUMMARY_ARMS:
                    for k in (0, 1):
                        t = torch.stack([r[n][arm][slot][k] for slot in self.SUMMARY_NAMES], -1)
                        yield "summary_%s_%s_%s.npy" % (n, arm, ("mean", "sd")[k]), t if arm == "factual" else t.transpose(0, 1)
        written = self._save_over_batches(
            results_dir, batches, lambda **d: self.intervention_summary(num_samples=num_samples, hypotheses=tabs, thresholds=thresholds, sense=sense, **d), rows)
        return written + self._save_arrays(results_dir, [("summary_hypotheses_%s.npy" % l, tabs[l]) for l in self.LABELS if l in tabs])

    def intervention_summary_lines(self, effect_mean, tables, with_threshold: bool):
        """One printed line per hypothesis of a ``save_intervention_summary`` pass from the central curve's ``effect_mean`` array
        ``[n, V, C, 8]`` and the hypothesis tables ``{label: [V, width]}``: per channel, the mean over trajectories of the paired effect on
        the peak and on the AUC and, with thresholds, of ``P_cf - P_f``."""
        import numpy as np
        m = np.asarray(effect_mean, dtype=np.float64)
        lines = []
        for v in range(m.shape[1]):
            tag = " ".join("%s=%s" % (l, np.asarray(t)[v].reshape(-1).tolist()) for l, t in tables.items())
            cells = []
            for c in range(m.shape[2]):
                cell = "c%d d_peak=%.4g d_auc=%.4g" % (c, m[:, v, c, 0].mean(), m[:, v, c, 4].mean())
                if with_threshold:
                    cell += " d_p_cross=%.3f" % m[:, v, c, 7].mean()
                cells.append(cell)
            lines.append("intervention_summary: %s  n=%d  %s" % (tag, m.shape[0], "  ".join(cells)))
        return lines

    # ---- sample quantiles: the credible band, the envelope, the median of every curve value over the draws ------------------------------
    QUANTILE_MAX_LEVELS = 8     # SLODE_QUANTILE_MAX_LEVELS

    @staticmethod
    def _quantile_ranks(levels, K: int):
        """``[(lo, hi, g)]`` per level for ``K`` sorted draws, numpy's default "linear" definition as ``slode_recon_quantiles`` forms it on the
        host in fp64: h = q (K - 1), lo = floor(h), hi = min(lo + 1, K - 1), g = float32(h - lo) (returned as the Python float of that fp32)."""
        import math
        import struct
        res = []
        for q in levels:
            h = float(q) * (K - 1)
            lo = min(max(int(math.floor(h)), 0), K - 1)
            res.append((lo, min(lo + 1, K - 1), struct.unpack("f", struct.pack("f", h - lo))[0]))
        return res

    def _sample_quantiles(self, v, levels):
        """The quantiles at ``levels`` over the draw axis of the curves ``v`` ``[rows, C, T, ns]``: ``[Lv, rows, C, T]`` float32 -- a sort
        along the draws and ``fma(g, v[hi] - v[lo], v[lo])`` on the ranks of ``_quantile_ranks`` (the difference rounded to fp32, the
        multiply-add formed in fp64 and rounded once), the rule of ``slode_recon_quantiles``.  Not ``torch.quantile``: its interpolation is
        not pinned and it limits the input size."""
        s = torch.sort(v.to(torch.float32), dim=-1).values
        out = []
        for lo, hi, g in self._quantile_ranks(levels, s.shape[-1]):
            v_lo, v_hi = s[..., lo], s[..., hi]
            out.append((g * (v_hi - v_lo).to(torch.float64) + v_lo.to(torch.float64)).to(torch.float32))
        return torch.stack(out, 0)

    def recon_quantiles(self, observations, is_post, num_samples: int, levels=(0.025, 0.975), eps=None, tile: int = 0, max_sweeps: int = 2,
                        **labels):
        """What users of ``multiple_samples`` take first -- ``np.percentile(samples, [2.5, 97.5], axis=-1)``, the credible band around a
        curve, the envelope, the median -- without the samples: ``{"levels": [Lv] (float64), "mu_50": [Lv, B, C, T], "mu_75": ..., "mu_25":
        ...}`` (``"mean"`` for the Gaussian family), the sample quantiles (numpy's default "linear" definition) at ``levels`` (1 to 8 values
        in [0, 1], any order) of every head curve value over ``num_samples`` latent draws.  ONE engine call (``slode_recon_quantiles``) on
        the draws of ``recon_moments`` that keeps only the ranks it needs, sorted, on chip: no ``[B, C, T, num_samples]`` tensor exists.
        A level whose rank is an integer (0: the minimum, 1: the maximum) is one of the draw values exactly.  ``eps`` ``[num_samples, B,
        L]`` makes it reproducible; None: rows k * B + b of one drawing call of the engine's generator, the draw ``recon_samples`` makes,
        and the counter moves by ``num_samples``.  ``tile``: time points per sweep over the draws (0: the engine's choice,
        ``Engine.quantile_plan``).  The composed route -- ``recon_samples`` over chunks of trajectories, ``torch.sort`` along the draws, the
        same rank rule -- is taken where the engine refuses (adaptive solver, strided observations, measured arms, LDS budget) or where
        the plan needs more than ``max_sweeps`` sweeps (central levels at many draws keep every draw per value: from three sweeps on the
        sort was measured faster)."""
        b = self._bind()
        B, ns = observations.shape[0], self._count(num_samples)
        lv = self._levels_list(levels, self.QUANTILE_MAX_LEVELS, open_at_zero=False)
        T = int(self.times.numel())
        if not 0 <= int(tile) <= T:
            raise ValueError("tile must lie in [0, T = %d], got %d" % (T, int(tile)))
        names = self.MOMENT_HEADS[bool(self.GAUSS)]

        def pack(out):
            return dict({"levels": torch.tensor(lv, dtype=torch.float64)}, **{n: out[q] for q, n in enumerate(names)})

        def fused():
            return pack(b.engine.recon_quantiles(b.flat, self._draws_batch(observations, labels, eps, ns), B, is_post, ns, lv, None, int(tile))
                        .unbind(1))

        def composed():
            parts = {n: [] for n in names}
            with self._counter_moves_by(ns, eps):
                for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
                    res = self.recon_samples(is_post=is_post, num_samples=ns, eps=e, **d)
                    for n in names:
                        parts[n].append(self._sample_quantiles(res[n], lv))
                    del res
            return pack([torch.cat(parts[n], 1) for n in names])

        def planned():
            if b.engine.quantile_plan(B, ns, lv, int(tile))[1] > int(max_sweeps):
                return composed()
            return fused()
        return self._fused_or_composed(planned, composed)

    def save_recon_quantiles(self, results_dir: str, batches, is_post, num_samples: int, levels=(0.025, 0.975)):
        """Runs ``recon_quantiles`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors) and writes
        ``<curve>_<post|prior>_sample_quantiles.npy``, float32 ``[n, Lv, C, T]`` (the trajectories in loader order), for every head curve and
        ``sample_quantile_levels.npy``, the levels.  One read-back, at the end.  Returns the paths."""
        names = self.MOMENT_HEADS[bool(self.GAUSS)]
        tag = "post" if is_post else "prior"
        return self._save_over_batches(
            results_dir, batches, lambda **d: self.recon_quantiles(is_post=is_post, num_samples=num_samples, levels=levels, **d),
            lambda r: (("%s_%s_sample_quantiles.npy" % (n, tag), r[n].transpose(0, 1)) for n in names),
            side=("sample_quantile_levels.npy", self._save_levels))

    @staticmethod
    def quantile_line(quantiles, levels, observations, tag):
        """One printed line of a ``save_recon_quantiles`` pass from the central curve's array ``[n, Lv, C, T]``, its levels and the
        observations ``[n, C, T]``: the mean width of the band between the lowest and the highest level, and the share of observation
        points inside it (bounds included)."""
        import numpy as np
        qv, lv, y = np.asarray(quantiles, dtype=np.float64), np.asarray(levels, dtype=np.float64), np.asarray(observations, dtype=np.float64)
        lo, hi = qv[:, int(lv.argmin())], qv[:, int(lv.argmax())]
        return "sample_quantiles_%s: n=%d  levels=[%g, %g]  mean_width=%.4g  inside=%.3f" % (
            tag, qv.shape[0], lv.min(), lv.max(), (hi - lo).mean(), ((y >= lo) & (y <= hi)).mean())

    # ---- mechanism curves: what the dynamics dx/dt = a - d x say at every grid point, over the draws --------------------------------------
    MECHANISM_NAMES = ("state", "production", "degradation", "set_point", "net_rate")   # the slots of slode_mechanism_moments, bit i each
    MECHANISM_SLOTS_PER_CALL = None      # most slots of one engine call; None: what the engine's plan says fits the LDS (at most 5)

    def mechanism_moments(self, observations, is_post, num_samples: int, quantities=None, eps=None, **labels):
        """Why the curves look as they do, in the model's own terms: the dynamics are dx/dt = a(t, z) - d(t, z) x, so a / d is the moving
        set point each state relaxes towards, 1 / d its local time constant and a - d x the net rate.  Returns ``{"quantities": names,
        name: (mean, sd), ...}``, mean and population sd over ``num_samples`` latent draws from the posterior q(z | x) (``is_post``) or the
        conditional prior, ``[B, T, S]`` each (the layout of ``solution_xt``), for ``"state"`` (x at the grid points), ``"production"`` (a
        at the grid times), ``"degradation"`` (d), ``"set_point"`` (a / d) and ``"net_rate"`` (a - d x); ``quantities`` names the ones
        wanted (default: all five; an unknown name raises ``ValueError``).  ONE engine call (``slode_mechanism_moments``) on the draws of
        ``recon_moments`` (same ``eps`` ``[num_samples, B, L]``, or one drawing call: the counter ends at n + 1) where the tables fit the
        LDS, else the fewest calls that do, all on the same noise: no ``[num_samples, B, T, S]`` tensor exists, and the split changes no
        bit.  Where the engine refuses (adaptive solver, strided observations, measured arms) the same dict is composed in chunks over B
        from ``decoder.ode_model.solve_ODE`` and the torch modules ``dynamics.prod`` / ``dynamics.degr`` on ``cat([t_i, z])``."""
        from .. import _lib as L
        b = self._bind()
        B, ns = observations.shape[0], self._count(num_samples)
        wanted = tuple(self.MECHANISM_NAMES if quantities is None else quantities)
        unknown = [q for q in wanted if q not in self.MECHANISM_NAMES]
        if unknown or not wanted:
            raise ValueError("quantities must name some of %r, got %r" % (self.MECHANISM_NAMES, quantities))
        sel = sorted({self.MECHANISM_NAMES.index(q) for q in wanted})      # the engine stores the selected slots in increasing slot order

        def pack(mean, sd):      # mean, sd: indexable by position in sel, [rows, T, S] each
            at = {i: j for j, i in enumerate(sel)}
            return dict({"quantities": wanted}, **{q: (mean[at[self.MECHANISM_NAMES.index(q)]], sd[at[self.MECHANISM_NAMES.index(q)]]) for q in wanted})

        def fused():
            eng = b.engine
            slices = self._fewest_calls(len(sel), self.MECHANISM_SLOTS_PER_CALL or L.MECHANISM_SLOTS,
                                        lambda n: eng.mechanism_plan(B, (1 << n) - 1))      # the LDS figure depends on the slot count alone
            bt = self._draws_batch(observations, labels, eps, ns)
            got = self._on_the_same_noise(eng, eps, slices, lambda lo, hi: eng.mechanism_moments(      # (drawing call n0 every time)
                b.flat, bt, B, is_post, ns, sum(1 << q for q in sel[lo:hi])))
            return pack([m.permute(0, 2, 1) for g in got for m in g[0].unbind(0)], [s.permute(0, 2, 1) for g in got for s in g[1].unbind(0)])

        def composed():
            with torch.no_grad():
                dyn = self.decoder.ode_model.dynamics
                t = torch.as_tensor(self.times, dtype=torch.float32).reshape(-1)
                cols = [([], []) for _ in sel]
                for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
                    obs = d.pop("observations")
                    loc, scale = self._loc_scale(obs, is_post, d)
                    z = (loc.unsqueeze(0) + scale.unsqueeze(0) * e.to(loc.device)).reshape(ns * (hi - lo), -1).to(torch.float32).contiguous()
                    x = self.decoder.ode_model.solve_ODE(z).to(torch.float32)                                          # [ns * rows, T, S]
                    tz = torch.cat([t.to(z.device).reshape(1, -1, 1).expand(z.shape[0], -1, 1), z.unsqueeze(1).expand(-1, t.numel(), -1)], dim=2)
                    a, dg = dyn.prod(tz).to(torch.float32), dyn.degr(tz).to(torch.float32)                              # [ns * rows, T, S]
                    vals = (lambda: x, lambda: a, lambda: dg, lambda: a / dg, lambda: a - dg * x)
                    for j, q in enumerate(sel):
                        v = vals[q]()
                        m, s = self._mean_sd(v.reshape(ns, hi - lo, v.shape[1], v.shape[2]).permute(1, 2, 3, 0).contiguous())      # (contiguous draws: the sum's order does not depend on the chunk)
                        cols[j][0].append(m); cols[j][1].append(s)
                    del x, a, dg, tz
                return pack([torch.cat(c[0], 0) for c in cols], [torch.cat(c[1], 0) for c in cols])
        return self._fused_or_composed(fused, composed)

    def save_mechanism_moments(self, results_dir: str, batches, is_post, num_samples: int):
        """Runs ``mechanism_moments`` (all five quantities) over ``batches`` (an iterable of device batch dicts: ``observations`` + the label
        tensors) and writes ``mechanism_<name>_<post|prior>_mean.npy`` / ``..._sd.npy``, float32 ``[n, T, S]`` (the trajectories in loader
        order).  One read-back, at the end.  Returns the paths."""
        tag = "post" if is_post else "prior"
        return self._save_over_batches(
            results_dir, batches, lambda **d: self.mechanism_moments(is_post=is_post, num_samples=num_samples, **d),
            lambda r: (("mechanism_%s_%s_%s.npy" % (n, tag, ("mean", "sd")[k]), r[n][k]) for n in self.MECHANISM_NAMES for k in (0, 1)))

    @staticmethod
    def mechanism_line(res, tag):
        """One printed line of a ``save_mechanism_moments`` pass from ``res`` = ``{name: mean array [n, T, S]}`` (``"production"``,
        ``"degradation"``, ``"set_point"``): per state component, the mean over trajectories and time of the mean production, degradation
        and set point."""
        import numpy as np
        a, d, sp = (np.asarray(res[k], dtype=np.float64) for k in ("production", "degradation", "set_point"))
        cells = ["x%d a=%.4g d=%.4g a/d=%.4g" % (s, a[..., s].mean(), d[..., s].mean(), sp[..., s].mean()) for s in range(a.shape[-1])]
        return "mechanism_%s: n=%d  %s" % (tag, a.shape[0], "  ".join(cells))

    # ---- simultaneous (sup-t) credible bands: one critical value per curve, from the draws' largest standardised deviation ----------------
    BAND_MAX_LEVELS = 8     # SLODE_JOINT_BAND_MAX_LEVELS

    @staticmethod
    def _band_levels(levels, K: int):
        """``[(r, z)]`` per level for ``K`` draws, as ``slode_joint_band`` forms them on the host in fp64: the rank r = min(K, max(1,
        ceil(level K - 1e-9))), counted from 1, and the pointwise half-width z = Phi^-1((1 + level) / 2) (inf at level 1)."""
        import math
        from statistics import NormalDist
        return [(min(K, max(1, int(math.ceil(float(p) * K - 1e-9)))), math.inf if float(p) >= 1.0 else NormalDist().inv_cdf((1.0 + float(p)) / 2.0))
                for p in levels]

    def simultaneous_band(self, observations, is_post, num_samples: int, levels=(0.95,), sd_floor: float = 0.0, eps=None,
                          return_draws: bool = False, **labels):
        """The band that may be read as a statement about the WHOLE curve.  A band drawn from per-point intervals (``mean +- 1.96 sd`` of
        ``recon_moments``, the quantiles of ``recon_quantiles``) holds each point with 95 % probability and the entire curve with less --
        how much less depends on how correlated the curve is along time.  The simultaneous (sup-t) band is ``mean +- crit sd`` with ONE
        number per curve: the level-quantile over the ``num_samples`` = K draws of dev_k = max_t |v_k(t) - mean(t)| / sd(t).  Returns
        ``{"levels": [Lv] (float64), "mu_50": {...}, "mu_75": ..., "mu_25": ...}`` (``"mean"`` for the Gaussian family), per head curve a
        dict with ``"mean"``, ``"sd"`` ``[B, C, T]`` (the tensors of ``recon_moments`` on the same noise), ``"crit"`` ``[Lv, B, C]`` (the
        r-th smallest deviation, r = ceil(level K): one of the deviations exactly), ``"lower"`` / ``"upper"`` ``[Lv, B, C, T]`` (``mean -+
        crit sd``), ``"pointwise_joint"`` ``[Lv, B, C]`` (the share of draws wholly inside the POINTWISE band ``mean +- z sd``, z =
        Phi^-1((1 + level) / 2): what the naive band really holds), ``"obs_dev"`` ``[B, C]`` (the deviation of the observed curve),
        ``"obs_inside"`` ``[Lv, B, C]`` (bool: ``obs_dev <= crit``, the observation leaves the band nowhere), ``"points"`` ``[B, C]`` (the
        time points with ``sd > sd_floor``; the others take no part) and, with ``return_draws``, ``"dev"`` ``[K, B, C]``.  1 to 8 levels in
        (0, 1], any order.  The deviation of a draw from its own sample mean is bounded by sqrt(K - 1) sample sds whatever the model:
        below about K = 20 a 95 % critical value is a property of K, not of the model.  ONE engine call (``slode_joint_band``) that walks
        the draws of ``recon_moments`` twice on the same noise: no ``[B, C, T, K]`` tensor exists.  ``eps`` ``[K, B, L]`` makes it
        reproducible; None: one drawing call of the engine's generator, as ``recon_moments``.  Where the engine refuses (adaptive solver,
        strided observations, measured arms, LDS budget) the same dict is composed from ``recon_samples`` in chunks over B: torch mean /
        population std, the same division, ``amax`` over T, ``torch.sort`` over the draws, the same rank rule."""
        import math
        b = self._bind()
        B, ns = observations.shape[0], self._count(num_samples)
        if ns < 2:
            raise ValueError("num_samples must be >= 2 (the sd of one draw is 0), got %d" % ns)
        lv = self._levels_list(levels, self.BAND_MAX_LEVELS, open_at_zero=True)
        floor = float(sd_floor)
        if not (floor >= 0.0 and math.isfinite(floor)):
            raise ValueError("sd_floor must be finite and >= 0, got %r" % (sd_floor,))
        names = self.MOMENT_HEADS[bool(self.GAUSS)]

        def pack(per_curve):      # per_curve[q] = (mean, sd [rows, C, T], crit, joint [rows, C, Lv], obs_dev, points [rows, C], dev [rows, C, K])
            out = {"levels": torch.tensor(lv, dtype=torch.float64)}
            for n, (mean, sd, crit, joint, odev, points, dev) in zip(names, per_curve):
                crit, joint = crit.permute(2, 0, 1), joint.permute(2, 0, 1)
                half = crit.unsqueeze(-1) * sd.unsqueeze(0)
                out[n] = {"mean": mean, "sd": sd, "crit": crit, "lower": mean.unsqueeze(0) - half, "upper": mean.unsqueeze(0) + half,
                          "pointwise_joint": joint, "obs_dev": odev, "obs_inside": odev.unsqueeze(0) <= crit, "points": points}
                if return_draws:
                    out[n]["dev"] = dev.permute(2, 0, 1)
            return out

        def fused():
            mean, sd, crit, joint, odev, dev = b.engine.joint_band(b.flat, self._draws_batch(observations, labels, eps, ns), B, is_post, ns, lv,
                                                                   floor, dev=True if return_draws else None)
            return pack([(mean[q], sd[q], crit[q], joint[q], odev[q, ..., 0], odev[q, ..., 1], None if dev is None else dev[q])
                         for q in range(len(names))])

        def composed():
            rz = self._band_levels(lv, ns)
            cols = {n: [] for n in names}
            with self._counter_moves_by(1, eps):
                for lo, hi, e, d in self._chunks(observations, labels, ns, eps):
                    res = self.recon_samples(is_post=is_post, num_samples=ns, eps=e, **d)
                    y = d["observations"].to(torch.float32)
                    for n in names:
                        v = res[n].to(torch.float32)                                                       # [rows, C, T, ns]
                        mean, sd = self._mean_sd(v)
                        on = sd > floor
                        neg = torch.full_like(sd, -1.0)
                        e_k = torch.where(on.unsqueeze(-1), (v - mean.unsqueeze(-1)).abs() / sd.unsqueeze(-1), neg.unsqueeze(-1))
                        dev = e_k.amax(dim=2).clamp_min(0.0)                                                # [rows, C, ns]
                        odev = torch.where(on, (y.to(mean.device) - mean).abs() / sd, neg).amax(dim=2).clamp_min(0.0)
                        srt = torch.sort(dev, dim=-1).values
                        crit = torch.stack([srt[..., r - 1] for r, _ in rz], -1)
                        joint = torch.stack([(dev <= torch.tensor(z, dtype=torch.float32)).sum(-1).to(torch.float32) / float(ns) for _, z in rz], -1)
                        cols[n].append((mean, sd, crit, joint, odev, on.sum(dim=2).to(torch.float32), dev))
                    del res
            return pack([tuple(torch.cat(c, 0) for c in zip(*cols[n])) for n in names])
        return self._fused_or_composed(fused, composed)

    BAND_FILES = ("mean", "sd", "crit", "pointwise_joint", "obs_dev")

    def save_simultaneous_band(self, results_dir: str, batches, is_post, num_samples: int, levels=(0.95,)):
        """Runs ``simultaneous_band`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors) and writes,
        for every head curve, ``<curve>_<post|prior>_band_{mean,sd}.npy`` ``[n, C, T]``, ``..._band_{crit,pointwise_joint}.npy``
        ``[n, Lv, C]`` and ``..._band_obs_dev.npy`` ``[n, C]`` (the trajectories in loader order), and ``band_levels.npy``.  One
        read-back, at the end.  Returns the paths."""
        names = self.MOMENT_HEADS[bool(self.GAUSS)]
        tag = "post" if is_post else "prior"
        return self._save_over_batches(
            results_dir, batches, lambda **d: self.simultaneous_band(is_post=is_post, num_samples=num_samples, levels=levels, **d),
            lambda r: (("%s_%s_band_%s.npy" % (n, tag, k), r[n][k].transpose(0, 1) if k in ("crit", "pointwise_joint") else r[n][k])
                       for n in names for k in self.BAND_FILES), side=("band_levels.npy", self._save_levels))

    @classmethod
    def band_line(cls, crit, joint, obs_dev, levels, tag):
        """One printed line of a ``save_simultaneous_band`` pass from the central curve's arrays ``crit``, ``joint`` ``[n, Lv, C]`` and
        ``obs_dev`` ``[n, C]`` and the levels: per level, the mean critical value beside the pointwise z, the mean share of draws wholly
        inside the pointwise band, and the share of subject-channels whose observation lies wholly inside the simultaneous band."""
        import numpy as np
        cv, jv, ov = (np.asarray(a, dtype=np.float64) for a in (crit, joint, obs_dev))
        lv = [float(x) for x in np.asarray(levels, dtype=np.float64).reshape(-1)]
        cells = ["%g: crit=%.3f (z=%.3f) pointwise_joint=%.3f obs_inside=%.3f" % (p, cv[:, j].mean(), z, jv[:, j].mean(), (ov <= cv[:, j]).mean())
                 for j, (p, (_, z)) in enumerate(zip(lv, cls._band_levels(lv, 2)))]
        return "joint_band_%s: n=%d  levels=%s  %s" % (tag, cv.shape[0], "[" + ", ".join("%g" % p for p in lv) + "]", "  ".join(cells))

    # ---- per-trajectory bounds from K posterior draws: nothing summed over the batch -----------------------------------------------------
    BOUND_NAMES =("elbo", "iw_bound", "ess", "nll")     # the slots of one slode_traj_bounds row, in order

    def trajectory_bounds(self, observations, num_draws: int, eps=None, return_draws: bool = False, **labels):
        """Per trajectory, from ``num_draws`` = K posterior draws z_k = loc(x) + scale(x) eps_k: ``{"elbo": [B], "iw_bound": [B], "ess": [B],
        "nll": [B]}`` -- the -ELBO of the trajectory (mean over k of the main loss of that single row: the summand of
        ``Trace_ELBO(num_particles=K).evaluate_loss``), the importance-weighted bound -log(1/K sum_k exp(-loss_k)) (<= elbo; a tighter
        estimate of -log p(x | labels), comparable between the ALD and Gauss variants), the effective sample size of the importance weights
        (in [1, K]) and the mean negative log-likelihood term -- plus ``"loss": [K, B]``, the per-draw losses, with ``return_draws``.  ONE
        engine call (``slode_traj_bounds``): the encoder runs once per trajectory, the K solves of a trajectory in one workgroup.  ``eps``
        ``[K, B, L]`` makes it reproducible; None takes drawing calls n .. n + K - 1 of the engine's generator (draw k of trajectory b: row b
        of call n + k, as a K-particle ELBO step draws).  What the engine refuses (adaptive solver, strided observations, measured arms,
        LDS budget) raises its SlodeError: no other call yields a per-trajectory loss to compose from."""
        b = self._bind()
        B, K = observations.shape[0], self._count(num_draws, "num_draws")
        bounds, loss = b.engine.traj_bounds(b.flat, self._draws_batch(observations, labels, eps, K), B, K)
        res = {n: bounds[:, i] for i, n in enumerate(self.BOUND_NAMES)}
        if return_draws:
            res["loss"] = loss
        return res

    def save_trajectory_bounds(self, results_dir: str, batches, num_draws: int):
        """Runs ``trajectory_bounds`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors) and writes the table
        ``bounds_post.npy``, float32 ``[n, 4]`` with the columns of ``BOUND_NAMES`` and the trajectories in loader order, beside the
        reference's result files.  One read-back, at the end.  Returns the path."""
        import os
        import numpy as np
        rows = []
        for d in batches:
            r = self.trajectory_bounds(num_draws=num_draws, **d)
            rows.append(torch.stack([r[n] for n in self.BOUND_NAMES], dim=1))
        table = torch.cat(rows, 0).cpu().numpy().astype(np.float32) if rows else np.zeros((0, len(self.BOUND_NAMES)), np.float32)
        os.makedirs(results_dir, exist_ok=True)
        path = os.path.join(results_dir, "bounds_post.npy")
        np.save(path, table)
        return path

    # ---- posterior refinement: per-trajectory ELBO ascent on (loc, log scale), the encoder's posterior as the start ------------------------
    def _given_posterior(self, observations, posterior):
        """``posterior`` = (loc, scale) as float32 ``[B, L]`` tensors on the observations' device."""
        loc, scale = posterior
        B = observations.shape[0]
        loc, scale = (torch.as_tensor(t, dtype=torch.float32, device=observations.device).reshape(B, -1).contiguous() for t in (loc, scale))
        if loc.shape != scale.shape or loc.shape[1] != self._bind().engine.spec.latent_dim:
            raise ValueError("posterior must be (loc, scale), each [%d, %d], got %s and %s"
                             % (B, self._bind().engine.spec.latent_dim, tuple(loc.shape), tuple(scale.shape)))
        return loc, scale

    def refine_posterior(self, observations, num_draws: int, num_steps: int, lr: float = 0.05, mask=None, eps=None, return_trace: bool = False,
                         **labels):
        """Closes the amortisation gap subject by subject: every trajectory takes ``num_steps`` Adam steps (``lr``) on its own (loc, log
        scale), starting from the encoder's, against its own -ELBO over ``num_draws`` = K noise rows that stay fixed for the whole call --
        ``{"loc": [B, L], "scale": [B, L], "elbo0": [B], "elbo": [B], "best_step": [B]}``: the best iterate, the -ELBO at the encoder's
        posterior and at the best iterate (``elbo <= elbo0`` by construction), the step the best iterate was found at -- plus, with
        ``return_trace``, ``"grad0": [B, 2 L]`` (the gradient at the encoder's posterior with respect to (loc, log scale)) and ``"trace":
        [num_steps + 1, B]`` (the -ELBO of every iterate).  ``mask`` ``[B, C, T]`` (weights >= 0, or bool): the likelihood term of (c, t)
        counts that much -- a prefix of the window (``mask[:, :, t0:] = 0``), a dropped channel -- while the encoder, which gives the
        start, still reads the whole block; None: every weight 1.  ONE engine call (``slode_posterior_refine``): forward solve, backward pass
        and optimiser of a trajectory run in one workgroup.  ``eps`` ``[K, B, L]`` makes it reproducible; None takes drawing calls n .. n + K
        - 1 of the engine's generator, as ``trajectory_bounds`` does.  What the engine refuses (adaptive solver, strided observations,
        measured arms, the proc family -- its main loss scores the labels, LDS budget) raises its SlodeError: there is no composed route.
        Decode or forecast the result with ``recon_samples(posterior=(loc, scale))`` / ``forecast_samples(posterior=...)``."""
        b = self._bind()
        B, K = observations.shape[0], self._count(num_draws, "num_draws")
        if mask is not None:    # the engine takes the weights in the observations' own layout
            mask = self._obs_layout(observations, mask)
        loc, scale, elbo, grad0, trace, best = b.engine.posterior_refine(
            b.flat, self._draws_batch(observations, labels, eps, K), B, K, int(num_steps), lr, mask=mask,
            grad0=None if return_trace else False, trace=None if return_trace else False)
        res = {"loc": loc, "scale": scale, "elbo0": elbo[:, 0], "elbo": elbo[:, 1], "best_step": best}
        if return_trace:
            res["grad0"], res["trace"] = grad0, trace
        return res

    def save_refined_posterior(self, results_dir: str, batches, num_draws: int, num_steps: int, lr: float = 0.05):
        """Runs ``refine_posterior`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors, optionally
        ``mask``) and writes ``refined_loc.npy`` / ``refined_scale.npy`` (float32 ``[n, L]``) and ``refined_elbo.npy`` (float32 ``[n, 2]``:
        the -ELBO before and after), the trajectories in loader order, beside the reference's result files.  One read-back, at the end.
        Returns the three paths."""
        parts = {"refined_loc.npy": [], "refined_scale.npy": [], "refined_elbo.npy": []}
        for d in batches:
            r = self.refine_posterior(num_draws=num_draws, num_steps=num_steps, lr=lr, **d)
            parts["refined_loc.npy"].append(r["loc"])
            parts["refined_scale.npy"].append(r["scale"])
            parts["refined_elbo.npy"].append(torch.stack([r["elbo0"], r["elbo"]], dim=1))
        if not parts["refined_loc.npy"]:
            raise ValueError("save_refined_posterior: no batches")
        return self._save_arrays(results_dir, [(f, torch.cat(v, 0)) for f, v in parts.items()])

    # ---- pointwise predictive density: per-point lppd and the WAIC terms from K posterior draws ----------------------------------------------
    POINTWISE_NAMES = ("lppd_in", "p_waic_in", "mean_ll_in", "n_in", "lppd_out", "mean_ll_out", "n_out", "ess")   # one summary row, in order
    POINTWISE_WEIGHTS = {"posterior": 0, "importance": 1}

    def _obs_layout(self, observations, mask):
        """``mask`` (weights >= 0 or bool, broadcastable to the observations) as a float32 tensor with the observations' shape AND strides."""
        m = torch.as_tensor(mask, device=observations.device).to(torch.float32).expand(observations.shape)
        out = torch.empty_strided(observations.shape, observations.stride(), dtype=torch.float32, device=observations.device)
        out.copy_(m)
        return out

    def pointwise_density(self, observations, num_draws: int, weights: str = "posterior", mask=None, posterior=None, eps=None,
                          return_draws: bool = False, **labels):
        """Where does the model fail, and which of two models predicts better?  Per observation point (c, t), over ``num_draws`` = K
        posterior draws with normalised weights w_k: ``"lppd"`` = log sum_k w_k p(y | z_k), ``"mean_ll"`` = sum_k w_k log p(y | z_k),
        ``"p_waic"`` = the weighted variance of log p(y | z_k) and ``"elpd_waic"`` = lppd - p_waic, ``[B, C, T]`` each; per trajectory
        (``[B]`` each) ``"lppd_in"``, ``"p_waic_in"``, ``"mean_ll_in"``, ``"n_in"`` over the points the mask counts as observed (> 0),
        ``"lppd_out"``, ``"mean_ll_out"``, ``"n_out"`` over the others, and ``"ess"``, the effective sample size of the weights; with
        ``return_draws`` (importance weights) ``"loss"`` ``[K, B]``, the per-draw losses.  ``weights``: ``"posterior"`` (w_k = 1 / K, the
        draws of q(z | x) as they come) or ``"importance"`` (w_k ~ exp(-loss_k), self-normalised; loss_k the per-draw loss of
        ``trajectory_bounds`` with the mask on its likelihood terms).  ``mask`` ``[B, C, T]`` (weights >= 0, or bool; None: every point
        observed); the planes cover every point either way.  ``posterior`` = (loc, scale) ``[B, L]`` replaces the encoder's: "fit on a
        prefix, score the suffix" is ``refine_posterior(mask=prefix)`` and then this call with its (loc, scale) and the same mask, read at
        ``"lppd_out"``.  ONE engine call (``slode_pointwise_density``); ``eps`` ``[K, B, L]`` makes it reproducible, None takes drawing
        calls n .. n + K - 1 as ``trajectory_bounds`` does.  Where the engine refuses (adaptive solver, strided observations, measured
        arms, LDS budget) the same dict is composed from ``recon_samples`` in chunks of ``MOMENTS_CHUNK_ROWS``, scored and folded in torch
        fp64; importance weights of a family whose main loss scores the labels (proc) cannot be composed and raise ValueError."""
        if weights not in self.POINTWISE_WEIGHTS:
            raise ValueError("weights must be 'posterior' or 'importance', got %r" % (weights,))
        b = self._bind()
        B, K, imp = observations.shape[0], self._count(num_draws, "num_draws"), weights == "importance"
        if return_draws and not imp:
            raise ValueError("return_draws needs weights='importance': posterior weights form no per-draw loss")
        if mask is not None:
            mask = self._obs_layout(observations, mask)
        post = None if posterior is None else self._given_posterior(observations, posterior)

        def fused():
            point, summary, loss = b.engine.pointwise_density(
                b.flat, self._draws_batch(observations, labels, eps, K), B, K, self.POINTWISE_WEIGHTS[weights], mask=mask,
                loc=None if post is None else post[0], scale=None if post is None else post[1], loss_kb=None if return_draws else False)
            return point, summary, loss

        point, summary, loss = self._fused_or_composed(fused, lambda: self._pointwise_composed(observations, K, imp, mask, post, eps, labels))
        res = {"lppd": point[0], "mean_ll": point[1], "p_waic": point[2], "elpd_waic": point[0] - point[2]}
        res.update({n: summary[:, i] for i, n in enumerate(self.POINTWISE_NAMES)})
        if return_draws:
            res["loss"] = loss
        return res

    def _pointwise_composed(self, observations, K, imp, mask, post, eps, labels):
        """The composed route: ``(point [3, B, C, T], summary [B, 8], loss [K, B] or None)`` from the materialised curves of ``recon_samples``
        (``MOMENTS_CHUNK_ROWS // K`` rows at a time, ONE drawing call for the whole batch), every point term and every fold in fp64."""
        if imp and self.AUX and getattr(self._bind().engine.spec, "labels_in_main", False):
            raise ValueError("pointwise_density: importance weights of the %s family cannot be composed (its main loss scores the labels on z; "
                             "no unfused call returns those terms per draw): use weights='posterior' or a fixed-grid solver" % self.FAMILY)
        f64 = torch.float64
        sd = torch.nn.functional.softplus(self.decoder.constant_std.detach()).to(f64)[None, :, :, None]     # [1, C, T, 1]
        d = float(self.config.quantile_diff)
        planes, rows, losses = [], [], []
        with torch.no_grad():
            for lo, hi, e, batch in self._chunks(observations, labels, K, eps):
                obs = batch["observations"]
                pst = None if post is None else (post[0][lo:hi], post[1][lo:hi])
                s = self.recon_samples(is_post=True, num_samples=K, eps=e, posterior=pst, **batch)
                y = obs.to(f64)[..., None]
                if self.GAUSS:
                    ell = -torch.log(sd) - 0.5 * math.log(2.0 * math.pi) - 0.5 * ((y - s["mean"].to(f64)) / sd) ** 2
                else:
                    ell = 0.0
                    for name, tau in (("mu_50", 0.5), ("mu_75", 0.5 + d), ("mu_25", 0.5 - d)):
                        mu = s[name].to(f64)
                        ell = ell + torch.where(y >= mu, torch.full_like(mu, tau), torch.full_like(mu, 1.0 - tau)) * (-torch.log(2.0 * sd) - (y - mu).abs() / sd)
                w = torch.ones_like(y[..., 0]) if mask is None else mask[lo:hi].to(f64)                    # [rows, C, T]
                if imp:
                    loc, scale = (t.to(f64) for t in (self.encoder.forward(obs) if pst is None else pst))
                    ploc, pscale = (t.to(f64) for t in self._prior_loc_scale({k: v for k, v in batch.items() if k != "observations"}))
                    z = s["z"].to(f64)                                                                      # [K, rows, L]
                    log_q = torch.distributions.Normal(loc, scale).log_prob(z).sum(-1)
                    log_p = torch.distributions.Normal(ploc, pscale).log_prob(z).sum(-1)
                    loss = -((w[..., None] * ell).sum((1, 2)).t() + log_p - log_q)                          # [K, rows]
                    lw = torch.log_softmax(-loss, dim=0)
                    losses.append(loss)
                else:
                    lw = torch.full((K, hi - lo), -math.log(K), dtype=f64, device=obs.device)
                lwp = lw.t()[:, None, None, :]                                                              # [rows, 1, 1, K]
                lppd = torch.logsumexp(lwp + ell, dim=-1)
                mean = (lwp.exp() * ell).sum(-1)
                var = (lwp.exp() * (ell - mean[..., None]) ** 2).sum(-1)
                inn = (w > 0).to(f64)
                out = 1.0 - inn
                ess = 1.0 / (2.0 * lw).exp().sum(0)
                rows.append(torch.stack([(lppd * inn).sum((1, 2)), (var * inn).sum((1, 2)), (mean * inn).sum((1, 2)), inn.sum((1, 2)),
                                         (lppd * out).sum((1, 2)), (mean * out).sum((1, 2)), out.sum((1, 2)), ess], dim=1))
                planes.append(torch.stack([lppd, mean, var]))
                del s, ell
        return (torch.cat(planes, 1).to(torch.float32), torch.cat(rows, 0).to(torch.float32),
                torch.cat(losses, 1).to(torch.float32) if imp else None)

    def save_pointwise_density(self, results_dir: str, batches, num_draws: int, weights: str = "posterior"):
        """Runs ``pointwise_density`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors, optionally
        ``mask`` / ``posterior``) and writes ``pointwise_lppd_<tag>.npy``, ``pointwise_p_waic_<tag>.npy``, ``pointwise_mean_ll_<tag>.npy``
        (float32 ``[n, C, T]``) and ``waic_<tag>.npy`` (float32 ``[n, 8]``, the columns of ``POINTWISE_NAMES``), ``<tag>`` = ``post``
        (posterior weights) or ``iw`` (importance weights), the trajectories in loader order, beside the reference's result files.  One
        read-back, at the end.  Returns the four paths."""
        tag = "post" if weights == "posterior" else "iw"
        parts = {"pointwise_lppd_%s.npy" % tag: [], "pointwise_p_waic_%s.npy" % tag: [], "pointwise_mean_ll_%s.npy" % tag: [], "waic_%s.npy" % tag: []}
        for d in batches:
            r = self.pointwise_density(num_draws=num_draws, weights=weights, **d)
            for f, v in zip(parts, (r["lppd"], r["p_waic"], r["mean_ll"], torch.stack([r[n] for n in self.POINTWISE_NAMES], dim=1))):
                parts[f].append(v)
        if not parts["waic_%s.npy" % tag]:
            raise ValueError("save_pointwise_density: no batches")
        return self._save_arrays(results_dir, [(f, torch.cat(v, 0)) for f, v in parts.items()])

    @staticmethod
    def waic_line(table, p_waic, num_draws: int) -> str:
        """The printed line of ``--waic``: total elpd_waic = sum (lppd_in - p_waic_in) and its standard error sqrt(n var_b(elpd_b)) over the
        n trajectories, total p_waic, and the share of points with p_waic > 0.4 (the usual WAIC reliability warning).  ``table``: ``[n, 8]``
        (``waic_post.npy``); ``p_waic``: ``[n, C, T]``."""
        import numpy as np
        table, p_waic = np.asarray(table, np.float64), np.asarray(p_waic, np.float64)
        elpd = table[:, 0] - table[:, 1]
        n = elpd.shape[0]
        return "waic: K=%d  n=%d  elpd_waic=%.4f  se=%.4f  p_waic=%.4f  share(p_waic>0.4)=%.4f" % (
            int(num_draws), n, elpd.sum(), float(np.sqrt(n * elpd.var())) if n else 0.0, table[:, 1].sum(), float((p_waic > 0.4).mean()) if p_waic.size else 0.0)

    # ---- PSIS leave-one-out: per-point elpd_loo and the Pareto khat from K posterior draws ------------------------------------------------
    LOO_NAMES = ("elpd_loo_in", "lppd_in", "n_in", "n_bad_in", "khat_max_in", "elpd_loo_out", "lppd_out", "n_out")   # one summary row, in order
    LOO_FIT_ELEMENTS = 1 << 24      # composed route: most fp64 elements of the [points, grid, tail] table of one chunk of points

    @staticmethod
    def loo_tail_length(num_draws: int) -> int:
        """M = min(ceil(min(0.2 K, 3 sqrt K)), K - 1): the number of largest importance ratios the generalised Pareto tail is fitted to."""
        K = int(num_draws)
        return min(int(math.ceil(min(0.2 * K, 3.0 * math.sqrt(K)))), K - 1)

    @classmethod
    def _psis_loo(cls, ell):
        """``(elpd_loo, khat, tail)`` of per-draw log-densities ``ell`` ``[..., K]`` (fp64), vectorised over the points: the rule of
        ``slode_pointwise_loo`` (include/slode.h) -- sort, the tail above the cutoff, the Zhang & Stephens fit with the prior of Vehtari
        et al., the smoothed log-ratios in rank order, the self-normalised estimate.  ``tail``: the M + 1 smallest values, ascending,
        ``[M + 1, ...]``."""
        f64 = torch.float64
        shp, K = ell.shape[:-1], ell.shape[-1]
        M = cls.loo_tail_length(K)
        ls = torch.sort(ell.reshape(-1, K).to(f64), dim=-1).values
        N = ls.shape[0]
        a = ls[:, :1] - ls                                                    # [N, K], 0 at rank 0, non-increasing
        cut = a[:, M].clamp_min(math.log(2.2250738585072014e-308))
        ec = cut.exp()
        in_tail = a[:, :M] > cut[:, None]                                     # [N, M]: the ranks of the tail (a prefix)
        n = in_tail.sum(1)
        khat = torch.full((N,), float("inf"), dtype=f64, device=ell.device)
        logw = a.clone()
        fit = n >= 5
        if M >= 5 and bool(fit.any()):
            rows = max(1, cls.LOO_FIT_ELEMENTS // ((30 + int(math.isqrt(M))) * M))
            idx = fit.nonzero().reshape(-1)
            for lo in range(0, idx.numel(), rows):
                sel = idx[lo:lo + rows]
                nn, msk, e = n[sel], in_tail[sel], ec[sel]
                nf = nn.to(f64)
                x = torch.where(msk, a[sel, :M].exp() - e[:, None], torch.zeros((), dtype=f64, device=ell.device))   # [R, M] by rank (descending x)
                xq = x.gather(1, (nn - torch.floor(nf / 4.0 + 0.5).long())[:, None])[:, 0]       # x_[floor(n / 4 + 0.5) - 1], ascending order
                xn = 1.0 - e                                                                         # x_[n - 1]: rank 0
                m = 30 + torch.floor(nf.sqrt()).long()
                j = torch.arange(1, 30 + int(math.isqrt(M)) + 1, dtype=f64, device=ell.device)[None, :]
                on = j <= m[:, None].to(f64)
                b = (1.0 - (m[:, None].to(f64) / (j - 0.5)).sqrt()) / (3.0 * xq[:, None]) + 1.0 / xn[:, None]      # [R, J]
                kj = (torch.log1p(-b[:, :, None] * x[:, None, :]) * msk[:, None, :]).sum(-1) / nf[:, None]
                L = nf[:, None] * (torch.log(-b / kj) - kj - 1.0)
                w = torch.softmax(torch.where(on, L, torch.full_like(L, float("-inf"))), dim=1)       # 1 / sum_j' exp(L_j' - L_j)
                w = torch.where(w >= 10.0 * 2.0 ** -52, w, torch.zeros_like(w))
                w = w / w.sum(1, keepdim=True)
                bs = (w * torch.where(on, b, torch.zeros_like(b))).sum(1)
                ks = (torch.log1p(-bs[:, None] * x) * msk).sum(1) / nf
                sigma = -ks / bs
                kh = (nf * ks + 5.0) / (nf + 10.0)
                ok = torch.isfinite(kh) & torch.isfinite(sigma)
                r = torch.arange(M, dtype=f64, device=ell.device)[None, :]
                p = ((nf[:, None] - r) - 0.5) / nf[:, None]                                         # rank r <-> ascending index n - r
                p = torch.where(msk, p, torch.full_like(p, 0.5))
                s = torch.log(sigma[:, None] * torch.expm1(-kh[:, None] * torch.log1p(-p)) / kh[:, None] + e[:, None]).clamp_max(0.0)
                put = msk & ok[:, None]
                lw = logw[sel]
                lw[:, :M] = torch.where(put, s, lw[:, :M])
                logw[sel] = lw
                khat[sel] = torch.where(ok, kh, khat[sel])
        elpd = torch.logsumexp(logw + ls, dim=1) - torch.logsumexp(logw, dim=1)
        return elpd.reshape(shp), khat.reshape(shp), ls[:, :M + 1].t().reshape((M + 1,) + tuple(shp))

    def pointwise_loo(self, observations, num_draws: int, mask=None, posterior=None, eps=None, tile: int = 0, max_sweeps: int = 2,
                      return_tail: bool = False, **labels):
        """The remedy where ``pointwise_density`` warns that WAIC is unreliable, and the honest comparison of two fitted models:
        Pareto-smoothed importance-sampling leave-one-out (Vehtari, Gelman & Gabry 2017) from ``num_draws`` = K posterior draws.  Per
        observation point (c, t), ``[B, C, T]`` each: ``"elpd_loo"``, the log predictive density of the point with that point left
        out; ``"khat"``, the shape of the generalised Pareto tail of its importance ratios -- the estimate can be trusted below 0.5, is
        usable up to 0.7, and +inf says the tail was too short to smooth (K < 21, or ties); ``"lppd"`` (bit for bit
        ``pointwise_density``'s) and ``"p_loo"`` = lppd - elpd_loo.  Per trajectory (``[B]`` each): ``"elpd_loo_in"``, ``"lppd_in"``,
        ``"n_in"``, ``"n_bad_in"`` (points with khat > 0.7) and ``"khat_max_in"`` over the points the mask counts as observed (> 0),
        ``"elpd_loo_out"``, ``"lppd_out"``, ``"n_out"`` over the others; with ``return_tail`` ``"tail"`` ``[M + 1, B, C, T]``, the
        smallest per-draw log-densities of every point, ascending.  ``mask`` / ``posterior`` / ``eps``: as ``pointwise_density``
        (posterior weights); the counter moves by K.  ONE engine call (``slode_pointwise_loo``) that keeps only those M + 1 values per
        point, sorted, on chip: no ``[B, C, T, K]`` tensor exists.  ``tile``: time points per sweep over the draws (0: the engine's
        choice, ``Engine.loo_plan``).  The composed route -- ``recon_samples`` over chunks of trajectories, the point terms and the
        smoothing in torch fp64 -- is taken where the engine refuses (adaptive solver, strided observations, measured arms, LDS
        budget) or where the plan needs more than ``max_sweeps`` sweeps."""
        b = self._bind()
        B, K = observations.shape[0], self._count(num_draws, "num_draws")
        T = int(self.times.numel())
        if not 0 <= int(tile) <= T:
            raise ValueError("tile must lie in [0, T = %d], got %d" % (T, int(tile)))
        if mask is not None:
            mask = self._obs_layout(observations, mask)
        post = None if posterior is None else self._given_posterior(observations, posterior)

        def fused():
            return b.engine.pointwise_loo(b.flat, self._draws_batch(observations, labels, eps, K), B, K, mask=mask,
                                          loc=None if post is None else post[0], scale=None if post is None else post[1], tile=int(tile),
                                          tail=True if return_tail else None)

        def composed():
            return self._loo_composed(observations, K, mask, post, eps, labels)

        def planned():
            if b.engine.loo_plan(B, K, int(tile))[1] > int(max_sweeps):
                return composed()
            return fused()
        point, summary, tail = self._fused_or_composed(planned, composed)
        res = {"elpd_loo": point[0], "khat": point[1], "lppd": point[2], "p_loo": point[2] - point[0]}
        res.update({n: summary[:, i] for i, n in enumerate(self.LOO_NAMES)})
        if return_tail:
            res["tail"] = tail
        return res

    def _loo_composed(self, observations, K, mask, post, eps, labels):
        """The composed route: ``(point [3, B, C, T], summary [B, 8], tail [M + 1, B, C, T])`` from the materialised curves of
        ``recon_samples`` (``MOMENTS_CHUNK_ROWS // K`` rows at a time), every point term, fold and fit in fp64.  The generator's counter
        ends where the engine call leaves it: at n + K."""
        f64 = torch.float64
        sd = torch.nn.functional.softplus(self.decoder.constant_std.detach()).to(f64)[None, :, :, None]     # [1, C, T, 1]
        d = float(self.config.quantile_diff)
        planes, rows, tails = [], [], []
        with torch.no_grad(), self._counter_moves_by(K, eps):
            for lo, hi, e, batch in self._chunks(observations, labels, K, eps):
                obs = batch["observations"]
                pst = None if post is None else (post[0][lo:hi], post[1][lo:hi])
                s = self.recon_samples(is_post=True, num_samples=K, eps=e, posterior=pst, **batch)
                y = obs.to(f64)[..., None]
                if self.GAUSS:
                    ell = -torch.log(sd) - 0.5 * math.log(2.0 * math.pi) - 0.5 * ((y - s["mean"].to(f64)) / sd) ** 2
                else:
                    ell = 0.0
                    for name, tau in (("mu_50", 0.5), ("mu_75", 0.5 + d), ("mu_25", 0.5 - d)):
                        mu = s[name].to(f64)
                        ell = ell + torch.where(y >= mu, torch.full_like(mu, tau), torch.full_like(mu, 1.0 - tau)) * (-torch.log(2.0 * sd) - (y - mu).abs() / sd)
                del s
                elpd, khat, tail = self._psis_loo(ell)
                lppd = torch.logsumexp(ell, dim=-1) - math.log(K)
                del ell
                plane = torch.stack([elpd, khat, lppd]).to(torch.float32)                                   # the sums: of the rounded planes
                pe, pk, pl = plane[0].to(f64), plane[1].to(f64), plane[2].to(f64)
                inn = (torch.ones_like(pe) if mask is None else mask[lo:hi].to(f64)) > 0
                out = ~inn
                zero = torch.zeros((), dtype=f64, device=obs.device)
                rows.append(torch.stack([torch.where(inn, pe, zero).sum((1, 2)), torch.where(inn, pl, zero).sum((1, 2)), inn.sum((1, 2)).to(f64),
                                         (inn & (pk > 0.7)).sum((1, 2)).to(f64),
                                         torch.where(inn, pk, torch.full_like(pk, float("-inf"))).amax((1, 2)),
                                         torch.where(out, pe, zero).sum((1, 2)), torch.where(out, pl, zero).sum((1, 2)), out.sum((1, 2)).to(f64)], dim=1))
                planes.append(plane)
                tails.append(tail.to(torch.float32))
        return torch.cat(planes, 1), torch.cat(rows, 0).to(torch.float32), torch.cat(tails, 1)

    def save_pointwise_loo(self, results_dir: str, batches, num_draws: int):
        """Runs ``pointwise_loo`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors, optionally
        ``mask`` / ``posterior``) and writes ``pointwise_elpd_loo_post.npy``, ``pointwise_khat_post.npy`` (float32 ``[n, C, T]``) and
        ``loo_post.npy`` (float32 ``[n, 8]``, the columns of ``LOO_NAMES``), the trajectories in loader order.  One read-back, at the
        end.  Returns the three paths."""
        parts = {"pointwise_elpd_loo_post.npy": [], "pointwise_khat_post.npy": [], "loo_post.npy": []}
        for d in batches:
            r = self.pointwise_loo(num_draws=num_draws, **d)
            for f, v in zip(parts, (r["elpd_loo"], r["khat"], torch.stack([r[n] for n in self.LOO_NAMES], dim=1))):
                parts[f].append(v)
        if not parts["loo_post.npy"]:
            raise ValueError("save_pointwise_loo: no batches")
        return self._save_arrays(results_dir, [(f, torch.cat(v, 0)) for f, v in parts.items()])

    @staticmethod
    def loo_line(table, khat, num_draws: int) -> str:
        """The printed line of ``--loo``: total elpd_loo = sum elpd_loo_in and its standard error sqrt(n var_b(elpd_b)) over the n
        trajectories, total p_loo = sum (lppd_in - elpd_loo_in), and the shares of points with khat > 0.7 and with khat > 0.5.
        ``table``: ``[n, 8]`` (``loo_post.npy``); ``khat``: ``[n, C, T]``."""
        import numpy as np
        table, khat = np.asarray(table, np.float64), np.asarray(khat, np.float64)
        elpd = table[:, 0]
        n = elpd.shape[0]
        return "loo: K=%d  n=%d  elpd_loo=%.4f  se=%.4f  p_loo=%.4f  share(khat>0.7)=%.4f  share(khat>0.5)=%.4f" % (
            int(num_draws), n, elpd.sum(), float(np.sqrt(n * elpd.var())) if n else 0.0, (table[:, 1] - table[:, 0]).sum(),
            float((khat > 0.7).mean()) if khat.size else 0.0, float((khat > 0.5).mean()) if khat.size else 0.0)

    # ---- label evidence: which input does the generative model believe produced these curves? -------------------------------------------
    EVIDENCE_NAMES = ("elbo", "iw_bound", "ess", "log_post")    # the slots of one slode_label_evidence row, in order

    @classmethod
    def label_grid(cls, **values):
        """The Cartesian product of per-label value lists as hypothesis tables: ``label_grid(iext=[0, 1], rtpr=[0, 1])`` gives
        ``{"iext": [4, 1], "rtpr": [4, 1]}`` (float32), the first name varying slowest.  A value may be a row of several columns
        (``aR=torch.eye(3)``: three hypotheses for a label of width 3)."""
        import itertools
        if not values:
            raise ValueError("label_grid needs at least one label")
        for name in values:
            if name not in cls.LABELS:
                raise ValueError("label_grid: %r is not a label of the %s family (labels: %s)" % (name, cls.FAMILY, ", ".join(cls.LABELS)))
        rows = {n: torch.as_tensor(v, dtype=torch.float32) for n, v in values.items()}
        rows = {n: v.reshape(v.shape[0], -1) if v.dim() > 0 else v.reshape(1, 1) for n, v in rows.items()}
        index = list(itertools.product(*(range(v.shape[0]) for v in rows.values())))
        return {n: v[[ix[j] for ix in index]].contiguous() for j, (n, v) in enumerate(rows.items())}

    @classmethod
    def _hypothesis_tables(cls, hypotheses):
        """``hypotheses`` = {label name: [V, width]} for a non-empty subset of ``LABELS`` as ``(V, {name: float32 [V, width]})``."""
        if not hypotheses:
            raise ValueError("hypotheses must name at least one label of the %s family (labels: %s)" % (cls.FAMILY, ", ".join(cls.LABELS)))
        tabs, V = {}, None
        for name, val in hypotheses.items():
            if name not in cls.LABELS:
                raise ValueError("hypotheses: %r is not a label of the %s family (labels: %s)" % (name, cls.FAMILY, ", ".join(cls.LABELS)))
            t = torch.as_tensor(val).to(torch.float32)
            t = t.reshape(t.shape[0], -1) if t.dim() > 0 else t.reshape(1, 1)
            if V is not None and t.shape[0] != V:
                raise ValueError("hypotheses[%r] has %d rows, the others %d: every table needs the same V" % (name, t.shape[0], V))
            tabs[name], V = t.contiguous(), t.shape[0]
        return V, tabs

    @classmethod
    def hypothesis_match(cls, hypotheses, **labels):
        """``[B]`` int64: the index of the first hypothesis whose hypothesised columns equal the trajectory's own labels, -1 if none does."""
        V, tabs = cls._hypothesis_tables(hypotheses)
        B = next(iter(labels.values())).shape[0]
        hit = None
        for name, t in tabs.items():
            own = labels[name].reshape(B, -1).to(torch.float32)
            if own.shape[1] != t.shape[1]:
                raise ValueError("hypotheses[%r] must be [V, %d], got %s" % (name, own.shape[1], tuple(t.shape)))
            eq = (own[:, None, :] == t.to(own.device)[None, :, :]).all(dim=-1)             # [B, V]
            hit = eq if hit is None else hit & eq
        first = torch.argmax(hit.to(torch.int64), dim=1)
        return torch.where(hit.any(dim=1), first, torch.full_like(first, -1))

    def default_hypotheses(self, **labels):
        """The hypotheses ``--label-evidence`` scores: cvs {0, 1}^2 over iext, rtpr; challenge {0, 1}^2 over symptoms, shedding; proc the
        identity rows of aR x the identity rows of aS (widths from ``labels``), C12 / C6 left as each subject's own."""
        if self.FAMILY == "proc":
            B = labels["aR"].shape[0]
            return self.label_grid(aR=torch.eye(labels["aR"].reshape(B, -1).shape[1]), aS=torch.eye(labels["aS"].reshape(B, -1).shape[1]))
        return self.label_grid(**{l: [0.0, 1.0] for l in self.LABELS[:2]})

    def label_evidence(self, observations, num_draws: int, hypotheses, log_prior=None, eps=None, return_draws: bool = False, **labels):
        """The generative model's own answer to "which input produced these curves?", p(u | x) ~ p(u) p(x | u), for V label hypotheses
        shared by all trajectories: ``hypotheses`` = {label name: [V, width]} for a non-empty subset of ``LABELS`` (``label_grid`` builds
        the Cartesian product); a label that is not named keeps each trajectory's own value.  Per hypothesis, p(x | u_v) is estimated by the
        importance-weighted bound over ``num_draws`` = K posterior draws z_k = loc(x) + scale(x) eps_k -- the bound ``trajectory_bounds``
        gives for those labels, at the price of one encoder pass and K solves for all V.  Returns ``{"elbo", "iw_bound", "ess",
        "log_post": [B, V]; "best": [B]`` (arg-max of log_post) ``; "match": [B]`` (the hypothesis that equals the trajectory's own labels,
        -1 if none) ``}`` plus ``"loss": [V, K, B]`` with ``return_draws``.  The ESS is per hypothesis: q(z | x) is a poor proposal for a
        wrong u, and an ESS near 1 says the bound rests on one draw.  ``log_prior``: ``[V]`` (None: uniform).  ``eps`` ``[K, B, L]`` makes
        it reproducible; None takes drawing calls n .. n + K - 1 of the engine's generator, as ``trajectory_bounds``.  ONE engine call
        (``slode_label_evidence``); what the engine refuses raises its SlodeError."""
        b = self._bind()
        B, K = observations.shape[0], self._count(num_draws, "num_draws")
        V, tabs = self._hypothesis_tables(hypotheses)
        dev = observations.device
        hyp = [tabs[l].to(dev) if l in tabs else None for l in self.LABELS]
        lp = None if log_prior is None else torch.as_tensor(log_prior).to(dev, torch.float32).reshape(-1).contiguous()
        ev, best, loss = b.engine.label_evidence(b.flat, self._draws_batch(observations, labels, eps, K), B, K, hyp, V, log_prior=lp)
        res = {n: ev[:, :, i] for i, n in enumerate(self.EVIDENCE_NAMES)}
        res["best"] = best
        res["match"] = self.hypothesis_match(tabs, **{l: labels[l] for l in tabs})
        if return_draws:
            res["loss"] = loss
        return res

    def save_label_evidence(self, results_dir: str, batches, num_draws: int, hypotheses):
        """Runs ``label_evidence`` over ``batches`` (an iterable of device batch dicts: ``observations`` + the label tensors) and writes
        ``evidence_post.npy`` (float32 ``[n, V, 4]``, the columns of ``EVIDENCE_NAMES``, trajectories in loader order), ``evidence_best.npy``
        and ``evidence_match.npy`` (int32 ``[n]``) and ``evidence_hypotheses_<label>.npy`` (``[V, width]``) per hypothesised label.  One
        read-back, at the end.  Returns the paths."""
        V, tabs = self._hypothesis_tables(hypotheses)
        rows, best, match = [], [], []
        for d in batches:
            r = self.label_evidence(num_draws=num_draws, hypotheses=tabs, **d)
            rows.append(torch.stack([r[n] for n in self.EVIDENCE_NAMES], dim=2))
            best.append(r["best"].to(torch.int32))
            match.append(r["match"].to(torch.int32))
        cat = lambda parts, shp, dt: torch.cat(parts, 0).cpu() if parts else torch.zeros(shp, dtype=dt)   # noqa: E731
        named = [("evidence_post.npy", cat(rows, (0, V, len(self.EVIDENCE_NAMES)), torch.float32)),
                 ("evidence_best.npy", cat(best, (0,), torch.int32)), ("evidence_match.npy", cat(match, (0,), torch.int32))]
        named += [("evidence_hypotheses_%s.npy" % l, tabs[l]) for l in self.LABELS if l in tabs]
        return self._save_arrays(results_dir, named)

    @staticmethod
    def label_evidence_line(post, best, match) -> str:
        """One line from the files of ``save_label_evidence``: the share of subjects with best == match, the mean posterior mass exp(log_post)
        on the matching hypothesis and the median ESS there, over the subjects whose own labels are among the hypotheses."""
        import numpy as np
        post, best, match = np.asarray(post), np.asarray(best), np.asarray(match)
        on = match >= 0
        if not on.any():
            return "label_evidence: V=%d  no subject's labels are among the hypotheses (n=%d)" % (post.shape[1], len(match))
        at = post[on, match[on]]
        return "label_evidence: V=%d  matched=%d/%d  best==match=%.4f  mean_post_at_match=%.4f  median_ess_at_match=%.2f" % (
            post.shape[1], int(on.sum()), len(match), float((best[on] == match[on]).mean()), float(np.exp(at[:, 3].astype(np.float64)).mean()),
            float(np.median(at[:, 2])))
