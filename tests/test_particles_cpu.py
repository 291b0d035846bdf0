"""Trace_ELBO(num_particles=K) without a GPU: the Pyro stand-ins' arguments, the plumbing from SVI down to the engine calls (with an
engine double that records what it is handed), and the noise convention of K particles restated in numpy (tests/rng_math.py):
particle k of a step that starts at drawing call n is drawing call n + k, trajectory index unchanged."""
import numpy as np
import pytest
import torch

from tests import rng_math as R


def test_trace_elbo_takes_any_positive_integer():
    from structured_latent_odes_amd.svi import Trace_ELBO
    assert Trace_ELBO().num_particles == 1
    assert Trace_ELBO(num_particles=4).num_particles == 4
    assert Trace_ELBO(num_particles=3, vectorize_particles=True, max_plate_nesting=2).num_particles == 3   # other keywords: ignored
    assert Trace_ELBO(num_particles=np.int64(2)).num_particles == 2
    for bad in (0, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            Trace_ELBO(num_particles=bad)


class RecordingEngine:
    """Engine double: same method names as structured_latent_odes_amd.engine.Engine for the step path; records every call's particle
    count and eps shape, writes a loss, applies no arithmetic."""
    L_ = 4

    def __init__(self):
        self.device = torch.device("cpu")
        self.n_params = 10
        self.spec = type("S", (), {"latent_dim": self.L_})()
        self.calls = []

    def rng_state(self):
        return 0, 0, 0

    def aux_only_region(self):
        return 0, 0

    def adam_region(self, lo, hi, delta):
        pass

    def payload_floats(self, kind):
        return 16

    def make_batch(self, obs, labels, eps=None, particles=1):
        B = obs.shape[0]
        if eps is not None:
            want = (B, self.L_) if particles == 1 else (particles, B, self.L_)
            if tuple(eps.shape) != want:
                raise ValueError("eps must be %s" % (want,))
        self.calls.append(("make_batch", particles, None if eps is None else tuple(eps.shape)))
        return ("batch", particles)

    def svi_step(self, kind, params, batch, B, loss_out, grads=None, adam=None, particles=1):
        assert batch == ("batch", particles)
        self.calls.append(("svi_step", kind, particles, grads is not None, adam[3] if adam is not None else None))
        loss_out[0] = 1.0
        return loss_out

    def grad_partial(self, kind, params, batch, B, payload, particles=1):
        self.calls.append(("grad_partial", kind, particles))

    def grad_apply(self, kind, params, batch, B, payload, loss_out, grads, adam=None, particles=1):
        self.calls.append(("grad_apply", kind, particles, adam[3] if adam is not None else None))
        loss_out[0] = 1.0
        return loss_out

    def adam_step(self, params, grads, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8):
        self.calls.append(("adam_step", step))


class FakeModel:
    """What svi.SVI needs of a MechanisticModel: bound model / guide methods, _bind(), LABELS."""
    LABELS = ("iext",)

    def __init__(self):
        eng = RecordingEngine()
        self._b = type("B", (), {"engine": eng, "flat": torch.zeros(12), "n_total": 12})()

    def _bind(self):
        return self._b

    def model(self):
        pass

    def guide(self):
        pass

    def model_meta(self):
        pass

    def guide_meta(self):
        pass


def _svis(K):
    from structured_latent_odes_amd.svi import SVI, Adam, Trace_ELBO
    m = FakeModel()
    opt = Adam({"lr": 1e-3})
    elbo = Trace_ELBO(num_particles=K)
    return m, opt, SVI(m.model, m.guide, opt, loss=elbo), SVI(m.model_meta, m.guide_meta, opt, loss=elbo)


def test_svi_hands_the_particle_count_to_every_engine_call():
    from structured_latent_odes_amd import _lib as L
    B, K = 5, 3
    m, opt, main, aux = _svis(K)
    eng = m._bind().engine
    batch = dict(observations=torch.zeros(B, 3, 20), iext=torch.zeros(B))
    for svi, kind in ((main, L.SVI_MAIN), (aux, L.SVI_AUX)):
        t0 = opt._flat.t
        eng.calls.clear()
        assert svi.step(**batch) == 1.0
        assert eng.calls == [("make_batch", K, None), ("svi_step", kind, K, True, t0 + 1)]        # ONE engine step, K inside it
        assert opt._flat.t == t0 + 1                                                            # the optimizer steps once
        eng.calls.clear()
        svi.step_async(**batch)
        assert eng.calls == [("make_batch", K, None), ("svi_step", kind, K, True, t0 + 2)] and opt._flat.t == t0 + 2
        eng.calls.clear()
        svi.evaluate_loss(**batch)
        assert eng.calls == [("make_batch", K, None), ("svi_step", kind, K, False, None)] and opt._flat.t == t0 + 2
        # explicit noise: one particle-major [K, B, L] tensor
        eng.calls.clear()
        svi.step(eps=torch.zeros(K, B, eng.L_), **batch)
        assert eng.calls[0] == ("make_batch", K, (K, B, eng.L_)) and opt._flat.t == t0 + 3
        with pytest.raises(ValueError):
            svi.step(eps=torch.zeros(B, eng.L_), **batch)
        with pytest.raises(ValueError):
            svi.evaluate_loss(eps=torch.zeros(K + 1, B, eng.L_), **batch)
        assert opt._flat.t == t0 + 3                                                            # a refused step does not count


def test_data_parallel_routes_carry_the_particle_count():
    from structured_latent_odes_amd import _lib as L
    B, K = 4, 3
    m, opt, main, aux = _svis(K)
    eng = m._bind().engine
    batch = dict(observations=torch.zeros(B, 3, 20), iext=torch.zeros(B))
    for svi, kind in ((main, L.SVI_MAIN), (aux, L.SVI_AUX)):
        svi._impl.unfused = True
        svi._impl.dp_payload = "G"                        # small payload: grad_partial -> (all-reduce) -> grad_apply
        t0 = opt._flat.t
        eng.calls.clear()
        svi.step(**batch)
        assert eng.calls == [("make_batch", K, None), ("grad_partial", kind, K), ("grad_apply", kind, K, t0 + 1)]
        svi._impl.dp_payload = "grad"                     # flat gradient: gradient-only step -> (all-reduce) -> Adam
        eng.calls.clear()
        svi.step(**batch)
        assert eng.calls == [("make_batch", K, None), ("svi_step", kind, K, True, None), ("adam_step", t0 + 2)]
        assert opt._flat.t == t0 + 2


def test_one_particle_calls_do_not_mention_particles():
    """K = 1 is the call the engine has always received: no particles keyword (an engine double that predates it keeps working)."""
    m, opt, main, aux = _svis(1)
    eng = m._bind().engine
    seen = []
    eng.make_batch = lambda obs, labels, eps=None, **kw: seen.append(kw) or "b"
    eng.svi_step = lambda kind, params, batch, B, loss_out, grads=None, adam=None, **kw: seen.append(kw) or loss_out
    main.step(observations=torch.zeros(2, 3, 20), iext=torch.zeros(2))
    aux.evaluate_loss(observations=torch.zeros(2, 3, 20), iext=torch.zeros(2))
    assert seen == [{}, {}, {}, {}]


def test_training_forwards_config_num_particles():
    import inspect
    from structured_latent_odes_amd import training
    assert "Trace_ELBO(num_particles=config.num_particles)" in inspect.getsource(training)


def test_noise_convention_of_k_particles_in_numpy():
    """Particle k of a step at counter n is drawing call n + k at the same trajectory index: the K draws differ pairwise, and a shard
    [b0, b0 + B) of particle k is rows b0 .. b0 + B - 1 of the unsharded draw (sharding is a matter of first_trajectory alone)."""
    seed, n, K, L_ = 0xC0FFEE, 11, 4, 8
    full = [R.normals(seed, n + k, 0, 64, L_) for k in range(K)]
    for a in range(K):
        for b in range(a):
            assert not np.array_equal(full[a], full[b])
            assert (full[a] != full[b]).mean() > 0.99
    b0, B = 17, 24
    for k in range(K):
        assert np.array_equal(R.normals(seed, n + k, b0, B, L_), full[k][b0:b0 + B])
    # the raw words too: counter word 2 is n + k, word 0 the global trajectory
    assert np.array_equal(R.raw_words(seed, n + 2, b0, B, L_), R.raw_words(seed, n + 2, 0, 64, L_)[b0:b0 + B])
