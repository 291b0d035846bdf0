"""What the CPU tests of the plan entry points share: the hand count of the LDS pieces every kernel on slode_forward.h carves first (fwd_lds)
and an Engine that only knows its shape.  Each test module spells out its kernel's own pieces (moment tables, deviations, capture table, ...)
beside them.  Not imported by the product."""


def r4(n):
    """n floats rounded up to a multiple of four: every LDS piece begins on 16 bytes."""
    return (n + 3) & ~3


def fwd_shared_pieces(T, S, C, L, H, n_u, gauss, generic=False):
    """Floats of the shared forward pieces in carve order, each rounded up to four: the step table A and b, (T - 1) S each; one row of
    2 + 2 S floats rounded up to four per hidden unit (w_t | u_j | W_g[S] | W_d[S]; S = 8 in the run-time-S build, ``generic``); the
    transposed first layers L x 2 H; their biases 2 H; the init net's output layer H S + S; the head weights Q C S; the dynamics biases
    2 S; z; the labels max(n_u, 1); the init net's hidden layer H; x0."""
    Q = 1 if gauss else 3
    row = (2 + 2 * (8 if generic else S) + 3) & ~3
    return [r4(n) for n in ((T - 1) * S, (T - 1) * S, H * row, L * 2 * H, 2 * H, H * S + S, Q * C * S, 2 * S, L, max(n_u, 1), H, S)]


def fwd_shared_floats(T, S, C, L, H, n_u, gauss, generic=False):
    return sum(fwd_shared_pieces(T, S, C, L, H, n_u, gauss, generic))


def spec_shared_floats(spec, T, generic=False):
    """``fwd_shared_floats`` of an engine ModelSpec."""
    return fwd_shared_floats(T, spec.ode_state_dim, spec.n_channels, spec.latent_dim, spec.ode_hidden_dim, spec.n_u, spec.gauss, generic)


def host_engine(case, T=None):
    """An Engine that only knows its shape -- case ``case`` of eval_stats_util.CASES on a grid of ``T`` points (None: the case's own):
    what the plans need."""
    from structured_latent_odes_amd import _lib as L, engine as E
    from tests import eval_stats_util as EU
    fam, kw, _, T0 = EU.CASES[case]

    class _E(E.Engine):
        def __init__(self, spec, T):
            self.spec, self.T, self._shapes = spec, T, {}
            self.lib = L.load()

    return _E({"cvs": E.cvs_spec, "challenge": E.challenge_spec, "proc": E.proc_spec}[fam](solver="rk4", **kw), T or T0)
