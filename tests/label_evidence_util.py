"""Test infrastructure of the label evidence (slode_label_evidence): hypothesis tables for the seeded cases of tests/traj_bounds_util.py, the
label matrix of one hypothesis, the per-hypothesis fp64 oracle (TU.oracle_rows with ``u`` replaced) and the fp64 reduction of V x K per-draw
losses to the call's slots.  Not imported by the product.

Bars.  Slots 0-2 of a column and its losses are compared bitwise with Engine.traj_bounds on the substituted labels, and against the oracle at
the bars of tests/traj_bounds_util.py.  Slot 3 against the fp64 recomputation from the kernel's own loss_vkb: 2^-23 |value| + 1e-6 -- one fp32
rounding of the result plus the differences between two fp64 exp / log libraries and summation orders (1e-6 nat is 1e9 ulp of an fp64 value of
order 1000: far above them, far below any difference between hypotheses)."""
import numpy as np
import torch

from tests import traj_bounds_util as TU
from tests.eval_gpu_util import WIDTHS


def offsets(fam):
    """Column ranges [(lo, hi)] of the family's label tensors in u."""
    out, o = [], 0
    for w in WIDTHS[fam]:
        out.append((o, o + w))
        o += w
    return out


def binary_grid(c):
    """{0, 1}^2 over the two labels of cvs / challenge: hypothesis tables [None or [4, width]] per label tensor."""
    g = torch.tensor([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]])
    return [g[:, 0:1].contiguous(), g[:, 1:2].contiguous()]


def batch_rows(c, V=4):
    """The first V label rows of the batch as hypotheses over every label tensor."""
    return [c["u"][:V, lo:hi].contiguous().clone() for lo, hi in offsets(c["fam"])]


def seeded(c, V, only=None):
    """V deterministic hypotheses: binary columns first, real-valued shifts beyond the binary ones (cvs / challenge); one-hot aR / aS and
    the C12 / C6 of batch row v mod B moved by 0.1 per wrap (proc).  ``only``: the indices of the hypothesised tensors (others None)."""
    fam, B = c["fam"], c["B"]
    v = torch.arange(V)
    if fam == "proc":
        aR = torch.nn.functional.one_hot(v % 3, 3).float()
        aS = torch.nn.functional.one_hot((v // 3) % 4, 4).float()
        shift = (0.1 * (v // 12)).float()[:, None]
        tabs = [aR, aS, c["u"][v % B, 7:8] + shift, c["u"][v % B, 8:9] - shift]
    else:
        tabs = [((v & 1).float() + 0.25 * (v >> 2).float())[:, None], (((v >> 1) & 1).float() - 0.125 * (v >> 2).float())[:, None]]
    tabs = [t.contiguous().clone() for t in tabs]
    return [t if only is None or i in only else None for i, t in enumerate(tabs)]


def substituted(c, tabs, v):
    """The label matrix u [B, n_u] of hypothesis v: the batch's own with the columns of every hypothesised tensor replaced by its row v."""
    u = c["u"].clone()
    for (lo, hi), t in zip(offsets(c["fam"]), tabs):
        if t is not None:
            u[:, lo:hi] = t[v]
    return u


def oracle(c, tabs, eps=None, rows=None, dtype=torch.float64):
    """TU.oracle_rows per hypothesis: dict(loss [V, K, B], nll [V, K, B], mag [V, K, B])."""
    V = next(t for t in tabs if t is not None).shape[0]
    per = [TU.oracle_rows(dict(c, u=substituted(c, tabs, v)), eps=eps, rows=rows, dtype=dtype) for v in range(V)]
    return {k: np.stack([p[k] for p in per]) for k in ("loss", "nll", "mag")}


def reduce64(loss, log_prior=None):
    """The call's slots from per-draw losses [V, K, B] in fp64: (elbo, iw_bound, ess, log_post), [B, V] each, and best [B]."""
    loss = np.asarray(loss, dtype=np.float64)
    V = loss.shape[0]
    cols = [TU.reduce64(loss[v]) for v in range(V)]
    elbo, iw, ess = (np.stack([col[i] for col in cols], axis=1) for i in range(3))
    t = (0.0 if log_prior is None else np.asarray(log_prior, dtype=np.float64)[None, :]) - iw
    m = t.max(axis=1, keepdims=True)
    post = t - (m + np.log(np.exp(t - m).sum(axis=1, keepdims=True)))
    return elbo, iw, ess, post, post.argmax(axis=1)


def post_bar(value):
    return 2.0 ** -23 * np.abs(value) + 1e-6
