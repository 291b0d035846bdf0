"""Test infrastructure of the calibration pass (slode_calibration): the comparison rule of tests/test_calibration_cpu.py and
tests/test_gpu_calibration.py, the numpy restatement of the kernel's accumulation (phase M6'' of calibration_kernel and
calibration_merge), the fp64 oracle by cohort and the constructed observations.  Not imported by the product.

The comparison rule (a condition, not a measurement).  An indicator compares two quantities; a (draw, member, c, t) point is NEAR for that
indicator when the two quantities differ by no more than the sum of their bars: the suite's bar for one head value, RU.MEAN_BAR max(1, |v|),
and 0 for an observation.  Against the fp64 oracle a count may differ from the oracle's by at most the number of near points in its cell
(indicator, cohort, c, t), and by nothing elsewhere.  Over a whole case the near (point, indicator) pairs may be at most NEAR_SHARE = 1e-3
of all such pairs: above that the check fails rather than excusing them (the share per indicator is printed beside it).  `inside`
compares y with v_2 and with v_1: near for either; `cross` compares v_2 with v_0 and v_0 with v_1: near for either pair, each with both
bars.

Float bars against the oracle: the pinball summand is 1-Lipschitz in v, so a mean of terms whose v is within the per-value bar is within the
mean of the bars; the factor 2 covers the accumulation: 2 MEAN_BAR x the oracle's mean of max(1, |v_j|) over the cell.  width = mean of
v_1 - v_2: the sum of that bar for v_1 and for v_2.

Accumulation bound (accumulation_bar), u = 2^-24.  The kernel forms every summand in fp32 from exact fp32 inputs and adds it into an fp64
slot; the chunk partials and the sum over t are added in fp64, divided in fp64, rounded once to fp32.
  pinball summand fl(fl(y - v) w), w = tau or fl(tau - 1): three roundings, relative error <= 3u + O(u^2) < 4u of |term|
  width summand fl(v_1 - v_2): one rounding, <= u |term|
  fp64 additions of N terms: <= N 2^-53 sum|term|, below u^2 N sum|term|: invisible for N < 2^29
  one rounding of the fp32 output: u |mean|, and |mean| <= mean|term|
                                                               -> |error| <= 5 u mean|term|  (pinball terms are >= 0: mean|term| = pinball)
The bound has no factor in the number of terms.  The rejected form, ONE fp32 running sum over the chunk x K terms, has one: every addition
rounds to the running sum's ulp, up to N u / 2 in all; on curves that vary by a few ulp every addition rounds the same way, and at 1280
terms the form misses the bound several times over (tests/test_calibration_cpu.py).  Two chunk sizes differ by at most the bound of each:
10 u mean|term|."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import cohort_util as CU
from tests import eval_stats_util as EU
from tests import recon_moments_util as RU
from tests.cohort_util import member_lists, oracle_draws, parity_ids, thin_band   # noqa: F401  (the issue's CU.*: shared as they stand)
from tests.recon_moments_util import _f32

MEAN_BAR = RU.MEAN_BAR
NEAR_SHARE = 1e-3
U = 2.0 ** -24
PHI2, PHIM2 = 0.97724986805182079, 0.022750131948179195
NAMES = ("below0", "below1", "below2", "inside", "cross")


def nominal(ospec):
    """[3] fp64: the nominal levels of the three curves."""
    if ospec.gauss:
        return np.array([0.5, PHI2, PHIM2])
    d = float(ospec.quantile_diff)
    return np.array([0.5, 0.5 + d, 0.5 - d])


def bar(v):
    return MEAN_BAR * np.maximum(1.0, np.abs(v))


# ---- indicators and summands of given curves ----------------------------------------------------------------------------------------------
def indicators(y, v):
    """y [...], v [3, ...] (broadcastable): the five indicators [5, ...] as bool, comparisons false on NaN."""
    b = [y < v[j] for j in range(3)]
    return np.stack(np.broadcast_arrays(*(b + [(v[2] <= y) & b[1], (v[2] > v[0]) | (v[0] > v[1])])))


def near(y, v, factor=1.0):
    """[5, ...] bool: the near points of every indicator under the comparison rule.  factor = 2: two fp32 evaluations of the curves, each
    within the bar of the truth, compared with each other (the model's decoder against the fused kernel)."""
    n = [np.abs(y - v[j]) <= factor * bar(v[j]) for j in range(3)]
    pair = lambda a, b: np.abs(v[a] - v[b]) <= factor * (bar(v[a]) + bar(v[b]))
    return np.stack(np.broadcast_arrays(*(n + [n[1] | n[2], pair(2, 0) | pair(0, 1)])))


def summands64(y, v, tau):
    """[4, ...] fp64: pinball 0..2 and the width, exact arithmetic on the given values."""
    y, v = np.asarray(y, np.float64), np.asarray(v, np.float64)
    return np.stack(np.broadcast_arrays(*([(y - v[j]) * (tau[j] - (y < v[j])) for j in range(3)] + [v[1] - v[2]])))


# ---- the accumulation of calibration_kernel (phase M6'') and calibration_merge, operation by operation -----------------------------------
def tau32(tau):
    """(tau, fl(tau - 1)) in fp32, as the kernel holds them."""
    t = _f32(tau)
    return t, _f32(t - np.float32(1.0))


def summands_f32(y, v, tau):
    """[4, ...] fp32: the kernel's summands fl(fl(y - v) w) and fl(v_1 - v_2) of fp32 inputs."""
    y, v = _f32(y), _f32(v)
    t, tm = tau32(tau)
    out = [_f32(_f32(y - v[j]) * np.where(y < v[j], tm[j], t[j]).astype(np.float32)) for j in range(3)]
    return np.stack(out + [_f32(v[1] - v[2]) + np.zeros_like(y)])


def chunk_partial(y, v, tau):
    """y [n, C, T], v [3, n, K, C, T] fp32, members and draws in list order -> (n, counts int32 [5, C, T], sums fp64 [4, C, T]): the
    partial the kernel writes -- every summand formed in fp32, added into the fp64 slot in order."""
    n, K = v.shape[1:3]
    cnt = np.zeros((5,) + y.shape[1:], np.int32)
    acc = np.zeros((4,) + y.shape[1:], np.float64)
    for j in range(n):
        for k in range(K):
            cnt += indicators(_f32(y[j]), _f32(v[:, j, k])).astype(np.int32)
            acc += summands_f32(y[j], v[:, j, k], tau).astype(np.float64)
    return n, cnt, acc


def chunk_partial_running_f32(y, v, tau):
    """The form the kernel does NOT use: one fp32 running sum per slot over the chunk's members x draws."""
    n, K = v.shape[1:3]
    cnt = np.zeros((5,) + y.shape[1:], np.int32)
    acc = np.zeros((4,) + y.shape[1:], np.float32)
    for j in range(n):
        for k in range(K):
            cnt += indicators(_f32(y[j]), _f32(v[:, j, k])).astype(np.int32)
            acc = _f32(acc + summands_f32(y[j], v[:, j, k], tau))
    return n, cnt, acc


def tree_sum_t(a, nt=256):
    """The merge's sum over t of a [..., T] in fp64: thread i adds t = i, i + 256, ...; a shuffle-down tree over the 64 lanes of each wave;
    the four wave sums as ((w0 + w1) + w2) + w3."""
    a = np.asarray(a, np.float64)
    T = a.shape[-1]
    per = np.zeros(a.shape[:-1] + (nt,), np.float64)
    for t in range(T):
        per[..., t % nt] += a[..., t]
    w = per.reshape(a.shape[:-1] + (nt // 64, 64)).copy()
    off = 32
    while off:
        w[..., :off] = w[..., :off] + w[..., off:2 * off]      # lane i += lane i + off (lanes >= off are not read again)
        off >>= 1
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def merge(partials, K, running=False):
    """calibration_merge: the partials of one cohort -- four contiguous slices of ceil(n / 4), each added in slot order, the slices as
    ((s0 + s1) + s2) + s3 -- -> (counts int32 [5, C, T], pinball fp32 [3, C], width fp32 [C]).
    running: the rejected form all the way -- fp32 partial sums, fp32 over the partials and over t."""
    N = sum(p[0] for p in partials)
    cnt = sum(p[1] for p in partials)
    if running:
        acc = np.zeros_like(partials[0][2])
        for p in partials:
            acc = _f32(acc + p[2])
        tot = np.zeros(acc.shape[:-1], np.float32)
        for t in range(acc.shape[-1]):
            tot = _f32(tot + acc[..., t])
        mean = _f32(tot / np.float32(N * K * acc.shape[-1]))
    else:
        q = -(-len(partials) // 4)
        slices = []
        for s in range(4):
            acc = np.zeros_like(partials[0][2])
            for p in partials[s * q:(s + 1) * q]:
                acc = acc + p[2]
            slices.append(acc)
        acc = ((slices[0] + slices[1]) + slices[2]) + slices[3]
        mean = _f32(tree_sum_t(acc) / (float(N) * K * acc.shape[-1]))
    return cnt, mean[:3], mean[3]


def scheme(y, v, tau, R, running=False):
    """y [n, C, T], v [3, n, K, C, T]: chunks of R consecutive members, one partial each, merged."""
    n, K = v.shape[1:3]
    part = chunk_partial_running_f32 if running else chunk_partial
    return merge([part(y[lo:lo + R], v[:, lo:lo + R], tau) for lo in range(0, n, R)], K, running)


def accumulation_bar(mean_abs_term):
    """The bound of the module docstring on a float output whose summands have this mean absolute value."""
    return 5.0 * U * np.asarray(mean_abs_term, np.float64)


# ---- the fp64 oracle by cohort ---------------------------------------------------------------------------------------------------------
def oracle_curves(c, is_post, eps=None):
    """[3, ns, B, C, T] fp64: the three curves of every draw -- the oracle's heads (ALD) or mean, mean + 2 s, mean - 2 s (Gauss)."""
    mu = oracle_draws(c, is_post, eps)
    if not c["ospec"].gauss:
        return mu
    w = 2.0 * F.softplus(EU.f64(c["p"])["decoder.constant_std"]).numpy()
    return np.stack([mu[0], mu[0] + w, mu[0] - w])


def reduce_by_cohort(y, v, tau, ids, G, factor=1.0):
    """y [B, C, T], v [3, ns, B, C, T] -> dict: counts int64 [5, G, C, T], near int64 [5, G, C, T], pinball [3, G, C], width [G, C] (NaN:
    empty cohort), scale [3, G, C] (the mean of max(1, |v_j|) over the cell), points (members x draws x C x T over all cohorts) and
    near_share [5] per indicator, near_total over all (point, indicator) pairs."""
    ns, B, C, T = v.shape[1:]
    ind, nr = indicators(y[None], v), near(y[None], v, factor)         # [5, ns, B, C, T]
    sm = summands64(y[None], v, tau)                                   # [4, ns, B, C, T]
    out = dict(counts=np.zeros((5, G, C, T), np.int64), near=np.zeros((5, G, C, T), np.int64), pinball=np.full((3, G, C), np.nan),
               width=np.full((G, C), np.nan), scale=np.full((3, G, C), np.nan), count=np.zeros(G, np.int64), factor=factor)
    ids = np.asarray(ids)
    for g in range(G):
        sel = np.flatnonzero(ids == g)
        out["count"][g] = sel.size
        if sel.size:
            out["counts"][:, g] = ind[:, :, sel].sum((1, 2))
            out["near"][:, g] = nr[:, :, sel].sum((1, 2))
            m = sm[:, :, sel].mean((1, 2, 4))
            out["pinball"][:, g], out["width"][g] = m[:3], m[3]
            out["scale"][:, g] = np.maximum(1.0, np.abs(v[:, :, sel])).mean((1, 2, 4))
    out["points"] = int((ids >= 0).sum()) * ns * C * T
    out["near_share"] = out["near"].sum((1, 2, 3)) / max(out["points"], 1)
    out["near_total"] = float(out["near_share"].mean())
    return out


def oracle_calibration(c, is_post, ids, G, obs=None, eps=None):
    y = (c["obs"] if obs is None else obs).double().numpy()
    return reduce_by_cohort(y, oracle_curves(c, is_post, eps), nominal(c["ospec"]), ids, G)


def constructed_case(case):
    """RU.build(case, "rk4", B=9, ns=7) with observations that make the counts mean something, on the prior side where the construction is
    not circular: y = fp32(head 0 of one extra prior draw + 0.05 max(1, |v|) N(0, 1)); the extra draw torch.randn(1, B, L, seed 99), the
    noise default_rng(4)."""
    c = RU.build(case, "rk4", B=9, ns=7)
    extra = torch.randn(1, 9, c["ospec"].latent_dim, generator=torch.Generator().manual_seed(99))
    v = oracle_draws(c, False, extra)[0, 0]                             # [B, C, T]
    y = v + 0.05 * np.maximum(1.0, np.abs(v)) * np.random.default_rng(4).standard_normal(v.shape)
    return c, torch.from_numpy(y.astype(np.float32))


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def check(got, want, tag, ns):
    """got: (below [3, G, C, T], inside, cross, pinball, width) -- tensors or arrays, None: not asked; want: reduce_by_cohort's dict.
    Prints the near shares and the worst ratios, then asserts the comparison rule and the float bars; empty cohorts: counts 0, floats NaN."""
    below, inside, cross, pinball, width = (None if x is None else _np(x) for x in got)
    live = want["count"] > 0
    share = want["near_share"]
    ints = [below[0], below[1], below[2], inside, cross]
    diff = [None if x is None else np.abs(x.astype(np.int64) - want["counts"][i]) for i, x in enumerate(ints)]
    cells = [0 if d is None else int((d > 0).sum()) for d in diff]
    line = "%s: near share %.2e (per indicator %s); cells that differ %s" % (tag, want["near_total"], " ".join("%.1e" % s for s in share), cells)
    assert want["near_total"] <= NEAR_SHARE, (tag, "too many near points to excuse", share)
    for i, (x, d) in enumerate(zip(ints, diff)):
        if x is None:
            continue
        assert x.min() >= 0 and np.all(x <= (want["count"] * ns).reshape(-1, 1, 1)), (tag, NAMES[i], "a count out of range")
        assert np.all(x[~live] == 0), (tag, NAMES[i], "an empty cohort must count 0")
        assert np.all(d <= want["near"][i]), (tag, NAMES[i], int((d > want["near"][i]).sum()), "cells beyond their near points")
    if pinball is not None:
        assert np.isnan(pinball[:, ~live]).all() and np.isfinite(pinball[:, live]).all(), tag
        rp = float((np.abs(pinball - want["pinball"])[:, live] / (2 * MEAN_BAR * want["factor"] * want["scale"][:, live])).max()) if live.any() else 0.0
        line += "; pinball error / bar %.3e" % rp
        assert rp <= 1.0, (tag, "pinball", rp)
    if width is not None:
        assert np.isnan(width[~live]).all() and np.isfinite(width[live]).all(), tag
        rw = float((np.abs(width - want["width"])[live] / (MEAN_BAR * want["factor"] * (want["scale"][1] + want["scale"][2])[live])).max()) if live.any() else 0.0
        line += "; width error / bar %.3e" % rw
        assert rw <= 1.0, (tag, "width", rw)
    print(line)
    return cells
