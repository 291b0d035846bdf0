"""Test infrastructure of the cohort moments (slode_cohort_moments): every bar of tests/test_cohort_cpu.py and tests/test_gpu_cohort.py,
the numpy restatement of the kernel's accumulation (phase M6' of cohort_moments_kernel and the fp64 merge), the member lists of a cohort
assignment and the fp64 oracle composed by cohort.  Not imported by the product.

Oracle bars -- the suite's own, derived as in the docstring of tests/test_gpu_recon_moments.py from the bar of one head value,
1e-4 max(1, |mu|): a mean of values within that bar is within it (MEAN_BAR); each sd is a scaled 2-norm of centred values within the
bar, so by the triangle inequality its error is at most the bar, and twice it covers the accumulation (SD_BAR, both sds).  The mean
observation is an fp32 sum of at most R exact fp32 values per chunk, the chunk sums added and divided in fp64 and rounded once: at most
(R - 1) u per chunk sum relative to R max|y|, i.e. (R - 1) u max|y| on the mean, plus the final rounding: within (R + 1) u max|y|,
u = 2^-24 (obs_bar).  l1 sums T absolute differences of the two: the sum over t of the mean's bar plus T times the observation bar.

Accumulation bounds (accumulation_bars), u = 2^-24, one partial = R members x K draws, n = R K values; D = the largest distance of a
value from its chunk's first value (chunk_spread).  As RU.accumulation_bars:
  d = fl(v - v00): |error| <= u D;  t1: n - 1 additions of terms <= D: <= n^2 u D on the sum, n u D on the chunk's mean
  mean of a chunk = v00 + t1 / n formed in fp64; the fp64 merge adds nothing visible; one rounding to fp32 -> u |mean| + (n + 1) u D
  t2 likewise <= (n + 2) u n D^2; var = (t2 - t1^2 / n) / n in fp64: <= 3 (n + 1) u D^2; Chan's between-chunk term uses chunk means
  with error <= n u D against a distance <= 2 D: 4 n u D^2 more on the variance at most, which the factor below absorbs for R >= 1:
  sd error = var error / (2 sd), and the one rounding of the fp32 output            -> 1.5 (R K + R + 1) u D^2 / sd + u sd
  member means: m1 has K terms (<= K^2 u D), mb = fl(m1 / K): <= (K + 1) u D each; b1, b2 have R terms: the same form with the R
  member means, each carrying its own (K + 1) u D: var error <= 3 (R + 1) u D^2 + 2 D (K + 1) u D <= 3 (R K + R + 1) u D^2
                                                                                         -> 1.5 (R K + R + 1) u D^2 / sd_subjects + u sd_subjects
(The output's own rounding is the whole error where a partial holds one value, R = K = 1: D = 0 there.)
A numpy run of the restatement below (fp32 partials, fp64 Chan merge) on curves whose sd is 1e-4 of their level stayed within 0.94 of
the mean bound and a factor ten under the sd bounds; tests/test_cohort_cpu.py repeats it."""
import numpy as np
import torch

from oracle import slode_oracle as O
from tests import eval_stats_util as EU
from tests import recon_moments_util as RU
from tests.recon_moments_util import _f32, _fma32

MEAN_BAR, SD_BAR = RU.MEAN_BAR, RU.SD_BAR
SPREAD = RU.SPREAD
U = 2.0 ** -24


# ---- member lists ----------------------------------------------------------------------------------------------------------------------
def member_lists(ids, G):
    """(members int32 [M], offsets int32 [G + 1]) of ids [B] (negative: no cohort): stable, batch order inside a cohort."""
    ids = np.asarray(ids, dtype=np.int64)
    members = np.concatenate([np.flatnonzero(ids == g) for g in range(G)] + [np.zeros(0, np.int64)]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([(ids == g).sum() for g in range(G)])]).astype(np.int32)
    return members, offsets


def parity_ids():
    """B = 23, G = 5, cohort sizes (7, 0, 11, 1, 2), two trajectories in no cohort, members interleaved in batch order."""
    ids = np.array([0] * 7 + [2] * 11 + [3] + [4] * 2 + [-1] * 2)
    return ids[np.random.RandomState(5).permutation(23)], 5


# ---- the accumulation of cohort_moments_kernel (phase M6') and cohort_merge_kernel, operation by operation ----------------------------
def chunk_partial_f32(vals):
    """vals [members of the chunk, K, ...] fp32 in list order -> (n, v00, t1, t2, b1, b2), the partial the kernel writes."""
    vals = _f32(vals)
    n, K = vals.shape[:2]
    v00 = vals[0, 0]
    t1, t2, b1, b2 = (np.zeros_like(v00) for _ in range(4))
    for j in range(n):
        m1 = np.zeros_like(v00)
        for k in range(K):
            if j or k:
                dv = _f32(vals[j, k] - v00)
                t1 = _f32(t1 + dv)
                t2 = _fma32(dv, dv, t2)
                m1 = _f32(m1 + dv)
        mb = _f32(m1 / np.float32(K))
        b1 = _f32(b1 + mb)
        b2 = _fma32(mb, mb, b2)
    return n, v00, t1, t2, b1, b2


def chunk_partial_plain_f32(vals):
    """The form the kernel does NOT use: fp32 sums of v and v^2 (and of the member means and their squares), no shift."""
    vals = _f32(vals)
    n, K = vals.shape[:2]
    s1, s2, b1, b2 = (np.zeros_like(vals[0, 0]) for _ in range(4))
    for j in range(n):
        m1 = np.zeros_like(s1)
        for k in range(K):
            s1 = _f32(s1 + vals[j, k])
            s2 = _fma32(vals[j, k], vals[j, k], s2)
            m1 = _f32(m1 + vals[j, k])
        mb = _f32(m1 / np.float32(K))
        b1 = _f32(b1 + mb)
        b2 = _fma32(mb, mb, b2)
    return n, np.zeros_like(s1), s1, s2, b1, b2


def merge64(partials, K):
    """cohort_merge_kernel: every partial as (count, mean, M2) of its values and of its member means in fp64, Chan's update in slot order;
    (mean, sd, sd_subjects) in fp32."""
    nA = mA = 0.0
    meanA = M2A = meanbA = M2bA = 0.0
    for n, v00, t1, t2, b1, b2 in partials:
        v00, t1, t2, b1, b2 = (np.asarray(x, np.float64) for x in (v00, t1, t2, b1, b2))
        nk = float(n * K)
        meanB, M2B = v00 + t1 / nk, (np.maximum(t2 - t1 * t1 / nk, 0.0) if nk > 1 else 0.0 * t2)
        meanbB, M2bB = v00 + b1 / n, (np.maximum(b2 - b1 * b1 / n, 0.0) if n > 1 else 0.0 * b2)
        nn, d = nA + nk, meanB - meanA
        meanA, M2A, nA = meanA + d * (nk / nn), M2A + M2B + d * d * (nA * nk / nn), nn
        nn, d = mA + n, meanbB - meanbA
        meanbA, M2bA, mA = meanbA + d * (n / nn), M2bA + M2bB + d * d * (mA * n / nn), nn
    return _f32(meanA), _f32(np.sqrt(M2A / nA)), _f32(np.sqrt(M2bA / mA))


def cohort_scheme_f32(vals, R, partial=chunk_partial_f32):
    """vals [n members, K, ...]: chunks of R consecutive members, one partial each, merged."""
    n, K = vals.shape[:2]
    return merge64([partial(vals[lo:lo + R]) for lo in range(0, n, R)], K)


def chunk_spread(vals64, R):
    """D [...]: the largest distance of a value from the first value of its chunk."""
    n = vals64.shape[0]
    return np.max([np.abs(vals64[lo:lo + R] - vals64[lo, 0]).max((0, 1)) for lo in range(0, n, R)], 0)


def accumulation_bars(mean64, sd64, sdb64, D, R, K):
    """(mean, sd, sd_subjects) bounds of the module docstring; an sd of exactly 0 has no bound here (the callers compare those exactly)."""
    n = R * K
    with np.errstate(divide="ignore", invalid="ignore"):
        return (U * np.abs(mean64) + (n + 1) * U * D, 1.5 * (n + R + 1) * U * D * D / sd64 + U * sd64, 1.5 * (n + R + 1) * U * D * D / sdb64 + U * sdb64)


def thin_band(n, K, shape=(5, 11), seed=3, level=1.0, rel=1e-4):
    """[n, K, *shape] fp32 curves whose sd is ``rel`` of their level: a member effect and a draw effect of the same size."""
    g = np.random.default_rng(seed)
    base = level * (1.0 + g.random(shape))
    return _f32(base * (1.0 + rel * (g.standard_normal((n, 1) + shape) + g.standard_normal((n, K) + shape))))


def moments64(vals):
    """fp64 (mean, sd over members x draws, sd over the members' draw means) of vals [n, K, ...]."""
    v = np.asarray(vals, np.float64)
    return v.mean((0, 1)), v.reshape((-1,) + v.shape[2:]).std(0), v.mean(1).std(0)


# ---- the fp64 oracle by cohort -----------------------------------------------------------------------------------------------------------
def _nan(shape):
    return np.full(shape, np.nan)


def compose(mean_b, sd_b, obs, ids, G):
    """Per-trajectory fp64 moments [Q, B, C, T] (RU.oracle_moments) and observations [B, C, T] composed by cohort: mean = mean of the
    member means; sd^2 = mean over members of sd_b^2 + (mean_b - mean)^2; sd_subjects = np.std of the member means; obs_mean; l1."""
    Q, B, C, T = mean_b.shape
    mean, sd, sdb, om, l1 = _nan((Q, G, C, T)), _nan((Q, G, C, T)), _nan((Q, G, C, T)), _nan((G, C, T)), _nan((G, C))
    for g in range(G):
        sel = np.flatnonzero(np.asarray(ids) == g)
        if sel.size:
            mean[:, g] = mean_b[:, sel].mean(1)
            sd[:, g] = np.sqrt((sd_b[:, sel] ** 2 + (mean_b[:, sel] - mean[:, g][:, None]) ** 2).mean(1))
            sdb[:, g] = np.std(mean_b[:, sel], 1)
            om[g] = obs[sel].mean(0)
            l1[g] = np.abs(om[g] - mean[0, g]).sum(-1)
    return mean, sd, sdb, om, l1


def oracle_draws(c, is_post, eps=None):
    """[Q, ns, B, C, T] fp64: the oracle's head curves of every draw (what RU.oracle_moments reduces)."""
    ospec, p64 = c["ospec"], EU.f64(c["p"])
    obs, u, times = c["obs"].double(), c["u"].double(), c["times"].double()
    e = (c["eps"] if eps is None else eps).double()
    ns, B, L = e.shape
    with torch.no_grad():
        loc, scale = O.encoder_conv(p64, obs, ospec.pool_size) if is_post else O.prior_loc_scale(p64, ospec, u)
        mu = RU.oracle_curves(p64, ospec, (loc.unsqueeze(0) + scale.unsqueeze(0) * e).reshape(ns * B, L), times, ospec.solver)
    return mu.reshape(mu.shape[0], ns, B, mu.shape[2], mu.shape[3]).numpy()


def oracle_cohorts(c, is_post, ids, G, clip=None, eps=None):
    """(mean, sd, sd_subjects, obs_mean, l1) in fp64.  Without clipping RU.oracle_moments composed by cohort; with it the per-draw curves,
    clipped by comparison, reduced per trajectory first."""
    obs = c["obs"].double().numpy()
    if clip is None:
        mean_b, sd_b = RU.oracle_moments(c, is_post, eps)
    else:
        mu = oracle_draws(c, is_post, eps)
        mu = np.where(mu < clip, clip, mu)
        mean_b, sd_b = mu.mean(1), mu.std(1)
    return compose(mean_b, sd_b, obs, ids, G)


def obs_bar(obs, R):
    return (R + 1) * U * float(np.abs(np.asarray(obs, np.float64)).max())


def check(got, want, obs, R, tag):
    """got: the five outputs (tensors or arrays; None: not asked); want: oracle_cohorts.  Prints the worst ratios error / bar over the
    non-empty cohorts, then asserts: empty cohorts all NaN, the rest finite and within the bars."""
    g = [None if x is None else (x.detach().double().cpu().numpy() if torch.is_tensor(x) else np.asarray(x, np.float64)) for x in got]
    wmean = want[0]
    live = ~np.isnan(wmean[0, :, 0, 0])
    scale = np.maximum(1.0, np.abs(wmean[:, live]))
    bars = [MEAN_BAR * scale, SD_BAR * scale, SD_BAR * scale, np.full(want[3][live].shape, obs_bar(obs, R)),
            (MEAN_BAR * scale[0]).sum(-1) + wmean.shape[-1] * obs_bar(obs, R)]
    ratios = []
    for i, (x, w, bar) in enumerate(zip(g, want, bars)):
        if x is None:
            ratios.append(float("nan"))
            continue
        sel = (slice(None), live) if i < 3 else (live,)
        assert np.isnan(x[(slice(None), ~live) if i < 3 else (~live,)]).all(), (tag, i, "an empty cohort must be NaN")
        assert np.isfinite(x[sel]).all(), (tag, i)
        ratios.append(float((np.abs(x[sel] - w[sel]) / bar).max()) if live.any() else 0.0)
    print("%s: error / bar: mean %.3e, sd %.3e, sd_subjects %.3e, obs_mean %.3e, l1 %.3e" % ((tag,) + tuple(ratios)))
    for i, r in enumerate(ratios):
        assert not r > 1.0, (tag, ("mean", "sd", "sd_subjects", "obs_mean", "l1")[i], r)
