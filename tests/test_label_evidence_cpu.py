"""CPU tests of the label evidence: the C ABI of slode_label_evidence, its refusal ladder on a hand-filled handle
(tests/evidence_refusals/evidence_refusals.cpp), and the test infrastructure the GPU tests rest on -- the algebra the kernel relies on (only
log p(z | u) and the label terms depend on the hypothesis), the two regimes of the test inputs on the fp64 oracle, label_grid and the match
index."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import slode_oracle as O
from tests import label_evidence_util as LU
from tests import traj_bounds_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["h", "s", "lay", "params", "times", "stage_t", "batch", "num_draws", "hyp_labels", "V", "log_prior", "evidence", "best", "loss_vkb",
        "workspace", "workspace_bytes", "stream"]


def test_abi_exports_label_evidence_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    assert hasattr(lib, "slode_label_evidence") and "slode_label_evidence" in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 210
    assert int(re.search(r"#define\s+SLODE_EVIDENCE_SLOTS\s+(\d+)", hdr).group(1)) == L.EVIDENCE_SLOTS == 4
    assert int(re.search(r"#define\s+SLODE_EVIDENCE_MAX_V\s+(\d+)", hdr).group(1)) == L.EVIDENCE_MAX_V == 64
    m = re.search(r"int\s+slode_label_evidence\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    at = lib.slode_label_evidence.argtypes
    assert len(at) == len(ARGS) and at[7] is C.c_int and at[9] is C.c_int and at[15] is C.c_size_t
    doc = hdr[:hdr.index("int slode_profile_read(")]
    assert '"traj_bounds", "label_evidence"' in doc[doc.rindex("/*"):]                   # the launch name is documented at slode_profile_read
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_label_evidence(None, None, None, None, None, None, None, 0, None, 0, None, None, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


# case -> the words its message must carry, written from include/slode.h in rung order: the ladder of slode_traj_bounds, then evidence, V,
# hyp_labels, n_labels, the LDS tables; then the label tensors and the workspace (SLODE_ENOSPC = -3)
_N = "slode_label_evidence"
LADDER = [
    ("handle NULL", -1, ["handle is NULL"]), ("shape NULL", -1, ["shape is NULL"]), ("layout NULL", -1, ["layout is NULL"]),
    ("params NULL", -1, ["params is NULL"]), ("batch NULL", -1, [_N, "batch", "is NULL"]), ("times NULL", -1, [_N, "times", "is NULL"]),
    ("stage_t NULL", -1, [_N, "stage_t", "is NULL"]), ("workspace NULL", -1, [_N, "workspace", "is NULL"]), ("bad shape", -1, ["T out of range"]),
    ("draws 0", -1, [_N, "num_draws = 0 < 1"]), ("draws 2^30", -1, [_N, "B x num_draws", "2^30 - 1"]),
    ("adaptive method 3", -1, [_N, "adaptive solver dopri5"]), ("adaptive method 4", -1, [_N, "adaptive solver bosh3"]),
    ("adaptive method 5", -1, [_N, "adaptive solver fehlberg2"]), ("adaptive method 6", -1, [_N, "adaptive solver adaptive_heun"]),
    ("particles 2", -1, [_N, "particles = 2"]), ("fold_on", -1, [_N, "measured arms"]), ("ode_pack", -1, [_N, "measured arms"]),
    ("ode_alg", -1, [_N, "measured arms"]), ("obs NULL", -1, [_N, "batch->obs is NULL"]), ("padded strides", -1, [_N, "observation strides (266, 1, 3)"]),
    ("channel-major strides of another T", -1, [_N, "observation strides (258, 87, 1)"]), ("no_fold", -1, [_N, "SLODE_NO_FOLD"]),
    ("evidence NULL", -1, [_N, "evidence is NULL"]), ("unaligned evidence", -1, [_N, "16-byte aligned"]), ("V 0", -1, [_N, "V = 0", "[1, 64]"]),
    ("V -1", -1, [_N, "V = -1"]), ("V 65", -1, [_N, "V = 65", "[1, 64]"]), ("hyp_labels NULL", -1, [_N, "hyp_labels is NULL"]),
    ("every hyp tensor NULL", -1, [_N, "every entry of hyp_labels is NULL"]), ("n_labels 0", -1, [_N, "n_labels is 0"]),
    ("LDS: num_draws 2000, V 64", -1, [_N, "LDS tables", "num_draws = 2000", "V = 64", "163840"]),
    ("LDS: num_draws 100000, V 1", -1, [_N, "LDS tables", "num_draws = 100000", "V = 1 "]),
    ("LDS: num_draws 2^24, V 64", -1, [_N, "LDS tables", "num_draws = 16777216", "V = 64"]),
    ("label columns 3, n_u 2", -1, ["label tensors have 3 columns"]), ("n_labels 5", -1, ["n_labels out of range"]),
    ("label tensor 1 NULL", -1, ["label tensor 1 is NULL"]), ("workspace too small", -3, ["workspace 64 B < required"]),
    ("one hyp tensor NULL; workspace too small", -3, ["workspace 64 B < required"]),
    # two conditions at once: the earlier rung speaks
    ("params NULL + batch NULL", -1, ["params is NULL"]), ("times NULL + draws 0", -1, ["is NULL"]), ("draws 0 + adaptive", -1, ["num_draws = 0"]),
    ("draws 2^30 + adaptive", -1, ["2^30 - 1"]), ("adaptive + particles 2", -1, ["adaptive solver bosh3"]), ("particles 2 + fold_on", -1, ["particles = 2"]),
    ("ode_alg + obs NULL", -1, ["measured arms"]), ("obs NULL + padded strides", -1, ["batch->obs is NULL"]),
    ("no_fold + evidence NULL", -1, ["observation strides"]), ("draws 0 + unaligned evidence", -1, ["num_draws = 0"]),
    ("unaligned evidence + V 0", -1, ["16-byte aligned"]), ("V 65 + hyp_labels NULL", -1, ["V = 65"]), ("hyp_labels NULL + n_labels 0", -1, ["hyp_labels is NULL"]),
    ("every hyp tensor NULL + LDS", -1, ["every entry of hyp_labels is NULL"]), ("LDS + label columns 3", -1, ["LDS tables"]),
    ("label columns 3 + workspace too small", -1, ["label tensors have 3 columns"]),
]


def test_label_evidence_refusals_on_a_hand_filled_handle(tmp_path):
    """Every refusing configuration of slode_label_evidence without a device, in rung order: status, the words of the message and the
    untouched drawing-call counter against LADDER; line by line against tests/golden/evidence_refusals.txt; the shared rungs carry the texts
    tests/golden/eval_refusals.txt records for slode_traj_bounds, the call's name (and, in the list of required pointers, ``bounds``) apart;
    and the memory that stands for the outputs untouched."""
    from tests.refusals_util import refusal_lines
    lines = refusal_lines("evidence_refusals", tmp_path)
    assert lines[-1] == "memory that stands for the outputs | untouched"
    want = open(os.path.join(ROOT, "tests", "golden", "evidence_refusals.txt")).read().splitlines()
    for i, (g, w) in enumerate(zip(lines, want)):
        assert g == w, "line %d:\n  got  %s\n  want %s" % (i + 1, g, w)
    assert len(lines) == len(want) == len(LADDER) + 1
    bounds = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "eval_refusals.txt")).read().splitlines():
        parts = line.split(" | ", 4)
        if len(parts) == 5 and parts[1] == "traj_bounds":
            bounds[parts[0]] = parts[4]
    shared = 0
    for line, (name, status, words) in zip(lines[:-1], LADDER):
        got_name, got_status, counter, msg = line.split(" | ", 3)
        assert got_name == name and int(got_status) == status and counter == "7", line      # refused, and nothing drawn
        for w in words:
            assert w in msg, (name, w, msg)
        if name in bounds and "LDS" not in name and "workspace too small" not in name:
            shared += 1
            assert msg == bounds[name].replace("slode_traj_bounds", _N).replace("batch / bounds / ", "batch / "), (name, msg, bounds[name])
    assert shared >= 30


CASES = {"cvs_ald": LU.binary_grid, "challenge_gauss": LU.binary_grid, "proc_gauss": LU.batch_rows}
_ORACLE = {}


def _oracle(case):
    """B = 6, K = 8, noise x 1e-3, rk4: computed once per case, shared, left unchanged."""
    if case not in _ORACLE:
        c = TU.build(case, "rk4", B=6, K=8)
        tabs = CASES[case](c)
        _ORACLE[case] = (c, tabs, LU.oracle(c, tabs, eps=1e-3 * c["eps"]))
    return _ORACLE[case]


@pytest.mark.parametrize("case", list(CASES))
def test_only_the_prior_and_the_label_terms_depend_on_the_hypothesis(case):
    """On the fp64 oracle: the nll part is identical across hypotheses, and loss_v - loss_v' equals the difference of log p(z | u) (plus the
    46 x label terms for proc), to 1e-12 relative to the term magnitudes."""
    from torch.distributions import Normal
    c, tabs, o = _oracle(case)
    assert np.array_equal(o["nll"], np.broadcast_to(o["nll"][:1], o["nll"].shape))
    ospec, p = c["ospec"], {k: v.double() for k, v in c["p"].items()}
    e = (1e-3 * c["eps"]).double()
    with torch.no_grad():
        loc, scale = O.encoder_conv(p, c["obs"].double(), ospec.pool_size)
        z = loc.unsqueeze(0) + scale.unsqueeze(0) * e
        part = []
        for v in range(o["loss"].shape[0]):
            u = LU.substituted(c, tabs, v).double()
            ploc, pscale = O.prior_loc_scale(p, ospec, u)
            t = -Normal(ploc, pscale).log_prob(z).sum(-1)
            if ospec.labels_in_main:
                t = t - torch.stack([torch.stack([ospec.aux_mult * O._label_terms(p, ospec, z[k, b:b + 1], u[b:b + 1]) for b in range(c["B"])])
                                     for k in range(z.shape[0])]).reshape(t.shape)
            part.append(t.numpy())
    part = np.stack(part)
    for v in range(1, len(part)):
        got, want = o["loss"][v] - o["loss"][0], part[v] - part[0]
        assert np.all(np.abs(got - want) <= 1e-12 * (o["mag"][v] + o["mag"][0])), (case, v, np.abs(got - want).max())


def test_cvs_posteriors_are_spread_over_the_hypotheses():
    """cvs_ald, {0, 1}^2: the importance-weighted bounds of a row lie 1.9 - 3.0 nat apart and every row has at least two hypotheses with
    posterior above 0.03 -- the normalisation is exercised."""
    _, _, o = _oracle("cvs_ald")
    _, iw, ess, post, _ = LU.reduce64(o["loss"])
    spread = iw.max(1) - iw.min(1)
    print("cvs_ald: spread %s, posterior %.3f .. %.3f" % (np.round(spread, 2), np.exp(post).min(), np.exp(post).max()))
    assert np.all((np.exp(post) > 0.03).sum(axis=1) >= 2)
    assert np.all(spread > 1.0) and np.all(spread < 5.0)
    assert np.allclose(np.exp(post).sum(axis=1), 1.0, atol=1e-12)
    assert np.all(ess >= 1.0) and np.all(ess <= 8.0)


def test_challenge_posteriors_are_concentrated_but_nowhere_zero():
    _, _, o = _oracle("challenge_gauss")
    _, iw, _, post, _ = LU.reduce64(o["loss"])
    spread = iw.max(1) - iw.min(1)
    print("challenge_gauss: spread %s" % np.round(spread, 2))
    assert np.all(spread > 10.0) and np.all(spread < 20.0) and np.all(np.exp(post) > 0.0)


def test_proc_posteriors_are_one_hot_and_stay_finite():
    """proc_gauss, the first four label rows of the batch as hypotheses: the bounds of a row lie 1370 - 2440 nat apart, so exp underflows
    for every hypothesis but the best -- log_post stays finite (no -inf, no NaN) and its maximum, the arg-max's value, is 0 in fp64; rows 0-3
    find their own labels."""
    _, _, o = _oracle("proc_gauss")
    _, iw, _, post, best = LU.reduce64(o["loss"])
    spread = iw.max(1) - iw.min(1)
    print("proc_gauss: spread %s, best %s" % (np.round(spread, 1), best))
    assert np.all(spread > 1000.0)
    assert np.isfinite(post).all() and np.all(post.max(axis=1) == 0.0) and np.all(post[np.arange(len(best)), best] == 0.0)
    assert np.all(np.sort(np.exp(post), axis=1)[:, :-1] < 1e-100)                      # one-hot far below any fp32 value
    assert best[0] == 0


def test_label_grid_and_the_match_index():
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel as Cvs
    from structured_latent_odes_amd.models.mechanistic_proc import MechanisticModel as Proc
    g = Cvs.label_grid(iext=[0, 1], rtpr=[0, 1])
    assert list(g) == ["iext", "rtpr"] and all(tuple(t.shape) == (4, 1) and t.dtype == torch.float32 for t in g.values())
    assert g["iext"].flatten().tolist() == [0, 0, 1, 1] and g["rtpr"].flatten().tolist() == [0, 1, 0, 1]
    assert tuple(Cvs.label_grid(iext=[0, 1, 2])["iext"].shape) == (3, 1)
    p = Proc.label_grid(aR=torch.eye(3), aS=torch.eye(4))
    assert tuple(p["aR"].shape) == (12, 3) and tuple(p["aS"].shape) == (12, 4)
    assert torch.equal(p["aR"][4], torch.tensor([0.0, 1.0, 0.0])) and torch.equal(p["aS"][4], torch.tensor([1.0, 0.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="not a label"):
        Cvs.label_grid(aR=[0, 1])
    with pytest.raises(ValueError):
        Cvs.label_grid()
    # match: hand-made labels; a subject whose labels are no hypothesis -> -1; an unnamed label is not compared
    iext = torch.tensor([[0.0], [1.0], [1.0], [0.5], [0.0]])
    rtpr = torch.tensor([[1.0], [1.0], [0.0], [0.0], [2.0]])
    assert Cvs.hypothesis_match(g, iext=iext, rtpr=rtpr).tolist() == [1, 3, 2, -1, -1]
    assert Cvs.hypothesis_match({"iext": g["iext"]}, iext=iext, rtpr=rtpr).tolist() == [0, 2, 2, -1, 0]       # first match on a tie
    aR = torch.eye(3)[[2, 0]]
    aS = torch.eye(4)[[3, 1]]
    assert Proc.hypothesis_match(p, aR=aR, aS=aS).tolist() == [11, 1]
    with pytest.raises(ValueError, match="same V"):
        Cvs.hypothesis_match({"iext": g["iext"], "rtpr": g["rtpr"][:2]}, iext=iext, rtpr=rtpr)
    with pytest.raises(ValueError, match=r"\[V, 1\]"):
        Cvs.hypothesis_match({"iext": torch.zeros(2, 2)}, iext=iext, rtpr=rtpr)
    with pytest.raises(ValueError, match="at least one label"):
        Cvs.hypothesis_match({}, iext=iext, rtpr=rtpr)


def test_the_printed_line():
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel as Cvs
    post = np.zeros((3, 2, 4), np.float32)
    post[:, :, 2] = [[1.5, 2.0], [3.0, 1.0], [2.0, 2.0]]
    post[:, :, 3] = np.log([[0.25, 0.75], [0.5, 0.5], [0.9, 0.1]])
    line = Cvs.label_evidence_line(post, np.array([1, 0, 0]), np.array([1, 1, -1]))
    assert line == "label_evidence: V=2  matched=2/3  best==match=0.5000  mean_post_at_match=0.6250  median_ess_at_match=1.50"
    assert "no subject" in Cvs.label_evidence_line(post, np.array([1, 0, 0]), np.array([-1, -1, -1]))
