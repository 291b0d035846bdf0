"""What the CPU tests of the whole-curve calls' refusal programs share (tests/{attribution,summary,quantile,mechanism,band}_refusals): the
rungs of slode_recon_moments' ladder as LADDER tuples, and the check of a program's output against its LADDER, its golden file and the texts
tests/golden/eval_refusals.txt records for slode_recon_moments.  Not imported by the product."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH, POST, PRIOR, PLAN = ("post", "prior"), ("post",), ("prior",), ("plan",)
WS = ["workspace 64 B < required"]


def shared_rungs(N, pointers, advice):
    """``(head, labels, two_at_once)``: the tuples (case, call columns, status, words of the message) of the rungs every program takes from
    slode_recon_moments' ladder, written from include/slode.h in rung order, for the call ``N`` with the pointer list ``pointers`` and
    the advice ``advice`` -- ``head``: the pointers, the draw count, what the fused kernels do not take, the posterior's observations;
    ``labels``: the label tensors and the workspace; ``two_at_once``: the earlier rung speaks.  A program's own rungs stand between them."""
    null = "%s: %s is NULL" % (N, pointers)
    head = [
        ("handle NULL", BOTH, -1, ["handle is NULL"]), ("shape NULL", BOTH, -1, ["shape is NULL"]), ("layout NULL", BOTH, -1, ["layout is NULL"]),
        ("params NULL", BOTH, -1, ["params is NULL"]), ("batch NULL", BOTH, -1, [null]), ("times NULL", BOTH, -1, [null]),
        ("stage_t NULL", BOTH, -1, [null]), ("workspace NULL", BOTH, -1, [null]),
        ("bad shape", BOTH, -1, ["T out of range"]), ("num_samples 0", BOTH, -1, [N, "num_samples = 0 < 1"]),
        ("num_samples 2^30", BOTH, -1, [N, "B x num_samples", "2^30 - 1"]),
        ("adaptive method 3", BOTH, -1, [N, "adaptive solver dopri5", advice]), ("adaptive method 4", BOTH, -1, [N, "adaptive solver bosh3"]),
        ("adaptive method 5", BOTH, -1, [N, "adaptive solver fehlberg2"]), ("adaptive method 6", BOTH, -1, [N, "adaptive solver adaptive_heun"]),
        ("particles 2", BOTH, -1, [N, "particles = 2"]), ("fold_on", BOTH, -1, [N, "measured arms"]), ("ode_pack", BOTH, -1, [N, "measured arms"]),
        ("ode_alg", BOTH, -1, [N, "measured arms"]), ("obs NULL", POST, -1, [N, "batch->obs is NULL"]),
        ("padded strides", POST, -1, [N, "observation strides (266, 1, 3)", advice]),
        ("channel-major strides of another T", POST, -1, [N, "observation strides (258, 87, 1)"]), ("no_fold", POST, -1, [N, "SLODE_NO_FOLD"]),
    ]
    labels = [
        ("label columns 3, n_u 2", BOTH, -1, ["label tensors have 3 columns"]), ("n_labels 5", BOTH, -1, ["n_labels out of range"]),
        ("label tensor 1 NULL", BOTH, -1, ["label tensor 1 is NULL"]), ("no label tensors", PRIOR, -1, [N, "the prior needs the label tensors"]),
        ("workspace too small", BOTH, -3, WS),
    ]
    two_at_once = [
        ("params NULL + batch NULL", BOTH, -1, ["params is NULL"]), ("times NULL + num_samples 0", BOTH, -1, ["is NULL"]),
        ("num_samples 0 + adaptive", BOTH, -1, ["num_samples = 0"]), ("adaptive + particles 2", BOTH, -1, ["adaptive solver bosh3"]),
        ("ode_alg + obs NULL", POST, -1, ["measured arms"]),
    ]
    return head, labels, two_at_once


def golden_lines(program, tmp_path):
    """The lines the refusal program prints, checked line by line against tests/golden/<program>.txt; the last one says that the memory
    that stands for the outputs is untouched."""
    from tests.refusals_util import refusal_lines
    lines = refusal_lines(program, tmp_path)
    assert lines[-1] == "memory that stands for the outputs | untouched"
    want = open(os.path.join(ROOT, "tests", "golden", program + ".txt")).read().splitlines()
    for i, (g, w) in enumerate(zip(lines, want)):
        assert g == w, "line %d:\n  got  %s\n  want %s" % (i + 1, g, w)
    assert len(lines) == len(want)
    return lines


def recon_texts(N):
    """case -> the message tests/golden/eval_refusals.txt records for slode_recon_moments, as the call ``N`` words it: its own name, and
    its pointer list without ``mean``."""
    recon = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "eval_refusals.txt")).read().splitlines():
        parts = line.split(" | ", 4)
        if len(parts) == 5 and parts[1] == "recon_moments":
            recon[parts[0]] = parts[4].replace("slode_recon_moments", N).replace("batch / mean / ", "batch / ")
    return recon


def check_ladder(program, tmp_path, ladder, N, advice, plan_line=None, not_shared=()):
    """The program's output against its golden file and, line for line, against ``ladder``: the case and call column, the status, the words
    of the message and the untouched drawing-call counter (7: refused, and nothing drawn); a rung shared with slode_recon_moments carries
    the text recorded for it, the name, the pointer list and the advice apart.  ``plan_line(name, counter, line)``: the check of a plan
    line whose counter column shows something else (such lines are left out of what follows).  ``not_shared``: words of the case names
    that are the call's own.  Returns ``(lines, shared, figures)``: the number of shared texts and, per "LDS: ..." case, the set of byte
    figures its lines name."""
    lines = golden_lines(program, tmp_path)
    expect = [(name, col, status, words) for name, cols, status, words in ladder for col in cols]
    assert len(lines) == len(expect) + 1
    recon = recon_texts(N)
    shared, figures = 0, {}
    for line, (name, col, status, words) in zip(lines[:-1], expect):
        got_name, got_col, got_status, counter, msg = line.split(" | ", 4)
        assert (got_name, got_col) == (name, col) and int(got_status) == status, line
        for w in words:
            assert w in msg, (name, w, msg)
        if col == "plan" and plan_line is not None:
            plan_line(name, int(counter), line)
            continue
        assert counter == "7", line
        if name.startswith("LDS: "):
            figures.setdefault(name, set()).add(re.search(r"\((\d+) B", msg).group(1))
        key = name.replace("num_samples", "draws")
        if col != "plan" and key in recon and "LDS" not in name and "workspace too small" not in name and not any(w in name for w in not_shared):
            shared += 1
            assert msg == recon[key].replace("reduce recon_samples instead", advice), (name, msg, recon[key])
    print("%d lines, %d of them word for word slode_recon_moments' texts" % (len(lines), shared))
    return lines, shared, figures
