"""CPU tests of csrc/ode_select.h, the one place that decides which ode_elbo_kernel instantiation a launch takes, with what grid, block
and dynamic LDS: the header compiled for the host (tests/ode_select/ode_select.cpp) and asked about a sweep of launch
descriptions -- the five named shapes, off-list and unsupported ones, a proc split whose cold ranges do not fit, grids beyond the
generic caps, forward / backward, grid == B and grid < B, every handle flag, external solutions, both gradient modes, B = 12 / 13, one and
two particles, a label head wider than 16 latent dims.

tests/golden/ode_select_table.txt holds, for every row of the sweep (each distinct answer once, with the numbers of its rows), what the
launcher did BEFORE the selection was a function of its
own: a copy of that launcher whose launch_one printed its template arguments, grid, threads and LDS bytes instead of launching, and whose
refusals printed their text, was run over these same rows.  ode_select must reproduce every line."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "ode_select_table.txt")
EULER, MIDPOINT, RK4 = 0, 1, 2
LDS_MAX = 160 * 1024

# name -> S H T C L likelihood method Hc family zg head0 (the program's header explains the last three)
SHAPES = {
    "metric":        (5, 25, 200, 3, 8, 0, RK4, 50, 1, 3, 0),
    "c0":            (5, 25, 100, 3, 4, 0, RK4, 50, 1, 1, 0),
    "c2":            (8, 25, 100, 4, 50, 0, RK4, 50, 2, 10, 0),
    "c4":            (5, 25, 300, 4, 15, 1, RK4, 50, 1, 5, 0),
    "ref_default":   (5, 25, 86, 3, 15, 0, MIDPOINT, 50, 1, 5, 0),
    "off_list_5":    (5, 25, 120, 3, 8, 0, RK4, 50, 1, 3, 0),
    "off_list_8":    (8, 25, 64, 4, 50, 0, RK4, 50, 2, 10, 0),
    "S_6":           (6, 25, 100, 3, 8, 0, RK4, 50, 1, 3, 0),                   # no instantiation for this (S, H)
    "H_20":          (5, 20, 100, 3, 8, 0, RK4, 50, 1, 3, 0),
    "c2_wide_split": (8, 25, 100, 4, 50, 0, RK4, 50, 2, 12, 0),                 # the cold ranges do not fit the work block
    "c2_euler":      (8, 25, 100, 4, 50, 0, EULER, 50, 2, 10, 0),               # with an external solution: the scorer
    "c2_euler_h20":  (8, 25, 100, 4, 50, 0, EULER, 50, 2, 10, 20),              # a label head of 20 latent dims: not the scorer
    "T_600":         (5, 25, 600, 3, 8, 0, RK4, 50, 1, 3, 0),                   # beyond the looped generic kernel's 512 threads
    "T_780_S_8":     (8, 25, 780, 4, 8, 0, EULER, 50, 0, 0, 0),                 # beyond S = 8's 768
    "T_1000_S_8":    (8, 25, 1000, 4, 8, 0, RK4, 50, 0, 0, 0),                  # beyond 160 KiB
    "metric_Hc_60":  (5, 25, 200, 3, 8, 0, RK4, 60, 1, 3, 0),                   # no fused encoder forward beyond Hc = 52
}
EXT_TOO = ("c2", "c2_wide_split", "c2_euler", "c2_euler_h20", "off_list_8")     # also scored with an external solution


def _row(shape, B=12, grid_full=1, bwd=1, ra=0, with_ll=1, loop=0, generic=0, alg=0, pack=0, encf=0, ext=0, particles=1):
    S, H, T, C, L, lik, method, Hc, fam, zg, head0 = SHAPES[shape]
    return (S, H, T, C, L, lik, method, B, B if grid_full else 4, bwd, ra, with_ll, loop, generic, alg, pack, encf, ext, particles, Hc, fam, zg, head0)


def sweep():
    rows = []
    modes = ((0, 0), (1, 0), (1, 1))                                            # (backward, reference_adjoint)
    for bwd, ra in modes:
        for full in (1, 0):
            for B in (12, 13):
                for alg in (0, 1, 2, 7):
                    for pack in (0, 4, 12, 14):
                        for encf in (0, 1):
                            for loop, generic in ((0, 0), (1, 0), (0, 1)):
                                rows.append(_row("metric", B, full, bwd, ra, 1, loop, generic, alg, pack, encf))
                for alg in (0, 1):
                    for pack in (0, 4, 12):
                        for encf in (0, 1):
                            rows.append(_row("metric", B, full, bwd, ra, alg=alg, pack=pack, encf=encf, ext=1))
                            rows.append(_row("metric", B, full, bwd, ra, alg=alg, pack=pack, encf=encf, particles=2))
    for shape in SHAPES:
        if shape == "metric":
            continue
        for ext in ((0, 1) if shape in EXT_TOO else (0,)):
            for bwd, ra in modes:
                for full in (1, 0):
                    for generic in (0, 1):
                        for pack in (0, 4):
                            for encf in (0, 1):
                                rows.append(_row(shape, 12, full, bwd, ra, 1, 0, generic, 0, pack, encf, ext))
                        rows.append(_row(shape, 12, full, bwd, ra, generic=generic, alg=1, ext=ext))
                    rows.append(_row(shape, 12, full, bwd, ra, loop=1, ext=ext))
                    rows.append(_row(shape, 13, full, bwd, ra, ext=ext))
                    rows.append(_row(shape, 12, full, bwd, ra, with_ll=0, ext=ext))
                    rows.append(_row(shape, 12, full, bwd, ra, alg=7, ext=ext))
                    rows.append(_row(shape, 12, full, bwd, ra, particles=2, ext=ext))
    return [" ".join(str(x) for x in r) for r in rows]


ROWS = sweep()


def _build(tmp, *flags):
    from structured_latent_odes_amd import _lib as L
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present: the host program is not built")
    lib = os.path.abspath(L.LIB_PATH)                                           # (slode_layout_init: the canonical layout of a shape)
    exe = str(tmp / "ode_select")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-O1", *flags, os.path.join(ROOT, "tests", "ode_select", "ode_select.cpp"),
                        "-o", exe, "-x", "none", lib, "-Wl,-rpath," + os.path.dirname(lib)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _ask(exe, lines, env=None):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """(the program's answer to every row of the sweep, the number of instantiations ode_dispatch names)"""
    exe = _build(tmp_path_factory.mktemp("ode_select"))
    out = _ask(exe, ROWS + ["mapped"])
    return out[:-1], int(out[-1])


def _selected(answers):
    """(request, variant: 17 ints, [carved, bound], dispatched: 14 ints) of the rows that select a kernel"""
    for req, ans in zip(ROWS, answers[0]):
        if not ans.startswith("refused: "):
            v, lay, disp = ([int(x) for x in part.split()] for part in ans.split("|"))
            assert len(v) == 17 and len(lay) == 2 and len(disp) == 14, ans
            yield req, v, lay, disp


def test_selection_reproduces_the_recorded_launcher(answers):
    """Every row of the sweep: the variant (template arguments, grid, threads, LDS bytes) or the refusal text the launcher gave before."""
    want = [None] * len(ROWS)
    for ln in open(TABLE):                                                      # <answer> | <the rows of the sweep that got it: i or i-j, ...>
        answer, rows = ln.rstrip("\n").split(" | ")
        for r in rows.split(","):
            lo, hi = (int(x) for x in (r.split("-") if "-" in r else (r, r)))
            assert want[lo:hi + 1] == [None] * (hi + 1 - lo)                    # no row twice, none beyond the sweep
            want[lo:hi + 1] = [answer] * (hi + 1 - lo)
    assert None not in want and 2000 <= len(ROWS) <= 5000                       # the table is the table of this sweep
    got = [a.split(" | ")[0] for a in answers[0]]
    bad = [(r, w, g) for r, w, g in zip(ROWS, want, got) if w != g]
    assert not bad, bad[:5]
    texts = {re.sub(r"\d+", "#", w) for w in want if w.startswith("refused: ")}
    assert len(texts) == 7, texts                                               # LDS, block size (two forms), arm shape, unknown arm, fused encoder, (S, H)


def test_lds_bytes_are_what_the_instantiation_carves(answers):
    """The layout invariant: the dynamic LDS of every selected launch is exactly what its instantiation lays out -- its own LdsMap for each
    of its PK trajectories, the tanh rows of ENCF, the arrival counters of SOFTB -- within 160 KiB, and the block within the size the
    instantiation declares; ode_dispatch names the instantiation the variant describes."""
    n = 0
    for req, v, (carved, bound), disp in _selected(answers):
        assert v[16] == carved, (req, v, carved)
        assert v[16] <= LDS_MAX and v[15] <= bound, (req, v, bound)
        assert v[:14] == disp, (req, v, disp)
        n += 1
    assert n > 1000


def _mangled_args(name):
    """the fourteen template arguments inside a mangled ode_elbo_kernel name: ...ode_elbo_kernelILi5ELi25ELb1E...Lin1E...EE"""
    args = re.findall(r"L([ib])(n?)(\d+)E", name.split("ode_elbo_kernelI", 1)[1].split("EEv", 1)[0] + "E")
    return tuple(-int(d) if neg else int(d) for _, neg, d in args)


def test_every_instantiation_is_reached_and_nothing_else_exists(answers):
    """Coverage: the sweep reaches 47 distinct instantiations, ode_dispatch names exactly 47, and -- where the library was built here, so
    that its resource remarks exist -- the object holds exactly those 47 kernels."""
    reached = {tuple(v[:14]) for _, v, _, _ in _selected(answers)}
    assert len(reached) == 47 and answers[1] == 47
    res = os.path.join(ROOT, "structured_latent_odes_amd", "csrc", "ode_kernel.res")
    if os.path.exists(res):
        names = set(re.findall(r"Function Name: (\S*ode_elbo_kernel\S*)", open(res).read()))
        assert len(names) == 47
        assert {_mangled_args(n) for n in names} == reached


def test_sweep_runs_clean_under_the_host_sanitizers(answers, tmp_path):
    """The same program with AddressSanitizer and UBSan in its host code (a stand-alone program; the library it links for
    slode_layout_init is not instrumented): the whole sweep, no report, the same answers."""
    exe = _build(tmp_path, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g")
    out = _ask(exe, ROWS + ["mapped"])
    assert out[:-1] == answers[0] and int(out[-1]) == answers[1]
