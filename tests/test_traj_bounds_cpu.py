"""CPU tests of the per-trajectory bounds: the C ABI of slode_traj_bounds, and the test infrastructure the GPU tests rest on -- the per-row
oracle of tests/traj_bounds_util.py against the batch-summed oracle, the reachability of the per-row bar in fp32, and the noise scale at
which the importance weights are not degenerate."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import slode_oracle as O
from tests import eval_stats_util as EU
from tests import traj_bounds_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_traj_bounds_as_documented():
    from structured_latent_odes_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    lib = L.load()
    assert hasattr(lib, "slode_traj_bounds") and "slode_traj_bounds" in L.EXPORTS
    assert int(re.search(r"#define\s+SLODE_VERSION\s+(\d+)", hdr).group(1)) == lib.slode_version() >= 160
    assert int(re.search(r"#define\s+SLODE_BOUND_SLOTS\s+(\d+)", hdr).group(1)) == L.BOUND_SLOTS == 4
    m = re.search(r"int\s+slode_traj_bounds\s*\(([^;]*)\)\s*;", hdr)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "s", "lay", "params", "times", "stage_t", "batch", "num_draws", "bounds", "loss_kb",
                                                         "workspace", "workspace_bytes", "stream"]
    at = lib.slode_traj_bounds.argtypes
    assert len(at) == len(args) and at[7] is C.c_int and at[11] is C.c_size_t
    # host-side refusals need no device: a NULL handle is refused before anything else
    assert lib.slode_traj_bounds(None, None, None, None, None, None, None, 0, None, None, None, 0, None) == -1
    assert b"handle is NULL" in lib.slode_last_error(None)


@pytest.mark.parametrize("case", list(EU.CASES))
def test_rows_of_the_per_row_oracle_sum_to_the_batch_oracle(case):
    """The main loss is separable over rows: for every draw, sum_b loss[k, b] == O.main_loss on the batch, to 1e-12 relative in fp64."""
    c = TU.build(case, "midpoint", K=2)
    rows = TU.oracle_rows(c)
    p64 = EU.f64(c["p"])
    for k in range(c["K"]):
        with torch.no_grad():
            want = O.main_loss(p64, c["ospec"], c["obs"].double(), c["u"].double(), c["eps"][k].double(), c["times"].double()).item()
        got = float(rows["loss"][k].sum())
        assert abs(got - want) <= 1e-12 * abs(want), (case, k, got, want)
    assert np.all(rows["mag"] > 0) and rows["loss"].shape == rows["nll"].shape == (2, c["B"])


@pytest.mark.parametrize("case", ["cvs_ald", "proc_gauss", "proc_ald", "challenge_gauss"])
def test_the_per_row_bar_is_reachable_in_fp32(case):
    """The same per-row oracle evaluated in fp32 stays well inside bar = 1e-5 x term magnitudes of the fp64 one (rk4, K = 4, first 5
    rows): measured 0.02 .. 0.22 of the bar; asserted at half of it."""
    c = TU.build(case, "rk4", K=4)
    rows = slice(0, 5)
    w64, w32 = TU.oracle_rows(c, rows=rows), TU.oracle_rows(c, rows=rows, dtype=torch.float32)
    ratio = float((np.abs(w32["loss"] - w64["loss"]) / (TU.REL * w64["mag"])).max())
    print("%s: fp32 oracle error / bar %.3f" % (case, ratio))
    assert ratio <= 0.5, (case, ratio)


@pytest.mark.parametrize("case", ["cvs_ald", "challenge_gauss"])
def test_noise_scaled_by_1e_3_gives_non_degenerate_weights(case):
    """Raw N(0, 1) noise: the per-draw losses are thousands of nats apart and the ESS is 1.00 on every row.  Noise x 1e-3, K = 8, first 6
    rows: at least half of the rows have 1.5 < ESS < 7.5 -- the scaling the GPU tests of the reduction use."""
    c = TU.build(case, "rk4", K=8)
    rows = slice(0, 6)
    raw = TU.reduce64(TU.oracle_rows(c, rows=rows)["loss"])[2]
    ess = TU.reduce64(TU.oracle_rows(c, eps=1e-3 * c["eps"], rows=rows)["loss"])[2]
    print("%s: ESS raw %s, noise x 1e-3 %s" % (case, np.round(raw, 2), np.round(ess, 2)))
    assert np.all(raw < 1.01)
    assert np.sum((ess > 1.5) & (ess < 7.5)) >= 3
    assert np.all(ess >= 1.0) and np.all(ess <= 8.0)
