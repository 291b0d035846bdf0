"""The refusal programs of the eval-side calls (tests/<name>/<name>.cpp over tests/refusals_common.h): built and run without a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def refusal_lines(name, tmp_path):
    """The lines that tests/<name>/<name>.cpp prints: its host pass compiled against the package's libslode.so, then run.  Skips where
    hipcc is absent."""
    from structured_latent_odes_amd import _lib as L
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present: the refusal program is not built")
    lib = os.path.abspath(L.LIB_PATH)
    exe = str(tmp_path / name)
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-O1", os.path.join(ROOT, "tests", name, name + ".cpp"),
                        "-o", exe, "-x", "none", lib, "-Wl,-rpath," + os.path.dirname(lib)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()
