"""Host-side logic that needs no GPU: the C ABI library loads and exports every symbol include/slode.h declares, the
parameter layout, loud failure without a device, state_dict compatibility of the mirrored modules.  (No compute calls.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from structured_latent_odes_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slode.h")).read()
    declared = sorted(set(re.findall(r"\b(slode_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) >= 16
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), "libslode.so does not export %s" % name
    assert sorted(_lib.EXPORTS) == declared


def _shape(**kw):
    from structured_latent_odes_amd import _lib as L
    d = dict(B=4, T=200, C=3, L=8, S=5, H=25, F=10, K=10, P=5, Hc=50, n_u=2, n_groups=2, method=L.RK4, likelihood=L.ALD,
             quantile_diff=0.475, rtol=1e-7, atol=1e-9)
    d.update(kw)
    s = L.Shape(**d)
    s.groups[0] = L.Group(0, 3, 0, 1)
    s.groups[1] = L.Group(3, 3, 1, 1)
    return s


def test_layout_matches_hand_count_and_rejects_bad_shapes():
    from structured_latent_odes_amd import _lib as L
    lib = L.load()
    lay = L.Layout()
    assert lib.slode_layout_init(C.byref(_shape()), C.byref(lay)) == 0
    # C1 has 96,462 parameters of which 2 x 126 belong to the auxiliary classifiers (not in the hot-path layout)
    assert lay.n_params == 96462 - 252
    assert lay.lin_w == 310 and lay.lin_b == 310 + 50 * 1870 and lay.ode_end == lay.n_params
    assert lib.slode_num_stage_times(C.byref(_shape())) == 3 * 199 + 1
    for bad in (dict(T=1), dict(C=5), dict(S=9), dict(L=65), dict(T=12), dict(method=7), dict(n_groups=5)):
        assert lib.slode_layout_init(C.byref(_shape(**bad)), C.byref(lay)) == -1, bad
        assert lib.slode_last_error(None)
    s = _shape()
    s.groups[1] = L.Group(2, 3, 1, 1)          # overlaps group 0
    assert lib.slode_layout_init(C.byref(s), C.byref(lay)) == -1


def test_workspace_accounts_for_the_dopri5_step_records():
    """slode_workspace_bytes (host arithmetic, no device needed): the adaptive solver's training path needs, on top of the fixed-grid
    workspace, the solution and dLoss/dx ([B,T,S] each), two [B,L] latent buffers, the per-trajectory step counts and the accepted-step
    records [kmax][B][S+2] with kmax = 2^26 / (B*(S+2)) clamped to [64, 2048], the [B][2][H][4S] running sums parked at the hidden
    units' switching times and the forward kernel's set-up tables per sixteen trajectories (include/slode.h)."""
    from structured_latent_odes_amd import _lib as L
    lib = L.load()
    lib.slode_workspace_bytes.restype = C.c_size_t
    for B in (70, 1024, 65536):
        fixed = lib.slode_workspace_bytes(None, C.byref(_shape(B=B, method=L.EULER)))
        adaptive = lib.slode_workspace_bytes(None, C.byref(_shape(B=B, method=L.DOPRI5)))
        s = _shape(B=B)
        kmax = max(64, min(2048, (1 << 26) // (B * (s.S + 2))))
        tabf = (32 + 25 * 16 + 16 * 32 * 5 + 16 * 26 * 8 * 4) + 16 * 32       # the forward kernel's tables of sixteen trajectories, handed to the reverse sweep
        need = 4 * (2 * B * s.T * s.S + 2 * B * s.L + B + kmax * B * (s.S + 2) + 2 * B * s.H * 4 * s.S   # (snapshots: one set per lane group of the reverse sweep)
                    + ((B + 15) // 16) * tabf)
        assert fixed > 0 and adaptive >= fixed + need, (B, fixed, adaptive, need)
        assert adaptive <= fixed + need + 4 * (64 * 8 + ((B + 15) // 16) * 8192), (B, fixed, adaptive, need)   # + alignment and slab rows


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
def test_no_cpu_fallback():
    from structured_latent_odes_amd import _lib as L, engine as E
    lib = L.load()
    h = C.c_void_p()
    assert lib.slode_create(C.byref(h), 0) == -2          # SLODE_EHIP: no HIP device, and no CPU backend to fall back to
    assert b"no CPU fallback" in lib.slode_last_error(None)
    with pytest.raises(L.SlodeError):
        E.Engine(E.cvs_spec(), 86)
    from structured_latent_odes_amd.configs import load_config_cvs
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    m = MechanisticModel(load_config_cvs(), torch.device("cpu"), torch.arange(0.0, 86.0))
    with pytest.raises(L.SlodeError):
        m.recon(observations=torch.zeros(2, 3, 86), iext=torch.zeros(2, 1), rtpr=torch.zeros(2, 1), is_post=True)


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from structured_latent_odes_amd import _lib as L
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(L.SlodeError):
        L.load()


def test_state_dict_keys_and_counts_match_the_reference(golden_dir):
    from structured_latent_odes_amd.configs import load_config_challenge, load_config_cvs, load_config_proc
    from structured_latent_odes_amd.models.mechanistic_challenge import MechanisticModel as MC
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.models.mechanistic_cvs_Gauss import MechanisticModelGauss
    from structured_latent_odes_amd.models.mechanistic_proc import MechanisticModel as MP
    m = MechanisticModel(load_config_cvs(), torch.device("cpu"), torch.arange(0.0, 86.0))
    assert sum(p.numel() for p in m.parameters()) == 40300                   # SURVEY 8(a) hand count
    sd = m.state_dict()
    g3 = np.load(os.path.join(golden_dir, "g3_dynamics.npz"))
    ref = sorted(k[len("d2.p."):] for k in g3.files if k.startswith("d2.p."))
    assert sorted(k for k in sd if k.startswith("decoder.ode_model.")) == ref  # incl. the aliased prod.* / degr.* keys
    assert sd["decoder.ode_model.dynamics.prod.0.weight"].data_ptr() == sd["decoder.ode_model.dynamics.dynamics_hidden.weight"].data_ptr()
    g1 = np.load(os.path.join(golden_dir, "g1_encoder_conv.npz"))
    assert sorted(k for k in sd if k.startswith("encoder.")) == sorted("encoder." + k[len("c0.p."):] for k in g1.files if k.startswith("c0.p."))
    g2 = np.load(os.path.join(golden_dir, "g2_encoder_mlp.npz"))
    assert sorted(k[len("q_iext_given_z_iext."):] for k in sd if k.startswith("q_iext_given_z_iext.")) == sorted(
        k[len("sig.p."):] for k in g2.files if k.startswith("sig.p."))
    assert sorted(k[len("p_z_iext_given_iext."):] for k in sd if k.startswith("p_z_iext_given_iext.")) == sorted(
        k[len("prior1.p."):] for k in g2.files if k.startswith("prior1.p."))
    g4 = np.load(os.path.join(golden_dir, "g4_decoders.npz"))
    dec_ref = sorted(k[len("ald.p."):] for k in g4.files if k.startswith("ald.p.") and "ode_model" not in k)
    assert sorted(k for k in sd if k.startswith("decoder.") and "ode_model" not in k) == dec_ref
    mg = MechanisticModelGauss(load_config_cvs(), torch.device("cpu"), torch.arange(0.0, 86.0))
    assert "decoder.output_mean.0.weight" in mg.state_dict()
    mp = MP(load_config_proc(), torch.device("cpu"), torch.arange(0.0, 86.0))
    assert {"constant_std_C_12", "constant_std_C_6", "q_C12_given_z_C12.sequential_mlp.3.0.0.weight"} <= set(mp.state_dict())
    assert mp.latent_dim == 50 and mp.model_spec().n_u == 9
    mc = MC(load_config_challenge(), torch.device("cpu"), torch.arange(0.0, 142.0))
    assert mc.model_spec().prior_groups[0].z_dim == 10 and mc.labels_to_u(symptoms=torch.ones(2, 1), shedding=torch.zeros(2, 1)).tolist() == [[1.0, 0.0]] * 2
    # load_state_dict round trip (best-model copy, training_cvs.py:330)
    m2 = MechanisticModel(load_config_cvs(), torch.device("cpu"), torch.arange(0.0, 86.0))
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_synthetic_batches_have_the_reference_layouts():
    from structured_latent_odes_amd.synthetic import synthetic_batch
    obs, labels, times = synthetic_batch("cvs", 8, 200, 3)
    assert obs.shape == (8, 3, 200) and obs.stride() == (600, 1, 3) and set(labels) == {"iext", "rtpr"}
    assert float(obs.min()) >= 0 and float(obs.max()) <= 1 and times.shape == (200,)
    obs, labels, times = synthetic_batch("proc", 4, 100, 4)
    assert obs.is_contiguous() and labels["aR"].sum(1).tolist() == [1.0] * 4 and float((times[1:] - times[:-1]).min()) > 0.19


def test_no_kernel_spills_or_parks_registers():
    """The build policy behind DESIGN 3.1 (a compiler-placed spill store under the wrong EXEC mask produced wrong gradients in round 1):
    every kernel of libslode.so fits its register budget -- no VGPR spills, no AGPR parking -- according to the compiler's own resource
    remarks kept next to the objects (the Makefile gates the link on the same check)."""
    import glob
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not glob.glob(os.path.join(root, "structured_latent_odes_amd", "csrc", "*.res")):
        pytest.skip("no compiler remarks next to the objects (library built elsewhere)")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_spills.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "no VGPR spills, no AGPR parking" in r.stdout


def test_clock_tools_find_their_anchors_in_the_dopri5_source():
    """tools/dp5_fwd_clk_build.py and tools/dp5_clk_build.py put cycle stamps into dopri5_kernel.hip by replacing lines of its text: every
    such line must still be in the source (the patch step asserts each one and needs no compiler), and the build step must take its
    sources and flags from csrc/Makefile -- a hand-kept list went stale without anybody noticing."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import dp5_clk_build
        import dp5_fwd_clk_build
    finally:
        sys.path.pop(0)
    src = dp5_clk_build.kernel_source()
    for tool, stamps in ((dp5_fwd_clk_build, ("CLK(8)", "acc[5] += c1 - c0", "dp5fwd lpt %d wg %d")), (dp5_clk_build, ("CLK();", "dp5bwd wg %d K %d"))):
        text = tool.patched_source()
        assert len(text) > len(src) and all(s in text and s not in src for s in stamps), tool.__name__
    _, flags, srcs = dp5_clk_build.makefile_build()
    mk = open(os.path.join(root, "structured_latent_odes_amd", "csrc", "Makefile")).read()
    assert dp5_clk_build.KERNEL in srcs and all(f in mk for f in srcs) and "--offload-arch=gfx950" in flags and "-ffp-contract=on" in flags
    assert sorted(srcs) == sorted(f for f in os.listdir(os.path.join(root, "structured_latent_odes_amd", "csrc")) if f.endswith(".hip") and not f.startswith("_"))


def test_chain_hand_off_is_write_through_in_the_isa():
    """enc_chain_kernel hands its per-unit conv rows to the last block to arrive with RELAXED agent-scope atomics: sc1 (write-through)
    stores, drained before the arrival count, and sc1 (L1-bypassing) loads in the reader -- no acquire fence on the fast path
    (encoder_fused.hip; MI355X_MICROARCH.md).  The language-level memory model does not order those accesses; what does is the sc1 bit
    on the instructions, so a compiler that stopped emitting it would silently break the hand-off: the ISA is checked here."""
    import glob
    import shutil
    import subprocess
    import tempfile
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "structured_latent_odes_amd", "csrc", "encoder_fused.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "enc.s")
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "--cuda-device-only", "-S", "-o", out, src],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    name = [l.split(":")[0] for l in asm.splitlines() if l.startswith("_ZN") and "enc_chain_kernelILi3ELi14" in l][0]
    body = asm[asm.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    stores = [l for l in body.splitlines() if "global_store_dword" in l and " sc1" in l]
    loads = [l for l in body.splitlines() if "global_load_dword" in l and " sc1" in l]
    atomics = [l for l in body.splitlines() if "global_atomic_add" in l]
    assert len(stores) >= 2 and len(loads) >= 16 and len(atomics) >= 1, (len(stores), len(loads), len(atomics))


def test_batch_keeps_its_converted_label_tensors_alive(monkeypatch):
    """slode_batch carries raw pointers.  A label tensor converted for the step (float64 -> float32, strided -> contiguous) exists only
    for that batch: the batch must hold it as long as it lives, or the caching allocator can hand its memory to the next allocation
    before the step reads it."""
    import gc
    import weakref
    from structured_latent_odes_amd import engine as E
    from structured_latent_odes_amd import svi as S
    B, T = 4, 20
    eng = E.Engine.__new__(E.Engine)   # (no device here; make_batch only reads shapes, strides and pointers)
    eng.device, eng.spec, eng.T = torch.device("cpu"), E.cvs_spec(3, 3, 2), T
    step = S.ELBOStep.__new__(S.ELBOStep)
    step.engine, step.world = eng, 1
    made = []
    label_list = S._label_list
    monkeypatch.setattr(S, "_label_list", lambda labels, u: [made.append(weakref.ref(t)) or t for t in label_list(labels, u)])
    labels = [torch.rand(B, 1, dtype=torch.float64), torch.rand(B, 2)[:, :1]]
    bt = step._batch(torch.rand(B, T, 3).permute(0, 2, 1), None, labels, None)
    gc.collect()
    assert all(r() is not None for r in made) and len(made) == 2
    assert [bt.labels[i] for i in range(2)] == [r().data_ptr() for r in made]
    assert all(r() is not t for r, t in zip(made, labels))   # (both were converted)
    del bt
    gc.collect()
    assert [r() for r in made] == [None, None]


def test_eval_side_lds_byte_totals_are_pinned():
    """The dynamic LDS regions of the four eval-side kernels, through the library's own functions (host arithmetic, no device needed),
    at the shapes DESIGN 3.6-3.9 quote: metric cvs T = 200, challenge-Gauss T = 300, proc T = 100; K = 64 draws for the bounds; the
    shape-specialised and the forced run-time-S form (proc's S = 8 rows are already SLODE_MAX_S wide).  The kernels share their forward
    pieces (csrc/slode_forward.h): a change there that moves any of these totals moves occupancy and the refusal thresholds."""
    from structured_latent_odes_amd import _lib as L, engine as E
    lib = L.load()

    class _E(E.Engine):
        def __init__(self, spec, T):
            self.spec, self.T, self._shapes = spec, T, {}

    def fn(mangled):
        f = getattr(lib, mangled)
        f.restype = C.c_size_t
        return f

    ev = fn("_Z20slode_eval_lds_bytesRK11slode_shape")
    rm = fn("_Z29slode_recon_moments_lds_bytesRK11slode_shapei")
    tb = fn("_Z27slode_traj_bounds_lds_bytesRK11slode_shapeii")
    iv = fn("_Z33slode_intervene_moments_lds_bytesRK11slode_shapei")
    # shape -> eval, then (recon, bounds at K = 64, intervene) specialised and forced generic
    want = {"cvs": (15920, (33600, 19792, 62464), (34400, 20592, 63264)),
            "challenge": (23920, (31792, 32320, 51120), (32592, 33120, 51920)),
            "proc": (12672, (35040, 25680, 54656), (35040, 25680, 54656))}
    for name, spec, T in (("cvs", E.cvs_spec(3, 3, 2, solver="rk4"), 200), ("challenge", E.challenge_spec(gauss=True, solver="rk4"), 300),
                          ("proc", E.proc_spec(z_g=10, z_eps=10, solver="rk4"), 100)):
        s = _E(spec, T).shape(1024)
        got = (ev(C.byref(s)),) + tuple((rm(C.byref(s), g), tb(C.byref(s), 64, g), iv(C.byref(s), g)) for g in (0, 1))
        assert got == want[name], (name, got, want[name])


def test_eval_side_refusals_match_the_recorded_ladder(tmp_path):
    """Every refusing configuration of slode_eval_stats / slode_recon_moments / slode_traj_bounds / slode_intervene_moments, on a
    hand-filled handle (tests/eval_refusals/eval_refusals.cpp: no device, no HIP call, no call that would be taken): status, message and
    the untouched drawing-call counter, line by line against tests/golden/eval_refusals.txt -- which check speaks first when two
    conditions hold included.  The file was recorded from the library before the four calls shared one host ladder."""
    from tests.refusals_util import refusal_lines
    got = refusal_lines("eval_refusals", tmp_path)
    want = open(os.path.join(ROOT, "tests", "golden", "eval_refusals.txt")).read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d:\n  got  %s\n  want %s" % (i + 1, g, w)
    assert len(got) == len(want) and len(want) > 150
