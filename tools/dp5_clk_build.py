"""Diagnostic build of libslode with cycle stamps in the dopri5 reverse sweep (printf from workgroups 0 and 100): where the kernel's time goes.
Usage (here): python tools/dp5_clk_build.py   -> structured_latent_odes_amd/libslode_clk.so ; on the GPU box:
SLODE_LIB_PATH=structured_latent_odes_amd/libslode_clk.so python tools/dp5_profile.py 3

patched_source() returns the kernel file's text with the stamps in (no compiler needed: tests/test_host_cpu.py calls it, so an anchor that
left the source fails a CPU test); build() compiles it in place of dopri5_kernel.hip with the source list and the flags of csrc/Makefile
(tools/dp5_fwd_clk_build.py builds through it too)."""
import os, re, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "structured_latent_odes_amd", "csrc")
KERNEL = "dopri5_kernel.hip"


class Patch:
    """Text with rep(): replace the first occurrence of an anchor, which must be there."""
    def __init__(self, text):
        self.text = text

    def rep(self, old, new):
        assert old in self.text, "anchor left the source: " + old[:70]
        self.text = self.text.replace(old, new, 1)


def kernel_source():
    return open(os.path.join(SRC, KERNEL)).read()


def patched_source():
    p = Patch(kernel_source())
    p.rep("  GroupLds<H> m;\n  float* s_gu = m.carve(smem, BTP);", "  unsigned long long clk[12]; int nclk = 0;\n#define CLK() clk[nclk++] = __builtin_readcyclecounter()\n  CLK();\n  GroupLds<H> m;\n  float* s_gu = m.carve(smem, BTP);")
    p.rep("  {\n    constexpr int ZQ = SLODE_MAX_L / G;\n    float zv[ZQ];", "  unsigned long long c_a = __builtin_readcyclecounter();\n  {\n    constexpr int ZQ = SLODE_MAX_L / G;\n    float zv[ZQ];")
    p.rep("  Units w;\n  unsigned dirmask;\n  if (k.tabs) {", "  unsigned long long c_b = __builtin_readcyclecounter(), c_c = c_b;\n  CLK();\n  Units w;\n  unsigned dirmask;\n  if (k.tabs) {")
    p.rep("  const float* s_us = m.u + slot * 32;\n  const int* s_rnk", "  CLK();\n  const float* s_us = m.u + slot * 32;\n  const int* s_rnk")
    p.rep("  const bool any_bad = __syncthreads_or(live && bad) != 0;", "  CLK();\n  const bool any_bad = __syncthreads_or(live && bad) != 0;\n  CLK();")
    p.rep("    __syncthreads();\n    for (int col = tid; col < (H + 1) * NTMP; col += BNT) {", "    CLK();\n    __syncthreads();\n    for (int col = tid; col < (H + 1) * NTMP; col += BNT) {")
    p.rep("  // ---- init net: x0 = sigmoid(W2 relu(W1 z + b1) + b2); the j = 0 output is x0 itself", "  CLK();\n  // ---- init net: x0 = sigmoid(W2 relu(W1 z + b1) + b2); the j = 0 output is x0 itself")
    p.rep("    // latent gradient of this trajectory: through the init net and (exact mode)", "    CLK();\n    // latent gradient of this trajectory: through the init net and (exact mode)")
    p.rep("    // sums over the workgroup's trajectories (fixed order): outer products with z", "    CLK();\n    // sums over the workgroup's trajectories (fixed order): outer products with z")
    s = p.text
    i = s.index("}  // namespace grp")
    j = s.rfind("}\n", 0, i)   # the reverse kernel's closing brace
    return s[:j] + "  CLK();\n  if ((blockIdx.x == 0 || blockIdx.x == 100) && tid == 0) printf(\"dp5bwd wg %d stage detail: requests + zero-fill %llu, latent rows %llu (%llu %llu)\\n\", (int)blockIdx.x, c_a-clk[0], c_b-c_a, c_c-c_b, clk[1]-c_c);\n  if ((blockIdx.x == 0 || blockIdx.x == 100) && tid == 0) printf(\"dp5bwd wg %d K %d cycles: stage %llu units+table %llu loop %llu wait %llu snapshots %llu colsums %llu initnet %llu latent %llu outer %llu\\n\", (int)blockIdx.x, K, clk[1]-clk[0], clk[2]-clk[1], clk[3]-clk[2], clk[4]-clk[3], clk[5]-clk[4], clk[6]-clk[5], clk[7]-clk[6], clk[8]-clk[7], clk[9]-clk[8]);\n" + s[j:]


def makefile_build():
    """(compiler, flags, sources) of csrc/Makefile: what `make` itself compiles libslode.so from"""
    mk = open(os.path.join(SRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, mk, re.M).group(1).strip()
    flags = var("CXXFLAGS").replace("$(ARCH)", os.environ.get("ARCH", var("ARCH"))).split()
    return os.environ.get("HIPCC", var("HIPCC")), flags, var("SRCS").split()


def build(text, out="libslode_clk.so"):
    """libslode with `text` in place of dopri5_kernel.hip -> structured_latent_odes_amd/<out>"""
    hipcc, flags, srcs = makefile_build()
    assert KERNEL in srcs, srcs
    tmp = "_dp5_clk.hip"
    open(os.path.join(SRC, tmp), "w").write(text)
    try:
        subprocess.check_call([hipcc] + flags + ["-shared", "-o", os.path.join("..", out)] + [tmp if f == KERNEL else f for f in srcs], cwd=SRC)
    finally:
        os.remove(os.path.join(SRC, tmp))
    print("built " + out)


if __name__ == "__main__":
    build(patched_source())
