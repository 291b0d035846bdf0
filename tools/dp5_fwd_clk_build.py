"""Diagnostic build of libslode with cycle counters in the dopri5 FORWARD solve, dopri5_fwd_kernel at every lane width (printf from
workgroups 0 and 100, each line names the lanes per trajectory it ran at): where the set-up's and an attempted step's time goes.
Usage (here): python tools/dp5_fwd_clk_build.py -> structured_latent_odes_amd/libslode_clk.so; on the GPU box:
SLODE_LIB_PATH=structured_latent_odes_amd/libslode_clk.so [SLODE_DP5_LPT=8|16|32|64] python tools/dp5_profile.py 2

patched_source() / build() as in tools/dp5_clk_build.py (the reverse sweep's tool), whose build step this one uses."""
from dp5_clk_build import Patch, build, kernel_source


def patched_source():
    s = kernel_source()
    i0 = s.index("dopri5_fwd_kernel(const DpK k) {")
    i1 = s.index("// ---- reverse mode over the recorded steps")
    # set-up detail: stamps inside load_units (workgroup 0, thread 0) through a __device__ array
    pre = Patch(s[:i0])
    pre.rep("template <int S, int H, int LPT = G>\n__device__ __forceinline__ unsigned load_units(",
            "__device__ unsigned long long g_clk[12];\n#define CLK(i) if (blockIdx.x == 0 && threadIdx.x == 0) g_clk[i] = __builtin_readcyclecounter()\n"
            "template <int S, int H, int LPT = G>\n__device__ __forceinline__ unsigned load_units(")
    pre.rep("  asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");              // this wave's LDS-DMA has landed; the barrier covers the others'\n  __syncthreads();",
            "  CLK(0);\n  asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n  __syncthreads();\n  CLK(1);")
    pre.rep("  const unsigned dirmask = group_or(dm);\n  __syncthreads();", "  const unsigned dirmask = group_or(dm);\n  __syncthreads();\n  CLK(2);")
    pre.rep("  __syncthreads();\n  // segment table, event by event", "  __syncthreads();\n  CLK(3);\n  // segment table, event by event")
    pre.rep("  __syncthreads();\n  return dirmask;", "  __syncthreads();\n  CLK(4);\n  return dirmask;")
    # the kernel: set-up stamps, then per attempt: evaluations, gather, combination + error, norm, accept block, factor
    b = Patch(s[i0:i1])
    stamp = lambda keep, i: "    asm volatile(\"\" :: %s); c1 = __builtin_readcyclecounter(); acc[%d] += c1 - c0; c0 = c1;\n" % (keep, i)
    b.rep("  extern __shared__ __attribute__((aligned(16))) float smem[];", "  extern __shared__ __attribute__((aligned(16))) float smem[];\n  const unsigned long long c_begin = __builtin_readcyclecounter();")
    b.rep("  InitRegs<S, H> ir;\n  init_request<S, H>(k.w2, k.b2, g, ir);\n  latent_store<LPT>(",
          "  CLK(7);\n  InitRegs<S, H> ir;\n  init_request<S, H>(k.w2, k.b2, g, ir);\n  asm volatile(\"\" ::: \"memory\"); CLK(8);\n  latent_store<LPT>(")
    b.rep("  float y = init_state<S, H>(ir, pre0, g, own);", "  float y = init_state<S, H>(ir, pre0, g, own);\n  asm volatile(\"\" :: \"v\"(y)); CLK(5);")
    b.rep("  int j = 1;\n  int steps = bad_grid", "  asm volatile(\"\" :: \"v\"(dt)); CLK(6);\n  unsigned long long c_set = __builtin_readcyclecounter(), acc[6] = {0, 0, 0, 0, 0, 0}, c0, c1;\n  int j = 1;\n  int steps = bad_grid")
    b.rep("    ++steps;\n", "    ++steps;\n    c0 = __builtin_readcyclecounter();\n")
    b.rep("    float av[NT], dv[NT];\n    if (NG == 1) {", stamp("\"v\"(ar[0])", 0) + "    float av[NT], dv[NT];\n    if (NG == 1) {")
    b.rep("    typename M::K kk;\n", stamp("\"v\"(av[0]), \"v\"(dv[NT - 1])", 5) + "    typename M::K kk;\n")
    b.rep("    const float ratio = group_rms_fast<S>(", stamp("\"v\"(er)", 1) + "    const float ratio = group_rms_fast<S>(")
    b.rep("    if (accept) {\n      const float t1 = t + dt;", stamp("\"v\"(ratio)", 2) + "    if (accept) {\n      const float t1 = t + dt;")
    b.rep("    if (act) {\n      float factor;", stamp("\"v\"(y), \"v\"(t)", 3) + "    if (act) {\n      float factor;")
    b.rep("      dt *= factor;\n    }\n  }\n", "      dt *= factor;\n    }\n    asm volatile(\"\" :: \"v\"(dt)); c1 = __builtin_readcyclecounter(); acc[4] += c1 - c0;\n  }\n"
          "  if (blockIdx.x == 0 && tid == 0) printf(\"dp5fwd lpt %d first phase: units_request issued %llu, init_request issued %llu\\n\", LPT, g_clk[7] - c_begin, g_clk[8] - c_begin);\n"
          "  if (blockIdx.x == 0 && tid == 0) printf(\"dp5fwd lpt %d set-up (cycles from kernel start): requests issued, latent rows staged %llu, all set-up operands landed %llu, unit sums %llu, rank %llu, segment table %llu, init state %llu, initial step %llu\\n\","
          " LPT, g_clk[0] - c_begin, g_clk[1] - c_begin, g_clk[2] - c_begin, g_clk[3] - c_begin, g_clk[4] - c_begin, g_clk[5] - c_begin, g_clk[6] - c_begin);\n"
          "  if ((blockIdx.x == 0 || blockIdx.x == 100) && tid == 0) printf(\"dp5fwd lpt %d wg %d attempts %d accepted %d: set-up %llu cycles; per attempt: evals %llu  gather %llu  combination+error %llu  norm %llu  accept block (records, outputs) %llu  factor %llu\\n\","
          " LPT, (int)blockIdx.x, steps, nacc, c_set - c_begin, acc[0] / steps, acc[5] / steps, acc[1] / steps, acc[2] / steps, acc[3] / steps, acc[4] / steps);\n")
    return pre.text + b.text + s[i1:]


if __name__ == "__main__":
    build(patched_source())
