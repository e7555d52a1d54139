"""Build the A/B libraries of the gfx950 SLP investigation:

  slp     the conv / GEMM sources (ls_conv*.hip) with SLP vectorisation on (the build that
          produced wrong LayerNorm-folded row-block rows), everything else as shipped;
  slp_bw  slp + every hand-written `s_waitcnt vmcnt(N)` (wait_vm, ls_common.h) replaced by
          __builtin_amdgcn_s_waitcnt (an S_WAITCNT the compiler's own waitcnt pass
          sees), i.e. no inline asm the compiler cannot reason about;
  slp_noasm  slp_bw + the row-block kernel's remaining inline asm (lgkmcnt waits and
          compiler memory barriers around s_barrier) replaced by __syncthreads(): the
          kernel then holds no hand-written asm at all;
  slp_nop slp + `-mllvm -amdgpu-snop-padding=4` (s_nop 4 before every instruction);
  slp_wz  slp + `-mllvm -amdgpu-waitcnt-forcezero` (every wait drains all counters);
  slp_sb  slp + a scheduling barrier right after the row-block LayerNorm loop, so
          the packed normalisation stays ahead of the first chunk's LDS reads/MFMAs
          instead of being interleaved with them.

Each goes to latentsync_amd/libls_hip_<name>.so; select with LS_HIP_LIB.  The
disassembly of each row-block LN kernel is written beside it (build/slp/<name>.s).
usage: python scripts/slp_variants.py"""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latentsync_amd", "csrc")
OUT = os.path.join(ROOT, "build", "slp")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result", "-munsafe-fp-atomics"]
HIPCC = "/opt/rocm/bin/hipcc"

WAIT_ASM = 'template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }'
# gfx9 S_WAITCNT simm16: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt_hi[15:14]; others at max
WAIT_BUILTIN = ("template <int N> __device__ __forceinline__ void wait_vm() "
                "{ __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0F70); }")
LN_END = "  wait_vm<0>();\n  __builtin_amdgcn_s_barrier();\n  asm volatile(\"\" ::: \"memory\");\n\n  f32x4 acc0[FM][FN]"


# the conv / GEMM translation units (the variants build all five with SLP on); the patched
# inline asm is the row-block kernel's, the wait_vm template is ls_common.h's
CONV = ("ls_conv.hip", "ls_conv_tiled.hip", "ls_conv_big.hip", "ls_conv_rowblock.hip", "ls_conv_halo.hip")
RB = "ls_conv_rowblock.hip"


def variant(name, edits=(), extra=()):
    """edits: (file, old, new), each `old` exactly once in csrc/file."""
    top = os.path.join(OUT, name)
    shutil.rmtree(top, ignore_errors=True)
    d = os.path.join(top, "pkg", "csrc")  # csrc/../../include/ls_hip.h resolves as in-tree
    shutil.copytree(CSRC, d)
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(top, "include"))
    for fn, old, new in edits:
        src = open(os.path.join(d, fn)).read()
        assert src.count(old) == 1, (fn, old)
        with open(os.path.join(d, fn), "w") as f:
            f.write(src.replace(old, new))
    objs = []
    procs = []
    for fn in sorted(os.listdir(d)):
        if not fn.endswith(".hip"):
            continue
        flags = FLAGS + (list(extra) if fn in CONV else ["-fno-slp-vectorize"])
        o = os.path.join(d, fn[:-4] + ".o")
        procs.append(subprocess.Popen([HIPCC] + flags + ["-c", os.path.join(d, fn), "-o", o]))
        objs.append(o)
    if any(p.wait() for p in procs):
        sys.exit(f"{name}: compile failed")
    lib = os.path.join(ROOT, "latentsync_amd", f"libls_hip_{name}.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
    # device disassembly of the LN-folded row-block kernel (FLAGS = RB_LN)
    s = subprocess.run([HIPCC] + FLAGS + list(extra) + ["--cuda-device-only", "-S",
                        os.path.join(d, RB), "-o", "-"], capture_output=True, text=True).stdout
    sym = "_ZN2ls20gemm_rowblock_kernelILi10ELi2ELi2ELi1EEEvNS_8ConvArgsE:"
    body = s[s.index(sym):]
    body = body[:body.index(".Lfunc_end", 1)]
    with open(os.path.join(OUT, f"{name}.s"), "w") as f:
        f.write(body)
    print(f"built {lib}: {body.count('v_pk_fma_f32')} v_pk_fma_f32 in the LN row-block kernel", flush=True)


def main():
    only = sys.argv[1:]
    if only:
        global variant
        build = variant
        variant = lambda name, edits=(), extra=(): build(name, edits, extra) if name in only else None
    os.makedirs(OUT, exist_ok=True)
    builtin_wait = ("ls_common.h", WAIT_ASM, WAIT_BUILTIN)
    variant("slp")
    variant("slp_bw", [builtin_wait])
    rb_sync = ('    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");\n    __builtin_amdgcn_s_barrier();\n'
               '    asm volatile("" ::: "memory");\n  };')
    ln_sync = '  __builtin_amdgcn_s_barrier();\n  asm volatile("" ::: "memory");\n\n  f32x4 acc0[FM][FN]'
    variant("slp_noasm", [builtin_wait, (RB, rb_sync, "    __syncthreads();\n  };"),
                          (RB, ln_sync, "  __syncthreads();\n\n  f32x4 acc0[FM][FN]")])
    # compiler-side knobs on the unchanged source: 4 wait states before every
    # instruction (a VALU / MFMA hazard that needs more nops than the compiler
    # inserts disappears), and every s_waitcnt forced to zero (a memory-counter race
    # disappears)
    variant("slp_nop", extra=["-mllvm", "-amdgpu-snop-padding=4"])
    variant("slp_wz", extra=["-mllvm", "-amdgpu-waitcnt-forcezero"])
    variant("slp_sb", [(RB, LN_END, LN_END.replace("  wait_vm<0>();\n", "  __builtin_amdgcn_sched_barrier(0);\n  wait_vm<0>();\n", 1))])


if __name__ == "__main__":
    main()
