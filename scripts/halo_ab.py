"""Halo 3x3 conv (conv3x3_halo_kernel): two or more builds of the library in ONE process on the
same buffers -- byte comparison of the outputs and the GroupNorm column sums, then the builds
alternated: ROUNDS rounds of the median of REPS launches per build and call.

    python scripts/halo_ab.py LIB_A LIB_B [LIB_C ...]      # A is the reference of the comparison
    python scripts/halo_ab.py --once LIB                   # each call 3 times (under rocprofv3)

The calls are the flagship's (bench.py configs[1], 48 windows = 768 frames in the UNet):
  u32   32^2 320 -> 320, GroupNorm affine + SiLU, residual, column sums, 768 images (BN 160)
  u16   16^2 640 -> 640, the same                                                   (BN 160)
  v512  VAE 64^2 512 -> 512, GroupNorm per image, column sums, 48 images   (BN 128, 16 x 16)
  v128  VAE 256^2 128 -> 128, the same, 16 images                          (BN 128, 16 x 8)
  ups   the UNet's 640-channel 16^2 -> 32^2 upsampler, phase form, 768 images  (BN 160, PH)
and, with --shapes test, eight small calls over the forms tests/test_gpu_halo_taps.py covers.
(The TF/s column counts the algorithmic 9-tap flops; the phase form executes 4/9 of them.)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from latentsync_amd import _lib, ops  # noqa: E402
from latentsync_amd.packing import pack_phase_weight, pack_weight  # noqa: E402

BF, DEV = torch.bfloat16, "cuda"
ROUNDS, REPS = int(os.environ.get("ROUNDS", 8)), int(os.environ.get("REPS", 20))


def load(path):
    _lib._lib = None
    return _lib.load(path)


def use(lib):
    _lib._lib = lib


def make_call(name, n, H, W, C1, C2, N, ipp, aff, res, ups=False, rowvec=False):
    g = torch.Generator(device=DEV).manual_seed(len(name) * 1000 + H + C1 + N)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    Cin = C1 + C2
    x = rn(n, H, W, C1).to(BF)
    w = (rn(N, Cin, 3, 3) / (9 * Cin) ** 0.5).cpu()
    pw = ops.Packed(pack_weight(w).to(BF).to(DEV), 0.1 * rn(N), Cin, 3, N)
    kw = {}
    if C2:
        kw["x2"] = rn(n, H, W, C2).to(BF)
    if ups:
        pw.phase = pack_phase_weight(w).to(BF).to(DEV).contiguous()
        kw["upsample"] = True
    if aff:
        kw["aff"] = (1 + 0.2 * rn(n // ipp, Cin), 0.3 * rn(n // ipp, Cin), ipp, True)
    if rowvec:
        kw["rowvec"] = (rn(n, N), H * W, N)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    if res:
        kw["res"] = rn(n, Ho, Wo, N).to(BF)
    out = torch.empty(n, Ho, Wo, N, dtype=BF, device=DEV)
    cs = torch.empty(n * Ho * Wo // 128, 2, N, dtype=torch.float32, device=DEV)
    flops = 2.0 * n * Ho * Wo * N * Cin * 9
    return name, (lambda: ops.conv(x, pw, out=out, gn_out=cs, **kw)), out, cs, flops, (x, pw, kw)


def calls(which):
    c = [("u32", 768, 32, 32, 320, 0, 320, 16, True, True), ("u16", 768, 16, 16, 640, 0, 640, 16, True, True),
         ("v512", 48, 64, 64, 512, 0, 512, 1, True, False), ("v128", 16, 256, 256, 128, 0, 128, 1, True, False),
         ("ups", 768, 16, 16, 640, 0, 640, 1, False, False, True)]
    if which == "test":  # small calls over the forms of tests/test_gpu_halo_taps.py
        c += [("t64", 2, 16, 16, 64, 0, 160, 1, True, True), ("t128", 2, 32, 48, 128, 0, 320, 2, True, True, False, True),
              ("t192", 2, 32, 48, 64, 128, 160, 1, True, False), ("t320", 2, 32, 48, 320, 0, 128, 2, True, True),
              ("t128n", 2, 32, 48, 128, 0, 128, 1, True, False), ("tn8", 2, 32, 48, 128, 0, 8, 1, True, False),
              ("tu160", 2, 16, 16, 192, 0, 160, 1, False, True, True), ("tu128", 2, 16, 16, 128, 0, 128, 1, False, False, True)]
    return [make_call(*a) for a in c]


def time_call(f):
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def main():
    args = sys.argv[1:]
    which = "bench"
    if "--shapes" in args:
        i = args.index("--shapes")
        which = args[i + 1]
        del args[i:i + 2]
    if args[0] == "--once":
        use(load(args[1]))
        for name, f, *_ in calls(which):
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            print("ran", name, flush=True)
        return
    libs = [(os.path.basename(p), load(p)) for p in args]
    bad = 0
    cl = calls(which)
    for name, f, out, cs, flops, (x, pw, kw) in cl:
        ref = None
        for ln, lib in libs:
            use(lib)
            out.zero_(); cs.zero_()
            plan = ops.conv_plan(x, pw, **kw)
            f()
            torch.cuda.synchronize()
            got = (out.view(torch.int16).clone(), cs.view(torch.int32).clone())
            if ref is None:
                ref = got
                print(f"{name}: family {plan['family']} BN {plan['halo_bn']} TH {plan['halo_th']} grid {plan['grid']}")
                continue
            same = torch.equal(ref[0], got[0]), torch.equal(ref[1], got[1])
            bad += not all(same)
            print(f"{name}: {ln} vs {libs[0][0]}: y bytes {'identical' if same[0] else 'DIFFER'}, "
                  f"column sums {'identical' if same[1] else 'DIFFER'}", flush=True)
    if os.environ.get("COMPARE_ONLY"):
        sys.exit(1 if bad else 0)
    for name, f, out, cs, flops, _ in cl[:5]:
        rows = {ln: [] for ln, _ in libs}
        for r in range(ROUNDS):
            for ln, lib in libs:
                use(lib)
                f(); torch.cuda.synchronize()
                rows[ln].append(time_call(f))
        for ln, v in rows.items():
            med = statistics.median(v)
            print(f"{name:5s} {ln:24s} median {med:8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  "
                  f"{flops / med / 1e6:6.0f} TF/s  rounds {' '.join(f'{t:.0f}' for t in v)}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
