"""Position-major 3x3 conv (tuning key 22) against the standard raster: builds of the library and
tuning variants in ONE process on the same buffers -- byte comparison of y and of the GroupNorm
column sums with the first variant, then the variants alternated: ROUNDS rounds of the median of
REPS launches per variant and call.

    python scripts/posmajor_ab.py PARENT_LIB NEW_LIB     # parent | new (cost model) | new, forced forms
    python scripts/posmajor_ab.py --once LIB [KEY22 [NAME]]  # the calls whose name contains NAME (default
                                                             # "8x8") 3 times each (under rocprofv3)

The calls are the flagship's 3x3 / stride 1 convs at the 8x8 and 4x4 levels (bench.py configs[1],
48 windows = 768 frames, N = 1280): K = 11520 and 23040 (the concat of two 1280-channel sources),
with the row vector of conv1 or the residual of conv2.  Variants per call: the parent library; the
new library as planned; at 4x4 also position-major forced on the 256 x 256 tile (key 22 = 2) and on
the 256 x 128 tile (key 22 = 2, key 2 = 6), and the standard raster on 256 x 128 (key 22 = 0,
key 2 = 6)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from latentsync_amd import _lib, ops  # noqa: E402
from latentsync_amd.packing import pack_weight  # noqa: E402

BF, DEV = torch.bfloat16, "cuda"
ROUNDS, REPS = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 20))
NB, N = 768, 1280


def load(path):
    _lib._lib = None
    try:
        return _lib.load(path)
    except AttributeError:  # a build from before ls_conv_posmajor_tile (the parent)
        sig = _lib._SIGS.pop("ls_conv_posmajor_tile")
        try:
            return _lib.load(path)
        finally:
            _lib._SIGS["ls_conv_posmajor_tile"] = sig


def make_call(name, hw, C1, C2, res, rowvec):
    g = torch.Generator(device=DEV).manual_seed(hw * 100 + C1 + C2 + res)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    Cin = C1 + C2
    x = rn(NB, hw, hw, C1).to(BF)
    w = (rn(N, Cin, 3, 3) / (9 * Cin) ** 0.5).cpu()
    pw = ops.Packed(pack_weight(w).to(BF).to(DEV), 0.1 * rn(N), Cin, 3, N)
    kw = {}
    if C2:
        kw["x2"] = rn(NB, hw, hw, C2).to(BF)
    if rowvec:  # one timestep row for the whole batch, as the UNet forward passes it
        kw["rowvec"] = (rn(1, N), NB * hw * hw, N)
    if res:
        kw["res"] = rn(NB, hw, hw, N).to(BF)
    out = torch.empty(NB, hw, hw, N, dtype=BF, device=DEV)
    cs = torch.empty(NB * hw * hw // 128, 2, N, dtype=torch.float32, device=DEV)
    flops = 2.0 * NB * hw * hw * N * Cin * 9
    return name, hw, (lambda: ops.conv(x, pw, out=out, gn_out=cs, **kw)), out, cs, flops, (x, pw, kw)


def calls():
    c = []
    for hw in (8, 4):
        c += [(f"{hw}x{hw} K11520 rowvec", hw, 1280, 0, False, True), (f"{hw}x{hw} K11520 res", hw, 1280, 0, True, False),
              (f"{hw}x{hw} K23040 rowvec", hw, 1280, 1280, False, True), (f"{hw}x{hw} K23040 res", hw, 1280, 1280, True, False)]
    return [make_call(*a) for a in c]


class variant:
    def __init__(self, name, lib, keys):
        self.name, self.lib, self.keys = name, lib, keys

    def __enter__(self):
        _lib._lib = self.lib
        for k, v in self.keys.items():
            assert self.lib.ls_set_tuning(k, v) == 0

    def __exit__(self, *exc):
        for k in self.keys:
            self.lib.ls_set_tuning(k, {22: 1, 2: 0}[k])
        return False


def time_call(f):
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def main():
    args = sys.argv[1:]
    if args[0] == "--once":
        lib = load(args[1])
        if len(args) > 2 and args[2] != "-":  # ("-": a build without the key, the parent)
            assert lib.ls_set_tuning(22, int(args[2])) == 0
        sel = args[3] if len(args) > 3 else "8x8"
        for name, hw, f, *_ in calls():
            if sel not in name:
                continue
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            print("ran", name, flush=True)
        return
    parent, new = load(args[0]), load(args[1])
    bad = 0
    for name, hw, f, out, cs, flops, (x, pw, kw) in calls():
        vs = [variant("parent", parent, {}), variant("new", new, {})]
        if hw == 4:
            vs += [variant("new pm 256x256", new, {22: 2}), variant("new pm 256x128", new, {22: 2, 2: 6}),
                   variant("new std 256x128", new, {22: 0, 2: 6})]
        ref = None
        for v in vs:
            with v:
                out.zero_(); cs.zero_()
                plan = ops.conv_plan(x, pw, out=out, gn_out=cs, workspace_bytes=ops.workspace(x.device).gemm.numel(), **kw)
                f()
                torch.cuda.synchronize()
            got = (out.view(torch.int16).clone(), cs.view(torch.int32).clone())
            form = f"tile {plan['bm']}x{plan['bn']} split {plan['split']} grid {plan['grid']}" + \
                   (f" posmajor {plan['posmajor']}" if v.lib is new else "")
            if ref is None:
                ref = got
                print(f"{name}: {v.name}: {form}")
                continue
            same = torch.equal(ref[0], got[0]), torch.equal(ref[1], got[1])
            bad += not all(same)
            print(f"{name}: {v.name}: {form}; y bytes {'identical' if same[0] else 'DIFFER'}, "
                  f"column sums {'identical' if same[1] else 'DIFFER'}", flush=True)
        if os.environ.get("COMPARE_ONLY"):
            continue
        rows = {v.name: [] for v in vs}
        for r in range(ROUNDS):
            for v in vs:
                with v:
                    f(); torch.cuda.synchronize()
                    rows[v.name].append(time_call(f))
        base = rows["parent"]
        spread = max(base) - min(base)
        for vn, t in rows.items():
            med = statistics.median(t)
            wins = vn != "parent" and all(b - a > spread for a, b in zip(t, base))
            print(f"{name:20s} {vn:16s} median {med:8.1f} us  {flops / med / 1e6:6.0f} TF/s  ratio {med / statistics.median(base):.3f}  "
                  f"rounds {' '.join(f'{a:.0f}' for a in t)}" + (f"  parent spread {spread:.1f} us" if vn == "parent" else
                                                                 f"  clears the criterion: {'yes' if wins else 'no'}"), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
