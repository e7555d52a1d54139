"""Times the S3FD detector's convs and one whole-clip detection (latentsync_amd/s3fd.py).

    python scripts/s3fd_bench.py            # both parts
    python scripts/s3fd_bench.py --layers   # the per-layer conv comparison only
    python scripts/s3fd_bench.py --clip     # the whole-clip time only

Per layer: ls_conv3x3_relu against ls_conv_general with ReLU on the same packed operand, for the
trunk's second conv of each stage at 32 frames of 180 x 320 (conv1_2 64 -> 64 at 180 x 320,
conv2_2 128 -> 128 at 90 x 160, conv3_2 256 -> 256 at 45 x 80, conv4_2 512 -> 512 at 23 x 40,
conv5_2 512 -> 512 at 11 x 20) and fc6 (512 -> 1024, dilation 6, 5 x 10), which has no
counterpart.  The two kernels alternate in one process after a warm-up; each figure is the
median of RUNS device-event timings of one launch, and TFLOP/s counts 2 * 9 * Cin * N per output
pixel (the padding taps included, so a kernel that skips them is credited with them).

Whole clip: S3FD.detect on 250 frames of 720 x 1280 at scale 0.25 (a 180 x 320 network input),
seeded weights (tests/s3fd_ref.py), wall time ending in a synchronise, median of 5.

Every line is printed and written to bench_out/s3fd_bench.log; DESIGN.md section 4.8 records
the table.
"""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import s3fd_ref as R  # noqa: E402
from latentsync_amd import ops, s3fd  # noqa: E402
from latentsync_amd.packing import pack_weight_general  # noqa: E402

RUNS = 7
FRAMES = 32
LAYERS = (("conv1_2", 64, 64, 180, 320, 1), ("conv2_2", 128, 128, 90, 160, 1), ("conv3_2", 256, 256, 45, 80, 1),
          ("conv4_2", 512, 512, 23, 40, 1), ("conv5_2", 512, 512, 11, 20, 1), ("fc6", 512, 1024, 5, 10, 6))
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def layers():
    g = torch.Generator().manual_seed(0)
    for name, cin, n, H, W, dil in LAYERS:
        x = torch.randn((FRAMES, H, W, cin), generator=g).relu().to(torch.bfloat16).cuda()
        w = torch.randn((n, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
        pw = ops.PackedGeneral(pack_weight_general(w).to(torch.bfloat16).cuda(), torch.zeros(n).cuda(), cin, (1, 3, 3))
        out = torch.empty((FRAMES, H, W, n), dtype=torch.bfloat16, device="cuda")
        new = lambda: ops.conv3x3_relu(x, pw, dil, out=out)
        old = (lambda: ops.conv_general(x, pw, (1, 1), (1, 1), relu=True, out=out)) if dil == 1 else None
        for _ in range(2):
            new()
            if old:
                old()
        torch.cuda.synchronize()
        tn, to = [], []
        for _ in range(RUNS):
            tn.append(timed(new))
            if old:
                to.append(timed(old))
        flop = 2.0 * 9 * cin * n * FRAMES * H * W
        mn = sorted(tn)[RUNS // 2]
        line = f"{name}: {cin} -> {n}, {FRAMES} x {H} x {W}, dilation {dil}: ls_conv3x3_relu {mn:.3f} ms ({flop / mn / 1e9:.1f} TFLOP/s)"
        if old:
            mo = sorted(to)[RUNS // 2]
            line += f"; ls_conv_general {mo:.3f} ms ({flop / mo / 1e9:.1f} TFLOP/s); general / new = {mo / mn:.2f}"
        say(line)


def clip(n=250, H=720, W=1280, scale=0.25):
    det = s3fd.S3FD(device="cuda", weights=R.case_weights())
    frames = torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    det.detect(frames, conf_th=0.9, scale=scale)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        boxes = det.detect(frames, conf_th=0.9, scale=scale)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    h, w = ops.s3fd_prep_size(H, W, scale)
    say(f"S3FD.detect on {n} frames of {H} x {W} at scale {scale} ({h} x {w} input, {det.chunk_frames(h, w)} frames a "
        f"chunk): wall incl. the copy of the boxes, 5 runs: " + ", ".join(f"{t * 1e3:.1f}" for t in ts) +
        f" ms; median {sorted(ts)[2] * 1e3:.1f} ms; {sum(len(b) for b in boxes)} boxes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--clip", action="store_true")
    a = ap.parse_args()
    if a.layers or not a.clip:
        layers()
    if a.clip or not a.layers:
        clip()
    out = os.path.join(REPO, "bench_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "s3fd_bench.log"), "w") as f:
        f.write("\n".join(LINES) + "\n")
