"""read_avi_device (Motion-JPEG decoded on the device) against read_avi (Pillow on the host)
on one clip, in one process, alternating the two: ms per frame of each, for the clip as this
project's encoder writes it (restart interval 10) and for the same clip re-saved through
Pillow without restart markers.  Writes one JSON file; the decoded frames of the two routes
are compared first.

    python scripts/mjpeg_decode_bench.py --out bench_out/mjpeg_decode.json
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/mjpeg_decode_bench.py --device-only --reps 3
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentsync_amd import video  # noqa: E402


def clip(n, H, W, seed=0):
    """Smooth content plus noise: low-resolution colour upsampled bicubically, +-6 of noise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    low = torch.rand((n, 3, H // 40, W // 40), generator=g, device="cuda")
    up = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False) * 255
    up = up + (torch.rand(up.shape, generator=g, device="cuda") - 0.5) * 12
    return up.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="only the device route (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_decode_bench: no HIP device; a CPU run measures nothing")
    from PIL import Image
    frames = clip(a.frames, a.height, a.width)
    own = video.encode_frames(frames, a.quality)
    plain = []
    for j in own:  # the same pixels through Pillow's encoder: 4:2:0, Annex K tables, no DRI
        b = io.BytesIO()
        Image.open(io.BytesIO(j)).save(b, "JPEG", quality=a.quality, subsampling="4:2:0")
        plain.append(b.getvalue())
    res = {"frames": a.frames, "height": a.height, "width": a.width, "quality": a.quality, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    with tempfile.TemporaryDirectory() as td:
        for name, jpgs in (("restart_interval_10", own), ("no_restart_markers", plain)):
            path = os.path.join(td, name + ".avi")
            video.write_avi(path, jpgs, 25)
            info = video.parse_jpeg(jpgs[0])
            dev = video.read_avi_device(path, "cuda")[0]  # warm-up of every shape, and the check
            case = {"bytes_per_frame": sum(map(len, jpgs)) // len(jpgs), "segments_per_frame": info.n_segments}
            if not a.device_only:
                host = video.read_avi(path)[0]
                case["device_equals_host"] = bool(torch.equal(dev.cpu(), torch.from_numpy(host)))
                t_host, t_dev = [], []
                for _ in range(a.reps):  # alternate the two routes
                    t_host += timed(lambda: torch.from_numpy(video.read_avi(path)[0]).cuda(), 1)
                    t_dev += timed(lambda: video.read_avi_device(path, "cuda"), 1)
                for k, t in (("host_read_avi", t_host), ("device_read_avi_device", t_dev)):
                    case[k + "_ms_per_frame"] = {"median": 1e3 * statistics.median(t) / a.frames,
                                                 "min": 1e3 * min(t) / a.frames, "max": 1e3 * max(t) / a.frames}
                # the device route without file reading and header parsing: upload + kernels
                packed = video.pack_frames(jpgs)
                up = lambda x: torch.from_numpy(x).cuda()
                scans = np.frombuffer(packed[0], np.uint8).copy()
                from latentsync_amd import ops

                def kernels():
                    data = up(scans)
                    ops.mjpeg_decode(data, up(packed[1]), packed[5], packed[6], up(packed[2]), up(packed[3]), packed[4])
                t = timed(kernels, a.reps + 1)[1:]
                case["upload_and_kernels_ms_per_frame"] = {"median": 1e3 * statistics.median(t) / a.frames}
            else:
                timed(lambda: video.read_avi_device(path, "cuda"), a.reps)
            res["cases"][name] = case
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
