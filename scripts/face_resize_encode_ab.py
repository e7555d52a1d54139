"""Cost of the ingest face resize in the encode graph, configs[1] shape (16 frames x 48
windows, R = 256): the plain engine (faces at R; the encode graph as it is without the
resize) against an engine fed 2R faces (WindowEngine(face_resolution=512)), both captured
in one process and replayed alternately, timed with device events; then the
ops.resize_faces_u8 call alone on the same 768 faces.

    python scripts/face_resize_encode_ab.py [out.json]     # default bench_out/face_resize_encode_ab.json
"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bench import SCHED_CFG, synthetic_window  # noqa: E402
from latentsync_amd import ops  # noqa: E402
from latentsync_amd.config import STAGE2_MODEL  # noqa: E402
from latentsync_amd.pipeline import WindowEngine, load_fixed_mask  # noqa: E402
from latentsync_amd.scheduler import DDIMScheduler  # noqa: E402
from latentsync_amd.unet import UNet3DConditionModel  # noqa: E402
from latentsync_amd.vae import AutoencoderKL  # noqa: E402

ROUNDS, REPLAYS, CALLS = 5, 5, 20


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "bench_out", "face_resize_encode_ab.json")
    dev = torch.device("cuda:0")
    F_, R, S, nw, steps = 16, 256, 512, 48, 20
    h = R // 8
    unet = UNet3DConditionModel(**STAGE2_MODEL).init_weights(41).to(dev).eval()
    vae = AutoencoderKL().init_weights(51).to(dev)
    mask = load_fixed_mask(R).to(dev)
    cd = unet.config.cross_attention_dim
    faces, audio, init, em, er = synthetic_window(F_ * nw, R, h, cd, 1000, dev)
    big = synthetic_window(F_ * nw, S, h, cd, 1000, dev)[0]
    plain = WindowEngine(unet, vae, DDIMScheduler(**SCHED_CFG), F_, R, steps, 1.0, windows=nw)
    resizing = WindowEngine(unet, vae, DDIMScheduler(**SCHED_CFG), F_, R, steps, 1.0, windows=nw, face_resolution=S)
    plain.load(faces, mask, audio, init, em, er)
    resizing.load(big, mask, audio, init, em, er)
    for eng in (plain, resizing):
        eng.capture()
        for _ in range(3):
            eng.graphs[0].replay()
    torch.cuda.synchronize()
    res = {"shape": f"{F_ * nw} faces, {S}x{S} -> {R}x{R}", "encode_plain_ms": [], "encode_resizing_ms": [],
           "resize_call_ms": []}
    for _ in range(ROUNDS):
        res["encode_plain_ms"].append(round(timed(plain.graphs[0].replay, REPLAYS), 3))
        res["encode_resizing_ms"].append(round(timed(resizing.graphs[0].replay, REPLAYS), 3))
    out = torch.empty((F_ * nw, 3, R, R), dtype=torch.uint8, device=dev)
    for _ in range(3):
        ops.resize_faces_u8(big, R, R, out=out)
    for _ in range(ROUNDS):
        res["resize_call_ms"].append(round(timed(lambda: ops.resize_faces_u8(big, R, R, out=out), CALLS), 4))
    res["bytes_in"], res["bytes_out"] = big.numel(), out.numel()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
