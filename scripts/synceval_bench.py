"""Times one classic-SyncNet evaluation (latentsync_amd/synceval.py) of a 250-frame crop track.

    python scripts/synceval_bench.py                      # SyncNetEval.evaluate on the HIP device
    python scripts/synceval_bench.py --reference <DIR>    # the reference's S, fp32, host cores

Seeded weights (tests/synceval_ref.py, case B), random 224 x 224 frames, noise audio.  The device
figure is the wall time of evaluate(frames=, audio=) -- the audio upload and the copy of the 31
means included -- median of 5 runs after a warm-up.  The reference figure runs S as
syncnet_eval.evaluate batches it (20 windows a batch) plus calc_pdist; cv2 and
python_speech_features are stubbed (S does not use them) and the MFCC comes from the float64
oracle.  The line is printed and written to bench_out/synceval_time.log or
bench_out/synceval_ref_cpu_time.log; DESIGN.md section 4.7 records both.
"""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import synceval_ref as R  # noqa: E402


def report(name, line):
    print(line)
    out = os.path.join(REPO, "bench_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, name), "w") as f:
        f.write(line + "\n")


def device(n):
    from latentsync_amd import synceval
    net = synceval.SyncNetEval().load_state_dict(R.case_weights("B")).to("cuda").eval()
    frames = torch.randint(0, 256, (n, 224, 224, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    audio = torch.from_numpy((3000 * np.random.RandomState(1).randn(n * 640) / 32768).astype(np.float32))
    res = net.evaluate(frames=frames, audio=audio)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = net.evaluate(frames=frames, audio=audio)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    report("synceval_time.log", f"evaluate on {n} frames ({n - 5} windows): wall incl. host copies, 5 runs: "
           + ", ".join(f"{t * 1e3:.1f}" for t in ts) + f" ms; median {sorted(ts)[2] * 1e3:.1f} ms; result {res}")


@torch.no_grad()
def reference(n, ref_dir):
    for name in ("cv2", "python_speech_features"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(1, ref_dir)
    from eval.syncnet.syncnet import S
    from eval.syncnet.syncnet_eval import calc_pdist
    net = S().float().eval()
    net.load_state_dict(R.case_weights("B"))
    imtv = torch.randint(0, 256, (1, 3, n, 224, 224), generator=torch.Generator().manual_seed(1)).float()
    audio = np.rint(3000 * np.random.RandomState(1).randn(n * 640))
    t0 = time.time()
    mf, _ = R.mfcc_oracle(audio)
    cct = torch.from_numpy(mf).float()[None, None]
    last = n - 5
    im_feat, cc_feat = [], []
    for i in range(0, last, 20):
        rng = range(i, min(last, i + 20))
        im_feat.append(net.forward_lip(torch.cat([imtv[:, :, v:v + 5] for v in rng], 0)))
        cc_feat.append(net.forward_aud(torch.cat([cct[:, :, :, v * 4:v * 4 + 20] for v in rng], 0)))
    d = calc_pdist(torch.cat(im_feat), torch.cat(cc_feat), vshift=15)
    torch.mean(torch.stack(d, 1), 1)
    report("synceval_ref_cpu_time.log", f"reference S fp32 on the host: {n} frames, {last} windows, "
           f"{time.time() - t0:.2f} s on {torch.get_num_threads()} threads ({os.cpu_count()} cores)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--reference", metavar="DIR", default=None, help="a checkout of the reference: time its S on the host")
    a = ap.parse_args()
    reference(a.frames, a.reference) if a.reference else device(a.frames)
