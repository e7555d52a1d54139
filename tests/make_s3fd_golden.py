"""Writes tests/golden/s3fd_{net,post,track}.npz: the REFERENCE's S3FD detector
(eval/detectors/s3fd: S3FDNet, Detect, PriorBox, S3FD.detect_faces, nms_) and
SyncNetDetector.track_face (eval/syncnet_detect.py) in fp32 on the CPU, on the seeded weights,
frames, synthetic head maps and tracker cases of tests/s3fd_ref.py.

    LATENTSYNC_REFERENCE=<reference checkout> python tests/make_s3fd_golden.py

The reference is imported at run time only, with stub modules for cv2, torchvision and
scenedetect in sys.modules.  cv2.resize in the stub is the project's OWN restatement
(s3fd_ref.resize_fx_u8), and the fixtures record that (resize_source): parity with cv2 itself
is unpinned.  Weights and inputs are functions of their seeds, so no fixture stores them.

  * s3fd_net.npz: two 304 x 432 frames at scale 0.25 (a 76 x 108 input, 697 priors) through the
    reference S3FDNet: every ReLU output and the three L2Norm outputs (whole up to 6144 elements,
    above that the RMS and SUBSAMPLE fixed positions), the six raw head maps as loc | conf NHWC,
    and PriorBox's table.  Asserted while generating: every stage's RMS lies in [0.1, 100] and
    at least 20 % of every ReLU output is non-zero.
  * s3fd_post.npz: the discrete stages on identical fp32 inputs.  Forward hooks that return a
    value replace the outputs of loc[i] / conf[i] by s3fd_ref.synthetic_heads; the reference's
    own forward tail, Detect and detect_faces produce the expected result.  Three cases (697
    priors; 5373 priors that are all candidates, for the exact top-5000 cut; no candidate).
    Seeds are searched until no score is within 1e-4 of 0.05 or conf_th, no IoU either NMS
    pass compares is within 1e-4 of its threshold, and the float64 restatement in s3fd_ref
    reproduces the reference's rows; the kept prior indices stored are the restatement's.
  * s3fd_track.npz: track_face on s3fd_ref.tracker_cases().
Not collected by pytest.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import s3fd_ref as R  # noqa: E402
from latentsync_amd import s3fd  # noqa: E402

CONF_TH = 0.9
POST_CASES = {  # name -> (image size, scale, synthetic_heads keywords, first seed)
    "work": (R.WORK_HW, R.WORK_SCALE, dict(), 100),
    "big": (R.BIG_INPUT, 1.0, None, 200),  # s3fd_ref.clustered_heads
    "none": (R.WORK_HW, R.WORK_SCALE, dict(lo=0.001, hi=0.04), 300),
}


def import_reference():
    ref = os.environ.get("LATENTSYNC_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set LATENTSYNC_REFERENCE to a checkout of the reference")
    sys.dont_write_bytecode = True
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1

    def resize(image, dsize=None, fx=0, fy=0, interpolation=1):
        assert tuple(dsize) == (0, 0) and fx == fy and interpolation == cv2.INTER_LINEAR
        return R.resize_fx_u8(image, fx)

    cv2.resize = resize
    sys.modules["cv2"] = cv2
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    for name, attr in (("scenedetect", None), ("scenedetect.video_manager", "VideoManager"),
                       ("scenedetect.scene_manager", "SceneManager"), ("scenedetect.stats_manager", "StatsManager"),
                       ("scenedetect.detectors", "ContentDetector")):
        m = types.ModuleType(name)
        if attr:
            setattr(m, attr, None)
        sys.modules.setdefault(name, m)
    sys.path.insert(1, ref)
    from eval.detectors.s3fd import S3FD
    from eval.detectors.s3fd.nets import S3FDNet
    from eval.syncnet_detect import SyncNetDetector
    return S3FD, S3FDNet, SyncNetDetector


def _store(out, label, t, seed, relu):
    flat = t.reshape(-1)
    rms = float(flat.double().pow(2).mean().sqrt())
    alive = float((flat != 0).double().mean())
    assert 0.1 <= rms <= 100.0, (label, rms)
    assert not relu or alive >= 0.2, (label, alive)
    out[label + "_shape"] = np.array(t.shape, dtype=np.int64)
    out[label + "_rms"] = np.float64(rms)
    idx = R.subsample_index(flat.numel(), seed)
    if idx is None:
        out[label] = flat.numpy().copy()
    else:
        out[label] = flat[idx].numpy().copy()
        out[label + "_idx"] = idx.numpy().astype(np.int32)
    print(f"{label}: {tuple(t.shape)} rms {rms:.3f} alive {alive:.2f}")


@torch.no_grad()
def generate_net(S3FDNet):
    net = S3FDNet(device="cpu").float().eval()
    keys = list(net.state_dict().keys())
    net.load_state_dict(R.case_weights(), strict=True)
    x = R.prep(R.case_frames(), R.WORK_SCALE)
    relu, l2, loc, conf = [], [], {}, {}
    hooks = []
    for m in net.vgg:
        if isinstance(m, torch.nn.ReLU):
            hooks.append(m.register_forward_hook(lambda mod, i, o: relu.append(o.clone())))
    for m in net.extras:  # forward applies F.relu to these itself
        hooks.append(m.register_forward_hook(lambda mod, i, o: relu.append(torch.relu(o.clone()))))
    for m in (net.L2Norm3_3, net.L2Norm4_3, net.L2Norm5_3):
        hooks.append(m.register_forward_hook(lambda mod, i, o: l2.append(o.clone())))
    for i in range(6):
        hooks.append(net.loc[i].register_forward_hook(lambda mod, inp, o, i=i: loc.__setitem__(i, o.clone())))
        hooks.append(net.conf[i].register_forward_hook(lambda mod, inp, o, i=i: conf.__setitem__(i, o.clone())))
    net(x)
    for h in hooks:
        h.remove()
    assert len(relu) == R.N_RELU and len(l2) == 3
    out = {"keys": np.array(keys), "seed": np.int64(R.NET_SEED), "frame_seed": np.int64(R.FRAME_SEED),
           "resize_source": np.array("s3fd_ref.resize_fx_u8"), "input_shape": np.array(x.shape, dtype=np.int64)}
    for j, t in enumerate(relu):
        _store(out, f"relu_{j}", t, R.NET_SEED * 100 + j, True)
    for j, t in enumerate(l2):
        _store(out, f"l2norm_{j}", t, R.NET_SEED * 100 + 50 + j, False)
    for j in range(6):
        _store(out, f"head_{j}", torch.cat([loc[j], conf[j]], 1).permute(0, 2, 3, 1).contiguous(), 0, False)
    out["priors"] = net.priors.numpy().astype(np.float32)
    assert out["priors"].shape == (697, 4), out["priors"].shape
    path = os.path.join(HERE, "golden", "s3fd_net.npz")
    np.savez(path, **out)
    print("s3fd_net:", len(keys), "keys,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)
    return keys


@torch.no_grad()
def generate_post(S3FD, S3FDNet):
    net = S3FDNet(device="cpu").float().eval()
    net.load_state_dict(R.case_weights(), strict=True)
    det = S3FD.__new__(S3FD)
    det.device, det.net = "cpu", net
    out = {"resize_source": np.array("s3fd_ref.resize_fx_u8"), "conf_th": np.float64(CONF_TH)}
    for name, (hw, scale, kw, seed0) in POST_CASES.items():
        h, w = R.cv_round(hw[0] * scale), R.cv_round(hw[1] * scale)
        sizes = s3fd.feature_map_sizes(h, w)
        image = np.zeros((hw[0], hw[1], 3), dtype=np.uint8)
        for seed in range(seed0, seed0 + 64):
            heads = R.synthetic_heads(seed, sizes, n=1, **kw) if kw is not None else R.clustered_heads(seed, (h, w))[0]
            hooks = []
            for i in range(6):
                nchw = heads[i].permute(0, 3, 1, 2).contiguous()
                hooks.append(net.loc[i].register_forward_hook(lambda m, a, o, t=nchw: t[:, :4].clone()))
                hooks.append(net.conf[i].register_forward_hook(lambda m, a, o, t=nchw: t[:, 4:].clone()))
            rows = net(torch.zeros(1, 3, h, w))[0, 1].numpy()          # (750, 5)
            final = det.detect_faces(image, conf_th=CONF_TH, scales=[scale])  # (k, 5) float64
            for hk in hooks:
                hk.remove()
            priors = net.priors.numpy()
            assert np.array_equal(priors, s3fd.prior_boxes(h, w, sizes)), "prior table differs from the reference's"
            d = R.detect_ref(heads, priors)
            count = int((rows[:, 0] > 0).sum())
            n = R.nms_ref(rows, CONF_TH, hw[1], hw[0])
            margins = dict(score=d["score_margin"], iou=d["iou_margin"], score2=n["score_margin"], iou2=n["iou_margin"])
            same = (count == d["idx"].size and np.allclose(rows[:count, 0], d["scores"], rtol=0, atol=1e-6) and
                    np.allclose(rows[:count, 1:], d["boxes"], rtol=1e-5, atol=1e-7) and
                    final.shape == n["boxes"].shape and np.allclose(final, n["boxes"], rtol=1e-12, atol=0))
            ok = same and d["score_margin"] >= R.MARGIN_SCORE and n["score_margin"] >= R.MARGIN_SCORE and \
                d["iou_margin"] >= R.MARGIN_IOU and n["iou_margin"] >= R.MARGIN_IOU
            print(f"{name} seed {seed}: P {priors.shape[0]} candidates {d['n_cand']} kept {count} final {final.shape[0]} "
                  f"same {same} margins {margins}")
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed satisfies the margins")
        if name == "big":
            assert d["n_cand"] == priors.shape[0] > 5000
            ncell = (h // R.CLUSTER_CELL) * (w // R.CLUSTER_CELL)
            assert count == ncell - R.CLUSTER_FORCED < 750, (count, ncell)  # the cut is what removes the forced cells
        if name == "none":
            assert d["n_cand"] == 0 and count == 0 and final.shape[0] == 0
        out.update({f"{name}_seed": np.int64(seed), f"{name}_hw": np.array(hw, dtype=np.int64),
                    f"{name}_scale": np.float64(scale), f"{name}_count": np.int64(count),
                    f"{name}_idx": d["idx"].astype(np.int32), f"{name}_rows": rows[:count].astype(np.float32),
                    f"{name}_final": final.astype(np.float64), f"{name}_final_idx": n["idx"].astype(np.int32),
                    f"{name}_n_cand": np.int64(d["n_cand"])})
    path = os.path.join(HERE, "golden", "s3fd_post.npz")
    np.savez(path, **out)
    print("s3fd_post:", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


def generate_track(SyncNetDetector):
    out = {}
    for name, dets in R.tracker_cases().items():
        tracks = SyncNetDetector.track_face(None, copy.deepcopy(dets))
        out[f"{name}_n"] = np.int64(len(tracks))
        for j, t in enumerate(tracks):
            out[f"{name}_{j}_frame"] = np.asarray(t["frame"], dtype=np.int64)
            out[f"{name}_{j}_bbox"] = np.asarray(t["bbox"], dtype=np.float64)
        print(f"track {name}: {len(tracks)} tracks", [(int(t['frame'][0]), int(t['frame'][-1])) for t in tracks])
    path = os.path.join(HERE, "golden", "s3fd_track.npz")
    np.savez(path, **out)
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    S3FD_, Net_, Det_ = import_reference()
    generate_track(Det_)
    generate_net(Net_)
    generate_post(S3FD_, Net_)
