"""The host side of the S3FD detector (latentsync_amd/s3fd.py) and the CPU restatement the GPU
tests lean on (tests/s3fd_ref.py), against the fixtures tests/make_s3fd_golden.py wrote from the
reference: the tracker, the prior table, the state dict, the bf16 restatement's error (REF_ERR,
which the GPU model test imports), the restated post-processing, and the pipeline's and the
server's argument handling with fakes."""
import copy
import os

import numpy as np
import pytest
import torch

import s3fd_ref as R
from conftest import golden
from latentsync_amd import s3fd
from latentsync_amd import serve as S
from latentsync_amd.pipeline import LipsyncPipeline

# max |bf16 restatement - golden| / RMS(golden), measured on the CPU; the device is allowed 2 x
# (tests/test_gpu_s3fd_model.py imports this table)
REF_ERR = dict(
    relu=[0.0128, 0.0171, 0.02, 0.0208, 0.021, 0.0208, 0.0239, 0.0249, 0.0319, 0.0296, 0.0314, 0.0351, 0.0446, 0.0447,
          0.038, 0.0355, 0.0367, 0.039, 0.039],
    l2norm=[0.0306, 0.0356, 0.0343],
    head=[0.0117, 0.0274, 0.0245, 0.0259, 0.0242, 0.013])


def ref_err(label):
    kind, j = label.rsplit("_", 1)
    return REF_ERR[kind][int(j)]


# ---------------------------------------------------------------- tracker
def test_track_faces_matches_the_reference():
    g = golden("s3fd_track.npz")
    cases = R.tracker_cases()
    expect = dict(short_gaps=1, long_gap=2, two_faces=2, too_short=0, small_face=1)
    for name, dets in cases.items():
        before = copy.deepcopy(dets)
        tracks = s3fd.track_faces(dets)
        assert dets == before, "track_faces consumed its argument"
        assert len(tracks) == int(g[f"{name}_n"]) == expect[name], name
        for j, t in enumerate(tracks):
            assert np.array_equal(t["frame"], g[f"{name}_{j}_frame"]), (name, j)
            assert t["bbox"].shape == g[f"{name}_{j}_bbox"].shape
            np.testing.assert_allclose(t["bbox"], g[f"{name}_{j}_bbox"], rtol=1e-12, atol=1e-9)
    # what the cases are about
    t = s3fd.track_faces(cases["short_gaps"])[0]
    assert t["frame"][0] == 0 and t["frame"][-1] == 139 and len(t["frame"]) == 140  # the gaps are filled
    a, b = s3fd.track_faces(cases["long_gap"])
    assert (a["frame"][-1], b["frame"][0]) == (69, 97)
    t = s3fd.track_faces(cases["small_face"])[0]
    assert np.mean(t["bbox"][:, 2] - t["bbox"][:, 0]) > 100


def test_track_faces_thresholds():
    dets = R.tracker_cases()["too_short"]
    assert s3fd.track_faces(dets) == []
    assert len(s3fd.track_faces(dets, min_track=49)) == 1
    assert s3fd.track_faces(dets, min_track=49, min_face_size=200) == []
    faces = s3fd.faces_from_detections([np.array([[1.0, 2.0, 3.0, 4.0, 0.95]]), np.zeros((0, 5))])
    assert faces == [[{"frame": 0, "bbox": [1.0, 2.0, 3.0, 4.0], "conf": 0.95}], []]


# ---------------------------------------------------------------- priors, state dict
def test_prior_table_bit_for_bit():
    g = golden("s3fd_net.npz")
    h, w = int(g["input_shape"][2]), int(g["input_shape"][3])
    assert (h, w) == (76, 108)
    sizes = s3fd.feature_map_sizes(h, w)
    assert sizes == [(19, 27), (10, 14), (5, 7), (2, 3), (1, 2), (1, 1)]
    p = s3fd.prior_boxes(h, w, sizes)
    assert p.shape == (697, 4) and p.dtype == np.float32
    assert np.array_equal(p.view(np.uint32), g["priors"].view(np.uint32))
    assert s3fd.feature_map_sizes(*R.BIG_INPUT) == [(48, 84), (24, 42), (12, 21), (6, 10), (3, 5), (2, 3)]


def test_state_dict_keys_and_round_trip():
    g = golden("s3fd_net.npz")
    assert list(s3fd.param_shapes()) == [str(k) for k in g["keys"]]
    sd = R.case_weights()
    net = s3fd.S3FDNet()
    with pytest.raises(RuntimeError, match="no weights"):
        net.state_dict()
    net.load_state_dict(sd)
    back = net.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match="missing keys"):
        net.load_state_dict({k: v for k, v in sd.items() if k != "L2Norm4_3.weight"})
    with pytest.raises(RuntimeError, match="unexpected keys"):
        net.load_state_dict(dict(sd, extra=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="shape"):
        net.load_state_dict(dict(sd, **{"vgg.31.weight": torch.zeros(1024, 512, 1, 1)}))
    with pytest.raises(RuntimeError, match="HIP device only"):
        net.head_maps(torch.zeros(1, 76, 108, 8, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError):
        net.train()
    assert s3fd.PATH_WEIGHT == "checkpoints/auxiliary/sfd_face.pth"


def test_chunking_keeps_conv1_2_under_the_budget():
    det = s3fd.S3FD.__new__(s3fd.S3FD)
    assert det.chunk_frames(180, 320) * 180 * 320 * 64 * 2 <= s3fd.ACT_BUDGET_BYTES
    assert (det.chunk_frames(180, 320) + 1) * 180 * 320 * 64 * 2 > s3fd.ACT_BUDGET_BYTES
    assert det.chunk_frames(4096, 4096) == 1


# ---------------------------------------------------------------- resize, restatement
def test_resize_restatement_sizes_and_copy():
    img = R.case_frames(1, (303, 430))[0].numpy()
    out = R.resize_fx_u8(img, 0.25)
    assert out.shape == (76, 108, 3)  # cvRound(75.75) = 76, cvRound(107.5) = 108: half to even
    assert np.array_equal(R.resize_fx_u8(img, 1.0), img)
    # at 1 / 4 the sample point lies between source pixels 4 d + 1 and 4 d + 2 on both axes
    v = img.astype(np.int64)
    want = v[1:300:4, 1:428:4] + v[1:300:4, 2:428:4] + v[2:300:4, 1:428:4] + v[2:300:4, 2:428:4]
    assert want.shape == (75, 107, 3)
    assert np.abs(out[:75, :107].astype(np.int64) * 4 - want).max() <= 4
    x = R.prep(torch.from_numpy(img)[None], 0.25)
    assert tuple(x.shape) == (1, 3, 76, 108)
    assert float(x[0, 0].max()) <= 255 - 123 and float(x[0, 2].min()) >= -104


def test_bf16_restatement_against_golden():
    """Measures REF_ERR: the error of the bf16-rounding restatement against the reference's fp32
    golden, per tensor; the GPU test allows the device twice that.  The fp32 restatement must
    reproduce the golden to fp32 accuracy, which pins the restatement's structure."""
    g = golden("s3fd_net.npz")
    assert str(g["resize_source"]) == "s3fd_ref.resize_fx_u8"
    sd, x = R.case_weights(), R.prep(R.case_frames(), R.WORK_SCALE)
    assert tuple(x.shape) == tuple(g["input_shape"])
    for bf16 in (False, True):
        o = R.forward(sd, x, bf16=bf16)
        for label, e in R.golden_errors(g, o["relu"], o["l2norm"], o["heads"]).items():
            print(f"bf16={bf16} {label}: err / rms {e:.3g}")
            if bf16:
                want = ref_err(label)
                assert 0.5 * want <= e <= 1.05 * want, (label, e, want)  # REF_ERR is this figure
            else:
                assert e < 1e-4, (label, e)


@pytest.mark.parametrize("name", ("work", "big", "none"))
def test_restated_postprocessing_reproduces_the_reference(name):
    """detect_ref / nms_ref (float64) against the rows the reference's own Detect and detect_faces
    produced on the same synthetic head maps, and the margins the exact GPU test rests on."""
    g = golden("s3fd_post.npz")
    hw, scale, seed = tuple(int(v) for v in g[f"{name}_hw"]), float(g[f"{name}_scale"]), int(g[f"{name}_seed"])
    heads, priors = post_case(name)
    d = R.detect_ref(heads, priors)
    rows = g[f"{name}_rows"]
    assert d["n_cand"] == int(g[f"{name}_n_cand"]) and d["idx"].size == int(g[f"{name}_count"]) == rows.shape[0]
    assert np.array_equal(d["idx"], g[f"{name}_idx"])
    np.testing.assert_allclose(d["scores"], rows[:, 0], rtol=0, atol=1e-6)
    np.testing.assert_allclose(d["boxes"], rows[:, 1:], rtol=1e-5, atol=1e-7)
    assert d["score_margin"] >= R.MARGIN_SCORE and d["iou_margin"] >= R.MARGIN_IOU
    assert d["score_gap"] > 0.5 * (0.04 if name == "none" else 0.9) / priors.shape[0]
    full = np.zeros((750, 5), dtype=np.float32)
    full[:rows.shape[0]] = rows
    n = R.nms_ref(full, float(g["conf_th"]), hw[1], hw[0])
    assert n["score_margin"] >= R.MARGIN_SCORE and n["iou_margin"] >= R.MARGIN_IOU
    assert np.array_equal(n["idx"], g[f"{name}_final_idx"])
    np.testing.assert_allclose(n["boxes"], g[f"{name}_final"], rtol=1e-12, atol=0)
    if name == "big":
        assert d["n_cand"] == priors.shape[0] == 5373 and d["idx"].size < 750
        # without the cut to the 5000 highest the forced cells would each add a box
        cells = (192 // R.CLUSTER_CELL) * (336 // R.CLUSTER_CELL)
        assert d["idx"].size == cells - R.CLUSTER_FORCED
    if name == "none":
        assert d["idx"].size == 0 and n["idx"].size == 0
    assert seed >= 100 and scale in (0.25, 1.0)


def post_case(name):
    """(head maps, prior table) of a post-processing case of tests/golden/s3fd_post.npz."""
    g = golden("s3fd_post.npz")
    hw, scale, seed = tuple(int(v) for v in g[f"{name}_hw"]), float(g[f"{name}_scale"]), int(g[f"{name}_seed"])
    h, w = R.cv_round(hw[0] * scale), R.cv_round(hw[1] * scale)
    sizes = s3fd.feature_map_sizes(h, w)
    if name == "big":
        heads = R.clustered_heads(seed, (h, w))[0]
    else:
        heads = R.synthetic_heads(seed, sizes, n=1, **(dict(lo=0.001, hi=0.04) if name == "none" else {}))
    return heads, s3fd.prior_boxes(h, w, sizes)


# ---------------------------------------------------------------- pipeline and server with fakes
class _FakeNet:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def evaluate(self, frames=None, audio=None):
        self.calls.append((tuple(frames.shape), int(audio.numel())))
        k = len(self.calls)
        return (3 * k, 7.0 + k, 2.0 * k)


class _FakeDetector:
    def __init__(self, dets):
        self.dets, self.seen = dets, None

    def detect(self, frames_u8, conf_th=0.9, scale=0.25):
        self.seen = (tuple(frames_u8.shape), conf_th, scale)
        return self.dets


def _planted(n, tracks):
    """Per-frame (k, 5) arrays holding each (x0, y0, size, first, last) track's drifting box."""
    out = []
    for i in range(n):
        rows = [[x0 + 0.5 * i, y0, x0 + 0.5 * i + sz, y0 + sz, 0.97] for (x0, y0, sz, a, b) in tracks if a <= i <= b]
        out.append(np.array(rows, dtype=np.float64).reshape(-1, 5))
    return out


def test_sync_evaluation_tracks_with_fakes(tmp_path, monkeypatch):
    from latentsync_amd import synceval
    from test_syncnet_pipeline_host import _write_wav
    n = 120
    _write_wav(tmp_path / "a.wav", n / 25)
    crops = []

    def crop_track(frames, boxes):
        crops.append((frames.shape[0], np.asarray(boxes).shape))
        return torch.zeros((frames.shape[0], 224, 224, 3), dtype=torch.uint8)

    monkeypatch.setattr(synceval, "crop_track", crop_track)
    pipe = LipsyncPipeline.__new__(LipsyncPipeline)
    frames = torch.zeros((n, 300, 400, 3), dtype=torch.uint8)
    det = _FakeDetector(_planted(n, [(20.0, 30.0, 150.0, 0, 99), (220.0, 40.0, 140.0, 40, 119)]))
    net = _FakeNet()
    got = pipe.sync_evaluation_tracks(net, det, frames, str(tmp_path / "a.wav"))
    assert det.seen == ((n, 300, 400, 3), 0.9, 0.25)
    assert [(int(t["frame"][0]), int(t["frame"][-1])) for t in pipe.last_face_tracks] == [(0, 99), (40, 119)]
    assert crops == [(100, (100, 4)), (80, (80, 4))]
    assert net.calls == [((100, 224, 224, 3), 64000), ((80, 224, 224, 3), 51200)]  # (last + 1 - first) / 25 s each
    # int(fmean([3, 6])) = 4, fmean([8, 9]), fmean([2, 4])
    assert got == (4, 8.5, 3.0) == (pipe.last_av_offset, pipe.last_lse_d, pipe.last_lse_c)
    # a track of at most min_track detections does not count; with none the reference raises
    with pytest.raises(ValueError, match="Face not detected"):
        pipe.sync_evaluation_tracks(net, _FakeDetector(_planted(n, [(20.0, 30.0, 150.0, 0, 49)])), frames,
                                    str(tmp_path / "a.wav"))
    assert pipe.last_face_tracks == []
    got = pipe.sync_evaluation_tracks(_FakeNet(), _FakeDetector(_planted(n, [(20.0, 30.0, 150.0, 0, 49)])), frames,
                                      str(tmp_path / "a.wav"), min_track=20)
    assert got == (3, 8.0, 2.0)
    with pytest.raises(ValueError, match="25 frames/s"):
        pipe.sync_evaluation_tracks(net, det, frames, str(tmp_path / "a.wav"), video_fps=30)
    with pytest.raises(ValueError, match="detection lists"):
        pipe.sync_evaluation_tracks(net, _FakeDetector([]), frames, str(tmp_path / "a.wav"))


def test_call_argument_handling(tmp_path):
    from test_syncnet_pipeline_host import _pipe
    pipe, kw = _pipe(tmp_path)
    out = str(tmp_path / "out.npz")
    net, det = _FakeNet(), _FakeDetector([])
    with pytest.raises(ValueError, match="needs face_boxes"):
        pipe(video_out_path=out, sync_eval=net, **kw)
    with pytest.raises(ValueError, match="detect\\(frames_u8"):
        pipe(video_out_path=out, sync_eval=net, face_detector=object(), **kw)
    with pytest.raises(ValueError, match="faces_only=True.*detector"):
        pipe(video_out_path=out, sync_eval=net, face_detector=det, **kw)
    with pytest.raises(ValueError, match="25 frames/s"):
        pipe(video_out_path=out, sync_eval=net, face_detector=det, video_fps=30, **dict(kw, faces_only=False))
    with pytest.raises(ValueError, match="no restored frames to detect faces in"):
        pipe(video_out_path=out, sync_eval=net, face_detector=det, **dict(kw, faces_only=False))
    # face_boxes= wins: its own path answers, the detector is never asked
    with pytest.raises(ValueError, match="face_boxes are in frame coordinates"):
        pipe(video_out_path=out, sync_eval=net, face_detector=det, face_boxes=np.zeros((16, 4)), **kw)
    assert det.seen is None
    # a detector without sync_eval= changes nothing
    pipe(video_out_path=out, face_detector=det, **kw)
    assert det.seen is None and "av_offset" not in np.load(out).files


class _StubPipeline:
    def __init__(self):
        self.calls = []

    def __call__(self, **kw):
        self.calls.append(kw)
        if "sync_eval" in kw:
            self.last_av_offset, self.last_lse_d, self.last_lse_c = -2, 7.25, 3.5
        open(kw["video_out_path"], "wb").close()


def test_run_job_reports_the_gate(tmp_path):
    from test_syncnet_pipeline_host import REPLY_KEYS, _job_files
    pipe = _StubPipeline()
    reply = S.run_job(pipe, _job_files(tmp_path), str(tmp_path), str(tmp_path / "results"), 256)
    assert set(reply) == REPLY_KEYS and "sync_eval" not in pipe.calls[0] and "face_detector" not in pipe.calls[0]
    # one of the two alone is not a gate
    pipe = _StubPipeline()
    pipe.sync_eval = object()
    reply = S.run_job(pipe, _job_files(tmp_path), str(tmp_path), str(tmp_path / "results"), 256)
    assert set(reply) == REPLY_KEYS and "sync_eval" not in pipe.calls[0]
    pipe = _StubPipeline()
    pipe.sync_eval, pipe.face_detector = object(), object()
    reply = S.run_job(pipe, _job_files(tmp_path), str(tmp_path), str(tmp_path / "results"), 256)
    assert set(reply) == REPLY_KEYS | {"av_offset", "lse_d", "lse_c"}
    assert (reply["av_offset"], reply["lse_d"], reply["lse_c"]) == (-2, 7.25, 3.5)
    assert isinstance(reply["av_offset"], int) and isinstance(reply["lse_d"], float)
    assert pipe.calls[0]["sync_eval"] is pipe.sync_eval and pipe.calls[0]["face_detector"] is pipe.face_detector


def test_worker_environment_names():
    src = open(os.path.join(os.path.dirname(S.__file__), "serve.py")).read()
    assert "LATENTSYNC_SYNCEVAL_CKPT" in src and "LATENTSYNC_S3FD_CKPT" in src
