"""LipsyncPipeline.__call__(..., sync_eval=net, face_detector=det) on the tiny pipeline of
tests/test_gpu_synceval_pipeline.py: the detector runs on the frames about to be written, the
boxes are tracked and every track is evaluated, as eval_sync_conf.syncnet_eval does.  A stub
detector with planted boxes puts tracking, per-track evaluation and aggregation under test
without a trained detector; one run uses the real S3FD on seeded weights."""
import numpy as np
import pytest
import torch

import s3fd_ref as R
from latentsync_amd import s3fd
from test_gpu_synceval_pipeline import H, N, W, rig  # noqa: F401  (the module-scoped tiny pipeline)

pytestmark = pytest.mark.gpu
TRACK_ARGS = dict(min_track=10, min_face_size=30)  # a second of 120 x 160 frames: the defaults (50, 100) fit no track here


class PlantedDetector:
    """detect() returns one drifting box per frame, none on `missing` frames."""

    def __init__(self, missing=(7, 8, 30)):
        self.missing, self.calls = set(missing), []

    def box(self, i):
        return [60.0 + 0.2 * i, 35.0 + 0.1 * i, 100.0 + 0.2 * i, 85.0 + 0.1 * i]

    def detect(self, frames_u8, conf_th=0.9, scale=0.25):
        assert frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and tuple(frames_u8.shape[1:]) == (H, W, 3)
        self.calls.append((frames_u8.shape[0], conf_th, scale))
        return [np.zeros((0, 5)) if i in self.missing else np.array([self.box(i) + [0.95]])
                for i in range(frames_u8.shape[0])]


def test_detector_path_equals_face_boxes_of_the_track(rig):  # noqa: F811
    pipe, net, call, _, _, _ = rig
    det = PlantedDetector()
    res = np.load(call("detected.npz", sync_eval=net, face_detector=det, face_track_args=TRACK_ARGS))
    n = res["frames"].shape[0]
    assert det.calls == [(n, 0.9, 0.25)]
    tracks = pipe.last_face_tracks
    assert len(tracks) == 1 and np.array_equal(tracks[0]["frame"], np.arange(n))
    want = np.array([det.box(i) for i in range(n)])  # the drift is linear: the interpolated rows are the planted ones
    np.testing.assert_allclose(tracks[0]["bbox"], want, rtol=0, atol=1e-9)
    got = (pipe.last_av_offset, pipe.last_lse_d, pipe.last_lse_c)
    assert isinstance(got[0], int) and int(res["av_offset"]) == got[0]
    assert float(res["lse_d"]) == float(np.float32(got[1])) and float(res["lse_c"]) == float(np.float32(got[2]))
    # the same clip through face_boxes= with the track's boxes
    boxes = np.full((N, 4), np.nan)
    boxes[:n] = tracks[0]["bbox"]
    boxes[n:] = tracks[0]["bbox"][-1]
    res2 = np.load(call("boxed.npz", sync_eval=net, face_boxes=boxes))
    assert np.array_equal(res2["frames"], res["frames"])
    assert (pipe.last_av_offset, pipe.last_lse_d, pipe.last_lse_c) == got
    # both given: face_boxes wins and the detector is not asked
    det2 = PlantedDetector()
    call("both.npz", sync_eval=net, face_boxes=boxes, face_detector=det2)
    assert det2.calls == [] and (pipe.last_av_offset, pipe.last_lse_d, pipe.last_lse_c) == got


def test_two_tracks_are_aggregated(rig):  # noqa: F811
    """A gap longer than num_failed_det splits the clip into two tracks; the result is the
    reference's aggregate of the two evaluations."""
    from statistics import fmean

    from latentsync_amd import synceval
    from latentsync_amd.audio import read_audio
    pipe, net, call, wav_path, _, _ = rig
    det = PlantedDetector(missing=range(10, 14))
    args = dict(TRACK_ARGS, num_failed_det=2, min_track=5)
    res = np.load(call("two.npz", sync_eval=net, face_detector=det, face_track_args=args))
    frames = torch.from_numpy(res["frames"]).cuda()
    n = frames.shape[0]
    tracks = pipe.last_face_tracks
    assert n >= 20 and [(int(t["frame"][0]), int(t["frame"][-1])) for t in tracks] == [(0, 9), (14, n - 1)]
    wav = read_audio(wav_path, 16000).float()
    want = int(n / 25 * 16000)
    wav = wav[:want] if wav.numel() >= want else torch.cat([wav, torch.zeros(want - wav.numel())])
    parts = []
    for t in tracks:
        f0, f1 = int(t["frame"][0]), int(t["frame"][-1]) + 1
        crop = synceval.crop_track(frames[f0:f1], t["bbox"])
        parts.append(net.evaluate(frames=crop, audio=wav[f0 * 640:f1 * 640]))
    assert pipe.last_av_offset == int(fmean([p[0] for p in parts]))
    assert pipe.last_lse_d == fmean([p[1] for p in parts]) and pipe.last_lse_c == fmean([p[2] for p in parts])


def test_no_track_raises_face_not_detected(rig):  # noqa: F811
    pipe, net, call, _, _, _ = rig
    with pytest.raises(ValueError, match="Face not detected"):
        call("x.npz", sync_eval=net, face_detector=PlantedDetector(), face_track_args=dict(min_face_size=30))  # min_track 50
    with pytest.raises(ValueError, match="needs face_boxes"):
        call("x.npz", sync_eval=net)


def test_real_detector_on_seeded_weights_completes(rig):  # noqa: F811
    """Seeded weights find no face worth the name: the run need only complete or raise the
    reference's "Face not detected"."""
    pipe, net, call, _, _, _ = rig
    real = s3fd.S3FD(device="cuda", weights=R.case_weights())
    try:
        call("real.npz", sync_eval=net, face_detector=real, face_track_args=TRACK_ARGS)
        assert isinstance(pipe.last_av_offset, int) and len(pipe.last_face_tracks) >= 1
    except ValueError as e:
        assert "Face not detected" in str(e)
