"""The sync-confidence score is opt-in: LipsyncPipeline.__call__ without syncnet= writes an
.npz with exactly the keys it wrote before and sets no new attribute, and serve.run_job's
reply has exactly its old keys unless the worker carries a network.  CPU only: the window loop
and the scorer are stand-ins (tests/test_gpu_syncnet_pipeline.py runs the real ones)."""
import os
import wave

import numpy as np
import torch

from latentsync_amd import serve as S
from latentsync_amd.pipeline import LipsyncPipeline

NPZ_KEYS = {"frames", "audio", "fps", "sample_rate", "padding_duration"}
REPLY_KEYS = {"message", "output_url", "gif_url", "elapsed_time", "request_uuid"}


def _write_wav(path, seconds, sr=16000, seed=1):
    a = np.random.default_rng(seed).normal(0, 0.1, int(seconds * sr)).clip(-1, 0.999)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes((a * 32768).astype("<i2").tobytes())


class _Audio:
    """Audio2Feature stand-in: one (2, 4) chunk per video frame of the clip."""

    def __init__(self, n):
        self.n = n

    def audio2feat(self, path):
        return None

    def feature2chunks(self, feature_array, fps):
        return [torch.zeros(2, 4) for _ in range(self.n)]


def _pipe(tmp_path, n=16, R=256):
    pipe = LipsyncPipeline.__new__(LipsyncPipeline)
    pipe.denoising_unet = type("U", (), {"device": torch.device("cpu")})()
    pipe.audio_encoder = _Audio(n)
    faces = torch.randint(0, 256, (n, 3, R, R), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    torch.save({"faces": faces, "boxes": [[0, 0, 8, 8]] * n, "affine_matrices": [np.eye(2, 3)] * n},
               tmp_path / "data.pth")
    _write_wav(tmp_path / "audio.wav", n / 25)

    def run_windows(f, chunks, keep, num_frames, *a, **k):
        u8 = f.permute(0, 2, 3, 1).contiguous()
        return f.float(), u8

    pipe.run_windows = run_windows
    return pipe, dict(video_path="none.mp4", audio_path=str(tmp_path / "audio.wav"), data_path=str(tmp_path / "data.pth"),
                      mask_image_path=None, faces_only=True)


def test_call_without_syncnet_is_unchanged(tmp_path):
    pipe, kw = _pipe(tmp_path)
    before = set(vars(pipe))
    pipe(video_out_path=str(tmp_path / "out.npz"), **kw)
    res = np.load(tmp_path / "out.npz")
    assert set(res.files) == NPZ_KEYS
    assert res["frames"].shape == (16, 256, 256, 3)
    assert set(vars(pipe)) == before and not hasattr(pipe, "last_sync_conf")


def test_call_with_syncnet_adds_the_scores(tmp_path):
    pipe, kw = _pipe(tmp_path)
    seen = {}

    def sync_confidence(net, faces_u8, audio_path, video_fps, num_frames):
        seen.update(net=net, shape=tuple(faces_u8.shape), audio=audio_path, fps=video_fps, F=num_frames)
        pipe.last_sync_scores = torch.tensor([0.25, 0.75])
        pipe.last_sync_conf = 0.5
        return pipe.last_sync_scores

    pipe.sync_confidence = sync_confidence
    net = object()
    pipe(video_out_path=str(tmp_path / "out.npz"), syncnet=net, **kw)
    res = np.load(tmp_path / "out.npz")
    assert set(res.files) == NPZ_KEYS | {"sync_scores", "sync_conf"}
    assert res["sync_scores"].tolist() == [0.25, 0.75] and float(res["sync_conf"]) == 0.5
    assert seen == dict(net=net, shape=(16, 256, 256, 3), audio=kw["audio_path"], fps=25, F=16)


class _StubPipeline:
    def __init__(self):
        self.calls = []

    def __call__(self, **kw):
        self.calls.append(kw)
        if "syncnet" in kw:
            self.last_sync_conf = 0.625
        open(kw["video_out_path"], "wb").close()


def _job_files(d):
    for n in ("v1.mp4", "v1.pth", "r1.wav"):
        open(os.path.join(d, n), "wb").close()
    return {"id": "r1", "video_id": "v1", "audio_url": "unused"}


def test_run_job_reply_without_syncnet_is_unchanged(tmp_path):
    pipe = _StubPipeline()
    reply = S.run_job(pipe, _job_files(tmp_path), str(tmp_path), str(tmp_path / "results"), 256)
    assert set(reply) == REPLY_KEYS
    assert "syncnet" not in pipe.calls[0]


def test_run_job_reports_sync_conf(tmp_path):
    pipe = _StubPipeline()
    pipe.syncnet = object()
    reply = S.run_job(pipe, _job_files(tmp_path), str(tmp_path), str(tmp_path / "results"), 256)
    assert set(reply) == REPLY_KEYS | {"sync_conf"} and reply["sync_conf"] == 0.625
    assert pipe.calls[0]["syncnet"] is pipe.syncnet
