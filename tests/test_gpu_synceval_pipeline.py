"""LipsyncPipeline.__call__(..., sync_eval=net, face_boxes=boxes) on the tiny pipeline of
tests/test_pipeline_call.py (tiny UNet, reduced VAE, 64 x 64 faces pasted back into 120 x 160
frames, 8-frame windows): the restored frames are cropped about the boxes and evaluated with the
classic SyncNet (seeded weights, case B of tests/synceval_ref.py)."""
import numpy as np
import pytest
import torch

import synceval_ref as R
from latentsync_amd import synceval
from latentsync_amd.audio import read_audio
from latentsync_amd.pipeline import LipsyncPipeline
from test_pipeline_call import SCHED, _align, _write_wav

pytestmark = pytest.mark.gpu
Rr, Fr, H, W, N = 64, 8, 120, 160, 48
FH, FW = 56, 48


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from latentsync_amd.audio import Audio2Feature
    from latentsync_amd.config import TINY_MODEL
    from latentsync_amd.scheduler import DDIMScheduler
    from latentsync_amd.unet import UNet3DConditionModel
    from latentsync_amd.vae import AutoencoderKL
    d = tmp_path_factory.mktemp("synceval_pipe")
    unet = UNet3DConditionModel(**TINY_MODEL).init_weights(3).to("cuda").eval()
    vae = AutoencoderKL(block_out_channels=(32, 64, 64, 64)).init_weights(4).to("cuda")
    pipe = LipsyncPipeline(vae, Audio2Feature.random(2, device="cuda"), unet, DDIMScheduler(**SCHED))
    _write_wav(d / "audio.wav", 0.88)
    faces = (torch.rand((N, 3, Rr, Rr), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)
    rng = np.random.default_rng(6)
    mats = [_align(80 + rng.uniform(-5, 5), 60 + rng.uniform(-5, 5), rng.uniform(0.8, 1.2), rng.uniform(-0.15, 0.15),
                   FH, FW) for _ in range(N)]
    torch.save({"faces": faces, "boxes": [[0, 0, FW, FH]] * N, "affine_matrices": mats}, d / "data.pth")
    np.save(d / "video.npy", rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8))
    # detector boxes about the face, drifting; one undetected interior frame
    t = np.arange(N)[:, None]
    boxes = np.array([[60.0, 35.0, 100.0, 85.0]]) + 0.2 * t
    boxes[7] = np.nan
    np.save(d / "boxes.npy", boxes)
    net = synceval.SyncNetEval().load_state_dict(R.case_weights("B")).to("cuda").eval()

    def call(out, video="video.npy", **kw):
        pipe(video_path=str(d / video), audio_path=str(d / "audio.wav"), video_out_path=str(d / out), num_frames=Fr,
             num_inference_steps=2, guidance_scale=1.0, data_path=str(d / "data.pth"), mask_image_path=None,
             generator=torch.Generator(device="cuda").manual_seed(1247), **kw)
        return d / out

    return pipe, net, call, str(d / "audio.wav"), boxes, str(d / "boxes.npy")


def test_call_evaluates_the_written_frames(rig):
    pipe, net, call, wav_path, boxes, boxes_path = rig
    res = np.load(call("scored.npz", sync_eval=net, face_boxes=boxes_path))
    frames = res["frames"]
    n = frames.shape[0]
    assert frames.shape[1:] == (H, W, 3) and n % Fr == 0 and 6 <= n <= N
    want = int(n / 25 * 16000)
    wav = read_audio(wav_path, 16000).float()
    wav = wav[:want] if wav.numel() >= want else torch.cat([wav, torch.zeros(want - wav.numel())])
    track = synceval.crop_track(torch.from_numpy(frames).cuda(), boxes[:n])
    off, lse_d, lse_c = net.evaluate(frames=track, audio=wav)
    assert (pipe.last_av_offset, pipe.last_lse_d, pipe.last_lse_c) == (off, lse_d, lse_c)
    assert res["av_offset"].dtype == np.int64 and int(res["av_offset"]) == off and -15 <= off <= 15
    assert res["lse_d"].dtype == np.float32 and float(res["lse_d"]) == float(np.float32(lse_d))
    assert float(res["lse_c"]) == float(np.float32(lse_c))
    assert np.isfinite(lse_d) and lse_d > 0 and np.isfinite(lse_c) and lse_c >= 0
    # the same call without the gate: the same frames, no extra fields
    plain = np.load(call("plain.npz"))
    assert np.array_equal(plain["frames"], frames) and "av_offset" not in plain.files
    # an array instead of a path
    pipe.last_av_offset = None
    call("scored2.npz", sync_eval=net, face_boxes=boxes.astype(np.float32))
    assert pipe.last_av_offset == off


def test_avi_output_is_unchanged_by_the_gate(rig):
    pipe, net, call, _, boxes, _ = rig
    plain = call("plain.avi").read_bytes()
    pipe.last_av_offset = pipe.last_lse_d = pipe.last_lse_c = None
    scored = call("scored.avi", sync_eval=net, face_boxes=boxes).read_bytes()
    assert scored == plain and len(plain) > 1000
    assert isinstance(pipe.last_av_offset, int) and pipe.last_lse_d > 0 and pipe.last_lse_c >= 0


def test_refusals(rig):
    pipe, net, call, _, boxes, _ = rig
    with pytest.raises(ValueError, match="needs face_boxes"):
        call("x.npz", sync_eval=net)
    with pytest.raises(ValueError, match="faces_only"):
        call("x.npz", sync_eval=net, face_boxes=boxes, faces_only=True)
    with pytest.raises(ValueError, match="no restored frames to evaluate"):
        call("x.npz", video="none.mp4", sync_eval=net, face_boxes=boxes)
    with pytest.raises(ValueError, match=f"{N - 1} box rows for {N} faces"):
        call("x.npz", sync_eval=net, face_boxes=boxes[:-1])
    with pytest.raises(ValueError, match="partly NaN"):
        bad = boxes.copy()
        bad[3, 0] = np.nan
        call("x.npz", sync_eval=net, face_boxes=bad)
    with pytest.raises(ValueError, match=r"\(N, 4\)"):
        call("x.npz", sync_eval=net, face_boxes=boxes[:, :3])
    with pytest.raises(ValueError, match="25 frames/s"):
        call("x.npz", sync_eval=net, face_boxes=boxes, video_fps=30)
