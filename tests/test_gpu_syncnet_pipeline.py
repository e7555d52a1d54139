"""LipsyncPipeline.__call__(..., syncnet=net) on the tiny pipeline of tests/test_pipeline_call.py
(tiny UNet, reduced VAE, 64 x 64 faces, 8-frame windows) with config A's towers scaled to that
face size: lower half 32 x 64 with 24 channels, mel windows of ceil(8 / 5 * 16) = 26 columns."""
import wave

import numpy as np
import pytest
import torch

from latentsync_amd import syncnet
from latentsync_amd.audio import read_audio
from latentsync_amd.pipeline import LipsyncPipeline

pytestmark = pytest.mark.gpu
SCHED = dict(beta_end=0.012, beta_schedule="scaled_linear", beta_start=0.00085, clip_sample=False,
             num_train_timesteps=1000, set_alpha_to_one=False, steps_offset=1)
Rr, Fr, N = 64, 8, 48
CONFIG = dict(  # 80 x 26 -> 40 x 26 -> 20 x 13 -> 10 x 6 -> 5 x 3 -> 2 x 1 -> 1 x 1; 32 x 64 -> 32 x 32 -> ... -> 1 x 1
    audio_encoder=dict(in_channels=1, block_out_channels=[32, 32, 64, 64, 64, 64],
                       downsample_factors=[[2, 1], 2, 2, 2, 2, [2, 1]], attn_blocks=[0, 0, 1, 0, 0, 0], dropout=0.0),
    visual_encoder=dict(in_channels=3 * Fr, block_out_channels=[32, 32, 64, 64, 64, 64],
                        downsample_factors=[[1, 2], 2, 2, 2, 2, 2], attn_blocks=[0, 0, 1, 0, 0, 0], dropout=0.0))


def _write_wav(path, seconds, sr=16000, seed=1):
    a = np.random.default_rng(seed).normal(0, 0.1, int(seconds * sr)).clip(-1, 0.999)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes((a * 32768).astype("<i2").tobytes())


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from latentsync_amd.audio import Audio2Feature
    from latentsync_amd.config import TINY_MODEL
    from latentsync_amd.scheduler import DDIMScheduler
    from latentsync_amd.unet import UNet3DConditionModel
    from latentsync_amd.vae import AutoencoderKL
    d = tmp_path_factory.mktemp("syncnet_pipe")
    unet = UNet3DConditionModel(**TINY_MODEL).init_weights(3).to("cuda").eval()
    vae = AutoencoderKL(block_out_channels=(32, 64, 64, 64)).init_weights(4).to("cuda")
    pipe = LipsyncPipeline(vae, Audio2Feature.random(2, device="cuda"), unet, DDIMScheduler(**SCHED))
    _write_wav(d / "audio.wav", 0.88)
    faces = (torch.rand((N, 3, Rr, Rr), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)
    torch.save({"faces": faces, "boxes": [[0, 0, 48, 56]] * N, "affine_matrices": [np.eye(2, 3)] * N}, d / "data.pth")
    net = syncnet.StableSyncNet(CONFIG).init_weights(9).to("cuda").eval()

    def call(out, **kw):
        pipe(video_path="none.mp4", audio_path=str(d / "audio.wav"), video_out_path=str(d / out), num_frames=Fr,
             num_inference_steps=2, guidance_scale=1.0, data_path=str(d / "data.pth"), mask_image_path=None,
             faces_only=True, generator=torch.Generator(device="cuda").manual_seed(1247), **kw)
        return d / out

    return pipe, net, call, str(d / "audio.wav")


def test_call_scores_the_synced_faces(rig):
    pipe, net, call, wav_path = rig
    res = np.load(call("scored.npz", syncnet=net))
    faces = res["frames"]  # faces_only: the synced aligned faces, run_windows' uint8 output
    n = faces.shape[0]
    assert faces.shape[1:] == (Rr, Rr, 3) and n % Fr == 0 and n >= 2 * Fr
    want = int(n / 25 * 16000)
    wav = read_audio(wav_path, 16000).float()
    wav = wav[:want] if wav.numel() >= want else torch.cat([wav, torch.zeros(want - wav.numel())])
    starts, _ = syncnet.window_plan(n, 1 + want // 200, 25, Fr, Fr)
    assert len(starts) >= 2
    scores, got_starts = syncnet.sync_scores(net, torch.from_numpy(faces).cuda(), wav, fps=25, num_frames=Fr, stride=Fr)
    assert got_starts == starts and res["sync_scores"].shape == (len(starts),) and res["sync_scores"].dtype == np.float32
    assert np.array_equal(res["sync_scores"], scores.cpu().numpy())
    assert np.isfinite(res["sync_scores"]).all() and (np.abs(res["sync_scores"]) <= 1 + 1e-6).all()
    assert torch.equal(pipe.last_sync_scores, scores.cpu()) and pipe.last_sync_scores.device.type == "cpu"
    assert pipe.last_sync_conf == float(scores.cpu().mean()) == float(res["sync_conf"])


def test_avi_output_is_unchanged_by_scoring(rig):
    pipe, net, call, _ = rig
    plain = call("plain.avi").read_bytes()
    pipe.last_sync_conf = pipe.last_sync_scores = None
    scored = call("scored.avi", syncnet=net).read_bytes()
    assert scored == plain and len(plain) > 1000
    assert pipe.last_sync_scores is not None and pipe.last_sync_scores.numel() >= 2
    assert pipe.last_sync_conf == float(pipe.last_sync_scores.mean())
