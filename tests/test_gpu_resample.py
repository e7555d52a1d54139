"""Sample-rate conversion on MI355X: ls_resample against a float64 numpy restatement of
its definition (written here, with the package's float64 taps), then through the public
audio path: read_audio, Audio2Feature.audio2feat and LipsyncPipeline.__call__ on WAV
files at 44.1 and 48 kHz.

Kernel acceptance is the fp32 dot-product bound, per output and in any summation order:
|y - y64| <= (T + 2) * 2^-24 * sum_j |h[p, j]| |x[base + j]| + 1e-30 -- T products and
T - 1 additions of relative error 2^-24 each (bounded by gamma_T <= (T + 1) * 2^-24), plus
one more unit for the rounding of the float64 taps to fp32."""
import functools
import math
import struct

import numpy as np
import pytest
import torch

from latentsync_amd import _lib, ops
from latentsync_amd.audio import (Audio2Feature, num_chunks, read_audio, read_wav, resample_taps, resample_taps64)
from latentsync_amd.config import TINY_MODEL
from latentsync_amd.pipeline import LipsyncPipeline
from latentsync_amd.scheduler import DDIMScheduler
from latentsync_amd.unet import UNet3DConditionModel
from latentsync_amd.vae import AutoencoderKL

pytestmark = pytest.mark.gpu
SCHED = dict(beta_end=0.012, beta_schedule="scaled_linear", beta_start=0.00085, clip_sample=False,
             num_train_timesteps=1000, set_alpha_to_one=False, steps_offset=1)
RATES = [48000, 44100, 22050, 8000, 11025, 44101]  # to 16 kHz: 1/3, 160/441, 320/441, 2/1, 640/441, 16000/44101


def definition_f64(x, sr_in, sr_out, n_sel=None):
    """(y64, bound) of the outputs n_sel (all when None): y[n] = sum_j h[p, j] x[base + j],
    base = n M // L, p = n M % L, x zero outside [0, n_in); bound = the module docstring's."""
    L, M, half, _ = resample_taps(sr_in, sr_out)
    h = resample_taps64(sr_in, sr_out)
    T = 2 * half + 1
    n_in = len(x)
    n_out = -(-n_in * L // M)
    n = np.arange(n_out, dtype=np.int64) if n_sel is None else np.asarray(n_sel, dtype=np.int64)
    xp = np.concatenate([np.zeros(half, np.float32), np.asarray(x, np.float32), np.zeros(half + M + 1, np.float32)])
    base, p = n * M // L, n * M % L
    y, mag = np.zeros(len(n)), np.zeros(len(n))
    for j in range(T):
        term = h[p, j] * xp[base + j].astype(np.float64)
        y += term
        mag += np.abs(term)
    return y, (T + 2) * 2.0 ** -24 * mag + 1e-30, n_out


def assert_within_bound(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())
    print(f"{what}: max |err| {err.max():.3e}, max err / bound {worst:.4f}")
    assert worst <= 1.0, f"{what}: an output misses the fp32 dot-product bound by {worst:.3f}x"


@pytest.mark.parametrize("sr", RATES)
def test_kernel_matches_definition(gpu, sr):
    L, M, half, taps = resample_taps(sr, 16000)
    g = math.gcd(sr, 16000)
    assert (L, M) == (16000 // g, sr // g) and taps.shape == (L, 2 * half + 1)
    for n_in in (1, 5, half, 2 * half + 1, 4001):
        x = (np.random.default_rng(sr + n_in).normal(0, 0.3, n_in)).astype(np.float32)
        want, bound, n_out = definition_f64(x, sr, 16000)
        y = ops.resample(torch.from_numpy(x).cuda(), sr, 16000)
        assert y.is_cuda and y.dtype == torch.float32 and y.shape == (n_out,) and n_out == math.ceil(n_in * L / M)
        assert_within_bound(y.cpu().numpy(), want, bound, f"{sr} -> 16000, n_in {n_in}")


def test_indices_beyond_32_bits(gpu):
    """306 s at 44.1 kHz: n * M passes 2^31 within the last 1000 outputs."""
    n_in, M = 13_500_000, 441
    x = np.random.default_rng(7).standard_normal(n_in, dtype=np.float32) * np.float32(0.3)
    y = ops.resample(torch.from_numpy(x), 44100, 16000)
    n_out = y.numel()
    assert n_out == math.ceil(n_in * 160 / 441) and (n_out - 1000) * M > 2 ** 31
    assert bool(torch.isfinite(y).all())
    for name, sel in (("first", np.arange(1000)), ("last", np.arange(n_out - 1000, n_out))):
        want, bound, _ = definition_f64(x, 44100, 16000, sel)
        assert_within_bound(y[torch.from_numpy(sel).cuda()].cpu().numpy(), want, bound, f"{name} 1000 of {n_out}")


# ---------------------------------------------------------------- the public path


def write_wav(path, a, sr, kind):
    """a: float (n,) or (n, ch) in [-1, 1); kind 's16' or 'f32'."""
    a = np.asarray(a, dtype=np.float64)
    ch = 1 if a.ndim == 1 else a.shape[1]
    if kind == "s16":
        tag, bits, raw = 1, 16, np.round(a * 32768).clip(-32768, 32767).astype("<i2").tobytes()
    else:
        tag, bits, raw = 3, 32, a.astype("<f4").tobytes()
    block = ch * bits // 8
    fmt = struct.pack("<HHIIHH", tag, ch, sr, sr * block, block, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(raw)) + raw
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


@pytest.mark.parametrize("sr,kind,ch", [(48000, "s16", 2), (44100, "f32", 1)])
def test_tones_through_read_audio(gpu, tmp_path, sr, kind, ch):
    L, M, half, _ = resample_taps(sr, 16000)
    n_in = sr // 2
    edge = math.ceil(half * L / M) + 2
    t_in = np.arange(n_in) / sr
    for f in (1000, 10000):
        a = 0.5 * np.sin(2 * np.pi * f * t_in)
        p = write_wav(tmp_path / f"{f}.wav", a if ch == 1 else np.stack([a] * ch, axis=1), sr, kind)
        y = read_audio(p)
        assert not y.is_cuda and y.dtype == torch.float32 and y.shape == (math.ceil(n_in * L / M),)
        y = y.numpy().astype(np.float64)[edge:-edge]
        t = np.arange(edge, edge + len(y)) / 16000.0
        if f == 1000:
            err = np.abs(y - 0.5 * np.sin(2 * np.pi * f * t)).max()
            print(f"{sr} Hz {kind} x{ch}: 1 kHz tone, steady-state error {err:.3e}")
            assert err <= 3e-5 + 2.0 ** -15
        else:
            print(f"{sr} Hz {kind} x{ch}: 10 kHz tone comes out at {np.abs(y).max():.3e}")
            assert np.abs(y).max() <= 5e-5 + 2.0 ** -15
    if sr == 48000:
        assert read_audio(p, 8000).shape == (math.ceil(n_in / 6),)


def test_equal_rates_return_the_input(gpu):
    x = torch.randn(100, device="cuda")
    assert ops.resample(x, 16000, 16000) is x


def test_validation(gpu):
    lib = _lib.load()
    args = lambda L, n_out: (16, 441, 16, L, 441, 107, 16, n_out, None)  # pointers never dereferenced
    assert lib.ls_resample(*args(160, 161)) == 1
    assert b"ls_resample" in lib.ls_last_error() and b"n_out" in lib.ls_last_error()
    assert lib.ls_resample(*args(0, 160)) == 1
    assert b"ls_resample" in lib.ls_last_error()
    assert lib.ls_resample(None, 441, 16, 160, 441, 107, 16, 160, None) == 1
    with pytest.raises(RuntimeError, match="ls_resample"):  # 1 MHz -> 8 kHz: the window of a block exceeds the LDS
        ops.resample(torch.zeros(1000, device="cuda"), 1_000_000, 8000)


def test_features_of_a_44k1_file(gpu, tmp_path):
    """audio2feat(path) == audio2feat(the decoded samples resampled by ops.resample): the
    same samples into the same kernels, and Whisper sees 16 kHz."""
    enc = Audio2Feature.random(2, device="cuda")
    n_in = 44100
    a = np.random.default_rng(3).normal(0, 0.1, (n_in, 2)).clip(-1, 0.999)
    p = write_wav(tmp_path / "a.wav", a, 44100, "s16")
    decoded, sr = read_wav(p)
    assert sr == 44100 and decoded.shape == (n_in,)
    feat = enc.audio2feat(p)
    ref = enc.audio2feat(ops.resample(decoded, 44100, 16000))
    n16 = math.ceil(n_in * 160 / 441)
    T50 = (n16 // 160) // 2
    assert feat.shape == (T50, 5, 384) and torch.isfinite(feat).all()
    assert torch.equal(feat, ref)
    assert len(enc.feature2chunks(feat, 25)) == num_chunks(T50, 25)


# ---------------------------------------------------------------- __call__

Fr, Rr, STEPS = 8, 64, 2


@pytest.fixture(scope="module")
def models():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    unet = UNet3DConditionModel(**TINY_MODEL).init_weights(9).to("cuda").eval()
    vae = AutoencoderKL(block_out_channels=(32, 64, 64, 64)).init_weights(10).to("cuda")
    return unet, vae


def _align(cx, cy, s, theta, fh, fw):
    c, sn = math.cos(theta) * s, math.sin(theta) * s
    rot = np.array([[c, -sn], [sn, c]])
    t = np.array([fw / 2.0, fh / 2.0]) - rot @ np.array([cx, cy])
    return np.concatenate([rot, t[:, None]], axis=1)


def test_call_with_a_44k1_stereo_wav(gpu, models, tmp_path):
    """__call__ on a 0.56 s, 44.1 kHz, stereo, 16-bit WAV (refused with NotImplementedError
    before the resampler): the .npz carries 16 kHz audio trimmed to the frames written."""
    unet, vae = models
    H, W, fh, fw, N = 120, 160, 56, 48, 24
    pipe = LipsyncPipeline(vae, Audio2Feature.random(2, device="cuda"), unet, DDIMScheduler(**SCHED))
    rng = np.random.default_rng(6)
    n_in = int(0.56 * 44100)
    write_wav(tmp_path / "audio.wav", rng.normal(0, 0.1, (n_in, 2)).clip(-1, 0.999), 44100, "s16")
    low = torch.rand((N, 3, 8, 8), generator=torch.Generator().manual_seed(61))
    faces = (torch.nn.functional.interpolate(low, size=(Rr, Rr), mode="bicubic") * 255).round().clamp(0, 255)
    mats = [_align(80 + rng.uniform(-5, 5), 60 + rng.uniform(-5, 5), rng.uniform(0.8, 1.2),
                   rng.uniform(-0.15, 0.15), fh, fw) for _ in range(N)]
    torch.save({"faces": faces.to(torch.uint8), "boxes": [[0, 0, fw, fh]] * N, "affine_matrices": mats},
               tmp_path / "data.pth")
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    np.save(tmp_path / "video.npy", frames)
    out_path = str(tmp_path / "out.npz")
    pipe(video_path=str(tmp_path / "video.npy"), audio_path=str(tmp_path / "audio.wav"), video_out_path=out_path,
         num_frames=Fr, num_inference_steps=STEPS, guidance_scale=1.0, height=Rr, width=Rr,
         data_path=str(tmp_path / "data.pth"), mask_image_path=None,
         generator=torch.Generator(device="cuda").manual_seed(1247))
    out = np.load(out_path)
    n = out["frames"].shape[0]
    assert 0 < n <= N and n % Fr == 0 and out["frames"].shape[1:] == (H, W, 3) and out["frames"].dtype == np.uint8
    assert int(out["sample_rate"]) == 16000
    assert out["audio"].dtype == np.float32 and 0 < out["audio"].shape[0] <= int(n / 25 * 16000)
    assert np.isfinite(out["audio"]).all() and np.abs(out["audio"]).max() < 1.0
    pipe.close()
