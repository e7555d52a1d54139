"""Device Motion-JPEG encoder on MI355X (csrc/ls_video.hip) against the CPU restatement
(tests/mjpeg_cpu.py): scan bytes and offsets equal byte for byte -- the arithmetic is
integer, so there is no tolerance -- then argument validation, and __call__ writing an .avi
that read_avi and Pillow decode.

End-to-end yardstick: outside the pasted face region the written frames are the input
frames through the encoder, and the encoder's decoded pixels equal those of Pillow's own
quality-95 4:2:0 encode (measured gap 0 dB, tests/test_avi_mjpeg.py), so the PSNR bound is
Pillow's PSNR on the same pixels minus DELTA_DB = 0."""
import functools
import io
import math

import numpy as np
import pytest
import torch

import mjpeg_cpu as mj
from latentsync_amd import _lib, ops, video
from latentsync_amd.audio import Audio2Feature
from latentsync_amd.config import TINY_MODEL
from latentsync_amd.pipeline import LipsyncPipeline
from latentsync_amd.scheduler import DDIMScheduler
from latentsync_amd.unet import UNet3DConditionModel
from latentsync_amd.vae import AutoencoderKL
from test_gpu_resample import SCHED, _align, write_wav

pytestmark = pytest.mark.gpu
DELTA_DB = 0.0  # tests/test_avi_mjpeg.py: the restatement decodes to Pillow's own pixels


@functools.lru_cache(maxsize=None)
def content(kind, n, H, W):
    if kind == "smooth":
        return mj.smooth_frames(n, H, W, 31 + H + W)
    if kind == "black":
        return np.zeros((n, H, W, 3), np.uint8)
    if kind == "checker":
        return np.stack([mj.checker_frame(H, W)] * n)
    if kind == "last":
        return np.stack([mj.last_coefficient_frame(H, W)] * n)
    return np.stack([mj.noise_frame(H, W, 7 + i) for i in range(n)])


def check_equal(frames, quality):
    ri = video.restart_interval()
    want = [mj.encode_scan(f, quality, ri) for f in frames]
    data, offsets = ops.mjpeg_encode(torch.from_numpy(frames).cuda(), quality)
    assert data.is_cuda and data.dtype == torch.uint8 and offsets.dtype == torch.int64
    off = offsets.cpu().tolist()
    assert off == [0] + np.cumsum([len(w) for w in want]).tolist()
    got = data.cpu().numpy().tobytes()
    for i, w in enumerate(want):
        assert got[off[i]:off[i + 1]] == w, f"frame {i} differs"
    return got, off


# (n, H, W): smaller than one MCU; edges in both directions, several frames; more MCUs in a
# row than a wave has lanes (66 -> intervals of 10 straddle the row end); 12 intervals a
# frame (the RSTm wrap); a row of 3 * W bytes and frame offsets that are odd
SHAPES = [(1, 8, 8), (3, 40, 56), (2, 24, 16 * 65 + 3), (1, 80, 16 * 23 + 1), (2, 17, 33)]


@pytest.mark.parametrize("quality", [1, 50, 95, 100])
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_smooth_frames_byte_equal(gpu, n, H, W, quality):
    assert video.restart_interval() == 10 == _lib.load().ls_mjpeg_restart_interval()
    got, off = check_equal(content("smooth", n, H, W), quality)
    if (H, W) == (80, 16 * 23 + 1):
        assert math.ceil(5 * 24 / video.restart_interval()) == 12 and got.count(b"\xff\xd0") >= 2  # RST0 twice


@pytest.mark.parametrize("kind,quality", [("black", 95), ("checker", 100), ("last", 1), ("noise", 100), ("noise", 1),
                                          ("checker", 50), ("last", 100)])
def test_content_cases_byte_equal(gpu, kind, quality):
    for n, H, W in ((2, 32, 48), (3, 40, 56), (1, 24, 16 * 65 + 3)):
        check_equal(content(kind, n, H, W), quality)


def test_decodes_with_pillow_to_pillows_own_pixels(gpu):
    Image = pytest.importorskip("PIL.Image")
    frames = content("smooth", 3, 40, 56)
    jpgs = video.encode_frames(torch.from_numpy(frames).cuda(), 95)
    ql, qc = video.quant_tables(95)
    for f, j in zip(frames, jpgs):
        b = io.BytesIO()
        Image.fromarray(f).save(b, "JPEG", qtables=[[int(v) for v in ql], [int(v) for v in qc]], subsampling=2,
                                optimize=False)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(j)).convert("RGB")),
                              np.asarray(Image.open(b).convert("RGB")))


def test_unaligned_view_and_short_output_buffer(gpu):
    """A contiguous slice whose base is odd (frame 1 of a 17x33 clip starts at byte 1683),
    and an output buffer smaller than the scans: nothing past the capacity is written,
    the offsets stay exact."""
    frames = content("noise", 3, 17, 33)
    dev = torch.from_numpy(frames).cuda()
    data, off = ops.mjpeg_encode(dev[1:], 100)
    full, off_full = ops.mjpeg_encode(dev, 100)
    assert torch.equal(off, off_full[1:] - off_full[1]) and torch.equal(data, full[off_full[1]:])
    lib = _lib.load()
    n, H, W = 3, 17, 33
    ws = torch.empty(lib.ls_mjpeg_workspace_bytes(n, H, W), dtype=torch.uint8, device="cuda")
    cap = int(off_full[1]) + 5
    out = torch.full((int(off_full[-1]) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rc = lib.ls_mjpeg_encode(dev.data_ptr(), n, H, W, 100, out.data_ptr(), cap, offs.data_ptr(), ws.data_ptr(),
                             ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(offs, off_full)
    assert torch.equal(out[:cap], full[:cap]) and bool((out[cap:] == 0xAB).all())


def test_validation(gpu):
    lib = _lib.load()
    good = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.mjpeg_encode(good[:, :, ::2], 90)
    with pytest.raises(ValueError, match="uint8"):
        ops.mjpeg_encode(good.float(), 90)
    with pytest.raises(ValueError, match="uint8"):
        ops.mjpeg_encode(good[..., 0], 90)
    for q in (0, 101):
        with pytest.raises(RuntimeError, match="ls_mjpeg_encode.*quality"):
            ops.mjpeg_encode(good, q)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.mjpeg_encode(good, 90, workspace=torch.empty(1024, dtype=torch.uint8, device="cuda"))
    assert lib.ls_mjpeg_workspace_bytes(1, 0, 16) == 0 and lib.ls_mjpeg_workspace_bytes(1, 16, 65536) == 0
    assert lib.ls_mjpeg_encode(None, 1, 16, 16, 90, 16, 16, 16, 16, 1 << 30, None) == 1  # pointers never dereferenced
    assert lib.ls_mjpeg_encode(16, 1, 16, 70000, 90, 16, 16, 16, 16, 1 << 30, None) == 1
    assert b"ls_mjpeg_encode" in lib.ls_last_error()
    assert lib.ls_mjpeg_encode(16, 1, 16, 16, 90, 16, 16, 16, None, 0, None) == 3
    data, off = ops.mjpeg_encode(good[:0], 90)
    assert data.numel() == 0 and off.tolist() == [0]


# ---------------------------------------------------------------- __call__

Fr, Rr, STEPS = 8, 64, 2


@pytest.fixture(scope="module")
def models():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    unet = UNet3DConditionModel(**TINY_MODEL).init_weights(9).to("cuda").eval()
    vae = AutoencoderKL(block_out_channels=(32, 64, 64, 64)).init_weights(10).to("cuda")
    return unet, vae


def test_call_writes_a_playable_avi(gpu, models, tmp_path):
    """The __call__ recipe of test_gpu_resample.py::test_call_with_a_44k1_stereo_wav with
    smooth 120x160 frames and an .avi output: 0.56 s of audio give 14 chunks, padded to 16
    frames with padding_duration 2 / 25 s, so T = 0.56 s keeps 14 frames and 8960 samples."""
    Image = pytest.importorskip("PIL.Image")
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
    frames = mj.smooth_frames(N, H, W, 77)
    np.save(tmp_path / "video.npy", frames)
    kw = dict(video_path=str(tmp_path / "video.npy"), audio_path=str(tmp_path / "audio.wav"), num_frames=Fr,
              num_inference_steps=STEPS, guidance_scale=1.0, height=Rr, width=Rr, data_path=str(tmp_path / "data.pth"),
              mask_image_path=None)
    pipe(video_out_path=str(tmp_path / "out.npz"), generator=torch.Generator(device="cuda").manual_seed(1247), **kw)
    npz = np.load(tmp_path / "out.npz")  # the .npz path is as before
    n_all, pad = npz["frames"].shape[0], float(npz["padding_duration"])
    assert n_all % Fr == 0 and npz["frames"].shape[1:] == (H, W, 3)
    keep_f, keep_a = video.trim_counts(n_all, 25, len(npz["audio"]), 16000, pad, False)
    assert 0 < keep_f == n_all - round(pad * 25) and keep_a == min(len(npz["audio"]), keep_f * 640)

    out_path = str(tmp_path / "out.avi")
    pipe(video_out_path=out_path, generator=torch.Generator(device="cuda").manual_seed(1247), **kw)
    got, fps, audio, sr = video.read_avi(out_path)
    assert fps == 25 and sr == 16000 and got.shape == (keep_f, H, W, 3) and got.dtype == np.uint8
    assert audio.shape == (keep_a,)
    s16 = video.audio_to_s16(npz["audio"][:keep_a])
    assert np.array_equal((audio * 32768).astype(np.int16), s16)
    # the same seed gives the same restored frames: the .avi holds their JPEG round trip
    ql, qc = video.quant_tables(95)
    for i in range(keep_f):
        b = io.BytesIO()
        Image.fromarray(npz["frames"][i]).save(b, "JPEG", qtables=[[int(v) for v in ql], [int(v) for v in qc]],
                                               subsampling=2, optimize=False)
        assert np.array_equal(got[i], np.asarray(Image.open(b).convert("RGB"))), i
    # outside the pasted face region the frames are the input frames, to within Pillow's own q95 PSNR
    same = (npz["frames"][:keep_f] == frames[:keep_f]).all(axis=(0, 3))
    assert same.mean() > 0.5
    ours, theirs = [], []
    for i in range(keep_f):
        b = io.BytesIO()
        Image.fromarray(frames[i]).save(b, "JPEG", qtables=[[int(v) for v in ql], [int(v) for v in qc]],
                                        subsampling=2, optimize=False)
        pil = np.asarray(Image.open(b).convert("RGB"))
        # pixels at least one MCU away from anything the paste touched
        far = ~_dilate(~same, 16)
        ours.append(((got[i].astype(np.float64) - frames[i])[far] ** 2).mean())
        theirs.append(((pil.astype(np.float64) - frames[i])[far] ** 2).mean())
    p_ours, p_theirs = (10 * np.log10(255 ** 2 / np.mean(v)) for v in (ours, theirs))
    print(f"outside the face region: PSNR {p_ours:.3f} dB, Pillow's own q95 encode {p_theirs:.3f} dB")
    assert p_ours >= p_theirs - DELTA_DB - 1e-9

    # faces_only: the aligned faces become the video; force_video_length keeps every frame
    pipe(video_out_path=str(tmp_path / "faces.avi"), faces_only=True, force_video_length=True, video_quality=80,
         generator=torch.Generator(device="cuda").manual_seed(1247), **kw)
    got, fps, audio, sr = video.read_avi(str(tmp_path / "faces.avi"))
    assert got.shape == (N, Rr, Rr, 3) and fps == 25 and audio.shape[0] <= int(N / 25 * 16000)
    pipe.close()


def _dilate(mask, r):
    """Binary dilation of a (H, W) mask by a (2r + 1)^2 square."""
    m = torch.from_numpy(mask)[None, None].float()
    return torch.nn.functional.max_pool2d(m, 2 * r + 1, stride=1, padding=r)[0, 0].numpy() > 0
