"""Ingest face resize on MI355X: ls_resize_faces_u8 against torchvision's v1
``transforms.Resize((R, R), BILINEAR, antialias=True)`` on uint8 (cast to fp32,
antialiased bilinear interpolate, torch.round, cast back -- restated with torch below,
torchvision is not a dependency), then the same resize as a node of the window engine's
captured encode graph, through run_windows / __call__, and behind ImageProcessor.

Acceptance of the kernel is tie-aware.  The same interpolate is computed in fp64; a pixel
whose fp64 value lies at least TIE = 1e-3 from a rounding boundary must equal the oracle
exactly, the others may differ by one level.  1e-3 is derived: two fp32 passes of at most
16 taps over values <= 255 move a sum by at most about 16 * 255 * 2^-24 * 2 ~ 5e-4."""
import functools
import math
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from latentsync_amd import ops
from latentsync_amd.config import TINY_MODEL
from latentsync_amd.pipeline import LipsyncPipeline, WindowEngine, load_fixed_mask
from latentsync_amd.scheduler import DDIMScheduler
from latentsync_amd.unet import UNet3DConditionModel
from latentsync_amd.vae import AutoencoderKL
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
SCHED = dict(beta_end=0.012, beta_schedule="scaled_linear", beta_start=0.00085, clip_sample=False,
             num_train_timesteps=1000, set_alpha_to_one=False, steps_offset=1)
TIE = 1e-3

# (in_h, in_w, out_h, out_w)
CASES = [(64, 64, 32, 32),    # exact 2:1: dyadic weights, frequent exact ties
         (48, 48, 32, 32),    # 1.5:1: the tap count alternates per pixel
         (37, 37, 24, 24),    # odd sizes, clipped supports at both borders
         (100, 100, 24, 24),  # 4.17:1: 10 taps
         (24, 24, 32, 32),    # upscale: support = 1
         (41, 37, 24, 32),    # non-square: h / w swaps
         (64, 32, 32, 32)]    # one dimension copied through


def oracle_resize(x, out_h, out_w):
    """torchvision 0.19 v1 Resize on a uint8 tensor, on the CPU."""
    y = F.interpolate(x.float(), size=(out_h, out_w), mode="bilinear", align_corners=False, antialias=True)
    return torch.round(y).to(torch.uint8)


def smooth_faces(n, h, w, seed):
    """A bicubic-upsampled low-resolution field, uint8 (n,3,h,w)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((n, 3, max(h // 8, 2), max(w // 8, 2)), generator=g)
    return (F.interpolate(low, size=(h, w), mode="bicubic") * 255).round().clamp(0, 255).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def case_data(n, case, kind):
    """Input, oracle and the near-boundary set of one case: computed once, never modified."""
    ih, iw, oh, ow = case
    if kind == "random":
        x = torch.randint(0, 256, (n, 3, ih, iw), generator=torch.Generator().manual_seed(ih * 1000 + iw + n),
                          dtype=torch.uint8)
    else:
        x = smooth_faces(n, ih, iw, ih * 1000 + iw + n)
    v64 = F.interpolate(x.double(), size=(oh, ow), mode="bilinear", align_corners=False, antialias=True)
    near = ((v64 - torch.floor(v64)) - 0.5).abs() < TIE
    return x, oracle_resize(x, oh, ow), v64, near


def assert_tie_aware(got, ref, near, what):
    d = (got.to(torch.int32) - ref.to(torch.int32)).abs()
    far_bad = int((d[~near] != 0).sum())
    print(f"{what}: near-boundary share {float(near.float().mean()):.4f}, differing there "
          f"{int((d[near] != 0).sum())}, differing elsewhere {far_bad}, max |diff| {int(d.max())}")
    assert far_bad == 0, f"{what}: {far_bad} pixels away from a rounding boundary differ from the oracle"
    assert int(d.max()) <= 1, f"{what}: a near-boundary pixel differs by {int(d.max())} levels"


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("n", [1, 19])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_kernel_matches_oracle(gpu, case, n, kind):
    ih, iw, oh, ow = case
    x, ref, v64, near = case_data(n, case, kind)
    got = ops.resize_faces_u8(x.cuda(), oh, ow)
    assert got.shape == (n, 3, oh, ow) and got.dtype == torch.uint8 and got.is_contiguous()
    got = got.cpu()
    assert_tie_aware(got, ref, near, f"{ih}x{iw}->{oh}x{ow} N={n} {kind}")
    if case == (64, 64, 32, 32):
        # interior weights are 1/8, 3/8, 3/8, 1/8: every product and sum is exact in fp32, so
        # the only freedom left is the rounding of exact .5 ties -- half to even, as torch.round
        inner = (slice(None), slice(None), slice(1, -1), slice(1, -1))
        ties = (v64[inner] - torch.floor(v64[inner])) == 0.5
        print(f"exact .5 ties in the interior: {float(ties.float().mean()):.4f}")
        if kind == "random":
            assert ties.any()
        assert torch.equal(got[inner], ref[inner])


def test_equal_size_is_a_copy_and_out_form(gpu):
    x = case_data(19, CASES[2], "random")[0].cuda()
    same = ops.resize_faces_u8(x, 37, 37)
    assert torch.equal(same, x)
    ref = ops.resize_faces_u8(x, 24, 24)
    out = torch.full((19, 3, 24, 24), 7, dtype=torch.uint8, device="cuda")
    ret = ops.resize_faces_u8(x, 24, 24, out=out)
    assert ret is out and torch.equal(out, ref)
    with pytest.raises(ValueError):
        ops.resize_faces_u8(x, 24, 24, out=torch.empty((19, 3, 24, 32), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="downscale factor above 7"):
        ops.resize_faces_u8(x, 5, 5)


def test_more_images_than_one_grid(gpu):
    """One image per grid z-slice, 65535 at the most per launch: a batch above that is cut
    into several launches (the second one starts at an offset into both buffers)."""
    n = 65535 + 3
    x = torch.randint(0, 256, (n, 3, 8, 8), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    got = ops.resize_faces_u8(x.cuda(), 4, 4).cpu()
    v64 = F.interpolate(x.double(), size=(4, 4), mode="bilinear", align_corners=False, antialias=True)
    near = ((v64 - torch.floor(v64)) - 0.5).abs() < TIE
    assert_tie_aware(got, oracle_resize(x, 4, 4), near, f"8x8->4x4 N={n}")


# ---------------------------------------------------------------- in the graph

Fr, Rr, STEPS = 8, 64, 2
LAT = Rr // 8


@pytest.fixture(scope="module")
def models():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    unet = UNet3DConditionModel(**TINY_MODEL).init_weights(9).to("cuda").eval()
    vae = AutoencoderKL(block_out_channels=(32, 64, 64, 64)).init_weights(10).to("cuda")
    return unet, vae


def window_inputs(n_win, seed):
    g = torch.Generator().manual_seed(seed)
    N = n_win * Fr
    audio = torch.randn((N, 50, 384), generator=g)
    init = torch.randn((1, 4, 1, LAT, LAT), generator=g)
    noise = [(torch.randn((Fr, 4, LAT, LAT), generator=g), torch.randn((Fr, 4, LAT, LAT), generator=g))
             for _ in range(n_win)]
    return audio, init, noise


def test_engine_resize_node_bit_identical_and_not_stale(gpu, models):
    """An engine built with face_resolution=128 and fed 128^2 faces computes, bit for bit,
    what the plain engine computes from the faces resized up front -- also for a second
    set of faces loaded into the already captured engine (a graph that baked in its first
    input, or skipped the resize on replay, fails here)."""
    unet, vae = models
    mask = load_fixed_mask(Rr).cuda()
    audio, init, noise = window_inputs(1, 31)
    resizing = WindowEngine(unet, vae, DDIMScheduler(**SCHED), Fr, Rr, STEPS, 1.0, face_resolution=128)
    plain = WindowEngine(unet, vae, DDIMScheduler(**SCHED), Fr, Rr, STEPS, 1.0)
    assert resizing.faces_src.shape == (Fr, 3, 128, 128) and plain.faces_src is None
    same = WindowEngine(unet, vae, DDIMScheduler(**SCHED), Fr, Rr, STEPS, 1.0, face_resolution=Rr)
    assert same.faces_src is None  # equal resolutions: no extra buffer, no resize node
    outs = []
    for seed in (32, 33):
        faces = smooth_faces(Fr, 128, 128, seed).cuda()
        args = (mask, audio.cuda(), init.cuda(), noise[0][0].cuda(), noise[0][1].cuda())
        resizing.load(faces, *args)
        plain.load(ops.resize_faces_u8(faces, Rr, Rr), *args)
        a, a8 = resizing.run().clone(), resizing.out_u8.clone()
        b, b8 = plain.run().clone(), plain.out_u8.clone()
        assert resizing.graphs is not None and plain.graphs is not None
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a8, b8)
        outs.append(a)
    assert not torch.equal(outs[0], outs[1])
    with pytest.raises(ValueError):
        resizing.load(torch.zeros((Fr, 3, Rr, Rr), dtype=torch.uint8, device="cuda"), *args)
    with pytest.raises(ValueError):
        plain.load(torch.zeros((Fr, 3, 128, 128), dtype=torch.uint8, device="cuda"), *args)
    for e in (resizing, plain, same):
        e.close()


def test_run_windows_resizes_and_matches_oracle(gpu, models, monkeypatch):
    """run_windows(faces_128, height=64) over 2 windows in one batch of 2 against the CPU
    oracle fed the oracle-resized faces, window by window; 3e-2 is the bound of
    test_gpu_pipeline.py::test_run_windows_batches_match_oracle for this configuration
    (smooth faces: a one-level flip of the resize is far below it)."""
    unet, vae = models
    monkeypatch.setitem(R.VAE_CFG, "block_out_channels", (32, 64, 64, 64))
    pipe = LipsyncPipeline(vae, None, unet, DDIMScheduler(**SCHED))
    pipe.windows_per_batch = 2
    n_win = 2
    N = n_win * Fr
    faces = smooth_faces(N, 128, 128, 41)
    small = oracle_resize(faces, Rr, Rr)
    mask = load_fixed_mask(Rr)
    audio, init, noise = window_inputs(n_win, 42)
    init = init.repeat(1, 1, N, 1, 1)
    out, out_u8 = pipe.run_windows(faces, audio.cuda(), mask, Fr, STEPS, 1.0, all_latents=init.cuda(),
                                   vae_noise=lambda i: (noise[i][0].cuda(), noise[i][1].cuda()), height=Rr)
    assert out.shape == (N, 3, Rr, Rr) and out_u8.shape == (N, Rr, Rr, 3)
    assert [k[2] for k in pipe._engines] == [128]  # the face resolution is part of the engine key
    for w in range(n_win):
        sl = slice(w * Fr, (w + 1) * Fr)
        ref = R.pipeline_window(unet.state_dict(), dict(unet.config), vae._sd, small[sl], mask, audio[sl],
                                init[:, :, sl][:, :, :1], noise[w][0], noise[w][1], num_steps=STEPS,
                                guidance_scale=1.0)
        e = rel_err(out[sl].cpu(), ref)
        print("run_windows 128 -> 64, window", w, e)
        assert e < 3e-2
    pipe.close()


def test_run_windows_upscale(gpu, models):
    """48^2 faces served at 64: shape, finiteness, and equality with the same call on the
    faces resized up front (the plain engine)."""
    unet, vae = models
    pipe = LipsyncPipeline(vae, None, unet, DDIMScheduler(**SCHED))
    faces = smooth_faces(Fr, 48, 48, 51).cuda()
    mask = load_fixed_mask(Rr)
    audio, init, noise = window_inputs(1, 52)
    kw = dict(all_latents=init.repeat(1, 1, Fr, 1, 1).cuda(),
              vae_noise=lambda i: (noise[i][0].cuda(), noise[i][1].cuda()))
    out, out_u8 = pipe.run_windows(faces, audio.cuda(), mask, Fr, STEPS, 1.0, height=Rr, **kw)
    assert out.shape == (Fr, 3, Rr, Rr) and out_u8.shape == (Fr, Rr, Rr, 3) and torch.isfinite(out).all()
    ref, ref_u8 = pipe.run_windows(ops.resize_faces_u8(faces, Rr, Rr), audio.cuda(), mask, Fr, STEPS, 1.0, **kw)
    assert sorted(k[2] is None for k in pipe._engines) == [False, True]  # a resizing and a plain engine
    assert torch.equal(out, ref) and torch.equal(out_u8, ref_u8)
    pipe.close()


def _align(cx, cy, s, theta, fh, fw):
    c, sn = math.cos(theta) * s, math.sin(theta) * s
    rot = np.array([[c, -sn], [sn, c]])
    t = np.array([fw / 2.0, fh / 2.0]) - rot @ np.array([cx, cy])
    return np.concatenate([rot, t[:, None]], axis=1)


def _write_wav(path, seconds, sr=16000, seed=1):
    a = np.random.default_rng(seed).normal(0, 0.1, int(seconds * sr)).clip(-1, 0.999)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes((a * 32768).astype("<i2").tobytes())


def test_call_with_faces_at_another_resolution(gpu, models, tmp_path, monkeypatch):
    """__call__ with a data.pth cut at 128^2 served at height = width = 64 (the request the
    parent of this feature refused with NotImplementedError): frames of the original
    video's size come out, and restore_video is handed 64^2 faces."""
    from latentsync_amd.audio import Audio2Feature
    unet, vae = models
    H, W, fh, fw, N = 120, 160, 56, 48, 24
    pipe = LipsyncPipeline(vae, Audio2Feature.random(2, device="cuda"), unet, DDIMScheduler(**SCHED))
    _write_wav(tmp_path / "audio.wav", 0.56)
    faces = smooth_faces(N, 128, 128, 61)
    rng = np.random.default_rng(6)
    mats = [_align(80 + rng.uniform(-5, 5), 60 + rng.uniform(-5, 5), rng.uniform(0.8, 1.2),
                   rng.uniform(-0.15, 0.15), fh, fw) for _ in range(N)]
    boxes = [[0, 0, fw, fh]] * N
    torch.save({"faces": faces, "boxes": boxes, "affine_matrices": mats}, tmp_path / "data.pth")
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    np.save(tmp_path / "video.npy", frames)
    seen = {}
    real = pipe.restore_video

    def spy(f, v, b, m):
        seen["faces"] = tuple(f.shape)
        return real(f, v, b, m)

    monkeypatch.setattr(pipe, "restore_video", spy)
    out_path = str(tmp_path / "out.npz")
    pipe(video_path=str(tmp_path / "video.npy"), audio_path=str(tmp_path / "audio.wav"), video_out_path=out_path,
         num_frames=Fr, num_inference_steps=STEPS, guidance_scale=1.0, height=Rr, width=Rr,
         data_path=str(tmp_path / "data.pth"), mask_image_path=None,
         generator=torch.Generator(device="cuda").manual_seed(1247))
    out = np.load(out_path)["frames"]
    n = out.shape[0]
    assert 0 < n <= N and n % Fr == 0 and out.shape[1:] == (H, W, 3) and out.dtype == np.uint8
    assert seen["faces"] == (n, 3, Rr, Rr)
    assert (out != frames[:n]).any()
    pipe.close()


def test_image_processor_prepare_masks_and_masked_images(gpu):
    from latentsync_amd import ImageProcessor
    faces = smooth_faces(Fr, 128, 128, 71)
    ip = ImageProcessor(Rr, device="cuda", mask_image=load_fixed_mask(Rr))
    pix, masked, masks = ip.prepare_masks_and_masked_images(faces)
    assert pix.shape == (Fr, 3, Rr, Rr) and masked.shape == (Fr, 3, Rr, Rr) and masks.shape == (Fr, 1, Rr, Rr)
    assert pix.dtype == masked.dtype == masks.dtype == torch.float32 and pix.is_cuda
    small = oracle_resize(faces, Rr, Rr)
    want = small.float() / 255 * 2 - 1
    v64 = F.interpolate(faces.double(), size=(Rr, Rr), mode="bilinear", align_corners=False, antialias=True)
    near = ((v64 - torch.floor(v64)) - 0.5).abs() < TIE
    d = (pix.cpu() - want).abs()
    assert torch.equal(pix.cpu()[~near], want[~near])
    assert float(d.max()) <= 2 / 255 + 1e-6
    assert torch.equal(masked, pix * masks)
    assert torch.equal(masks.cpu(), load_fixed_mask(Rr)[None, None].expand(Fr, 1, Rr, Rr))
    # channels-last input (the reference's shape[3] == 3 rule), process_images, resize
    assert torch.equal(ip.process_images(faces.permute(0, 2, 3, 1).numpy()), pix)
    assert_tie_aware(ip.resize(faces).cpu(), small, near, "ImageProcessor.resize 128 -> 64")
    one = ip.preprocess_fixed_mask_image(faces[0])
    assert one[0].shape == (3, Rr, Rr) and one[2].shape == (1, Rr, Rr) and torch.equal(one[0], pix[0])
