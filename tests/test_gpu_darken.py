"""Device face brightness restore on MI355X (csrc/ls_darken.hip, latentsync_amd/darken.py)
against the CPU restatement (tests/darken_cpu.py).  Every comparison is bit-exact: the
mask is float32 with a fixed order of rounded operations and everything after it is
8-bit, so there is no tolerance.  Then argument validation, and __call__ with
use_darken + face_landmarks equal to the restatement applied to the plain call's frames
(two plain runs of that recipe are bit-identical, which
test_gpu_mjpeg.py::test_call_writes_a_playable_avi relies on as well)."""
import functools

import numpy as np
import pytest
import torch

import darken_cpu as dc
from latentsync_amd import _lib, darken, ops
from latentsync_amd.audio import Audio2Feature
from latentsync_amd.config import TINY_MODEL
from latentsync_amd.pipeline import LipsyncPipeline
from latentsync_amd.scheduler import DDIMScheduler
from latentsync_amd.unet import UNet3DConditionModel
from latentsync_amd.vae import AutoencoderKL
from test_gpu_resample import SCHED, _align, write_wav

pytestmark = pytest.mark.gpu

# (H, W, n, missing frames, ellipse): the dilate box is 1, 2 (even: the anchor) and 3 wide.
# The first face sits near the top-left corner, so the blur reflects at two frame edges;
# frames 0-1 have no face (they take frame 5's mask x 0.8), 7-8 are a gap (the mask decays).
CASES = {
    "k1": (96, 128, 12, (0, 1, 7, 8), (0.22, 0.25, 0.13, 0.17)),
    "k2": (200, 232, 6, (3,), (0.55, 0.5, 0.2, 0.25)),
    "k3": (310, 420, 3, (), (0.8, 0.75, 0.15, 0.2)),  # bottom-right: the other two edges
}


@functools.lru_cache(maxsize=None)
def case(name):
    H, W, n, missing, (cx, cy, rx, ry) = CASES[name]
    assert darken.dilate_size(H, W) == int(name[1])
    frames = dc.noise_gradient_frames(n, H, W, 5 + H)
    lm = dc.ellipse_landmarks(n, 478, cx, cy, rx, ry, missing=missing, seed=H, drift=(3.0 / W, 2.0 / H))
    frames.setflags(write=False)
    lm.setflags(write=False)
    return frames, lm


@functools.lru_cache(maxsize=None)
def reference(name, f):
    frames, lm = case(name)
    ref = dc.enhance_face_brightness(frames, lm, f)
    ref.setflags(write=False)
    return ref


def run(frames, lm, f, **kw):
    dev = torch.from_numpy(np.array(frames)).cuda()
    out = darken.enhance_face_brightness(dev, lm, f, **kw)
    assert out.data_ptr() == dev.data_ptr()  # in place
    return out.cpu().numpy()


def assert_equal(got, want):
    bad = np.flatnonzero((got != want).any(axis=(1, 2, 3)))
    assert bad.size == 0, f"frames {bad.tolist()} differ, max {np.abs(got.astype(int) - want.astype(int)).max()}"


@pytest.mark.parametrize("name,f", [("k1", 1.25), ("k1", 0.8), ("k2", 1.25), ("k3", 1.25)])
def test_equals_the_restatement(gpu, name, f):
    frames, lm = case(name)
    want = reference(name, f)
    assert (want != frames).any()
    assert_equal(run(frames, lm, f), want)
    if f > 1:
        assert want.max() <= 235


def test_batch_boundaries_carry_the_state(gpu):
    """5 frames a batch: boundaries fall inside the detected run 2-6 (after frame 4) and
    inside the decay and the run after it (after frame 9); first_valid (frame 5) lies in a
    later batch than the frames 0-1 it serves."""
    frames, lm = case("k1")
    for f in (1.25, 0.8):
        assert_equal(run(frames, lm, f, frames_per_batch=5), reference("k1", f))
    assert_equal(run(frames, lm, 1.25, frames_per_batch=1), reference("k1", 1.25))


def test_passthrough(gpu):
    frames, lm = case("k1")
    none = np.full_like(lm, np.nan)
    assert_equal(run(frames, none, 1.25), frames)
    only3 = none[:4].copy()
    only3[3] = lm[3]
    got = run(frames[:4], only3, 1.25)
    assert_equal(got[:3], frames[:3])
    assert_equal(got, dc.enhance_face_brightness(frames[:4], only3, 1.25))
    assert (got[3] != frames[3]).any()


def test_unaligned_frames_and_brightness_one(gpu):
    """33 x 17 frames: 3 H W is odd, so the byte path runs (frame 1 starts at an odd
    address) and the last thread holds fewer than 4 pixels.  f = 1.0 is the reference's
    "no change" mode: the HSV round trip alone."""
    frames = dc.noise_gradient_frames(3, 33, 17, 9)
    lm = dc.ellipse_landmarks(3, 60, 0.5, 0.5, 0.3, 0.3, seed=4)
    for f in (1.25, 1.0):
        assert_equal(run(frames, lm, f), dc.enhance_face_brightness(frames, lm, f))


@pytest.mark.parametrize("kind", ["identical", "collinear"])
def test_degenerate_hulls(gpu, kind):
    H, W, n, P = 48, 56, 2, 30
    lm = np.empty((n, P, 2), np.float32)
    k = np.arange(P)
    for i in range(n):  # pixel centres: one point, or a diagonal run that stays a diagonal when expanded
        lm[i, :, 0] = (28 + 0.5) / W if kind == "identical" else (10 + k + 0.5) / W
        lm[i, :, 1] = (19 + 2 * i + 0.5) / H if kind == "identical" else (8 + i + k + 0.5) / H
    a, b = darken.face_hulls(lm[0], H, W)
    assert len(a) == len(b) == (1 if kind == "identical" else 2)
    frames = dc.noise_gradient_frames(n, H, W, 3)
    want = dc.enhance_face_brightness(frames, lm, 1.25)
    assert (want != frames).any()
    assert_equal(run(frames, lm, 1.25), want)


def test_validation(gpu):
    lib = _lib.load()
    frames, lm = case("k1")
    n, H, W, _ = frames.shape
    taps = darken.gaussian_taps(40)
    plan, verts, fv, roi = darken.build_tables(lm, H, W, len(taps))
    dev = torch.from_numpy(np.array(frames)).cuda()
    args = dict(plan=plan, verts=verts, first_valid=fv, roi=roi, taps=taps, dilate=1, c=0.25, brighten=True)
    ops.face_brighten(dev.clone(), **args)  # the arguments are good
    for bad, msg in ((dict(taps=taps[:80]), "tap count"), (dict(taps=taps[:0]), "(null pointer|tap count)"),
                     (dict(dilate=0), "dilate size"), (dict(roi=(0, 0, W + 1, 4)), "region of interest"),
                     (dict(roi=(0, 0, 0, 4)), "region of interest"), (dict(first_valid=n), "first_valid"),
                     (dict(taps=np.ones(131, np.float32) / 131), "tap count")):
        with pytest.raises(RuntimeError, match="ls_face_brighten.*" + msg):
            ops.face_brighten(dev, **{**args, **bad})
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.face_brighten(dev, workspace=torch.empty(1024, dtype=torch.uint8, device="cuda"), **args)
    with pytest.raises(ValueError, match="contiguous"):
        ops.face_brighten(dev[:, :, ::2], **args)
    with pytest.raises(ValueError, match="uint8"):
        ops.face_brighten(dev.float(), **args)
    with pytest.raises(ValueError, match="plan"):
        ops.face_brighten(dev, **{**args, "plan": plan[:3]})
    assert torch.equal(dev.cpu(), torch.from_numpy(np.array(frames)))  # nothing was launched
    # straight at the C ABI: the pointers are never dereferenced
    call = lambda fr=16, n_=1, H_=16, W_=16, ws=16, wsb=1 << 30: lib.ls_face_brighten(
        fr, n_, H_, W_, 16, 16, 1, -1, 0, 0, 8, 8, 16, 81, 1, 0.25, 1, 235, 0, ws, wsb, None)
    assert call(fr=None) == 1 and call(n_=0) == 1 and call(H_=0) == 1 and call(W_=65536) == 1
    assert b"ls_face_brighten" in lib.ls_last_error()
    assert call(ws=None, wsb=0) == 3 and call(wsb=1024) == 3
    assert lib.ls_face_brighten_workspace_bytes(0, 8, 8, 0) == 0 and lib.ls_face_brighten_workspace_bytes(1, 0, 8, 0) == 0
    # the workspace holds one batch: it does not grow with n past the batch
    assert lib.ls_face_brighten_workspace_bytes(1000, 64, 64, 5) == lib.ls_face_brighten_workspace_bytes(5, 64, 64, 5)
    assert lib.ls_face_brighten_workspace_bytes(10 ** 6, 700, 700, 0) < 128 << 20
    with pytest.raises(ValueError, match="landmark rows"):
        darken.enhance_face_brightness(dev, lm[:3], 1.25)


# ---------------------------------------------------------------- __call__

Fr, Rr, STEPS = 8, 64, 2


def test_call_brightens_the_restored_frames(gpu, tmp_path):
    """The __call__ recipe of test_gpu_mjpeg.py::test_call_writes_a_playable_avi, once plain
    and once with use_darken and landmarks: the second result is the restatement applied to
    the first (the landmarks are cut to the output length together with the faces)."""
    unet = UNet3DConditionModel(**TINY_MODEL).init_weights(9).to("cuda").eval()
    vae = AutoencoderKL(block_out_channels=(32, 64, 64, 64)).init_weights(10).to("cuda")
    H, W, fh, fw, N = 120, 160, 56, 48, 24
    pipe = LipsyncPipeline(vae, Audio2Feature.random(2, device="cuda"), unet, DDIMScheduler(**SCHED))
    rng = np.random.default_rng(6)
    write_wav(tmp_path / "audio.wav", rng.normal(0, 0.1, (int(0.56 * 44100), 2)).clip(-1, 0.999), 44100, "s16")
    low = torch.rand((N, 3, 8, 8), generator=torch.Generator().manual_seed(61))
    faces = (torch.nn.functional.interpolate(low, size=(Rr, Rr), mode="bicubic") * 255).round().clamp(0, 255)
    mats = [_align(80 + rng.uniform(-5, 5), 60 + rng.uniform(-5, 5), rng.uniform(0.8, 1.2),
                   rng.uniform(-0.15, 0.15), fh, fw) for _ in range(N)]
    torch.save({"faces": faces.to(torch.uint8), "boxes": [[0, 0, fw, fh]] * N, "affine_matrices": mats},
               tmp_path / "data.pth")
    np.save(tmp_path / "video.npy", dc.noise_gradient_frames(N, H, W, 77))
    lm = dc.ellipse_landmarks(N, 478, 0.5, 0.5, 0.2, 0.3, missing=(0, 6, 7, 20), seed=8, drift=(0.004, 0.003))
    np.save(tmp_path / "lm.npy", lm)
    kw = dict(video_path=str(tmp_path / "video.npy"), audio_path=str(tmp_path / "audio.wav"), num_frames=Fr,
              num_inference_steps=STEPS, guidance_scale=1.0, height=Rr, width=Rr, data_path=str(tmp_path / "data.pth"),
              mask_image_path=None)
    seed = lambda: torch.Generator(device="cuda").manual_seed(1247)
    pipe(video_out_path=str(tmp_path / "plain.npz"), generator=seed(), **kw)
    pipe(video_out_path=str(tmp_path / "bright.npz"), generator=seed(), use_darken=True, brightness_factor=1.25,
         face_landmarks=str(tmp_path / "lm.npy"), **kw)
    with pytest.raises(ValueError, match="landmark rows"):
        pipe(video_out_path=str(tmp_path / "x.npz"), generator=seed(), use_darken=True, brightness_factor=1.25,
             face_landmarks=lm[:5], **kw)
    with pytest.raises(ValueError, match="yields no frames"):
        pipe(video_out_path=str(tmp_path / "x.npz"), generator=seed(), use_darken=True, brightness_factor=1.25,
             face_landmarks=lm, **{**kw, "video_path": str(tmp_path / "missing.npy")})
    pipe.close()
    plain, bright = np.load(tmp_path / "plain.npz"), np.load(tmp_path / "bright.npz")
    n = plain["frames"].shape[0]
    assert 0 < n < N and bright["frames"].shape == plain["frames"].shape
    assert np.array_equal(plain["audio"], bright["audio"])
    want = dc.enhance_face_brightness(plain["frames"], lm[:n], 1.25)
    assert (want != plain["frames"]).any() and want.max() <= 235
    assert_equal(bright["frames"], want)
