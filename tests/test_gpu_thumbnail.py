"""The GIF thumbnail's kernels on MI355X (csrc/ls_thumb.hip) against their CPU restatement
(tests/thumb_cpu.py), exact equality throughout -- resize values, blended pixels, counts,
indices, LZW bytes and offsets -- then create_video_thumbnail_gif and __call__'s
thumbnail_path= end to end, read back with the restatement's own GIF parser."""
import functools

import numpy as np
import pytest
import torch

import mjpeg_cpu as mj
import thumb_cpu as tc
from latentsync_amd import _lib, ops
from latentsync_amd import thumbnail as T

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(n, H, W, seed=0):
    return np.stack([mj.noise_frame(H, W, seed + i) for i in range(n)])


# ------------------------------------------------------------------ resize


@pytest.mark.parametrize("shape,out", [((1, 7, 9), (3, 4)),          # both axes fractional, cells straddle
                                       ((1, 12, 1920), (4, 640)),    # integer factor 3 on both axes
                                       ((2, 90, 1923), (29, 640)),   # the max_width path, factor just above 3
                                       ((3, 33, 700), (30, 640)),
                                       # factor 10 / 7: weights 0.7, 0.3, 0.4 ... put many sums on exact .5
                                       # ties, which a fused multiply-add rounds the other way
                                       ((3, 48, 80), (33, 56)),
                                       ((1, 11, 20), (4, 20)),       # dw == W, dh < H
                                       ((1, 8, 10), (4, 5)),         # 2 x 2: (s + 2) >> 2
                                       ((1, 6, 8), (6, 8))])         # equal sizes: a copy
def test_resize_area_equals_the_restatement(gpu, shape, out):
    frames = noise(*shape, seed=shape[2])
    want = tc.resize_area(frames, *out)
    got = ops.resize_area_u8(dev(frames), *out)
    assert got.shape == (shape[0], out[0], out[1], 3) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    print(f"{shape} -> {out}: {(got != want).sum()} of {want.size} values differ")
    assert np.array_equal(got, want)
    if shape[1:] == out:
        assert np.array_equal(got, frames)


def test_resize_area_validation(gpu):
    lib = _lib.load()
    assert lib.ls_resize_area_u8(16, 1, 8, 8, 16, 9, 8, None) == 1 and b"downscale" in lib.ls_last_error()
    assert lib.ls_resize_area_u8(16, 1, 8, 8, 16, 8, 9, None) == 1
    assert lib.ls_resize_area_u8(None, 1, 8, 8, 16, 4, 4, None) == 1
    assert lib.ls_resize_area_u8(16, 0, 8, 8, 16, 4, 4, None) == 1
    assert lib.ls_resize_area_u8(16, 1, 8, 8, 16, 0, 4, None) == 1
    with pytest.raises(RuntimeError, match="ls_resize_area_u8"):
        ops.resize_area_u8(torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda"), 5, 4)


# ------------------------------------------------------------------ blend


def blend_layers(H, W, count):
    """Overlapping layers, one flush with each edge, a 1 x 1 layer, an empty one, and alpha
    maps that hold 0, 1, 128, 254 and 255."""
    rng = np.random.default_rng(H * W + count)
    special = np.array([0, 1, 128, 254, 255], np.uint8)

    def amap(h, w):
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        a.reshape(-1)[:min(5, a.size)] = special[:min(5, a.size)]
        return a
    base = [(0, 3, amap(H - 6, 9), (255, 0, 10)),                 # left edge
            (W - 7, 0, amap(H, 7), (1, 254, 128)),                # right edge, top to bottom
            (2, 0, amap(5, W - 4), (0, 0, 0)),                    # top edge
            (0, H - 4, amap(4, W), (255, 255, 255)),              # bottom edge, full width
            (W // 2, H // 2, amap(1, 1) | 1, (9, 99, 199)),       # 1 x 1
            (3, 3, np.zeros((0, 0), np.uint8), (5, 5, 5)),        # empty
            (W // 4, H // 4, amap(H // 2, W // 2), (200, 100, 0)),
            (W // 3, H // 3, amap(H // 2, W // 2), (0, 100, 200))]  # overlaps the one before
    while len(base) < count:
        k = len(base)
        base.append((k, k, amap(H // 3, W // 3), (k * 13 % 256, k * 29 % 256, k * 53 % 256)))
    return base[:count]


@pytest.mark.parametrize("H,W", [(37, 53), (64, 641)])
@pytest.mark.parametrize("count", [0, 8, 16])
def test_blend_equals_the_restatement(gpu, H, W, count):
    frames = noise(2, H, W, seed=count)
    layers = blend_layers(H, W, count)
    assert len(layers) == count
    want = tc.composite(frames, layers)
    d = dev(frames)
    assert ops.overlay_blend_u8(d, layers) is d
    got = d.cpu().numpy()
    assert np.array_equal(got, want)
    assert (want != frames).any() == (count > 0)


def test_blend_validation(gpu):
    lib = _lib.load()
    import ctypes as C
    one = (C.c_int32 * 8)(0, 0, 2, 2, 0, 1, 2, 3)
    assert lib.ls_overlay_blend_u8(None, 1, 4, 4, one, 1, 16, 4, None) == 1
    assert lib.ls_overlay_blend_u8(16, 1, 4, 4, one, 17, 16, 4, None) == 1 and b"layers" in lib.ls_last_error()
    assert lib.ls_overlay_blend_u8(16, 1, 4, 4, one, 1, 16, 3, None) == 1 and b"alpha_bytes" in lib.ls_last_error()
    assert lib.ls_overlay_blend_u8(16, 1, 4, 4, (C.c_int32 * 8)(0, 0, 2, 2, 0, 256, 2, 3), 1, 16, 4, None) == 1
    assert lib.ls_overlay_blend_u8(16, 1, 4, 4, (C.c_int32 * 8)(0, 0, -1, 2, 0, 1, 2, 3), 1, 16, 4, None) == 1
    assert lib.ls_overlay_blend_u8(16, 1, 4, 4, None, 0, None, 0, None) == 0  # no layer: nothing to do
    with pytest.raises(RuntimeError, match="ls_overlay_blend_u8"):
        ops.overlay_blend_u8(torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda"),
                             [(0, 0, np.ones((1, 1), np.uint8), (0, 0, 0))] * 17)


# ------------------------------------------------------------------ histogram, map


def hist_frames():
    grey = np.zeros((1, 4, 8, 3), np.uint8)
    grey.reshape(-1, 3)[:] = (np.arange(32) * 8)[:, None]  # exactly the colours (8 i, 8 i, 8 i)
    return {"noise": noise(3, 17, 33, seed=40), "one colour": np.full((1, 64, 640, 3), (200, 17, 99), np.uint8),
            "greys": grey}


@pytest.mark.parametrize("name", ["noise", "one colour", "greys"])
def test_hist_and_map_equal_the_restatement(gpu, name):
    frames = hist_frames()[name]
    want = tc.hist555(frames)
    got = ops.rgb555_hist(dev(frames))
    assert got.shape == (32768,) and got.dtype == torch.int64
    got = got.cpu().numpy()
    assert int(got.sum()) == frames.shape[0] * frames.shape[1] * frames.shape[2]
    assert np.array_equal(got, want)
    if name == "one colour":
        assert np.count_nonzero(got) == 1 and got[(200 >> 3) << 10 | (17 >> 3) << 5 | 99 >> 3] == 64 * 640
    if name == "greys":
        assert np.array_equal(np.nonzero(got)[0], np.arange(32) * 1057) and (got[got > 0] == 1).all()
    lut = np.random.default_rng(8).integers(0, 256, 32768, dtype=np.uint8)
    idx = ops.palette_map(dev(frames), dev(lut))
    assert idx.shape == frames.shape[:3] and idx.dtype == torch.uint8
    assert np.array_equal(idx.cpu().numpy(), tc.map_palette(frames, lut))


def test_hist_and_map_validation(gpu):
    lib = _lib.load()
    assert lib.ls_rgb555_hist(None, 1, 4, 4, 16, None) == 1 and lib.ls_rgb555_hist(16, 1, 0, 4, 16, None) == 1
    assert lib.ls_palette_map(16, 1, 4, 4, None, 16, None) == 1 and lib.ls_palette_map(16, 0, 4, 4, 16, 16, None) == 1
    with pytest.raises(ValueError, match="lut"):
        ops.palette_map(torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda"),
                        torch.zeros(256, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------ LZW


@functools.lru_cache(maxsize=None)
def lzw_case(name):
    """(indices (n, H, W), the restatement's bytes, its offsets); computed once."""
    c = tc.index_contents
    shape, kind = name
    H, W = shape[1:]
    if shape[0] == 1:
        idx = c(H, W)[kind][None]
    elif shape[0] == 3:
        idx = np.stack([c(H, W)[k] for k in ("noise", "flat", "gradient")])
    else:
        idx = np.stack([c(H, W)["gradient"], c(H, W)["noise"]]) if kind == "mixed" else \
            np.stack([c(H, W)["flat"], c(H, W)["flat"]])
    data, offsets = tc.lzw_strips(idx)
    return idx, data, offsets


LZW_CASES = [((1, 5, 3), "noise"), ((1, 5, 3), "flat"), ((1, 5, 3), "gradient"),
             ((3, 37, 53), "all"),                                     # H % strip rows != 0, odd bit offsets
             ((1, 64, 640), "noise"), ((1, 64, 640), "flat"), ((1, 64, 640), "gradient"),
             ((2, 16, 1024), "mixed"), ((2, 16, 1024), "flat")]


@pytest.mark.parametrize("case", LZW_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_lzw_equals_the_restatement(gpu, case):
    assert _lib.load().ls_gif_strip_rows() == tc.STRIP_ROWS
    idx, data, offsets = lzw_case(case)
    got, off = ops.gif_lzw(dev(idx))
    assert got.dtype == torch.uint8 and off.dtype == torch.int64 and got.is_cuda and off.is_cuda
    assert off.cpu().tolist() == offsets
    got = got.cpu().numpy().tobytes()
    assert got == data
    n, H, W = idx.shape
    for f in range(n):
        px, clears = tc.lzw_decode(got[offsets[f]:offsets[f + 1]])
        assert px == idx[f].tobytes()
        if case == ((1, 64, 640), "noise"):
            assert clears > (H + tc.STRIP_ROWS - 1) // tc.STRIP_ROWS  # CLEARs in the middle of strips
    if n == 3:
        assert len({offsets[f + 1] - offsets[f] for f in range(3)}) == 3


def test_lzw_overflow_contract(gpu):
    """Bytes past out_capacity are dropped, the offsets stay exact, ops.gif_lzw repeats once."""
    idx, data, offsets = lzw_case(((3, 37, 53), "all"))
    lib = _lib.load()
    d = dev(idx)
    half = len(data) // 2
    out = torch.full((len(data),), 0xAA, dtype=torch.uint8, device="cuda")
    off = torch.zeros(4, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.ls_gif_lzw_workspace_bytes(3, 37, 53), dtype=torch.uint8, device="cuda")
    rc = lib.ls_gif_lzw(d.data_ptr(), 3, 37, 53, out.data_ptr(), half, off.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0 and off.cpu().tolist() == offsets
    out = out.cpu().numpy()
    assert out[:half].tobytes() == data[:half] and (out[half:] == 0xAA).all()
    got, off2 = ops.gif_lzw(d, capacity=half)
    assert got.cpu().numpy().tobytes() == data and off2.cpu().tolist() == offsets


def test_lzw_validation(gpu):
    lib = _lib.load()
    need = lib.ls_gif_lzw_workspace_bytes(1, 16, 16)
    assert need > 0 and lib.ls_gif_lzw_workspace_bytes(0, 16, 16) == 0 and lib.ls_gif_lzw_workspace_bytes(1, 0, 16) == 0
    assert lib.ls_gif_lzw_workspace_bytes(1, 16, 65536) == 0
    args = lambda idx=16, n=1, H=16, W=16, out=16, cap=64, off=16, ws=16, wsb=need: (idx, n, H, W, out, cap, off, ws,
                                                                                      wsb, None)
    for bad in (dict(idx=None), dict(out=None), dict(off=None), dict(n=0), dict(H=0), dict(W=0), dict(cap=-1)):
        assert lib.ls_gif_lzw(*args(**bad)) == 1, bad
        assert b"ls_gif_lzw" in lib.ls_last_error()
    assert lib.ls_gif_lzw(*args(wsb=need - 1)) == 3 and lib.ls_gif_lzw(*args(ws=None)) == 3
    with pytest.raises(ValueError, match="gif_lzw"):
        ops.gif_lzw(torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------ end to end


def pinned_font(size):
    from PIL import ImageFont
    try:
        return ImageFont.truetype("DejaVuSans.ttf", size=size).path
    except OSError:
        return ImageFont.load_default(size)


def restated_thumbnail(frames, video_fps, duration, fps, text, font, shrink=False):
    """The pipeline of create_video_thumbnail_gif with every device step replaced by its
    restatement -> (palette, indices (n, h, w))."""
    fr = frames[T.select_frames(len(frames), video_fps, duration, fps)]
    w, h = T.thumbnail_size(frames.shape[2], frames.shape[1])
    if (h, w) != fr.shape[1:3]:
        fr = tc.resize_area(fr, h, w)
    fr = tc.composite(fr, T.overlay_layers(w, h, text, font=font))
    if shrink:
        fr = tc.resize_area(fr, int(h * 0.7), int(w * 0.7))
    palette, lut = T.design_palette(tc.hist555(fr))
    return palette, tc.map_palette(fr, lut)


@pytest.mark.parametrize("H,W", [(48, 80), (90, 1923)])
def test_thumbnail_file_equals_the_restated_pipeline(gpu, tmp_path, H, W):
    pytest.importorskip("PIL")
    frames = mj.smooth_frames(20, H, W, 11)
    w, h = T.thumbnail_size(W, H)
    font = pinned_font(max(18, h // 14))
    text = "Hello there, this is the subtitle of the thumbnail and it is a long one"
    path = str(tmp_path / "t.gif")
    d = dev(frames)
    size = T.create_video_thumbnail_gif(d, 25, path, duration=6, fps=3, subtitle_text=text, font=font)
    assert np.array_equal(d.cpu().numpy(), frames)  # the caller's frames are not drawn on
    blob = open(path, "rb").read()
    assert size == len(blob)
    g = tc.parse_gif(blob)
    assert (g["width"], g["height"], g["loop"]) == (w, h, 0) and (w, h) == ((80, 48) if W == 80 else (640, 29))
    assert len(g["frames"]) == 3 and all(f["delay"] == 33 and f["disposal"] == 0 for f in g["frames"])
    palette, idx = restated_thumbnail(frames, 25, 6, 3, text, font)
    assert np.array_equal(g["palette"], palette)
    for f in range(3):
        assert np.array_equal(g["frames"][f]["idx"], idx[f]), f
    from PIL import Image
    with Image.open(path) as im:
        assert im.n_frames == 3 and im.size == (w, h)
        im.seek(2)
        assert np.array_equal(np.array(im.convert("RGB")), palette[idx[2]])


def test_size_cap_redoes_the_file_once_at_70_percent(gpu, tmp_path):
    pytest.importorskip("PIL")
    frames = mj.smooth_frames(20, 48, 80, 11)
    font = pinned_font(18)
    path = str(tmp_path / "t.gif")
    T.create_video_thumbnail_gif(dev(frames), 25, path, duration=6, fps=3, subtitle_text="Hi", font=font,
                                 max_size_mb=0.001)  # about 1 KB: never met, and still only one more pass
    g = tc.parse_gif(open(path, "rb").read())
    assert (g["width"], g["height"]) == (56, 33) and len(g["frames"]) == 3
    palette, idx = restated_thumbnail(frames, 25, 6, 3, "Hi", font, shrink=True)
    assert np.array_equal(g["palette"], palette) and all(np.array_equal(g["frames"][f]["idx"], idx[f])
                                                         for f in range(3))


def test_thumbnail_argument_errors(gpu, tmp_path):
    d = torch.zeros((4, 8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="interval"):
        T.create_video_thumbnail_gif(d, 2, str(tmp_path / "x.gif"), duration=6, fps=3)
    with pytest.raises(ValueError, match="device"):
        T.create_video_thumbnail_gif(d.cpu(), 25, str(tmp_path / "x.gif"))
    assert not (tmp_path / "x.gif").exists()


# ------------------------------------------------------------------ __call__

from test_gpu_resample import SCHED, STEPS, Fr, Rr, _align, models, write_wav  # noqa: E402,F401


def test_call_writes_the_thumbnail_and_leaves_the_avi_alone(gpu, models, tmp_path):
    pytest.importorskip("PIL")
    from latentsync_amd.audio import Audio2Feature
    from latentsync_amd.pipeline import LipsyncPipeline
    from latentsync_amd.scheduler import DDIMScheduler
    unet, vae = models
    H, W, fh, fw, N = 120, 160, 56, 48, 24
    pipe = LipsyncPipeline(vae, Audio2Feature.random(2, device="cuda"), unet, DDIMScheduler(**SCHED))
    rng = np.random.default_rng(6)
    write_wav(tmp_path / "audio.wav", rng.normal(0, 0.1, int(0.9 * 16000)).clip(-1, 0.999), 16000, "s16")
    low = torch.rand((N, 3, 8, 8), generator=torch.Generator().manual_seed(61))
    faces = (torch.nn.functional.interpolate(low, size=(Rr, Rr), mode="bicubic") * 255).round().clamp(0, 255)
    mats = [_align(80 + rng.uniform(-5, 5), 60 + rng.uniform(-5, 5), rng.uniform(0.8, 1.2),
                   rng.uniform(-0.15, 0.15), fh, fw) for _ in range(N)]
    torch.save({"faces": faces.to(torch.uint8), "boxes": [[0, 0, fw, fh]] * N, "affine_matrices": mats},
               tmp_path / "data.pth")
    np.save(tmp_path / "video.npy", mj.smooth_frames(N, H, W, 4))

    def run(out, **kw):
        pipe(video_path=str(tmp_path / "video.npy"), audio_path=str(tmp_path / "audio.wav"),
             video_out_path=str(tmp_path / out), num_frames=Fr, num_inference_steps=STEPS, guidance_scale=1.0,
             height=Rr, width=Rr, data_path=str(tmp_path / "data.pth"), mask_image_path=None,
             generator=torch.Generator(device="cuda").manual_seed(1247), **kw)
        return (tmp_path / out).read_bytes()
    gif = tmp_path / "thumb.gif"
    with_gif = run("a.avi", thumbnail_path=str(gif), thumbnail_text="Hello there")
    g = tc.parse_gif(gif.read_bytes())
    assert (g["width"], g["height"], g["loop"]) == (W, H, 0)
    assert 1 <= len(g["frames"]) <= 3 and all(f["delay"] == 33 for f in g["frames"])
    assert len(np.unique(g["frames"][0]["idx"])) > 16  # a picture, not a flat field
    without = run("b.avi")
    assert without == with_gif
    assert sorted(p.name for p in tmp_path.glob("*.gif")) == ["thumb.gif"]
    pipe.close()
