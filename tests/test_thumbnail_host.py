"""The GIF thumbnail's host side (latentsync_amd/thumbnail.py) and the CPU restatement of its
device side (tests/thumb_cpu.py), without a GPU: the reference's frame selection and size
rules, the overlay layers against Pillow's own ImageDraw on the frame, the strip LZW stream
and the container against Pillow's GIF reader and the restatement's own decoder, the
palette's quality against Pillow's median cut, and serve.run_job's gif_url."""
import os

import numpy as np
import pytest

import mjpeg_cpu as mj
import thumb_cpu as tc
from latentsync_amd import serve as S
from latentsync_amd import thumbnail as T


def test_select_frames():
    assert T.select_frames(150, 25, 6, 3) == [0, 8, 16]
    assert T.select_frames(150, 25) == [0, 5, 10]  # duration 3, fps 5: 15 source frames, every 5th
    assert T.select_frames(10, 25, 6, 3) == [0, 8]
    assert T.select_frames(1, 30, 6, 3) == [0]
    with pytest.raises(ValueError, match="interval"):
        T.select_frames(150, 2, 6, 3)
    with pytest.raises(ValueError, match="no frame"):
        T.select_frames(0, 25, 6, 3)
    with pytest.raises(ValueError, match="no frame"):
        T.select_frames(150, 25, 0.1, 3)


def test_thumbnail_size():
    assert T.thumbnail_size(1920, 1080) == (640, 360)
    assert T.thumbnail_size(1923, 90) == (640, 29)  # int(640 / 21.366...) = int(29.95...)
    assert T.thumbnail_size(640, 360) == (640, 360)
    assert T.thumbnail_size(700, 33, max_width=640) == (640, 30)


# ------------------------------------------------------------------ overlay against Pillow


def pinned_font(size):
    """(what to pass as font=, the same font as an object)."""
    from PIL import ImageFont
    try:
        f = ImageFont.truetype("DejaVuSans.ttf", size=size)
        return f.path, f
    except OSError:
        f = ImageFont.load_default(size)
        return f, f


def draw_on_frame(frame, text, font):
    """The reference's draw calls (thumbnail.py:153-234) made with ImageDraw directly on the
    frame in "RGBA" mode, which blends every call with its ink's alpha."""
    from PIL import Image, ImageDraw
    img = Image.fromarray(frame)
    d = ImageDraw.Draw(img, "RGBA")
    w, h = img.size
    cx, cy, sz = w // 2, h // 2, min(w, h) // 3
    d.ellipse([(cx - sz // 2, cy - sz // 2), (cx + sz // 2, cy + sz // 2)], fill=(0, 0, 0, 128))
    d.polygon([(cx - sz // 4, cy - sz // 3), (cx + sz // 3, cy), (cx - sz // 4, cy + sz // 3)], fill=(255, 255, 255, 180))
    shown = T.truncate_text(text, font, w - 40)
    tw, th = T.text_size(shown, font)
    left, top = (w - tw) // 2 - 20, h - th - 20 - 10
    d.rectangle([left, top, left + tw + 40, top + th + 20], fill=(0, 0, 0, 180))
    tx, ty = (w - tw) // 2, top + 10
    for ox, oy in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        d.text((tx + ox, ty + oy), shown, font=font, fill=(0, 0, 0, 255))
    d.text((tx, ty), shown, font=font, fill=(255, 255, 255, 255))
    return np.array(img), shown


@pytest.mark.parametrize("H,W,text", [(48, 80, "Hi"), (361, 641, "Hello there Henrik, I wanted to show you how this "
                                                      "works on a subtitle that is far too long to fit")])
def test_layers_equal_imagedraw_on_the_frame(H, W, text):
    pytest.importorskip("PIL")
    arg, font = pinned_font(max(18, H // 14))
    frame = mj.noise_frame(H, W, 3)
    want, shown = draw_on_frame(frame, text, font)
    layers = T.overlay_layers(W, H, text, font=arg)
    assert len(layers) == 8 and len(layers) <= T.MAX_LAYERS
    assert [l[3] for l in layers] == [(0, 0, 0), (255, 255, 255)] + [(0, 0, 0)] * 5 + [(255, 255, 255)]
    assert set(np.unique(layers[0][2])) <= {0, 128} and set(np.unique(layers[2][2])) <= {0, 180}
    for x0, y0, a, _ in layers:
        assert a.dtype == np.uint8 and x0 >= 0 and y0 >= 0 and x0 + a.shape[1] <= W and y0 + a.shape[0] <= H
    got = tc.composite(frame, layers)
    assert (got != frame).any()
    assert np.array_equal(got, want)
    if W > 600:
        assert shown.endswith("...") and len(shown) < len(text)
        assert 64 < layers[7][2].max() <= 255 and len(np.unique(layers[7][2])) > 2  # antialiased glyph coverage


def test_missing_pillow_is_named(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(RuntimeError, match="Pillow"):
        T.overlay_layers(80, 48, "x")


# ------------------------------------------------------------------ the stream


SHAPES = [(37, 53), (64, 640), (5, 3), (16, 1024)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_stream_opens_in_pillow_and_in_the_own_decoder(tmp_path, H, W):
    Image = pytest.importorskip("PIL.Image")
    pal = tc.distinct_palette()
    for name, idx in tc.index_contents(H, W).items():
        data, offsets = tc.lzw_strips(idx[None])
        assert offsets == [0, len(data)]
        path = str(tmp_path / f"{name}.gif")
        size = T.write_gif(path, data, offsets, pal, W, H, 33)
        blob = open(path, "rb").read()
        assert size == len(blob) == os.path.getsize(path)
        g = tc.parse_gif(blob)
        assert (g["width"], g["height"], g["loop"]) == (W, H, 0) and np.array_equal(g["palette"], pal)
        assert len(g["frames"]) == 1 and g["frames"][0]["delay"] == 33 and g["frames"][0]["disposal"] == 0
        assert g["frames"][0]["box"] == (0, 0, W, H) and np.array_equal(g["frames"][0]["idx"], idx), name
        if (H, W, name) == (64, 640, "noise"):
            # 5120 pixels a strip fill the dictionary: CLEARs beyond one per strip
            assert g["frames"][0]["clears"] > (H + tc.STRIP_ROWS - 1) // tc.STRIP_ROWS
        with Image.open(path) as im:
            assert im.size == (W, H) and im.n_frames == 1
            assert im.info["duration"] == 330 and im.info["loop"] == 0
            assert np.array_equal(np.array(im.convert("RGB")), pal[idx]), name


def test_three_frames_of_different_lengths(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    H, W = 37, 53
    idx = np.stack(list(tc.index_contents(H, W).values()))
    data, offsets = tc.lzw_strips(idx)
    sizes = np.diff(offsets)
    assert len(offsets) == 4 and len(set(sizes.tolist())) == 3 and offsets[-1] == len(data)
    pal = tc.distinct_palette()
    path = str(tmp_path / "three.gif")
    T.write_gif(path, np.frombuffer(data, np.uint8), np.array(offsets), pal, W, H, 20)
    g = tc.parse_gif(open(path, "rb").read())
    assert g["loop"] == 0 and [f["delay"] for f in g["frames"]] == [20] * 3
    assert all(np.array_equal(f["idx"], idx[i]) for i, f in enumerate(g["frames"]))
    with Image.open(path) as im:
        assert im.n_frames == 3 and im.info["loop"] == 0
        for f in range(3):
            im.seek(f)
            assert im.info["duration"] == 200
            assert np.array_equal(np.array(im.convert("RGB")), pal[idx[f]])


def test_sub_blocks_are_255_bytes(tmp_path):
    idx = tc.index_contents(64, 640)["noise"][None]
    data, offsets = tc.lzw_strips(idx)
    path = str(tmp_path / "b.gif")
    T.write_gif(path, data, offsets, tc.distinct_palette(), 640, 64, 33)
    blob = open(path, "rb").read()
    pos = 13 + 768 + 19 + 8 + 10 + 1  # header + table + loop extension + control extension + descriptor + code size
    assert blob[pos - 1] == 8
    lengths = []
    while blob[pos]:
        lengths.append(blob[pos])
        pos += 1 + blob[pos]
    assert set(lengths[:-1]) == {255} and sum(lengths) == len(data) and blob[pos + 1] == 0x3B


# ------------------------------------------------------------------ palette quality


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_palette_no_worse_than_pillows_median_cut(kind):
    """Both figures are measured here, on identical pixels: ours must reach Pillow's
    quantize(256, MEDIANCUT, dither NONE) of the three frames stacked into one image."""
    Image = pytest.importorskip("PIL.Image")
    frames = mj.smooth_frames(3, 90, 160, 5) if kind == "smooth" else np.stack([mj.noise_frame(90, 160, s)
                                                                                 for s in (1, 2, 3)])
    palette, lut = T.design_palette(tc.hist555(frames))
    assert palette.shape == (256, 3) and palette.dtype == np.uint8 and lut.shape == (32768,) and lut.dtype == np.uint8
    ours = psnr(palette[tc.map_palette(frames, lut)], frames)
    stacked = Image.fromarray(frames.reshape(-1, 160, 3))
    q = stacked.quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE)
    theirs = psnr(np.array(q.convert("RGB")), frames.reshape(-1, 160, 3))
    print(f"{kind}: design_palette {ours:.2f} dB, Pillow MEDIANCUT {theirs:.2f} dB")
    assert ours >= theirs
    p2, l2 = T.design_palette(tc.hist555(frames))
    assert np.array_equal(p2, palette) and np.array_equal(l2, lut)  # deterministic


def test_lut_is_the_nearest_entry_lowest_index_on_ties():
    hist = np.zeros(32768, np.int64)
    hist[[0, 31, 32767]] = [5, 1, 9]  # three colours: three boxes, 253 unused (black) entries
    palette, lut = T.design_palette(hist)
    centres = np.array([[4, 4, 4], [4, 4, 252], [252, 252, 252]])
    assert sorted(map(tuple, palette[:3].tolist())) == sorted(map(tuple, centres.tolist()))
    assert (palette[3:] == 0).all()
    keys = np.arange(32768)
    c = np.stack([(keys >> 10) & 31, (keys >> 5) & 31, keys & 31], 1) * 8 + 4
    d = ((c[:, None, :] - palette[None].astype(np.int64)) ** 2).sum(2)
    assert np.array_equal(lut, d.argmin(1)) and lut.max() <= 3
    with pytest.raises(ValueError):
        T.design_palette(np.zeros(32768, np.int64))


# ------------------------------------------------------------------ serve.run_job


class StubPipeline:
    def __init__(self, make_gif):
        self.calls, self.make_gif = [], make_gif

    def __call__(self, **kw):
        self.calls.append(kw)
        open(kw["video_out_path"], "wb").close()
        if self.make_gif and kw.get("thumbnail_path"):
            open(kw["thumbnail_path"], "wb").close()


def _job(tmp_path, pipe, **extra):
    for n in ("v1.mp4", "v1.pth", "r1.wav"):
        open(os.path.join(tmp_path, n), "wb").close()
    payload = dict(id="r1", video_id="v1", audio_url="unused", **extra)
    return S.run_job(pipe, payload, str(tmp_path), str(tmp_path / "results"), 256)


def test_run_job_fills_gif_url_for_a_dynamic_clip_with_text(tmp_path):
    pipe = StubPipeline(make_gif=True)
    plain = _job(tmp_path, pipe)
    reply = _job(tmp_path, pipe, is_dynamic_clip=True, text="Hello")
    gif = str(tmp_path / "results" / "r1.gif")
    assert reply["gif_url"] == gif and os.path.exists(gif)
    assert pipe.calls[1]["thumbnail_path"] == gif and pipe.calls[1]["thumbnail_text"] == "Hello"
    assert set(reply) == set(plain) == {"message", "output_url", "gif_url", "elapsed_time", "request_uuid"}
    assert plain["gif_url"] is None
    assert {k: v for k, v in pipe.calls[1].items() if not k.startswith("thumbnail_")} == pipe.calls[0]


@pytest.mark.parametrize("extra", [{}, {"is_dynamic_clip": True}, {"text": "Hello"},
                                   {"is_dynamic_clip": True, "text": ""}, {"is_dynamic_clip": False, "text": "Hello"}])
def test_run_job_other_requests_are_unchanged(tmp_path, extra):
    pipe = StubPipeline(make_gif=True)
    reply = _job(tmp_path, pipe, **extra)
    assert reply["gif_url"] is None and not any(k.startswith("thumbnail") for k in pipe.calls[0])
    assert not os.path.exists(tmp_path / "results" / "r1.gif")


def test_run_job_gif_url_is_none_when_no_file_was_made(tmp_path):
    os.makedirs(tmp_path / "results")
    stale = tmp_path / "results" / "r1.gif"
    stale.write_bytes(b"an earlier request's file")
    pipe = StubPipeline(make_gif=False)
    reply = _job(tmp_path, pipe, is_dynamic_clip=True, text="Hello")
    assert pipe.calls[0]["thumbnail_path"] == str(stale)
    assert reply["gif_url"] is None and not stale.exists()
