"""The reply's GIF thumbnail -- create_video_thumbnail_gif (latentsync/utils/thumbnail.py
of the reference, called from scripts/api.py:164-174) -- made from the result's frames
where they already are, on the device.

The reference re-opens its mp4, resizes with cv2 (INTER_AREA), draws a play button and the
subtitle with Pillow and lets imageio / Pillow quantise and LZW-code every frame on one
core.  Here the host only designs tables and writes the container:

  frames (device) -> select -> ops.resize_area_u8 -> ops.overlay_blend_u8 (layers
  rasterised once by Pillow: shapes and glyphs, never frames) -> ops.rgb555_hist ->
  design_palette (host, 32768 counts in, 256 colours + a 32768-entry table out) ->
  ops.palette_map -> ops.gif_lzw -> write_gif (host: headers and sub-block framing).

What crosses to the host is the histogram (128 KB) and the LZW bytes; what crosses to the
device is the overlay's alpha maps and the table (32 KB).  DESIGN.md section 4.6.

Deviations from the reference, both deliberate: one global 256-colour table without
dithering instead of Pillow's per-frame palettes, and a size cap that retries once at
70 % of the size (the reference's `compress_gif` severe branch) -- its mild branch re-saves
with imageio's `nq` quantiser, which is not carried.
"""
import os
import struct

import numpy as np

DEFAULT_SUBTITLE = "Hello there Henrik, I wanted to show you..."
MAX_LAYERS = 16
_FONT_SEARCH = ("Arial.ttf", "DejaVuSans.ttf", "/System/Library/Fonts/Helvetica.ttc",
                "/usr/share/fonts/truetype/dejavu/DejaVuSans.ttf")


def _pil():
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError as e:
        raise RuntimeError("the thumbnail's play button and subtitle are rasterised with Pillow, which is not "
                           "installed (pip install Pillow)") from e
    return Image, ImageDraw, ImageFont


def select_frames(n_frames, video_fps, duration=3, fps=5):
    """Indices of the frames the reference keeps (thumbnail.py:100-141): frame i for
    i < int(duration * fps), i < n_frames and i % int(video_fps / fps) == 0.

    The oddity is the reference's and is kept: ``int(duration * fps)`` -- the number of GIF
    frames wanted -- bounds the *source* frame index, so the GIF shows the first
    duration * fps source frames subsampled, not the first ``duration`` seconds: duration 6
    at 3 frames/s from a 25 frames/s clip is frames 0, 8 and 16 (0.64 s of video played
    over one second), not 18 frames spanning six seconds."""
    interval = int(video_fps / fps)
    if interval == 0:
        raise ValueError(f"thumbnail fps {fps} above the video's {video_fps}: the frame interval int(video_fps / fps) "
                         "is 0")
    sel = [i for i in range(min(int(duration * fps), int(n_frames))) if i % interval == 0]
    if not sel:
        raise ValueError(f"no frame selected from {n_frames} frames (duration {duration}, fps {fps})")
    return sel


def thumbnail_size(width, height, max_width=640):
    """(width, height) of the thumbnail (thumbnail.py:89-98), in Python floats as there."""
    if width > max_width:
        return max_width, int(max_width / (width / height))
    return width, height


def load_font(font, size):
    """``font``: None (the reference's search: Arial, DejaVuSans, two system paths, then
    Pillow's default), a path (loaded at ``size``) or a Pillow font object (used as it is)."""
    _, _, ImageFont = _pil()
    if font is not None:
        return ImageFont.truetype(os.fspath(font), size=size) if isinstance(font, (str, os.PathLike)) else font
    for name in _FONT_SEARCH:
        try:
            return ImageFont.truetype(name, size=size)
        except OSError:
            continue
    return ImageFont.load_default()


def text_size(text, font):
    if hasattr(font, "getbbox"):
        l, t, r, b = font.getbbox(text)
        return r - l, b - t
    return int(font.getlength(text)), font.size


def truncate_text(text, font, max_width):
    """The longest prefix that fits max_width together with '...' (the whole text if it fits)."""
    if text_size(text, font)[0] <= max_width:
        return text
    room = max_width - text_size("...", font)[0]
    kept = ""
    for ch in text:
        if text_size(kept + ch, font)[0] > room:
            break
        kept += ch
    return kept + "..."


def overlay_layers(width, height, text, font=None):
    """The reference's draw calls (thumbnail.py:153-234) on a width x height frame, in order,
    as layers for ops.overlay_blend_u8: a list of (x0, y0, alpha uint8 (h, w), (r, g, b)).
    Each call is drawn with ImageDraw on an "L" image of the frame's size -- a shape with its
    ink's alpha as the fill (the map is that alpha inside, 0 outside), text with 255 (the map
    is the glyph coverage) -- and cropped to its bounding box; a call that leaves no pixel
    is an empty layer.  Blending the layers in order with Pillow's own formula gives what
    ImageDraw.Draw(frame, "RGBA") gives (tests/test_thumbnail_host.py)."""
    Image, ImageDraw, _ = _pil()
    font = load_font(font, max(18, height // 14))
    layers = []

    def layer(ink, alpha, draw):
        img = Image.new("L", (width, height), 0)
        draw(ImageDraw.Draw(img), alpha)
        box = img.getbbox()
        if box is None:
            layers.append((0, 0, np.zeros((0, 0), np.uint8), ink))
        else:
            layers.append((box[0], box[1], np.array(img.crop(box), dtype=np.uint8), ink))

    cx, cy, size = width // 2, height // 2, min(width, height) // 3
    layer((0, 0, 0), 128, lambda d, a: d.ellipse([(cx - size // 2, cy - size // 2), (cx + size // 2, cy + size // 2)],
                                                 fill=a))
    layer((255, 255, 255), 180, lambda d, a: d.polygon([(cx - size // 4, cy - size // 3), (cx + size // 3, cy),
                                                        (cx - size // 4, cy + size // 3)], fill=a))
    shown = truncate_text(text, font, width - 40)
    tw, th = text_size(shown, font)
    pad_x, pad_y = 20, 10
    left = (width - tw) // 2 - pad_x
    top = height - th - 20 - pad_y
    layer((0, 0, 0), 180, lambda d, a: d.rectangle([left, top, left + tw + 2 * pad_x, top + th + 2 * pad_y], fill=a))
    tx, ty = (width - tw) // 2, top + pad_y
    for ox, oy in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        layer((0, 0, 0), 255, lambda d, a, ox=ox, oy=oy: d.text((tx + ox, ty + oy), shown, font=font, fill=a))
    layer((255, 255, 255), 255, lambda d, a: d.text((tx, ty), shown, font=font, fill=a))
    return layers


# --------------------------------------------------------------------------- palette


def _box_stats(w, col):
    """(pixels, per-axis sum, per-axis W * sum of squares - sum^2) of a box, exact integers."""
    W = int(w.sum())
    s1 = [int((w * col[:, a]).sum()) for a in range(3)]
    s2 = [int((w * col[:, a] * col[:, a]).sum()) for a in range(3)]
    return W, s1, [W * s2[a] - s1[a] * s1[a] for a in range(3)]


def design_palette(hist):
    """32768 5-5-5 bin counts -> (palette uint8 (256, 3), lut uint8 (32768,)).

    A deterministic median cut over the occupied bins, each at its centre 8 v + 4 with its
    count as weight, in exact integer arithmetic: the box with the largest squared error is
    split, along its axis of largest weighted variance, at the weighted mean (lowest box /
    axis on ties), until there are 256 boxes or none can be split.  An entry is its box's
    rounded weighted mean; unused entries are black.  lut[bin] is the entry nearest to the
    bin's centre in squared RGB distance, the lowest index on ties."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    if hist.shape[0] != 32768 or (hist < 0).any() or not hist.any():
        raise ValueError("design_palette: 32768 non-negative counts, not all zero, expected")
    keys = np.nonzero(hist)[0]
    w_all = hist[keys]
    col_all = np.stack([(keys >> 10) & 31, (keys >> 5) & 31, keys & 31], axis=1).astype(np.int64) * 8 + 4
    boxes = []  # [bins (indices into keys), W, s1, var numerators, error]

    def add(bins):
        W, s1, num = _box_stats(w_all[bins], col_all[bins])
        boxes.append([bins, W, s1, num, sum(num) / W])

    add(np.arange(keys.shape[0]))
    while len(boxes) < 256:
        best = -1
        for i, b in enumerate(boxes):
            if b[4] > 0 and (best < 0 or b[4] > boxes[best][4]):
                best = i
        if best < 0:
            break
        bins, W, s1, num, _ = boxes.pop(best)
        axis = max(range(3), key=lambda a: (num[a], -a))
        low = col_all[bins, axis] * W <= s1[axis]  # centre <= weighted mean, exactly
        for part in (bins[low], bins[~low]):
            add(part)
    palette = np.zeros((256, 3), np.uint8)
    for i, (_, W, s1, _, _) in enumerate(boxes):
        palette[i] = [(2 * s + W) // (2 * W) for s in s1]
    centres = np.arange(32768)
    centres = (np.stack([(centres >> 10) & 31, (centres >> 5) & 31, centres & 31], axis=1) * 8 + 4).astype(np.int32)
    pal = palette.astype(np.int32)
    lut = np.empty(32768, np.uint8)
    for c0 in range(0, 32768, 4096):
        d = ((centres[c0:c0 + 4096, None, :] - pal[None, :len(boxes), :]) ** 2).sum(axis=2)
        lut[c0:c0 + 4096] = d.argmin(axis=1)  # the first minimum: the lowest index
    return palette, lut


# --------------------------------------------------------------------------- container


def write_gif(path, lzw_bytes, offsets, palette, width, height, delay_cs):
    """GIF89a with one global 256-entry colour table, a NETSCAPE2.0 loop-forever extension
    (what imageio's loop=0 writes) and, per frame, a graphic control extension (disposal 0,
    delay ``delay_cs`` centiseconds) and a full-frame image whose LZW data (minimum code
    size 8) is lzw_bytes[offsets[f]:offsets[f + 1]] cut into 255-byte sub-blocks.  Returns
    the number of bytes written."""
    palette = np.asarray(palette, dtype=np.uint8)
    if palette.shape != (256, 3):
        raise ValueError(f"write_gif: palette (256, 3) expected, got {palette.shape}")
    if not (1 <= width <= 65535 and 1 <= height <= 65535 and 0 <= delay_cs <= 65535):
        raise ValueError(f"write_gif: {width}x{height}, delay {delay_cs} outside the 16-bit fields")
    data = np.frombuffer(bytes(lzw_bytes), np.uint8) if isinstance(lzw_bytes, (bytes, bytearray, memoryview)) \
        else np.asarray(lzw_bytes, dtype=np.uint8)
    offsets = [int(o) for o in offsets]
    out = [b"GIF89a", struct.pack("<HHBBB", width, height, 0xF7, 0, 0), palette.tobytes(),
           b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00"]
    for f in range(len(offsets) - 1):
        out.append(b"\x21\xF9\x04" + struct.pack("<BHB", 0, delay_cs, 0) + b"\x00")
        out.append(b"\x2C" + struct.pack("<HHHHB", 0, 0, width, height, 0) + b"\x08")
        codes = data[offsets[f]:offsets[f + 1]]
        full, rest = divmod(codes.shape[0], 255)
        if full:
            blocks = np.empty((full, 256), np.uint8)
            blocks[:, 0] = 255
            blocks[:, 1:] = codes[:full * 255].reshape(full, 255)
            out.append(blocks.tobytes())
        if rest:
            out.append(bytes([rest]) + codes[full * 255:].tobytes())
        out.append(b"\x00")
    out.append(b"\x3B")
    blob = b"".join(out)
    with open(path, "wb") as f:
        f.write(blob)
    return len(blob)


# --------------------------------------------------------------------------- top level


def _encode(frames, path, delay_cs):
    from . import ops
    import torch
    hist = ops.rgb555_hist(frames)
    if frames.numel() // 3 < 2 ** 31:  # every count fits 32 bits: 128 KB cross to the host, not 256
        hist = hist.to(torch.int32)
    palette, lut = design_palette(hist.cpu().numpy())
    idx = ops.palette_map(frames, torch.from_numpy(lut).to(frames.device))
    data, offsets = ops.gif_lzw(idx)
    _, H, W, _ = frames.shape
    return write_gif(path, data.cpu().numpy(), offsets.cpu().tolist(), palette, W, H, delay_cs)


def create_video_thumbnail_gif(frames_dev_u8, video_fps, output_path, duration=3, fps=5,
                               subtitle_text=DEFAULT_SUBTITLE, max_width=640, max_size_mb=2, font=None):
    """The reference's create_video_thumbnail_gif on the result's frames: uint8 (N, H, W, 3) on
    the device, with ``video_fps`` standing for cv2's CAP_PROP_FPS.  The frames of
    select_frames (see there for the rule's oddity), area-resized to thumbnail_size, get the
    play button and the subtitle of overlay_layers and are written as a looping GIF with
    round(100 / fps) centiseconds per frame.  A file above ``max_size_mb`` MiB is redone
    once from the composited frames area-resized to int(h * 0.7) x int(w * 0.7).  Returns the
    number of bytes written."""
    import torch

    from . import ops
    if (not isinstance(frames_dev_u8, torch.Tensor) or frames_dev_u8.dtype != torch.uint8 or frames_dev_u8.dim() != 4
            or frames_dev_u8.shape[-1] != 3 or not frames_dev_u8.is_cuda):
        raise ValueError("create_video_thumbnail_gif: uint8 (N, H, W, 3) frames on the device expected")
    N, H, W, _ = frames_dev_u8.shape
    sel = select_frames(N, video_fps, duration, fps)
    w, h = thumbnail_size(W, H, max_width)
    if h < 1:
        raise ValueError(f"create_video_thumbnail_gif: {W}x{H} frames give a thumbnail of height {h}")
    layers = overlay_layers(w, h, subtitle_text, font)
    frames = frames_dev_u8[torch.tensor(sel, device=frames_dev_u8.device)].contiguous()
    if (w, h) != (W, H):
        frames = ops.resize_area_u8(frames, h, w)
    ops.overlay_blend_u8(frames, layers)
    delay_cs = int(round(100 / fps))
    size = _encode(frames, output_path, delay_cs)
    if size / (1024 * 1024) > max_size_mb and int(h * 0.7) >= 1 and int(w * 0.7) >= 1:
        size = _encode(ops.resize_area_u8(frames, int(h * 0.7), int(w * 0.7)), output_path, delay_cs)
    return size
