"""CPU restatement of the device side of the GIF thumbnail (csrc/ls_thumb.hip, DESIGN.md
section 4.6): numpy arithmetic and plain Python, written from the definitions in
include/ls_hip.h.  tests/test_thumbnail_host.py checks it against Pillow,
tests/test_gpu_thumbnail.py checks the device against it, value for value and byte for
byte.  Not a product path.

It also holds an independent GIF parser and LZW decoder (parse_gif), so the GPU tests need
no Pillow to read what the package writes."""
import numpy as np

STRIP_ROWS = 8
DBL_EPSILON = 2.220446049250313e-16


# ------------------------------------------------------------------ INTER_AREA


def area_tab(ssize, dsize, scale):
    """OpenCV's computeResizeAreaTab for one axis: [(dst index, src index, fp32 weight)] in
    its order -- per destination index the partial cell on the left, the full cells, the
    partial cell on the right."""
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cw = min(scale, ssize - f1)
        s1, s2 = int(np.ceil(f1)), int(np.floor(f2))
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        clamp = lambda s: min(max(s, 0), ssize - 1)
        if s1 - f1 > 1e-3:
            tab.append((d, clamp(s1 - 1), np.float32((s1 - f1) / cw)))
        for s in range(s1, s2):
            tab.append((d, clamp(s), np.float32(1.0 / cw)))
        if f2 - s2 > 1e-3:
            tab.append((d, clamp(s2), np.float32(min(min(f2 - s2, 1.0), cw) / cw)))
    return tab


def _ranked(tab, dsize):
    """The table by rank: [(dst indices, src indices, weights)] -- entry k of every
    destination index that has k + 1 entries or more."""
    per = [[] for _ in range(dsize)]
    for d, s, a in tab:
        per[d].append((s, a))
    out = []
    for k in range(max(len(p) for p in per)):
        ds = [d for d in range(dsize) if len(per[d]) > k]
        out.append((np.array(ds), np.array([per[d][k][0] for d in ds]),
                    np.array([per[d][k][1] for d in ds], dtype=np.float32)))
    return out


def resize_area(frames, dh, dw):
    """cv2.resize(frame, (dw, dh), interpolation=INTER_AREA) of uint8 (n, H, W, 3), downscale
    only: fp32, one rounding per operation, in OpenCV's order."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    assert dh <= H and dw <= W
    sx, sy = 1.0 / (dw / W), 1.0 / (dh / H)
    ix, iy = int(np.rint(sx)), int(np.rint(sy))
    if abs(sx - ix) < DBL_EPSILON and abs(sy - iy) < DBL_EPSILON:
        s = frames.astype(np.int32).reshape(n, dh, iy, dw, ix, 3).sum(axis=(2, 4))
        if ix == 2 and iy == 2:
            return ((s + 2) >> 2).astype(np.uint8)
        v = s.astype(np.float32) * (np.float32(1.0) / np.float32(ix * iy))
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    src = frames.astype(np.float32)
    buf = np.zeros((n, H, dw, 3), np.float32)
    for ds, ss, al in _ranked(area_tab(W, dw, sx), dw):
        buf[:, :, ds] = buf[:, :, ds] + src[:, :, ss] * al[None, None, :, None]
    out = np.zeros((n, dh, dw, 3), np.float32)
    for k, (ds, ss, be) in enumerate(_ranked(area_tab(H, dh, sy), dh)):
        term = be[None, :, None, None] * buf[:, ss]
        out[:, ds] = term if k == 0 else out[:, ds] + term
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ overlay, palette


def composite(frames, layers):
    """Blend the layers (x0, y0, alpha (h, w), (r, g, b)) in order into a copy of uint8
    (..., H, W, 3): t = ink a + dst (255 - a) + 128; dst = ((t >> 8) + t) >> 8."""
    out = np.array(frames, dtype=np.int64)
    H, W = out.shape[-3:-1]
    for x0, y0, alpha, ink in layers:
        alpha = np.asarray(alpha, dtype=np.int64)
        h, w = alpha.shape
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
        if ya >= yb or xa >= xb:
            continue
        a = alpha[ya - y0:yb - y0, xa - x0:xb - x0, None]
        dst = out[..., ya:yb, xa:xb, :]
        t = np.array(ink, dtype=np.int64) * a + dst * (255 - a) + 128
        out[..., ya:yb, xa:xb, :] = ((t >> 8) + t) >> 8
    return out.astype(np.uint8)


def keys555(frames):
    f = np.asarray(frames).astype(np.int64) >> 3
    return (f[..., 0] << 10) | (f[..., 1] << 5) | f[..., 2]


def hist555(frames):
    return np.bincount(keys555(frames).reshape(-1), minlength=32768)


def map_palette(frames, lut):
    return np.asarray(lut, dtype=np.uint8)[keys555(frames)]


# ------------------------------------------------------------------ LZW


class _Bits:
    """LSB-first bit writer."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, width):
        self.acc |= code << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def finish(self):
        """Pad to a whole byte with zeros."""
        if self.n:
            self.out.append(self.acc & 255)
        self.acc, self.n = 0, 0
        return bytes(self.out)


def lzw_strip(pixels, first, last, bits):
    """One strip (a flat sequence of indices) appended to `bits`: see ls_gif_lzw."""
    if first:
        bits.put(256, 9)
    table, width, nxt = {}, 9, 258
    prefix = int(pixels[0])
    for c in pixels[1:]:
        c = int(c)
        hit = table.get((prefix, c))
        if hit is not None:
            prefix = hit
            continue
        bits.put(prefix, width)
        code, nxt = nxt, nxt + 1
        if code == 4095:  # the dictionary is full: CLEAR at width 12, start over
            bits.put(256, width)
            table, width, nxt = {}, 9, 258
        else:
            table[(prefix, c)] = code
            if code == 1 << width:
                width += 1
        prefix = c
    bits.put(prefix, width)
    if nxt == 1 << width and width < 12:  # the bump a decoder makes after this last code
        width += 1
    bits.put(257 if last else 256, width)


def lzw_strips(idx, rows=STRIP_ROWS):
    """uint8 (n, H, W) indices -> (bytes, offsets): ls_gif_lzw's output."""
    idx = np.asarray(idx, dtype=np.uint8)
    n, H, W = idx.shape
    out, offsets = bytearray(), [0]
    for f in range(n):
        bits = _Bits()
        starts = list(range(0, H, rows))
        for r0 in starts:
            lzw_strip(idx[f, r0:r0 + rows].reshape(-1).tolist(), r0 == 0, r0 == starts[-1], bits)
        out += bits.finish()
        offsets.append(len(out))
    return bytes(out), offsets


def lzw_decode(data, min_size=8):
    """An ordinary GIF LZW decoder -> (indices as bytes, number of CLEAR codes read)."""
    clear, eoi = 1 << min_size, (1 << min_size) + 1
    acc, have, at = 0, 0, 0  # bits not yet consumed, their number, the next byte
    table = [bytes([i]) for i in range(clear)] + [b"", b""]
    width, prev, clears = min_size + 1, None, 0
    out = bytearray()
    while True:
        while have < width:
            assert at < len(data), "LZW data ends without EOI"
            acc |= data[at] << have
            have, at = have + 8, at + 1
        code = acc & ((1 << width) - 1)
        acc >>= width
        have -= width
        if code == clear:
            del table[eoi + 1:]
            width, prev, clears = min_size + 1, None, clears + 1
            continue
        if code == eoi:
            break
        if prev is None:
            assert code < clear, "first code after CLEAR is not a literal"
            entry = table[code]
        else:
            assert code <= len(table), f"code {code} beyond the table ({len(table)})"
            entry = table[code] if code < len(table) else table[prev] + table[prev][:1]
            if len(table) < 4096:
                table.append(table[prev] + entry[:1])
                if len(table) == 1 << width and width < 12:
                    width += 1
        out += entry
        prev = code
    assert at == len(data) and acc == 0, "data left after EOI"
    return bytes(out), clears


def parse_gif(blob):
    """-> dict(width, height, palette (k, 3) or None, loop (None: no NETSCAPE2.0 block),
    frames=[dict(delay, disposal, box, idx (h, w) uint8, clears)])."""
    assert blob[:6] == b"GIF89a"
    W, H, packed = int.from_bytes(blob[6:8], "little"), int.from_bytes(blob[8:10], "little"), blob[10]
    pos, palette = 13, None
    if packed & 0x80:
        k = 2 << (packed & 7)
        palette = np.frombuffer(blob[pos:pos + 3 * k], np.uint8).reshape(k, 3)
        pos += 3 * k

    def sub_blocks(p):
        data = bytearray()
        while blob[p]:
            data += blob[p + 1:p + 1 + blob[p]]
            p += 1 + blob[p]
        return bytes(data), p + 1

    g = dict(width=W, height=H, palette=palette, loop=None, frames=[])
    delay = disposal = None
    while True:
        b = blob[pos]
        if b == 0x3B:
            assert pos == len(blob) - 1, "bytes after the trailer"
            return g
        if b == 0x21:
            label = blob[pos + 1]
            data, end = sub_blocks(pos + 2)
            if label == 0xF9:
                assert blob[pos + 2] == 4
                disposal, delay = (data[0] >> 2) & 7, int.from_bytes(data[1:3], "little")
            elif label == 0xFF and data[:11] == b"NETSCAPE2.0" and data[11] == 1:
                g["loop"] = int.from_bytes(data[12:14], "little")
            pos = end
            continue
        assert b == 0x2C, f"unexpected block {b:#x} at {pos}"
        x, y, w, h = (int.from_bytes(blob[pos + 1 + 2 * i:pos + 3 + 2 * i], "little") for i in range(4))
        assert blob[pos + 9] == 0, "local colour table / interlace not expected"
        min_size = blob[pos + 10]
        data, pos = sub_blocks(pos + 11)
        px, clears = lzw_decode(data, min_size)
        assert len(px) == w * h, f"{len(px)} pixels decoded for a {w}x{h} image"
        g["frames"].append(dict(delay=delay, disposal=disposal, box=(x, y, w, h),
                                idx=np.frombuffer(px, np.uint8).reshape(h, w), clears=clears))


# ------------------------------------------------------------------ shared test content


def index_contents(H, W):
    """Index frames (H, W): noise (nothing repeats: the longest stream), one flat colour (the
    shortest) and a gradient."""
    yy, xx = np.mgrid[0:H, 0:W]
    return {"noise": np.random.default_rng(H * W).integers(0, 256, (H, W), dtype=np.uint8),
            "flat": np.full((H, W), 7, np.uint8),
            "gradient": ((xx * 255) // max(W - 1, 1) + yy).astype(np.uint8)}


def distinct_palette():
    """256 different colours, so equal RGB means equal index."""
    p = np.random.default_rng(1).permutation(1 << 24)[:256]
    return np.stack([p >> 16, (p >> 8) & 255, p & 255], axis=1).astype(np.uint8)
