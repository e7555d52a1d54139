"""CPU restatement of the device Motion-JPEG encoder (csrc/ls_video.hip, DESIGN.md section
16): integer numpy arithmetic plus a plain Python bit writer.  It states the definition a
second time, independently of the kernels; tests/test_avi_mjpeg.py checks it against
Pillow, tests/test_gpu_mjpeg.py checks the device bytes against it.  Not a product path.

Only the tables and the header builder are shared with the package (latentsync_amd.video);
the tables are themselves checked against the DHT / DQT segments Pillow writes."""
import numpy as np

from latentsync_amd import video

ZZ = np.array(video.ZIGZAG)


def pad_to_mcu(rgb):
    """Replicate the last column / row up to a multiple of 16."""
    H, W, _ = rgb.shape
    return np.pad(rgb, ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge")


def replicate_last_chroma_row(c, H):
    """Rows below the subsampled plane's last one, (H - 1) // 2, replicate it: libjpeg pads
    the downsampled rows, so for an even H the padding averages rows H - 2 and H - 1."""
    c = c.copy()
    last = (H - 1) // 2
    c[last + 1:] = c[last]
    return c


def ycc_420(rgb):
    """uint8 (H, W, 3), H and W multiples of 16 -> Y (H, W), Cb, Cr (H/2, W/2) int64.
    libjpeg rgb_ycc_convert (16-bit fixed point) and h2v2_downsample (bias 1, 2, 1, 2, ...)."""
    R, G, B = (rgb[..., i].astype(np.int64) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16

    def down(c):
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        bias = 1 + (np.arange(s.shape[1]) & 1)
        return (s + bias[None, :]) >> 2
    return Y, down(Cb), down(Cr)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, second):
    """jpeg_fdct_islow, one pass along the last axis (CONST_BITS 13, PASS1_BITS 2)."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 15 if second else 11
    o = [None] * 8
    if second:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    else:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, sh)
    o[6] = _descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5] = _descale(t4 + z1 + z3, sh), _descale(t5 + z2 + z4, sh)
    o[3], o[1] = _descale(t6 + z2 + z3, sh), _descale(t7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def fdct_islow(blocks):
    """(..., 8, 8) samples minus 128 -> 8 x the DCT coefficients, natural order."""
    a = _fdct_pass(blocks.astype(np.int64), False)                    # rows
    return _fdct_pass(a.swapaxes(-1, -2), True).swapaxes(-1, -2)      # columns


def quantise(coef, q):
    """Round half away from zero of coef / (8 q); AC clamped to +-1023."""
    q8 = q.astype(np.int64).reshape(8, 8) << 3
    a = (np.abs(coef) + (q8 >> 1)) // q8
    dc = a[..., 0, 0].copy()
    a = np.minimum(a, 1023)
    a[..., 0, 0] = dc
    return np.where(coef < 0, -a, a)


def frame_coefficients(rgb, quality):
    """uint8 (H, W, 3) -> (MCUs in raster order, 6, 64) zigzag coefficients."""
    ql, qc = video.quant_tables(quality)
    Y, Cb, Cr = ycc_420(pad_to_mcu(rgb))
    Cb, Cr = replicate_last_chroma_row(Cb, rgb.shape[0]), replicate_last_chroma_row(Cr, rgb.shape[0])
    my, mx = Y.shape[0] // 16, Y.shape[1] // 16

    def blocks(p, per):  # (my, mx, per, per, 8, 8): MCU raster, then the block raster inside an MCU
        return p.reshape(my, per, 8, mx, per, 8).transpose(0, 3, 1, 4, 2, 5) - 128

    y = quantise(fdct_islow(blocks(Y, 2)), ql).reshape(my * mx, 4, 64)
    c = [quantise(fdct_islow(blocks(p, 1)), qc).reshape(my * mx, 1, 64) for p in (Cb, Cr)]
    return np.concatenate([y] + c, axis=1)[..., ZZ]


def huff_codes(spec):
    """(BITS, HUFFVAL) -> {symbol: (code, length)} (T.81 Annex C)."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC = [huff_codes(video.HUFF_DC_LUMA), huff_codes(video.HUFF_DC_CHROMA)]
AC = [huff_codes(video.HUFF_AC_LUMA), huff_codes(video.HUFF_AC_CHROMA)]


class BitWriter:
    """MSB-first bits; flush() pads the last byte with 1 bits and stuffs 0x00 after 0xFF."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length

    def flush(self):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        raw = self.acc.to_bytes(self.n // 8, "big")
        return raw.replace(b"\xff", b"\xff\x00")


def _magnitude(v):
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def encode_block(bw, zz, pred, tab):
    diff = int(np.clip(int(zz[0]) - pred, -2047, 2047))
    n, extra = _magnitude(diff)
    bw.put(*DC[tab][n])
    bw.put(extra, n)
    run = 0
    for v in zz[1:].tolist():
        if v == 0:
            run += 1
            continue
        while run >= 16:
            bw.put(*AC[tab][0xF0])
            run -= 16
        n, extra = _magnitude(v)
        bw.put(*AC[tab][run << 4 | n])
        bw.put(extra, n)
        run = 0
    if run:
        bw.put(*AC[tab][0x00])


def scan_from_coefficients(coefs, Ri):
    """(MCUs, 6, 64) zigzag coefficients -> the entropy-coded scan: every interval of Ri
    MCUs coded on its own (predictors 0), RSTm between intervals, none after the last."""
    out = []
    n_int = -(-len(coefs) // Ri)
    for k in range(n_int):
        bw, pred = BitWriter(), [0, 0, 0]
        for mcu in coefs[k * Ri:(k + 1) * Ri]:
            for b in range(6):
                comp = 0 if b < 4 else b - 3
                encode_block(bw, mcu[b], pred[comp], 0 if b < 4 else 1)
                pred[comp] = int(mcu[b][0])
        out.append(bw.flush())
        if k < n_int - 1:
            out.append(bytes([0xFF, 0xD0 + (k & 7)]))
    return b"".join(out)


def encode_scan(rgb, quality, Ri):
    return scan_from_coefficients(frame_coefficients(rgb, quality), Ri)


def encode_jpeg(rgb, quality, Ri):
    H, W, _ = rgb.shape
    return video.jpeg_headers(H, W, quality, Ri) + encode_scan(rgb, quality, Ri) + video.JPEG_EOI


def wrap_coefficients(coefs, H, W, quality, Ri):
    return video.jpeg_headers(H, W, quality, Ri) + scan_from_coefficients(coefs, Ri) + video.JPEG_EOI


# ------------------------------------------------------------------ shared test content

def smooth_frames(n, H, W, seed):
    """Low-resolution noise upsampled bicubically, as the __call__ tests build faces."""
    import torch
    low = torch.rand((n, 3, max(2, H // 8), max(2, W // 8)), generator=torch.Generator().manual_seed(seed))
    up = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    return (up * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()


def checker_frame(H, W):
    """8x8 black / white blocks: at quality 100 the luma DC jumps by 2040 (category 11)."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat((((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def last_coefficient_frame(H, W):
    """Grey frame whose every 8x8 block is 128 + 127 cos((2x+1) 7 pi / 16) cos((2y+1) 7 pi / 16):
    its DCT is 4 * 127 at (7, 7) and rounding noise elsewhere, so at quality 1 (every step
    255) a luma block holds only zigzag coefficient 63 -- three ZRLs and no EOB."""
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    tile = np.round(128 + 127 * np.outer(c, c)).astype(np.uint8)
    g = np.tile(tile, (-(-H // 8), -(-W // 8)))[:H, :W]
    return np.repeat(g[..., None], 3, axis=2)


def noise_frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
