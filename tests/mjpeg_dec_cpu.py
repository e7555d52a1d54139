"""CPU restatement of the device Motion-JPEG decoder (csrc/ls_video_dec.hip, DESIGN.md
section 4.3): integer numpy arithmetic plus a plain Python bit reader.  It states the
definition a second time, independently of the kernels; tests/test_mjpeg_decode_host.py
pins it to libjpeg (Pillow) bit for bit, tests/test_gpu_mjpeg_decode.py checks the device
pixels against it.  Not a product path.

Only the header parser is shared with the package (video.parse_jpeg); the Huffman decode
here walks the canonical codes length by length (T.81 F.2.2.3) instead of using the
device's derived lookahead tables, so those are checked too.

Rules it shares with the kernel: the k-th marker inside a scan must be RST(k mod 8) and
there must be ceil(MCUs / Ri) - 1 of them (status 2); 0xFF 0x00 is the byte 0xFF and an
0xFF followed by anything else ends a segment's data; bits past the end are zeros; a
code longer than 16 bits or a DC category above 15 (3), a coefficient index past 63 (4)
and, checked after every block, more bits consumed than the segment holds (5) stop the
frame."""
import functools

import numpy as np

from latentsync_amd import video

ZZ = np.array(video.ZIGZAG)
ST_MARKERS, ST_CODE, ST_INDEX, ST_SHORT = 2, 3, 4, 5


def _codes(spec):
    """(BITS, HUFFVAL) -> {(length, code): symbol} (T.81 Annex C)."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


class BitReader:
    """MSB-first bits of one restart segment: unstuffed, cut at the first 0xFF that is not
    followed by 0x00, zero bits past the end."""

    def __init__(self, seg):
        out, i, n = bytearray(), 0, len(seg)
        while i < n:
            b = seg[i]
            i += 1
            if b == 0xFF:
                if i < n and seg[i] == 0:
                    i += 1
                else:
                    break
            out.append(b)
        self.real = 8 * len(out)
        self.buf = bytes(out) + bytes(8)
        self.pos = 0

    def peek16(self):
        i, off = self.pos >> 3, self.pos & 7
        if i + 3 > len(self.buf):
            return 0
        return (((self.buf[i] << 16) | (self.buf[i + 1] << 8) | self.buf[i + 2]) >> (8 - off)) & 0xFFFF

    def take(self, n):
        v = self.peek16() >> (16 - n)
        self.pos += n
        return v

    def symbol(self, codes):
        w = self.peek16()
        for length in range(1, 17):
            s = codes.get((length, w >> (16 - length)))
            if s is not None:
                self.pos += length
                return s
        return -1

    def extend(self, s):
        v = self.take(s)
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def decode_block(br, dc, ac, pred, out):
    """One block into out[64] (natural order) -> (new predictor, status)."""
    s = br.symbol(dc)
    if s < 0 or s > 15:
        return pred, ST_CODE
    if s:
        pred += br.extend(s)
    out[0] = pred
    k = 1
    while k < 64:
        rs = br.symbol(ac)
        if rs < 0:
            return pred, ST_CODE
        r, s = rs >> 4, rs & 15
        if s:
            k += r
            if k > 63:
                return pred, ST_INDEX
            out[ZZ[k]] = br.extend(s)
        elif r != 15:
            break
        else:
            k += 15
        k += 1
    return pred, ST_SHORT if br.pos > br.real else 0


def split_segments(scan, n_seg):
    """The scan's restart segments, or None when the markers are not RST0, RST1, ... in
    order and n_seg - 1 in number."""
    cuts = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    if len(cuts) != n_seg - 1 or any(scan[c + 1] & 7 != k & 7 for k, c in enumerate(cuts)):
        return None
    starts, ends = [0] + [c + 2 for c in cuts], cuts + [len(scan)]
    return [scan[a:b] for a, b in zip(starts, ends)]


def _geometry(info):
    hs, vs = {0: (1, 1), 1: (1, 1), 2: (2, 1), 3: (2, 2)}[info.mode]
    mcux, mcuy = -(-info.W // (8 * hs)), -(-info.H // (8 * vs))
    return hs, vs, mcux, mcuy


def decode_coefficients(jpg, info):
    """-> (list of int64 (blocks down, blocks across, 64) per component, status)."""
    hs, vs, mcux, mcuy = _geometry(info)
    shape = [(mcuy * vs, mcux * hs)] + [(mcuy, mcux)] * (info.ncomp - 1)
    coef = [np.zeros((h, w, 64), np.int64) for h, w in shape]
    n_mcu = mcux * mcuy
    ri = info.Ri if 0 < info.Ri < n_mcu else n_mcu
    segs = split_segments(jpg[info.scan_start:], -(-n_mcu // ri))
    if segs is None:
        return coef, ST_MARKERS
    dc, ac = [_codes(t) for t in info.huff_dc], [_codes(t) for t in info.huff_ac]
    status = 0
    for k, seg in enumerate(segs):
        br, pred = BitReader(seg), [0] * info.ncomp
        st = 0
        for m in range(k * ri, min((k + 1) * ri, n_mcu)):
            my, mx = divmod(m, mcux)
            for c in range(info.ncomp):
                nh, nv = (hs, vs) if c == 0 else (1, 1)
                for b in range(nh * nv):
                    pred[c], st = decode_block(br, dc[c], ac[c], pred[c], coef[c][my * nv + b // nh, mx * nh + b % nh])
                    if st:
                        break
                if st:
                    break
            if st:
                break
        status = max(status, st)
    return coef, status


def _idct_pass(d, shift):
    """jpeg_idct_islow, one pass along the last axis (CONST_BITS 13, PASS1_BITS 2)."""
    d = [d[..., i] for i in range(8)]
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(v + (1 << (shift - 1))) >> shift for v in o], axis=-1)


def idct_plane(coef, q):
    """(bh, bw, 64) coefficients x 64 quantiser steps (natural order) -> uint8-range plane."""
    bh, bw, _ = coef.shape
    blk = (coef * np.asarray(q, np.int64)).reshape(bh, bw, 8, 8)
    cols = _idct_pass(blk.swapaxes(-1, -2), 11).swapaxes(-1, -2)  # the column pass runs first
    px = np.clip(_idct_pass(cols, 18) + 128, 0, 255)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(p, W):
    """jdsample.c h2v1_fancy_upsample over the ceil(W / 2) real columns."""
    dw = (W + 1) // 2
    p = p[:, :dw]
    left, right = np.roll(p, 1, axis=1), np.roll(p, -1, axis=1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    return np.stack([even, odd], axis=-1).reshape(p.shape[0], 2 * dw)[:, :W]


def upsample_h2v2(p, H, W):
    """jdsample.c h2v2_fancy_upsample over the ceil(H / 2) x ceil(W / 2) real samples."""
    dh, dw = (H + 1) // 2, (W + 1) // 2
    p = p[:dh, :dw]
    up, down = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    rows = np.stack([3 * p + up, 3 * p + down], axis=1).reshape(2 * dh, dw)
    left, right = np.roll(rows, 1, axis=1), np.roll(rows, -1, axis=1)
    even, odd = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * rows[:, 0] + 8) >> 4, (4 * rows[:, -1] + 7) >> 4
    return np.stack([even, odd], axis=-1).reshape(2 * dh, 2 * dw)[:H, :W]


def decode_status(jpg):
    """One JPEG byte string -> (uint8 (H, W, 3) RGB, status).  The pixels mean nothing when
    the status is not 0."""
    jpg = bytes(jpg)
    info = video.parse_jpeg(jpg)
    assert info.on_device, info.reason
    coef, status = decode_coefficients(jpg, info)
    H, W = info.H, info.W
    planes = [idct_plane(c, q) for c, q in zip(coef, info.quant)]
    y = planes[0][:H, :W]
    if info.ncomp == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8), status
    if info.mode == 1:
        cb, cr = (p[:H, :W] for p in planes[1:])
    elif W <= 4:  # jdsample.c: a chroma plane of 1 or 2 columns is replicated, not filtered
        cb, cr = (np.repeat(np.repeat(p, 2 if info.mode == 3 else 1, axis=0), 2, axis=1)[:H, :W] for p in planes[1:])
    elif info.mode == 2:
        cb, cr = (upsample_h2v1(p[:H], W) for p in planes[1:])
    else:
        cb, cr = (upsample_h2v2(p, H, W) for p in planes[1:])
    cb, cr = cb - 128, cr - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8), status


@functools.lru_cache(maxsize=None)
def decode(jpg):
    """One good JPEG byte string -> uint8 (H, W, 3) RGB, cached: this is slow Python.  The
    result is shared between tests: do not write to it."""
    rgb, status = decode_status(jpg)
    assert status == 0, status
    rgb.setflags(write=False)
    return rgb
