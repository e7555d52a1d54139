"""Video files: Motion-JPEG in an AVI 1.0 container with 16-bit PCM audio (host side).

The writer is the job ffmpeg does for the reference's write_video (util.py:140-160) and
its audio mux (lipsync_pipeline.py:596-603), for the one format that needs no third-party
codec.  The frames are compressed where they already are: ops.mjpeg_encode (ls_mjpeg_encode,
csrc/ls_video.hip) returns every frame's entropy-coded scan, ``jpeg_headers`` builds the
segments in front of it on the host, and ``write_avi`` muxes complete JPEG byte strings
with the audio.  The way back in for ``read_video_frames`` is ``read_avi_device``: the host
reads each MJPG frame's headers (``parse_jpeg``), the device decodes the scans
(ops.mjpeg_decode, ls_mjpeg_decode, csrc/ls_video_dec.hip), so only compressed bytes are
uploaded; uncompressed 24-bit BI_RGB frames are uploaded as stored.  ``read_avi`` is the same
reader with the frames decoded on the host (MJPG with Pillow), for CPU-only hosts and for
JPEG flavours outside the device subset.  H.264 / mp4, OpenDML files above 2 GiB and
frame-rate conversion are out of scope.
"""
import io
import struct
from fractions import Fraction

import numpy as np

AVI_MAX_BYTES = 2 ** 31 - 1  # AVI 1.0: one RIFF chunk, signed 32-bit offsets in common readers

# ---------------------------------------------------------------------------- JPEG tables
# ITU-T T.81 Annex K.1 (natural order), K.3 (BITS, HUFFVAL); the device holds the same.
QBASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
              14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
QBASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# zigzag position -> natural index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
          14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
          53, 60, 61, 54, 47, 55, 62, 63)
HUFF_DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
HUFF_DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
HUFF_AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
HUFF_AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))


def quant_tables(quality):
    """(luma, chroma) quantisation steps in natural order, int (64,) each: the Annex K
    tables scaled by the libjpeg quality rule (jpeg_quality_scaling, jpeg_add_quant_table)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality must be in 1..100, got {quality}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(b, np.int64) * scale + 50) // 100, 1, 255) for b in (QBASE_LUMA, QBASE_CHROMA))


def _seg(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_headers(H, W, quality, Ri):
    """Every segment in front of a frame's scan: SOI, APP0 (JFIF 1.01), DQT x 2, SOF0
    (8-bit, Y 2x2 / Cb 1x1 / Cr 1x1), DHT x 4 (Annex K), DRI (``Ri`` MCUs), SOS.  A frame
    is jpeg_headers(...) + scan + EOI."""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"JPEG frame size {W}x{H} outside 1..65535")
    if not 1 <= Ri <= 65535:
        raise ValueError(f"restart interval {Ri} outside 1..65535")
    ql, qc = quant_tables(quality)
    out = [b"\xff\xd8", _seg(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for tq, t in ((0, ql), (1, qc)):
        out.append(_seg(0xDB, bytes([tq]) + bytes(int(t[z]) for z in ZIGZAG)))
    out.append(_seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, (bits, vals) in ((0x00, HUFF_DC_LUMA), (0x10, HUFF_AC_LUMA), (0x01, HUFF_DC_CHROMA),
                                (0x11, HUFF_AC_CHROMA)):
        out.append(_seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(_seg(0xDD, struct.pack(">H", Ri)))
    out.append(_seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


JPEG_EOI = b"\xff\xd9"


def restart_interval():
    """MCUs per restart interval of the device encoder (the DRI value of its streams)."""
    from . import _lib
    return int(_lib.load().ls_mjpeg_restart_interval())


def encode_frames(frames_dev_u8, quality=95):
    """Device uint8 (n, H, W, 3) RGB frames -> list of n complete JPEG byte strings.  Only
    the compressed bytes and the offsets are copied to the host."""
    from . import ops
    n, H, W, _ = frames_dev_u8.shape
    data, offsets = ops.mjpeg_encode(frames_dev_u8, quality)
    head = jpeg_headers(H, W, quality, restart_interval())
    off = offsets.cpu().tolist()
    raw = data.cpu().numpy().tobytes()
    return [head + raw[off[i]:off[i + 1]] + JPEG_EOI for i in range(n)]


# ---------------------------------------------------------------------------- JPEG reader

SAMPLING_MODES = {(1, 1): 1, (2, 1): 2, (2, 2): 3}  # luma (h, v) with chroma 1x1 -> the device's sampling mode
MODE_NAMES = ("grey", "4:4:4", "4:2:2", "4:2:0")
_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)",
              0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding (SOF10)", 0xCB: "arithmetic coding (SOF11)"}
_STD_HUFF = {(0, 0): HUFF_DC_LUMA, (0, 1): HUFF_DC_CHROMA, (1, 0): HUFF_AC_LUMA, (1, 1): HUFF_AC_CHROMA}


class JpegInfo:
    """What ``parse_jpeg`` found in front of a frame's scan.  ``reason`` is None when the
    frame is in the device subset (ls_mjpeg_decode), else why it is not; the geometry and
    table fields are complete only in the first case.
      H, W, ncomp; mode (index into MODE_NAMES); Ri (MCUs per restart interval, 0 = none);
      quant[c]: 64 quantiser steps of component c in natural order;
      huff_dc[c], huff_ac[c]: (BITS, HUFFVAL) of component c;
      scan_start: index in the byte string of the first entropy-coded byte (the scan runs
      to the end of the string); n_mcu, n_segments."""

    def __init__(self):
        self.H = self.W = self.ncomp = self.mode = self.Ri = self.scan_start = self.n_mcu = self.n_segments = 0
        self.quant, self.huff_dc, self.huff_ac, self.reason = [], [], [], None

    @property
    def on_device(self):
        return self.reason is None


def parse_jpeg(jpg):
    """Read the segments in front of the scan of one JPEG byte string -> JpegInfo.  SOI,
    APPn / COM (skipped; an Adobe APP14 is read for its transform), DQT, SOF, DHT, DRI and
    SOS are handled.  A frame without DHT gets the Annex K tables, the MJPG-in-AVI
    convention.  Anything outside the device subset -- 8-bit baseline (SOF0), one scan with
    Ss = 0, Se = 63, Ah = Al = 0, W and H >= 3, one component or Y 1x1 / 2x1 / 2x2 with Cb
    and Cr 1x1 -- sets ``reason``; a truncated or malformed header is a ValueError."""
    jpg = bytes(jpg)
    info = JpegInfo()
    n = len(jpg)
    if n < 4 or jpg[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG: no SOI marker")
    qt, q16, huff, comps, reasons = {}, set(), {}, None, []
    adobe = None
    i = 2
    while True:
        if i + 2 > n:
            raise ValueError(f"truncated JPEG header: no SOS marker in {n} bytes")
        if jpg[i] != 0xFF:
            raise ValueError(f"malformed JPEG header: byte 0x{jpg[i]:02X} at {i} where a marker is expected")
        m = jpg[i + 1]
        if m == 0xFF:  # fill byte
            i += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:  # stand-alone markers
            i += 2
            continue
        if m == 0xD9:
            raise ValueError("malformed JPEG: EOI before any scan")
        if i + 4 > n:
            raise ValueError(f"truncated JPEG header: marker 0x{m:02X} at byte {i} has no length")
        ln = struct.unpack(">H", jpg[i + 2:i + 4])[0]
        if ln < 2 or i + 2 + ln > n:
            raise ValueError(f"truncated JPEG header: segment 0x{m:02X} at byte {i} declares {ln} bytes, "
                             f"{n - i - 2} are left")
        p = jpg[i + 4:i + 2 + ln]
        if m == 0xDB:
            k = 0
            while k < len(p):
                pq, tq = p[k] >> 4, p[k] & 15
                size = 128 if pq else 64
                if pq > 1 or k + 1 + size > len(p):
                    raise ValueError("malformed JPEG: bad DQT segment")
                if pq:
                    q16.add(tq)
                    zz = struct.unpack(">64H", p[k + 1:k + 129])
                else:
                    q16.discard(tq)
                    zz = p[k + 1:k + 65]
                nat = [0] * 64
                for z, v in enumerate(zz):
                    nat[ZIGZAG[z]] = int(v)
                qt[tq] = tuple(nat)
                k += 1 + size
        elif m == 0xC4:
            k = 0
            while k < len(p):
                if k + 17 > len(p):
                    raise ValueError("malformed JPEG: bad DHT segment")
                tc, th = p[k] >> 4, p[k] & 15
                bits = tuple(p[k + 1:k + 17])
                cnt = sum(bits)
                if tc > 1 or cnt > 256 or k + 17 + cnt > len(p):
                    raise ValueError("malformed JPEG: bad DHT segment")
                huff[(tc, th)] = (bits, tuple(p[k + 17:k + 17 + cnt]))
                k += 17 + cnt
        elif m == 0xCC:
            reasons.append("arithmetic coding (DAC)")
        elif 0xC0 <= m <= 0xCF and m != 0xC8:
            if comps is not None:
                raise ValueError("malformed JPEG: two SOF segments")
            if len(p) < 6 or len(p) < 6 + 3 * p[5]:
                raise ValueError("truncated JPEG header: short SOF segment")
            if m != 0xC0:
                reasons.append(_SOF_NAMES.get(m, f"SOF{m - 0xC0}"))
            prec, info.H, info.W, info.ncomp = struct.unpack(">BHHB", p[:6])
            if prec != 8:
                reasons.append(f"{prec}-bit samples")
            comps = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(info.ncomp)]
        elif m == 0xDD:
            if len(p) < 2:
                raise ValueError("truncated JPEG header: short DRI segment")
            info.Ri = struct.unpack(">H", p[:2])[0]
        elif m == 0xEE and p[:5] == b"Adobe" and len(p) >= 12:
            adobe = p[11]
        elif m == 0xDA:
            if comps is None:
                raise ValueError("malformed JPEG: SOS before SOF")
            if len(p) < 1 or len(p) < 4 + 2 * p[0]:
                raise ValueError("truncated JPEG header: short SOS segment")
            ns = p[0]
            scan = [(p[1 + 2 * c], p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(ns)]
            ss, se, ahal = p[1 + 2 * ns:4 + 2 * ns]
            info.scan_start = i + 2 + ln
            break
        i += 2 + ln
    if info.ncomp not in (1, 3):
        reasons.append(f"{info.ncomp} components")
    if ns != info.ncomp or [s[0] for s in scan] != [c[0] for c in comps]:
        reasons.append("more than one scan")
    elif (ss, se, ahal) != (0, 63, 0):
        reasons.append(f"scan parameters Ss = {ss}, Se = {se}, Ah/Al = 0x{ahal:02X}")
    if info.H < 3 or info.W < 3:
        reasons.append(f"{info.W}x{info.H} is smaller than 3x3")
    if info.ncomp == 3:
        if adobe == 0 or (adobe is None and [c[0] for c in comps] == [82, 71, 66]):
            reasons.append("RGB components (Adobe transform 0)")
        fac = [(c[1], c[2]) for c in comps]
        if fac[1] != (1, 1) or fac[2] != (1, 1) or fac[0] not in SAMPLING_MODES:
            reasons.append("sampling factors " + ", ".join(f"{h}x{v}" for h, v in fac))
        else:
            info.mode = SAMPLING_MODES[fac[0]]
    if any(c[3] in q16 for c in comps):
        reasons.append("16-bit quantisation tables")
    if reasons:
        info.reason = "; ".join(reasons)
        return info
    for (_, _, _, tq), (_, td, ta) in zip(comps, scan):
        if tq not in qt:
            raise ValueError(f"malformed JPEG: quantisation table {tq} is not defined")
        info.quant.append(qt[tq])
        for tc, th, dst in ((0, td, info.huff_dc), (1, ta, info.huff_ac)):
            tab = huff.get((tc, th)) if huff else _STD_HUFF.get((tc, th))
            if tab is None:
                raise ValueError(f"malformed JPEG: Huffman table {'DA'[tc]}C {th} is not defined")
            if tc == 0 and any(v > 15 for v in tab[1]):
                raise ValueError("malformed JPEG: a DC Huffman table holds a category above 15")
            dst.append(tab)
    hs, vs = (1, 1) if info.mode == 0 else next(k for k, v in SAMPLING_MODES.items() if v == info.mode)
    info.n_mcu = -(-info.W // (8 * hs)) * -(-info.H // (8 * vs))
    info.n_segments = -(-info.n_mcu // info.Ri) if 0 < info.Ri < info.n_mcu else 1
    return info


HUFF_TABLE_INTS = 228  # int32 per device Huffman table (include/ls_hip.h)


def huff_device_table(bits, vals):
    """(BITS, HUFFVAL) -> int32 (228,), jdhuff.c's derived table (jpeg_make_d_derived_tbl):
    uint16 [256] lookahead, length << 8 | symbol for every code of up to 8 bits; int32 [18]
    maxcode by length (-1 = no code of that length, [17] a sentinel); int32 [18] valoffset;
    uint8 [256] HUFFVAL."""
    sizes = np.repeat(np.arange(1, 17), bits)
    if len(sizes) != len(vals) or len(sizes) > 256:
        raise ValueError("malformed JPEG: Huffman table counts and values disagree")
    codes = np.zeros(len(sizes), np.int64)
    code = 0
    for k in range(len(sizes)):
        if k and sizes[k] != sizes[k - 1]:
            code <<= int(sizes[k] - sizes[k - 1])
        if code >= 1 << int(sizes[k]):
            raise ValueError("malformed JPEG: Huffman table has more codes than its lengths allow")
        codes[k] = code
        code += 1
    look = np.zeros(256, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    maxcode[17] = 0xFFFFF
    p = 0
    for l in range(1, 17):
        if bits[l - 1]:
            valoff[l] = p - codes[p]
            p += bits[l - 1]
            maxcode[l] = codes[p - 1]
    for k in np.nonzero(sizes <= 8)[0]:
        l = int(sizes[k])
        first = int(codes[k]) << (8 - l)
        look[first:first + (1 << (8 - l))] = (l << 8) | int(vals[k])
    val = np.zeros(256, np.uint8)
    val[:len(vals)] = vals
    return np.concatenate([look.view(np.int32), maxcode, valoff, val.view(np.int32)])


_STATUS_TEXT = {1: "the scan lies outside the buffer", 2: "restart markers missing, surplus or out of order",
                3: "a Huffman code longer than 16 bits", 4: "a coefficient index past 63",
                5: "the entropy-coded data ends before the last MCU"}


def pack_frames(jpegs):
    """The host half of ``decode_frames``: n JPEG byte strings (or (bytes, JpegInfo) pairs)
    of one size -> (scans bytes, descriptors int64 (n, 8), quantisers int16 (n_quant, 64),
    Huffman tables int32 (n_huff, 228), max segments per frame, H, W), the arguments of
    ops.mjpeg_decode in the layouts of include/ls_hip.h.  The scans are concatenated and
    the tables deduplicated: most files repeat one set, files with optimised tables
    carry one per frame."""
    infos = [j if isinstance(j, tuple) else (bytes(j), parse_jpeg(j)) for j in jpegs]
    if not infos:
        raise ValueError("decode_frames: no frames")
    H, W = infos[0][1].H, infos[0][1].W
    qidx, hidx, desc, scans, pos = {}, {}, [], [], 0
    pack = lambda idx: sum(v << (16 * c) for c, v in enumerate(idx))
    for i, (jpg, info) in enumerate(infos):
        if not info.on_device:
            raise ValueError(f"frame {i} is not in the device subset of JPEG ({info.reason})")
        if (info.H, info.W) != (H, W):
            raise ValueError(f"frame {i} is {info.W}x{info.H}, frame 0 is {W}x{H}")
        q = [qidx.setdefault(t, len(qidx)) for t in info.quant]
        dc = [hidx.setdefault(t, len(hidx)) for t in info.huff_dc]
        ac = [hidx.setdefault(t, len(hidx)) for t in info.huff_ac]
        scan = jpg[info.scan_start:]
        desc.append((pos, len(scan), info.Ri, info.mode, pack(q), pack(dc), pack(ac), 0))
        scans.append(scan)
        pos += len(scan)
    if len(qidx) > 65535 or len(hidx) > 65535:
        raise ValueError("decode_frames: more than 65535 distinct tables in one call")
    quant = np.array(list(qidx), np.int16)  # steps are 1..255
    huff = np.stack([huff_device_table(*t) for t in hidx])
    return (b"".join(scans), np.array(desc, np.int64), quant, huff, max(info.n_segments for _, info in infos), H, W)


def decode_frames_status(jpegs, device):
    """``decode_frames`` without the final check: -> (frames uint8 (n, H, W, 3) on the
    device, status list of n ints).  Frames with a non-zero status are undefined, the
    others exact."""
    import torch
    from . import ops
    scans, desc, quant, huff, max_seg, H, W = pack_frames(jpegs)
    if not torch.cuda.is_available():
        raise RuntimeError("decode_frames: the Motion-JPEG decoder runs on the HIP device, and none is present "
                           "(read_avi decodes on the host)")
    device = torch.device(device)
    up = lambda a: torch.from_numpy(a).to(device)
    data = up(np.frombuffer(scans or b"\0", np.uint8).copy())
    frames, status = ops.mjpeg_decode(data, up(desc), H, W, up(quant), up(huff), max_seg)
    return frames, status.cpu().tolist()


def decode_frames(jpegs, device):
    """n complete JPEG byte strings of one size -> uint8 (n, H, W, 3) RGB on ``device``
    (ls_mjpeg_decode).  The host reads the headers, deduplicates the quantisers and the
    Huffman tables and uploads the concatenated scans; everything else runs on the device.
    A frame outside the device subset or one the device could not decode is a ValueError
    naming it."""
    frames, status = decode_frames_status(jpegs, device)
    for i, s in enumerate(status):
        if s:
            raise ValueError(f"frame {i} is not a decodable JPEG ({_STATUS_TEXT.get(s, f'status {s}')})")
    return frames


# ---------------------------------------------------------------------------- AVI writer

def audio_to_s16(audio):
    """float samples -> int16 as round(clip(x, -1, 1) * 32767)."""
    a = np.asarray(audio, dtype=np.float64).reshape(-1)
    return np.round(np.clip(a, -1.0, 1.0) * 32767.0).astype("<i2")


def trim_counts(n_frames, fps, n_audio, sample_rate, padding_duration, keep_all):
    """(frames kept, audio samples kept) of the written clip.  The reference's trim
    (lipsync_pipeline.py:599-602) cuts the muxed file at T = n / fps - padding_duration
    unless start_from_backwards or force_video_length is set (``keep_all``): frames with
    i / fps < T and samples with j / sample_rate < T stay.  With ``keep_all`` every frame
    stays and the audio is cut to int(n / fps * sample_rate).  T is formed in rationals:
    fps and padding_duration (k / fps as a float) are taken to the nearest fraction with a
    denominator up to 10^6, so float dust cannot move a frame across the cut (the
    reference's awk prints T with 6 significant digits)."""
    n_frames, n_audio = int(n_frames), int(n_audio)
    if keep_all:
        return n_frames, min(n_audio, int(n_frames / fps * sample_rate))
    fps = Fraction(fps).limit_denominator(10 ** 6)
    T = Fraction(n_frames) / fps - Fraction(padding_duration).limit_denominator(10 ** 6)
    if T <= 0:
        return 0, 0
    ceil = lambda x: -((-x.numerator) // x.denominator)  # i < T * fps  <=>  i <= ceil(T * fps) - 1
    return min(n_frames, ceil(T * Fraction(fps))), min(n_audio, ceil(T * sample_rate))


def _fps_ratio(fps):
    fr = Fraction(fps).limit_denominator(100000)
    if fr <= 0:
        raise ValueError(f"fps must be positive, got {fps}")
    return fr.numerator, fr.denominator  # dwRate, dwScale


def _jpeg_size(jpg):
    """(H, W) from the first SOF0..SOF2 segment of a JPEG byte string."""
    if jpg[:2] != b"\xff\xd8":
        raise ValueError("write_avi: a frame does not start with the JPEG SOI marker")
    i = 2
    while i + 4 <= len(jpg):
        if jpg[i] != 0xFF:
            break
        m, ln = jpg[i + 1], struct.unpack(">H", jpg[i + 2:i + 4])[0]
        if m in (0xC0, 0xC1, 0xC2):
            H, W = struct.unpack(">HH", jpg[i + 5:i + 9])
            return H, W
        i += 2 + ln
    raise ValueError("write_avi: no SOF segment in the first frame")


def _audio_split(n_samples, n_frames, fps, sample_rate):
    """Sample index where the audio chunk of each video frame starts (n_frames + 1 bounds):
    frame i carries samples [round(i * sr / fps), round((i + 1) * sr / fps)), the last one the rest."""
    b = [min(n_samples, int(round(i * sample_rate / fps))) for i in range(n_frames)]
    return b + [n_samples]


def _pad(n):
    return n + (n & 1)


HDRL_BYTES = 4 + (8 + 56) + 2 * (12 + 8 + 56) + (8 + 40) + (8 + 18)  # 'hdrl' + avih + 2 x (LIST strl, strh) + strf x 2


def avi_file_size(jpeg_lens, audio_chunk_bytes):
    """Size in bytes of the file write_avi produces for these chunk payload lengths
    (``audio_chunk_bytes`` empty when there is no audio stream)."""
    chunks = list(jpeg_lens) + [b for b in audio_chunk_bytes if b]
    movi = 4 + sum(8 + _pad(c) for c in chunks)
    hdrl = HDRL_BYTES if len(audio_chunk_bytes) else HDRL_BYTES - (12 + 8 + 56) - (8 + 18)
    return 12 + (8 + hdrl) + (8 + movi) + (8 + 16 * len(chunks))


def write_avi(path, jpeg_frames, fps, audio=None, sample_rate=16000):
    """Write complete JPEG byte strings (one per frame, all of one size) and optional mono
    float audio as a plain AVI 1.0 file: RIFF 'AVI ' { LIST hdrl { avih, LIST strl (vids /
    MJPG, BITMAPINFOHEADER), LIST strl (auds, WAVEFORMATEX PCM s16 mono) }, LIST movi {
    00dc / 01wb interleaved per video frame }, idx1 }.  Chunks are padded to even length.
    A file that would exceed 2^31 - 1 bytes is refused before anything is written."""
    frames = [bytes(j) for j in jpeg_frames]
    if not frames:
        raise ValueError("write_avi: no frames")
    H, W = _jpeg_size(frames[0])
    rate, scale = _fps_ratio(fps)
    fps_f = rate / scale
    n = len(frames)
    pcm = None if audio is None else audio_to_s16(audio)
    sample_rate = int(sample_rate)
    bounds = _audio_split(len(pcm), n, fps_f, sample_rate) if pcm is not None else None
    a_bytes = [2 * (bounds[i + 1] - bounds[i]) for i in range(n)] if pcm is not None else []
    total = avi_file_size([len(j) for j in frames], a_bytes)
    if total > AVI_MAX_BYTES:
        raise ValueError(f"write_avi: {path} would be {total} bytes, above the AVI 1.0 limit of 2^31 - 1 = "
                         f"{AVI_MAX_BYTES} bytes (OpenDML is out of scope): lower the quality or split the clip")
    movi, index, pos = [b"movi"], [], 4  # index offsets count from the 'movi' FourCC

    def add(ckid, payload):
        nonlocal pos
        index.append(struct.pack("<4sIII", ckid, 0x10, pos, len(payload)))  # AVIIF_KEYFRAME
        movi.append(ckid + struct.pack("<I", len(payload)) + payload + b"\0" * (len(payload) & 1))
        pos += 8 + _pad(len(payload))

    for i, j in enumerate(frames):
        add(b"00dc", j)
        if pcm is not None and a_bytes[i]:
            add(b"01wb", pcm[bounds[i]:bounds[i + 1]].tobytes())
    movi = b"".join(movi)
    max_v = max(len(j) for j in frames)
    max_a = max(a_bytes) if a_bytes else 0
    n_streams = 2 if pcm is not None else 1
    bytes_per_sec = int(sum(len(j) for j in frames) * fps_f / n) + (2 * sample_rate if pcm is not None else 0)
    avih = struct.pack("<14I", int(round(1e6 / fps_f)), bytes_per_sec, 0, 0x10 | 0x100, n, 0, n_streams,
                       max(max_v, max_a), W, H, 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n, max_v, 0xFFFFFFFF, 0,
                         0, 0, W, H)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    chunk = lambda cid, body: cid + struct.pack("<I", len(body)) + body + b"\0" * (len(body) & 1)
    lst = lambda kind, body: b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body
    hdrl = chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh_v) + chunk(b"strf", strf_v))
    if pcm is not None:
        strh_a = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, sample_rate, 0, len(pcm),
                             max_a, 0xFFFFFFFF, 2, 0, 0, 0, 0)
        strf_a = struct.pack("<HHIIHHH", 1, 1, sample_rate, 2 * sample_rate, 2, 16, 0)
        hdrl += lst(b"strl", chunk(b"strh", strh_a) + chunk(b"strf", strf_a))
    body = b"AVI " + lst(b"hdrl", hdrl) + b"LIST" + struct.pack("<I", len(movi)) + movi + chunk(b"idx1", b"".join(index))
    assert 8 + len(body) == total, (8 + len(body), total)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


def write_video(path, frames_dev_u8, fps, audio=None, sample_rate=16000, quality=95):
    """Encode device uint8 (n, H, W, 3) frames as Motion-JPEG on the device and mux them
    with the audio into ``path`` (AVI)."""
    return write_avi(path, encode_frames(frames_dev_u8, quality), fps, audio, sample_rate)


# ---------------------------------------------------------------------------- AVI reader

def _chunks(buf, start, end, path, where):
    """Yield (id, payload start, size) of the chunks in buf[start:end], honouring pad bytes;
    a chunk whose header or payload passes ``end`` is a truncation."""
    pos = start
    while pos < end:
        if pos + 8 > end:
            raise ValueError(f"{path}: truncated chunk header in {where} at byte {pos}")
        cid, size = struct.unpack("<4sI", buf[pos:pos + 8])
        if pos + 8 + size > end:
            raise ValueError(f"{path}: truncated {where}: chunk {cid!r} at byte {pos} declares {size} bytes, "
                             f"{end - pos - 8} are left")
        yield cid, pos + 8, size
        pos += 8 + _pad(size)


def _decode_bi_rgb(raw, W, H, path):
    top_down = H < 0
    H = abs(H)
    stride = (W * 3 + 3) & ~3
    if len(raw) < stride * H:
        raise ValueError(f"{path}: truncated BI_RGB frame ({len(raw)} bytes, {stride * H} expected)")
    a = np.frombuffer(raw, np.uint8, stride * H).reshape(H, stride)[:, :W * 3].reshape(H, W, 3)[..., ::-1]
    return np.ascontiguousarray(a if top_down else a[::-1])


def _walk_avi(path):
    """The RIFF walk shared by read_avi and read_avi_device: -> (codec 'mjpg' | 'rgb', W,
    signed H, fps, list of video chunk payloads, audio float32 mono or None, sample_rate).
    Unknown chunks are skipped, pad bytes honoured, 'rec ' lists descended; PCM 16-bit
    audio is returned as s16 / 32768 (more channels are averaged).  Any other video codec,
    audio format, or a truncated file is a ValueError naming the file."""
    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 12 or buf[:4] != b"RIFF" or buf[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF/AVI file")
    riff_end = 8 + struct.unpack("<I", buf[4:8])[0]
    if riff_end > len(buf):
        raise ValueError(f"{path}: truncated: the RIFF header declares {riff_end} bytes, the file has {len(buf)}")
    streams, movi, fps_avih = [], None, None
    for cid, p, size in _chunks(buf, 12, riff_end, path, "RIFF"):
        kind = buf[p:p + 4] if cid == b"LIST" else None
        if kind == b"hdrl":
            for c2, p2, s2 in _chunks(buf, p + 4, p + size, path, "hdrl"):
                if c2 == b"avih" and s2 >= 4:
                    us = struct.unpack("<I", buf[p2:p2 + 4])[0]
                    fps_avih = 1e6 / us if us else None
                elif c2 == b"LIST" and buf[p2:p2 + 4] == b"strl":
                    st = {}
                    for c3, p3, s3 in _chunks(buf, p2 + 4, p2 + s2, path, "strl"):
                        if c3 in (b"strh", b"strf"):
                            st[c3] = buf[p3:p3 + s3]
                    streams.append(st)
        elif kind == b"movi":
            movi = (p + 4, p + size)
    if movi is None:
        raise ValueError(f"{path}: no movi list")
    vid = aud = None
    for i, st in enumerate(streams):
        if len(st.get(b"strh", b"")) < 36 or b"strf" not in st:
            raise ValueError(f"{path}: stream {i} has a truncated strh or no strf")
        if st[b"strh"][:4] == b"vids" and vid is None:
            vid = i
        elif st[b"strh"][:4] == b"auds" and aud is None:
            aud = i
    if vid is None:
        raise ValueError(f"{path}: no video stream")
    strh, strf = streams[vid][b"strh"], streams[vid][b"strf"]
    if len(strf) < 40:
        raise ValueError(f"{path}: truncated BITMAPINFOHEADER ({len(strf)} bytes)")
    scale, rate = struct.unpack("<II", strh[20:28])
    fps = rate / scale if scale and rate else fps_avih
    if not fps:
        raise ValueError(f"{path}: the video stream declares no frame rate")
    W, Hs, _, bitcount, comp = struct.unpack("<iiHH4s", strf[4:20])
    if comp.upper() == b"MJPG":
        codec = "mjpg"
    elif comp == b"\0\0\0\0" and bitcount == 24:
        codec = "rgb"
    else:
        name = comp.decode("latin-1") if comp.strip(b"\0") else f"BI_RGB with {bitcount} bits"
        raise ValueError(f"{path}: unsupported video codec FourCC {name!r} (MJPG and 24-bit BI_RGB are read)")
    sr, n_ch = None, 1
    if aud is not None:
        fa = streams[aud][b"strf"]
        if len(fa) < 16:
            raise ValueError(f"{path}: truncated WAVEFORMAT ({len(fa)} bytes)")
        tag, n_ch, sr, _, _, bits = struct.unpack("<HHIIHH", fa[:16])
        if tag != 1 or bits != 16 or n_ch < 1:
            raise ValueError(f"{path}: unsupported audio format (wFormatTag 0x{tag:04X}, {bits} bits): 16-bit PCM "
                             "is read")
    frames, pcm = [], []

    def walk(start, end):
        for cid, p, size in _chunks(buf, start, end, path, "movi"):
            if cid == b"LIST":
                walk(p + 4, p + size)
            elif cid[:2].isdigit() and int(cid[:2]) == vid and cid[2:] in (b"dc", b"db") and size:
                frames.append(buf[p:p + size])
            elif aud is not None and cid[:2].isdigit() and int(cid[:2]) == aud and cid[2:] == b"wb":
                pcm.append(buf[p:p + size])

    walk(*movi)
    audio = None
    if aud is not None:
        a = np.frombuffer(b"".join(pcm), "<i2")
        a = a[:len(a) // n_ch * n_ch].astype(np.float32) / np.float32(32768.0)
        audio = a if n_ch == 1 else a.reshape(-1, n_ch).mean(axis=1, dtype=np.float32)
    return codec, W, Hs, fps, frames, audio, sr


def read_avi(path):
    """-> (frames uint8 (N, H, W, 3) RGB, fps, audio float32 mono or None, sample_rate),
    all on the host: MJPG frames are decoded with Pillow, 24-bit BI_RGB frames directly
    (the route of CPU-only hosts; ``read_avi_device`` decodes on the device).  The
    container rules and errors are ``_walk_avi``'s."""
    codec, W, Hs, fps, frames, audio, sr = _walk_avi(path)
    if codec == "mjpg":
        from PIL import Image
        dec = []
        for i, j in enumerate(frames):
            try:
                with Image.open(io.BytesIO(j)) as im:
                    dec.append(np.asarray(im.convert("RGB")))
            except Exception as e:  # Pillow raises OSError / SyntaxError subclasses for bad streams
                raise ValueError(f"{path}: frame {i} is not a decodable JPEG ({e})") from e
            if dec[-1].shape != (abs(Hs), W, 3):
                raise ValueError(f"{path}: frame {i} is {dec[-1].shape[1]}x{dec[-1].shape[0]}, the header says "
                                 f"{W}x{abs(Hs)}")
    else:
        dec = [_decode_bi_rgb(j, W, Hs, path) for j in frames]
    out = np.stack(dec) if dec else np.zeros((0, abs(Hs), W, 3), np.uint8)
    return out, fps, audio, sr


def _avi_device_infos(frames):
    """parse_jpeg of every MJPG chunk -> (list of JpegInfo, None), or (None, why) when a
    header cannot be parsed or a frame is outside the device subset."""
    infos = []
    for i, j in enumerate(frames):
        try:
            info = parse_jpeg(j)
        except ValueError as e:
            return None, f"frame {i}: {e}"
        if not info.on_device:
            return None, f"frame {i}: {info.reason}"
        infos.append(info)
    return infos, None


def read_avi_device(path, device, _walked=None):
    """``read_avi`` with the frames decoded on ``device``: -> (frames uint8 (N, H, W, 3) RGB
    device tensor, fps, audio, sample_rate).  MJPG frames go through ``decode_frames`` (only
    compressed bytes are uploaded); BI_RGB frames are uploaded as stored and flipped there.
    Errors are read_avi's, plus a ValueError for a frame outside the device subset of JPEG
    (read_avi decodes those on the host)."""
    import torch
    codec, W, Hs, fps, frames, audio, sr = _walked or _walk_avi(path)
    device = torch.device(device)
    H = abs(Hs)
    if not frames:
        return torch.zeros((0, H, W, 3), dtype=torch.uint8, device=device), fps, audio, sr
    if codec == "mjpg":
        infos, why = _avi_device_infos(frames)
        if infos is None:
            raise ValueError(f"{path}: {why} -- not in the device subset of JPEG")
        for i, info in enumerate(infos):
            if (info.H, info.W) != (H, W):
                raise ValueError(f"{path}: frame {i} is {info.W}x{info.H}, the header says {W}x{H}")
        out, status = decode_frames_status(list(zip(frames, infos)), device)
        for i, s in enumerate(status):
            if s:
                raise ValueError(f"{path}: frame {i} is not a decodable JPEG ({_STATUS_TEXT.get(s, f'status {s}')})")
    else:
        stride = (W * 3 + 3) & ~3
        for j in frames:
            if len(j) < stride * H:
                raise ValueError(f"{path}: truncated BI_RGB frame ({len(j)} bytes, {stride * H} expected)")
        raw = torch.frombuffer(bytearray(b"".join(j[:stride * H] for j in frames)), dtype=torch.uint8).to(device)
        out = raw.view(len(frames), H, stride)[:, :, :W * 3].reshape(len(frames), H, W, 3).flip(3)  # BGR -> RGB
        out = (out if Hs < 0 else out.flip(1)).contiguous()  # bottom-up unless the height is negative
    return out, fps, audio, sr


def read_avi_auto(path, device=None):
    """The reader of pipeline.read_video_frames: ``read_avi_device`` when ``device`` is a
    HIP device and every frame is in the device subset, else ``read_avi``, unchanged."""
    import torch
    if device is None or not torch.cuda.is_available() or torch.device(device).type != "cuda":
        return read_avi(path)
    walked = _walk_avi(path)
    if walked[0] == "mjpg" and _avi_device_infos(walked[4])[0] is None:
        return read_avi(path)
    return read_avi_device(path, device, walked)
