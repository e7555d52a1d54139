"""Video files: Motion-JPEG in an AVI 1.0 container with 16-bit PCM audio (host side).

The writer is the job ffmpeg does for the reference's write_video (util.py:140-160) and
its audio mux (lipsync_pipeline.py:596-603), for the one format that needs no third-party
codec.  The frames are compressed where they already are: ops.mjpeg_encode (ls_mjpeg_encode,
csrc/ls_video.hip) returns every frame's entropy-coded scan, ``jpeg_headers`` builds the
segments in front of it on the host, and ``write_avi`` muxes complete JPEG byte strings
with the audio.  ``read_avi`` is the way back in for ``read_video_frames``: MJPG frames
(decoded with Pillow -- JPEG entropy decoding is serial host work, what ffmpeg does for
the reference) and uncompressed 24-bit BI_RGB frames.  H.264 / mp4, OpenDML files above
2 GiB and frame-rate conversion are out of scope.
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


def read_avi(path):
    """-> (frames uint8 (N, H, W, 3) RGB, fps, audio float32 mono or None, sample_rate).
    Walks the RIFF tree (unknown chunks skipped, pad bytes honoured, 'rec ' lists
    descended); MJPG frames are decoded with Pillow, 24-bit BI_RGB frames directly; PCM
    16-bit audio is returned as s16 / 32768 (more channels are averaged).  Any other video
    codec, audio format, or a truncated file is a ValueError naming the file."""
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
    audio = None
    if aud is not None:
        a = np.frombuffer(b"".join(pcm), "<i2")
        a = a[:len(a) // n_ch * n_ch].astype(np.float32) / np.float32(32768.0)
        audio = a if n_ch == 1 else a.reshape(-1, n_ch).mean(axis=1, dtype=np.float32)
    return out, fps, audio, sr
