"""Host side of the Motion-JPEG decoder without a GPU: the CPU restatement
(tests/mjpeg_dec_cpu.py) equals Pillow / libjpeg bit for bit over sizes, contents, samplings,
qualities, table kinds and restart intervals -- which pins the oracle of
tests/test_gpu_mjpeg_decode.py to libjpeg -- and video.parse_jpeg classifies files into and
out of the device subset."""
import io
import struct

import numpy as np
import pytest

import mjpeg_cpu as mj
import mjpeg_dec_cpu as dec
from latentsync_amd import video

Image = pytest.importorskip("PIL.Image")

# 7 sizes from the smallest the subset holds to several MCUs, odd ones included
SIZES = [(3, 3), (8, 8), (5, 19), (16, 16), (17, 33), (31, 24), (48, 64)]
SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
QUALITIES = [1, 20, 75, 95, 100]


def pillow_jpeg(rgb, sampling, quality, optimize=False, restart=0, **kw):
    im = Image.fromarray(rgb)
    if sampling == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = sampling
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    im.save(b, "JPEG", quality=quality, optimize=optimize, **kw)
    return b.getvalue()


def pillow_decode(jpg):
    return np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))


def frame(kind, H, W):
    return mj.smooth_frames(1, max(H, 2), max(W, 2), 5 + H + W)[0][:H, :W] if kind == "smooth" else \
        mj.noise_frame(H, W, 11 + H + W)


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_equals_pillow(H, W, sampling):
    """2 contents x 5 qualities x standard / optimised tables x with / without restart
    markers for every size and sampling: 7 x 4 x 40 = 1120 files, no tolerance."""
    n = 0
    for kind in ("smooth", "noise"):
        rgb = frame(kind, H, W)
        for quality in QUALITIES:
            for optimize in (False, True):
                for restart in (0, 2):
                    jpg = pillow_jpeg(rgb, sampling, quality, optimize, restart)
                    info = video.parse_jpeg(jpg)
                    assert info.on_device and (info.H, info.W, info.Ri) == (H, W, restart)
                    assert video.MODE_NAMES[info.mode] == sampling
                    got, status = dec.decode_status(jpg)
                    assert status == 0
                    assert np.array_equal(got, pillow_decode(jpg)), (kind, quality, optimize, restart)
                    n += 1
    assert n == 40


def strip_dht(jpg):
    """The byte string without its DHT segments."""
    out, i = [jpg[:2]], 2
    while jpg[i + 1] != 0xDA:
        ln = struct.unpack(">H", jpg[i + 2:i + 4])[0]
        if jpg[i + 1] != 0xC4:
            out.append(jpg[i:i + 2 + ln])
        i += 2 + ln
    return b"".join(out) + jpg[i:]


@pytest.mark.parametrize("sampling", ["4:2:0", "4:4:4", "grey"])
def test_frame_without_dht_gets_the_annex_k_tables(sampling):
    """The MJPG-in-AVI convention: Pillow writes the Annex K tables when it does not
    optimise, so the stripped file decodes to the same pixels."""
    jpg = pillow_jpeg(frame("smooth", 24, 40), sampling, 90)
    bare = strip_dht(jpg)
    assert b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")] and len(bare) < len(jpg) - 100
    assert np.array_equal(dec.decode(bare), dec.decode(jpg))
    assert np.array_equal(dec.decode(bare), pillow_decode(jpg))
    # our own encoder's files too, stripped or not
    own = mj.encode_jpeg(frame("smooth", 24, 40), 90, 10)
    assert np.array_equal(dec.decode(strip_dht(own)), pillow_decode(own))


def test_huff_device_table_is_jdhuffs_derived_table():
    """Every code of the four Annex K tables decodes through the lookahead / maxcode /
    valoffset form to its symbol."""
    for spec in (video.HUFF_DC_LUMA, video.HUFF_DC_CHROMA, video.HUFF_AC_LUMA, video.HUFF_AC_CHROMA):
        t = video.huff_device_table(*spec)
        assert t.dtype == np.int32 and t.shape == (video.HUFF_TABLE_INTS,)
        look, maxcode, valoff = t[:128].view(np.uint16), t[128:146], t[146:164]
        val = t[164:].view(np.uint8)
        for (length, code), sym in dec._codes(spec).items():
            if length <= 8:
                for tail in (0, (1 << (8 - length)) - 1):
                    assert look[(code << (8 - length)) | tail] == (length << 8 | sym)
            else:
                assert look[code >> (length - 8)] == 0
                assert all(code >> (length - l) > maxcode[l] for l in range(9, length)) and code <= maxcode[length]
                assert val[code + valoff[length]] == sym
    with pytest.raises(ValueError, match="Huffman"):
        video.huff_device_table((3,) + (0,) * 15, (0, 1, 2))  # three codes of one bit


def test_parse_jpeg_in_the_subset():
    rgb = frame("smooth", 20, 28)
    for sampling, mode, ncomp, n_mcu in (("4:4:4", 1, 3, 12), ("4:2:2", 2, 3, 6), ("4:2:0", 3, 3, 4), ("grey", 0, 1, 12)):
        info = video.parse_jpeg(pillow_jpeg(rgb, sampling, 80))
        assert info.on_device and info.reason is None
        assert (info.mode, info.ncomp, info.n_mcu, info.n_segments, info.Ri) == (mode, ncomp, n_mcu, 1, 0)
        assert len(info.quant) == len(info.huff_dc) == len(info.huff_ac) == ncomp
    jpg = mj.encode_jpeg(rgb, 95, 3)
    info = video.parse_jpeg(jpg)
    assert info.on_device and (info.H, info.W, info.mode, info.Ri, info.n_segments) == (20, 28, 3, 3, 2)
    assert jpg[info.scan_start - 14:info.scan_start - 12] == b"\xff\xda"  # the SOS segment is 2 + 12 bytes
    ql, qc = video.quant_tables(95)
    assert info.quant == [tuple(ql), tuple(qc), tuple(qc)]
    assert info.huff_dc == [video.HUFF_DC_LUMA, video.HUFF_DC_CHROMA, video.HUFF_DC_CHROMA]
    assert info.huff_ac == [video.HUFF_AC_LUMA, video.HUFF_AC_CHROMA, video.HUFF_AC_CHROMA]
    # padding behind the scan and a missing EOI are harmless
    assert np.array_equal(dec.decode(jpg[:-2] + b"\0\0\0"), dec.decode(jpg))


def test_parse_jpeg_out_of_the_subset():
    rgb = frame("smooth", 20, 28)
    cases = [(pillow_jpeg(rgb, "4:2:0", 80, progressive=True), "progressive")]
    b = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(b, "JPEG", quality=80)
    cases.append((b.getvalue(), "4 components"))
    try:
        cases.append((pillow_jpeg(rgb, (4, 1, 1, 1, 1, 1), 80), "sampling factors 4x1"))
    except (TypeError, ValueError, OSError):
        pass  # this Pillow does not take raw sampling factors
    cases.append((pillow_jpeg(rgb[:2], "4:4:4", 80), "smaller than 3x3"))
    base = pillow_jpeg(rgb, "4:4:4", 80)
    sos = video.parse_jpeg(base).scan_start - 14  # a 3-component SOS segment is 2 + 12 bytes
    assert base[sos:sos + 2] == b"\xff\xda"
    dqt16 = b"\xff\xdb" + struct.pack(">HB64H", 2 + 1 + 128, 0x10, *([300] * 64))  # Pq = 1 redefines table 0
    cases.append((base[:sos] + dqt16 + base[sos:], "16-bit quantisation"))
    sof = base.index(b"\xff\xc0")
    cases.append((base[:sof + 1] + b"\xc1" + base[sof + 2:], "SOF1"))
    cases.append((base[:sof + 4] + b"\x0c" + base[sof + 5:], "12-bit"))
    adobe = b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0)
    cases.append((base[:2] + adobe + base[2:], "Adobe transform 0"))
    for jpg, why in cases:
        info = video.parse_jpeg(jpg)
        assert not info.on_device and why in info.reason, (why, info.reason)
        with pytest.raises(ValueError, match="not in the device subset"):
            video.decode_frames([jpg], "cpu")


def test_truncated_or_malformed_header_is_a_value_error():
    jpg = pillow_jpeg(frame("smooth", 20, 28), "4:2:0", 80)
    info = video.parse_jpeg(jpg)
    for cut in (0, 1, 3, 10, 30, info.scan_start - 5):
        with pytest.raises(ValueError, match="truncated|not a JPEG"):
            video.parse_jpeg(jpg[:cut])
    with pytest.raises(ValueError, match="not a JPEG"):
        video.parse_jpeg(b"RIFF" + jpg)
    with pytest.raises(ValueError, match="malformed"):
        video.parse_jpeg(jpg[:2] + b"\x00\x00" + jpg[2:])
    own = mj.encode_jpeg(frame("smooth", 20, 28), 80, 10)  # SOI, APP0 (18 bytes), DQT 0, DQT 1 (69 bytes each)
    assert own[20:22] == own[89:91] == b"\xff\xdb" and own[158:160] == b"\xff\xc0"
    with pytest.raises(ValueError, match="quantisation table 1 is not defined"):
        video.parse_jpeg(own[:89] + own[158:])


def test_restatement_status_rules():
    """The bad-stream rules the kernel shares: markers, a code that never ends, running out."""
    rgb = frame("noise", 32, 48)
    jpg = mj.encode_jpeg(rgb, 90, 2)
    info = video.parse_jpeg(jpg)
    head, scan = jpg[:info.scan_start], jpg[info.scan_start:-2]
    assert dec.decode_status(jpg)[1] == 0
    assert dec.decode_status(head + scan[:len(scan) // 2])[1] == dec.ST_MARKERS
    assert dec.decode_status(head + scan.replace(b"\xff\xd1", b"\xff\xd2", 1))[1] == dec.ST_MARKERS
    one = mj.encode_jpeg(rgb, 90, 6)  # 6 MCUs: a single segment, no markers
    i1 = video.parse_jpeg(one)
    assert i1.n_segments == 1
    assert dec.decode_status(one[:i1.scan_start] + one[i1.scan_start:-2][:200])[1] == dec.ST_SHORT
    assert dec.decode_status(one[:i1.scan_start] + b"\xff\x00" * 400)[1] == dec.ST_CODE


def test_read_video_frames_avi_without_a_device_is_the_host_route(tmp_path):
    """With no device named the .avi route is read_avi, unchanged (numpy frames), and the
    device decoder has no CPU path."""
    import torch
    from latentsync_amd.pipeline import read_video_frames
    frames = mj.smooth_frames(3, 24, 40, 3)
    jpgs = [mj.encode_jpeg(f, 90, 10) for f in frames]
    path = str(tmp_path / "clip.avi")
    video.write_avi(path, jpgs, 25)
    got = read_video_frames(path, 25)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    assert np.array_equal(got, np.stack([dec.decode(j) for j in jpgs]))
    assert np.array_equal(got, video.read_avi(path)[0])
    assert np.array_equal(read_video_frames(path, 25, device="cpu"), got)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            video.decode_frames(jpgs, "cuda")
