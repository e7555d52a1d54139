"""Host side of the video writer (no GPU): the CPU restatement of the device Motion-JPEG
encoder (tests/mjpeg_cpu.py) against Pillow, the AVI container (write_avi / read_avi), and
the .avi wiring of read_video_frames and of __call__'s trim.

Quality yardstick.  The restatement repeats libjpeg's integer arithmetic exactly (colour
conversion, 2x2 chroma average, islow DCT, quantiser, edge padding of every block that
reaches into the frame), so the measured gap to Pillow's own encode with the same tables,
4:2:0 and optimize=False is 0: the decoded pixels are EQUAL on every test frame (40x56,
8x8, 17x33, 64x64; smooth and noise content; qualities 1, 50, 95, 100), and without
restart markers even the scan bytes are.  DELTA_DB = 0 states that; the tests assert
equal pixels, which is stronger than any PSNR margin."""
import io
import struct
import warnings

import numpy as np
import pytest

import mjpeg_cpu as mj
from latentsync_amd import video
from latentsync_amd.pipeline import read_video_frames

Image = pytest.importorskip("PIL.Image")

DELTA_DB = 0.0  # measured gap restatement - Pillow: 0 dB (equal decoded pixels), doubled: 0
RI = 10         # the device encoder's restart interval (asserted on the GPU in test_gpu_mjpeg.py)


def pil_encode(rgb, quality):
    ql, qc = video.quant_tables(quality)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", qtables=[[int(v) for v in ql], [int(v) for v in qc]], subsampling=2,
                              optimize=False)
    return b.getvalue()


def pil_decode(jpg, size=None):
    """Decode with every warning an error; ``size`` = the expected (H, W)."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(jpg)) as im:
            assert im.format == "JPEG" and im.mode == "RGB"
            if size is not None:
                assert im.size == (size[1], size[0])
            im.load()
            return np.asarray(im.convert("RGB"))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def assert_decodes_like_pillow(rgb, quality, ri=RI, what=""):
    H, W, _ = rgb.shape
    ours = pil_decode(mj.encode_jpeg(rgb, quality, ri), (H, W))
    ref = pil_decode(pil_encode(rgb, quality), (H, W))
    gap = psnr(ref, rgb) - psnr(ours, rgb)
    print(f"{what} {H}x{W} q{quality}: PSNR ours {psnr(ours, rgb):.3f} dB, Pillow {psnr(ref, rgb):.3f} dB")
    assert gap <= DELTA_DB
    assert np.array_equal(ours, ref)
    return ours


def segments(jpg):
    """[(marker, payload)] of the segments up to and including SOS."""
    i, out = 2, []
    while True:
        m, ln = jpg[i + 1], struct.unpack(">H", jpg[i + 2:i + 4])[0]
        out.append((m, jpg[i + 4:i + 2 + ln]))
        i += 2 + ln
        if m == 0xDA:
            return out, i


# ------------------------------------------------------------------ restatement vs Pillow

def test_tables_are_the_ones_pillow_writes():
    rgb = mj.noise_frame(16, 16, 0)
    for q in (1, 37, 50, 95, 100):
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, "JPEG", quality=q, subsampling=2, optimize=False)
        theirs, _ = segments(b.getvalue())
        ours, _ = segments(video.jpeg_headers(16, 16, q, RI))
        assert [p for m, p in theirs if m == 0xDB] == [p for m, p in ours if m == 0xDB], q
        dht = {p[0]: p for m, p in ours if m == 0xC4}
        blob = b"".join(p for m, p in theirs if m == 0xC4)
        i = 0
        while i < len(blob):
            n = 17 + sum(blob[i + 1:i + 17])
            assert dht.pop(blob[i]) == blob[i:i + n]
            i += n
        assert not dht
        assert [p for m, p in theirs if m in (0xC0, 0xDA)] == [p for m, p in ours if m in (0xC0, 0xDA)]
    assert [m for m, _ in ours] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert dict(ours)[0xDD] == struct.pack(">H", RI)


@pytest.mark.parametrize("H,W", [(40, 56), (8, 8), (17, 33), (64, 64)])
def test_restatement_is_valid_jpeg_and_matches_pillow(H, W):
    for q in (1, 50, 95, 100):
        assert_decodes_like_pillow(mj.smooth_frames(1, H, W, 3)[0], q, what="smooth")
    assert_decodes_like_pillow(mj.noise_frame(H, W, 1), 95, what="noise")


def test_scan_without_restarts_equals_libjpegs():
    rgb = mj.smooth_frames(1, 48, 64, 5)[0]
    for q in (50, 95, 100):
        pj = pil_encode(rgb, q)
        _, start = segments(pj)
        assert mj.scan_from_coefficients(mj.frame_coefficients(rgb, q), 10 ** 6) == pj[start:-2]


# ------------------------------------------------------------------ coding edge cases

def test_black_frame_is_all_eob():
    rgb = np.zeros((32, 48, 3), np.uint8)
    co = mj.frame_coefficients(rgb, 95)
    assert (co[..., 1:] == 0).all() and (co[:, :4, 0] == -1024 // 2).all()  # DC step 2 at q95: -1024 / 2
    assert np.array_equal(assert_decodes_like_pillow(rgb, 95, what="black"), rgb)


def test_checker_has_dc_differences_of_category_11():
    rgb = mj.checker_frame(32, 48)
    co = mj.frame_coefficients(rgb, 100)
    y_dc = co[:, :4, 0]
    assert set(np.unique(y_dc)) == {-1024, 1016}
    assert abs(int(y_dc[0, 1]) - int(y_dc[0, 0])) == 2040 and (2040).bit_length() == 11
    assert_decodes_like_pillow(rgb, 100, what="checker")


def test_last_coefficient_only_blocks_code_three_zrl_and_no_eob():
    rgb = mj.last_coefficient_frame(32, 48)
    co = mj.frame_coefficients(rgb, 1)
    assert (co[:, :4, :63] == 0).all() and (np.abs(co[:, :4, 63]) == 2).all() and (co[:, 4:] == 0).all()
    bw = mj.BitWriter()
    mj.encode_block(bw, co[0, 0], 0, 0)
    zrl, dc0 = mj.AC[0][0xF0], mj.DC[0][0]
    sym = mj.AC[0][14 << 4 | 2]
    assert bw.n == dc0[1] + 3 * zrl[1] + sym[1] + 2  # DC category 0, ZRL x 3, (run 14, size 2) + 2 bits, no EOB
    head = dc0[0]
    for _ in range(3):
        head = head << zrl[1] | zrl[0]
    assert bw.acc >> (bw.n - dc0[1] - 3 * zrl[1]) == head
    assert_decodes_like_pillow(rgb, 1, what="last coefficient")
    # the same through coefficients alone, in all six blocks of every MCU
    only = np.zeros((6, 6, 64), np.int64)
    only[..., 63] = 3
    pil_decode(mj.wrap_coefficients(only, 32, 48, 50, RI), (32, 48))


def test_noise_at_q100_stuffs_many_ff_bytes():
    rgb = mj.noise_frame(48, 80, 2)
    scan = mj.encode_scan(rgb, 100, RI)
    assert scan.count(b"\xff\x00") >= 20
    i = 0
    while (i := scan.find(b"\xff", i)) >= 0:  # every 0xFF is stuffed or a restart marker
        assert scan[i + 1] == 0 or 0xD0 <= scan[i + 1] <= 0xD7
        i += 2
    assert_decodes_like_pillow(rgb, 100, what="noise")


def test_restart_markers_wrap_modulo_8():
    rgb = mj.smooth_frames(1, 24, 16 * 95 + 5, 8)[0]  # 2 x 96 MCUs = 20 intervals of 10
    scan = mj.encode_scan(rgb, 95, RI)
    marks = [scan[i + 1] - 0xD0 for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [k % 8 for k in range(19)]
    assert_decodes_like_pillow(rgb, 95, what="20 intervals")
    assert_decodes_like_pillow(mj.smooth_frames(1, 48, 48, 9)[0], 95, ri=1, what="Ri 1, 9 intervals")


# ------------------------------------------------------------------ container

def _clip(n=5, H=24, W=40, q=90):
    frames = mj.smooth_frames(n, H, W, 12)
    jpgs = []
    for i, f in enumerate(frames):
        s = io.BytesIO()
        Image.fromarray(f).save(s, "JPEG", quality=q)
        j = s.getvalue()
        jpgs.append(j if len(j) % 2 == i % 2 else j + b"\0")  # odd and even chunk lengths (a byte after EOI is legal)
    return frames, jpgs


def _walk(buf, start, end):
    pos = start
    while pos < end:
        cid, size = struct.unpack("<4sI", buf[pos:pos + 8])
        assert pos % 2 == 0 and pos + 8 + size <= end, (cid, pos, size, end)
        yield cid, pos, size
        pos += 8 + size + (size & 1)
    assert pos == end


def test_avi_round_trip_and_structure(tmp_path):
    frames, jpgs = _clip()
    assert {len(j) % 2 for j in jpgs} == {0, 1}
    n, fps, sr = len(jpgs), 25, 16000
    audio = np.random.default_rng(4).uniform(-1.2, 1.2, 3333).astype(np.float32)  # some samples clip
    path = str(tmp_path / "a.avi")
    video.write_avi(path, jpgs, fps, audio, sr)
    got, got_fps, got_audio, got_sr = video.read_avi(path)
    assert got_fps == fps and got_sr == sr
    assert np.array_equal(got, np.stack([pil_decode(j) for j in jpgs]))
    s16 = np.round(np.clip(audio.astype(np.float64), -1, 1) * 32767).astype(np.int16)
    assert got_audio.dtype == np.float32 and np.array_equal((got_audio * 32768).astype(np.int16), s16)
    assert s16.min() == -32767 and s16.max() == 32767

    buf = open(path, "rb").read()
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI " and struct.unpack("<I", buf[4:8])[0] == len(buf) - 8
    top = {(cid, buf[p + 8:p + 12] if cid == b"LIST" else None): (p, s) for cid, p, s in _walk(buf, 12, len(buf))}
    assert list(top) == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hp, hs = top[(b"LIST", b"hdrl")]
    hdrl = list(_walk(buf, hp + 12, hp + 8 + hs))
    assert [c for c, _, _ in hdrl] == [b"avih", b"LIST", b"LIST"]
    avih = struct.unpack("<14I", buf[hdrl[0][1] + 8:hdrl[0][1] + 64])
    mp, ms = top[(b"LIST", b"movi")]
    chunks = list(_walk(buf, mp + 12, mp + 8 + ms))
    vid = [(p, s) for c, p, s in chunks if c == b"00dc"]
    aud = [(p, s) for c, p, s in chunks if c == b"01wb"]
    assert [buf[p + 8:p + 8 + s] for p, s in vid] == jpgs
    assert b"".join(buf[p + 8:p + 8 + s] for p, s in aud) == s16.astype("<i2").tobytes()
    assert [c for c, _, _ in chunks[:4]] == [b"00dc", b"01wb", b"00dc", b"01wb"]  # interleaved per frame
    assert avih[0] == 40000 and avih[4] == n and avih[6] == 2 and avih[8:10] == (40, 24) and avih[3] & 0x10
    assert avih[7] == max(s for _, s in vid + aud)  # dwSuggestedBufferSize
    for k, (kind, handler, length, sugg, scale_rate) in enumerate((
            (b"vids", b"MJPG", n, max(s for _, s in vid), (1, 25)),
            (b"auds", b"\0\0\0\0", len(s16), max(s for _, s in aud), (1, sr)))):
        lp = hdrl[1 + k][1]
        sub = list(_walk(buf, lp + 12, lp + 8 + hdrl[1 + k][2]))
        assert [c for c, _, _ in sub] == [b"strh", b"strf"] and sub[0][2] == 56
        strh = buf[sub[0][1] + 8:sub[0][1] + 64]
        assert strh[:4] == kind and strh[4:8] == handler
        assert struct.unpack("<II", strh[20:28]) == scale_rate
        assert struct.unpack("<II", strh[32:40]) == (length, sugg)
        strf = buf[sub[1][1] + 8:sub[1][1] + 8 + sub[1][2]]
        if k == 0:
            assert struct.unpack("<IiiHH4sI", strf[:24]) == (40, 40, 24, 1, 24, b"MJPG", 40 * 24 * 3)
        else:
            assert struct.unpack("<HHIIHHH", strf) == (1, 1, sr, 2 * sr, 2, 16, 0)
    ip, isz = top[(b"idx1", None)]
    assert isz == 16 * len(chunks)
    for k, (cid, p, s) in enumerate(chunks):
        ckid, flags, off, size = struct.unpack("<4sIII", buf[ip + 8 + 16 * k:ip + 24 + 16 * k])
        assert (ckid, size) == (cid, s) and flags & 0x10 and mp + 8 + off == p  # offsets from the 'movi' FourCC
    assert video.avi_file_size([len(j) for j in jpgs], [s for _, s in aud]) == len(buf)

    video.write_avi(path, jpgs, 30000 / 1001)  # video only, NTSC rate
    got, got_fps, got_audio, got_sr = video.read_avi(path)
    assert got.shape == (n, 24, 40, 3) and got_audio is None and got_sr is None and abs(got_fps - 29.97) < 1e-3


def _bi_rgb_avi(frames, fps=25, fourcc=b"\0\0\0\0", bits=24, junk=True):
    n, H, W, _ = frames.shape
    stride = (W * 3 + 3) & ~3
    chunk = lambda cid, body: cid + struct.pack("<I", len(body)) + body + b"\0" * (len(body) & 1)
    lst = lambda kind, body: b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body
    movi = b""
    for f in frames:
        rows = np.zeros((H, stride), np.uint8)
        rows[:, :W * 3] = f[::-1, :, ::-1].reshape(H, W * 3)  # bottom-up, BGR
        movi += chunk(b"00db", rows.tobytes())
        if junk:
            movi += chunk(b"JUNK", b"abc")  # unknown chunk with a pad byte
    avih = struct.pack("<14I", 1000000 // fps, 0, 0, 0, n, 0, 1, stride * H, W, H, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"DIB ", 0, 0, 0, 0, 1, fps, 0, n, stride * H, 0, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, bits, fourcc, stride * H, 0, 0, 0, 0)
    body = b"AVI " + lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    body += chunk(b"JUNK", b"\0" * 7) + lst(b"movi", movi)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_bi_rgb_with_padded_rows(tmp_path):
    frames = np.random.default_rng(5).integers(0, 256, (3, 5, 6, 3), dtype=np.uint8)  # W = 6: 18-byte rows -> 20
    p = tmp_path / "raw.avi"
    p.write_bytes(_bi_rgb_avi(frames))
    got, fps, audio, sr = video.read_avi(str(p))
    assert np.array_equal(got, frames) and fps == 25 and audio is None and sr is None


def test_documented_errors(tmp_path, monkeypatch):
    frames = np.zeros((2, 4, 6, 3), np.uint8)
    p = tmp_path / "x.avi"
    p.write_bytes(_bi_rgb_avi(frames, fourcc=b"H264"))
    with pytest.raises(ValueError, match="H264"):
        video.read_avi(str(p))
    p.write_bytes(_bi_rgb_avi(frames, bits=32))
    with pytest.raises(ValueError, match="32 bits"):
        video.read_avi(str(p))
    good = _bi_rgb_avi(frames, junk=False)
    cut = good[:-30]  # the last frame chunk of the movi list loses its tail
    p.write_bytes(cut[:4] + struct.pack("<I", len(cut) - 8) + cut[8:])
    with pytest.raises(ValueError, match="truncated"):
        video.read_avi(str(p))
    p.write_bytes(cut)  # the RIFF header still declares the full size
    with pytest.raises(ValueError, match="truncated"):
        video.read_avi(str(p))
    p.write_bytes(b"RIFF\x04\0\0\0WAVE")
    with pytest.raises(ValueError, match="not a RIFF/AVI"):
        video.read_avi(str(p))
    _, jpgs = _clip(2)
    out = tmp_path / "big.avi"
    monkeypatch.setattr(video, "avi_file_size", lambda *a: 2 ** 31)
    with pytest.raises(ValueError, match=r"2\^31 - 1"):
        video.write_avi(str(out), jpgs, 25)
    assert not out.exists()  # refused before anything is written
    with pytest.raises(ValueError, match="no frames"):
        video.write_avi(str(out), [], 25)


# ------------------------------------------------------------------ wiring

def test_read_video_frames_reads_an_avi(tmp_path):
    frames, jpgs = _clip(3)
    path = str(tmp_path / "in.avi")
    video.write_avi(path, jpgs, 25, np.zeros(1000, np.float32))
    got = read_video_frames(path, 25)
    assert got.dtype == np.uint8 and np.array_equal(got, np.stack([pil_decode(j) for j in jpgs]))
    assert np.array_equal(read_video_frames(path), got)
    with pytest.raises(ValueError, match="video_fps"):
        read_video_frames(path, 30)
    assert read_video_frames(str(tmp_path / "missing.avi"), 25) is None


def test_run_job_output_format(tmp_path):
    """serve.run_job: output_format picks the extension of video_out_path; "npz" by default."""
    from latentsync_amd import serve
    seen = []

    def pipeline(**kw):
        seen.append(kw["video_out_path"])

    for name in ("v1.mp4", "v1.pth", "j1.wav"):
        (tmp_path / name).write_bytes(b"-")
    job = {"id": "j1", "video_id": "v1", "audio_url": str(tmp_path / "j1.wav")}
    for extra, ext in (({}, "npz"), ({"output_format": None}, "npz"), ({"output_format": "npz"}, "npz"),
                       ({"output_format": "avi"}, "avi")):
        res = serve.run_job(pipeline, dict(job, **extra), str(tmp_path), str(tmp_path / "results"), 64)
        assert res["output_url"] == seen[-1] == str(tmp_path / "results" / f"j1.{ext}")
    with pytest.raises(ValueError, match="output_format"):
        serve.run_job(pipeline, dict(job, output_format="mp4"), str(tmp_path), str(tmp_path / "results"), 64)
    assert serve.RequestPayload(id="a", video_id="b", audio_url="c").model_dump()["output_format"] is None


def test_trim_counts():
    """T = n / fps - padding_duration; frames i / fps < T and samples j / sr < T stay."""
    tc = video.trim_counts
    assert tc(24, 25, 16000, 16000, 0.0, False) == (24, 15360)
    assert tc(24, 25, 15000, 16000, 0.0, False) == (24, 15000)     # shorter audio is kept whole
    for k in range(16):                                              # every padding __call__ can produce
        n = 32
        kf, ka = tc(n, 25, 10 ** 6, 16000, k / 25, False)
        assert (kf, ka) == (n - k, (n - k) * 640), k
        assert all(i / 25 < n / 25 - k / 25 + 1e-9 for i in range(kf))
    assert tc(16, 25, 10 ** 6, 16000, 0.02, False) == (16, 9920)     # T = 0.62 s: frame 15 starts at 0.60 s
    assert tc(16, 25, 10 ** 6, 16000, 0.05, False) == (15, 9440)     # T = 0.59 s
    assert tc(16, 30000 / 1001, 10 ** 6, 44100, 0.0, False) == (16, 23544)  # ceil(16 * 1001 / 30000 * 44100)
    assert tc(16, 25, 10 ** 6, 16000, 0.64, False) == (0, 0)
    assert tc(16, 25, 10 ** 6, 16000, 0.4, True) == (16, 10240)      # start_from_backwards / force_video_length
    assert tc(16, 25, 5000, 16000, 0.4, True) == (16, 5000)
