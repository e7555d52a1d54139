"""WAV ingest on the host (no GPU): the RIFF/WAVE reader of latentsync_amd.audio over
every sample format, channel count and container quirk it promises, its errors, its
bit-compatibility with the 16-bit / 16 kHz reader it replaces, and the design of the
polyphase resampling filter (resample_taps) applied by a float64 numpy restatement of
its definition written here.

Design bounds: steady-state passband error <= 3e-5 and stopband amplitude <= 5e-5, twice
the 1.2e-5 / 1.6e-5 and 2.4e-5 of the numpy prototype the filter was specified with
(the factor absorbs I0 / sinc library differences).  Measured here: passband 1.15e-5
(down) and 1.54e-5 (up), stopband 2.37e-5."""
import functools
import math
import struct

import numpy as np
import pytest

from latentsync_amd import audio as A
from latentsync_amd.audio import load_wav, read_wav, resample_taps, resample_taps64

GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")  # KSDATAFORMAT_SUBTYPE_*: tag + this


def fmt_chunk(tag, ch, rate, bits, extensible=False, valid_bits=None):
    block = ch * bits // 8
    if not extensible:
        return struct.pack("<HHIIHH", tag, ch, rate, rate * block, block, bits)
    return struct.pack("<HHIIHHHHI", 0xFFFE, ch, rate, rate * block, block, bits, 22, valid_bits or bits,
                       (1 << ch) - 1) + struct.pack("<H", tag) + GUID_TAIL


def chunk(cid, body, size=None):
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def riff(*chunks, form=b"WAVE"):
    body = form + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def s24_bytes(v):
    return (v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def samples(kind, n, seed):
    """(raw little-endian bytes, the defined fp32 value of every sample)."""
    rng = np.random.default_rng(seed)
    if kind == "u8":
        v = rng.integers(0, 256, n).astype(np.uint8)
        v[:2] = (0, 255)
        return v.tobytes(), ((v.astype(np.float64) - 128) / 128).astype(np.float32)
    if kind in ("s16", "s24", "s32"):
        bits = int(kind[1:])
        v = rng.integers(-2 ** (bits - 1), 2 ** (bits - 1), n, dtype=np.int64)
        v[:2] = (-2 ** (bits - 1), 2 ** (bits - 1) - 1)
        raw = s24_bytes(v) if bits == 24 else v.astype(f"<i{bits // 8}").tobytes()
        return raw, (v.astype(np.float64) / 2.0 ** (bits - 1)).astype(np.float32)
    v = rng.normal(0, 0.3, n).astype("<f4" if kind == "f32" else "<f8")
    return v.tobytes(), v.astype(np.float32)


FORMATS = {"u8": (1, 8), "s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "f32": (3, 32), "f64": (3, 64)}


@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("kind", ["u8", "s16", "s24", "s32", "f32", "f64", "ext-s24", "ext-f32", "ext-s24in32"])
def test_formats_and_channels(tmp_path, kind, ch):
    ext = kind.startswith("ext-")
    base = kind[4:] if ext else kind
    valid = None
    if base == "s24in32":  # 24 valid bits in a 32-bit container: the container width scales
        base, valid = "s32", 24
    tag, bits = FORMATS[base]
    n = 257
    raw, want = samples(base, n * ch, seed=bits + ch)
    p = write(tmp_path / "a.wav", riff(chunk(b"fmt ", fmt_chunk(tag, ch, 22050, bits, ext, valid)), chunk(b"data", raw)))
    got, sr = read_wav(p)
    assert sr == 22050 and got.dtype == np.float32 and got.shape == (n,)
    if ch == 1:
        assert np.array_equal(got, want)
    else:
        ref = np.mean(want.reshape(n, ch), axis=1, dtype=np.float32)
        assert np.abs(got.astype(np.float64) - ref).max() <= ch * 2.0 ** -24


def test_container_quirks(tmp_path):
    raw, want = samples("s16", 100, 3)
    fmt = chunk(b"fmt ", fmt_chunk(1, 1, 16000, 16))
    lst = chunk(b"LIST", b"INFOISFT\x03\0\0\0ab\0")  # 15 bytes: odd, padded
    assert len(lst) == 8 + 16
    for name, blob in {
        "list_first": riff(lst, fmt, chunk(b"fact", struct.pack("<I", 100)), chunk(b"data", raw)),
        "list_between": riff(fmt, lst, chunk(b"bext", b"x" * 7), chunk(b"data", raw), chunk(b"LIST", b"tail")),
        "streamed": riff(fmt, chunk(b"data", raw, size=0xFFFFFFFF)),
        "streamed0": riff(fmt, chunk(b"data", raw, size=0)),
    }.items():
        got, sr = read_wav(write(tmp_path / (name + ".wav"), blob))
        assert sr == 16000 and np.array_equal(got, want), name
    # a stereo file cut in the middle of its 31st frame, the data size still claiming 50
    raw2, want2 = samples("s16", 100, 4)
    fmt_stereo = chunk(b"fmt ", fmt_chunk(1, 2, 16000, 16))
    blob = riff(fmt_stereo, chunk(b"data", raw2))
    cut = blob[:12 + len(fmt_stereo) + 8 + 30 * 4 + 3]
    got, _ = read_wav(write(tmp_path / "cut.wav", cut))
    assert np.array_equal(got, want2[:60].reshape(30, 2).mean(1))


def test_errors(tmp_path):
    raw, _ = samples("s16", 16, 5)
    fmt = chunk(b"fmt ", fmt_chunk(1, 1, 16000, 16))
    cases = {
        "mulaw": (riff(chunk(b"fmt ", fmt_chunk(7, 1, 8000, 8)), chunk(b"data", raw)), "0x0007"),
        "adpcm": (riff(chunk(b"fmt ", fmt_chunk(2, 1, 8000, 4)), chunk(b"data", raw)), "0x0002"),
        "avi": (riff(fmt, chunk(b"data", raw), form=b"AVI "), "AVI "),
        "id3": (b"ID3\x04\0\0\0\0\0\x21" + b"\0" * 64, "compressed audio is out of scope"),
        "ogg": (b"OggS\0\x02" + b"\0" * 64, "compressed audio is out of scope"),
        "m4a": (b"\0\0\0\x20ftypM4A " + b"\0" * 64, "compressed audio is out of scope"),
        "fmt_after_data": (riff(chunk(b"data", raw), fmt), "fmt"),
        "no_fmt": (riff(chunk(b"LIST", b"abcd")), "fmt"),
        "no_data": (riff(fmt), "data"),
        "zero_channels": (riff(chunk(b"fmt ", fmt_chunk(1, 0, 16000, 16)), chunk(b"data", raw)), "zero channels"),
        "zero_rate": (riff(chunk(b"fmt ", fmt_chunk(1, 1, 0, 16)), chunk(b"data", raw)), "zero sample rate"),
        "s12": (riff(chunk(b"fmt ", fmt_chunk(1, 1, 16000, 12)), chunk(b"data", raw)), "12-bit"),
        "f16": (riff(chunk(b"fmt ", fmt_chunk(3, 1, 16000, 16)), chunk(b"data", raw)), "16-bit"),
        "empty": (b"", "RIFF"),
    }
    for name, (blob, needle) in cases.items():
        p = write(tmp_path / (name + ".wav"), blob)
        with pytest.raises(ValueError) as e:
            read_wav(p)
        assert p in str(e.value) and needle in str(e.value), (name, str(e.value))
        with pytest.raises(ValueError):
            load_wav(p)


def test_bit_identical_to_the_16_bit_reader(tmp_path, monkeypatch):
    """Every file the previous reader accepted (s16, 16 kHz, 1 or 2 channels) decodes to
    the same bits: int16 / 32768 in fp32, then .reshape(-1, ch).mean(1) -- on the host
    alone, the device resampler is never reached."""
    def no_device(*a, **k):
        raise AssertionError("a 16 kHz file must not reach the device resampler")

    monkeypatch.setattr(A.ops, "resample", no_device)
    for ch in (1, 2):
        x = np.random.default_rng(ch).integers(-32768, 32768, 4000 * ch).astype("<i2")
        p = write(tmp_path / f"c{ch}.wav", riff(chunk(b"fmt ", fmt_chunk(1, ch, 16000, 16)), chunk(b"data", x.tobytes())))
        want = x.astype(np.float32) / 32768.0
        if ch > 1:
            want = want.reshape(-1, ch).mean(1)
        got = load_wav(p)
        assert got.dtype == want.dtype and np.array_equal(got, want)


def test_previously_refused_inputs_load(tmp_path):
    """16 kHz float and 24-bit files: the 16-bit reader raised NotImplementedError."""
    for kind in ("f32", "s24"):
        tag, bits = FORMATS[kind]
        raw, want = samples(kind, 500, 9)
        p = write(tmp_path / f"{kind}.wav", riff(chunk(b"fmt ", fmt_chunk(tag, 1, 16000, bits)), chunk(b"data", raw)))
        assert np.array_equal(load_wav(p), want)
        assert np.array_equal(A.read_audio(p).numpy(), want)


def test_rate_conversion_needs_the_device(tmp_path, monkeypatch):
    """Without a HIP device a file at another rate is refused: there is no CPU resampler."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    raw, _ = samples("s16", 500, 10)
    p = write(tmp_path / "a.wav", riff(chunk(b"fmt ", fmt_chunk(1, 1, 44100, 16)), chunk(b"data", raw)))
    with pytest.raises(RuntimeError, match="HIP device"):
        load_wav(p)


# ---------------------------------------------------------------- filter design


def test_resample_taps_shapes_and_symmetry():
    want = {44100: (160, 441), 48000: (1, 3), 22050: (320, 441), 8000: (2, 1), 16000: (1, 1)}
    for sr, (L, M) in want.items():
        l, m, half, taps = resample_taps(sr, 16000)
        fc = min(1.0, L / M) * 0.95
        assert (l, m) == (L, M) and half == math.ceil(32 / fc)
        h = resample_taps64(sr, 16000)
        T = 2 * half + 1
        assert taps.shape == h.shape == (L, T) and taps.dtype == np.float32 and h.dtype == np.float64
        assert np.array_equal(taps, h.astype(np.float32))
        assert np.abs(h.sum(1) - 1).max() <= 1e-12
        # h[p, j] == h[(L - p) % L, -j + (p != 0)], j in [-half, half] at column j + half
        for p in range(L):
            q, s = (L - p) % L, int(p != 0)
            j = np.arange(-half + s, half + 1)
            assert np.abs(h[p, j + half] - h[q, -j + s + half]).max() <= 1e-12, (sr, p)
    assert resample_taps(44100, 16000)[3] is resample_taps(44100, 16000)[3]  # cached


def resample_f64(x, L, M, half, h):
    """The definition, in float64: y[n] = sum_j h[p, j] x[base + j], base = n M // L,
    p = n M % L, x zero outside [0, n_in), n_out = ceil(n_in L / M)."""
    n_in = len(x)
    n_out = -(-n_in * L // M)
    xp = np.concatenate([np.zeros(half), np.asarray(x, dtype=np.float64), np.zeros(half + M + 1)])
    t = np.arange(n_out, dtype=np.int64) * M
    base, p = t // L, t % L
    y = np.zeros(n_out)
    for j in range(2 * half + 1):
        y += h[p, j] * xp[base + j]
    return y


@functools.lru_cache(maxsize=None)
def tone_response(sr, f):
    """Steady-state part of a unit sine at f Hz resampled sr -> 16 kHz, and its times."""
    L, M, half, _ = resample_taps(sr, 16000)
    n_in = int(0.25 * sr)
    x = np.sin(2 * np.pi * f * np.arange(n_in) / sr)
    y = resample_f64(x, L, M, half, resample_taps64(sr, 16000))
    assert len(y) == math.ceil(n_in * L / M)
    edge = math.ceil(half * L / M) + 2
    return y[edge:-edge], np.arange(len(y))[edge:-edge] / 16000.0


def test_design_figures():
    worst = {"down_pass": 0.0, "stop": 0.0, "up_pass": 0.0}
    for sr in (44100, 48000, 32000, 24000, 22050):
        for f in (100, 1000, 3000, 6000):
            y, t = tone_response(sr, f)
            assert len(y) > 1000
            worst["down_pass"] = max(worst["down_pass"], np.abs(y - np.sin(2 * np.pi * f * t)).max())
        for f in (8600, 9000, 10000, 15000, 20000):
            if f < sr / 2:
                worst["stop"] = max(worst["stop"], np.abs(tone_response(sr, f)[0]).max())
    for sr in (8000, 11025):
        for f in (100, 1000, 3000):
            y, t = tone_response(sr, f)
            worst["up_pass"] = max(worst["up_pass"], np.abs(y - np.sin(2 * np.pi * f * t)).max())
    print("resampler design figures:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert worst["down_pass"] <= 3e-5 and worst["up_pass"] <= 3e-5
    assert worst["stop"] <= 5e-5
