"""Device Motion-JPEG decoder on MI355X (csrc/ls_video_dec.hip) against the CPU restatement
(tests/mjpeg_dec_cpu.py, pinned to libjpeg by tests/test_mjpeg_decode_host.py): decoded
pixels equal bit for bit -- the arithmetic is integer, so there is no tolerance -- then the
status path for bad streams, argument validation, the AVI reader and __call__ reading an
.avi on the device.

Shapes are the encoder tests' (tests/test_gpu_mjpeg.py), for the same reasons: a single
block; partial MCUs both ways with odd chroma sizes; several frames; more MCUs in a row
than a wave has lanes; 12 restart segments (the RSTm index wraps past 7); the same frame
at Ri = 1 (120 segments: two entropy waves).  A frame gets up to 16 entropy waves, so a
lane loops over segments only past 1024 of them: the greyscale 80 x 1043 frame at Ri = 1
(1310 segments) is there for that loop."""
import functools
import io

import numpy as np
import pytest
import torch

import mjpeg_cpu as mj
import mjpeg_dec_cpu as dec
from latentsync_amd import _lib, ops, video
from latentsync_amd.audio import Audio2Feature
from latentsync_amd.config import TINY_MODEL
from latentsync_amd.pipeline import LipsyncPipeline, read_video_frames
from latentsync_amd.scheduler import DDIMScheduler
from latentsync_amd.unet import UNet3DConditionModel
from latentsync_amd.vae import AutoencoderKL
from test_avi_mjpeg import _bi_rgb_avi
from test_gpu_mjpeg import content
from test_gpu_resample import SCHED, _align, write_wav

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def own_jpeg(kind, i, H, W, quality, ri, dri=True):
    """Frame i of content(kind, ...) as this project's encoder writes it (4:2:0, Annex K
    tables, restart interval ri); dri=False: one segment and no DRI segment at all."""
    jpg = mj.encode_jpeg(content(kind, 3, H, W)[i], quality, ri if dri else 65535)
    if not dri:
        at = jpg.index(b"\xff\xdd\x00\x04")
        jpg = jpg[:at] + jpg[at + 6:]
        assert video.parse_jpeg(jpg).Ri == 0
    return jpg


@functools.lru_cache(maxsize=None)
def pillow_jpeg(kind, i, H, W, sampling, quality, optimize=False, restart=0):
    Image = pytest.importorskip("PIL.Image")
    im = Image.fromarray(content(kind, 3, H, W)[i])
    kw = dict(quality=quality, optimize=optimize)
    if sampling == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = sampling
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def check_equal(jpgs):
    want = np.stack([dec.decode(j) for j in jpgs])
    got = video.decode_frames(jpgs, "cuda")
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == want.shape
    for i in range(len(jpgs)):
        assert torch.equal(got[i].cpu(), torch.from_numpy(want[i])), f"frame {i} differs"
    return got


SHAPES = [(1, 8, 8), (2, 17, 33), (3, 40, 56), (2, 24, 16 * 65 + 3), (1, 80, 16 * 23 + 1)]


@pytest.mark.parametrize("quality", [1, 95])
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_smooth_frames_equal(gpu, n, H, W, quality):
    """Files as this project's encoder writes them (Ri = 10), and the same frames without DRI."""
    check_equal([own_jpeg("smooth", i, H, W, quality, 10) for i in range(n)])
    check_equal([own_jpeg("smooth", i, H, W, quality, 10, dri=False) for i in range(n)])


def test_restart_segments_wrap_and_exceed_the_lanes(gpu):
    H, W = 80, 16 * 23 + 1
    j10, j1 = own_jpeg("smooth", 0, H, W, 95, 10), own_jpeg("smooth", 0, H, W, 95, 1)
    assert video.parse_jpeg(j10).n_segments == 12 and j10.count(b"\xff\xd0") >= 2  # RST0 twice
    assert video.parse_jpeg(j1).n_segments == 120  # more than one wave of lanes
    check_equal([j10])
    check_equal([j1])
    grey = pillow_jpeg("smooth", 0, 80, 16 * 65 + 3, "grey", 90, restart=1)
    assert video.parse_jpeg(grey).n_segments == 10 * 131 > 1024  # a lane takes a second segment
    check_equal([grey])


@pytest.mark.parametrize("kind,quality", [("black", 95), ("checker", 100), ("last", 1), ("noise", 100), ("noise", 1),
                                          ("checker", 50), ("last", 100)])
def test_content_cases_equal(gpu, kind, quality):
    """Black: every block is EOB only; last: coefficient 63 and no EOB; noise at quality 1
    and 100: ZRL runs and 16-bit codes, stuffed 0xFF bytes."""
    for n, H, W in ((2, 32, 48), (1, 24, 16 * 65 + 3)):
        check_equal([own_jpeg(kind, i, H, W, quality, 10) for i in range(n)])
    check_equal([own_jpeg(kind, 0, 32, 48, quality, 10, dri=False)])


@pytest.mark.parametrize("sampling", ["4:4:4", "4:2:2", "4:2:0", "grey"])
def test_samplings_equal(gpu, sampling):
    """Pillow's files: every sampling, with and without DRI, standard and optimised tables,
    odd sizes (partial MCUs, odd chroma planes) and planes of 2 columns (no fancy filter)."""
    for H, W in ((17, 33), (40, 56), (3, 3), (9, 4)):
        for kind, quality in (("smooth", 90), ("noise", 1), ("noise", 100)):
            check_equal([pillow_jpeg(kind, 0, H, W, sampling, quality, restart=r) for r in (0, 3)])
            check_equal([pillow_jpeg(kind, 0, H, W, sampling, quality, optimize=True)])


def test_tables_that_differ_from_frame_to_frame(gpu):
    """Optimised tables: one set per frame in one call, deduplicated where frames repeat."""
    jpgs = [pillow_jpeg(k, i, 40, 56, "4:2:0", q, optimize=True) for k, i, q in
            (("smooth", 0, 90), ("noise", 1, 60), ("smooth", 2, 30), ("smooth", 0, 90), ("checker", 0, 75))]
    _, desc, quant, huff, _, _, _ = video.pack_frames(jpgs)
    assert len(huff) > 8 and len(quant) > 4 and (desc[0, 4:7] == desc[3, 4:7]).all() and (desc[0, 5] != desc[1, 5])
    check_equal(jpgs)


def test_one_call_mixing_all_samplings(gpu):
    jpgs = [pillow_jpeg("smooth", 0, 17, 33, s, 85, restart=r) for s, r in
            (("4:2:0", 0), ("grey", 2), ("4:4:4", 0), ("4:2:2", 1), ("4:2:0", 1))] + [own_jpeg("noise", 0, 17, 33, 100, 10)]
    assert [video.parse_jpeg(j).mode for j in jpgs] == [3, 0, 1, 2, 3, 3]
    check_equal(jpgs)


def test_view_at_an_odd_byte_offset(gpu):
    """The scans start at byte 1 of their allocation; rows of 3 * 33 = 99 bytes put every
    second output row at an odd address too."""
    jpgs = [own_jpeg("noise", i, 17, 33, 100, 10) for i in range(2)]
    scans, desc, quant, huff, max_seg, H, W = video.pack_frames(jpgs)
    buf = torch.from_numpy(np.frombuffer(b"\xff" + scans, np.uint8).copy()).cuda()
    up = lambda a: torch.from_numpy(a).cuda()
    got, status = ops.mjpeg_decode(buf[1:], up(desc), H, W, up(quant), up(huff), max_seg)
    assert status.tolist() == [0, 0] and status.dtype == torch.int32
    assert torch.equal(got.cpu(), torch.from_numpy(np.stack([dec.decode(j) for j in jpgs])))


def test_more_frames_than_one_batch(gpu):
    """1100 small frames pass the 1024 frames of one batch: the second batch reuses the
    workspace and lands behind the first in the output."""
    jpgs = [own_jpeg("smooth", i, 40, 56, 95, 10) for i in range(3)]
    many = [jpgs[i % 3] for i in range(1100)]
    got = video.decode_frames(many, "cuda")
    want = torch.from_numpy(np.stack([dec.decode(j) for j in jpgs])).cuda()
    assert torch.equal(got, want[torch.arange(1100, device="cuda") % 3])


# ---------------------------------------------------------------- round trips

def test_encoder_round_trip_equals_pillows_decode(gpu):
    Image = pytest.importorskip("PIL.Image")
    frames = content("smooth", 3, 40, 56)
    jpgs = video.encode_frames(torch.from_numpy(frames).cuda(), 95)
    got = video.decode_frames(jpgs, "cuda").cpu().numpy()
    for g, j in zip(got, jpgs):
        assert np.array_equal(g, np.asarray(Image.open(io.BytesIO(j)).convert("RGB")))


def test_read_avi_device_equals_read_avi(gpu, tmp_path):
    pytest.importorskip("PIL.Image")
    frames = content("smooth", 3, 40, 56)
    path = str(tmp_path / "clip.avi")
    audio = np.random.default_rng(3).uniform(-0.5, 0.5, 1920)
    video.write_video(path, torch.from_numpy(frames).cuda(), 25, audio, 16000, quality=90)
    want, fps, a, sr = video.read_avi(path)
    got, fps_d, a_d, sr_d = video.read_avi_device(path, "cuda")
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want))
    assert (fps_d, sr_d) == (fps, sr) == (25, 16000) and np.array_equal(a_d, a)
    via = read_video_frames(path, 25, "cuda")
    assert torch.is_tensor(via) and via.is_cuda and torch.equal(via, got)
    raw = np.random.default_rng(5).integers(0, 256, (3, 5, 6, 3), dtype=np.uint8)  # 18-byte rows padded to 20
    p = tmp_path / "raw.avi"
    p.write_bytes(_bi_rgb_avi(raw))
    got, fps, a, sr = video.read_avi_device(str(p), "cuda")
    assert got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(raw)) and fps == 25 and a is None and sr is None
    assert torch.equal(read_video_frames(str(p), 25, "cuda").cpu(), torch.from_numpy(video.read_avi(str(p))[0]))


def test_avi_outside_the_subset_takes_the_host_route(gpu, tmp_path):
    pytest.importorskip("PIL.Image")
    jpgs = [pillow_jpeg("smooth", i, 40, 56, "4:2:0", 90) for i in range(2)]
    prog = io.BytesIO()
    from PIL import Image
    Image.fromarray(content("smooth", 3, 40, 56)[2]).save(prog, "JPEG", quality=90, progressive=True)
    path = str(tmp_path / "mixed.avi")
    video.write_avi(path, jpgs + [prog.getvalue()], 25)
    got = read_video_frames(path, 25, "cuda")
    assert isinstance(got, np.ndarray) and np.array_equal(got, video.read_avi(path)[0])
    with pytest.raises(ValueError, match="mixed.avi: frame 2: progressive"):
        video.read_avi_device(path, "cuda")
    other = str(tmp_path / "size.avi")
    video.write_avi(other, [jpgs[0], pillow_jpeg("smooth", 0, 17, 33, "4:2:0", 90)], 25)
    with pytest.raises(ValueError, match=r"size.avi: frame 1 is 33x17, the header says 56x40"):
        video.read_avi_device(other, "cuda")


# ---------------------------------------------------------------- bad streams (the status path, once each)

def _bad_avi(tmp_path, name, bad):
    good = own_jpeg("smooth", 0, 40, 56, 95, 10, dri=False)
    path = str(tmp_path / name)
    video.write_avi(path, [good, bad, good], 25)
    return path, good


def test_scan_cut_in_half(gpu, tmp_path):
    good = own_jpeg("smooth", 1, 40, 56, 95, 10, dri=False)
    info = video.parse_jpeg(good)
    bad = good[:info.scan_start + (len(good) - info.scan_start) // 2]
    assert dec.decode_status(bad)[1] == dec.ST_SHORT
    path, good = _bad_avi(tmp_path, "cut.avi", bad)
    with pytest.raises(ValueError, match=r"cut.avi: frame 1 is not a decodable JPEG \(.*ends before the last MCU"):
        video.read_avi_device(path, "cuda")
    frames, status = video.decode_frames_status([good, bad, good], "cuda")
    assert status == [0, dec.ST_SHORT, 0]
    want = torch.from_numpy(dec.decode(good).copy())
    assert torch.equal(frames[0].cpu(), want) and torch.equal(frames[2].cpu(), want)
    # with restart markers the cut shows as missing markers
    withri = own_jpeg("smooth", 1, 40, 56, 95, 1)
    half = withri[:video.parse_jpeg(withri).scan_start + 150]
    assert dec.decode_status(half)[1] == dec.ST_MARKERS
    assert video.decode_frames_status([good, half], "cuda")[1] == [0, dec.ST_MARKERS]


def test_scan_that_never_forms_a_code(gpu, tmp_path):
    good = own_jpeg("smooth", 1, 40, 56, 95, 10, dri=False)
    bad = good[:video.parse_jpeg(good).scan_start] + b"\xff\x00" * 300
    assert dec.decode_status(bad)[1] == dec.ST_CODE
    path, good = _bad_avi(tmp_path, "ones.avi", bad)
    with pytest.raises(ValueError, match=r"ones.avi: frame 1 is not a decodable JPEG \(.*longer than 16 bits"):
        video.read_avi_device(path, "cuda")
    with pytest.raises(ValueError, match=r"^frame 1 is not a decodable JPEG"):
        video.decode_frames([good, bad, good], "cuda")
    frames, status = video.decode_frames_status([good, bad, good], "cuda")
    assert status == [0, dec.ST_CODE, 0]
    want = torch.from_numpy(dec.decode(good).copy())
    assert torch.equal(frames[0].cpu(), want) and torch.equal(frames[2].cpu(), want)


def test_validation(gpu):
    lib = _lib.load()
    scans, desc, quant, huff, max_seg, H, W = video.pack_frames([own_jpeg("smooth", 0, 40, 56, 95, 10)])
    up = lambda a: torch.from_numpy(a).cuda()
    data, d, q, h = up(np.frombuffer(scans, np.uint8).copy()), up(desc), up(quant), up(huff)
    with pytest.raises(ValueError, match="frames must be"):
        ops.mjpeg_decode(data, d.int(), H, W, q, h)
    with pytest.raises(ValueError, match="data must be"):
        ops.mjpeg_decode(data.cpu(), d, H, W, q, h)
    with pytest.raises(ValueError, match="huff must be"):
        ops.mjpeg_decode(data, d, H, W, q, h[:, :200].contiguous())
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.mjpeg_decode(data, d, H, W, q, h, workspace=torch.empty(1024, dtype=torch.uint8, device="cuda"))
    for bad_h, bad_w in ((2, 56), (40, 2), (65536, 56), (40, 65536)):
        assert lib.ls_mjpeg_decode_workspace_bytes(1, bad_h, bad_w) == 0
        with pytest.raises(RuntimeError, match="ls_mjpeg_decode.*3 <= H, W <= 65535"):
            ops.mjpeg_decode(data, d, bad_h, bad_w, q, h)
    assert lib.ls_mjpeg_decode_workspace_bytes(0, 40, 56) == 0
    need = lib.ls_mjpeg_decode_workspace_bytes(1, 40, 56)
    assert 0 < need == lib.ls_mjpeg_decode_workspace_bytes(1, 33, 49) < lib.ls_mjpeg_decode_workspace_bytes(2, 40, 56)
    # the workspace stops growing with n: one batch of a fixed budget
    assert lib.ls_mjpeg_decode_workspace_bytes(10 ** 6, 1080, 1920) == lib.ls_mjpeg_decode_workspace_bytes(10 ** 5, 1080, 1920)
    assert lib.ls_mjpeg_decode_workspace_bytes(10 ** 6, 1080, 1920) <= (512 << 20) + 256
    # pointers are never dereferenced: validation fails first
    args = lambda **kw: [kw.get(k, v) for k, v in (("data", 16), ("nb", 64), ("frames", 16), ("n", 1), ("H", 40), ("W", 56),
                                                   ("quant", 16), ("nq", 1), ("huff", 16), ("nh", 1), ("segs", 1),
                                                   ("out", 16), ("status", 16), ("ws", 16), ("wsb", 1 << 30),
                                                   ("stream", None))]
    for kw in (dict(data=None), dict(frames=None), dict(quant=None), dict(huff=None), dict(out=None), dict(status=None),
               dict(n=0), dict(H=2), dict(W=65536), dict(nb=-1), dict(nq=0), dict(nh=0)):
        assert lib.ls_mjpeg_decode(*args(**kw)) == 1, kw
    assert b"ls_mjpeg_decode" in lib.ls_last_error()
    assert lib.ls_mjpeg_decode(*args(ws=None, wsb=0)) == 3 and lib.ls_mjpeg_decode(*args(wsb=need - 1)) == 3


# ---------------------------------------------------------------- __call__

Fr, Rr, STEPS = 8, 64, 2


def test_call_reads_an_avi_on_the_device(gpu, tmp_path, monkeypatch):
    """The __call__ recipe of test_gpu_mjpeg.py::test_call_writes_a_playable_avi: with
    video_path = x.avi (decoded on the device) the written .npz frames are those of the run
    on the .npy of read_avi(x.avi)'s frames."""
    pytest.importorskip("PIL.Image")
    unet = UNet3DConditionModel(**TINY_MODEL).init_weights(9).to("cuda").eval()
    vae = AutoencoderKL(block_out_channels=(32, 64, 64, 64)).init_weights(10).to("cuda")
    H, W, fh, fw, N = 120, 160, 56, 48, 24
    pipe = LipsyncPipeline(vae, Audio2Feature.random(2, device="cuda"), unet, DDIMScheduler(**SCHED))
    rng = np.random.default_rng(6)
    write_wav(tmp_path / "audio.wav", rng.normal(0, 0.1, (int(0.56 * 44100), 2)).clip(-1, 0.999), 44100, "s16")
    low = torch.rand((N, 3, 8, 8), generator=torch.Generator().manual_seed(61))
    faces = (torch.nn.functional.interpolate(low, size=(Rr, Rr), mode="bicubic") * 255).round().clamp(0, 255)
    mats = [_align(80 + rng.uniform(-5, 5), 60 + rng.uniform(-5, 5), rng.uniform(0.8, 1.2),
                   rng.uniform(-0.15, 0.15), fh, fw) for _ in range(N)]
    torch.save({"faces": faces.to(torch.uint8), "boxes": [[0, 0, fw, fh]] * N, "affine_matrices": mats},
               tmp_path / "data.pth")
    avi = str(tmp_path / "video.avi")
    video.write_video(avi, torch.from_numpy(mj.smooth_frames(N, H, W, 77)).cuda(), 25, quality=95)
    np.save(tmp_path / "video.npy", video.read_avi(avi)[0])
    calls = []
    real = video.read_avi_device
    monkeypatch.setattr(video, "read_avi_device", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    kw = dict(audio_path=str(tmp_path / "audio.wav"), num_frames=Fr, num_inference_steps=STEPS, guidance_scale=1.0,
              height=Rr, width=Rr, data_path=str(tmp_path / "data.pth"), mask_image_path=None)
    for name, path in (("a", avi), ("b", str(tmp_path / "video.npy"))):
        pipe(video_path=path, video_out_path=str(tmp_path / f"{name}.npz"),
             generator=torch.Generator(device="cuda").manual_seed(1247), **kw)
    assert calls == [avi]  # the .avi went through the device reader
    a, b = np.load(tmp_path / "a.npz"), np.load(tmp_path / "b.npz")
    assert a["frames"].shape == b["frames"].shape and a["frames"].shape[1:] == (H, W, 3)
    assert np.array_equal(a["frames"], b["frames"]) and np.array_equal(a["audio"], b["audio"])
    pipe.close()
