"""The kernels of csrc/ls_synceval.hip, each against its definition: ls_mfcc against the float64
oracle, ls_conv_general per element against a float64 convolution (tests/parity.py bounds,
guard bands, NaN-framed inputs), ls_maxpool2d exactly, ls_sync_offset against float64 and on
planted shifts, ls_crop_track exactly against the CPU restatement of cv2.resize."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity as P
import synceval_ref as R
from latentsync_amd import _lib, ops, synceval
from latentsync_amd.packing import pack_weight_general

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nan_framed(x):
    """x (n, H, W, C) as a view of a NaN-filled device buffer: NaN pixel rows before and after
    all images and a pitch of C + 8."""
    n, H, W, C = x.shape
    g = P.guarded((n, H, W, C), pitch=C + 8, pad_rows=2 * W + 2, dtype=BF, device=DEV)
    g.view.copy_(x.to(BF).to(DEV))
    return g.view


# ---------------------------------------------------------------- ls_mfcc
@pytest.mark.parametrize("n", (400, 401, 560, 561, 8000))
def test_mfcc_matches_oracle(gpu, n):
    """|got - oracle| <= 2^-9 max(1, |oracle|): the only consumer stores bf16.  The oracle may
    mark at most 1 % of the elements as too ill-conditioned to judge; on this signal it marks
    none (tests/test_synceval_host.py checks that on the CPU)."""
    x = R.mfcc_test_signal(n)
    ref, ok = R.mfcc_oracle(x)
    assert (~ok).mean() <= 0.01
    g = P.guarded((13, ref.shape[1]), dtype=torch.float32, device=DEV)
    filt = torch.from_numpy(synceval.mfcc_filters()).to(DEV)
    xd = torch.from_numpy(x).float().to(DEV)
    snap = P.snapshot(xd)
    # the guarded view of an unpitched (13, T) array is contiguous
    ops.mfcc(xd, filt, out=g.view)
    torch.cuda.synchronize()
    got = g.view.double().cpu().numpy()
    bound = 2.0 ** -9 * np.maximum(1.0, np.abs(ref))
    ratio = np.abs(got - ref) / bound
    print(f"n {n}: T {ref.shape[1]}, worst err / bound {ratio[ok].max():.3f}, skipped {(~ok).sum()}")
    assert np.isfinite(got).all() and (ratio[ok] <= 1.0).all(), np.argwhere(~(ratio <= 1.0) & ok)[:8]
    P.assert_guard_intact(g, "mfcc")
    P.assert_unchanged(xd, snap, "audio")


def test_mfcc_silence_and_invalid(gpu):
    lib = _lib.load()
    filt = torch.from_numpy(synceval.mfcc_filters()).to(DEV)
    ref, _ = R.mfcc_oracle(np.zeros(800))
    got = ops.mfcc(torch.zeros(800, device=DEV), filt).double().cpu().numpy()
    assert (np.abs(got - ref) <= 2.0 ** -9 * np.maximum(1.0, np.abs(ref))).all()  # the epsilon floor
    g = P.guarded((13, 4), dtype=torch.float32, device=DEV)
    x = torch.zeros(800, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.ls_mfcc(x.data_ptr(), 0, filt.data_ptr(), g.view.data_ptr(), s) == 1
    assert lib.ls_mfcc(None, 800, filt.data_ptr(), g.view.data_ptr(), s) == 1
    assert lib.ls_mfcc(x.data_ptr(), 800, None, g.view.data_ptr(), s) == 1
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view).all())


# ---------------------------------------------------------------- ls_conv_general
# (name, window, stride, pad, T, H, W, live input channels, Cin, N, relu, fp32 output)
CONV_CASES = (
    ("c577_s2_cin3", (5, 7, 7), (2, 2), (0, 0), 6, 15, 15, 3, 8, 96, True, False),      # K 1960 -> 1984; 2 steps
    ("c155_s2_p1", (1, 5, 5), (2, 2), (1, 1), 2, 8, 8, 96, 96, 256, True, False),       # K 2400 -> 2432: split K
    ("c133_p1", (1, 3, 3), (1, 1), (1, 1), 1, 11, 9, 192, 192, 384, False, False),      # K 1728, M 99: a partial tile
    ("c133_p1_relu", (1, 3, 3), (1, 1), (1, 1), 1, 11, 9, 192, 192, 384, True, False),
    ("c166_valid_1step", (1, 6, 6), (1, 1), (0, 0), 1, 6, 6, 256, 256, 512, True, False),  # K 9216, M 1
    ("c166_valid_3steps", (1, 6, 6), (1, 1), (0, 0), 3, 6, 6, 256, 256, 512, True, False),  # M 3
    ("c154_valid", (1, 5, 4), (1, 1), (0, 0), 2, 5, 4, 64, 64, 24, False, False),       # N 24: two channel tiles
    ("linear512_f32", (1, 1, 1), (1, 1), (0, 0), 7, 1, 1, 512, 512, 1024, False, True),
    ("linear512_relu", (1, 1, 1), (1, 1), (0, 0), 3, 1, 1, 512, 512, 512, True, False),
    ("linear512_n10_f32", (1, 1, 1), (1, 1), (0, 0), 2, 1, 1, 512, 512, 10, False, True),  # one channel tile, N % 4
)


def make_conv(case):
    name, win, stride, pad, T, H, W, live, Cin, N, relu, f32 = case
    seed = sum(map(ord, name))
    x = torch.zeros(T, H, W, Cin)
    x[..., :live] = P.bf16_round(rnd(T, H, W, live, seed=seed))
    kt, kh, kw = win
    w = P.bf16_round(rnd(N, live, kt, kh, kw, seed=seed + 1, scale=1 / math.sqrt(kt * kh * kw * live)))
    b = rnd(N, seed=seed + 2, scale=0.1)
    x5 = P.f64(x[..., :live]).permute(3, 0, 1, 2)[None]
    conv = lambda a, ww, bb: F.conv3d(a, ww, bb, stride=(1,) + stride, padding=(0,) + pad)[0].permute(1, 2, 3, 0)
    ref = conv(x5, P.f64(w), P.f64(b))
    mag = conv(x5.abs(), P.f64(w).abs(), P.f64(b).abs())
    k_terms = kt * kh * kw * live
    out_dtype = torch.float32 if f32 else BF
    if relu:  # ReLU is 1-Lipschitz: the pre-activation bound carries over, then the one rounding of the result
        bound = P.gemm_bound(ref, mag, k_terms, None) + P._u_out(out_dtype) * ref.clamp_min(0) * P.SLACK
        ref = ref.clamp_min(0)
    else:
        bound = P.gemm_bound(ref, mag, k_terms, out_dtype)
    pw = ops.PackedGeneral(pack_weight_general(w, Cin).to(BF).to(DEV), b.float().to(DEV), Cin, win)
    return x, pw, ref, bound


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_general_parity(gpu, case):
    name, win, stride, pad, T, H, W, live, Cin, N, relu, f32 = case
    x, pw, ref, bound = make_conv(case)
    xd = nan_framed(x)
    snap = P.snapshot(xd)
    To, Ho, Wo = ref.shape[:3]
    assert (Ho, Wo) == ops.conv_out_hw(H, W, win, stride, pad) and To == T - win[0] + 1
    dt = torch.float32 if f32 else BF
    g = P.guarded((To, Ho, Wo, N), pitch=(N + 7) // 8 * 8 + 8, dtype=dt, device=DEV)
    ops.conv_general(xd, pw, stride, pad, relu=relu, out=g.view, out_f32=f32)
    torch.cuda.synchronize()
    worst = P.assert_elementwise(g.view, ref, bound, where=dict(rows=16, cols=16), name=name)
    P.assert_guard_intact(g, name)
    P.assert_unchanged(xd, snap, name + " input")
    print(f"{name}: K {pw.K} M {To * Ho * Wo} worst err/bound {worst:.3f}")
    # step independence: every step computed alone equals the steps computed together, bit for bit
    if To > 1:
        xc = x.to(BF).to(DEV)
        for t in range(To):
            one = ops.conv_general(xc[t:t + win[0]].contiguous(), pw, stride, pad, relu=relu, out_f32=f32)
            torch.cuda.synchronize()
            assert torch.equal(one[0], g.view[t]), (name, t)


def test_conv_general_invalid_arguments_launch_nothing(gpu):
    lib = _lib.load()
    Cin, N, T, H, W = 16, 32, 3, 8, 8
    x = torch.zeros((T, H, W, Cin), dtype=BF, device=DEV)
    w = torch.zeros((N, 1024), dtype=BF, device=DEV)
    g = P.guarded((T, H, W, N), pitch=N + 8, dtype=BF, device=DEV)
    base = dict(x=x.data_ptr(), ldx=Cin, T=T, H=H, W=W, cin=Cin, w=w.data_ptr(), K=192, kt=1, kh=3, kw=3, sh=1, sw=1,
                ph=1, pw=1, act=0, y=g.view.data_ptr(), ldy=N + 8, f32=0)

    def call(**kw):
        a = dict(base, **kw)
        return lib.ls_conv_general(a["x"], a["ldx"], a["T"], a["H"], a["W"], a["cin"], a["w"], a["K"], N, None, a["kt"],
                                   a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["act"], a["y"], a["ldy"],
                                   a["f32"], torch.cuda.current_stream().cuda_stream)

    bad = (dict(x=None), dict(w=None), dict(y=None), dict(kt=0), dict(kt=6, K=6 * 9 * 16), dict(kh=8, K=8 * 3 * 16 + 0),
           dict(kw=0), dict(sh=0), dict(sw=3), dict(ph=2), dict(pw=-1), dict(act=2), dict(f32=2), dict(cin=12, K=128),
           dict(ldx=Cin + 4), dict(ldx=8), dict(ldy=N - 8), dict(ldy=N + 4), dict(K=256), dict(K=144),
           dict(kt=5, T=4, K=5 * 9 * 16 + 48), dict(kh=7, kw=7, H=4, W=4, K=7 * 7 * 16 + 48 - 64 + 64),
           dict(x=x.data_ptr() + 2), dict(w=w.data_ptr() + 8), dict(y=g.view.data_ptr() + 2))
    for kw in bad:
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view.float()).all()), "a refused call wrote its output"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((g.view == 0).all())
    P.assert_guard_intact(g, "the accepted call")


# ---------------------------------------------------------------- ls_maxpool2d
POOL_CASES = (("k3_s2_7x7", (3, 3), (2, 2), (0, 0), 7, 7, (3, 3)),
              ("k3_s12_13x20", (3, 3), (1, 2), (0, 0), 13, 20, (11, 9)),
              ("k3_s2_p1_6x6", (3, 3), (2, 2), (1, 1), 6, 6, (3, 3)),
              ("k2_s1_p01_5x4", (2, 2), (1, 1), (0, 1), 5, 4, (4, 5)))


@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_maxpool_exact(gpu, case):
    """All inputs are negative: a zero pad (instead of -inf) would win at the border."""
    name, win, stride, pad, H, W, out_hw = case
    n, C = 2, 24
    x = P.bf16_round(-rnd(n, H, W, C, seed=len(name)).abs() - 0.125)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), win, stride, pad).permute(0, 2, 3, 1)
    assert tuple(ref.shape[1:3]) == out_hw
    xd = nan_framed(x)
    snap = P.snapshot(xd)
    g = P.guarded((n,) + out_hw + (C,), pitch=C + 8, dtype=BF, device=DEV)
    ops.maxpool2d(xd, win, stride, pad, out=g.view)
    torch.cuda.synchronize()
    assert torch.equal(g.view.float().cpu(), ref), name
    assert float(g.view.float().max()) < 0
    P.assert_guard_intact(g, name)
    P.assert_unchanged(xd, snap, name + " input")


def test_maxpool_invalid_arguments_launch_nothing(gpu):
    lib = _lib.load()
    x = torch.zeros((1, 6, 6, 16), dtype=BF, device=DEV)
    g = P.guarded((1, 6, 6, 16), pitch=24, dtype=BF, device=DEV)

    def call(kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, C=16, ldx=16, ldy=24, H=6):
        return lib.ls_maxpool2d(x.data_ptr(), ldx, 1, H, 6, C, kh, kw, sh, sw, ph, pw, g.view.data_ptr(), ldy,
                                torch.cuda.current_stream().cuda_stream)

    for kw in (dict(kh=4), dict(kw=0), dict(sh=3), dict(sw=0), dict(ph=2), dict(kh=1, ph=1), dict(C=12), dict(ldx=12),
               dict(ldy=20), dict(ldy=8), dict(H=0)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view.float()).all())
    assert call() == 0


# ---------------------------------------------------------------- ls_sync_offset
OFFSET_CASES = [(n, v, k) for n in (4, 6, 40) for v in (5, 15) for k in (-4, -3, 0, 3, 4) if abs(k) < n]


@pytest.mark.parametrize("n,vshift,k", OFFSET_CASES)
def test_sync_offset_planted_shift(gpu, n, vshift, k):
    """cc_feat[i] = im_feat[i - k] + small noise (unrelated rows where i - k leaves the clip).
    dists[i][j] compares im[i] with cc[i + j - vshift] = im[i + j - vshift - k], which is im[i]
    at j = vshift + k: the minimum sits there and av_offset = vshift - argmin is exactly -k --
    over this k set the recovered offsets are -4, -3, 0, 3, 4.  n = 4 lies below both vshifts, 6
    between them, 40 above; dists and mean_dists against float64."""
    D = 64
    gen = torch.Generator().manual_seed(100 * n + vshift + k)
    im = torch.randn(n, D, generator=gen)
    cc = torch.randn(n, D, generator=gen)
    for i in range(n):
        if 0 <= i - k < n:
            cc[i] = im[i - k] + 0.01 * torch.randn(D, generator=gen)
    win = 2 * vshift + 1
    gd = P.guarded((n, win), dtype=torch.float32, device=DEV)
    gm = P.guarded((1, win), dtype=torch.float32, device=DEV)
    imd, ccd = im.to(DEV), cc.to(DEV)
    ops.sync_offset(imd, ccd, vshift, dists=gd.view, mean_dists=gm.view[0])
    torch.cuda.synchronize()
    rd, rm = R.pdist(im, cc, vshift)
    # D squares (a subtraction, the eps, the square: 3 roundings each), D - 1 additions in any
    # order, the root: (D / 2 + 4) 2^-24 relative, within elem_bound's 16 2^-24 (D / 32 + 1) |ref|
    P.assert_elementwise(gd.view, rd, P.elem_bound(rd, rd * (D / 32 + 1), torch.float32), name="dists")
    # the mean adds n of them (n 2^-24 relative) and divides
    P.assert_elementwise(gm.view[0], rm, P.elem_bound(rm, rm * (D / 32 + n / 16 + 2), torch.float32), name="mean_dists")
    P.assert_guard_intact(gd, "dists")
    P.assert_guard_intact(gm, "mean_dists")
    off, mn, conf = synceval.offset_from_means(gm.view[0].cpu().numpy(), vshift)
    assert off == -k and conf > 0
    assert int(torch.argmin(rm)) == vshift + k


def test_sync_offset_is_deterministic_and_validates(gpu):
    lib = _lib.load()
    im, cc = rnd(33, 1024, seed=1).to(DEV), rnd(33, 1024, seed=2).to(DEV)
    a = ops.sync_offset(im, cc, 15)
    b = ops.sync_offset(im, cc, 15)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    g = P.guarded((33, 31), dtype=torch.float32, device=DEV)
    m = torch.zeros(31, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for n, D, v in ((0, 1024, 15), (33, 0, 15), (33, 1024, 16), (33, 1024, -1)):
        assert lib.ls_sync_offset(im.data_ptr(), cc.data_ptr(), n, D, v, g.view.data_ptr(), m.data_ptr(), s) == 1
    assert lib.ls_sync_offset(None, cc.data_ptr(), 33, 1024, 15, g.view.data_ptr(), m.data_ptr(), s) == 1
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view).all())


# ---------------------------------------------------------------- ls_crop_track
def test_crop_track_exact(gpu):
    """40 x 32 frames, one plan row per situation: the crop reaches into the 110-valued padding on
    the top, the bottom, the left and the right; a crop of exactly 448 x 448 (the 2 x 2 area
    path); an upscale of a crop inside the frame; a downscale; an anisotropic crop."""
    H, W = 40, 32
    plans = np.array([
        (0, 30, 12, 40, 10),        # top padding (rows 0..9 of the padded frame)
        (35, 60, 12, 40, 10),       # bottom padding
        (15, 45, 0, 28, 10),        # left padding
        (15, 45, 30, 52, 10),       # right padding
        (5, 453, 2, 450, 210),      # exactly 448 x 448
        (12, 32, 8, 24, 0),         # 20 x 16 inside the frame: upscale
        (20, 320, 30, 310, 150),    # 300 x 280: downscale
        (0, 240, 100, 130, 100),    # 240 x 30: down on one axis, up on the other
        (3, 227, 3, 227, 100),      # 224 x 224: the identity size
    ], dtype=np.int32)
    n = plans.shape[0]
    frames = torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    want = R.crop_video_ref(frames.numpy(), plans)
    g = P.guarded((n * 224 * 224, 3), dtype=torch.uint8, device=DEV)
    fd = frames.to(DEV)
    snap = P.snapshot(fd)
    out = g.view.view(n, 224, 224, 3)
    ops.crop_track(fd, torch.from_numpy(plans).to(DEV), out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(n):
        diff = np.argwhere(got[i] != want[i])
        assert diff.size == 0, (i, plans[i].tolist(), diff[:4].tolist(), got[i][tuple(diff[0])], want[i][tuple(diff[0])])
    P.assert_guard_intact(g, "crop_track")
    P.assert_unchanged(fd, snap, "frames")


def test_crop_track_from_boxes(gpu):
    n, H, W = 16, 40, 32
    frames = torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(10), dtype=torch.uint8)
    boxes = np.tile(np.array([[8.0, 10.0, 24.0, 30.0]]), (n, 1)) + 0.25 * np.arange(n)[:, None]
    boxes[5] = np.nan
    plan = synceval.crop_plan(boxes)
    got = synceval.crop_track(frames.to(DEV), boxes)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, 224, 224, 3) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), R.crop_video_ref(frames.numpy(), plan))
    with pytest.raises(ValueError, match="boxes for"):
        synceval.crop_track(frames.to(DEV), boxes[:-1])
    with pytest.raises(ValueError, match="device"):
        synceval.crop_track(frames, boxes)
    lib = _lib.load()
    g = P.guarded((224 * 224, 3), dtype=torch.uint8, device=DEV)
    pl = torch.zeros(5, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    fd = frames.to(DEV)
    assert lib.ls_crop_track(fd.data_ptr(), 0, H, W, pl.data_ptr(), g.view.data_ptr(), s) == 1
    assert lib.ls_crop_track(fd.data_ptr(), 1, 0, W, pl.data_ptr(), g.view.data_ptr(), s) == 1
    assert lib.ls_crop_track(fd.data_ptr(), 1, H, W, None, g.view.data_ptr(), s) == 1
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool((g.view == 0xA5).all())
