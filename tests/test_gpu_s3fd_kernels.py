"""The kernels of csrc/ls_s3fd.hip, each against its definition: ls_conv3x3_relu per element
against a float64 convolution (tests/parity.py bounds, guard bands, NaN-framed inputs, one live
tap at a time), ls_maxpool2x2_ceil and ls_s3fd_prep exactly, ls_l2norm_scale per element, and
every entry point's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity as P
import s3fd_ref as R
from latentsync_amd import _lib, ops
from latentsync_amd.packing import pack_weight_general

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nan_framed(x):
    """x (n, H, W, C) as a view of a NaN-filled device buffer: NaN pixel rows before and after
    all images and a pitch of C + 8."""
    n, H, W, C_ = x.shape
    g = P.guarded((n, H, W, C_), pitch=C_ + 8, pad_rows=7 * W + 8, dtype=BF, device=DEV)
    g.view.copy_(x.to(BF).to(DEV))
    return g.view


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- ls_conv3x3_relu
CONV_KINDS = ((64, 64, 1), (256, 512, 1), (512, 1024, 6))
CONV_HW = ((19, 27), (5, 7), (2, 3), (1, 1))
CONV_CASES = [(cin, n, dil, hw) for cin, n, dil in CONV_KINDS for hw in CONV_HW + (((13, 9),) if dil == 6 else ())]


@pytest.mark.parametrize("cin,N,dil,hw", CONV_CASES, ids=[f"c{c}_n{n}_d{d}_{h}x{w}" for c, n, d, (h, w) in CONV_CASES])
def test_conv3x3_relu_parity(gpu, cin, N, dil, hw):
    """The weight is zero except at one tap at a time, so a misplaced tap shows; the other
    taps multiply whatever the kernel loaded for them by zero, so a load from the NaN frame
    around the images (a tap in the padding must be a zero operand, never a load) shows too.
    3 images and the first alone: the same bits.  19 x 27 x 3 = 1539 pixels are 13 blocks, the
    last one partial; at dilation 6 only the centre tap is live on 2 x 3 and 1 x 1, and on
    13 x 9 the side taps are live on some columns only."""
    H, W = hw
    seed = cin + N + dil + 31 * H + W
    x = P.bf16_round(rnd(3, H, W, cin, seed=seed))
    wt = P.bf16_round(rnd(N, cin, seed=seed + 1, scale=cin ** -0.5))
    b = rnd(N, seed=seed + 2, scale=0.1)
    y0 = P.f64(x) @ P.f64(wt).T               # (3, H, W, N): the live tap's product at the tap's source pixel
    m0 = P.f64(x).abs() @ P.f64(wt).abs().T
    xd = nan_framed(x)
    snap = P.snapshot(xd)
    x1 = x[:1].to(BF).to(DEV).contiguous()
    worst = 0.0
    for tap in range(9):
        dy, dx = (tap // 3 - 1) * dil, (tap % 3 - 1) * dil
        w4 = torch.zeros(N, cin, 3, 3)
        w4[:, :, tap // 3, tap % 3] = wt
        pw = ops.PackedGeneral(pack_weight_general(w4).to(BF).to(DEV), b.float().to(DEV), cin, (1, 3, 3))
        ref = torch.zeros_like(y0)
        mag = torch.zeros_like(y0)
        ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
        yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
        if ys.start < ys.stop and xs.start < xs.stop:
            ref[:, ys, xs] = y0[:, yt, xt]
            mag[:, ys, xs] = m0[:, yt, xt]
        ref, mag = ref + P.f64(b), mag + P.f64(b).abs()
        # ReLU is 1-Lipschitz: the pre-activation bound carries over, then the one rounding of the result
        bound = P.gemm_bound(ref, mag, cin, None) + P.U_BF16 * ref.clamp_min(0) * P.SLACK
        g = P.guarded((3, H, W, N), pitch=N + 8, dtype=BF, device=DEV)
        ops.conv3x3_relu(xd, pw, dil, out=g.view)
        one = ops.conv3x3_relu(x1, pw, dil)
        torch.cuda.synchronize()
        name = f"c{cin}_n{N}_d{dil}_{H}x{W} tap {tap}"
        worst = max(worst, P.assert_elementwise(g.view, ref.clamp_min(0), bound, where=dict(rows=128, cols=64), name=name))
        P.assert_guard_intact(g, name)
        assert torch.equal(one[0], g.view[0]), name + ": image 0 alone differs from image 0 of the batch"
    P.assert_unchanged(xd, snap, "conv input")
    print(f"c{cin}_n{N}_d{dil}_{H}x{W}: worst err/bound {worst:.3f}")


def test_conv3x3_relu_all_taps_against_conv_general(gpu):
    """A dense weight on an odd map: per element against float64, and ls_conv_general (which takes
    the same packed operand) within the same bound."""
    cin, N, H, W = 128, 64, 7, 11
    x = P.bf16_round(rnd(2, H, W, cin, seed=5))
    w4 = P.bf16_round(rnd(N, cin, 3, 3, seed=6, scale=(9 * cin) ** -0.5))
    b = rnd(N, seed=7, scale=0.1)
    x64 = P.f64(x).permute(0, 3, 1, 2)
    ref = F.conv2d(x64, P.f64(w4), P.f64(b), padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(x64.abs(), P.f64(w4).abs(), P.f64(b).abs(), padding=1).permute(0, 2, 3, 1)
    bound = P.gemm_bound(ref, mag, 9 * cin, None) + P.U_BF16 * ref.clamp_min(0) * P.SLACK
    pw = ops.PackedGeneral(pack_weight_general(w4).to(BF).to(DEV), b.float().to(DEV), cin, (1, 3, 3))
    xd = nan_framed(x)
    g = P.guarded((2, H, W, N), pitch=N + 8, dtype=BF, device=DEV)
    ops.conv3x3_relu(xd, pw, 1, out=g.view)
    other = ops.conv_general(xd, pw, (1, 1), (1, 1), relu=True)
    torch.cuda.synchronize()
    P.assert_elementwise(g.view, ref.clamp_min(0), bound, where=dict(rows=128, cols=64), name="dense 3x3")
    P.assert_elementwise(other, ref.clamp_min(0), bound, name="ls_conv_general on the same operand")
    P.assert_guard_intact(g, "dense 3x3")


def test_conv3x3_relu_invalid_arguments_launch_nothing(gpu):
    lib = _lib.load()
    cin, N, H, W = 64, 64, 4, 4
    x = torch.zeros((1, H, W, cin), dtype=BF, device=DEV)
    w = torch.zeros((N, 9 * cin), dtype=BF, device=DEV)
    g = P.guarded((1, H, W, N), pitch=N + 8, dtype=BF, device=DEV)
    base = dict(x=x.data_ptr(), ldx=cin, n=1, H=H, W=W, cin=cin, w=w.data_ptr(), N=N, dil=1, y=g.view.data_ptr(), ldy=N + 8)

    def call(**kw):
        a = dict(base, **kw)
        return lib.ls_conv3x3_relu(a["x"], a["ldx"], a["n"], a["H"], a["W"], a["cin"], a["w"], a["N"], None, a["dil"],
                                   a["y"], a["ldy"], stream())

    bad = (dict(x=None), dict(w=None), dict(y=None), dict(dil=0), dict(dil=2), dict(dil=7), dict(cin=32), dict(cin=96),
           dict(cin=1088), dict(N=32), dict(N=72), dict(ldx=cin - 8), dict(ldx=cin + 4), dict(ldy=N - 8), dict(ldy=N + 4),
           dict(n=0), dict(H=0), dict(W=-1), dict(x=x.data_ptr() + 2), dict(w=w.data_ptr() + 8), dict(y=g.view.data_ptr() + 2))
    for kw in bad:
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view.float()).all()), "a refused call wrote its output"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((g.view == 0).all())
    P.assert_guard_intact(g, "the accepted call")


# ---------------------------------------------------------------- ls_maxpool2x2_ceil
@pytest.mark.parametrize("hw", ((19, 27), (1, 1), (2, 3)), ids=lambda v: f"{v[0]}x{v[1]}")
def test_maxpool_ceil_exact(gpu, hw):
    """All inputs are negative: a zero in the clipped part of the last window would win."""
    H, W = hw
    n, C_ = 2, 24
    x = P.bf16_round(-rnd(n, H, W, C_, seed=H * W).abs() - 0.125)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
    assert tuple(ref.shape[1:3]) == ((H + 1) // 2, (W + 1) // 2)
    xd = nan_framed(x)
    snap = P.snapshot(xd)
    g = P.guarded(tuple(ref.shape), pitch=C_ + 8, dtype=BF, device=DEV)
    ops.maxpool2x2_ceil(xd, out=g.view)
    torch.cuda.synchronize()
    assert torch.equal(g.view.float().cpu(), ref)
    assert float(g.view.float().max()) < 0
    P.assert_guard_intact(g, "ceil pool")
    P.assert_unchanged(xd, snap, "ceil pool input")


def test_maxpool_ceil_invalid_arguments_launch_nothing(gpu):
    lib = _lib.load()
    x = torch.zeros((1, 5, 5, 16), dtype=BF, device=DEV)
    g = P.guarded((1, 3, 3, 16), pitch=24, dtype=BF, device=DEV)
    base = dict(x=x.data_ptr(), ldx=16, n=1, H=5, W=5, C=16, y=g.view.data_ptr(), ldy=24)

    def call(**kw):
        a = dict(base, **kw)
        return lib.ls_maxpool2x2_ceil(a["x"], a["ldx"], a["n"], a["H"], a["W"], a["C"], a["y"], a["ldy"], stream())

    for kw in (dict(x=None), dict(y=None), dict(C=12), dict(C=0), dict(ldx=8), dict(ldx=20), dict(ldy=8), dict(ldy=20),
               dict(n=0), dict(H=0), dict(W=0), dict(x=x.data_ptr() + 2), dict(y=g.view.data_ptr() + 2)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view.float()).all())
    assert call() == 0
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "the accepted call")


# ---------------------------------------------------------------- ls_l2norm_scale
@pytest.mark.parametrize("C_", (256, 512, 8))
def test_l2norm_scale_parity(gpu, C_):
    """x / (sqrt(sum x^2) + 1e-10) w per element under parity.elem_bound with |ref| as the term
    magnitude; an all-zero row gives 0, not NaN; a huge and a tiny row keep their scale."""
    n, H, W = 2, 3, 5
    x = rnd(n, H, W, C_, seed=C_)
    x[0, 1, 2] = 0.0
    x[1, 0, 0] *= 1e4
    x[1, 2, 4] *= 1e-4
    x = P.bf16_round(x)
    wgt = 10.0 * (1.0 + 0.1 * rnd(C_, seed=C_ + 1))
    x64 = P.f64(x)
    ref = x64 / (x64.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10) * P.f64(wgt)
    xd = nan_framed(x)
    snap = P.snapshot(xd)
    g = P.guarded((n, H, W, C_), pitch=C_ + 8, dtype=BF, device=DEV)
    ops.l2norm_scale(xd, wgt.to(DEV), out=g.view)
    torch.cuda.synchronize()
    worst = P.assert_elementwise(g.view, ref, P.elem_bound(ref, ref.abs(), BF), name=f"l2norm C {C_}")
    assert bool((g.view[0, 1, 2] == 0).all())
    P.assert_guard_intact(g, "l2norm")
    P.assert_unchanged(xd, snap, "l2norm input")
    print(f"l2norm C {C_}: worst err/bound {worst:.3f}")


def test_l2norm_scale_invalid_arguments_launch_nothing(gpu):
    lib = _lib.load()
    x = torch.zeros((4, 16), dtype=BF, device=DEV)
    wgt = torch.ones(16, device=DEV)
    g = P.guarded((4, 16), pitch=24, dtype=BF, device=DEV)
    base = dict(x=x.data_ptr(), ldx=16, M=4, C=16, w=wgt.data_ptr(), y=g.view.data_ptr(), ldy=24)

    def call(**kw):
        a = dict(base, **kw)
        return lib.ls_l2norm_scale(a["x"], a["ldx"], a["M"], a["C"], a["w"], a["y"], a["ldy"], stream())

    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(C=12), dict(C=0), dict(C=8200), dict(ldx=8), dict(ldy=8),
               dict(ldy=20), dict(M=0), dict(x=x.data_ptr() + 2), dict(y=g.view.data_ptr() + 2), dict(w=wgt.data_ptr() + 4)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view.float()).all())
    assert call() == 0
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "the accepted call")


# ---------------------------------------------------------------- ls_s3fd_prep
@pytest.mark.parametrize("hw,s", (((304, 432), 0.25), ((303, 430), 0.25), ((37, 53), 1.0)),
                         ids=("304x432_quarter", "303x430_quarter", "37x53_copy"))
def test_prep_exact(gpu, hw, s):
    """Exact against s3fd_ref.prep; 303 x 430 at 1 / 4 gives 75.75 x 107.5 -> 76 x 108 (cvRound,
    half to even) with the last row and column sampled past the frame's edge."""
    frames = R.case_frames(2, hw, seed=hw[0] + hw[1])
    ref = R.prep(frames, s).permute(0, 2, 3, 1)
    h, w = ref.shape[1:3]
    assert (h, w) == ops.s3fd_prep_size(hw[0], hw[1], s) == ((76, 108) if s == 0.25 else hw)
    fd = frames.to(DEV)
    snap = P.snapshot(fd)
    g = P.guarded((2, h, w, 8), dtype=BF, device=DEV)
    ops.s3fd_prep(fd, s, out=g.view)
    torch.cuda.synchronize()
    got = g.view.float().cpu()
    assert torch.equal(got[..., :3], ref)
    assert bool((got[..., 3:] == 0).all())
    P.assert_guard_intact(g, "prep")
    P.assert_unchanged(fd, snap, "frames")
    if s == 1.0:
        mean = torch.tensor([123.0, 117.0, 104.0])
        assert torch.equal(got[..., :3], frames.float() - mean)


def test_prep_invalid_arguments_launch_nothing(gpu):
    lib = _lib.load()
    f = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV)
    g = P.guarded((1, 16, 16, 8), dtype=BF, device=DEV)
    base = dict(f=f.data_ptr(), n=1, H=16, W=16, s=1.0, out=g.view.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return lib.ls_s3fd_prep(a["f"], a["n"], a["H"], a["W"], C.c_double(a["s"]), a["out"], stream())

    for kw in (dict(f=None), dict(out=None), dict(n=0), dict(H=0), dict(W=40000), dict(s=0.0), dict(s=-0.25), dict(s=1.5),
               dict(s=float("nan")), dict(s=0.5), dict(s=0.01), dict(out=g.view.data_ptr() + 2)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view.float()).all())
    with pytest.raises(ValueError, match="0.5 is refused"):
        ops.s3fd_prep(f, 0.5)
    assert call() == 0
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "the accepted call")
