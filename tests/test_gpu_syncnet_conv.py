"""ls_conv3x3_strided per element (tests/parity.py): every case inside a sentinel guard band
with a pitch above N, the input a pitched view whose surroundings are NaN (a tap that should
read zero but reads memory fails), acceptance |got - ref| <= gemm_bound against a float64
convolution of the bf16 inputs.  Prints the worst err / bound ratio of each case."""
import math

import pytest
import torch
import torch.nn.functional as F

import parity as P
from latentsync_amd import _lib, ops
from latentsync_amd.packing import pack_weight

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (name, (sh, sw, top, left), n_img, H, W, Ho, Wo, Cin, N)
CASES = (
    ("w2_top", (1, 2, 1, 0), 3, 16, 32, 16, 16, 32, 32),
    ("h2_left", (2, 1, 0, 1), 1, 20, 13, 10, 13, 32, 32),
    ("s23_longk", (2, 3, 0, 0), 3, 2, 3, 1, 1, 512, 96),       # K = 4608: the waves split K; M = 3
    ("s22_tails", (2, 2, 0, 0), 1, 5, 6, 3, 3, 40, 24),        # K 360 -> 384, N tail
    ("s11_pad1", (1, 1, 1, 1), 2, 9, 7, 9, 7, 64, 72),         # = ls_conv2d pad 1; channel-chunk-major K
    ("s32_splitk_tapmajor", (3, 2, 1, 0), 2, 4, 5, 2, 3, 232, 10),  # K = 2088: split K, tap-major; N % 4: scalar tail
)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nan_framed(x):
    """x (n, H, W, C) as a view of a NaN-filled device buffer: two NaN pixels rows before and
    after all images and a pitch of C + 8."""
    n, H, W, C = x.shape
    g = P.guarded((n, H, W, C), pitch=C + 8, pad_rows=2 * W + 2, dtype=BF, device=DEV)
    g.view.copy_(x.to(BF).to(DEV))
    return g.view


def make(case):
    name, (sh, sw, pt, pl), n, H, W, Ho, Wo, Cin, N = case
    seed = sum(map(ord, name))
    x = P.bf16_round(rnd(n, H, W, Cin, seed=seed))
    w = P.bf16_round(rnd(N, Cin, 3, 3, seed=seed + 1, scale=1 / math.sqrt(9 * Cin)))
    b = rnd(N, seed=seed + 2, scale=0.1)
    pb, pr = (Ho - 1) * sh + 3 - H - pt, (Wo - 1) * sw + 3 - W - pl  # zero padding the outputs reach
    xp = F.pad(P.f64(x).permute(0, 3, 1, 2), (pl, max(pr, 0), pt, max(pb, 0)))
    w64 = P.f64(w)
    ref = F.conv2d(xp, w64, P.f64(b), stride=(sh, sw))[:, :, :Ho, :Wo].permute(0, 2, 3, 1)
    mag = F.conv2d(xp.abs(), w64.abs(), P.f64(b).abs(), stride=(sh, sw))[:, :, :Ho, :Wo].permute(0, 2, 3, 1)
    assert ref.shape == (n, Ho, Wo, N)
    pw = ops.Packed(pack_weight(w).to(BF).to(DEV), b.float().to(DEV), Cin, 3, N)
    return x, pw, ref, P.gemm_bound(ref, mag, 9 * Cin, BF)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_strided_conv_parity(gpu, case):
    name, (sh, sw, pt, pl), n, H, W, Ho, Wo, Cin, N = case
    x, pw, ref, bound = make(case)
    xd = nan_framed(x)
    snap = P.snapshot(xd)
    g = P.guarded((n, Ho, Wo, N), pitch=(N + 7) // 8 * 8 + 8, dtype=BF, device=DEV)
    ops.conv3x3_strided(xd, pw, (sh, sw), (pt, pl), (Ho, Wo), out=g.view)
    torch.cuda.synchronize()
    worst = P.assert_elementwise(g.view, ref, bound, where=dict(rows=16, cols=16), name=name)
    P.assert_guard_intact(g, name)
    P.assert_unchanged(xd, snap, name + " input")
    print(f"{name}: worst err/bound {worst:.3f}")


def test_stride1_pad1_agrees_with_conv2d(gpu):
    """(1, 1, 1, 1) is ls_conv2d's pad-1 conv: both sit within the bound of the same reference."""
    case = CASES[4]
    x, pw, ref, bound = make(case)
    xd = x.to(BF).to(DEV)
    y = ops.conv(xd, pw)
    torch.cuda.synchronize()
    worst = P.assert_elementwise(y, ref, bound, name="ls_conv2d pad 1")
    print(f"ls_conv2d on the same case: worst err/bound {worst:.3f}")


def test_invalid_arguments_launch_nothing(gpu):
    lib = _lib.load()
    Cin, N, H, W = 32, 32, 8, 8
    x = torch.zeros((1, H, W, Cin), dtype=BF, device=DEV)
    w = torch.zeros((N, 320), dtype=BF, device=DEV)
    g = P.guarded((1, H, W, N), pitch=N + 8, dtype=BF, device=DEV)

    def call(sh=1, sw=1, pt=1, pl=1, cin=Cin, ldx=Cin, K=320, ldy=N + 8):
        return lib.ls_conv3x3_strided(x.data_ptr(), ldx, 1, H, W, cin, w.data_ptr(), K, N, None, sh, sw, pt, pl, H, W,
                                      g.view.data_ptr(), ldy, torch.cuda.current_stream().cuda_stream)

    for kw in (dict(sh=0), dict(sw=4), dict(sh=4), dict(pt=2), dict(pl=2), dict(cin=28, K=256), dict(ldx=Cin + 4),
               dict(ldy=N + 4), dict(K=384)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    P.assert_guard_intact(g, "refused calls")
    assert bool(torch.isnan(g.view.float()).all()), "a refused call wrote its output"
    assert call() == 0
