"""The tap schedule of conv3x3_halo_kernel (ls_conv_halo.hip): a tap's MFMAs first, its halo
batch (GroupNorm affine + SiLU, the next batch's loads) behind them, the next tap's A
fragments read in two halves -- k-step 0 into the registers this tap's k-step 0 released,
k-step 1 last and still in flight across the barrier (the closing wait is lgkmcnt(4), not 0).
What that can break is WHEN something is read or published: a fragment read before the barrier
that publishes its image, a halo batch stored over an image still being read, a weight slot
overwritten under a pending read, a chunk transition or the last chunk (which has no next halo)
taking the wrong order.  So the cases walk the chunk counts and forms at which the order
differs, on images small enough for a CPU reference: one chunk (only the last-chunk path),
two (one transition), three (both halo image parities; the 3-slot ring wraps), five chunks on
the 16 x 16 128-column form, the 16 x 8 form, the dual source, two column tiles, GroupNorm
samples of one and two images, residual, per-frame row vector, column sums, the 9-tap upsample
form, the phase form (4 taps per chunk, a batch every tap) and the narrow tile.

Reference: fp32 torch conv of the bf16-rounded operands (the activated input rounded to bf16
as the halo image holds it), with the bound of tests/test_gpu_halo.py for the same forms
(rel < 1e-2 in the 2-norm).  A fault of the schedule is local -- one patch, one column tile --
and the rounding error of the bf16 output is the same everywhere, so the same bound is also
asserted for every block's own outputs.  Column sums: against the sums of the stored output,
with test_gpu_halo.py's tolerance."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from latentsync_amd import ops
from latentsync_amd.packing import pack_phase_weight, pack_weight

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16


def _bf(t):
    return t.to(BF).float()


def _block_errs(y, ref, bh, bn):
    """rel_err of every (bh x 16 pixels) x bn columns block of y (n, H, W, N)."""
    n, H, W, N = y.shape
    cut = lambda t: t.double().reshape(n, H // bh, bh, W // 16, 16, -1, min(bn, N)).permute(0, 1, 3, 5, 2, 4, 6).flatten(4)
    d, r = cut(y - ref), cut(ref)
    return d.norm(dim=-1) / (r.norm(dim=-1) + 1e-30)


def _case(n, H, W, C1, C2, N, ipp, aff, rowvec, res, ups, want):
    """ups: 0 plain, 1 the 9-tap upsample form, 2 the phase form; want = (family, BN, TH)."""
    g = torch.Generator().manual_seed(n * 1000 + H + 3 * W + C1 + 7 * C2 + N + ups)
    Cin = C1 + C2
    x = _bf(torch.randn(n, H, W, C1, generator=g) * 2 + 0.5)
    x2 = _bf(torch.randn(n, H, W, C2, generator=g)) if C2 else None
    w = _bf(torch.randn(N, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5)
    b = 0.1 * torch.randn(N, generator=g)
    pw = ops.Packed(pack_weight(w).to(BF).to(DEV), b.to(DEV), Cin, 3, N)
    if ups == 2:
        pw.phase = pack_phase_weight(w).to(BF).to(DEV).contiguous()
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    S = n // ipp
    scale = (1 + 0.2 * torch.randn(S, Cin, generator=g)).float()
    shift = (0.3 * torch.randn(S, Cin, generator=g)).float()
    tv = torch.randn(n, N, generator=g) if rowvec else None
    rv = _bf(torch.randn(n, Ho, Wo, N, generator=g)) if res else None
    xd = x.to(BF).to(DEV)
    kw = {}
    if x2 is not None:
        kw["x2"] = x2.to(BF).to(DEV)
    if ups:
        kw["upsample"] = True
    if aff:
        kw["aff"] = (scale.to(DEV), shift.to(DEV), ipp, True)
    if rowvec:
        kw["rowvec"] = (tv.to(DEV), Ho * Wo, N)
    if res:
        kw["res"] = rv.to(BF).to(DEV)
    plan = ops.conv_plan(xd, pw, **kw)
    assert (plan["family"], plan["halo_bn"], plan["halo_th"]) == want, plan
    assert plan["halo_gn"] == int(aff) and plan["halo_ph"] == int(ups == 2)
    y = ops.conv(xd, pw, gn_out=True, **kw)
    torch.cuda.synchronize()
    xin = torch.cat([x, x2], -1) if x2 is not None else x
    if aff:
        sc = scale.repeat_interleave(ipp, 0)[:, None, None, :]
        sh = shift.repeat_interleave(ipp, 0)[:, None, None, :]
        xin = _bf(F.silu(xin * sc + sh))
    xin = xin.permute(0, 3, 1, 2)
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w, b, padding=1).permute(0, 2, 3, 1)
    if rowvec:
        ref = ref + tv[:, None, None, :]
    if res:
        ref = ref + rv
    yc = y.float().cpu()
    e = rel_err(yc, ref)
    eb = _block_errs(yc, ref, 16 if ups == 2 else want[2], want[1])
    print(f"halo taps {n}x{H}x{W} {C1}+{C2}->{N} ups {ups} {want}: rel {e:.2e}, worst block {float(eb.max()):.2e}")
    assert y.shape == (n, Ho, Wo, N) and e < 1e-2
    assert float(eb.max()) < 1e-2, (eb >= 1e-2).nonzero()[:8]
    # column sums (sum, sum of squares per 128-row slot): per-sample totals against the stored output
    cs = y.gn_cs.view(S, -1, 2, N).double().sum(1).cpu()
    yd = yc.double().reshape(S, -1, N)
    want_cs = torch.stack([yd.sum(1), (yd * yd).sum(1)], 1)
    assert torch.allclose(cs, want_cs, rtol=2e-3, atol=1e-2 * Ho * Wo * ipp ** 0.5)


@pytest.mark.parametrize("H,W,C1,C2,N,ipp,aff,rowvec,res,want", [
    (16, 16, 64, 0, 160, 1, True, False, True, (3, 160, 16)),    # one chunk, one patch: all four borders
    (32, 48, 128, 0, 320, 2, True, True, False, (3, 160, 16)),   # one transition, two column tiles, 2-image samples
    (32, 48, 64, 128, 160, 1, True, False, True, (3, 160, 16)),  # dual source, three chunks: both halo parities
    (32, 48, 192, 0, 160, 1, False, True, True, (3, 160, 16)),   # no input affine (the other instance), row vector + residual
    (32, 48, 320, 0, 128, 2, True, False, True, (3, 128, 16)),   # 16 x 16 128-column form: five chunks, the 3-slot ring wraps
    (16, 16, 192, 0, 128, 1, True, False, False, (3, 128, 8)),   # 16 x 8 form, one image = two patches
    (32, 48, 128, 0, 128, 2, True, True, True, (3, 128, 8)),     # 16 x 8 form, border + interior patches
    (32, 48, 128, 0, 8, 1, True, False, False, (3, 16, 8)),      # the narrow tile
    (16, 16, 64, 0, 8, 1, True, False, True, (3, 16, 8)),        # narrow, one chunk
])
def test_halo_taps(gpu, H, W, C1, C2, N, ipp, aff, rowvec, res, want):
    _case(2, H, W, C1, C2, N, ipp, aff, rowvec, res, 0, want)


@pytest.mark.parametrize("H,W,Cin,N,res,ups,want", [
    (8, 8, 128, 160, False, 1, (3, 160, 16)),    # 9-tap upsample form: halo pixel (y, x) reads input (y >> 1, x >> 1)
    (16, 24, 192, 128, True, 1, (3, 128, 8)),
    (16, 16, 64, 160, True, 2, (4, 160, 16)),    # phase form: 4 taps per chunk, one chunk
    (16, 32, 192, 320, False, 2, (4, 160, 16)),  # three chunks, two column tiles, two patches
    (16, 16, 128, 128, True, 2, (4, 128, 8)),    # phase form on the 16 x 8 tile
    (16, 16, 320, 128, False, 2, (4, 128, 16)),  # phase form, 3-slot ring (slot (chunk + tap) % 3), five chunks
])
def test_halo_taps_upsample(gpu, H, W, Cin, N, res, ups, want):
    _case(2, H, W, Cin, 0, N, 1, False, False, res, ups, want)
