"""The phase form of the nearest-x2 upsample convs (ls_conv_desc.upsample == 2; ls_conv_path 4
on the halo-tile kernel, 5 on the tiled kernels) per element with guard bands, as tests/test_gpu_edges_gemm.py does it for the other kernels.

Reference: conv_reference(..., upsample=True) in fp64 on the bf16-rounded inputs and PER-TAP
weights.  Bound: gemm_bound(ref, mag, 4 Cin, bf16, prologue=True, prod_mag=prod) -- 4 Cin
accumulations per output, and the 2^-8 prod_mag term covers the one bf16 rounding of each
summed weight (|sum_taps w| <= sum_taps |w|, so sum |a| |round(sum w) - sum w| <= 2^-8 prod_mag).
An fp64 evaluation with the bf16-rounded phase weights is checked against the same bound on
the CPU, so the bound holds for the reference alone.  The phase form is also compared with
today's 9-tap upsample=True path: every element within the sum of the two bounds.  The
GroupNorm column sums of the halo phase form's epilogue (slots of 128 stored pixels of one output
parity) and of the tiled phase form's read pass give the same scale and shift as a read pass over
the stored output."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import parity as P
import test_gpu_edges_gemm as E
from conftest import rel_err
from latentsync_amd import ops
from latentsync_amd.packing import pack_phase_weight, phase_tap_sums

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16


def packed_phase(w, b):
    pw = E.packed(w, b, 3)
    pw.phase = pack_phase_weight(w).to(BF).to(DEV).contiguous()
    return pw


@functools.lru_cache(maxsize=None)
def case(H, W, Cin, N):
    """Inputs, the fp64 reference and both bounds of one shape (n_img 3), shared by the tests."""
    x = P.bf16_round(E.rnd(3, H, W, Cin, seed=H + W + Cin))
    w = P.bf16_round(E.rnd(N, Cin, 3, 3, seed=N + Cin + 1, scale=1 / math.sqrt(9 * Cin)))
    b = E.rnd(N, seed=2, scale=0.1)
    ref, mag, prod = E.conv_reference(x, None, w, b, 3, upsample=True)
    r = P.bf16_round(E.rnd(3, 2 * H, 2 * W, N, seed=77))
    return x, w, b, ref, mag, prod, r


def bounds(ref, mag, prod, Cin):
    return (P.gemm_bound(ref, mag, 4 * Cin, BF, prologue=True, prod_mag=prod),  # the phase form
            P.gemm_bound(ref, mag, 9 * Cin, BF))                                 # the 9-tap form


def phase_eval64(x, w, b):
    """fp64 evaluation of the four phase convs with the bf16-ROUNDED summed weights."""
    n, H, W, _ = x.shape
    w4 = P.f64(P.bf16_round(phase_tap_sums(w)))
    xp = F.pad(P.f64(x).permute(0, 3, 1, 2), (1, 1, 1, 1))
    out = torch.zeros(n, w.shape[0], 2 * H, 2 * W, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], w4[2 * py + px])
    return out.permute(0, 2, 3, 1) + P.f64(b)


def run_phase(name, H, W, Cin, N, res, tune=None, path=4):
    """The phase form and today's 9-tap form of one call, each into a guarded output."""
    x, w, b, ref, mag, prod, r = case(H, W, Cin, N)
    if res:
        ref, mag = ref + P.f64(r), mag + P.f64(r).abs()
    b4, b9 = bounds(ref, mag, prod, Cin)
    # the bound holds for the reference alone: rounded phase weights, exact arithmetic
    ev = phase_eval64(x, w, b) + (P.f64(r) if res else 0.0)
    assert bool(((ev - ref).abs() <= b4).all()), name
    pw, pw9 = packed_phase(w, b), E.packed(w, b, 3)
    xd = E.dev_bf(x)
    kw = {"res": E.wide(r, N + 8)} if res else {}
    g = P.guarded((3, 2 * H, 2 * W, N), pitch=N + 8, pad_rows=3, dtype=BF, device=DEV)
    g9 = P.guarded((3, 2 * H, 2 * W, N), pitch=N + 8, pad_rows=3, dtype=BF, device=DEV)
    inputs = E.snaps(xd, pw.w, pw.phase, pw.bias, kw.get("res"))
    with E.tuning(**(tune or {})):
        assert ops.conv_path(xd, pw, upsample=True, out=g.view, **kw) == path, name
        ops.conv(xd, pw, upsample=True, out=g.view, **kw)
        worst = E.finish(name, g, ref, b4, inputs)
        ops.conv(xd, pw9, upsample=True, out=g9.view, **kw)
        E.finish(name + " (9-tap)", g9, ref, b9, [])
    # equivalence: the two paths within the sum of their bounds, per element
    P.assert_elementwise(g.view.reshape(ref.shape), P.f64(g9.view.reshape(ref.shape)), b4 + b9, where=E.FRAG,
                         name=name + " vs 9-tap")
    return worst


# (tuning key 16 picks the patch form of the 128-column tile only)
HALO = [(Cin, N, th8, res) for Cin in (64, 128) for N in (128, 160) for th8 in (1, 0) for res in (False, True)
        if th8 == 1 or N == 128]


@pytest.mark.parametrize("Cin,N,th8,res", HALO)
def test_phase_halo(gpu, Cin, N, th8, res):
    """16 x 16 -> 32 x 32 (one 16 x 16 patch per image and parity, or two 16 x 8) and 16 x 32
    (two patches side by side: the inner patch edge reads its neighbour's pixels, the outer
    edges zeros), n_img 3, one and two channel chunks, both tile widths, both patch forms of the
    128-column tile (tuning key 16), without and with a residual of pitch N + 8."""
    worst = 0.0
    for H, W in ((16, 16), (16, 32)):
        worst = max(worst, run_phase(f"phase halo Cin {Cin} N {N} th8 {th8} {H}x{W} res {res}", H, W, Cin, N, res,
                                     tune=dict(k16=th8)))
    print(f"phase halo Cin {Cin} N {N} th8 {th8} res {res}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("N", [128, 160])
def test_phase_halo_three_chunks(gpu, N):
    """Cin 192: three chunks -- the weight ring's slot of a tap, (4 ci + t) % 3 on the 3-slot
    ring, changes from chunk to chunk, and both halo images are reused."""
    worst = run_phase(f"phase halo Cin 192 N {N}", 16, 16, 192, N, True, tune=dict(k16=0))
    print(f"phase halo Cin 192 N {N}: worst err/bound {worst:.3f}")


# tiled form: the auto tile, and the forced 256 x 256 (tile id 5) and 128 x 160 (id 9) tiles
TILED = [(hw, Cin, N, tile) for hw in ((4, 4), (8, 8), (5, 7)) for Cin in (64, 128) for N in (40, 320)
         for tile in (0, 5, 9)]


@pytest.mark.parametrize("hw,Cin,N,tile", TILED)
def test_phase_tiled(gpu, hw, Cin, N, tile):
    """4 x 4 -> 8 x 8, 8 x 8 -> 16 x 16 and 5 x 7 -> 10 x 14 (a parity's 48 / 192 / 105 rows: below
    one tile, and not a tile multiple), n_img 3, one and two chunks, N 40 (a ragged column tile)
    and 320 (more than one column tile), without and with a residual."""
    worst = 0.0
    for res in (False, True):
        worst = max(worst, run_phase(f"phase tiled {hw} Cin {Cin} N {N} tile {tile} res {res}", *hw, Cin, N, res,
                                     tune=dict(k2=tile), path=5))
    print(f"phase tiled {hw} Cin {Cin} N {N} tile {tile}: worst err/bound {worst:.3f}")


# (form, H, W, Cin, N, n_img, tuning, path): the halo epilogue's slots on every instance that
# fills them -- 160 columns, 128 columns on 16 x 8 and on 16 x 16 patches, two patch columns --
# and the tiled phase form's read pass (colsum_pass_kernel) on 8 x 8 images, below a halo patch
COLSUM = [("epilogue", 16, 16, 64, 160, 8, {}, 4), ("epilogue", 16, 16, 64, 128, 8, dict(k16=1), 4),
          ("epilogue", 16, 16, 64, 128, 8, dict(k16=0), 4), ("epilogue", 16, 32, 64, 128, 8, dict(k16=1), 4),
          ("epilogue", 16, 32, 64, 160, 8, {}, 4), ("read_pass", 8, 8, 64, 320, 8, {}, 5),
          ("read_pass", 8, 8, 128, 64, 8, {}, 5)]


@pytest.mark.parametrize("ips", [1, 4])
@pytest.mark.parametrize("form,H,W,Cin,N,n,tune,path", COLSUM)
def test_phase_column_sums(gpu, form, H, W, Cin, N, n, tune, path, ips):
    """gn_out=True: the GroupNorm scale and shift from .gn_cs equal those of a read pass over
    the stored bf16 output (rel 1e-4, as test_gn_colsum), for one-image and 4-image samples.
    epilogue: the halo phase form's own sums (every slot 128 stored pixels of one parity of one
    image).  read_pass: the tiled phase form, whose sums come from colsum_pass_kernel."""
    x = P.bf16_round(E.rnd(n, H, W, Cin, seed=5) + 0.5)
    w = P.bf16_round(E.rnd(N, Cin, 3, 3, seed=6, scale=1 / math.sqrt(9 * Cin)))
    pw = packed_phase(w, E.rnd(N, seed=7) + 1.0)
    xd = E.dev_bf(x)
    with E.tuning(**tune):
        assert ops.conv_path(xd, pw, upsample=True) == path
        y = ops.conv(xd, pw, upsample=True, gn_out=True)
    cs = y.gn_cs.double().cpu()
    S = n // ips
    assert cs.shape == (n * 4 * H * W // 128, 2, N)
    yf = y.float().cpu().double().reshape(S, -1, N)
    s1, s2 = yf.sum(1), (yf * yf).sum(1)
    tot = cs.reshape(S, -1, 2, N).sum(1)  # the slots of a sample lie in its own range
    assert (tot[:, 0] - s1).abs().max() <= 1e-5 * yf.abs().sum(1).max()
    assert (tot[:, 1] - s2).abs().max() <= 1e-5 * s2.max()
    gamma, beta = (1 + 0.1 * E.rnd(N, seed=8)).to(DEV), (0.1 * E.rnd(N, seed=9)).to(DEV)
    sc, sh = ops.group_norm(y, 32, 1e-6, gamma, beta, S)
    sc2, sh2 = ops.group_norm(y.clone(), 32, 1e-6, gamma, beta, S)  # no producer sums: the read pass
    assert rel_err(sc.cpu(), sc2.cpu()) < 1e-4 and rel_err(sh.cpu(), sh2.cpu()) < 1e-4
