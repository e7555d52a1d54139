"""The position-major form of the tiled 3x3 / stride 1 / pad 1 conv (tuning key 22 = 2:
wherever legal) against the standard raster (key 22 = 0) and an fp32 conv2d on the host.

A position-major tile is 256 frames at one pixel; its K loop leaves out the taps that fall
into the zero padding there.  Those K-tiles only ever added products with a zero factor and
the surviving terms keep their order, so y must be BIT-EQUAL to the standard raster's (compared
as int16, no tolerance).  Against the host's fp32 conv2d every element is within
parity.gemm_bound(9 Cin accumulations, bf16 out), the bound of the other conv edge tests.

Shapes: 4x4 and 8x8 images (every position class: 4 corners, edges, an interior); n_img 256
(one full frame group), 272 (a ragged group of 16 rows) and 520 (two full groups and a ragged
one); Cin 64, 64 + 64 through x2, and 192 (one, two and three chunks), x at a pitch above C;
N 256, 320 (a ragged second column tile) and 128 (the 256 x 128 tile); residual on and off,
bias on; y at pitch N + 8 inside sentinel rows.  Row vectors (not in the shapes above): one row
for the whole call (folded into the tile's column constants) and one per 256 rows (looked up
per row, 16 different ones in a 4x4 tile).  The 4x4 cases also run on the forced 256 x 128 tile
(tuning key 2 = 6).  The references are computed once per shape and shared."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import parity as P
import test_gpu_edges_gemm as E
from latentsync_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
SENTINEL = 0x7FC1  # a bf16 NaN with a payload
PAD_ROWS = 3

# (hw, n_img, (C1, C2), N, res, rowvec: 0 none, 1 one row per 256 rows, 2 one row for the call)
CASES = [
    (8, 520, (64, 0), 128, True, 0),
    (8, 272, (64, 64), 320, True, 0),
    (8, 256, (192, 0), 256, False, 0),
    (4, 520, (192, 0), 320, True, 0),
    (4, 272, (64, 0), 256, False, 0),
    (4, 256, (64, 64), 128, True, 0),
    (4, 272, (64, 0), 320, True, 1),
    (8, 256, (64, 0), 256, False, 2),
]
# (case, forced tile id): every case on the planner's tile, the 4x4 ones on 256 x 128 too
RUNS = [(c, 0) for c in CASES] + [(c, 6) for c in CASES if c[0] == 4]


@functools.lru_cache(maxsize=None)
def case(hw, n, C1, C2, N, res, rv):
    """Inputs (bf16-rounded, standard normal; a non-zero bias so that no output is exactly
    zero), the host's fp32 conv2d and the per-element bound."""
    Cin = C1 + C2
    x = P.bf16_round(E.rnd(n, hw, hw, Cin, seed=hw + n + Cin))
    w = P.bf16_round(E.rnd(N, Cin, 3, 3, seed=N + Cin + 1, scale=1 / math.sqrt(9 * Cin)))
    b = E.rnd(N, seed=2, scale=0.1) + 0.5
    r = P.bf16_round(E.rnd(n, hw, hw, N, seed=77)) if res else None
    M = n * hw * hw
    t = E.rnd({0: 1, 1: M // 256, 2: 1}[rv], N, seed=5) if rv else None
    xc = x.permute(0, 3, 1, 2)
    ref = F.conv2d(xc, w, None, padding=1).permute(0, 2, 3, 1) + b
    mag = F.conv2d(xc.abs(), w.abs(), None, padding=1).permute(0, 2, 3, 1) + b.abs()
    if rv:
        rows = t[torch.arange(M) // (256 if rv == 1 else M)].reshape(ref.shape)
        ref, mag = ref + rows, mag + rows.abs()
    if res:
        ref, mag = ref + r, mag + r.abs()
    return x, w, b, r, t, ref, P.gemm_bound(ref, mag, 9 * Cin, BF)


def guarded_y(M, N):
    buf = torch.full((M + 2 * PAD_ROWS, N + 8), SENTINEL, dtype=torch.int16, device=DEV)
    return buf, buf.view(BF)[PAD_ROWS:PAD_ROWS + M, :N]


def assert_guards(name, buf, M, N):
    assert bool((buf[:PAD_ROWS] == SENTINEL).all()) and bool((buf[PAD_ROWS + M:] == SENTINEL).all()), \
        f"{name}: rows outside y were written"
    assert bool((buf[PAD_ROWS:PAD_ROWS + M, N:] == SENTINEL).all()), f"{name}: the guard columns were written"
    assert not bool((buf[PAD_ROWS:PAD_ROWS + M, :N] == SENTINEL).any()), f"{name}: elements of y were not written"


@pytest.mark.parametrize("c,tile", RUNS, ids=[f"{c[0]}x{c[0]}-n{c[1]}-c{c[2][0]}+{c[2][1]}-N{c[3]}-res{int(c[4])}-rv{c[5]}"
                                              f"-tile{t}" for c, t in RUNS])
def test_posmajor(gpu, c, tile):
    hw, n, (C1, C2), N, res, rv = c
    name = f"posmajor {hw}x{hw} n_img {n} Cin {C1}+{C2} N {N} res {res} rowvec {rv} tile {tile}"
    x, w, b, r, t, ref, bound = case(hw, n, C1, C2, N, res, rv)
    M = n * hw * hw
    pw = E.packed(w, b, 3)
    kw = dict(split_k=1)
    x1 = E.wide(x[..., :C1], C1 + 8)
    if C2:
        kw["x2"] = E.wide(x[..., C1:], C2 + 16)
    if res:
        kw["res"] = E.wide(r, N + 8)
    if rv:
        kw["rowvec"] = (t.float().to(DEV).contiguous(), 256 if rv == 1 else M, N)
    inputs = E.snaps(x1, kw.get("x2"), pw.w, pw.bias, kw.get("res"))
    lib = _lib.load()
    out = {}
    try:
        assert lib.ls_set_tuning(2, tile) == 0
        for key22 in (0, 2):
            assert lib.ls_set_tuning(22, key22) == 0
            buf, y = guarded_y(M, N)
            cs = torch.full((M // 128, 2, N), float("nan"), dtype=torch.float32, device=DEV)
            view = y.view(n, hw, hw, N)
            plan = ops.conv_plan(x1, pw, out=view, gn_out=cs, **kw)
            assert plan["posmajor"] == (1 if key22 else 0), (name, plan)
            if key22:
                assert (plan["bm"], plan["bn"]) == (256, 128 if tile == 6 or N < 256 else 256), (name, plan)
                assert plan["grid"] == hw * hw * -(-n // 256) * -(-N // plan["bn"])
            ops.conv(x1, pw, out=view, gn_out=cs, **kw)
            torch.cuda.synchronize()
            assert_guards(f"{name} key22 {key22}", buf, M, N)
            out[key22] = (y, cs, plan)
    finally:
        lib.ls_set_tuning(22, 1)
        lib.ls_set_tuning(2, 0)
    for i, (tns, snap) in enumerate(inputs):
        P.assert_unchanged(tns, snap, f"{name} input {i}")
    (y0, cs0, plan0), (y2, cs2, _) = out[0], out[2]
    # bit-equal to the standard raster
    same = y0.contiguous().view(torch.int16) == y2.contiguous().view(torch.int16)
    assert bool(same.all()), f"{name}: {int((~same).sum())} of {same.numel()} elements differ from the standard raster"
    # the host's fp32 conv2d, per element
    worst = P.assert_elementwise(y2.reshape(ref.shape), ref, bound, where=E.FRAG, name=name)
    # column sums: the read pass over the same bytes is bit-equal; a standard plan that sums in its
    # epilogue adds the same 128 stored values in another order (parity.colsum_bound for each)
    if plan0["colsum_rows"]:
        assert torch.equal(cs0.view(torch.int32), cs2.view(torch.int32)), f"{name}: column sums differ"
    else:
        cref, cb = P.colsum_bound(y2.contiguous())
        P.assert_elementwise(cs0, cref, cb, name=name + " column sums (standard)")
        P.assert_elementwise(cs2, cref, cb, name=name + " column sums")
        P.assert_elementwise(cs2, P.f64(cs0), 2 * cb, name=name + " column sums vs standard")
    print(f"{name}: worst err/bound {worst:.3f}")
