"""The position-major form of the tiled 3x3 conv in the plan (ls_conv_plan, host only, no GPU):
where ls_conv_plan_info.posmajor is reported under tuning key 22 (0 never, 1 by the cost model,
2 wherever legal), and the launch order ls_conv_posmajor_tile -- the host twin of the kernel's
pm_tile_of -- as a bijection that gives every XCD the same tap-unit total to within one tile."""
import ctypes as C

import pytest

from latentsync_amd import _lib


def _desc(**over):
    """The 8x8 flagship 3x3 descriptor (dummy pointers, never dereferenced) with fields replaced."""
    d = _lib.ConvDesc()
    d.x1 = d.w = d.y = 4096
    d.C1, d.ld1, d.n_img, d.H, d.W, d.Ho, d.Wo = 1280, 1280, 768, 8, 8, 8, 8
    d.ksize, d.stride, d.pad, d.K, d.N, d.ldy = 3, 1, 1, 9 * 1280, 1280, 1280
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _plan(key22, **over):
    lib = _lib.load()
    info = _lib.ConvPlanInfo()
    assert lib.ls_set_tuning(22, key22) == 0
    try:
        assert lib.ls_conv_plan(C.byref(_desc(**over)), C.byref(info)) == 0, lib.ls_last_error().decode()
    finally:
        assert lib.ls_set_tuning(22, 1) == 0
    return info


CAT = dict(C1=640, ld1=640, C2=640, ld2=640, x2=4096)
# descriptors the form must not be reported for, under the cost model (key 22 = 1) ...
NOT_CHOSEN = {
    "n_img16": dict(n_img=16),
    "n_img64": dict(n_img=64),
    "n_img255": dict(n_img=255),
    "level4x4_n_img16": dict(H=4, W=4, Ho=4, Wo=4, n_img=16),  # (an equal critical path, 11 times the tap-units)
    "level4x4_n_img64": dict(H=4, W=4, Ho=4, Wo=4, n_img=64),
}
# ... and under any value of the key: it is not legal
NOT_LEGAL = {
    "stride2": dict(stride=2, Ho=4, Wo=4),
    "upsample1": dict(upsample=1, Ho=16, Wo=16),
    "upsample2": dict(upsample=2, Ho=16, Wo=16, K=4 * 1280),
    "ksize1": dict(ksize=1, pad=0, K=1280),
    "affine": dict(aff_scale=4096, aff_shift=4096, imgs_per_sample=16),
    "split_k": dict(split_k=4, workspace=4096, workspace_bytes=1 << 40),
    "cin_not_64": dict(C1=1288, ld1=1288, K=11648),
    "rowvec_per_frame": dict(rowvec=4096, rows_per_vec=64),
}
LEGAL = {
    "flagship": dict(),
    "flagship_x2": CAT,
    "residual_rowvec": dict(res=4096, ldr=1280, rowvec=4096, rows_per_vec=768 * 64),
    "f32_out": dict(y_f32=1),
    "level4x4": dict(H=4, W=4, Ho=4, Wo=4),
    "n_img16": dict(n_img=16),
    "small_64_256": dict(C1=64, ld1=72, K=576, N=256, ldy=264, n_img=256),
    "small_cat_320": dict(C1=64, ld1=72, C2=64, ld2=64, x2=4096, K=1152, N=320, ldy=328, n_img=272),
    "small_192_128": dict(C1=192, ld1=200, K=1728, N=128, ldy=136, n_img=520, H=4, W=4, Ho=4, Wo=4),
}


def test_field_is_last_and_mirrored():
    names = [f for f, _ in _lib.ConvPlanInfo._fields_]
    assert names[-2:] == ["workspace_bytes", "posmajor"]
    assert _lib.ConvPlanInfo.workspace_bytes.offset == 22 * 4  # (the offsets before it are unchanged)
    assert _lib.ConvPlanInfo.posmajor.offset == 22 * 4 + 8


@pytest.mark.parametrize("over", [dict(), CAT], ids=["x1", "x1_x2"])
def test_flagship_8x8_by_cost_model(over):
    p = _plan(1, **over)
    assert (p.family, p.posmajor, p.bm, p.bn, p.ks, p.tapu, p.buf, p.epi, p.split) == (0, 1, 256, 256, 3, 1, 1, 0, 1)
    assert (p.grid, p.threads, p.lds_bytes) == (64 * 3 * 5, 512, 133120)
    std = _plan(0, **over)
    assert std.posmajor == 0 and (std.family, std.bm, std.bn, std.grid) == (0, 256, 256, 960)
    # the GroupNorm column sums stay a read pass over y in natural row order
    cs = _plan(1, gn_colsum_out=4096, **over)
    assert cs.posmajor == 1 and cs.colsum_rows == 768 * 64 == _plan(0, gn_colsum_out=4096, **over).colsum_rows


def test_flagship_4x4_by_cost_model():
    """240 blocks in either form, one per CU: the critical paths are equal (9 tap-units) and the
    position-major form has fewer tap-units in all (100 of 144 per frame), so it is taken."""
    p = _plan(1, H=4, W=4, Ho=4, Wo=4)
    assert (p.family, p.posmajor, p.bm, p.bn, p.split, p.grid) == (0, 1, 256, 256, 1, 16 * 3 * 5)


@pytest.mark.parametrize("name", list(NOT_CHOSEN))
def test_not_chosen_by_cost_model(name):
    assert _plan(1, **NOT_CHOSEN[name]).posmajor == 0


@pytest.mark.parametrize("name", list(NOT_LEGAL))
@pytest.mark.parametrize("key22", [1, 2])
def test_not_legal(name, key22):
    assert _plan(key22, **NOT_LEGAL[name]).posmajor != 1


@pytest.mark.parametrize("name", list(LEGAL))
def test_key22(name):
    p = _plan(2, **LEGAL[name])
    over = LEGAL[name]
    n, hw, N = over.get("n_img", 768), over.get("H", 8) * over.get("W", 8), over.get("N", 1280)
    bn = 256 if N >= 256 else 128
    assert (p.posmajor, p.family, p.bm, p.bn, p.buf, p.split) == (1, 0, 256, bn, 1, 1)
    assert p.epi == (2 if over.get("y_f32") else 0)
    assert p.grid == hw * -(-n // 256) * -(-N // bn)
    assert _plan(0, **LEGAL[name]).posmajor == 0  # never


def test_key22_values():
    lib = _lib.load()
    for v in (-1, 3):
        assert lib.ls_set_tuning(22, v) == 1
        assert "position-major" in lib.ls_last_error().decode()
    assert lib.ls_set_tuning(22, 1) == 0


def _order(H, W, G, ntn):
    lib = _lib.load()
    out = (C.c_int32 * 4)()
    rows = []
    for b in range(H * W * G * ntn):
        assert lib.ls_conv_posmajor_tile(H, W, G, ntn, b, out) == 0
        rows.append(tuple(out))
    return rows


@pytest.mark.parametrize("n_img", [256, 272, 768])
@pytest.mark.parametrize("hw", [8, 4])
@pytest.mark.parametrize("ntn", [5, 10, 1])
def test_launch_order(hw, n_img, ntn):
    G = -(-n_img // 256)
    rows = _order(hw, hw, G, ntn)
    # a bijection onto (pos, g, tn)
    assert sorted(r[:3] for r in rows) == [(p, g, t) for p in range(hw * hw) for g in range(G) for t in range(ntn)]
    for pos, _, _, taps in rows:
        y, x = divmod(pos, hw)
        assert taps == (2 if y in (0, hw - 1) else 3) * (2 if x in (0, hw - 1) else 3)
    # block b runs on XCD b % 8: equal tap-unit totals to within one tile (9), heaviest tiles first
    tot = [sum(r[3] for r in rows[x::8]) for x in range(8)]
    assert max(tot) - min(tot) <= 9, tot
    for x in range(8):
        taps = [r[3] for r in rows[x::8]]
        assert taps == sorted(taps, reverse=True)
    # the column tiles of a (position, frame group) are neighbours on one XCD, but for the few
    # runs an XCD's share of a class cuts
    cut = sum(1 for x in range(8) for a, b in zip(rows[x::8], rows[x::8][1:]) if a[:2] != b[:2] and b[2] != 0)
    assert cut <= 8 * 3


def test_launch_order_refusals():
    lib = _lib.load()
    out = (C.c_int32 * 4)()
    for args in ((2, 8, 1, 1, 0), (8, 8, 0, 1, 0), (8, 8, 1, 0, 0), (8, 8, 1, 1, 64), (8, 8, 1, 1, -1)):
        assert lib.ls_conv_posmajor_tile(*args, out) == 1
    assert lib.ls_conv_posmajor_tile(8, 8, 1, 1, 0, None) == 1
