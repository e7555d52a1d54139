"""The yardstick of the per-element parity tests, tested on the CPU (tests/parity.py).

For every GEMM and attention shape of the GPU edge files an emulation of the kernel's
arithmetic (bf16 inputs, fp32 accumulation, round-to-nearest-even to bf16; for attention
also exp2, P rounded to bf16 and an fp32 row sum) must PASS the derived bound, and planted
defects of the kind tiled kernels really have must be REJECTED by it -- while the old
whole-output Frobenius ratio (conftest.rel_err < 1e-2) lets the GEMM defects through, which
is kept on record here."""
import math

import pytest
import torch
import torch.nn.functional as F

import parity as P
from conftest import rel_err

LOG2E = 1.4426950408889634


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def gemm_case(M, K, N, seed=0):
    """bf16-rounded x (M, K), w (N, K), residual (M, N); fp32 bias (N,); fp64 ref, mag."""
    x = P.bf16_round(rnd(M, K, seed=seed + 1))
    w = P.bf16_round(rnd(N, K, seed=seed + 2, scale=1 / math.sqrt(K)))
    b = rnd(N, seed=seed + 3, scale=0.1)
    res = P.bf16_round(rnd(M, N, seed=seed + 4))
    ref = P.f64(x) @ P.f64(w).T + P.f64(b) + P.f64(res)
    mag = P.f64(x).abs() @ P.f64(w).abs().T + P.f64(b).abs() + P.f64(res).abs()
    return x, w, b, res, ref, mag


def emulate_gemm(x, w, b, res, truncate=False):
    """fp32 accumulation (torch's fp32 matmul), fp32 epilogue, then bf16: RNE, or truncation."""
    acc = x @ w.T
    if b is not None:
        acc = acc + b
    acc = acc + res
    if truncate:
        return (acc.view(torch.int32) & -65536).view(torch.float32)
    return acc.to(torch.bfloat16).float()


# every ksize-1 shape of tests/test_gpu_edges_gemm.py (K = the real Cin: the padded tail adds
# exact zeros), its row-block / scalar-epilogue / epilogue-operand shapes, the 3x3 convs as the
# GEMMs they are (M = output pixels, K = 9 Cin), and the suite's own small shapes
GEMM_SHAPES = [(M, Cin, N) for Cin, _, N in P.EDGE_KN for M in P.EDGE_M] + \
    [(256, 320, 192), (512, 320, 192), (384, 640, 192), (129, 72, 20), (300, 320, 64),
     (105, 9 * 8, 40), (324, 9 * 72, 40), (1728, 9 * 128, 40), (1024, 9 * 128, 160), (512, 9 * 64, 8)] + \
    [(129, 320, 72), (200, 640, 320), (150, 72, 40), (64, 5120, 128)]


@pytest.mark.parametrize("M,K,N", GEMM_SHAPES)
def test_gemm_emulation_passes(M, K, N):
    x, w, b, res, ref, mag = gemm_case(M, K, N)
    bound = P.gemm_bound(ref, mag, K, torch.bfloat16)
    worst = P.assert_elementwise(emulate_gemm(x, w, b, res), ref, bound, where=dict(rows=16, cols=16))
    print(f"gemm emulation {M}x{K}x{N}: err/bound {worst:.3f}")
    assert worst > 0.2  # the bound is not vacuous: correct arithmetic uses a good part of it


@pytest.mark.parametrize("M,K,N", [(129, 320, 72), (200, 640, 320), (150, 72, 40)])
def test_gemm_truncation_rejected(M, K, N):
    assert K <= 640
    x, w, b, res, ref, mag = gemm_case(M, K, N)
    bound = P.gemm_bound(ref, mag, K, torch.bfloat16)
    got = emulate_gemm(x, w, b, res, truncate=True)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got, ref, bound)
    worst = float(((P.f64(got) - ref).abs() / bound).max())
    print(f"truncation {M}x{K}x{N}: err/bound {worst:.2f}, Frobenius {rel_err(got, ref):.2e}")
    assert 1.5 < worst < 2.1  # a full ulp instead of half of one
    assert rel_err(got, ref) < 1e-2  # on record: the Frobenius ratio passes it


@pytest.mark.parametrize("M,K,N", [(129, 320, 72), (200, 640, 320), (150, 72, 40)])
def test_gemm_dropped_bias_column_rejected(M, K, N):
    x, w, b, res, ref, mag = gemm_case(M, K, N)
    bound = P.gemm_bound(ref, mag, K, torch.bfloat16)
    col = int((b.abs() - 0.04).abs().argmin())  # an ordinary column (|bias| about 0.04)
    b2 = b.clone()
    b2[col] = 0.0
    got = emulate_gemm(x, w, b2, res)
    with pytest.raises(AssertionError, match=rf"col {col};"):
        P.assert_elementwise(got, ref, bound)
    worst = float(((P.f64(got) - ref).abs() / bound).max())
    print(f"dropped bias column {M}x{K}x{N}: err/bound {worst:.1f}, Frobenius {rel_err(got, ref):.2e}")
    assert worst > 5
    assert rel_err(got, ref) < 1e-2


def test_gemm_zeroed_row_rejected():
    """One output row of 16384 zeroed: 1 / sqrt(16384) = 0.8 % in the Frobenius ratio."""
    M, K, N = 16384, 64, 8
    x, w, b, res, ref, mag = gemm_case(M, K, N)
    bound = P.gemm_bound(ref, mag, K, torch.bfloat16)
    got = emulate_gemm(x, w, b, res)
    got[12345] = 0.0
    with pytest.raises(AssertionError, match=r"row 12345, .*row tile 771 of 16 rows"):
        P.assert_elementwise(got, ref, bound, where=dict(rows=16, cols=8))
    assert rel_err(got, ref) < 1e-2


def test_conv_border_tap_rejected():
    """A 3x3 conv whose left tap at one x = 0 pixel reads the pixel before it in memory (the
    last pixel of the row above) instead of the zero padding."""
    n, C, H, W, N = 3, 24, 32, 32, 40
    x = P.bf16_round(rnd(n, C, H, W, seed=11))
    w = P.bf16_round(rnd(N, C, 3, 3, seed=12, scale=1 / math.sqrt(9 * C)))
    b = rnd(N, seed=13, scale=0.1)
    ref = F.conv2d(P.f64(x), P.f64(w), P.f64(b), padding=1)
    mag = F.conv2d(P.f64(x).abs(), P.f64(w).abs(), P.f64(b).abs(), padding=1)
    bound = P.gemm_bound(ref, mag, 9 * C, torch.bfloat16)
    acc = F.conv2d(x, w, b, padding=1)
    good = acc.to(torch.bfloat16).float()
    P.assert_elementwise(good.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1))
    img, y = 1, 7
    acc[img, :, y, 0] += w[:, :, 1, 0] @ x[img, :, y - 1, W - 1]
    got = acc.to(torch.bfloat16).float()
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1))
    assert rel_err(got, ref) < 1e-2


# ---------------------------------------------------------------- attention
def emulate_attn(q, k, v, scale, q_prescaled, drop_key=None, sum_without=None):
    """The kernels' arithmetic in torch: scores in log2 units (Q pre-scaled and re-rounded to
    bf16 where the kernel does that, else the fp32 score scaled), exp2 relative to the row
    maximum, an fp32 row sum of the unrounded P, P rounded to bf16 for P V, o to bf16."""
    c2 = scale * LOG2E
    if q_prescaled:
        s = P.bf16_round(q * c2) @ k.transpose(-1, -2)
    else:
        s = (q @ k.transpose(-1, -2)) * c2
    if drop_key is not None:
        s[..., drop_key] = -float("inf")
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    lsum = p.clone()
    if sum_without is not None:
        lsum[..., sum_without] = 0.0
    o = (P.bf16_round(p) @ v) / lsum.sum(-1, keepdim=True)
    return o.to(torch.bfloat16).float()


def attn_shapes():
    out = [(name, d, heads, nq, nk, pre) for name, d, heads, nq, nk, pre in P.ATTN_CASES]
    out += [(f"seqm_d{d}_{n}x{n}", d, 8, n, n, False) for d, n in P.SEQM_CASES]
    return out


@pytest.mark.parametrize("name,d,heads,nq,nk,pre", attn_shapes())
@pytest.mark.parametrize("inputs", ["random", "needle"])
def test_attention_emulation_passes(name, d, heads, nq, nk, pre, inputs):
    if inputs == "needle":
        q, k, v = P.needle_qkv(2, heads, nq, nk, d, seed=5)
    else:
        q, k, v = (P.bf16_round(rnd(2, heads, n, d, seed=s)) for n, s in ((nq, 1), (nk, 2), (nk, 3)))
    scale = 1 / math.sqrt(d)
    ref, bound = P.attn_bound(q, k, v, scale, q_prescaled=pre)
    worst = P.assert_elementwise(emulate_attn(q, k, v, scale, pre), ref, bound)
    print(f"attention emulation {name} {inputs}: err/bound {worst:.3f}")
    if inputs == "needle":  # the needle rows put most of their weight on their tile-boundary key
        p = torch.softmax(scale * (P.f64(q) @ P.f64(k).transpose(-1, -2)), -1)
        for i, j in enumerate(P.needle_keys(nk)[:nq]):
            # (at d = 4 a short needle key makes a long query, and other random keys outscore it:
            # the weight is required from d = 36 on)
            wt = p[..., i, j]
            assert d < 36 or float(wt.min()) > 0.5, (i, j, wt)


@pytest.mark.parametrize("name,d,heads,nq,nk,pre", [c for c in attn_shapes() if c[4] > 1])
def test_attention_dropped_needle_key_rejected(name, d, heads, nq, nk, pre):
    q, k, v = P.needle_qkv(1, heads, nq, nk, d, seed=5)
    scale = 1 / math.sqrt(d)
    ref, bound = P.attn_bound(q, k, v, scale, q_prescaled=pre)
    p = torch.softmax(scale * (P.f64(q) @ P.f64(k).transpose(-1, -2)), -1)
    for i, j in enumerate(P.needle_keys(nk)[:nq]):
        got = emulate_attn(q, k, v, scale, pre, drop_key=j)
        ratio = ((P.f64(got) - ref).abs() / bound)[..., i, :].amax(-1)  # per (batch, head), the needle row
        heavy = p[..., i, j] > 0.5  # where the dropped key carries most of the row (all of them from d = 36)
        assert bool(heavy.all()) or d < 36
        if bool(heavy.any()):
            assert float(ratio[heavy].min()) > 10, (name, j, ratio)
            with pytest.raises(AssertionError, match="err/bound"):
                P.assert_elementwise(got, ref, bound)


@pytest.mark.parametrize("name,d,heads,nq,nk,pre", [c for c in attn_shapes() if c[4] > 1])
def test_attention_row_sum_missing_key_rejected(name, d, heads, nq, nk, pre):
    q, k, v = P.needle_qkv(1, heads, nq, nk, d, seed=5)
    scale = 1 / math.sqrt(d)
    ref, bound = P.attn_bound(q, k, v, scale, q_prescaled=pre)
    j = P.needle_keys(nk)[-1]  # the last key: the partial tile's edge
    got = emulate_attn(q, k, v, scale, pre, sum_without=j)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got, ref, bound)


# ---------------------------------------------------------------- activations, elementwise
@pytest.mark.parametrize("kind", ["gelu", "silu", "geglu"])
def test_activation_emulation_passes(kind):
    M, K, N = 129, 320, 64
    x, w, b, res, _, _ = gemm_case(M, K, N)
    pre = P.f64(x) @ P.f64(w).T + P.f64(b)
    mag = P.f64(x).abs() @ P.f64(w).abs().T + P.f64(b).abs()
    b_pre = P.gemm_bound(pre, mag, K, None)
    acc = x @ w.T + b
    if kind == "geglu":
        ref, bound = P.geglu_bound(pre[:, :32], b_pre[:, :32], pre[:, 32:], b_pre[:, 32:], torch.bfloat16)
        got = (acc[:, :32] * F.gelu(acc[:, 32:])).to(torch.bfloat16).float()
    else:
        ref, bound = P.act_bound(kind, pre, b_pre, torch.bfloat16)
        got = (F.gelu(acc) if kind == "gelu" else F.silu(acc)).to(torch.bfloat16).float()
    worst = P.assert_elementwise(got, ref, bound)
    print(f"{kind} emulation: err/bound {worst:.3f}")
    with pytest.raises(AssertionError):  # the activation left out
        P.assert_elementwise((acc[:, :32] if kind == "geglu" else acc).to(torch.bfloat16).float(), ref, bound)


# ---------------------------------------------------------------- guard bands
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
def test_guard_band_detects_one_stray_element(dtype):
    g = P.guarded((3, 5, 20), pitch=28, pad_rows=2, dtype=dtype)
    assert tuple(g.view.shape) == (3, 5, 20) and g.view.stride() == (5 * 28, 28, 1)
    P.assert_guard_intact(g)
    g.view.copy_(torch.ones(3, 5, 20).to(dtype))  # the whole view may be written
    P.assert_guard_intact(g)
    bits = g.buf.view(g.bits_dtype)
    first = (g.view.data_ptr() - g.buf.data_ptr()) // g.buf.element_size()
    for stray in (first - 1, first + 20, first + 27, first + 14 * 28 + 20, 0, bits.numel() - 1):
        keep = bits[stray].clone()
        bits[stray] = 0
        with pytest.raises(AssertionError, match="outside the requested view"):
            P.assert_guard_intact(g)
        bits[stray] = keep
    P.assert_guard_intact(g)


def test_guard_band_offset_view_and_unwritten_elements():
    g = P.guarded((4, 16), pitch=24, dtype=torch.bfloat16, offset=2)
    assert (g.view.data_ptr() - g.buf.data_ptr()) % 16 == 4  # 16-byte alignment broken on purpose
    ref = torch.zeros(4, 16, dtype=torch.float64)
    with pytest.raises(AssertionError, match="err/bound"):  # an element never written is a NaN
        P.assert_elementwise(g.view, ref, torch.ones_like(ref))
    g.view.zero_()
    assert P.assert_elementwise(g.view, ref, torch.ones_like(ref)) == 0.0
    P.assert_guard_intact(g)


def test_assert_unchanged():
    x = rnd(7, 9).to(torch.bfloat16)
    snap = P.snapshot(x)
    P.assert_unchanged(x, snap)
    x.view(torch.int16)[3, 4] ^= 1  # one bit
    with pytest.raises(AssertionError, match="changed"):
        P.assert_unchanged(x, snap)
