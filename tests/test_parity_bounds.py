"""The yardstick of the per-element parity tests, tested on the CPU (tests/parity.py).

For every GEMM and attention shape of the GPU edge files an emulation of the kernel's
arithmetic (bf16 inputs, fp32 accumulation, round-to-nearest-even to bf16; for attention
also exp2, P rounded to bf16 and an fp32 row sum) must PASS the derived bound, and planted
defects of the kind tiled kernels really have must be REJECTED by it -- while the old
whole-output Frobenius ratio (conftest.rel_err < 1e-2) lets the GEMM defects through, which
is kept on record here.  The fp8 attention (ls_attention_fp8) has its own restatement at the end: a
walk of the keys in attn8_kernel's tile order, which must pass attn_fp8_bound on every case of the
GPU file, and seven planted defects that must leave it."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import parity as P
from conftest import rel_err
from oracle import fp8_cpu as Q8

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


# ---------------------------------------------------------------- LayerNorm / row statistics
def emulate_ln(x, gamma, beta, pe_row, eps, order="lanes", truncate=False, stats_only=False):
    """layernorm_kernel in fp32: "lanes" sums as the kernel does (lane sub owns chunks sub + 16 q
    of 8 channels, then a 16-lane xor tree), "pairwise" is torch's own fp32 sum."""
    rows, C = x.shape

    def rsum(v):
        if order == "pairwise":
            return v.sum(-1, keepdim=True)
        CC = C // 8
        pad = torch.zeros(rows, (-CC) % 16 * 8)
        t = torch.cat([v, pad], 1).reshape(rows, -1, 16, 8)  # (q, lane, j)
        acc = torch.zeros(rows, 16)
        for q in range(t.shape[1]):
            for j in range(8):
                acc = acc + t[:, q, :, j]
        for o in (8, 4, 2, 1):
            acc = acc + acc[:, torch.arange(16) ^ o]
        return acc[:, :1]

    mean = rsum(x) / C
    d = x - mean
    rstd = torch.rsqrt(rsum(d * d) / C + eps)
    if stats_only:
        return torch.cat([mean, rstd], 1)
    o = d * rstd * gamma + beta
    if pe_row is not None:
        o = o + pe_row
    if truncate:
        return (o.view(torch.int32) & -65536).view(torch.float32)
    return o.to(torch.bfloat16).float()


@pytest.mark.parametrize("C", P.LN_C)
@pytest.mark.parametrize("mean_sigmas", [0, 30])
@pytest.mark.parametrize("order", ["lanes", "pairwise"])
def test_layernorm_emulation_passes(C, mean_sigmas, order):
    for rows in P.LN_ROWS:
        x, gamma, beta, pe = P.ln_case(rows, C, mean_sigmas)
        for pe_row in (None, P.ln_pe_rows(pe, rows)):
            ref, bound = P.ln_bound(x, gamma, beta, pe_row, P.LN_EPS, torch.bfloat16)
            worst = P.assert_elementwise(emulate_ln(x, gamma, beta, pe_row, P.LN_EPS, order), ref, bound)
            P.assert_elementwise(ref.to(torch.bfloat16), ref, bound)  # the rounded reference alone
        sref, sbound = P.row_stats_bound(x, P.LN_EPS)
        ws = P.assert_elementwise(emulate_ln(x, gamma, beta, None, P.LN_EPS, order, stats_only=True), sref, sbound)
        P.assert_elementwise(sref.float(), sref, sbound)
    print(f"layernorm emulation C {C} mean {mean_sigmas} {order}: err/bound {worst:.3f}, stats {ws:.3f}")


def test_layernorm_neighbour_statistics_rejected():
    rows, C = 257, 320
    _, gamma, beta, _ = P.ln_case(rows, C, 0)
    x = P.bf16_round(rnd(rows, C, seed=3))  # rows of one distribution: the neighbour's statistics are close
    ref, bound = P.ln_bound(x, gamma, beta, None, P.LN_EPS, torch.bfloat16)
    got = emulate_ln(x, gamma, beta, None, P.LN_EPS)
    st = emulate_ln(x, gamma, beta, None, P.LN_EPS, stats_only=True)
    r = 130
    got[r] = ((x[r] - st[r + 1, 0]) * st[r + 1, 1] * gamma + beta).to(torch.bfloat16).float()
    with pytest.raises(AssertionError, match=rf"row {r},"):
        P.assert_elementwise(got, ref, bound)
    assert rel_err(got, ref) < 1e-2
    sref, sbound = P.row_stats_bound(x, P.LN_EPS)
    st[r] = st[r + 1]
    with pytest.raises(AssertionError, match=rf"row {r},"):
        P.assert_elementwise(st, sref, sbound)


def test_layernorm_wrong_frame_pe_rejected():
    """The first row after a frame boundary still gets the previous frame's pe row."""
    rows, C = 6000, 136
    x, gamma, beta, pe = P.ln_case(rows, C, 0)
    pe_row = P.ln_pe_rows(pe, rows)
    ref, bound = P.ln_bound(x, gamma, beta, pe_row, P.LN_EPS, torch.bfloat16)
    bad = pe_row.clone()
    r = 5 * P.LN_PE_RPF
    bad[r] = pe_row[r - 1]
    got = emulate_ln(x, gamma, beta, bad, P.LN_EPS)
    with pytest.raises(AssertionError, match=rf"row {r},"):
        P.assert_elementwise(got, ref, bound)
    assert rel_err(got, ref) < 1e-2


@pytest.mark.parametrize("C", [136, 320])
def test_layernorm_truncation_rejected(C):
    x, gamma, beta, _ = P.ln_case(33, C, 0)
    ref, bound = P.ln_bound(x, gamma, beta, None, P.LN_EPS, torch.bfloat16)
    got = emulate_ln(x, gamma, beta, None, P.LN_EPS, truncate=True)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got, ref, bound)
    assert rel_err(got, ref) < 1e-2


def test_ln_propagate_covers_a_perturbed_input():
    """|d a| of a = (x - mu) r under |dx| <= b, for the worst-sign and for random perturbations."""
    x, _, _, _ = P.ln_case(33, 320, 3)
    x = P.f64(x)
    b = 2.0 ** -8 * x.abs()

    def norm(v):
        d = v - v.mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + P.LN_EPS)
        return d * r, r

    a, r = norm(x)
    bound = P.ln_propagate(a, r, b) * P.SLACK
    worst = 0.0
    for seed, sign in enumerate([torch.sign(a), -torch.sign(a), None, None, None]):
        s = sign if sign is not None else torch.sign(rnd(*x.shape, seed=seed).double())
        worst = max(worst, P.assert_elementwise(norm(x + s * b)[0], a, bound))
    print(f"ln_propagate: err/bound {worst:.3f}")
    assert worst > 0.2


# ---------------------------------------------------------------- GroupNorm statistics
def emulate_gn_stats(x, groups, eps, gamma, beta, nsplit, R, order="forward", naive_group=None):
    """gn_stats_kernel: per (split, thread row r, channel) an fp32 chain over every R-th row of
    the split of d = x - k_g and d * d ("fma": the square added unrounded), fp64 from there on.
    naive_group: that group's variance as fp32 E[x^2] - E[x]^2 of unshifted fp32 sums."""
    S, pps, C = x.shape
    cpg = C // groups
    k = x[:, :1, ::cpg].repeat_interleave(cpg, 2)
    d = x - k
    S1 = torch.zeros(S, C, dtype=torch.float64)
    S2 = torch.zeros(S, C, dtype=torch.float64)
    for split in range(nsplit):
        p0, p1 = pps * split // nsplit, pps * (split + 1) // nsplit
        seg = d[:, p0:p1]
        n_t = -(-(p1 - p0) // R)
        seg = torch.cat([seg, torch.zeros(S, n_t * R - (p1 - p0), C)], 1).reshape(S, n_t, R, C)
        a1, a2 = torch.zeros(S, R, C), torch.zeros(S, R, C)
        ts = range(n_t) if order != "backward" else range(n_t - 1, -1, -1)
        for t in ts:
            a1 = a1 + seg[:, t]
            a2 = (a2.double() + seg[:, t].double() ** 2).float() if order == "fma" else a2 + seg[:, t] * seg[:, t]
        S1 += a1.double().sum(1)
        S2 += a2.double().sum(1)
    n = float(pps * cpg)
    m1 = S1.reshape(S, groups, cpg).sum(-1) / n
    var = (S2.reshape(S, groups, cpg).sum(-1) / n - m1 * m1).clamp_min(0.0)
    mean = (x[:, 0, ::cpg].double() + m1).float()
    rstd = (1.0 / torch.sqrt(var + eps)).float()
    if naive_group is not None:
        xg = x.reshape(S, pps, groups, cpg)[:, :, naive_group]
        m = xg.sum((1, 2)) / n
        v = (xg * xg).sum((1, 2)) / n - m * m
        rstd[:, naive_group] = torch.rsqrt(v.clamp_min(0.0) + eps)
    sc = gamma * rstd.repeat_interleave(cpg, 1)
    return sc, beta - mean.repeat_interleave(cpg, 1) * sc


def gn_check(got, ref, bound, name):
    ws = P.assert_elementwise(got[0], ref[0], bound[0], name=f"{name} scale")
    return max(ws, P.assert_elementwise(got[1], ref[1], bound[1], name=f"{name} shift"))


@pytest.mark.parametrize("name,C1,C2,groups,n_samples,pps", P.GN_CASES, ids=[c[0] for c in P.GN_CASES])
@pytest.mark.parametrize("mean_sigmas", P.GN_MEANS)
def test_groupnorm_stats_emulation_passes(name, C1, C2, groups, n_samples, pps, mean_sigmas):
    C = C1 + C2
    x, gamma, beta = P.gn_case(C1, C2, n_samples, pps, mean_sigmas)
    R = P.gn_R(C)
    ns = P.gn_nsplit(n_samples, pps, C)
    worst = 0.0
    # the launcher's split with three summation orders, and the extreme splits (one block per
    # sample: the longest per-thread chains; one block per 8 R rows, at most 4096: the shortest)
    runs = [(ns, o) for o in ("forward", "backward", "fma")]
    runs += [(e, "forward") for e in {1, max(1, min(pps // (8 * R), 4096))} - {ns} if C * pps <= 4096 * 320]
    for nsplit, order in runs:
        ref, bound = P.gn_stats_bound(x, groups, P.GN_EPS, gamma, beta, nsplit, R)
        got = emulate_gn_stats(x, groups, P.GN_EPS, gamma, beta, nsplit, R, order)
        worst = max(worst, gn_check(got, ref, bound, f"{name} nsplit {nsplit} {order}"))
    gn_check((ref[0].float(), ref[1].float()), ref, bound, f"{name} rounded reference")
    print(f"groupnorm stats emulation {name} mean {mean_sigmas}: err/bound {worst:.3f}")


def test_groupnorm_unshifted_variance_rejected():
    """One group's variance as E[x^2] - E[x]^2 in fp32 at mean / std = 30: 900 parts of cancellation."""
    C, groups, S, pps = 320, 32, 3, 4096
    x, gamma, beta = P.gn_case(C, 0, S, pps, 30)
    R, ns = P.gn_R(C), P.gn_nsplit(S, pps, C)
    ref, bound = P.gn_stats_bound(x, groups, P.GN_EPS, gamma, beta, ns, R)
    got = emulate_gn_stats(x, groups, P.GN_EPS, gamma, beta, ns, R, naive_group=17)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got[0], ref[0], bound[0])
    ratio = (P.f64(got[0]) - ref[0]).abs() / bound[0]
    cols = sorted(set(torch.nonzero(ratio > 1.0)[:, 1].tolist()))
    assert cols and all(c // 10 == 17 for c in cols), cols
    print(f"unshifted variance: err/bound {float(ratio.max()):.1f}, Frobenius {rel_err(got[0], ref[0]):.2e}")
    assert rel_err(got[0], ref[0]) < 1e-2 and rel_err(got[1], ref[1]) < 1e-2


@pytest.mark.parametrize("cpg,slots,C1,C2", P.GN_COLSUM_CASES)
def test_groupnorm_colsum_emulation_passes(cpg, slots, C1, C2):
    cs1, cs2, gamma, beta = P.gn_colsum_case(cpg, slots, C1, C2)
    cs = cs1 if cs2 is None else torch.cat([cs1, cs2], 2)
    ref, bound = P.gn_colsum_bound(cs, slots, 32, P.GN_EPS, gamma, beta)
    n = float(slots * 128 * cpg)
    t = cs.double().reshape(3, slots, 2, 32, cpg)
    worst = 0.0
    for flip in (False, True):  # two fp64 summation orders
        tt = t.flip(1, 4) if flip else t
        s1, s2 = tt[:, :, 0].sum((1, 3)), tt[:, :, 1].sum(3).sum(1)
        mean = s1 / n
        rstd = (1.0 / torch.sqrt((s2 / n - mean * mean).clamp_min(0.0) + P.GN_EPS)).float()
        sc = gamma * rstd.repeat_interleave(cpg, 1)
        sh = beta - mean.float().repeat_interleave(cpg, 1) * sc
        worst = max(worst, gn_check((sc, sh), ref, bound, "colsum finalize"))
    # the bound is not vacuous: a variance off by 1e-5 of itself is outside it
    bad = gamma * (1.0 / torch.sqrt(((s2 / n - mean * mean) * (1 + 1e-5)) + P.GN_EPS)).float().repeat_interleave(cpg, 1)
    with pytest.raises(AssertionError):
        P.assert_elementwise(bad, ref[0], bound[0])
    print(f"groupnorm colsum emulation cpg {cpg} slots {slots} C1 {C1}: err/bound {worst:.3f}")


@pytest.mark.parametrize("M", [128, 384])
@pytest.mark.parametrize("N", [8, 40, 320])
def test_colsum_emulation_passes(M, N):
    y = P.bf16_round(rnd(M, N, seed=M + N) + 2.0)
    ref, bound = P.colsum_bound(y)
    t = y.reshape(M // 128, 128, N)
    for order in ("kernel", "pairwise"):
        if order == "kernel":  # 8 row lanes of 16 rows each, then merged in turn
            s1, s2 = torch.zeros(M // 128, 8, N), torch.zeros(M // 128, 8, N)
            for r in range(16):
                s1, s2 = s1 + t[:, 8 * r:8 * r + 8], (s2.double() + t[:, 8 * r:8 * r + 8].double() ** 2).float()
            a1, a2 = s1[:, 0], s2[:, 0]
            for k in range(1, 8):
                a1, a2 = a1 + s1[:, k], a2 + s2[:, k]
        else:
            a1, a2 = t.sum(1), (t * t).sum(1)
        worst = P.assert_elementwise(torch.stack([a1, a2], 1), ref, bound)
    P.assert_elementwise(ref.float(), ref, bound)
    got = torch.stack([a1, a2], 1)
    got[0, 0, N - 1] -= t[0, 127, N - 1]  # one row left out of one column
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got, ref, bound)
    print(f"colsum emulation {M}x{N}: err/bound {worst:.3f}")


@pytest.mark.parametrize("name,C1,C2,S,pps", P.GN_APPLY_CASES, ids=[c[0] for c in P.GN_APPLY_CASES])
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_apply_emulation_passes(name, C1, C2, S, pps, silu):
    x, scale, shift = apply_case(C1, C2, S, pps)
    ref, bound = P.gn_apply_bound(x, scale, shift, silu)
    pre = x * scale[:, None] + shift[:, None]
    got = (F.silu(pre) if silu else pre).to(torch.bfloat16).float()
    worst = P.assert_elementwise(got, ref, bound)
    P.assert_elementwise(ref.to(torch.bfloat16), ref, bound)
    print(f"groupnorm apply emulation {name} silu {silu}: err/bound {worst:.3f}")


def apply_case(C1, C2, S, pps, seed=0, mean_sigmas=2):
    """x and the fp32 (scale, shift) of its own 32-group GroupNorm (so neighbouring samples have
    nearly equal affines, as in the model)."""
    x, gamma, beta = P.gn_case(C1, C2, S, pps, mean_sigmas, seed=seed)
    (sc, sh), _ = P.gn_stats_bound(x, 32, P.GN_EPS, gamma, beta, 1, 1)
    return x, sc.float(), sh.float()


def test_groupnorm_apply_previous_sample_affine_rejected():
    """The first block pass (ppb = 16 pixels at C = 128) of sample 1 with sample 0's (scale, shift)."""
    C, S, pps = 128, 3, 1024
    x, scale, shift = apply_case(C, 0, S, pps, mean_sigmas=0)  # samples of one distribution: nearly equal affines
    ref, bound = P.gn_apply_bound(x, scale, shift, True)
    pre = x * scale[:, None] + shift[:, None]
    pre[1, :16] = x[1, :16] * scale[0] + shift[0]
    got = F.silu(pre).to(torch.bfloat16).float()
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got.reshape(S * pps, C), ref.reshape(S * pps, C), bound.reshape(S * pps, C))
    ratio = ((P.f64(got) - ref).abs() / bound).reshape(S * pps, C).amax(1)
    bad = torch.nonzero(ratio > 1.0).reshape(-1)
    assert int(bad.min()) >= pps and int(bad.max()) < pps + 16
    print(f"previous sample's affine: err/bound {float(ratio.max()):.1f}, Frobenius {rel_err(got, ref):.2e}")
    assert rel_err(got, ref) < 1e-2


# ---------------------------------------------------------------- fused FeedForward kernels
def bfr(t):
    return t.to(torch.bfloat16).float()


def mm(a, w, order):
    """a w^T in fp32: torch's own order, or 32-wide k-steps accumulated in turn (the MFMA loop)."""
    if order == "torch":
        return a @ w.T
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in range(0, a.shape[1], 32):
        acc = acc + a[:, k:k + 32] @ w[:, k:k + 32].T
    return acc


def ff_body(a, c, order, swap=None, drop=None):
    """GEGLU(W1 a + b1) W2^T in fp32 with G rounded to bf16; swap = two inner columns of W2
    exchanged (a packing permutation off by one slot); drop = (rows, chunk): that 32-column
    inner chunk never accumulated for those rows."""
    pre = mm(a, c["w1g"], order) + c["b1f"].float()
    G = bfr(pre[:, :P.FF_INNER] * F.gelu(pre[:, P.FF_INNER:]))
    w2 = c["w2r"]
    if swap is not None:
        w2 = w2.clone()
        w2[:, list(swap)] = w2[:, list(reversed(swap))]
    if drop is not None:
        G = G.clone()
        G[drop[0], 32 * drop[1]:32 * drop[1] + 32] = 0.0
    return mm(G, w2, order)


def emulate_ff(c, order="torch", **defect):
    x, st = c["x"], c["stats"]
    a = bfr(torch.addcmul(-(st[:, :1] * st[:, 1:]), x, st[:, 1:]))
    return bfr(ff_body(a, c, order, **defect) + c["b2"] + x)


def ff_ref(c):
    return P.ff_bound(c["x"], c["stats"], c["w1g"], c["b1f"], c["b1_mag"], c["w2r"], c["b2"])


@pytest.mark.parametrize("M", P.FF_M)
def test_feedforward_emulation_passes(M):
    c = P.ff_case(M)
    ref, bound = ff_ref(c)
    for order in ("torch", "ksteps"):
        worst = P.assert_elementwise(emulate_ff(c, order), ref, bound)
    P.assert_elementwise(ref.to(torch.bfloat16), ref, bound)
    print(f"feedforward emulation M {M}: err/bound {worst:.3f}")


def _rejected(got, ref, bound, what):
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got, ref, bound)
    worst = float(((P.f64(got) - ref).abs() / bound).max())
    fro = rel_err(got, ref)
    print(f"{what}: err/bound {worst:.1f}, Frobenius {fro:.2e}")
    assert fro < 1e-2  # on record: the Frobenius ratio passes it
    return worst


@pytest.mark.parametrize("swap", [(1, 2), (33, 34), (29, 30), (1277, 1278)])
def test_feedforward_swapped_w2_columns_rejected(swap):
    c = P.ff_case(300)
    ref, bound = ff_ref(c)
    _rejected(emulate_ff(c, swap=swap), ref, bound, f"W2 inner columns {swap} swapped")


@pytest.mark.parametrize("swap", [(3, 4), (15, 16), (31, 32), (1278, 1279)])
def test_feedforward_swapped_needle_columns_far_outside(swap):
    """A swap that involves a needle column (8 times the weight) is two orders outside."""
    c = P.ff_case(129)
    ref, bound = ff_ref(c)
    worst = float(((P.f64(emulate_ff(c, swap=swap)) - ref).abs() / bound).max())
    print(f"W2 needle columns {swap} swapped: err/bound {worst:.1f}")
    assert worst > 50


@pytest.mark.parametrize("chunk", [5, 17, 38])
def test_feedforward_dropped_chunk_rejected(chunk):
    """One wave (16 rows of 1200) skips one 32-column inner chunk."""
    c = P.ff_case(1200)
    ref, bound = ff_ref(c)
    _rejected(emulate_ff(c, drop=(slice(640, 656), chunk)), ref, bound, f"inner chunk {chunk} dropped for 16 rows")


@pytest.mark.parametrize("k", P.FF_W1_NEEDLES)
def test_feedforward_dropped_w1_k_column_rejected(k):
    c = P.ff_case(300)
    ref, bound = ff_ref(c)
    c2 = dict(c, w1g=c["w1g"].clone())
    c2["w1g"][:, k] = 0.0
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(emulate_ff(c2), ref, bound)


def emulate_ff_chain(c, order="torch"):
    C = P.FF_C
    h2 = bfr(mm(c["o"], c["wor"], order) + c["bo"] + c["h1"])
    mean = h2.sum(1, keepdim=True) * (1.0 / C)
    d = h2 - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) * (1.0 / C) + 1e-5)
    a = bfr(d * rstd)
    y = bfr(ff_body(a, c, order) + (h2 + c["b2"]))
    z = bfr(mm(y, c["wpr"], order) + c["bp"] + c["xb"])
    t = z.reshape(-1, 128, C)
    return z, torch.stack([t.sum(1), (t * t).sum(1)], 1)


def ff_chain_ref(c):
    return P.ff_chain_bound(c["o"], c["h1"], c["xb"], c["wor"], c["bo"], c["w1g"], c["b1f"], c["b1_mag"], c["w2r"],
                            c["b2"], c["wpr"], c["bp"], 1e-5)


@pytest.mark.parametrize("M", P.FF_CHAIN_M)
def test_ff_chain_emulation_passes(M):
    c = P.ff_chain_case(M)
    ref, bound = ff_chain_ref(c)
    for order in ("torch", "ksteps"):
        z, cs = emulate_ff_chain(c, order)
        worst = P.assert_elementwise(z, ref, bound)
        wc = P.assert_elementwise(cs, *P.colsum_bound(z))
    P.assert_elementwise(ref.to(torch.bfloat16), ref, bound)
    print(f"ff_chain emulation M {M}: err/bound {worst:.3f}, column sums {wc:.3f}")
    # a proj_out that forgets the block input on one row is outside the bound
    z[77] = z[77] - c["xb"][77]
    with pytest.raises(AssertionError, match="row 77,"):
        P.assert_elementwise(z, ref, bound)


# ---------------------------------------------------------------- fused attention kernels
def emulate_xattn(c, L, order="torch", leak_rows=None, drop_tail=None):
    """xattn_fused_kernel in fp32 / bf16.  leak_rows: for those query rows one zero key >= L stays
    unmasked (score 0, value 0: only the row sum grows); drop_tail = (rows, head): dims 32 .. 39
    of that head never reach the out-projection for those rows."""
    C, H, D, hw = 320, 8, 40, P.XA_HW
    x, st = c["x"], c["stats"]
    M = x.shape[0]
    n = M // hw
    a = bfr(torch.addcmul(-(st[:, :1] * st[:, 1:]), x, st[:, 1:]))
    q = bfr(mm(a, c["wqr"], order) + c["bqf"].float())
    q4 = q.reshape(n, hw, H, D).permute(0, 2, 1, 3)
    k = c["kv"][:, :C].reshape(n, L, H, D).permute(0, 2, 1, 3)
    v = c["kv"][:, C:].reshape(n, L, H, D).permute(0, 2, 1, 3)
    s = q4 @ k.transpose(-1, -2)
    mx = s.amax(-1, keepdim=True)
    leak = torch.zeros(M, dtype=torch.bool)
    if leak_rows is not None:
        leak[leak_rows] = True
        mx = torch.where(leak.reshape(n, 1, hw, 1), mx.clamp_min(0.0), mx)
    p = bfr(torch.exp2(s - mx))
    l = p.sum(-1, keepdim=True) + torch.where(leak.reshape(n, 1, hw, 1), bfr(torch.exp2(-mx)), torch.zeros(()))
    o = bfr((p @ v) * (1.0 / l)).permute(0, 2, 1, 3).reshape(M, C)
    if drop_tail is not None:
        o = o.clone()
        o[drop_tail[0], 40 * drop_tail[1] + 32:40 * drop_tail[1] + 40] = 0.0
    y = bfr(mm(o, c["wor"], order) + c["bo"] + x)
    t = y.reshape(M, 10, 32)  # statistics of the stored rows: fp32 per 32-column chunk, then fp64
    s1, s2 = t.sum(-1).double().sum(-1) / C, (t * t).sum(-1).double().sum(-1) / C
    stats = torch.stack([s1, 1.0 / torch.sqrt((s2 - s1 * s1).clamp_min(0.0) + 1e-5)], 1).float()
    return y, stats


def xattn_ref(c, L):
    return P.xattn_bound(c["x"], c["stats"], c["wqr"], c["bqf"], c["bq_mag"], c["kv"], L, P.XA_HW, c["wor"], c["bo"])


@pytest.mark.parametrize("L", P.XA_L)
def test_xattn_emulation_passes(L):
    c = P.xattn_case(L)
    ref, bound = xattn_ref(c, L)
    for order in ("torch", "ksteps"):
        y, st = emulate_xattn(c, L, order)
        worst = P.assert_elementwise(y, ref, bound)
        ws = P.assert_elementwise(st, *P.stored_row_stats_bound(y, 1e-5))
    P.assert_elementwise(ref.to(torch.bfloat16), ref, bound)
    print(f"xattn emulation L {L}: err/bound {worst:.3f}, statistics {ws:.3f}")


@pytest.mark.parametrize("L", [5, 7])
def test_xattn_unmasked_key_rejected(L):
    """One query row keeps key slot L (zeros in LDS) in the softmax."""
    c = P.xattn_case(L)
    ref, bound = xattn_ref(c, L)
    y, _ = emulate_xattn(c, L, leak_rows=slice(150, 151))
    _rejected(y, ref, bound, f"key {L} of {L} left unmasked for one row")


@pytest.mark.parametrize("L,head", [(50, 0), (50, 7), (64, 3)])
def test_xattn_dropped_head_tail_rejected(L, head):
    """Eight rows lose dims 32 .. 39 of one head (the third k-step of its head pair)."""
    c = P.xattn_case(L)
    ref, bound = xattn_ref(c, L)
    y, _ = emulate_xattn(c, L, drop_tail=(slice(272, 280), head))
    _rejected(y, ref, bound, f"head {head} dims 32..39 dropped in the out-projection")


def emulate_tattn(c, C, S, Fr, order="torch", leak=None):
    """tattn_fused_kernel in fp32 / bf16; leak = (sample, pixel, head): frame Fr (a zero row,
    whose LayerNorm is beta + pe[Fr]) stays in that pixel's softmax for that head."""
    H, B = 8, P.TA_SAMPLES
    D = C // H
    x = c["x"]
    frame = (torch.arange(x.shape[0]) // S) % Fr
    mean = x.sum(1, keepdim=True) * (1.0 / C)
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) * (1.0 / C) + 1e-5)
    ln = bfr(torch.addcmul(c["bpe"][frame], d * rstd, c["gamma"]))
    if leak is not None:  # one more row per (sample, pixel): frame Fr of every pixel, used for one only
        Fe = Fr + 1
        lne = torch.zeros(B, Fe, S, C)
        lne[:, :Fr] = ln.reshape(B, Fr, S, C)
        lne[:, Fr] = bfr(c["bpe"][Fr])
        ln, Fk = lne.reshape(B * Fe * S, C), Fe
    else:
        Fk = Fr
    q, k, v = (bfr(mm(ln, w, order)).reshape(B, Fk, S, H, D).permute(0, 2, 3, 1, 4) for w in (c["wqp"], c["wkr"], c["wvr"]))
    s = q @ k.transpose(-1, -2)  # (B, S, H, Fk, Fk), log2 units
    if leak is not None:
        mask = torch.ones(B, S, H, dtype=torch.bool)
        mask[leak] = False
        s[..., Fr] = torch.where(mask[..., None], torch.full_like(s[..., Fr], -float("inf")), s[..., Fr])
    p = bfr(torch.exp2(s - s.amax(-1, keepdim=True)))
    o = bfr((p @ v) * (1.0 / p.sum(-1, keepdim=True)))[:, :, :, :Fr]
    return o.permute(0, 3, 1, 2, 4).reshape(B * Fr * S, C)


def tattn_ref(c, S, Fr):
    return P.tattn_bound(c["x"], c["gamma"], c["bpe"], c["wqp"], c["wkr"], c["wvr"], P.TA_SAMPLES, Fr, S, 8, 1e-5)


@pytest.mark.parametrize("C,S", P.TA_CASES)
@pytest.mark.parametrize("Fr", P.TA_F)
def test_tattn_emulation_passes(C, S, Fr):
    c = P.tattn_case(C, S, Fr)
    ref, bound = tattn_ref(c, S, Fr)
    for order in ("torch", "ksteps"):
        worst = P.assert_elementwise(emulate_tattn(c, C, S, Fr, order), ref, bound)
    P.assert_elementwise(ref.to(torch.bfloat16), ref, bound)
    print(f"temporal attention emulation C {C} F {Fr}: err/bound {worst:.3f}")


@pytest.mark.parametrize("C,S,Fr", [(320, 64, 5), (640, 64, 7), (640, 64, 5)])
def test_tattn_unmasked_frame_rejected(C, S, Fr):
    c = P.tattn_case(C, S, Fr)
    ref, bound = tattn_ref(c, S, Fr)
    got = emulate_tattn(c, C, S, Fr, leak=(1, 37, 4))
    P.assert_elementwise(emulate_tattn(c, C, S, Fr), ref, bound)
    _rejected(got, ref, bound, f"frame {Fr} of {Fr} left unmasked for one pixel and head")


# ---------------------------------------------------------------- attn_bound's input-error terms
def test_attn_bound_input_errors_cover_a_perturbation():
    q, k, v = (P.bf16_round(rnd(2, 2, n, 40, seed=s)) for n, s in ((33, 1), (20, 2), (20, 3)))
    scale = 1 / math.sqrt(40)
    ref0, b0 = P.attn_bound(q, k, v, scale)
    bq, bk, bv = (2.0 ** -8 * t.abs() for t in (q, k, v))
    ref, b = P.attn_bound(q, k, v, scale, q_err=bq, k_err=bk, v_err=bv)
    assert torch.equal(ref, ref0) and bool((b > b0).all())
    assert torch.equal(P.attn_bound(q, k, v, scale, q_err=0 * bq, k_err=0 * bk, v_err=0 * bv)[1], b0)
    worst = 0.0
    for seed in range(4):
        sg = [torch.sign(rnd(*t.shape, seed=10 * seed + i)) for i, t in enumerate((q, k, v))]
        got = P.attn_bound(q + sg[0] * bq, k + sg[1] * bk, v + sg[2] * bv, scale)[0]
        worst = max(worst, P.assert_elementwise(got, ref, b - b0 * (1 - 2.0 ** -6)))  # the input terms alone
    print(f"attn_bound input errors: err/bound {worst:.3f}")
    assert worst > 0.05


# ---------------------------------------------------------------- fused conv features
# (tests/test_gpu_edges_conv_fused.py): the LayerNorm fold in both arithmetics, the row statistics
# and column sums of the stored output, the affine folded into the row-block A rows
def trunc_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def ln_fold_case(M, K, N, mean_sigmas, seed=0, needles=0):
    """P.ln_case rows with their fp32 statistics, a sparse bf16 weight (its first `needles` rows
    one-hot: output column n is a[:, 7 n] alone), the host's fp32 colsum, bias, residual."""
    x = P.ln_case(M, K, mean_sigmas, seed)[0]
    w = P.sparse_weight(N, K, 8, seed + N + K)
    for n in range(needles):
        w[n] = 0.0
        w[n, 7 * n] = 1.0
    w = P.bf16_round(w)
    return dict(x=x, st=P.host_row_stats(x), w=w, colsum=w.sum(1), b=rnd(N, seed=seed + 3, scale=0.1),
                res=P.bf16_round(rnd(M, N, seed=seed + 4)))


def emulate_ln_fold(c, form, order="torch", st=None, drop_colsum=None, truncate_a=False, out=torch.bfloat16):
    """Both forms of the fold in fp32.  rows: a = x rstd + (-mean rstd) rounded to bf16 (or
    truncated), then the GEMM; epilogue: rstd (acc - mean colsum) on the raw accumulators
    (drop_colsum: that column's colsum term left out).  st: the statistics rows the kernel uses."""
    st = c["st"] if st is None else st
    m, r = st[:, :1], st[:, 1:]
    if form == "rows":
        a = torch.addcmul(-(m * r), c["x"], r)
        acc = mm(trunc_bf16(a) if truncate_a else bfr(a), c["w"], order)
    else:
        cs = c["colsum"].clone()
        if drop_colsum is not None:
            cs[drop_colsum] = 0.0
        acc = r * (mm(c["x"], c["w"], order) - m * cs)
    y = acc + c["b"] + c["res"]
    return y if out is None else y.to(out).float()


def ln_fold_ref(c, form, out=torch.bfloat16):
    return P.ln_fold_bound(c["x"], c["st"], c["w"], c["colsum"], c["b"], res=c["res"], out_dtype=out, form=form)


@pytest.mark.parametrize("form", ["rows", "epilogue"])
@pytest.mark.parametrize("mean_sigmas", [0, 30])
@pytest.mark.parametrize("M,K,N", [(300, 320, 72), (257, 640, 64)])
def test_ln_fold_emulation_passes(M, K, N, mean_sigmas, form):
    c = ln_fold_case(M, K, N, mean_sigmas)
    for out in (torch.bfloat16, torch.float32, None):
        ref, bound = ln_fold_ref(c, form, out)
        for order in ("torch", "ksteps"):
            got = emulate_ln_fold(c, form, order, out=None if out is None else out)
            worst = P.assert_elementwise(got, ref, bound)
        if out is not None:
            P.assert_elementwise(ref.to(out), ref, bound)  # the rounded reference alone
        print(f"ln fold emulation {form} {M}x{K}x{N} mean {mean_sigmas} out {out}: err/bound {worst:.3f}")
    # rowvec and out_scale enter like the residual
    rv = rnd(M, N, seed=9)
    ref, bound = P.ln_fold_bound(c["x"], c["st"], c["w"], c["colsum"], c["b"], rowvec=rv, res=c["res"], out_scale=0.5, form=form)
    got = bfr((emulate_ln_fold(c, form, out=None) + rv) * 0.5)
    P.assert_elementwise(got, ref, bound)


def test_ln_fold_forms_share_a_reference_and_the_host_colsum_is_charged():
    """Both forms have one fp64 reference.  The epilogue form subtracts mean * colsum with the
    colsum it is handed: a colsum off by 2^-12 of itself (a host that summed in bf16 steps) passes
    the bound made with that colsum -- the host term is computed, not tolerated -- and fails the
    bound made with the exact one."""
    c = ln_fold_case(300, 320, 72, 30)
    (ref_r, _), (ref_e, b_e) = ln_fold_ref(c, "rows", torch.float32), ln_fold_ref(c, "epilogue", torch.float32)
    assert float((ref_r - ref_e).abs().max()) < 1e-9
    worst = P.assert_elementwise(emulate_ln_fold(c, "epilogue", "ksteps", out=torch.float32), ref_e, b_e)
    c2 = dict(c, colsum=c["colsum"] * (1 + 2.0 ** -12))
    got = emulate_ln_fold(c2, "epilogue", out=torch.float32)
    ref2, b2 = ln_fold_ref(c2, "epilogue", torch.float32)
    assert torch.equal(ref2, ref_e)
    w2 = P.assert_elementwise(got, ref2, b2)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got, ref_e, b_e)
    print(f"epilogue fold at 30 sigma, fp32 out: err/bound {worst:.3f}; with the host's own colsum error {w2:.3f}")


@pytest.mark.parametrize("form", ["rows", "epilogue"])
def test_ln_fold_neighbour_statistics_rejected(form):
    c = ln_fold_case(257, 320, 72, 0)
    c["x"] = P.bf16_round(rnd(257, 320, seed=3))  # rows of one distribution: the neighbour's statistics are close
    c["st"] = P.host_row_stats(c["x"])
    ref, bound = ln_fold_ref(c, form)
    P.assert_elementwise(emulate_ln_fold(c, form), ref, bound)
    r = 130
    st = c["st"].clone()
    st[r] = c["st"][r + 1]
    got = emulate_ln_fold(c, form, st=st)
    with pytest.raises(AssertionError, match=rf"\(rows \[{r}\]\)"):
        P.assert_elementwise(got, ref, bound)
    _rejected(got, ref, bound, f"ln fold {form}: row {r} with its neighbour's statistics")  # Frobenius lets it through


@pytest.mark.parametrize("mean_sigmas,frobenius_passes", [(0, True), (30, False)])
def test_ln_fold_missing_colsum_term_rejected(mean_sigmas, frobenius_passes):
    """One column without mean * colsum[c].  At a mean near 0 the term is small and the Frobenius
    ratio lets it through; at 30 sigma it is large enough for any check."""
    c = ln_fold_case(300, 320, 72, mean_sigmas)
    ref, bound = ln_fold_ref(c, "epilogue")
    col = int((c["colsum"].abs() - 0.5).abs().argmin())  # an ordinary column (|colsum| about 0.5)
    got = emulate_ln_fold(c, "epilogue", drop_colsum=col)
    with pytest.raises(AssertionError, match=rf"col {col};"):
        P.assert_elementwise(got, ref, bound)
    ratio = (P.f64(got) - ref).abs() / bound
    assert sorted(set(torch.nonzero(ratio > 1.0)[:, 1].tolist())) == [col]
    fro = rel_err(got, ref)
    print(f"missing colsum term, mean {mean_sigmas}: err/bound {float(ratio.max()):.1f}, Frobenius {fro:.2e}")
    assert (fro < 1e-2) == frobenius_passes


def test_ln_fold_truncated_operand_rejected():
    """The normalised A truncated to bf16 instead of rounded: up to a whole bf16 step of a_k
    where the bound has half of one.  The pre-activation value (out_dtype None, what geglu_bound
    composes) rejects it on the one-hot weight rows, where the error of a_k arrives alone.  After
    the output's own rounding to bf16 the bound has a second half step, of the OUTPUT: the defect
    is still outside wherever bias and residual leave an output smaller than a_k.  The Frobenius
    ratio passes either way (on record)."""
    c = ln_fold_case(300, 320, 72, 0, needles=8)
    ref, bound = ln_fold_ref(c, "rows", None)
    P.assert_elementwise(emulate_ln_fold(c, "rows", out=None), ref, bound)
    got = emulate_ln_fold(c, "rows", truncate_a=True, out=None)
    ratio = (P.f64(got) - ref).abs() / bound
    bad = ratio[:, :8] > 1.0
    print(f"truncated A, pre-activation: err/bound {float(ratio.max()):.2f}, {int(bad.sum())} of {bad.numel()} needle elements outside")
    assert float(bad.float().mean()) > 0.2 and 1.2 < float(ratio[:, :8].max()) < 2.1
    _rejected(got, ref, bound, "ln fold rows: A truncated (pre-activation)")
    ref16, bound16 = ln_fold_ref(c, "rows")
    w16 = float(((P.f64(emulate_ln_fold(c, "rows", truncate_a=True)) - ref16).abs() / bound16).max())
    print(f"truncated A, bf16 out: err/bound {w16:.2f}")
    assert w16 > 1.2


def emulate_stored_row_stats(y, eps, chunk_order=False):
    """The row-block RB_STATS epilogue on the stored rows y: per 32-column chunk and lane group
    (columns 4 lg .. + 3 of both 16-column fragments) an fp32 chain of 8, double from there."""
    M, N = y.shape
    t = y.reshape(M, N // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(M, N // 32, 4, 8)
    s1, s2 = torch.zeros(M, N // 32, 4), torch.zeros(M, N // 32, 4)
    for j in range(8):
        s1 = s1 + t[..., j]
        s2 = (s2.double() + t[..., j].double() ** 2).float()  # fdot2 / fma: the square unrounded
    S1, S2 = s1.double().sum((1, 2)), s2.double().sum((1, 2))
    mean = S1 / N
    var = (S2 / N - mean * mean).clamp_min(0.0)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], 1).float()


@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("offset", [0.0, 3.0])
def test_stored_row_stats_emulation_passes(N, offset):
    y32 = rnd(300, N, seed=N) * (0.5 + rnd(300, 1, seed=1).abs()) + offset
    y = bfr(y32)
    ref, bound = P.stored_row_stats_bound(y, 1e-5, chain=8)
    worst = P.assert_elementwise(emulate_stored_row_stats(y, 1e-5), ref, bound)
    P.assert_elementwise(ref.float(), ref, bound)
    print(f"stored row statistics N {N} offset {offset}: err/bound {worst:.3f}")
    # the statistics of the unrounded fp32 values instead of the stored bf16 ones
    got = emulate_stored_row_stats(y32, 1e-5)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got, ref, bound)
    ratio = (P.f64(got) - ref).abs() / bound
    print(f"  from the unrounded values: err/bound {float(ratio.max()):.1f}, rows outside {int((ratio > 1).any(1).sum())} of 300, "
          f"Frobenius {rel_err(got, ref):.2e}")
    assert float((ratio > 1).any(1).float().mean()) > 0.9 and rel_err(got, ref) < 1e-2
    # one row's statistics written one row further down
    got = emulate_stored_row_stats(y, 1e-5)
    got[200] = got[199]
    with pytest.raises(AssertionError, match=r"row 200,"):
        P.assert_elementwise(got, ref, bound)


def emulate_slot_sums_csg2(t, rpi):
    """store_tile_plain_pre's CSG = 2 form on the rows of the slots t (slots, 128, N): a thread sums
    its rows (r0, r0 + rpi, ...) of the slot in fp32, then the rpi partials of a column in turn."""
    S, R, N = t.shape
    q1, q2 = torch.zeros(S, rpi, N), torch.zeros(S, rpi, N)
    for it in range(R // rpi):
        v = t[:, it * rpi:(it + 1) * rpi]
        q1, q2 = q1 + v, (q2.double() + v.double() ** 2).float()
    a1, a2 = torch.zeros(S, N), torch.zeros(S, N)
    for r in range(rpi):
        a1, a2 = a1 + q1[:, r], a2 + q2[:, r]
    return torch.stack([a1, a2], 1)


@pytest.mark.parametrize("family,th,H,W", [(3, 16, 32, 32), (3, 8, 32, 16), (4, 16, 64, 32), (4, 8, 32, 32), (0, -1, 16, 16)])
def test_halo_slot_sums_emulation_passes(family, th, H, W):
    """P.halo_slot_rows: every output pixel in exactly one slot, a slot = 8 rows x 16 pixels of one
    patch (of one parity in the phase form); the CSG = 2 sums of those rows pass colsum_bound, and
    a slot that misses one row, or sums the unrounded values, does not."""
    n, N = 2, 40
    plan = dict(family=family, halo_th=th)
    rows = P.halo_slot_rows(plan, n, H, W)
    assert rows.shape == (n * H * W // 128, 128)
    img, yy, xx = rows // (H * W), rows % (H * W) // W, rows % W
    step = 2 if family == 4 else 1
    if family in (3, 4):
        assert bool((img == img[:, :1]).all())
        assert bool(((yy.amax(1) - yy.amin(1)) == 7 * step).all()) and bool(((xx.amax(1) - xx.amin(1)) == 15 * step).all())
        assert bool((yy % step == yy[:, :1] % step).all()) and bool((xx % step == xx[:, :1] % step).all())  # one parity
        # the first slot of the second image starts that image's numbering (ls_conv_halo.hip "img * HW")
        assert int(rows[H * W // 128].min()) >= H * W
    if family == 3 and th == 16:  # 16 x 16 patches: slot 1 is the lower half of patch 0, slot 2 starts patch 1 (x0 = 16)
        assert rows[1, 0] == 8 * W and rows[2, 0] == 16
    if family == 3 and th == 8:   # 8 x 16 patches on a 16-wide image: slot 1 is the patch below
        assert rows[1, 0] == 8 * W
    if family == 4:               # parity 1 (py 0, px 1) follows all patches of parity 0
        assert rows[(H // 2) * (W // 2) // 128, 0] == 1
    y32 = rnd(n * H * W, N, seed=H + W) + 1.0
    y = bfr(y32)
    ref, bound = P.colsum_bound(y[rows.reshape(-1)])
    for rpi in (32, 25, 64):  # 128-column tiles (NT / 16), 160 columns (512 / 20: 25 rows per iteration of 64), narrow
        t = y[rows.reshape(-1)].reshape(-1, 128, N)
        if 128 % rpi:  # 64-row passes of ceil(64 / 25) iterations: pad the pass with zeros
            t = torch.cat([t.reshape(-1, 2, 64, N), torch.zeros(t.shape[0], 2, 75 - 64, N)], 2).reshape(-1, 150, N)
        worst = P.assert_elementwise(emulate_slot_sums_csg2(t, rpi), ref, bound)
    print(f"slot sums family {family} th {th}: err/bound {worst:.3f}")
    good = emulate_slot_sums_csg2(y[rows.reshape(-1)].reshape(-1, 128, N), 32)
    bad = good.clone()
    bad[3, 0] -= y[rows[3, 77]]
    bad[3, 1] -= y[rows[3, 77]] ** 2
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(bad, ref, bound, name="slot 3 misses a row")
    unrounded = emulate_slot_sums_csg2(y32[rows.reshape(-1)].reshape(-1, 128, N), 32)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(unrounded, ref, bound, name="sums of the unrounded values")
    # per-sample totals (what the suite compared before) cannot see a row that moved to the next slot
    moved = good.clone()
    moved[0, 0] -= y[rows[0, 77]]
    moved[1, 0] += y[rows[0, 77]]  # (slots 0 and 1 lie in one image)
    assert torch.allclose(moved.reshape(n, -1, 2, N).double().sum(1), good.reshape(n, -1, 2, N).double().sum(1), rtol=2e-3, atol=1e-2 * H * W)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(moved, ref, bound, name="a row summed into the next slot")


def test_rowblock_previous_sample_affine_rejected():
    """The row-block kernel's affine prologue (a = bf16(x scale[s] + shift[s])) with block 1 (rows
    256 .. 511 = sample 1) reading sample 0's affine; nearly equal affines, as in the model."""
    K, N, S, pps = 320, 64, 24, 256
    x, scale, shift = apply_case(K, 0, S, pps, mean_sigmas=0)
    w = P.bf16_round(P.sparse_weight(N, K, 8, 5))
    b = rnd(N, seed=6, scale=0.1)
    sc, sh = P.f64(scale)[:, None], P.f64(shift)[:, None]
    a64 = P.f64(x) * sc + sh
    a_abs = a64.abs() + 1.1 * 2.0 ** -12 * ((P.f64(x) * sc).abs() + sh.abs())  # E.conv_reference's |a'|
    ref = (a64 @ P.f64(w).T + P.f64(b)).reshape(S * pps, N)
    prod = (a_abs @ P.f64(w).abs().T).reshape(S * pps, N)
    bound = P.gemm_bound(ref, prod + P.f64(b).abs(), K, torch.bfloat16, prologue=True, prod_mag=prod)

    def run(sample_of):
        a = bfr(torch.addcmul(shift[sample_of][:, None], x, scale[sample_of][:, None]))
        return bfr(a.reshape(S * pps, K) @ w.T + b)

    own = torch.arange(S)
    worst = P.assert_elementwise(run(own), ref, bound)
    prev = own.clone()
    prev[1] = 0
    got = run(prev)
    with pytest.raises(AssertionError, match="err/bound"):
        P.assert_elementwise(got, ref, bound)
    ratio = ((P.f64(got) - ref).abs() / bound).amax(1)
    bad = torch.nonzero(ratio > 1.0).reshape(-1)
    assert int(bad.min()) >= pps and int(bad.max()) < 2 * pps
    fro = rel_err(got, ref)
    print(f"row-block affine: err/bound {worst:.3f}; previous sample's: {float(ratio.max()):.1f}, {bad.numel()} rows outside, Frobenius {fro:.2e}")
    assert bad.numel() > pps // 2 and fro < 1e-2


@pytest.mark.parametrize("M,N,K,fm,chunks", [(21760, 192, 320, 2, {1, 2}), (32768, 192, 320, 2, {3}), (4096, 2560, 320, 2, {5}),
                                             (65536, 192, 320, 2, {6}), (32768, 64, 640, 1, {2}), (32768, 192, 640, 2, {3}),
                                             (512, 192, 320, 2, {1}), (384, 192, 640, 1, {1})])
def test_rb_chunk_counts(M, N, K, fm, chunks):
    """The steady-state shapes of the GPU file against plan_rowblock's formula, and against the
    grid the library itself plans (host only)."""
    nch, ntm = N // 32, M // (128 * fm)
    ntn = max(1, min(nch, -(-256 // ntm)))
    assert P.rb_chunk_counts(dict(family=1, rb_fm=fm, grid=ntm * ntn), N, M) == chunks
    with pytest.raises(AssertionError):
        P.rb_chunk_counts(dict(family=1, rb_fm=fm, grid=ntm * ntn + 1), N, M)
    from latentsync_amd import _lib, ops
    lib = _lib.load()
    x = torch.empty(1, 1, M, K, dtype=torch.bfloat16)
    pw = ops.Packed(torch.empty(N, K, dtype=torch.bfloat16), None, K, 1, N)
    lib.ls_set_tuning(15, int(fm == 2))
    try:
        plan = ops.conv_plan(x, pw, out=torch.empty(1, 1, M, N, dtype=torch.bfloat16), workspace_bytes=0)
    finally:
        lib.ls_set_tuning(15, 1)
    assert plan["family"] == 1 and plan["rb_fm"] == fm and plan["rb_flags"] == 0, plan
    assert P.rb_chunk_counts(plan, N, M) == chunks


# ---------------------------------------------------------------- fp8 attention (ls_attention_fp8)
def emulate_attn_fp8_tiled(q, k, v, scale, **defect):
    """attn8_kernel's key walk for one (batch, head): q (nq, d), k / v (nk, d) bf16 values ->
    (o fp32 (nq, d), not yet rounded to bf16, trace).  oracle.fp8_cpu.attention_fp8 takes the row
    maximum in one pass; this restatement moves m as the kernel does:
      * 128-key tiles in two 64-key halves; the keys past nk of the partial tile are -inf (their K
        rows are the buffer load's zeros, their V codes zero, the sum row 1.0 all the same);
      * the first half sets m = ceil(half max) - 7; afterwards m moves by dlt = ceil(half max - m)
        - 7 whenever a half's maximum exceeds m + 8 ("need = first || mt[g] > TAU");
      * a move multiplies the accumulators, the sum column included, by 2^-dlt; when any row of a
        wave (32 rows: QG 2 x 16) moves in a tile's second half, the wave's first-half P, packed
        against the old m, is accumulated on its own first ("pv(pk)" with the second half zeroed);
      * p = e4m3(2^(s - m)), accumulated against the dequantised V^T and its constant row D.
    trace: moved (nq, tiles, 2) bool and dlt (nq, tiles, 2), per (tile, half).

    Planted defects (keywords): drop_key=j (its score -inf), sum_without=j (row D of V^T zero at
    key j), unmask=j (a key past nk not masked), skip_rescale (alpha = 1 on a move in a later
    tile), skip_flush (no separate accumulation of the first half), scale_off=(tile, lg) (that lane
    group's 32 keys dequantised with a scale byte one too high), swap_keys=(j1, j2) (their V^T
    columns exchanged)."""
    nq, D = q.shape
    nk = k.shape[0]
    nt = -(-nk // Q8.KT)
    qs = P.bf16_round(q.float() * (scale * LOG2E))
    kp = torch.zeros(nt * Q8.KT, D)
    kp[:nk] = k.float()
    codes, e8 = Q8.quant_vt(v)
    vq = Q8.dequant_vt(codes, e8, nt * Q8.KT)
    if "scale_off" in defect:
        t, lg = defect["scale_off"]
        vq[t * Q8.KT + Q8.key_perm()[32 * lg:32 * lg + 32]] *= 2.0
    if "swap_keys" in defect:
        j1, j2 = defect["swap_keys"]
        vq[[j1, j2]] = vq[[j2, j1]]
    va = torch.cat([vq, torch.ones(nt * Q8.KT, 1)], 1)
    if "sum_without" in defect:
        va[defect["sum_without"], D] = 0.0
    s_all = qs @ kp.t()
    if "drop_key" in defect:
        s_all[:, defect["drop_key"]] = -float("inf")
    valid = torch.arange(nt * Q8.KT) < nk
    if "unmask" in defect:
        valid[defect["unmask"]] = True
    wave = torch.arange(nq) // 32
    m = torch.zeros(nq)
    acc = torch.zeros(nq, D + 1)
    moved = torch.zeros(nq, nt, 2, dtype=torch.bool)
    dlts = torch.zeros(nq, nt, 2)
    for t in range(nt):
        pend = torch.zeros(nq, 64)
        for hf in range(2):
            k0 = t * Q8.KT + 64 * hf
            s = s_all[:, k0:k0 + 64] - m[:, None]
            s = torch.where(valid[k0:k0 + 64], s, torch.full_like(s, -float("inf")))
            mt = s.amax(-1)
            first = t == 0 and hf == 0
            need = torch.ones(nq, dtype=torch.bool) if first else mt > 8.0
            again = (torch.zeros(int(wave[-1]) + 1).index_add_(0, wave, need.float()) > 0)[wave]
            if hf == 1 and not defect.get("skip_flush"):
                acc[again] += pend[again] @ va[k0 - 64:k0]
                pend[again] = 0.0
            dlt = torch.where(need, torch.ceil(mt) - 7.0, torch.zeros(nq))
            alpha = torch.zeros(nq) if first else torch.exp2(-dlt)
            if defect.get("skip_rescale") and t > 0:
                alpha = torch.ones(nq)
            m = m + dlt
            s = s - dlt[:, None]
            acc = acc * alpha[:, None]
            moved[:, t, hf], dlts[:, t, hf] = need, dlt
            p = torch.exp2(s).to(torch.float8_e4m3fn).float()
            if hf == 0:
                pend = p
            else:
                acc += torch.cat([pend, p], 1) @ va[k0 - 64:k0 + 64]
    return acc[:, :D] / acc[:, D:], dict(moved=moved, dlt=dlts)


_FP8 = {c[0]: c for c in P.FP8_CASES}
_FP8_CACHE = {}


def fp8_case(name):
    """Inputs, fp64 reference, bound and the clean tile-order emulation (per pair, with its trace)
    of one case of P.FP8_CASES, computed once."""
    if name not in _FP8_CACHE:
        _, d, batch, heads, nq, nk, kind = _FP8[name]
        q, k, v = P.fp8_qkv(d, batch, heads, nq, nk, kind)
        scale = 1 / math.sqrt(d)
        ref, bound, parts = P.attn_fp8_bound(q, k, v, scale, parts=True)
        emu = [[emulate_attn_fp8_tiled(q[b, h], k[b, h], v[b, h], scale) for h in range(heads)] for b in range(batch)]
        o = torch.stack([torch.stack([e[0] for e in row]) for row in emu])
        w = torch.softmax(scale * (P.f64(q) @ P.f64(k).transpose(-1, -2)), -1)
        _FP8_CACHE[name] = dict(q=q, k=k, v=v, scale=scale, ref=ref, bound=bound, parts=parts, o=o, w=w,
                                trace=[[e[1] for e in row] for row in emu])
    return _FP8_CACHE[name]


@pytest.mark.parametrize("name", list(_FP8))
def test_fp8_tiled_emulation_passes(name):
    """The tile-order walk passes attn_fp8_bound, and agrees with the one-pass emulation
    (oracle.fp8_cpu.attention_fp8, the same fp32 scores) within the bound's terms that are not a
    normal-range quantisation: the fp32 / score term and twice the subnormal-p term (the two m
    differ by 2^k, k in {0, 1}, so a p of the key set the term counts sits on a 2^-9 grid in one
    walk and on a finer one in the other: each is within 2^-10 of the unrounded p)."""
    c = fp8_case(name)
    worst = P.assert_elementwise(bfr(c["o"]), c["ref"], c["bound"], where=dict(rows=16, cols=16), name=name)
    q, k, v = c["q"], c["k"], c["v"]
    one = torch.stack([torch.stack([Q8.attention_fp8(q[b, h], k[b, h], v[b, h], c["scale"]) for h in range(q.shape[1])])
                       for b in range(q.shape[0])])
    tol = c["parts"]["score"] + 2 * c["parts"]["sub"] + P.TINY
    agree = P.assert_elementwise(c["o"], P.f64(one), tol, name=f"{name} tile-order vs one-pass")
    print(f"fp8 emulation {name}: err/bound {worst:.3f}, tile-order vs one-pass {agree:.3f} of its tolerance")


def test_fp8_cases_cover_the_running_max():
    """Read from the emulation's trace and the fp64 weights alone: the case list holds rows whose m
    moves in a second half, rows whose m moves in a later tile by at most 3 while the keys before
    that half keep more than 1 % of the row's weight (so a missed rescale shows), rows whose m
    never moves after the first half although there are more keys, and rows whose first m is negative."""
    second = later = never = negative = 0
    for name, d, batch, heads, nq, nk, kind in P.FP8_CASES:
        c = fp8_case(name)
        for b in range(batch):
            for h in range(heads):
                mv, dl = c["trace"][b][h]["moved"], c["trace"][b][h]["dlt"]
                after = mv.clone()
                after[:, 0, 0] = False
                assert bool(mv[:, 0, 0].all()) and bool((dl[after] >= 2).all())  # a later move is by 2 at least
                second += int(mv[:, :, 1].any(1).sum())
                negative += int((dl[:, 0, 0] < 0).sum())
                if nk > 64:
                    never += int((~mv.reshape(nq, -1)[:, 1:].any(1)).sum())
                before = torch.cumsum(c["w"][b, h], -1)
                for t in range(1, mv.shape[1]):
                    for hf in range(2):
                        k0 = min(t * 128 + 64 * hf, nk)
                        later += int((mv[:, t, hf] & (dl[:, t, hf] <= 3) & (before[:, k0 - 1] > 0.01)).sum())
    print(f"fp8 coverage: {second} rows move in a second half, {later} small moves in a later tile, "
          f"{never} rows never move again, {negative} rows start at a negative m")
    assert second > 0 and later > 0 and never > 0 and negative > 0


OLD_ROWS = 32768  # rows of the largest output tests/test_gpu_fp8.py takes its ratios over: (1, 4096, 4096, 8, 40)


def fp8_defect_rows(name, candidates, what):
    """Plant each (row, defect) of `candidates` into that one row of pair (0, 0) of the clean
    emulation; returns [(row, err/bound of the row, rejected, rel vs emulation, rel vs fp64)].
    The Frobenius ratios are taken over the case's whole output, as tests/test_gpu_fp8.py does."""
    c = fp8_case(name)
    clean = bfr(c["o"])
    out = []
    for row, defect in candidates:
        bad, _ = emulate_attn_fp8_tiled(c["q"][0, 0], c["k"][0, 0], c["v"][0, 0], c["scale"], **defect)
        got = clean.clone()
        got[0, 0, row] = bfr(bad[row])
        ratio = float(((P.f64(got) - c["ref"]).abs() / c["bound"])[0, 0, row].max())
        try:
            P.assert_elementwise(got, c["ref"], c["bound"], name=what)
            rejected = False
        except AssertionError as e:
            assert f"(rows [{row}])" in str(e), str(e)  # pair (0, 0)'s row: the only one outside
            rejected = True
        assert rejected == (ratio > 1.0)
        out.append((row, ratio, rejected, rel_err(got, clean), rel_err(got, c["ref"])))
        print(f"{name} {what} {defect} in row {row}: err/bound {ratio:.2f}, Frobenius vs emulation {out[-1][3]:.2e}, "
              f"vs fp64 {out[-1][4]:.2e}")
    return out


def fp8_old_check_blind(name, res):
    """What tests/test_gpu_fp8.py asserts of an output -- rel_err < 6e-2 against the fp64 softmax
    and < 4e-3 against the emulation -- for the rejected one-row defects of `res`: at least one of
    them stays under both.  The ratio against fp64 is taken over the case's output as it is.  The
    one against the emulation cannot be: a case here has 4 to 520 rows, and a row that leaves a
    bound about 13 % of itself wide weighs at least 0.13 / sqrt(520) = 5.7e-3 in such an output.
    The outputs of that file have 3200 to 32768 rows, and one wrong row among R error-free ones of
    like size weighs 1 / sqrt(R): the measured ratio is taken times sqrt(rows / OLD_ROWS), what the
    same row weighs in the largest output that file checks."""
    _, d, batch, heads, nq, nk, kind = _FP8[name]
    shrink = math.sqrt(batch * heads * nq / OLD_ROWS)
    hidden = [(r, e * shrink, f) for r, _, rej, e, f in res if rej and e * shrink < 4e-3 and f < 6e-2]
    print(f"{name}: the Frobenius check lets through the defect in rows {[r for r, _, _ in hidden]}")
    assert hidden, res


def _needle_rows(name):
    """(row, key, strong) of pair (0, 0)'s needle rows whose key carries most of the row's weight.
    strong: w_j |v_j| is, in some column, above 4 times what all the other keys together bring
    (sum_i w_i |v_i|).  V spans 2^-6 .. 2^6 per key, so under a small needle the other keys' few
    per cent of the weight make most of the row and of its bound: a defect in the needle's VALUE
    must show on the strong rows, and may hide on the others."""
    c = fp8_case(name)
    _, d, batch, heads, nq, nk, kind = _FP8[name]
    w, v = c["w"][0, 0], P.f64(c["v"][0, 0])
    rows = []
    for i, j in enumerate(P.fp8_needle_keys(nk)[:nq]):
        own = w[i, j] * v[j].abs()
        rest = w[i] @ v.abs() - own
        if float(w[i, j]) > 0.5:
            rows.append((i, j, float(own.max()) > 4 * float(rest.max())))
    assert rows
    return rows


FP8_NEEDLE_MUT = [n for n in _FP8 if n.endswith("needle") and _FP8[n][5] > 1]


@pytest.mark.parametrize("name", FP8_NEEDLE_MUT)
def test_fp8_dropped_needle_key_rejected(name):
    res = fp8_defect_rows(name, [(i, dict(drop_key=j)) for i, j, _ in _needle_rows(name)], "dropped key")
    assert all(rej and ratio > 3 for _, ratio, rej, _, _ in res), res
    fp8_old_check_blind(name, res)


@pytest.mark.parametrize("name", FP8_NEEDLE_MUT)
def test_fp8_row_sum_missing_key_rejected(name):
    res = fp8_defect_rows(name, [(i, dict(sum_without=j)) for i, j, _ in _needle_rows(name)], "row sum without key")
    assert all(rej and ratio > 3 for _, ratio, rej, _, _ in res), res
    fp8_old_check_blind(name, res)


def _strong_rejected(name, cand, res):
    strong = {i for i, _, st in _needle_rows(name) if st}
    hit = [rej for (row, _), (_, _, rej, _, _) in zip(cand, res) if row in strong]
    assert hit and all(hit), res
    return len(hit)


@pytest.mark.parametrize("name", FP8_NEEDLE_MUT)
def test_fp8_scale_byte_off_by_one_rejected(name):
    """The scale byte of the needle key's lane group (32 keys of its tile) one too high: rejected
    on every strong needle row."""
    perm = Q8.key_perm()
    cand = [(i, dict(scale_off=(j // 128, int((perm == j % 128).nonzero()) // 32))) for i, j, _ in _needle_rows(name)]
    res = fp8_defect_rows(name, cand, "scale byte + 1")
    _strong_rejected(name, cand, res)
    fp8_old_check_blind(name, res)


@pytest.mark.parametrize("name", FP8_NEEDLE_MUT)
def test_fp8_exchanged_keys_rejected(name):
    """The needle key's V^T column exchanged with that of the key 4 further on (the next lane
    group's, same j) or, at the tile's or the key set's end, 4 back: rejected on every strong
    needle row."""
    nk = _FP8[name][5]
    cand = []
    for i, j, _ in _needle_rows(name):
        j2 = j + 4 if (j + 4) // 128 == j // 128 and j + 4 < nk else j - 4
        if j2 >= 0:
            cand.append((i, dict(swap_keys=(j, j2))))
    res = fp8_defect_rows(name, cand, "exchanged keys")
    _strong_rejected(name, cand, res)
    fp8_old_check_blind(name, res)


@pytest.mark.parametrize("d", [40, 80])
def test_fp8_unmasked_key_rejected(d):
    """Key nk = 1 of the one-key case left unmasked: its K row is the buffer load's zeros (score
    0), its V codes are zero, the sum row is 1.0 there too.  The rows whose only score is below
    -4 (in log2 units) lose most of their value to it."""
    name = f"d{d}_1x1_random6"
    c = fp8_case(name)
    ok = False
    for b in range(2):
        for h in range(2):
            s = float(P.bf16_round(c["q"][b, h] * (c["scale"] * LOG2E)) @ c["k"][b, h].t())
            bad, _ = emulate_attn_fp8_tiled(c["q"][b, h], c["k"][b, h], c["v"][b, h], c["scale"], unmask=1)
            ratio = float(((P.f64(bfr(bad)) - c["ref"][b, h]).abs() / c["bound"][b, h]).max())
            print(f"{name} pair ({b}, {h}) score {s:.1f}: unmasked key 1, err/bound {ratio:.2f}")
            if s < -4:
                ok = True
                with pytest.raises(AssertionError, match="err/bound"):
                    P.assert_elementwise(bfr(bad), c["ref"][b, h], c["bound"][b, h])
    assert ok


def _moving_rows(name, second_half):
    """Rows of pair (0, 0) whose m moves in a later tile (second_half False) or in a second half
    (True) while the keys before that half keep more than 5 % of the row's weight."""
    c = fp8_case(name)
    nk = _FP8[name][5]
    mv = c["trace"][0][0]["moved"]
    before = torch.cumsum(c["w"][0, 0], -1)
    rows = set()
    for t in range(0 if second_half else 1, mv.shape[1]):
        for hf in ((1,) if second_half else (0, 1)):
            k0 = min(t * 128 + 64 * hf, nk)
            rows |= set(torch.nonzero(mv[:, t, hf] & (before[:, k0 - 1] > 0.05)).reshape(-1).tolist())
    return sorted(rows)


@pytest.mark.parametrize("name", ["d40_70x257_random6", "d80_70x257_random6", "d40_129x385_random6", "d80_129x385_random6"])
def test_fp8_skipped_rescale_rejected(name):
    """alpha = 1 where m moves in a later tile: the earlier keys keep 2^dlt times their weight."""
    rows = _moving_rows(name, False)
    res = fp8_defect_rows(name, [(r, dict(skip_rescale=True)) for r in rows], "skipped rescale")
    assert sum(rej for _, _, rej, _, _ in res) >= len(res) // 2 > 0, res
    fp8_old_check_blind(name, res)


@pytest.mark.parametrize("name", ["d40_130x128_random6", "d80_130x129_random6", "d40_129x385_random6", "d80_129x385_random6"])
def test_fp8_skipped_first_half_flush_rejected(name):
    """m moves in a tile's second half and the first half's P, packed against the old m, is
    accumulated after the rescale instead of before it."""
    rows = _moving_rows(name, True)
    res = fp8_defect_rows(name, [(r, dict(skip_flush=True)) for r in rows], "skipped first-half flush")
    assert sum(rej for _, _, rej, _, _ in res) >= len(res) // 2 > 0, res
    fp8_old_check_blind(name, res)


# ---------------------------------------------------------------- Whisper log-mel (ls_log_mel)
@functools.lru_cache(maxsize=None)
def mel_fb(n_mels=80):
    from latentsync_amd.audio import mel_filters
    return torch.from_numpy(mel_filters(n_mels=n_mels))


@functools.lru_cache(maxsize=None)
def mel_oracle(n, kind, t_pad=None, n_mels=80):
    return P.log_mel_bound(P.mel_signal(n, kind), mel_fb(n_mels), t_pad or n // P.MEL_HOP)


def emulate_log_mel(wave, filters, t_pad, hann="periodic", pad="reflect", block_floor=False, frame_offset=0,
                    truncate=False):
    """log_mel_kernel + mel_norm_kernel restated in fp32 torch: the window and the twiddles as fp32
    tables, fp32 products and sums (torch's fp32 matmul: another order than the kernel's chain,
    which the bound allows), log10, the clip-wide floor, (x + 4) / 4, bf16 round-to-nearest.
    Returns (l fp32 (T, n_mels), v (t_pad, n_mels) as fp32).  The switches plant one defect each."""
    x = wave.float()
    n = x.numel()
    T = n // P.MEL_HOP
    m = torch.arange(P.MEL_NFFT)
    win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * m.double() / (P.MEL_NFFT if hann == "periodic" else P.MEL_NFFT - 1)).float()
    j = (torch.arange(T)[:, None] + frame_offset) * P.MEL_HOP + m[None, :] - P.MEL_NFFT // 2
    if pad == "reflect":
        j = j.abs()
        j = torch.where(j >= n, 2 * (n - 1) - j, j).clamp(0, n - 1)
        xw = x[j] * win
    else:
        inside = (j >= 0) & (j < n)
        xw = torch.where(inside, x[j.clamp(0, n - 1)], torch.zeros(())) * win
    ph = 2.0 * math.pi * ((torch.arange(P.MEL_NFREQ)[:, None] * m[None, :]) % P.MEL_NFFT).double() / P.MEL_NFFT
    re, im = xw @ torch.cos(ph).float().T, -(xw @ torch.sin(ph).float().T)
    s = (re * re + im * im) @ filters.float().T
    l = torch.log10(s.clamp_min(1e-10))
    if block_floor:
        nb = -(-T // P.MEL_BLOCK)
        lp = torch.full((nb * P.MEL_BLOCK, l.shape[1]), -float("inf"))
        lp[:T] = l
        fl = (lp.reshape(nb, -1).amax(1) - 8.0).repeat_interleave(P.MEL_BLOCK)[:T, None]
    else:
        fl = l.max() - 8.0
    v32 = (torch.maximum(l, fl) + 4.0) / 4.0
    vb = (v32.view(torch.int32) & -65536).view(torch.float32) if truncate else v32.to(torch.bfloat16).float()
    v = torch.zeros(t_pad, l.shape[1])
    v[:T] = vb
    return l, v


# every (n, signal, n_mels) of tests/test_gpu_edges_audio.py
MEL_SIGNALS = [(n, "mix", 80) for n in P.MEL_N] + [(P.MEL_FLOOR_N, k, 80) for k in P.MEL_FLOOR_KINDS] + [(4159, "mix", 128)]


@pytest.mark.parametrize("n,kind,n_mels", MEL_SIGNALS)
def test_log_mel_emulation_passes_and_bound_is_narrow(n, kind, n_mels):
    """The fp32 restatement passes both bounds on every signal the GPU file uses, and the bound
    cannot hide a failure behind its width: at most 1 % of the fp32 log-mel elements of a signal
    have a half-width above 2^-6 (those are still checked, against their own bound)."""
    T = n // P.MEL_HOP
    l_ref, l_b, v_ref, v_b = mel_oracle(n, kind, T + 3, n_mels)
    l, v = emulate_log_mel(P.mel_signal(n, kind), mel_fb(n_mels), T + 3)
    wl = P.assert_elementwise(l, l_ref, l_b, name="log-mel")
    wv = P.assert_elementwise(v, v_ref, v_b, name="normalised mel")
    assert float(v[T:].abs().max()) == 0.0
    wide = float((l_b > 2.0 ** -6).double().mean())
    print(f"log-mel emulation n {n} {kind} mels {n_mels}: err/bound l {wl:.3f} v {wv:.3f}; half-width median {float(l_b.median()):.2e} "
          f"max {float(l_b.max()):.2e}, {100 * wide:.2f} % above 2^-6")
    assert wide <= 0.01
    if kind == "zeros":
        assert bool((v[:T] == -1.5).all())
    if kind == "noise1e-3":
        assert float(l_ref.max()) < 0  # the negative branch of the ordered-uint maximum


def mel_mutant_ratios(n, kind, **defect):
    l_ref, l_b, v_ref, v_b = mel_oracle(n, kind)
    l, v = emulate_log_mel(P.mel_signal(n, kind), mel_fb(), n // P.MEL_HOP, **defect)
    return (P.f64(l) - l_ref).abs() / l_b, (P.f64(v) - v_ref).abs() / v_b


def test_log_mel_symmetric_hann_rejected():
    rl, rv = mel_mutant_ratios(4159, "mix", hann="symmetric")
    print(f"symmetric Hann: {100 * float((rl > 1).double().mean()):.1f} % of the fp32 log-mel values outside (worst "
          f"{float(rl.max()):.1f}), {100 * float((rv > 1).double().mean()):.1f} % of the bf16 outputs (worst {float(rv.max()):.1f})")
    assert float(rl.max()) > 4 and float((rl > 1).double().mean()) > 0.3
    assert float(rv.max()) > 1


def test_log_mel_zero_padding_rejected():
    """Zero instead of reflect padding: only the frames whose window leaves the clip differ."""
    rl, rv = mel_mutant_ratios(4159, "mix", pad="zero")
    bad = sorted(set(torch.nonzero(rl > 1)[:, 0].tolist()))
    print(f"zero padding: worst err/bound l {float(rl.max()):.0f} v {float(rv.max()):.0f}, frames {bad}")
    assert float(rl.max()) > 10 and float(rv.max()) > 1
    assert set(bad) <= {0, 1, 24} and 0 in bad


def test_log_mel_block_floor_rejected():
    """The floor from each block's own maximum: invisible in l, caught in v wherever a quiet
    block sits more than 8 below the clip's loudest frame."""
    rl, rv = mel_mutant_ratios(P.MEL_FLOOR_N, "zeros_after", block_floor=True)
    assert float(rl.max()) <= 1
    print(f"per-block floor: worst err/bound v {float(rv.max()):.0f}")
    assert float(rv.max()) > 50
    for kind in ("loud_first", "loud_last"):  # these two cases separate the floors as well
        assert float(mel_mutant_ratios(P.MEL_FLOOR_N, kind, block_floor=True)[1].max()) > 1, kind


def test_log_mel_frame_offset_rejected():
    rl, rv = mel_mutant_ratios(4159, "mix", frame_offset=1)
    print(f"one frame of offset: worst err/bound l {float(rl.max()):.0f} v {float(rv.max()):.0f}")
    assert float(rl.max()) > 10 and float(rv.max()) > 10


def test_log_mel_truncation_rejected():
    rl, rv = mel_mutant_ratios(4159, "mix", truncate=True)
    assert float(rl.max()) <= 1
    print(f"bf16 truncation: worst err/bound v {float(rv.max()):.2f}, {100 * float((rv > 1).double().mean()):.1f} % outside")
    assert 1.3 < float(rv.max()) < 2.1  # up to a full ulp instead of half of one


# ---------------------------------------------------------------- time embedding (ls_elem.hip)
def emulate_timestep(t, dim, shift, flip, swap=False, no_shift=False):
    """timestep_embed_kernel in fp32 torch, operation by operation."""
    half = dim // 2
    i = torch.arange(half, dtype=torch.float32)
    den = torch.tensor(float(half), dtype=torch.float32) - (0.0 if no_shift else torch.tensor(float(shift), dtype=torch.float32))
    e = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * i / den)
    arg = torch.as_tensor(t, dtype=torch.float32).reshape(-1, 1) * e[None, :]
    sn, cs = torch.sin(arg), torch.cos(arg)
    return torch.cat([cs, sn] if bool(flip) != swap else [sn, cs], 1)


TS_VALUES = [float(t) for t in P.TS_T] + [0.25, 500.5, 998.75]


@pytest.mark.parametrize("dim", P.TS_DIMS)
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("shift", [0, 1])
def test_timestep_emulation_passes_and_mutants_rejected(dim, flip, shift):
    ref, b = P.timestep_bound(torch.tensor(TS_VALUES), dim, shift, flip)
    worst = P.assert_elementwise(emulate_timestep(TS_VALUES, dim, shift, flip), ref, b, name="timestep")
    print(f"timestep emulation dim {dim} flip {flip} shift {shift}: err/bound {worst:.3f}, widest bound {float(b.max()):.2e}")
    assert float(b.max()) < 2e-3  # no wider than the absolute tolerance it replaces
    with pytest.raises(AssertionError, match="err/bound"):  # sin and cos swapped under flip
        P.assert_elementwise(emulate_timestep(TS_VALUES, dim, shift, flip, swap=True), ref, b)
    if shift:  # half where half - shift belongs
        with pytest.raises(AssertionError, match="err/bound"):
            P.assert_elementwise(emulate_timestep(TS_VALUES, dim, shift, flip, no_shift=True), ref, b)


def small_linear_case(M, K, N, seed=0):
    """fp32 x (M, K) of deviation 2 (SiLU is far from the identity), bf16-rounded W (N, K), fp32 bias."""
    x = 2.0 * rnd(M, K, seed=seed + M + K)
    w = P.bf16_round(rnd(N, K, seed=seed + N + K + 1, scale=1 / math.sqrt(K)))
    return x, w, rnd(N, seed=seed + N + 2, scale=0.1)


def emulate_small_linear(x, w, bias, silu_in):
    a = x * torch.sigmoid(x) if silu_in else x
    y = a @ w.T
    return y if bias is None else y + bias


@pytest.mark.parametrize("M,K,N", P.SMALL_LINEAR_CASES)
@pytest.mark.parametrize("silu_in", [False, True])
def test_small_linear_emulation_passes_and_mutants_rejected(M, K, N, silu_in):
    x, w, b = small_linear_case(M, K, N)
    for bias in (b, None):
        ref, bound = P.dot_bound(x, w, bias, silu_in)
        worst = P.assert_elementwise(emulate_small_linear(x, w, bias, silu_in), ref, bound, name="small_linear")
        with pytest.raises(AssertionError, match="err/bound"):  # SiLU skipped / applied unasked
            P.assert_elementwise(emulate_small_linear(x, w, bias, not silu_in), ref, bound)
    ref, bound = P.dot_bound(x, w, b, silu_in)
    col = int(b.abs().argmax())
    b2 = b.clone()
    b2[col] = 0.0
    with pytest.raises(AssertionError, match=rf"col {col};"):  # a dropped bias column
        P.assert_elementwise(emulate_small_linear(x, w, b2, silu_in), ref, bound)
    print(f"small_linear emulation {M}x{K}x{N} silu {silu_in}: err/bound {worst:.3f}")
