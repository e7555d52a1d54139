"""Per-element acceptance of a kernel's output against an fp64 reference, with a bound
derived from the kernel's arithmetic, and sentinel guard bands around every output.

A Frobenius ratio over a whole output (conftest.rel_err) cannot see one wrong row, one
column without its bias, truncation instead of round-to-nearest, or a write outside the
requested output.  The helpers here can (tests/test_parity_bounds.py shows it on the CPU).

Number formats: bf16 has an 8-bit significand, so round-to-nearest-even (what f2bf / pack2
of ls_common.h do, one v_cvt_pk_bf16_f32) has unit roundoff 2^-8; fp32 has 2^-24.  One fp32
operation in ANY rounding mode (truncation included) is within 2^-23 relative.
"""
import math

import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
E_F32 = 2.0 ** -23             # one fp32 operation, any rounding mode
SLACK = 1.0 + 2.0 ** -6        # second-order terms of the first-order bounds below
TINY = 2.0 ** -126             # results below the smallest normal may flush to zero

GELU_LIP, SILU_LIP = 1.13, 1.1  # max |f'| of the erf GELU (1.129 at x = sqrt(2)) and of SiLU (1.0998)
GELU_ERR = 2.6e-5              # |gelu_erf - exact| on all of R (ls_common.h; tests/test_gelu_form.py pins it)


def f64(t):
    return torch.as_tensor(t).detach().to("cpu").to(torch.float64)


def bf16_round(t):
    """Round to bf16 (nearest even) and return as float32: the inputs every kernel sees."""
    return torch.as_tensor(t).to(torch.bfloat16).to(torch.float32)


def _u_out(out_dtype):
    if out_dtype is None:
        return 0.0
    if out_dtype == torch.bfloat16:
        return U_BF16
    if out_dtype == torch.float32:
        return U_F32
    raise ValueError(f"no unit roundoff for {out_dtype}")


def _slack(b):
    return b * SLACK + TINY


def gemm_bound(ref, mag, k_terms, out_dtype, prologue=False, prod_mag=None):
    """Per-element bound B of a fused GEMM output.

    ref = out_scale (sum_k a_k w_k + bias + rowvec + res) in fp64 on the bf16-rounded inputs,
    mag = the same expression with every term replaced by its absolute value.

        B = u_out |ref| + (k_terms + 4) 2^-23 mag + [prologue] 2^-8 prod_mag

      * u_out |ref|: the one rounding of the result to the output format (2^-8 bf16, 2^-24
        fp32; out_dtype None = no output rounding: the pre-activation value of act_bound).
      * (k_terms + 4) 2^-23 mag: the products a_k w_k of two bf16 numbers are exact in fp32;
        every one of the k_terms accumulations and the <= 4 epilogue operations (bias,
        rowvec, residual, scale) rounds once, in any mode and any order -- the standard
        recursive-summation bound gamma_n |terms| with the any-rounding-mode unit 2^-23.  The
        order is free, so split-K slabs and the MFMA's internal tree are covered.
      * prologue: the kernel builds A itself (GroupNorm affine + SiLU) and rounds it to bf16
        for the MFMA, while ref uses the unrounded fp64 activation: each a_k is within 2^-8
        relative (+ the fp32 evaluation, covered by the SLACK factor), so the sum moves by at
        most 2^-8 prod_mag with prod_mag = out_scale sum_k |a_k w_k|.
    The whole bound is multiplied by (1 + 2^-6) and gets + 2^-126.
    """
    ref, mag = f64(ref), f64(mag)
    b = _u_out(out_dtype) * ref.abs() + (k_terms + 4) * E_F32 * mag
    if prologue:
        if prod_mag is None:
            raise ValueError("prologue=True needs prod_mag = out_scale * sum_k |a_k w_k|")
        b = b + U_BF16 * f64(prod_mag)
    return _slack(b)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _silu(x):
    return x * torch.sigmoid(x)


def act_bound(kind, ref_pre, b_pre, out_dtype):
    """(act(ref_pre), bound) for an activation epilogue: B_act = L B_pre + e_act + u_out |act(ref)|.

    b_pre = gemm_bound(..., out_dtype=None) of the pre-activation value (the kernel keeps it in
    fp32).  L = max |f'| (1.13 GELU, 1.1 SiLU) carries the input error through; e_act is the
    evaluation error at the exact input: 2.6e-5 for gelu_erf, 8 2^-23 |x| for silu (x, the
    log2(e) product, v_exp_f32 and v_rcp_f32 at 1 ulp each, the add and the final product:
    6 roundings of relative size 2^-23 on a result of magnitude <= |x|, rounded up to 8)."""
    x = f64(ref_pre)
    b_pre = f64(b_pre)
    if kind == "gelu":
        y, lip, e_act = _gelu(x), GELU_LIP, torch.full_like(x, GELU_ERR)
    elif kind == "silu":
        y, lip, e_act = _silu(x), SILU_LIP, 8 * E_F32 * x.abs()
    else:
        raise ValueError(kind)
    return y, _slack(lip * b_pre + e_act + _u_out(out_dtype) * y.abs())


def geglu_bound(ref_h, b_h, ref_g, b_g, out_dtype):
    """(h gelu(g), bound) by the product rule: with gelu(g) known to B_G = 1.13 b_g + 2.6e-5 and
    h to b_h, |h' G' - h G| <= |h| B_G + |G| b_h + b_h B_G, plus the fp32 product's own rounding
    (2^-23 |ref|) and the output rounding u_out |ref|."""
    h, g = f64(ref_h), f64(ref_g)
    b_h, b_g = f64(b_h), f64(b_g)
    G = _gelu(g)
    b_G = GELU_LIP * b_g + GELU_ERR
    ref = h * G
    b = h.abs() * b_G + G.abs() * b_h + b_h * b_G + (E_F32 + _u_out(out_dtype)) * ref.abs()
    return ref, _slack(b)


def attn_bound(q, k, v, scale, q_prescaled=False):
    """(ref, B) in fp64 for o = softmax(scale q k^T) v; q (..., nq, d), k / v (..., nk, d).

        B = 2^-8 |ref| + (2 2^-8 + 2 expm1(delta) + (nk + 4) 2^-23) sum_j p_j |v_j|
        delta = max_j ((d + 2) 2^-23 [+ 2^-8 if q_prescaled]) scale sum_d |q_d| |k_jd|

      * 2^-8 |ref|: the output's rounding to bf16.
      * one 2^-8: P rounded to bf16 in front of the PV MFMA; the other 2^-8: a row sum taken
        from the other form of P (rounded vs. unrounded), so numerator and denominator do not
        cancel their rounding.
      * delta: the error of a score in natural-log units -- d accumulations and the scale /
        max-subtraction in fp32, any rounding.  A score error e changes p_j by a factor within
        e^(+-e) in the numerator and the row sum alike: 2 expm1(delta) relative to sum p |v|.
      * (nk + 4) 2^-23: the PV accumulation, the row-sum accumulation and the final 1 / l.
      * q_prescaled (extension of the issue's derivation, found by reading the kernels):
        attn3_kernel (ls_attn.hip, "qf[g][kc] = ... pack8(f)" after "f[e] *= c2"), and
        attn5_kernel / attnw_kernel with the same lines, multiply Q by scale log2(e) once and
        round the product back to bf16 before the QK^T MFMA.  Each q_d then carries a relative
        error of up to 2^-8, i.e. a score error of up to 2^-8 scale sum_d |q_d| |k_jd|, which
        adds to delta.  attn_kernel and attn_seqm_kernel scale the fp32 score instead.
    The same (1 + 2^-6), + 2^-126 slack as gemm_bound."""
    q, k, v = f64(q), f64(k), f64(v)
    d, nk = q.shape[-1], k.shape[-2]
    s = scale * (q @ k.transpose(-1, -2))
    p = torch.softmax(s, dim=-1)
    ref = p @ v
    smag = scale * (q.abs() @ k.abs().transpose(-1, -2))
    delta = ((d + 2) * E_F32 + (U_BF16 if q_prescaled else 0.0)) * smag.amax(dim=-1, keepdim=True)
    pv = p @ v.abs()
    b = U_BF16 * ref.abs() + (2 * U_BF16 + 2 * torch.expm1(delta) + (nk + 4) * E_F32) * pv
    return ref, _slack(b)


def elem_bound(ref, term_mag, out_dtype):
    """Elementwise kernels (ls_elem.hip): 2^-8 |ref| (1 + 2^-6) for the bf16 rounding, plus
    16 2^-24 term_mag for the fp32 evaluation (at most 8 operations in any rounding mode on
    terms of total magnitude term_mag); fp32 outputs take the second term alone."""
    ref, term_mag = f64(ref), f64(term_mag)
    b = 16 * U_F32 * term_mag
    if out_dtype == torch.bfloat16:
        b = b + U_BF16 * ref.abs() * SLACK
    return b + TINY


def assert_elementwise(got, ref, bound, where=None, name="output"):
    """max(|got - ref| / bound) <= 1 over EVERY element (no mask, no percentile).  Returns the
    worst ratio.  `where` = dict(rows=<rows per tile>, cols=<columns per tile>): the tile sizes
    used to name the failing tile; got is viewed as (rows, cols) = (prod of the leading dims,
    last dim)."""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    ratio = err / bound
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))  # NaN / inf got
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        flat = int(ratio.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        ncol = ratio.shape[-1] if ratio.dim() else 1
        r, c = flat // ncol, flat % ncol
        tr, tc = (where or {}).get("rows", 16), (where or {}).get("cols", 16)
        nbad = int((ratio > 1.0).sum())
        bad_rows = sorted(set((torch.nonzero(ratio.reshape(-1, ncol) > 1.0)[:, 0]).tolist()))
        raise AssertionError(
            f"{name}: err/bound = {worst:.3g} at index {idx} (row {r}, col {c}; row tile {r // tr} of {tr} rows, "
            f"column tile {c // tc} of {tc} columns): got {float(got[idx])!r} ref {float(ref[idx])!r} "
            f"bound {float(bound[idx]):.3g}; {nbad} of {ratio.numel()} elements exceed the bound "
            f"(rows {bad_rows[:8]}{'...' if len(bad_rows) > 8 else ''})")
    return worst


# ---------------------------------------------------------------- guard bands
_SENTINEL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC0A5A5),
             torch.uint8: (torch.uint8, 0xA5)}


class Guarded:
    """A view of the requested shape and pitch inside a larger buffer filled with a sentinel
    bit pattern (bf16 0x7FC1 and fp32 0x7FC0A5A5 are NaNs with a payload; bytes 0xA5)."""

    def __init__(self, buf, view, bits_dtype, sentinel):
        self.buf, self.view, self.bits_dtype, self.sentinel = buf, view, bits_dtype, sentinel

    @property
    def first(self):
        """Element index of the view's first element in buf."""
        return (self.view.data_ptr() - self.buf.data_ptr()) // self.buf.element_size()

    def rows(self, nrows, pitch, before=0):
        """A (nrows, pitch) tensor over the buffer that starts `before` elements in front of
        the view: the whole rows a kernel addresses when it writes only some channels."""
        return torch.as_strided(self.buf, (nrows, pitch), (pitch, 1), self.first - before)


def guarded(shape, pitch=None, pad_rows=2, dtype=torch.bfloat16, device="cpu", offset=0):
    """shape = (..., cols): the view has prod(leading dims) rows of `cols` elements, `pitch`
    elements apart (default cols), with pad_rows sentinel rows before and after (and the
    pitch - cols columns beside every row).  offset shifts the view by that many elements
    (to break 16-byte alignment).  The view itself starts as the sentinel too, so an element
    the kernel never wrote fails the parity check as a NaN."""
    bits_dtype, sentinel = _SENTINEL[dtype]
    cols = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    pitch = cols if pitch is None else pitch
    assert pitch >= cols and 0 <= offset
    n = (rows + 2 * pad_rows) * pitch + offset + 8
    buf = torch.full((n,), sentinel, dtype=bits_dtype, device=device).view(dtype)
    start = pad_rows * pitch + offset
    v = buf[start:start + rows * pitch].view(rows, pitch)[:, :cols]
    strides = []
    acc = pitch
    for s in reversed(shape[:-1]):
        strides.append(acc)
        acc *= s
    view = torch.as_strided(v, tuple(shape), tuple(reversed(strides)) + (1,))
    return Guarded(buf, view, bits_dtype, sentinel)


def assert_guard_intact(g, name="output"):
    """Bit for bit, everything of the buffer outside the view still holds the sentinel."""
    bits = g.buf.view(g.bits_dtype).cpu()
    mask = torch.ones(bits.shape, dtype=torch.bool)
    v = g.view
    first = (v.data_ptr() - g.buf.data_ptr()) // g.buf.element_size()
    idx = torch.arange(v.numel()).reshape(v.shape)
    off = torch.zeros_like(idx) + first
    rem = idx
    for dim in range(v.dim() - 1, -1, -1):
        off = off + (rem % v.shape[dim]) * v.stride(dim)
        rem = rem // v.shape[dim]
    mask[off.reshape(-1)] = False
    want = torch.tensor(g.sentinel, dtype=torch.int64)
    got = bits.to(torch.int64)
    if g.bits_dtype != torch.uint8:
        nbits = 8 * bits.element_size()
        got = got & ((1 << nbits) - 1)
    bad = torch.nonzero(mask & (got != want)).reshape(-1)
    if bad.numel():
        pitch = v.stride(-2) if v.dim() > 1 else v.shape[-1]
        rel = [int(b) - first for b in bad[:8]]
        raise AssertionError(f"{name}: {bad.numel()} element(s) outside the requested view were overwritten; first at "
                             f"(row, col) relative to the view: {[(r // pitch, r % pitch) for r in rel]}")


def snapshot(t):
    return t.detach().clone()


def assert_unchanged(t, snap, name="input"):
    """Bit for bit equal to its snapshot (inputs a kernel must not write)."""
    bits = {2: torch.int16, 4: torch.int32, 1: torch.uint8, 8: torch.int64}[t.element_size()]
    a, b = t.contiguous().view(bits), snap.contiguous().view(bits)
    if not torch.equal(a, b):
        n = int((a != b).sum())
        raise AssertionError(f"{name}: {n} element(s) of an input tensor changed")


# ---------------------------------------------------------------- shared case lists
# (the GPU edge tests run them; tests/test_parity_bounds.py emulates each on the CPU)
EDGE_M = (1, 127, 129, 257, 300)
# (Cin, K, N): K = Cin rounded up to 64 (Cin 72 -> K 128 has a zero-padded tail)
EDGE_KN = ((64, 64, 8), (72, 128, 40), (320, 320, 72), (640, 640, 160), (384, 384, 200))

NEEDLE_KEYS = (0, 15, 16, 31, 32, 63, 64, 127, 128)

# (name, d, heads, nq, nk, q_prescaled): one per dispatch branch of ls_attention
ATTN_CASES = (
    ("attn3_d40_65x50", 40, 2, 65, 50, True),
    ("attn3_d80_130x130", 80, 2, 130, 130, True),
    ("attn3_d64_17x77", 64, 2, 17, 77, True),
    ("attn3_d160_33x40", 160, 2, 33, 40, True),
    ("attn5_d40_130x130", 40, 2, 130, 130, True),
    ("attn5_d40_70x300", 40, 2, 70, 300, True),
    ("attnw512_20x130", 512, 1, 20, 130, True),
    ("generic_d40_65x7", 40, 2, 65, 7, False),
    ("generic_d36_16x20", 36, 2, 16, 20, False),
    ("generic_d256_16x40", 256, 2, 16, 40, False),
    ("generic_d4_16x33", 4, 2, 16, 33, False),
)
SEQM_CASES = tuple((d, n) for d in (40, 80, 160) for n in (1, 7, 16))


def needle_keys(nk):
    return sorted({j for j in NEEDLE_KEYS + (nk - 2, nk - 1) if 0 <= j < nk})


def needle_qkv(batch, heads, nq, nk, d, seed):
    """bf16-rounded q (batch, heads, nq, d), k, v (batch, heads, nk, d), random, with query row
    i (i < number of needle keys, i < nq) rewritten to 8 sqrt(d) k_j / |k_j|^2 for needle key j:
    at scale 1 / sqrt(d) its score on key j is 8, so that tile-boundary key carries most of
    the row's weight."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(batch, heads, nq, d, generator=g)
    k = torch.randn(batch, heads, nk, d, generator=g)
    v = torch.randn(batch, heads, nk, d, generator=g)
    k = bf16_round(k)
    for i, j in enumerate(needle_keys(nk)):
        if i >= nq:
            break
        kj = k[:, :, j]
        q[:, :, i] = 8.0 * math.sqrt(d) * kj / (kj * kj).sum(-1, keepdim=True)
    return bf16_round(q), k, bf16_round(v)
