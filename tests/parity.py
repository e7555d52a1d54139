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


def attn_bound(q, k, v, scale, q_prescaled=False, q_err=None, k_err=None, v_err=None):
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
      * q_err / k_err / v_err (optional, shaped like q / k / v): per-element bounds of what the
        kernel's own q, k, v differ from the reference's by (a fused kernel that projects and
        rounds them itself).  A score moves by at most
        scale sum_d (b_q |k| + |q| b_k + b_q b_k), which joins delta (per row, the maximum over
        the keys); v_j moving by b_v_j moves the result by at most sum_j p_j b_v_j, which joins
        B.  Without them the bound is what it was.
    The same (1 + 2^-6), + 2^-126 slack as gemm_bound."""
    q, k, v = f64(q), f64(k), f64(v)
    d, nk = q.shape[-1], k.shape[-2]
    s = scale * (q @ k.transpose(-1, -2))
    p = torch.softmax(s, dim=-1)
    ref = p @ v
    smag = scale * (q.abs() @ k.abs().transpose(-1, -2))
    delta = ((d + 2) * E_F32 + (U_BF16 if q_prescaled else 0.0)) * smag.amax(dim=-1, keepdim=True)
    if q_err is not None or k_err is not None:
        bq = f64(q_err) if q_err is not None else torch.zeros_like(q)
        bk = f64(k_err) if k_err is not None else torch.zeros_like(k)
        s_in = scale * (bq @ k.abs().transpose(-1, -2) + q.abs() @ bk.transpose(-1, -2) + bq @ bk.transpose(-1, -2))
        delta = delta + s_in.amax(dim=-1, keepdim=True)
    pv = p @ v.abs()
    b = U_BF16 * ref.abs() + (2 * U_BF16 + 2 * torch.expm1(delta) + (nk + 4) * E_F32) * pv
    if v_err is not None:
        b = b + p @ f64(v_err)
    return ref, _slack(b)


U_E4M3 = 2.0 ** -4             # e4m3 keeps 3 fraction bits: round-to-nearest is within 2^-4 relative
FP8_KT = 128                   # keys per tile of attn8_kernel / vt8_quant_kernel


def fp8_scale_exponent(v):
    """The exponent e = e8 - 127 of vt8_quant_kernel's e8m0 scale, per 128-key tile and head-dim
    column: v (..., nk, d) -> (..., ceil(nk / 128), d) int64.  ls_attn.hip: "ex = (int)((
    __float_as_uint(amax) >> 23) & 0xff) - 127", "e = amax > 0.f ? ex - 7 : -127", "e8 = max(0,
    min(254, e + 127))", amax over the tile's 128 keys (the 32 of a thread, then the two xor
    shuffles over the row's four lane groups; keys past nk are zeros)."""
    v = f64(v)
    nk, d = v.shape[-2:]
    nt = -(-nk // FP8_KT)
    vp = torch.zeros(v.shape[:-2] + (nt * FP8_KT, d), dtype=torch.float64)
    vp[..., :nk, :] = v.abs()
    amax = vp.reshape(v.shape[:-2] + (nt, FP8_KT, d)).amax(-2)
    _, ex = torch.frexp(amax)  # amax = f 2^ex, f in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, ex.to(torch.int64) - 1 - 7, torch.full_like(ex, -127, dtype=torch.int64))
    return (e + 127).clamp(0, 254) - 127


def attn_fp8_bound(q, k, v, scale, parts=False):
    """(ref, B) in fp64 for o = softmax(scale q k^T) v of ls_attention_fp8 (vt8_quant_kernel +
    attn8_kernel, ls_attn.hip); q (..., nq, d), k / v (..., nk, d) bf16-rounded.  With eps = 2^-4
    (e4m3's unit roundoff), w the softmax weights and o = ref:

        B = 2^-8 |o|
          + (2 eps / (1 - eps)) sum_j w_j |v_j - o|
          + (2 expm1(delta) + (nk + 6) 2^-23) sum_j w_j |v_j|
          + (1 + 2 eps / (1 - eps)) (sum_j w_j b_v,j + 2^-16 sum_{j: w_j < 2^-11 max w} |v_j - o|)

      * 2^-8 |o|: "w.x = pack2(oacc[g][nd][0] * inv, ...)", the one rounding to bf16.
      * p to e4m3: "pk[g][4 * hf + f] = __builtin_amdgcn_cvt_pk_fp8_f32(fast_exp2(s[g][f][2]), ...)"
        rounds every p to 3 fraction bits, p^ = p (1 + e), |e| <= eps in e4m3's normal range.
        Row D of V^T is the constant 1.0 ("d == D ? 0x38383838u : 0u"), so "lt = __shfl(oacc[g][NDL]
        [RL], ...)" is the sum of the SAME p^ the numerator uses: the weights the kernel applies are
        w^_j = p^_j / sum p^, each within a factor (1 +- eps) / (1 -+ eps) of w_j, and sum w^ =
        sum w = 1, so sum (w^_j - w_j) v_j = sum (w^_j - w_j)(v_j - o): the term is centred on o
        and nearly vanishes on a row one key dominates.
      * delta, in natural-log units, the error of a score:
            delta = ((d + 2) 2^-23 + 2^-8) max_j scale sum_d |q_d| |k_jd|
                  + (d + 2) 2^-23 (max_j |s_j| + 8 ln 2)
        The first line is attn_bound's delta with q_prescaled=True ("f[e] *= c2; qf[g][kc] = ...
        pack8(f)": Q times scale log2(e), rounded to bf16 again).  The second line (an extension,
        read from "s[g][f] = ...mfma_f32_16x16x32_bf16(kf, qf[g][kc], kc == 0 ? negm[g] : s[g][f]"):
        the accumulation chain starts at -m, so its partial sums are as large as |m| + sum |q k|, and
        the integer m is within 8 of a score of the row ("dlt = need ? ceilf(mt[g]) - 7.f", taken
        again whenever "mt[g] > TAU").  It is 10^-4 of the first.  A score error e moves p_j by
        e^(+-e) in numerator and row sum alike.
      * (nk + 6) 2^-23: nk accumulations each of numerator and row sum in the MFMA's fp32
        accumulator (p^ times an e4m3 code times a power of two is exact), "1.f / lt" and the
        product with it; the rescale "oacc[g][i] *= alpha" is the same factor on numerator and sum.
      * b_v,j = max(eps |v_j|, 2^(e - 10)), e = fp8_scale_exponent: "cvt_pk_fp8_f32(v[4 * f] * inv_s,
        ...)" rounds v 2^-e (the tile's row maximum in [128, 256), under e4m3's 448) to nearest:
        2^-4 relative on normal codes, half the 2^-9 subnormal step below 2^-6.  The kernel's
        weights multiply it: sum w^_j b_v,j <= (1 + 2 eps / (1 - eps)) sum w_j b_v,j.
      * subnormal p: under the m in force a half's largest p is at most 2^8 and the row's largest
        was in (2^6, 2^7] when m last moved, so the row sum is at least 2^6 (1 - eps); a p below
        2^-6 lands on e4m3's 2^-9 grid, off by up to 2^-10 absolute, i.e. 2^-16 / (1 - eps) of the
        row sum -- a later rescale shrinks both alike.  Such a key has w_j < 2^-12 max w; the set is
        taken at 2^-11 to cover the score error.  With e_j the absolute errors, numerator - o * sum
        = sum e_j (v_j - o), hence |v_j - o| (restated from |v_j|: the row sum carries e_j too).
    The usual (1 + 2^-6), + 2^-126 slack.  parts=True also returns the terms by name (before the
    slack): round, pquant, score, vquant, sub."""
    q, k, v = f64(q), f64(k), f64(v)
    d, nk = q.shape[-1], k.shape[-2]
    s = scale * (q @ k.transpose(-1, -2))
    w = torch.softmax(s, dim=-1)
    ref = w @ v
    smag = scale * (q.abs() @ k.abs().transpose(-1, -2))
    delta = ((d + 2) * E_F32 + U_BF16) * smag.amax(-1, keepdim=True) \
        + (d + 2) * E_F32 * (s.abs().amax(-1, keepdim=True) + 8 * math.log(2.0))
    e = fp8_scale_exponent(v).repeat_interleave(FP8_KT, dim=-2)[..., :nk, :]
    b_v = torch.maximum(U_E4M3 * v.abs(), torch.pow(2.0, e.to(torch.float64) - 10))
    sub = (w < 2.0 ** -11 * w.amax(-1, keepdim=True)).to(torch.float64)
    # sum_j w_ij |v_jd - o_id| and the subnormal keys' sum_j |v_jd - o_id|, one leading index at a time
    lead = ref.shape[:-2]
    wf, sf, vf, of = (t.reshape((-1,) + t.shape[-2:]) for t in (w, sub, v, ref))
    cen, csub = torch.empty_like(of), torch.empty_like(of)
    for i in range(of.shape[0]):
        dev = (vf[i][None, :, :] - of[i][:, None, :]).abs()  # (nq, nk, d)
        cen[i] = (wf[i][:, :, None] * dev).sum(1)
        csub[i] = (sf[i][:, :, None] * dev).sum(1)
    cen, csub = cen.reshape(lead + cen.shape[-2:]), csub.reshape(lead + csub.shape[-2:])
    g = 2 * U_E4M3 / (1 - U_E4M3)
    t = dict(round=U_BF16 * ref.abs(), pquant=g * cen,
             score=(2 * torch.expm1(delta) + (nk + 6) * E_F32) * (w @ v.abs()),
             vquant=(1 + g) * (w @ b_v), sub=(1 + g) * 2.0 ** -16 * csub)
    b = _slack(t["round"] + t["pquant"] + t["score"] + t["vquant"] + t["sub"])
    return (ref, b, t) if parts else (ref, b)


def elem_bound(ref, term_mag, out_dtype):
    """Elementwise kernels (ls_elem.hip): 2^-8 |ref| (1 + 2^-6) for the bf16 rounding, plus
    16 2^-24 term_mag for the fp32 evaluation (at most 8 operations in any rounding mode on
    terms of total magnitude term_mag); fp32 outputs take the second term alone."""
    ref, term_mag = f64(ref), f64(term_mag)
    b = 16 * U_F32 * term_mag
    if out_dtype == torch.bfloat16:
        b = b + U_BF16 * ref.abs() * SLACK
    return b + TINY


# ---------------------------------------------------------------- LayerNorm, row statistics
def _ln_parts(x, eps):
    """fp64 row quantities of x (rows, C) and the first-order bounds of layernorm_kernel's
    (mean, rstd) (ls_norm.hip), shared by ln_bound and row_stats_bound.

      * mean: C - 1 fp32 additions in any order (per-lane chains, then the 16-lane shuffle tree)
        and one division -- or, in ff_chain_kernel and tattn_fused_kernel, the product with the
        rounded constant 1.f / C, two roundings: |mean' - mu| <= b_mu = (C + 1) 2^-23 mean|x|.
      * the second pass sums fl(x - mean')^2.  With delta = mean' - mu, sum (d - delta)^2 =
        sum d^2 + C delta^2 exactly (sum d = 0), so the mean's error enters the variance only as
        delta^2; every term carries the subtraction's rounding twice and the product's once,
        the sum C - 1 additions, then / C (or * (1.f / C): two) and + eps:
        b_v = (C + 5) 2^-23 (var + eps) + b_mu^2.
      * rstd = rsqrtf(var' + eps), 1 ulp (v_rsq_f32): b_r = r (b_v / (2 (var + eps)) + 2^-23).
    """
    x = f64(x)
    C = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    b_mu = (C + 1) * E_F32 * x.abs().mean(-1, keepdim=True)
    b_v = (C + 5) * E_F32 * (var + eps) + b_mu * b_mu
    b_r = r * (0.5 * b_v / (var + eps) + E_F32)
    return mu, d, r, b_mu, b_r


def ln_bound(x, gamma, beta, pe_row, eps, out_dtype):
    """(ref, B) for y = (x - mu) r gamma + beta (+ pe_row) of layernorm_kernel (ls_norm.hip);
    x (rows, C) bf16-rounded, gamma / beta (C,) fp32, pe_row None or (rows, C): the pe row each
    output row must receive.  ref in fp64; with a = (x - mu) r and (b_mu, b_r) of _ln_parts:

        B = u_out |ref| + |gamma| (r b_mu + |x - mu| b_r) + 5 2^-23 (|a gamma| + |beta| + |pe|)

      * r b_mu: the subtracted mean is off by b_mu; |x - mu| b_r: rstd is off by b_r.
      * 5 2^-23 mag: "(v - mean) * rstd * g + b (+ pe)" is a subtraction, two products and two
        additions, each within 2^-23 of a partial result no larger than mag (a contraction to
        fma only removes roundings).
      * u_out |ref|: the one rounding to bf16 (pack8).
    (1 + 2^-6) and + 2^-126 as everywhere: the products of two first-order terms."""
    mu, d, r, b_mu, b_r = _ln_parts(x, eps)
    g, b = f64(gamma), f64(beta)
    a = d * r
    ref = a * g + b
    mag = (a * g).abs() + b.abs()
    if pe_row is not None:
        ref = ref + f64(pe_row)
        mag = mag + f64(pe_row).abs()
    bnd = _u_out(out_dtype) * ref.abs() + g.abs() * (r * b_mu + d.abs() * b_r) + 5 * E_F32 * mag
    return ref, _slack(bnd)


def row_stats_bound(x, eps):
    """(ref, B), both (rows, 2), for the (mean, rstd) pair of ls_row_stats: the statistics branch
    of layernorm_kernel stores its fp32 mean and rstd as they are, so B = (b_mu, b_r) of
    _ln_parts with the usual slack."""
    mu, _, r, b_mu, b_r = _ln_parts(x, eps)
    return torch.cat([mu, r], -1), _slack(torch.cat([b_mu, b_r], -1))


def ln_propagate(a, r, b_x):
    """First-order effect of a per-element input error b_x on a = (x - mu) r along the last
    dimension (r (..., 1) = 1 / sqrt(var + eps)): for a kernel that normalises a value it has
    itself rounded (ff_chain_kernel's h2, xattn's y).

        |da_i| <= r (b_i + mean(b)) + |a_i| r mean(|a| b)

    From da_i = r (dx_i - dmu) + (x_i - mu) dr with |dmu| <= mean(b), and dr = -r^3 dvar / 2,
    dvar = 2 mean((x - mu)(dx - dmu)) = 2 mean((x - mu) dx) (the dmu part vanishes: mean(x - mu)
    = 0), so |dr| <= r^2 mean(|a| b) and |(x_i - mu) dr| = |a_i| r mean(|a| b).  Second-order
    terms (b^2) are left to the SLACK factor of the bound this feeds."""
    a, r, b_x = f64(a), f64(r), f64(b_x)
    return r * (b_x + b_x.mean(-1, keepdim=True)) + a.abs() * r * (a.abs() * b_x).mean(-1, keepdim=True)


# ---------------------------------------------------------------- GroupNorm statistics
def _gn_ref(mean, var, eps, gamma, beta, cpg):
    """fp64 (scale, shift) (S, C) from per-(sample, group) mean / var (S, G)."""
    r = 1.0 / torch.sqrt(var + eps)
    C = mean.shape[1] * cpg
    g = f64(gamma) if gamma is not None else torch.ones(C, dtype=torch.float64)
    b = f64(beta) if beta is not None else torch.zeros(C, dtype=torch.float64)
    rc, mc = r.repeat_interleave(cpg, 1), mean.repeat_interleave(cpg, 1)
    scale = g * rc
    return scale, b - mc * scale, r, rc, mc, g, b


def _gn_affine_bound(b_mean, b_r, r, rc, mc, g, b, scale, cpg):
    """The tail both GroupNorm finalisers share: sc = gamma * rstd' (one fp32 product) and
    shift = beta - mean' * sc (a product and a subtraction), mean' and rstd' fp32:
        b_sc = |gamma| b_r + 2^-23 |sc|
        b_sh = |sc| b_mean + |mean| b_sc + 2^-23 |mean sc| + 2^-23 (|beta| + |mean sc|)"""
    b_rc, b_mc = b_r.repeat_interleave(cpg, 1), b_mean.repeat_interleave(cpg, 1)
    b_sc = g.abs() * b_rc + E_F32 * scale.abs()
    ms = (mc * scale).abs()
    b_sh = scale.abs() * b_mc + mc.abs() * b_sc + E_F32 * ms + E_F32 * (b.abs() + ms)
    return _slack(b_sc), _slack(b_sh)


def gn_stats_bound(x, groups, eps, gamma, beta, nsplit, R):
    """((scale, shift) fp64, (B_scale, B_shift)), each (S, C), for gn_stats_kernel (ls_norm.hip);
    x (S, pps, C) bf16-rounded (a concat already joined), nsplit and R as ls_groupnorm computes
    them (gn_nsplit; R = 256 / (C / 8) rows of threads, 1 from C / 8 > 256).

    The kernel shifts by k_g = x[s, 0, g cpg] and sums d = x - k_g and d^2 per thread in fp32,
    a thread taking every R-th row of its split: n_t = ceil(ceil(pps / nsplit) / R) terms.
    Everything after the per-thread sums is fp64 (2^-53: left to the slack).
      * S1: each d carries the subtraction's rounding, the chain n_t - 1 additions:
        |S1' - S1| <= n_t 2^-23 sum |d|, so b_m1 = n_t 2^-23 mean|d| on m1 = S1 / n.
      * S2: fl(d)^2 carries two subtraction roundings and the product's, the chain n_t - 1:
        |S2' - S2| <= (n_t + 2) 2^-23 sum d^2.
      * var = S2 / n - m1^2: b_var = (n_t + 2) 2^-23 S2 / n + 2 |m1| b_m1 + b_m1^2 (the
        cancellation the shift leaves is paid through S2 / n = var + m1^2).
      * mean' = (float)(k_g + m1): b_mean = b_m1 + 2^-24 |mean|;
        rstd' = (float)(1 / sqrt(var + eps)): b_r = r (b_var / (2 (var + eps)) + 2^-24).
      * then _gn_affine_bound."""
    x = f64(x)
    S, pps, C = x.shape
    cpg = C // groups
    xg = x.reshape(S, pps, groups, cpg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    scale, shift, r, rc, mc, g, b = _gn_ref(mean, var, eps, gamma, beta, cpg)
    n_t = -(-(-(-pps // nsplit)) // R)
    d = xg - xg[:, :1, :, :1]
    m1 = d.mean((1, 3))
    b_m1 = n_t * E_F32 * d.abs().mean((1, 3))
    b_var = (n_t + 2) * E_F32 * (d * d).mean((1, 3)) + 2 * m1.abs() * b_m1 + b_m1 * b_m1
    b_mean = b_m1 + U_F32 * mean.abs()
    b_r = r * (0.5 * b_var / (var + eps) + U_F32)
    return (scale, shift), _gn_affine_bound(b_mean, b_r, r, rc, mc, g, b, scale, cpg)


def gn_colsum_bound(cs, slots_per_sample, groups, eps, gamma, beta, slot_rows=128):
    """((scale, shift) fp64, (B_scale, B_shift)) for gn_colsum_finalize_kernel; cs (slots, 2, C)
    the given fp32 column sums (a concat already joined along C).  The reference is fp64 on
    those very sums, so what remains is the kernel's fp64 tree (each of the slots cpg terms
    within 2^-52 of sum |terms| whatever the order; var = s2 / n - mean^2 cancels in fp64:
    2^-52 (s2 / n + mean^2) counted once more), the casts (float)mean and (float)rstd
    (2^-24 each), and _gn_affine_bound."""
    cs = f64(cs)
    C = cs.shape[-1]
    cpg = C // groups
    S = cs.shape[0] // slots_per_sample
    n = float(slots_per_sample * slot_rows * cpg)
    t = cs.reshape(S, slots_per_sample, 2, groups, cpg)
    s1, s2 = t[:, :, 0].sum((1, 3)), t[:, :, 1].sum((1, 3))
    a1, a2 = t[:, :, 0].abs().sum((1, 3)), t[:, :, 1].abs().sum((1, 3))
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    scale, shift, r, rc, mc, g, b = _gn_ref(mean, var, eps, gamma, beta, cpg)
    nt = slots_per_sample * cpg
    e64 = 2.0 ** -52
    b_mean64 = nt * e64 * a1 / n
    b_var = nt * e64 * a2 / n + 2 * mean.abs() * b_mean64 + e64 * (a2 / n + mean * mean)
    b_mean = b_mean64 + U_F32 * mean.abs()
    b_r = r * (0.5 * b_var / (var + eps) + U_F32)
    return (scale, shift), _gn_affine_bound(b_mean, b_r, r, rc, mc, g, b, scale, cpg)


def colsum_bound(y, slot_rows=128):
    """(ref, B), each (M / 128, 2, N), for ls_gn_colsum (colsum_pass_kernel, ls_conv.hip): per
    128-row slot the column sums of y and of y^2.  y is bf16, so y^2 is exact in fp32 (and the
    kernel's fma adds it unrounded); what rounds is the additions: 8 chains of 16 rows and the
    8-way merge, fewer than 128 in all, any order: B = 128 2^-23 sum |terms|.
    The other producers of ls_conv_desc.gn_colsum_out sum the same 128 stored bf16 values of a
    slot and column in fp32, each in its own order, so the bound is theirs too when y is the
    kernel's own stored output with its rows in slot order (halo_slot_rows):
      * the tiled epilogue, per pass (store_tile_plain_pre: "t1 += x; t2 = fmaf(x, x, t2)" over
        the WTM staged rows, "g1 += t1" over the slot's passes);
      * the halo conv's register partials (CSG = 2: "q1[j] += b[j]; q2[j] = fmaf(b[j], b[j],
        q2[j])" over a thread's stored rows, then "t1 += v.x" over the RPI threads of a column);
      * the row-block GEMM (RB_GNCS: "t += (v >> 3) ? b * b : b" over a lane's FM rows, row16_sum
        over the 16 lanes, merge_cs "t += part[(sl * WPS + w) * 64 + e]" over the slot's waves;
        b * b of a bf16 b is exact in fp32, contracted to an fma or not)."""
    y = f64(y)
    M, N = y.shape
    t = y.reshape(M // slot_rows, slot_rows, N)
    ref = torch.stack([t.sum(1), (t * t).sum(1)], 1)
    mag = torch.stack([t.abs().sum(1), (t * t).sum(1)], 1)
    return ref, _slack(slot_rows * E_F32 * mag)


def gn_apply_bound(x, scale, shift, silu_on):
    """(ref, B) for y = act(x scale + shift) of gn_apply_kernel / gn_apply_u_kernel; x (S, pps, C)
    bf16-rounded, scale / shift (S, C) the fp32 values handed to the kernel.  The affine is one
    fmaf (2 2^-23 (|x scale| + |shift|) covers the unfused form too), then act_bound's SiLU
    term or, without it, the bf16 rounding alone."""
    x, sc, sh = f64(x), f64(scale)[:, None, :], f64(shift)[:, None, :]
    pre = x * sc + sh
    b_pre = 2 * E_F32 * ((x * sc).abs() + sh.abs())
    if silu_on:
        return act_bound("silu", pre, b_pre, torch.bfloat16)
    return pre, _slack(b_pre + U_BF16 * pre.abs())


# ---------------------------------------------------------------- composing a fused kernel's bound
def chain_linear(b_gemm, w, b_in):
    """A linear stage out = in w^T whose input is itself only known to b_in (rows, K): the
    stage's own gemm_bound b_gemm (rows, N) plus sum_k |w_nk| b_in_k."""
    return f64(b_gemm) + f64(b_in) @ f64(w).abs().transpose(-1, -2)


def chain_round(b, value):
    """An intermediate the kernel rounds to bf16 (and the reference does not): + 2^-8 |value|."""
    return f64(b) + U_BF16 * f64(value).abs()


def ln_from_stats_bound(x, stats):
    """(a, B) for the in-register LayerNorm of ff_fused_kernel / xattn_fused_kernel (ls_ff.hip
    "v[e] = (__bf16)fmaf((float)v[e], rstd, nmr)" with "nmr = -mr.x * mr.y"; the same two lines
    in ls_xattn.hip): a = (x - mean) rstd in fp64 from the GIVEN fp32 (mean, rstd) rows, one
    rounded product nmr, one fma, one rounding to bf16:
        B = 2^-8 |a| + 2 2^-23 (|x rstd| + |mean rstd|)"""
    x, st = f64(x), f64(stats)
    m, r = st[:, :1], st[:, 1:2]
    a = (x - m) * r
    return a, _slack(U_BF16 * a.abs() + 2 * E_F32 * ((x * r).abs() + (m * r).abs()))


def _linear(a, w, bias=None, res=None):
    """(value, magnitude) of a w^T (+ bias) (+ res) in fp64."""
    a, w = f64(a), f64(w)
    v, m = a @ w.T, a.abs() @ w.abs().T
    for t in (bias, res):
        if t is not None:
            v, m = v + f64(t), m + f64(t).abs()
    return v, m


def _geglu_ff(a, b_a, w1g, b1, b1_mag, w2):
    """The FeedForward body both fused kernels share (ff_fused_kernel's chunk loop, reused by
    ff_chain_kernel's phase B): pre = W1 a + b1 in fp32 (C accumulations; a known to b_a; the
    host folded b1 = b + W beta in fp32: (C + 2) 2^-23 b1_mag), G = h gelu(g) rounded to bf16
    ("gv[r] = (__bf16)((acc[0][r] + hb0[r]) * gelu_erf(acc[1][r] + gb0[r]))"): geglu_bound.
    Returns (G, b_G, W2 G, its magnitude, the bound chain_linear(., W2, b_G) adds)."""
    W1 = f64(w1g)
    inner, C = W1.shape[0] // 2, W1.shape[1]
    pre, mag = _linear(a, W1, b1)
    b_pre = chain_linear(gemm_bound(pre, mag, C, None), W1, b_a) + (C + 2) * E_F32 * f64(b1_mag)
    G, b_G = geglu_bound(pre[:, :inner], b_pre[:, :inner], pre[:, inner:], b_pre[:, inner:], torch.bfloat16)
    return G, b_G


def ff_bound(x, stats, w1g, b1, b1_mag, w2, b2):
    """(ref, B) for y = x + W2 GEGLU(W1 LN(x) + b1) + b2 of ff_fused_kernel, composed stage by
    stage: ln_from_stats_bound -> _geglu_ff -> the second GEMM (inner accumulations, + b2 + x,
    one rounding to bf16) with chain_linear for G's own bound.  w1g (2 inner, C) = [h; g] rows
    with gamma folded and rounded to bf16 once, b1 its fp64 bias b + W beta with b1_mag =
    |b| + |W| |beta|; w2 (C, inner) bf16-rounded."""
    a, b_a = ln_from_stats_bound(x, stats)
    G, b_G = _geglu_ff(a, b_a, w1g, b1, b1_mag, w2)
    y, mag = _linear(G, w2, b2, x)
    return y, chain_linear(gemm_bound(y, mag, G.shape[1], torch.bfloat16), w2, b_G)


def ff_chain_bound(o, h1, xb, wo, bo, w1g, b1, b1_mag, w2, b2, wp, bp, eps):
    """(ref z, B) for ff_chain_kernel (ls_ff.hip), the kernel's intermediate roundings in order:
      1. h2 = o Wo^T + bo + h1 rounded to bf16 (phase A: "init_cols(a.bo); proj(0);" then
         "pk0 = pack2(out[f][t][0] + ...)": C accumulations, bias, residual): gemm_bound(bf16).
      2. LayerNorm of that rounded h2 with the kernel's own fp32 statistics ("mean =
         xor16_32_sum(s1) * (1.0f / C)", "rstd = rsqrtf(...)"), rounded to bf16
         (acc_to_operand: "v[e] = (__bf16)((out[f][2 * s + (e >> 2)][e & 3] - mean) * rstd)"):
         ln_propagate of b_h2, the statistics' own error r b_mu + |h2 - mu| b_r (_ln_parts),
         and (2^-8 + 3 2^-23) |a| for the subtraction, the product and the rounding.
      3. the FeedForward body (_geglu_ff); its accumulators start at h2 + b2 ("out[f][t][0] +=
         b.x"), so y = h2 + W2 G + b2 carries b_h2 one to one, and is rounded to bf16 as phase
         C's operand ("acc_to_operand(f, 0.f, 1.f)").
      4. z = y Wp^T + bp + xb rounded to bf16 (phase C and the epilogue's pack2)."""
    C = f64(wo).shape[0]
    h2, mag = _linear(o, wo, bo, h1)
    b_h2 = gemm_bound(h2, mag, C, torch.bfloat16)
    mu, d, r, b_mu, b_r = _ln_parts(h2, eps)
    a = d * r
    b_a = _slack(ln_propagate(a, r, b_h2) + r * b_mu + d.abs() * b_r + (U_BF16 + 3 * E_F32) * a.abs())
    G, b_G = _geglu_ff(a, b_a, w1g, b1, b1_mag, w2)
    y, mag = _linear(G, w2, b2, h2)
    b_y = chain_linear(gemm_bound(y, mag, G.shape[1], torch.bfloat16), w2, b_G) + b_h2
    z, mag = _linear(y, wp, bp, xb)
    return z, chain_linear(gemm_bound(z, mag, C, torch.bfloat16), wp, b_y)


def stored_row_stats_bound(y, eps, chain=8):
    """(ref, B), each (rows, 2), for (mean, rstd) of the STORED bf16 rows y as a GEMM epilogue
    emits them (xattn_fused_kernel: "c1 += (b0 + b1) + (b2 + b3)", "c2 = fmaf(b0, b0, ...)" per
    32-column chunk, then double): fp32 chains of `chain` terms (8 2^-23 of sum |y|, of sum y^2),
    fp64 from there on, var = S2 / C - mean^2 paying 2 |mean| b_mean, the casts 2^-24.
    The same bound holds for the row-block GEMM's RB_STATS epilogue (ls_conv_rowblock.hip,
    "cs1[i] = __builtin_amdgcn_fdot2_f32_bf16(py, one2, ...fdot2_f32_bf16(px, one2, cs1[i], ...))"
    over the 2 fragments of a 32-column chunk, then "S1[i] += (double)cs1[i]"): a lane sums 8
    stored values per chunk in fp32 and everything after that in double.  Where the plan reports
    a trailing ls_row_stats pass instead (ls_conv_plan_info.row_stats), row_stats_bound applies."""
    y = f64(y)
    mu = y.mean(-1, keepdim=True)
    m2 = (y * y).mean(-1, keepdim=True)
    var = (m2 - mu * mu).clamp_min(0.0)
    r = 1.0 / torch.sqrt(var + eps)
    b_m = chain * E_F32 * y.abs().mean(-1, keepdim=True)
    b_var = chain * E_F32 * m2 + 2 * mu.abs() * b_m
    return torch.cat([mu, r], -1), _slack(torch.cat([b_m + U_F32 * mu.abs(), r * (0.5 * b_var / (var + eps) + U_F32)], -1))


def ln_fold_bound(x, stats, w, colsum, bias, rowvec=None, res=None, out_scale=1.0, out_dtype=torch.bfloat16,
                  form="rows"):
    """(ref, B), each (M, N), for a LayerNorm-folded linear of ls_conv2d (ln_rowstats / ln_colsum):

        ref = out_scale (sum_k (x_k - mean) rstd w_k + bias + rowvec + res)      in fp64

    on the operands handed to the kernel: x (M, K) bf16-rounded, stats (M, 2) the GIVEN fp32
    (mean, rstd) rows, w (N, K) the packed bf16 weight (gamma folded, logical row order), colsum
    (N,) the fp32 ln_colsum as handed over, bias (N,) fp32 or None, rowvec / res (M, N) or None
    (the row each output row receives).  out_dtype None: the pre-activation value (compose with
    act_bound / geglu_bound as for any GEMM).  The fold has two arithmetics:

    form="rows": gemm_rowblock_kernel (ls_conv_rowblock.hip) normalises its register-resident A
      rows, "v[e] = (__bf16)fmaf((float)v[e], rstd, nmr)" with "nmr = -mrow[i].x * mrow[i].y",
      and runs a plain GEMM on them (colsum is not read).  So a = (x - mean) rstd is known to
      ln_from_stats_bound's b_a, and
          B = gemm_bound(ref, mag, K, out_dtype) + |out_scale| sum_k |w_k| b_a_k      (chain_linear)
      with mag = |out_scale| (sum_k |a_k w_k| + |bias| + |rowvec| + |res|).

    form="epilogue": the tiled kernels (store_tile_plain_pre "x = mr[it].y * (v[j] - mr[it].x *
      cs[j])", store_tile_geglu "h[j] = mr[it].y * (s[j] - mr[it].x * ch[j]) + bh[j]", ln_fold8
      "v[j] = mr.y * (v[j] - mr.x * cs[j])" for epi_chunk / epi_geglu8 / the split-K reduce)
      accumulate the RAW rows, acc = sum_k x_k w_k, and fold afterwards.  The K accumulations
      round at the size of sum |x_k w_k|, which a large row mean makes far larger than the
      result: that cancellation is the form's real cost and is what the bound charges,
          mag = |out_scale| (rstd (sum_k |x_k w_k| + |mean colsum|) + |bias| + |rowvec| + |res|)
          B   = gemm_bound(ref, mag, K + 3, out_dtype) + |out_scale| rstd |mean| |colsum - sum_k w_k|
      * K + 3: the product mean * colsum, the subtraction and the product with rstd are three
        more fp32 operations on partial results no larger than mag (gemm_bound's own + 4 are the
        bias, rowvec, residual and scale);
      * the last term is no tolerance: the kernel subtracts mean * colsum with the fp32 colsum
        the host summed, the reference mean * sum_k w_k exactly; their difference is computed
        here in fp64 from the operands."""
    x, st, w = f64(x), f64(stats), f64(w)
    K = x.shape[1]
    m, r = st[:, :1], st[:, 1:2]
    s = abs(float(out_scale))
    if form == "rows":
        a, b_a = ln_from_stats_bound(x, stats)
        v, mag = a @ w.T, a.abs() @ w.abs().T
        host = None
    elif form == "epilogue":
        cs = f64(colsum)
        wsum = w.sum(1)
        v = r * (x @ w.T - m * wsum)
        mag = r * (x.abs() @ w.abs().T + (m * cs).abs())
        host = r * m.abs() * (cs - wsum).abs()
    else:
        raise ValueError(form)
    for t in (bias, rowvec, res):
        if t is not None:
            v, mag = v + f64(t), mag + f64(t).abs()
    ref, mag = v * float(out_scale), mag * s
    if form == "rows":
        return ref, chain_linear(gemm_bound(ref, mag, K, out_dtype), w, s * b_a)
    return ref, gemm_bound(ref, mag, K + 3, out_dtype) + s * host


def halo_slot_rows(plan, n_img, H, W):
    """(M / 128, 128) int64: the output rows (pixel index (img H + y) W + x of the H x W OUTPUT
    image) whose stored values each 128-row GroupNorm slot of gn_colsum_out sums, for the plan
    (ops.conv_plan) of the call.  Every family but the halo kernel numbers its slots by
    consecutive rows.  conv3x3_halo_kernel (ls_conv_halo.hip, "m0v = ... (int)(img * HW) + (tyb *
    tpr + txb) * (TH * TW)" and store_tile_plain's "(m0 + (long)p * WTM) / CS_ROWS") numbers
    them patch-major: TH x 16 patches (TH = plan halo_th, 16 or 8) in raster order within an
    image, TH 16 / 128 slots per patch, a slot = 8 consecutive image rows of the patch.  Its
    phase form (family 4, "((ph * tpc + tyb) * tpr + txb) * (TH * TW)") patches the H/2 x W/2
    INPUT image, parity ph = 2 py + px outermost within an image, and patch pixel (r, c) is
    stored at output pixel (2 (y0 + r) + py, 2 (x0 + c) + px)."""
    M = n_img * H * W
    assert M % 128 == 0
    if plan["family"] not in (3, 4):
        return torch.arange(M).reshape(M // 128, 128)
    TH, TW = plan["halo_th"], 16
    ph_form = plan["family"] == 4
    Hp, Wp = (H // 2, W // 2) if ph_form else (H, W)  # the image the patches tile
    tpr, tpc = Wp // TW, Hp // TH
    lr = torch.arange(TH * TW)
    r, c = lr // TW, lr % TW
    out = torch.empty(M, dtype=torch.int64)
    for img in range(n_img):
        for ph in range(4 if ph_form else 1):
            for tyb in range(tpc):
                for txb in range(tpr):
                    y, x = tyb * TH + r, txb * TW + c
                    if ph_form:
                        m0v = img * 4 * Hp * Wp + ((ph * tpc + tyb) * tpr + txb) * TH * TW
                        y, x = 2 * y + (ph >> 1), 2 * x + (ph & 1)
                    else:
                        m0v = img * H * W + (tyb * tpr + txb) * TH * TW
                    out[m0v + lr] = (img * H + y) * W + x
    assert torch.equal(out.sort().values, torch.arange(M))  # every output pixel in exactly one slot
    return out.reshape(M // 128, 128)


def rb_chunk_counts(plan, N, M):
    """The set of 32-column chunks per block of gemm_rowblock_kernel for the plan's grid: block
    (rb, ns) owns chunks "[nch * ns / a.ntn, nch * (ns + 1) / a.ntn)" with nch = N / 32 (N the
    packed width) and plan_rowblock's "ntn = max(1, min(nch, (256 + ntm - 1) / ntm))", ntm = M /
    (128 rb_fm); ntm ntn must be the plan's grid.  One chunk: first chunk and the final
    epilogue only; two: the odd tail; three: one steady-state pair; more: the 3-stage ring
    wraps and the past-the-end DMA reload runs in the branch-free body."""
    assert plan["family"] == 1
    nch, ntm = N // 32, M // (128 * plan["rb_fm"])
    ntn = max(1, min(nch, (256 + ntm - 1) // ntm))
    assert ntm * ntn == plan["grid"], (ntm, ntn, plan["grid"])
    return {nch * (ns + 1) // ntn - nch * ns // ntn for ns in range(ntn)}


def _heads(t, n, rows, heads):
    """(n rows, heads d) -> (n, heads, rows, d)."""
    return t.reshape(n, rows, heads, -1).permute(0, 2, 1, 3)


def xattn_bound(x, stats, wq, bq, bq_mag, kv, L, hw, wo, bo, heads=8):
    """(ref y, B) for xattn_fused_kernel (ls_xattn.hip), stage by stage:
      1. a = LN(x) from the given statistics, bf16: ln_from_stats_bound.
      2. q' = Wq a + bq in log2 units (wq = W gamma log2(e) / sqrt(d) rounded to bf16 once, as
         packing.pack_xattn_q / ops.pack_cross_attention do; bq its fp64 bias, folded in fp32 on
         the host: (C + 2) 2^-23 bq_mag), rounded to bf16 ("qk0[r] = (__bf16)(qa[0][r] + bq[0])").
      3. softmax(ln 2 q' k^T) v over the image's L keys: attn_bound with q_err = b_q (P rounded to
         bf16, the row sum of the rounded P, o / l rounded to bf16: "ofr[ja][r] = (__bf16)(o[0][r] *
         inv)" -- attn_bound's three 2^-8 terms).
      4. y = x + Wo o + bo, C accumulations (the padded k-slots add exact zeros), bf16."""
    x = f64(x)
    M, C = x.shape
    n_img = M // hw
    a, b_a = ln_from_stats_bound(x, stats)
    q, mag = _linear(a, wq, bq)
    b_q = chain_round(chain_linear(gemm_bound(q, mag, C, None), wq, b_a) + (C + 2) * E_F32 * f64(bq_mag), q)
    kv = f64(kv)
    k, v = _heads(kv[:, :C], n_img, L, heads), _heads(kv[:, C:2 * C], n_img, L, heads)
    o, b_o = attn_bound(_heads(q, n_img, hw, heads), k, v, math.log(2.0), q_err=_heads(b_q, n_img, hw, heads))
    o, b_o = (t.permute(0, 2, 1, 3).reshape(M, C) for t in (o, b_o))
    y, mag = _linear(o, wo, bo, x)
    return y, chain_linear(gemm_bound(y, mag, C, torch.bfloat16), wo, b_o)


def tattn_bound(x, gamma, bpe, wq_packed, wk, wv, n_samples, F, S, heads, eps):
    """(ref o, B) for tattn_fused_kernel (ls_motion.hip); x rows "(b f) s".
      1. LayerNorm with the kernel's own fp32 statistics, + (beta + pe[f]), bf16
         ("v[e] = (__bf16)fmaf(((float)v[e] - mean[i]) * rstd[i], g8[e], b8[e])"): ln_bound.
      2. q', k, v = W ln (C accumulations), each rounded to bf16 ("pack4(acc[i][j], 1.f)"):
         gemm_bound + chain_linear + chain_round.  wq_packed is wq log2(e) / sqrt(d) rounded to
         bf16 as ops.pack_temporal stores it; the reference divides the pre-scale out again in
         fp64 and takes the softmax at scale 1 / sqrt(d).
      3. softmax over the F frames of a pixel and P V: attn_bound with q_err, k_err, v_err."""
    x = f64(x)
    C = x.shape[1]
    d = C // heads
    sc = math.log2(math.e) / math.sqrt(d)
    frame = (torch.arange(x.shape[0]) // S) % F
    ln, b_ln = ln_bound(x, gamma, torch.zeros(C), f64(bpe)[frame], eps, torch.bfloat16)
    out = []
    for w in (f64(wq_packed) / sc, wk, wv):
        p, mag = _linear(ln, w)
        b_p = chain_round(chain_linear(gemm_bound(p, mag, C, None), w, b_ln), p)
        # rows (b f) s -> (b, s, head, f, d)
        out += [t.reshape(n_samples, F, S, heads, d).permute(0, 2, 3, 1, 4) for t in (p, b_p)]
    q, b_q, k, b_k, v, b_v = out
    o, b_o = attn_bound(q, k, v, 1.0 / math.sqrt(d), q_err=b_q, k_err=b_k, v_err=b_v)
    back = lambda t: t.permute(0, 3, 1, 2, 4).reshape(n_samples * F * S, C)
    return back(o), back(b_o)


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


def needle_qkv(batch, heads, nq, nk, d, seed, keys=None):
    """bf16-rounded q (batch, heads, nq, d), k, v (batch, heads, nk, d), random, with query row
    i (i < number of needle keys, i < nq) rewritten to 8 sqrt(d) k_j / |k_j|^2 for needle key j:
    at scale 1 / sqrt(d) its score on key j is 8, so that tile-boundary key carries most of
    the row's weight.  keys: the needle keys (default needle_keys(nk))."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(batch, heads, nq, d, generator=g)
    k = torch.randn(batch, heads, nk, d, generator=g)
    v = torch.randn(batch, heads, nk, d, generator=g)
    k = bf16_round(k)
    for i, j in enumerate(needle_keys(nk) if keys is None else keys):
        if i >= nq:
            break
        kj = k[:, :, j]
        q[:, :, i] = 8.0 * math.sqrt(d) * kj / (kj * kj).sum(-1, keepdim=True)
    return bf16_round(q), k, bf16_round(v)


# ---------------------------------------------------------------- fp8 attention cases
# (tests/test_gpu_edges_fp8.py runs them; tests/test_parity_bounds.py walks each on the CPU)
# attn8_kernel: 128 queries per block (4 waves x QG 2 x 16), 128-key tiles in two 64-key halves,
# an LDS ring of depth 2.  (nq, nk, batch, heads):
FP8_SHAPES = (
    (1, 1, 2, 2),      # one key
    (17, 77, 2, 2),    # a single partial tile, its second half partly masked
    (33, 64, 2, 2),    # the second half entirely masked
    (130, 128, 2, 2),  # exactly one full tile, no partial one; two query blocks, the second of 2 rows
    (130, 129, 2, 2),  # one key in the partial tile
    (70, 257, 2, 2),   # three tiles: the ring's slot is reused
    (129, 385, 2, 2),  # four tiles
    (65, 300, 1, 3),   # a grid of 3 blocks: attn_xcd_remap's remainder branch
)
FP8_CASES = tuple((f"d{d}_{nq}x{nk}_{kind}", d, batch, heads, nq, nk, kind)
                  for d in (40, 80) for nq, nk, batch, heads in FP8_SHAPES for kind in ("needle", "random6"))
# keys that separate the three fields of the permutation 16 (j >> 2) + 4 lg + (j & 3)
FP8_PERM_KEYS = (3, 4, 12, 20, 67, 191, 192, 256)


def fp8_needle_keys(nk):
    return sorted({j for j in NEEDLE_KEYS + FP8_PERM_KEYS + (nk - 2, nk - 1) if 0 <= j < nk})


def fp8_qkv(d, batch, heads, nq, nk, kind, seed=37):
    """bf16-rounded q (batch, heads, nq, d), k, v (batch, heads, nk, d) of an fp8 case.
    "needle": needle_qkv on fp8_needle_keys, V times a power of two in 2^-6 .. 2^6 per (batch,
    head, key), so a scale byte from another row or tile shows.  "random6": Gaussian, Q times 6:
    scores of deviation 6 (8.7 in log2 units), so the running m moves often and by little.
    (The seed is one at which the one-key cases have a row with a score below -4 at d 40 and 80:
    tests/test_parity_bounds.py asserts that, and its coverage conditions, from the inputs.)"""
    seed = 100000 * seed + 1000 * nq + 10 * nk + d
    if kind == "needle":
        q, k, v = needle_qkv(batch, heads, nq, nk, d, seed, keys=fp8_needle_keys(nk))
        g = torch.Generator().manual_seed(seed + 1)
        return q, k, v * torch.pow(2.0, torch.randint(-6, 7, (batch, heads, nk, 1), generator=g).float())
    if kind != "random6":
        raise ValueError(kind)
    g = torch.Generator().manual_seed(seed)
    r = lambda n: bf16_round(torch.randn(batch, heads, n, d, generator=g))
    q, k, v = r(nq), r(nk), r(nk)
    return bf16_round(6.0 * q), k, v


# ---------------------------------------------------------------- norm cases (tests/test_gpu_edges_norm.py)
LN_C = (8, 136, 320, 520, 1024, 1280, 1536, 1664, 2048)  # layernorm_kernel<NCH>: 1, 2, 3, 5, 8, 10, 12, 16, 16
LN_ROWS = (1, 15, 17, 33)
LN_PE_RPF, LN_PE_FRAMES = 3, 4  # the frame index wraps inside 33 rows
LN_EPS = 1e-5


def ln_case(rows, C, mean_sigmas, seed=0):
    """bf16-rounded x (rows, C) with row standard deviations 0.5 .. 2 and row means of
    mean_sigmas standard deviations; fp32 gamma, beta (C,), pe (LN_PE_FRAMES, C)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + rows)
    sig = 0.5 + 1.5 * torch.rand(rows, 1, generator=g)
    x = bf16_round(sig * (torch.randn(rows, C, generator=g) + mean_sigmas))
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    pe = 0.5 * torch.randn(LN_PE_FRAMES, C, generator=g)
    return x, gamma, beta, pe


def ln_pe_rows(pe, rows, rpf=LN_PE_RPF, frames=LN_PE_FRAMES):
    """The pe row every output row receives: pe[(row // rpf) % frames]."""
    return pe[(torch.arange(rows) // rpf) % frames]


GN_THREADS = 256


def gn_R(C):
    """Pixel rows of threads per block of gn_stats_kernel (ls_norm.hip, "if (CC <= GN_THREADS)
    { R = GN_THREADS / CC; ..." and the same two lines in gn_nsplit / ls_groupnorm)."""
    CC = C // 8
    return GN_THREADS // CC if CC <= GN_THREADS else 1


def gn_nsplit(n_samples, pps, C):
    """gn_nsplit of ls_norm.hip: min(ceil(512 / n_samples), pps / (8 R)), clamped to [1, 4096]."""
    ns = min(-(-512 // n_samples), pps // (8 * gn_R(C)))
    return max(1, min(ns, 4096))


def _gn_cases():
    out = []
    for C in (32, 96, 320):  # 32 groups; C = 96: cpg 3, groups straddle the 16-byte chunks
        for pps in (1, 7, 8 * gn_R(C) + 1, 4096):
            out.append((f"c{C}_p{pps}", C, 0, 32, 3, pps))
    for pps in (1, 7, 9):  # C / 8 = 320 > 256 threads: the nchunk > 1 branch, R = 1
        out.append((f"c2560_p{pps}", 2560, 0, 32, 3, pps))
    out.append(("c2560_p4096_one", 2560, 0, 32, 1, 4096))  # 512 splits on one accumulator and ticket
    for pps in (1, 7, 8 * gn_R(128) + 1, 4096):  # 64 groups: the L = 4 branch
        out.append((f"c128g64_p{pps}", 128, 0, 64, 3, pps))
    for pps in (1, 7, 8 * gn_R(160) + 1, 4096):  # concat: group 19 (channels 95 .. 99) straddles x1 | x2
        out.append((f"cat96+64_p{pps}", 96, 64, 32, 3, pps))
    out.append(("c32_520x4", 32, 0, 32, 520, 4))  # nsplit 1, many samples
    out.append(("c32_p4096_one", 32, 0, 32, 1, 4096))
    out.append(("c320_p4096_one", 320, 0, 32, 1, 4096))
    return tuple(out)


GN_CASES = _gn_cases()  # (name, C1, C2, groups, n_samples, pps)
GN_MEANS = (0, 10, 30)  # mean / std
GN_EPS = 1e-5


def gn_case(C1, C2, n_samples, pps, mean_sigmas, seed=0):
    """bf16-rounded x (n_samples, pps, C1 + C2), unit standard deviation, sample s at a mean of
    mean_sigmas (1 + s / 8), and the x2 half of a concat a further 5 higher (so the group that
    straddles the boundary sees both levels); fp32 gamma, beta."""
    C = C1 + C2
    g = torch.Generator().manual_seed(1000 * seed + 13 * C + pps + n_samples)
    x = torch.randn(n_samples, pps, C, generator=g)
    x = x + mean_sigmas * (1.0 + torch.arange(n_samples).reshape(-1, 1, 1) / 8.0)
    if C2:
        x[:, :, C1:] += 5.0
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    return bf16_round(x), gamma, beta


# ls_groupnorm_colsum on synthetic column sums: (cpg, slots per sample, C1, C2 or None = the rest),
# 32 groups, 3 samples; the concat boundary C1 falls inside a group wherever cpg > 1
_GN_COLSUM_C1 = {1: 24, 3: 64, 5: 96, 40: 768}
GN_COLSUM_CASES = tuple((cpg, slots, C1, C2) for cpg in (1, 3, 5, 40) for slots in (1, 3)
                        for C1, C2 in ((32 * cpg, 0), (_GN_COLSUM_C1[cpg], None)))


def gn_colsum_case(cpg, slots, C1, C2, seed=0):
    """fp32 column sums cs1 (3 slots, 2, C1), cs2 (3 slots, 2, C2) or None, as a producer would
    emit them for data of mean 2 and unit deviation; gamma, beta."""
    C = 32 * cpg
    C2 = C - C1 if C2 is None else C2
    g = torch.Generator().manual_seed(1000 * seed + 17 * cpg + slots + C1)
    y = bf16_round(torch.randn(3 * slots * 128, C, generator=g) + 2.0).reshape(3 * slots, 128, C)
    cs = torch.stack([y.sum(1), (y * y).sum(1)], 1)  # fp32 sums: the kernel's input as it is
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    cs1 = cs[:, :, :C1].contiguous()
    cs2 = cs[:, :, C1:].contiguous() if C2 else None
    return cs1, cs2, gamma, beta


# ls_groupnorm_apply: (name, C1, C2, n_samples, pps).  ppb = 256 / (C / 8) pixels per block pass;
# gn_apply_u_kernel (4 ppb pixels per block) needs ppb >= 2 and 4 ppb <= pps, else gn_apply_kernel
GN_APPLY_CASES = (
    ("u_c128_88x3", 128, 0, 3, 88),       # ppb 16: 264 = 4 * 64 + 8, lanes pl >= 8 of the last block have no pixel;
                                          # 88 = 64 + 24: a sample boundary inside the second block's range
    ("u_c96_64x3", 96, 0, 3, 64),         # CC 12, ppb 21: 252 live threads of 256, blocks of 84 pixels over samples of 64
    ("stride_c96_9x5", 96, 0, 5, 9),      # 4 ppb = 84 > pps: the grid-stride kernel, a sample boundary in every pass
    ("stride_c1280_5x3", 1280, 0, 3, 5),  # ppb 1, 160 live lanes of 192: the grid-stride kernel
    ("u_cat96+64_50x3", 96, 64, 3, 50),   # concat, ppb 12, blocks of 48 pixels over samples of 50
    ("stride_cat64+32_9x5", 64, 32, 5, 9),
)


# ---------------------------------------------------------------- fused transformer-block cases
# (tests/test_gpu_edges_ff.py, tests/test_gpu_edges_fused_attn.py)
#
# A composed bound is a worst case: every stage adds sum_k |w_k| b_k, which for dense Gaussian
# weights is about 0.64 sqrt(K) times what the same errors add up to with random signs -- at
# K = 320 / 1280 the bound would be ten to twenty bf16 steps wide and a dropped column would fit
# inside it.  The weights here are therefore a weak dense background (deviation 2^-6 / sqrt(K):
# every packed position still carries a distinct value) under `nnz` strong entries per row
# (deviation 1 / sqrt(nnz)) at random columns, so |sum w a| is within a small factor of
# sum |w a| and the bound stays a few bf16 steps wide.
FF_C, FF_INNER = 320, 1280
FF_M = (1, 127, 129, 300)
FF_CHAIN_M = (128, 384)
FF_W2_NEEDLES = (0, 3, 4, 15, 16, 31, 32, 1279)  # inner columns of W2 scaled by 8
FF_W1_NEEDLES = (0, 31, 32, 319)                 # k-columns of W1 scaled by 8
LOG2E = math.log2(math.e)


def sparse_weight(n, k, nnz, seed, bg=2.0 ** -6):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * (bg / math.sqrt(k))
    idx = torch.rand(n, k, generator=g).argsort(1)[:, :nnz]
    return w.scatter_(1, idx, torch.randn(n, nnz, generator=g) / math.sqrt(nnz))


def host_row_stats(x, eps=1e-5):
    """fp32 (mean, rstd) rows as a producer would hand them over (the kernels take them as they are)."""
    x = f64(x)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return torch.cat([mu, 1.0 / torch.sqrt(var + eps)], -1).float()


def _ff_weights(seed):
    """Logical FeedForward tensors: gamma, beta, w1 (2 inner, C) = [h; g], b1, w2 (C, inner), b2,
    and what the reference uses: w1g = w1 gamma rounded to bf16 once (unet._Dev.packed_ln), b1f =
    b1 + w1 beta in fp64 with its magnitude, w2 rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    C, inner = FF_C, FF_INNER
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w1 = sparse_weight(2 * inner, C, 8, seed + 1)
    w1[:, list(FF_W1_NEEDLES)] *= 8.0
    b1 = 0.1 * torch.randn(2 * inner, generator=g)
    w2 = sparse_weight(C, inner, 16, seed + 2)
    w2[:, list(FF_W2_NEEDLES)] *= 8.0
    b2 = 0.1 * torch.randn(C, generator=g)
    return dict(gamma=gamma, beta=beta, w1=w1, b1=b1, w2=w2, b2=b2,
                w1g=bf16_round(w1 * gamma[None, :]), b1f=f64(b1) + f64(w1) @ f64(beta),
                b1_mag=f64(b1).abs() + f64(w1).abs() @ f64(beta).abs(), w2r=bf16_round(w2))


def ff_case(M, seed=0):
    """ls_feedforward inputs: x (M, C) bf16-rounded, its fp32 row statistics, _ff_weights."""
    g = torch.Generator().manual_seed(100 * seed + M)
    x = bf16_round(4.0 * torch.randn(M, FF_C, generator=g) + 0.5)
    return dict(x=x, stats=host_row_stats(x), **_ff_weights(40 + seed))


def ff_chain_case(M, seed=0):
    """ls_ff_chain inputs: o, h1, xb (M, C), to_out (wo, bo), the FeedForward, proj_out (wp, bp)."""
    g = torch.Generator().manual_seed(200 * seed + M)
    r = lambda *s: torch.randn(*s, generator=g)
    C = FF_C
    out = dict(o=bf16_round(r(M, C)), h1=bf16_round(4.0 * r(M, C) + 0.5), xb=bf16_round(4.0 * r(M, C)),
               wo=sparse_weight(C, C, 8, seed + 61), bo=0.1 * r(C), wp=sparse_weight(C, C, 8, seed + 62), bp=0.1 * r(C),
               **_ff_weights(50 + seed))
    out["wor"], out["wpr"] = bf16_round(out["wo"]), bf16_round(out["wp"])
    return out


XA_HW, XA_IMGS = 128, 3
XA_L = (1, 7, 50, 64)
XA_NEEDLE_KEYS = (0, 15, 16, 31, 32)  # and L - 1: V rows scaled by 16


def xattn_case(L, seed=0):
    """ls_cross_attention_block inputs: x (3 * 128, 320), its statistics, to_q (C, C) with norm2's
    gamma / beta, kv (3 L, 2 C) = k | v with small keys (scores within a fraction of a log2 unit:
    the bound's score term stays small) and the V rows of the needle keys scaled by 16, to_out."""
    C, heads = 320, 8
    M = XA_IMGS * XA_HW
    g = torch.Generator().manual_seed(300 * seed + L)
    r = lambda *s: torch.randn(*s, generator=g)
    x = bf16_round(4.0 * r(M, C) + 0.5)
    gamma, beta = 1.0 + 0.2 * r(C), 0.1 * r(C)
    wq, wo, bo = sparse_weight(C, C, 8, seed + 71), sparse_weight(C, C, 8, seed + 72), 0.1 * r(C)
    kv = torch.cat([0.25 * r(XA_IMGS * L, C), r(XA_IMGS * L, C)], 1)
    for j in sorted({j for j in XA_NEEDLE_KEYS + (L - 1,) if j < L}):
        kv[j::L, C:] *= 16.0
    sc = LOG2E / math.sqrt(C // heads)
    return dict(x=x, stats=host_row_stats(x), gamma=gamma, beta=beta, wq=wq, wo=wo, bo=bo, kv=bf16_round(kv),
                wqr=bf16_round((wq * gamma[None, :]) * sc), bqf=(f64(wq) @ f64(beta)) * sc,
                bq_mag=(f64(wq).abs() @ f64(beta).abs()) * sc, wor=bf16_round(wo))


TA_CASES = ((320, 16), (640, 8))  # (C, S): two blocks per sample each
TA_F = (1, 5, 7, 16)
TA_SAMPLES = 2


def tattn_case(C, S, F, seed=0):
    """ls_temporal_attention inputs: x rows "(b f) s" (2 F S, C), LayerNorm gamma / beta, pe (24, C),
    the logical wq, wk (small, as xattn_case's keys), wv, and wqp = wq log2(e) / sqrt(d) rounded to
    bf16 as ops.pack_temporal stores it, wkr, wvr."""
    heads = 8
    g = torch.Generator().manual_seed(400 * seed + C + F)
    r = lambda *s: torch.randn(*s, generator=g)
    x = bf16_round(2.0 * r(TA_SAMPLES * F * S, C) + 0.5)
    gamma, beta, pe = 1.0 + 0.2 * r(C), 0.1 * r(C), 0.5 * r(24, C)
    wq, wk, wv = sparse_weight(C, C, 8, seed + 81), 0.25 * sparse_weight(C, C, 8, seed + 82), sparse_weight(C, C, 8, seed + 83)
    sc = LOG2E / math.sqrt(C // heads)
    bpe = beta.reshape(1, C).repeat(16, 1) + pe[:16]
    return dict(x=x, gamma=gamma, beta=beta, pe=pe, bpe=bpe, wq=wq, wk=wk, wv=wv, wqp=bf16_round(wq * sc),
                wkr=bf16_round(wk), wvr=bf16_round(wv))


# ---------------------------------------------------------------- Whisper log-mel (ls_audio.hip)
MEL_NFFT, MEL_HOP, MEL_NFREQ, MEL_BLOCK = 400, 160, 201, 8  # MEL_BLOCK: frames per block of log_mel_kernel
MEL_LOG_FLOOR = float(torch.tensor(1e-10, dtype=torch.float32))  # the kernel's 1e-10f


def mel_frame_index(n, T):
    """(T, 400) int64: the sample frame t reads at window position m, t 160 + m - 200 reflected
    once at either end (torch.stft centre=True, pad_mode="reflect"; n > 200 keeps it in range)."""
    j = torch.arange(T)[:, None] * MEL_HOP + torch.arange(MEL_NFFT)[None, :] - MEL_NFFT // 2
    j = j.abs()
    return torch.where(j >= n, 2 * (n - 1) - j, j)


def log_mel_bound(wave, filters, t_pad):
    """(l_ref, l_bound, v_ref, v_bound) in fp64 for ls_log_mel (log_mel_kernel + mel_norm_kernel,
    ls_audio.hip): l (T, n_mels) the fp32 log-mel rows of the workspace, v (t_pad, n_mels) the bf16
    output; wave (n,) fp32 samples, filters (n_mels, 201) fp32, T = n // 160.

    Oracle: the exact STFT -- periodic Hann 400 (0.5 - 0.5 cos(2 pi m / 400)), hop 160, centre
    reflect padding (mel_frame_index), X_k = sum_m x_m w_m e^(-2 pi i k m / 400) with the twiddle
    index k m reduced mod 400 in integers, P_k = |X_k|^2, s_b = sum_k f_bk P_k, l = log10(max(s,
    1e-10)); floor = max(l) - 8 over the whole clip, v = (max(l, floor) + 4) / 4, rows T .. t_pad
    zero.

    Bound, as an interval carried through the monotone steps:
      * one DFT component.  With A_f = sum_m |x_m w_m| of the frame, re and im are each off by at
        most E_f = (400 + 8) 2^-23 A_f: 400 sequential fp32 accumulations in any rounding (the
        products may or may not be contracted), and 8 more units for what each term carries
        before it is summed -- the sincospif table (cs[], sn[] within 2 ulp), the Hann value 0.5 -
        0.5 cs[m] (a product and a subtraction of numbers <= 1), the product with the sample and
        the product with the twiddle.
      * P_k = re^2 + im^2: |dP_k| <= 2 (|re| + |im|) E_f + 2 E_f^2 + 3 2^-23 P_k (two squares and
        the addition).
      * s_b: the filter weights are non-negative, so ds_b = sum_k f_bk dP_k + 202 2^-23 s_b (201
        products and additions of non-negative terms, any order).
      * l in [log10(max(s - ds, 1e-10)), log10(max(s + ds, 1e-10))], widened by 4 2^-23 |l| for
        log10f (2 ulp) and fmaxf's exactness; l_bound is the larger distance of l_ref to an end.
      * the floor lies between the maxima of the two ends minus 8 (the kernel's maximum is the
        maximum of values inside their intervals; ord_enc / atomicMax are exact), and
        v = (max(l, floor) + 4) / 4 is monotone in l and in the floor, so its interval comes from
        the two ends; then 3 2^-23 (|max(l, floor)| + 4) / 4 for the three fp32 operations (- 8,
        + 4, / 4) and 2^-8 |v| for the round-to-nearest bf16 store (f2bf).  v_bound is the larger
        distance of v_ref to an end.  The zero rows are exact (their bound is the 2^-126 of the
        slack alone; the GPU test also compares their bits).
    (1 + 2^-6) and + 2^-126 as everywhere."""
    x = f64(wave).reshape(-1)
    fb = f64(filters)
    n = x.numel()
    T = n // MEL_HOP
    n_mels = fb.shape[0]
    m = torch.arange(MEL_NFFT)
    win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * m.to(torch.float64) / MEL_NFFT)
    xw = x[mel_frame_index(n, T)] * win  # (T, 400)
    ph = 2.0 * math.pi * ((torch.arange(MEL_NFREQ)[:, None] * m[None, :]) % MEL_NFFT).to(torch.float64) / MEL_NFFT
    re, im = xw @ torch.cos(ph).T, -(xw @ torch.sin(ph).T)  # (T, 201)
    pw = re * re + im * im
    E = (MEL_NFFT + 8) * E_F32 * xw.abs().sum(1, keepdim=True)
    dP = 2 * (re.abs() + im.abs()) * E + 2 * E * E + 3 * E_F32 * pw
    s = pw @ fb.T
    ds = dP @ fb.T + (MEL_NFREQ + 1) * E_F32 * s
    log = lambda t: torch.log10(t.clamp_min(MEL_LOG_FLOOR))
    l_ref, lo, hi = log(s), log(s - ds), log(s + ds)
    lo, hi = lo - 4 * E_F32 * lo.abs(), hi + 4 * E_F32 * hi.abs()
    l_bound = _slack(torch.maximum(hi - l_ref, l_ref - lo))
    lo, hi = l_ref - l_bound, l_ref + l_bound  # the slack carried on
    norm = lambda l, fl: (torch.maximum(l, fl) + 4.0) / 4.0
    f_ref, f_lo, f_hi = l_ref.max() - 8.0, lo.max() - 8.0, hi.max() - 8.0
    f_lo, f_hi = f_lo - E_F32 * f_lo.abs(), f_hi + E_F32 * f_hi.abs()
    v, v_lo, v_hi = norm(l_ref, f_ref), norm(lo, f_lo), norm(hi, f_hi)
    ops3 = 3 * E_F32 * (torch.maximum(torch.maximum(lo, f_lo).abs(), torch.maximum(hi, f_hi).abs()) + 4.0) / 4.0
    b = torch.maximum(v_hi - v, v - v_lo) + ops3 + U_BF16 * torch.maximum(v_lo.abs(), v_hi.abs())
    v_ref = torch.zeros(t_pad, n_mels, dtype=torch.float64)
    v_bound = torch.zeros(t_pad, n_mels, dtype=torch.float64)
    v_ref[:T], v_bound[:T] = v, b
    return l_ref, l_bound, v_ref, _slack(v_bound)


def mel_signal(n, kind="mix", seed=1):
    """fp32 test waves of n samples (shared by the CPU demonstrations and the GPU cases).
    "mix": a 100 Hz -> 7 kHz chirp of amplitude 0.2 plus white noise of deviation 0.2 -- every band
    of every frame has energy, so no band sits on spectral leakage alone.  The floor cases:
    "zeros_after" (the mix, exact zeros from the middle on), "quiet_after" (the mix, from the
    middle on at -60 dB), "loud_first" / "loud_last" (the mix at 1e-4, more than 8 in log10 power
    below its first 160 samples / the span of its last frame, which stay at full level), "zeros", "noise1e-3" (white noise of deviation 1e-3: every log value is
    negative).  (The seed is one at which no band of the one- and two-frame clips falls, by chance,
    thousands of times below its neighbours: tests/test_parity_bounds.py asserts from the inputs
    that at most 1 % of the bounds of any signal used are wider than 2^-6.)"""
    g = torch.Generator().manual_seed(1000 * seed + n)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    dur = max(n / 16000.0, 1e-3)
    chirp = 0.2 * torch.sin(2 * math.pi * (100.0 * t + 0.5 * (7000.0 - 100.0) / dur * t * t))
    mix = (chirp + 0.2 * torch.randn(n, generator=g, dtype=torch.float64)).float()
    h = n // 2
    if kind == "mix":
        return mix
    if kind == "zeros_after":
        mix[h:] = 0.0
        return mix
    if kind == "quiet_after":
        mix[h:] *= 1e-3
        return mix
    if kind in ("loud_first", "loud_last"):
        mix *= 1e-4
        if kind == "loud_first":
            mix[:MEL_HOP] *= 1e4
        else:
            mix[(n // MEL_HOP - 1) * MEL_HOP - MEL_HOP // 2:] *= 1e4
        return mix
    if kind == "zeros":
        return torch.zeros(n)
    if kind == "noise1e-3":
        return (1e-3 * torch.randn(n, generator=g, dtype=torch.float64)).float()
    raise ValueError(kind)


MEL_N = (201, 319, 320, 1279, 1319, 1320, 4000, 4159, 40000)  # T = 1, 1, 2, 7, 8, 8, 25, 25, 250
MEL_FLOOR_KINDS = ("zeros_after", "quiet_after", "loud_first", "loud_last", "zeros", "noise1e-3")
MEL_FLOOR_N = 4159  # T = 25: three full blocks of 8 frames and one frame in the partial block


# ---------------------------------------------------------------- time embedding (ls_elem.hip)
LN_10000 = math.log(10000.0)


def timestep_bound(t, dim, shift, flip=True):
    """(ref, B), each (len(t), dim) fp64, for ls_timestep_embed / ls_timestep_embed_f32
    (timestep_embed_kernel, timestep_embed_f32_kernel of ls_elem.hip); t the timesteps as the
    kernel converts them to fp32 (integers, or the fp32 values themselves).

        ref[:, i], ref[:, half + i] = cos, sin (flip) or sin, cos of t exp(-ln(10000) i / (half - shift))

    in fp64, half = dim / 2.  The kernel's argument "t * expf(-9.210340371976184f * (float)i /
    ((float)half - shift))" carries 7 roundings of at most 2^-23 each (any mode): the constant, the
    product with i, the subtraction half - shift and the division -- four that reach expf's input x_i =
    ln(10000) i / (half - shift) and so move its result by a relative |x_i| each --, expf itself
    (2: 1 ulp of OCML's expf, rounded up), and the product with t.  The error of the argument is
    therefore proportional to it, |d arg| <= (4 x_i + 3) 2^-23 |arg|, and sin and cos (slope <= 1)
    move by no more; sinf / cosf add 4 2^-23 absolute (2 ulp of a result <= 1, rounded up).  At
    i = 0 every step is exact (0 / d = 0, expf(0) = 1, t * 1 = t): only the 4 2^-23 remain.
    The slack of gemm_bound on top."""
    t = f64(t).reshape(-1, 1)
    half = dim // 2
    i = torch.arange(half, dtype=torch.float64)[None, :]
    x = LN_10000 * i / (half - float(shift))
    arg = t * torch.exp(-x)
    rel = torch.where(i == 0, torch.zeros_like(x), (4 * x + 3) * E_F32)
    b = _slack(rel * arg.abs() + 4 * E_F32)
    sn, cs = torch.sin(arg), torch.cos(arg)
    ref = torch.cat([cs, sn] if flip else [sn, cs], 1)
    return ref, torch.cat([b, b], 1)


def dot_bound(x, w, bias, silu_in):
    """(ref, B), each (M, N) fp64, for ls_small_linear (small_linear_kernel, ls_elem.hip):
    y = act(x) W^T + bias with x (M, K) fp32, W (N, K) bf16-rounded, bias (N,) fp32 or None, fp32 out.

        B = 2^-24 |ref| + (2 K + 8 + 64 + 4) 2^-23 mag + [silu_in] sum_k |w_k| 8 2^-23 |x_k|
        mag = sum_k |act(x_k) w_k| + |bias|

    gemm_bound with k_terms = 2 K + 72: x is fp32 and W bf16, so -- unlike the MFMA GEMMs -- every
    product "f[j] * xs[mm * K + k + j]" rounds: K products and K additions, plus the 8-wide inner
    sum "s += ..." that is added to acc[mm] and the 64-lane wave_sum; gemm_bound's own + 4 holds the
    bias.  (No single term passes through more than 1 + 8 + K / 512 + 6 + 1 of these roundings, so
    the count is generous; it is the count an order-free restatement may use.)  With silu_in the
    kernel evaluates silu(x_k) in fp32 before the sum: act_bound's evaluation term 8 2^-23 |x_k| on
    every x_k, carried through |w_k|.  The result is stored unrounded (fp32): u_out = 2^-24."""
    x, w = f64(x), f64(w)
    K = x.shape[1]
    a = _silu(x) if silu_in else x
    ref, mag = _linear(a, w, bias)
    b = gemm_bound(ref, mag, 2 * K + 8 + 64, torch.float32)
    if silu_in:
        b = b + _slack((8 * E_F32 * x.abs()) @ w.abs().T)
    return ref, b


TS_T = (1, 501, 951, 999)
TS_DIMS = (320, 6)
# (M, K, N): one row; the model's three layers' shapes; N % 4 = 1 (waves past N return early);
# M = 9 / 19 (a last row chunk of 1 / 3 rows), K = 8 (one lane works) and K = 2048, M = 1024 (the limits)
SMALL_LINEAR_CASES = ((1, 320, 1280), (2, 1280, 1280), (8, 1280, 3001), (9, 8, 5), (19, 2048, 7), (1024, 320, 6))
