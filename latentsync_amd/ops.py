"""Thin torch-tensor wrappers over the C-ABI (include/ls_hip.h).

Tensors are device buffers owned by the caller (torch caching allocator); the
wrappers only compute shapes, fill the descriptors and launch on the current
HIP stream, so every call is capturable in a hipGraph (torch.cuda.CUDAGraph).
Activations are NHWC bf16: (images, H, W, C) with frames folded into images.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import check

ACT_NONE, ACT_GEGLU, ACT_GELU, ACT_SILU = 0, 1, 2, 3
_GN_EPILOGUE = True  # False: GroupNorm statistics by a read pass (tests patch it)
GN_SLOT_ROWS = 128  # LS_GN_SLOT_ROWS
# False: upsample convs with phase-packed weights (Packed.phase) stay on the 9-tap form (tests patch it)
_UPS_PHASE = True


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Workspace:
    """Fixed-size per-device scratch (split-K partials, GroupNorm partials).  Never
    re-allocated after creation so captured graphs keep valid pointers."""

    def __init__(self, device, gemm_bytes=256 << 20, gn_bytes=24 << 20):
        self.gemm = torch.empty(gemm_bytes, dtype=torch.uint8, device=device)
        self.gn = torch.zeros(gn_bytes, dtype=torch.uint8, device=device)  # GN arrival counters start at 0


_WS = {}


def workspace(device) -> Workspace:
    key = torch.device(device).index or 0
    if key not in _WS:
        _WS[key] = Workspace(device)
    return _WS[key]


class Packed:
    """A contraction operand ready for ls_conv2d: w bf16 [N][K] (tap-major,
    K padded to 64), bias fp32 [N] or None."""

    def __init__(self, w, bias, cin, ksize, n_out, geglu=False):
        self.w, self.bias, self.cin, self.ksize = w, bias, cin, ksize
        self.N, self.K = w.shape
        self.n_out = n_out
        self.geglu = geglu
        self.colsum = None  # set for LayerNorm-folded weights (unet._Dev.packed_ln)
        self.pe_rows = None  # W pe table for a folded LayerNorm + positional encoding
        # bf16 [4][N][4 cin]: the phase-packed form of a 3x3 weight (packing.pack_phase_weight)
        # for conv(..., upsample=True); w stays the 9-tap operand for the shapes it cannot take
        self.phase = None


def _ld(t):
    """Pixel stride of an NHWC view (n, H, W, C): pixel p = (img*H + y)*W + x must
    live at p * ld (channels contiguous)."""
    n, H, W, C_ = t.shape
    st = t.stride()
    ld = st[2] if W > 1 else (st[1] if H > 1 else (st[0] if n > 1 else C_))
    ok = (C_ == 1 or st[3] == 1) and (W == 1 or st[2] == ld) and (H == 1 or st[1] == W * ld) and \
        (n == 1 or st[0] == H * W * ld)
    if not ok:
        raise ValueError(f"NHWC view with non-uniform pixel strides {tuple(st)} for shape {tuple(t.shape)}")
    return ld


def conv_path(x, pw: Packed, **kw):
    """Which kernel family ls_conv2d takes for this call (ls_conv_path: 0 tiled, 1 row-block,
    2 register-staged, 3 halo-tile 3x3, 4 / 5 the halo-tile / tiled phase form of an upsample
    conv) -- host only, nothing is launched."""
    return conv(x, pw, _query="path", **kw)


def conv_plan(x, pw: Packed, **kw):
    """The plan ls_conv2d makes for this call (ls_conv_plan), as a dict of the integers of
    ls_conv_plan_info: family (= conv_path), kernel instance, launch geometry, trailing passes
    -- host only, nothing is launched.  None where the library refuses the descriptor
    (_lib.load().ls_last_error() has the reason)."""
    return conv(x, pw, _query="plan", **kw)


def conv(x, pw: Packed, *, x2=None, aff=None, stride=1, pad=None, upsample=False, out_hw=None, rowvec=None,
         res=None, out_scale=1.0, act=ACT_NONE, out=None, out_f32=False, split_k=0, ln_stats=None,
         stats_out=None, gn_out=False, aff_materialize=False, workspace_bytes=None, _query=None):
    """Fused conv/linear.  x (n, H, W, C1) [+ x2 (n, H, W, C2)] -> (n, Ho, Wo, n_out).
    aff = (scale[S][C], shift[S][C], imgs_per_sample, silu); rowvec = (t[S][ld], rows_per_vec, ld[, mod]);
    ln_stats = (mean, rstd) rows from row_stats(): LayerNorm folded into pw (pw.colsum);
    stats_out = fp32 (rows, 2) receiving row_stats() of the output (eps 1e-5);
    upsample = nearest x2 before the 3x3: with pw.phase set, as four 2x2 phase convs
    (ls_conv_desc.upsample = 2) where ls_conv_path takes that form (4, 5), else the 9-tap form;
    gn_out = also emit the output's GroupNorm column sums (ls_conv_desc.gn_colsum_out),
    attached to the result as `.gn_cs` for group_norm() (when rows % 128 == 0); a caller's
    contiguous fp32 (rows / 128, 2, n_out) tensor instead of True receives them (shape-checked);
    aff_materialize = when the call would take the register-staged GEMM for the affine
    prologue (ls_conv_path 2), apply it with ls_groupnorm_apply first instead (the
    row-block GEMM folds it into its register-resident A rows);
    workspace_bytes = a cap on the split-K workspace of this call (0: none; default: all of it,
    handed over with the launch -- conv_path / conv_plan then answer for a call without one)."""
    lib = _lib.load()
    n, H, W, C1 = x.shape
    C2 = x2.shape[3] if x2 is not None else 0
    assert C1 + C2 == pw.cin, (C1, C2, pw.cin)
    ks = pw.ksize
    if pad is None:
        pad = 1 if ks == 3 else 0
    if out_hw is not None:
        Ho, Wo = out_hw
    elif ks == 1:
        Ho, Wo = H, W
    else:
        He, We = (2 * H, 2 * W) if upsample else (H, W)
        Ho, Wo = (He + 2 * pad - 3) // stride + 1, (We + 2 * pad - 3) // stride + 1
    n_out = pw.n_out if act != ACT_GEGLU else pw.N // 2
    if out is None:
        out = torch.empty((n, Ho, Wo, n_out), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    ws = workspace(x.device)
    d = _lib.ConvDesc()
    d.x1, d.x2, d.C1, d.C2 = _p(x), _p(x2), C1, C2
    d.ld1, d.ld2 = _ld(x), (_ld(x2) if x2 is not None else 0)
    d.n_img, d.H, d.W, d.Ho, d.Wo = n, H, W, Ho, Wo
    d.ksize, d.stride, d.pad, d.upsample = ks, stride, pad, int(upsample)
    if aff is not None:
        d.aff_scale, d.aff_shift, d.imgs_per_sample, d.silu_in = _p(aff[0]), _p(aff[1]), aff[2], int(aff[3])
    d.w, d.K, d.N = _p(pw.w), pw.K, pw.N
    d.bias = _p(pw.bias)
    if rowvec is not None:
        d.rowvec, d.rows_per_vec, d.rowvec_ld = _p(rowvec[0]), rowvec[1], rowvec[2]
        d.rowvec_mod = rowvec[3] if len(rowvec) > 3 else 0
    if ln_stats is not None:
        assert pw.colsum is not None, "ln_stats needs LayerNorm-folded weights"
        d.ln_rowstats, d.ln_colsum = _p(ln_stats), _p(pw.colsum)
    if res is not None:
        d.res, d.ldr = _p(res), (_ld(res) if res.dim() == 4 else res.stride(-2))
    d.out_scale = out_scale
    d.act = act
    assert tuple(out.shape) == (n, Ho, Wo, n_out), (tuple(out.shape), (n, Ho, Wo, n_out))
    d.y, d.ldy, d.y_f32 = _p(out), _ld(out), int(out.dtype == torch.float32)
    d.split_k = split_k
    if workspace_bytes:
        d.workspace, d.workspace_bytes = _p(ws.gemm), min(workspace_bytes, ws.gemm.numel())
    if stats_out is not None:
        assert stats_out.dtype == torch.float32 and stats_out.is_contiguous() and stats_out.numel() == 2 * n * Ho * Wo
        assert pw.n_out == pw.N and act != ACT_GEGLU, "row statistics over the real output channels only"
        d.row_stats_out, d.row_stats_eps = _p(stats_out), 1e-5
    if upsample and pw.phase is not None and _UPS_PHASE and aff is None:
        # the one decision: the library says whether this call has a phase-form kernel
        # (4 halo-tile, 5 tiled); an input affine never has one, so it is not asked
        d.upsample, d.w, d.K = 2, _p(pw.phase), pw.phase.shape[2]
        if lib.ls_conv_path(C.byref(d)) not in (4, 5):
            d.upsample, d.w, d.K = 1, _p(pw.w), pw.K
    if aff is not None and aff_materialize and not _query and lib.ls_conv_path(C.byref(d)) == 2:
        xa = group_norm_apply(x, aff[0], aff[1], n // aff[2], bool(aff[3]), x2=x2)
        return conv(xa, pw, stride=stride, pad=pad, upsample=upsample, out_hw=out_hw, rowvec=rowvec, res=res,
                    out_scale=out_scale, act=act, out=out, out_f32=out_f32, split_k=split_k, ln_stats=ln_stats,
                    stats_out=stats_out, gn_out=gn_out, workspace_bytes=workspace_bytes)
    cs = None
    cs_ok = (n * Ho * Wo) % GN_SLOT_ROWS == 0 and out.dtype == torch.bfloat16 and act != ACT_GEGLU
    if torch.is_tensor(gn_out):  # the caller's buffer: always filled (no silent skip)
        assert cs_ok and pw.n_out == pw.N, "gn_out buffer: rows % 128 == 0, bf16 output, no GEGLU"
        assert gn_out.dtype == torch.float32 and gn_out.is_contiguous() and gn_out.device == x.device and \
            tuple(gn_out.shape) == (n * Ho * Wo // GN_SLOT_ROWS, 2, n_out), (tuple(gn_out.shape), gn_out.dtype)
        cs = gn_out
    elif gn_out and _GN_EPILOGUE and cs_ok:
        assert pw.n_out == pw.N
        cs = torch.empty((n * Ho * Wo // GN_SLOT_ROWS, 2, n_out), dtype=torch.float32, device=x.device)
    if cs is not None:
        d.gn_colsum_out = _p(cs)
    # the questions are asked without the split-K workspace unless workspace_bytes names one:
    # the library splits K on its own only where it has a workspace, so a shape it would split
    # (few tiles, deep K) is answered here as unsplit
    if _query == "path":
        return lib.ls_conv_path(C.byref(d))
    if _query == "plan":
        info = _lib.ConvPlanInfo()
        if lib.ls_conv_plan(C.byref(d), C.byref(info)) != 0:
            return None
        return {f: getattr(info, f) for f, _ in info._fields_}
    if workspace_bytes is None:
        d.workspace, d.workspace_bytes = _p(ws.gemm), ws.gemm.numel()
    check(lib.ls_conv2d(C.byref(d), _stream()), "ls_conv2d")
    if cs is not None:
        out.gn_cs = cs
    return out


def linear(x2d, pw: Packed, **kw):
    """Token-row linear: x2d (rows, C) -> (rows, n_out).  x2d / res / out may be
    row-strided views (stride(1) == 1)."""
    rows = x2d.shape[0]
    for k in ("res", "out"):
        if kw.get(k) is not None and kw[k].dim() == 2:
            kw[k] = kw[k].unsqueeze(0).unsqueeze(0)
    y = conv(x2d.unsqueeze(0).unsqueeze(0), pw, **kw)
    return y.view(rows, y.shape[-1]) if y.is_contiguous() else y[0, 0]


def gn_colsum(x):
    """Column sums of an existing NHWC bf16 activation (ls_gn_colsum), attached as
    x.gn_cs -- for GroupNorm inputs no GEMM epilogue produced."""
    lib = _lib.load()
    C_ = x.shape[-1]
    rows = x.numel() // C_
    cs = torch.empty((rows // GN_SLOT_ROWS, 2, C_), dtype=torch.float32, device=x.device)
    check(lib.ls_gn_colsum(_p(x), C_, rows, C_, _p(cs), _stream()), "ls_gn_colsum")
    x.gn_cs = cs
    return cs


def _colsums(x, pps):
    cs = getattr(x, "gn_cs", None)
    if cs is None or pps % GN_SLOT_ROWS or not x.is_contiguous():
        return None
    C_ = x.shape[-1]
    return cs if tuple(cs.shape) == (x.numel() // C_ // GN_SLOT_ROWS, 2, C_) else None


def group_norm(x, groups, eps, gamma, beta, n_samples, x2=None):
    """GroupNorm statistics -> (scale, shift) fp32 [n_samples][C].  From the producer's
    column sums (x.gn_cs, conv(..., gn_out=True)) when present, else a read pass."""
    lib = _lib.load()
    C1 = x.shape[-1]
    C2 = x2.shape[-1] if x2 is not None else 0
    pps = x.numel() // C1 // n_samples
    scale = torch.empty((n_samples, C1 + C2), dtype=torch.float32, device=x.device)
    shift = torch.empty_like(scale)
    cs1 = _colsums(x, pps)
    cs2 = _colsums(x2, pps) if x2 is not None else None
    if cs1 is not None and (x2 is None or cs2 is not None):
        check(lib.ls_groupnorm_colsum(_p(cs1), _p(cs2), C1, C2, n_samples, pps, groups, eps, _p(gamma), _p(beta),
                                      _p(scale), _p(shift), _stream()), "ls_groupnorm_colsum")
        return scale, shift
    ws = workspace(x.device)
    check(lib.ls_groupnorm(_p(x), _p(x2), C1, C2, n_samples, pps, groups, eps, _p(gamma), _p(beta), _p(scale),
                           _p(shift), _p(ws.gn), ws.gn.numel(), _stream()), "ls_groupnorm")
    return scale, shift


def group_norm_apply(x, scale, shift, n_samples, silu, x2=None):
    """Materialise act(GN(x | x2)) -> (n, H, W, C1 + C2) bf16."""
    lib = _lib.load()
    C1 = x.shape[-1]
    C2 = x2.shape[-1] if x2 is not None else 0
    n_pix = x.numel() // C1
    y = torch.empty(x.shape[:-1] + (C1 + C2,), dtype=torch.bfloat16, device=x.device)
    check(lib.ls_groupnorm_apply(_p(x), _p(x2), C1, C2, n_pix, n_pix // n_samples, _p(scale), _p(shift), int(silu),
                                 _p(y), _stream()), "ls_groupnorm_apply")
    return y


def affine_act(x, scale, shift, n_samples, silu):
    return group_norm_apply(x, scale, shift, n_samples, silu)


def row_stats(x2d, eps=1e-5):
    """(mean, rstd) fp32 per row of x2d (rows, C) (row-strided views allowed)."""
    lib = _lib.load()
    rows, C_ = x2d.shape
    assert x2d.stride(1) == 1
    st = torch.empty((rows, 2), dtype=torch.float32, device=x2d.device)
    check(lib.ls_row_stats(_p(x2d), x2d.stride(0), rows, C_, eps, _p(st), _stream()), "ls_row_stats")
    return st


def layer_norm(x2d, gamma, beta, eps=1e-5, pe=None, pe_rows_per_frame=1, pe_frames=1):
    """x2d (rows, C), rows may be strided (x2d.stride(1) == 1); y dense (rows, C)."""
    lib = _lib.load()
    rows, C_ = x2d.shape
    assert x2d.stride(1) == 1
    y = torch.empty((rows, C_), dtype=x2d.dtype, device=x2d.device)
    check(lib.ls_layernorm(_p(x2d), x2d.stride(0), rows, C_, eps, _p(gamma), _p(beta), _p(pe), pe_rows_per_frame, pe_frames, _p(y),
                           _stream()), "ls_layernorm")
    return y


def attention(q, k, v, o, *, batch, z2, heads, nq, nk, head_dim, qs, ks, vs, os_, scale=None, fp8=False,
              fp8_workspace=None):
    """qs/ks/vs/os_ = (sb1, sb2, si, sh) element strides; q/k/v/o base tensors
    (may be offset views).  fp8=True: ls_attention_fp8 (P V on the block-scaled e4m3
    MFMA, configs[4]); its V quantisation lands in `fp8_workspace` (uint8, allocated
    here when None -- tests pass their own to read it back)."""
    lib = _lib.load()
    d = _lib.AttnDesc()
    d.q, d.k, d.v, d.o = _p(q), _p(k), _p(v), _p(o)
    for t, st in zip("qkvo", (qs, ks, vs, os_)):
        for name, val in zip(("sb1", "sb2", "si", "sh"), st):
            setattr(d, f"{t}_{name}", int(val))
    d.batch, d.z2, d.heads, d.nq, d.nk, d.head_dim = batch, z2, heads, nq, nk, head_dim
    d.scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    if fp8:
        n = lib.ls_attention_fp8_workspace_bytes(C.byref(d))
        if n == 0:
            raise ValueError(f"ls_attention_fp8: head_dim {head_dim} unsupported (40, 80)")
        if fp8_workspace is None:
            fp8_workspace = torch.empty(n, dtype=torch.uint8, device=q.device)
        check(lib.ls_attention_fp8(C.byref(d), _p(fp8_workspace), fp8_workspace.numel(), _stream()),
              "ls_attention_fp8")
        return o
    check(lib.ls_attention(C.byref(d), _stream()), "ls_attention")
    return o


class TemporalPack:
    """Packed operands of ls_temporal_attention for one VersatileAttention block."""

    def __init__(self, w, gamma, bpe, C, heads, eps=1e-5):
        self.w, self.gamma, self.bpe, self.C, self.heads, self.eps = w, gamma, bpe, C, heads, eps


def pack_temporal(wq, wk, wv, ln_weight, ln_bias, pe, heads, device):
    """ls_temporal_attention operands (include/ls_hip.h) from the reference tensors of one
    VersatileAttention block and its LayerNorm (motion_module.py:203-218, :262-313):
    q|k|v rows per 80-channel group as (q_t, k_t, v_t) 16-row tiles, the q rows scaled
    by log2(e)/sqrt(d) (the kernel's softmax works in log2 units), gamma, and
    beta + pe[f] for f < 16."""
    C = wq.shape[0]
    d = C // heads
    sc = math.log2(math.e) / math.sqrt(d)
    rows = []
    for g in range(C // 80):
        for t in range(5):  # (q_t, k_t, v_t): 16-channel tiles of the group in turn
            cs = slice(80 * g + 16 * t, 80 * g + 16 * t + 16)
            rows += [wq[cs].float() * sc, wk[cs].float(), wv[cs].float()]
    w = torch.cat(rows).to(torch.bfloat16)
    bpe = ln_bias.float().reshape(1, C).repeat(16, 1)
    if pe is not None:
        n = min(16, pe.shape[0])
        bpe[:n] += pe[:n].float().cpu()
    return TemporalPack(w.to(device).contiguous(), ln_weight.float().to(device).contiguous(),
                        bpe.to(device).contiguous(), C, heads)


def temporal_attention_ok(C, heads, F, S):
    """Shapes ls_temporal_attention takes (else the q|k|v GEMM + ls_attention path)."""
    return heads == 8 and 1 <= F <= 16 and ((C == 320 and S % 16 == 0) or (C == 640 and S % 8 == 0))


def temporal_attention(x2d, pk: TemporalPack, n_samples, F, S, out=None):
    """LayerNorm + pe + q|k|v + temporal SDPA of a motion-module attention block in one
    launch (ls_temporal_attention).  x2d (n_samples*F*S, C) rows "(b f) s" -> o, same rows."""
    lib = _lib.load()
    rows, C_ = x2d.shape
    assert C_ == pk.C and rows == n_samples * F * S and x2d.stride(1) == 1
    if out is None:
        out = torch.empty((rows, C_), dtype=torch.bfloat16, device=x2d.device)
    d = _lib.TAttnDesc()
    d.x, d.ldx, d.gamma, d.bpe, d.w = _p(x2d), x2d.stride(0), _p(pk.gamma), _p(pk.bpe), _p(pk.w)
    d.o, d.ldo = _p(out), out.stride(0)
    d.C, d.heads, d.n_samples, d.F, d.S, d.eps = pk.C, pk.heads, n_samples, F, S, pk.eps
    check(lib.ls_temporal_attention(C.byref(d), _stream()), "ls_temporal_attention")
    return out


def feedforward_ok(x2d, w1: "Packed", w2: "Packed"):
    """Shapes ls_feedforward takes (else the GEGLU row-block GEMM + the W2 GEMM)."""
    return (x2d.shape[1] == 320 and w1.N == 2560 and w1.K == 320 and w1.geglu and w2.N == 320 and w2.K == 1280
            and x2d.stride(1) == 1 and x2d.stride(0) % 8 == 0)


def feedforward(x2d, ln_stats, w1: "Packed", w2: "Packed", w2ff, out=None):
    """y = x + W2 GEGLU(W1 LN(x) + b1) + b2 in one launch (ls_feedforward): x2d (M, 320)
    rows, ln_stats (M, 2) their (mean, rstd); w1 the LN-folded GEGLU operand, w2 the W2
    operand (bias), w2ff = packing.pack_ff_w2(W2) bf16."""
    lib = _lib.load()
    M, C_ = x2d.shape
    if out is None:
        out = torch.empty((M, C_), dtype=torch.bfloat16, device=x2d.device)
    d = _lib.FFDesc()
    d.x, d.ln_rowstats, d.w1, d.b1 = _p(x2d), _p(ln_stats), _p(w1.w), _p(w1.bias)
    d.w2, d.b2, d.y = _p(w2ff), _p(w2.bias), _p(out)
    d.M, d.ldx, d.ldy, d.C, d.inner = M, x2d.stride(0), out.stride(0), C_, w1.N // 2
    check(lib.ls_feedforward(C.byref(d), _stream()), "ls_feedforward")
    return out


class FFChainPack:
    """ls_ff_chain operands of one block tail (packing.pack_ff_chain): to_out, the
    LN-folded GEGLU W1 (k permuted), W2 (pack_ff_w2), proj_out (k permuted)."""

    def __init__(self, wo, bo, w1, b1, w2, b2, wp, bp, C, inner, eps):
        self.wo, self.bo, self.w1, self.b1, self.w2, self.b2, self.wp, self.bp = wo, bo, w1, b1, w2, b2, wp, bp
        self.C, self.inner, self.eps = C, inner, eps


def pack_ff_chain(wo: "Packed", ff1: "Packed", ff2: "Packed", po: "Packed", eps=1e-5):
    """FFChainPack from the packed operands of the unfused path: to_out (C, C) + bias, the
    LN-folded GEGLU W1 (interleaved, gamma folded) + bias, W2 + bias, proj_out + bias."""
    from .packing import pack_ff_w2, permute_k_acc
    Cc = wo.N
    bf = lambda t: t.to(torch.bfloat16).contiguous()
    w1 = permute_k_acc(ff1.w.float())
    return FFChainPack(bf(pack_ff_w2(wo.w.float()[:, :Cc], permute=False)), wo.bias.float().contiguous(), bf(w1),
                       ff1.bias.float().contiguous(), bf(pack_ff_w2(ff2.w.float()[:, :ff2.K])),
                       ff2.bias.float().contiguous(), bf(pack_ff_w2(po.w.float()[:, :Cc])),
                       po.bias.float().contiguous(), Cc, ff1.N // 2, eps)


def ff_chain_ok(o2d, pk: "FFChainPack"):
    return (pk is not None and o2d.shape[1] == 320 and pk.inner == 1280 and o2d.shape[0] % 128 == 0
            and o2d.stride(1) == 1 and o2d.stride(0) % 8 == 0)


def ff_chain(o2d, h1, xb, pk: "FFChainPack", shape=None, gn_out=True):
    """z = proj_out(FF(LN(h2)) + h2) + xb with h2 = to_out(o) + h1, one launch (ls_ff_chain);
    o2d / h1 / xb (M, C) rows; z is allocated with `shape` (default (M, C)) and carries
    .gn_cs (its GroupNorm column sums) for group_norm()."""
    lib = _lib.load()
    M, C_ = o2d.shape
    res = torch.empty(shape or (M, C_), dtype=torch.bfloat16, device=o2d.device)
    out = res.view(M, C_)
    cs = torch.empty((M // GN_SLOT_ROWS, 2, C_), dtype=torch.float32, device=o2d.device) if gn_out else None
    d = _lib.FFChainDesc()
    d.o, d.wo, d.bo, d.h1 = _p(o2d), _p(pk.wo), _p(pk.bo), _p(h1)
    d.w1, d.b1, d.w2, d.b2, d.wp, d.bp = _p(pk.w1), _p(pk.b1), _p(pk.w2), _p(pk.b2), _p(pk.wp), _p(pk.bp)
    d.xb, d.z, d.cs_out = _p(xb), _p(out), _p(cs)
    d.M, d.ldo, d.ldh, d.ldxb, d.ldz = M, o2d.stride(0), h1.stride(0), xb.stride(0), out.stride(0)
    d.C, d.inner, d.eps = C_, pk.inner, float(pk.eps)
    check(lib.ls_ff_chain(C.byref(d), _stream()), "ls_ff_chain")
    if cs is not None:
        res.gn_cs = cs
    return res


class XAttnPack:
    """ls_cross_attention_block operands of one BasicTransformerBlock's attn2 + norm2
    (packing.pack_xattn_q / pack_xattn_wo)."""

    def __init__(self, wq, bq, wo, bo, C, heads):
        self.wq, self.bq, self.wo, self.bo, self.C, self.heads = wq, bq, wo, bo, C, heads


def pack_cross_attention(wq, ln_weight, ln_bias, wo, bo, heads, device):
    """XAttnPack from the reference tensors: to_q.weight (C, C), norm2 gamma / beta,
    to_out.0.weight (C, C) / bias -- LayerNorm folded (W gamma, W beta) in fp32 before the
    single bf16 rounding."""
    from .packing import pack_xattn_q, pack_xattn_wo
    w = wq.float().cpu()
    gamma, beta = ln_weight.float().cpu(), ln_bias.float().cpu()
    pq, pb = pack_xattn_q(w * gamma[None, :], w @ beta, heads)
    po = pack_xattn_wo(wo.float().cpu(), heads)
    bf = lambda t: t.to(torch.bfloat16).to(device).contiguous()
    return XAttnPack(bf(pq), pb.to(device).contiguous(), bf(po), bo.float().to(device).contiguous(), w.shape[0], heads)


def cross_attention_ok(x2d, pk, L, hw):
    """Shapes ls_cross_attention_block takes (else q GEMM + ls_attention + out GEMM)."""
    return (pk is not None and x2d.shape[1] == 320 and pk.heads == 8 and 1 <= L <= 64 and hw % 128 == 0
            and x2d.shape[0] % hw == 0 and x2d.stride(1) == 1 and x2d.stride(0) % 8 == 0)


def cross_attention_block(x2d, ln_stats, pk: XAttnPack, kv, L, hw, stats_out, out=None, eps=1e-5):
    """y = x + to_out(attn(to_q(LN(x)), k, v)) for the audio cross attention in one launch
    (ls_cross_attention_block); stats_out (M, 2) receives y's LayerNorm row statistics."""
    lib = _lib.load()
    M, C_ = x2d.shape
    if out is None:
        out = torch.empty((M, C_), dtype=torch.bfloat16, device=x2d.device)
    assert stats_out.dtype == torch.float32 and stats_out.is_contiguous() and stats_out.numel() == 2 * M
    assert kv.stride(1) == 1 and kv.shape[0] == (M // hw) * L and kv.shape[1] >= 2 * C_
    d = _lib.XAttnDesc()
    d.x, d.ln_rowstats, d.wq, d.bq, d.kv, d.wo, d.bo = _p(x2d), _p(ln_stats), _p(pk.wq), _p(pk.bq), _p(kv), \
        _p(pk.wo), _p(pk.bo)
    d.y, d.stats_out = _p(out), _p(stats_out)
    d.M, d.ldx, d.ldy, d.ldkv, d.C, d.heads, d.L, d.hw, d.eps = M, x2d.stride(0), out.stride(0), kv.stride(0), C_, \
        pk.heads, L, hw, eps
    check(lib.ls_cross_attention_block(C.byref(d), _stream()), "ls_cross_attention_block")
    return out


def attention_fp8_workspace_bytes(*, batch, heads, nk, head_dim):
    lib = _lib.load()
    d = _lib.AttnDesc()
    d.batch, d.z2, d.heads, d.nq, d.nk, d.head_dim = batch, 1, heads, 1, nk, head_dim
    return lib.ls_attention_fp8_workspace_bytes(C.byref(d))


def small_linear(x, w, bias, silu_in=False, out=None):
    lib = _lib.load()
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    check(lib.ls_small_linear(_p(x), M, K, _p(w), _p(bias), N, int(silu_in), _p(out), _stream()), "ls_small_linear")
    return out


def timestep_embed(timesteps_i32, step_i32, B, dim, flip=True, shift=0.0, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty((B, dim), dtype=torch.float32, device=timesteps_i32.device)
    check(lib.ls_timestep_embed(_p(timesteps_i32), _p(step_i32), B, dim, int(flip), float(shift), _p(out), _stream()),
          "ls_timestep_embed")
    return out


def timestep_embed_f32(t_f32, dim, flip=True, shift=0.0, out=None):
    """One embedding row per fp32 timestep (forward()'s float / per-sample timesteps)."""
    lib = _lib.load()
    B = t_f32.numel()
    if out is None:
        out = torch.empty((B, dim), dtype=torch.float32, device=t_f32.device)
    check(lib.ls_timestep_embed_f32(_p(t_f32), B, dim, int(flip), float(shift), _p(out), _stream()),
          "ls_timestep_embed_f32")
    return out


def ddim_cfg_step(eps, Bu, guidance, lat, coef, step, unet_in):
    lib = _lib.load()
    P = lat.shape[0]
    check(lib.ls_ddim_cfg_step(_p(eps), eps.shape[-1], Bu, P, float(guidance), _p(lat), _p(coef), _p(step),
                               _p(unet_in), unet_in.shape[-1], _stream()), "ls_ddim_cfg_step")


def resize_faces_u8(src, out_h, out_w, out=None):
    """ImageProcessor.resize (image_processor.py:42-44) of uint8 faces (N,3,H,W) ->
    (N,3,out_h,out_w) uint8: torchvision's antialiased bilinear Resize with its
    round-half-even back to uint8.  ``out`` is a caller's static buffer."""
    lib = _lib.load()
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[1] != 3 or not src.is_cuda:
        raise ValueError(f"resize_faces_u8: uint8 (N,3,H,W) on the device expected, got {src.dtype} "
                         f"{tuple(src.shape)} on {src.device}")
    if not src.is_contiguous():
        raise ValueError("resize_faces_u8: src must be contiguous")
    N, _, Hi, Wi = src.shape
    out_h, out_w = int(out_h), int(out_w)
    if out is None:
        out = torch.empty((N, 3, out_h, out_w), dtype=torch.uint8, device=src.device)
    elif (out.dtype != torch.uint8 or tuple(out.shape) != (N, 3, out_h, out_w) or out.device != src.device or
          not out.is_contiguous()):
        raise ValueError(f"resize_faces_u8: out must be contiguous uint8 {(N, 3, out_h, out_w)} on {src.device}")
    if N:
        check(lib.ls_resize_faces_u8(_p(src), N, Hi, Wi, out_h, out_w, _p(out), _stream()), "ls_resize_faces_u8")
    return out


_RESAMPLE_TAPS = {}  # (sr_in, sr_out, device index) -> (L, M, half, device taps)


def resample(x, sr_in, sr_out):
    """Mono fp32 samples at sr_in -> ceil(n * L / M) samples at sr_out as a device fp32
    tensor (ls_resample with audio.resample_taps' filter).  x: a 1-D tensor or array, on
    the host or the device.  Equal rates return x itself, with no launch."""
    if sr_in == sr_out:
        return x
    from .audio import resample_taps
    lib = _lib.load()
    x = torch.as_tensor(x)
    if x.dim() != 1 or x.numel() < 1:
        raise ValueError(f"resample: a non-empty 1-D signal expected, got shape {tuple(x.shape)}")
    device = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = x.to(device, torch.float32).contiguous()
    key = (int(sr_in), int(sr_out), device.index)
    if key not in _RESAMPLE_TAPS:
        L, M, half, taps = resample_taps(sr_in, sr_out)
        _RESAMPLE_TAPS[key] = (L, M, half, torch.tensor(taps, device=device))
    L, M, half, taps = _RESAMPLE_TAPS[key]
    n_in = x.numel()
    n_out = -(-n_in * L // M)
    y = torch.empty(n_out, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        check(lib.ls_resample(_p(x), n_in, _p(taps), L, M, half, _p(y), n_out, _stream()), "ls_resample")
    return y


def mjpeg_encode(frames_u8, quality=95, workspace=None):
    """Motion-JPEG scans of uint8 RGB frames (n, H, W, 3) on the device (ls_mjpeg_encode):
    -> (bytes uint8 (total,), offsets int64 (n + 1,)), both on the device; frame f's
    entropy-coded scan is bytes[offsets[f]:offsets[f + 1]] (headers: video.jpeg_headers).
    The output buffer starts at half the raw size and the call is repeated once with the
    exact size in the rare case the scans are larger (the kernels drop what does not fit
    and still report exact offsets).  ``workspace``: a caller's uint8 scratch tensor of at
    least ls_mjpeg_workspace_bytes.  There is no CPU path."""
    lib = _lib.load()
    if (not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or
            frames_u8.shape[-1] != 3 or not frames_u8.is_cuda):
        raise ValueError("mjpeg_encode: uint8 (n, H, W, 3) on the device expected, got "
                         f"{getattr(frames_u8, 'dtype', type(frames_u8))} {tuple(getattr(frames_u8, 'shape', ()))}")
    if not frames_u8.is_contiguous():
        raise ValueError("mjpeg_encode: frames must be contiguous")
    n, H, W, _ = frames_u8.shape
    device = frames_u8.device
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=device), offsets
    quality = int(quality)
    with torch.cuda.device(device):
        need = lib.ls_mjpeg_workspace_bytes(n, H, W)
        if workspace is None:
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != device:
            raise ValueError("mjpeg_encode: workspace must be a contiguous uint8 tensor on the frames' device")
        capacity = n * H * W * 3 // 2 + 4096
        for _ in range(2):
            out = torch.empty(capacity, dtype=torch.uint8, device=device)
            check(lib.ls_mjpeg_encode(_p(frames_u8), n, H, W, quality, _p(out), capacity, _p(offsets), _p(workspace),
                                      workspace.numel(), _stream()), "ls_mjpeg_encode")
            total = int(offsets[-1].item())
            if total <= capacity:
                return out[:total], offsets
            capacity = total
    raise RuntimeError("mjpeg_encode: the encoded size changed between two runs on the same frames")


def mjpeg_decode(data, frames, H, W, quant, huff, max_segments=1, workspace=None):
    """Motion-JPEG scans on the device -> (RGB uint8 (n, H, W, 3), status int32 (n,)), both
    on the device (ls_mjpeg_decode).  ``data``: uint8 1-D, the entropy-coded scans;
    ``frames``: int64 (n, 8) descriptors; ``quant``: uint16 / int16 (n_quant, 64);
    ``huff``: int32 (n_huff, 228) -- the layouts are in include/ls_hip.h,
    video.decode_frames builds them.  A non-zero status marks a frame that could not be
    decoded; the others are exact.  ``workspace``: a caller's uint8 scratch tensor of at
    least ls_mjpeg_decode_workspace_bytes.  There is no CPU path."""
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise RuntimeError("mjpeg_decode: the Motion-JPEG decoder runs on the HIP device, and none is present")
    for name, t, dt, tail in (("data", data, (torch.uint8,), None), ("frames", frames, (torch.int64,), 8),
                              ("quant", quant, (torch.uint16, torch.int16), 64), ("huff", huff, (torch.int32,), 228)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dt or not t.is_contiguous() or \
                t.dim() != (1 if tail is None else 2) or (tail is not None and (t.shape[1] != tail or t.shape[0] < 1)):
            raise ValueError(f"mjpeg_decode: {name} must be a contiguous device tensor of {dt[0]}"
                             + ("" if tail is None else f" (rows, {tail})") + ", got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    device = data.device
    if any(t.device != device for t in (frames, quant, huff)):
        raise ValueError("mjpeg_decode: data, frames, quant and huff must be on one device")
    n, H, W = frames.shape[0], int(H), int(W)
    with torch.cuda.device(device):
        need = lib.ls_mjpeg_decode_workspace_bytes(n, H, W)
        if workspace is None:
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != device:
            raise ValueError("mjpeg_decode: workspace must be a contiguous uint8 tensor on the data's device")
        ok = need > 0  # 0: a size ls_mjpeg_decode refuses; allocate nothing of that size
        out = torch.empty((n, H, W, 3) if ok else (0,), dtype=torch.uint8, device=device)
        status = torch.empty(n, dtype=torch.int32, device=device)
        check(lib.ls_mjpeg_decode(_p(data), data.numel(), _p(frames), n, H, W, _p(quant), quant.shape[0], _p(huff),
                                  huff.shape[0], int(max_segments), _p(out if ok else status), _p(status),
                                  _p(workspace), workspace.numel(), _stream()), "ls_mjpeg_decode")
    return out, status


def face_brighten(frames_u8, plan, verts, first_valid, roi, taps, dilate, c, brighten, max_value=235,
                  frames_per_batch=0, workspace=None):
    """The face brightness restore of use_darken requests (ls_face_brighten), in place on
    uint8 RGB frames (n, H, W, 3) on the device; returns the tensor.  ``plan`` int32 (n, 4),
    ``verts`` int32 (V, 2), ``first_valid``, ``roi`` = (x, y, w, h) and ``taps`` float32 are
    darken.build_tables' / darken.gaussian_taps' (arrays or tensors; the layouts are in
    include/ls_hip.h).  ``frames_per_batch``: frames whose masks are held at once (0: a fixed
    budget).  ``workspace``: a caller's uint8 scratch tensor of at least
    ls_face_brighten_workspace_bytes.  There is no CPU path."""
    lib = _lib.load()
    if (not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or
            frames_u8.shape[-1] != 3 or not frames_u8.is_cuda):
        raise ValueError("face_brighten: uint8 (n, H, W, 3) on the device expected, got "
                         f"{getattr(frames_u8, 'dtype', type(frames_u8))} {tuple(getattr(frames_u8, 'shape', ()))}")
    if not frames_u8.is_contiguous():
        raise ValueError("face_brighten: frames must be contiguous")
    n, H, W, _ = frames_u8.shape
    device = frames_u8.device
    plan = torch.as_tensor(plan).to(device).contiguous()
    verts = torch.as_tensor(verts).to(device).contiguous()
    taps = torch.as_tensor(taps).to(device).contiguous()
    if plan.dtype != torch.int32 or tuple(plan.shape) != (n, 4):
        raise ValueError(f"face_brighten: plan must be int32 {(n, 4)}, got {plan.dtype} {tuple(plan.shape)}")
    if verts.dtype != torch.int32 or verts.dim() != 2 or verts.shape[1] != 2 or verts.shape[0] < 1:
        raise ValueError(f"face_brighten: verts must be int32 (V, 2), got {verts.dtype} {tuple(verts.shape)}")
    if taps.dtype != torch.float32 or taps.dim() != 1:
        raise ValueError(f"face_brighten: taps must be float32 (n_taps,), got {taps.dtype} {tuple(taps.shape)}")
    if n == 0:
        return frames_u8
    rx, ry, rw, rh = (int(v) for v in roi)
    fpb = int(frames_per_batch)
    with torch.cuda.device(device):
        need = lib.ls_face_brighten_workspace_bytes(n, rh, rw, fpb)
        if workspace is None:
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != device:
            raise ValueError("face_brighten: workspace must be a contiguous uint8 tensor on the frames' device")
        check(lib.ls_face_brighten(_p(frames_u8), n, H, W, _p(plan), _p(verts), verts.shape[0], int(first_valid),
                                   rx, ry, rw, rh, _p(taps), taps.numel(), int(dilate), float(c), int(bool(brighten)),
                                   int(max_value), fpb, _p(workspace), workspace.numel(), _stream()),
              "ls_face_brighten")
    return frames_u8


def prep_pixels(faces_u8, mask, ld=8, pix=None, masked=None):
    lib = _lib.load()
    F_, _, R, _ = faces_u8.shape
    if pix is None:
        pix = torch.empty((F_, R, R, ld), dtype=torch.bfloat16, device=faces_u8.device)
    if masked is None:
        masked = torch.empty_like(pix)
    check(lib.ls_prep_pixels(_p(faces_u8), F_, R, _p(mask), _p(pix), _p(masked), ld, _stream()), "ls_prep_pixels")
    return pix, masked


def vae_sample(moments, eps, scaling, shift, dst, c_off):
    lib = _lib.load()
    P = eps.shape[0]
    check(lib.ls_vae_sample(_p(moments), moments.shape[-1], _p(eps), P, float(scaling), float(shift), _p(dst),
                            dst.shape[-1], c_off, _stream()), "ls_vae_sample")


def pack_unet_input(lat, cond, mask, F_, R, h, Bu, unet_in):
    lib = _lib.load()
    check(lib.ls_pack_unet_input(_p(lat), _p(cond), _p(mask), F_, R, h, Bu, _p(unet_in), unet_in.shape[-1],
                                 _stream()), "ls_pack_unet_input")


def scale_latents(lat, inv_scaling, shift, z):
    lib = _lib.load()
    check(lib.ls_scale_latents(_p(lat), lat.shape[0], float(inv_scaling), float(shift), _p(z), z.shape[-1],
                               _stream()), "ls_scale_latents")


def paste_back(dec, pix, mask, out_nchw=None, out_u8=None):
    lib = _lib.load()
    F_, R = dec.shape[0], dec.shape[1]
    check(lib.ls_paste_back(_p(dec), dec.shape[-1], _p(pix), pix.shape[-1], _p(mask), F_, R, _p(out_nchw),
                            _p(out_u8), _stream()), "ls_paste_back")


def conv3x3_strided(x, pw: Packed, stride, pad, out_hw, out=None):
    """3x3 conv with per-axis strides and one-sided zero padding (ls_conv3x3_strided):
    x (n, H, W, Cin) bf16 NHWC -> (n, Ho, Wo, N) bf16; stride = (sh, sw) in 1..3, pad =
    (top, left) in 0..1, out_hw = (Ho, Wo) -- taps past the bottom / right edge read zero.
    pw is the ordinary packed 3x3 operand.  ``out`` may be a pitched NHWC view."""
    lib = _lib.load()
    n, H, W, Cin = x.shape
    assert pw.ksize == 3 and pw.cin == Cin, (pw.ksize, pw.cin, Cin)
    Ho, Wo = out_hw
    if out is None:
        out = torch.empty((n, Ho, Wo, pw.N), dtype=torch.bfloat16, device=x.device)
    assert tuple(out.shape) == (n, Ho, Wo, pw.N) and out.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
    check(lib.ls_conv3x3_strided(_p(x), _ld(x), n, H, W, Cin, _p(pw.w), pw.K, pw.N, _p(pw.bias), stride[0], stride[1],
                                 pad[0], pad[1], Ho, Wo, _p(out), _ld(out), _stream()), "ls_conv3x3_strided")
    return out


def syncnet_mel(wav, filters, out=None):
    """SyncNet mel front end (ls_syncnet_mel): wav fp32 (n,) at 16 kHz, filters fp32 (80, 401),
    both on the device -> fp32 (T, 80) frame-major, T = 1 + n // 200."""
    lib = _lib.load()
    if wav.dim() != 1 or wav.dtype != torch.float32 or not wav.is_cuda or not wav.is_contiguous() or wav.numel() < 1:
        raise ValueError(f"syncnet_mel: a non-empty contiguous fp32 1-D device tensor expected, got {wav.dtype} "
                         f"{tuple(wav.shape)} on {wav.device}")
    assert tuple(filters.shape) == (80, 401) and filters.dtype == torch.float32 and filters.is_contiguous()
    T = 1 + wav.numel() // 200
    if out is None:
        out = torch.empty((T, 80), dtype=torch.float32, device=wav.device)
    assert tuple(out.shape) == (T, 80) and out.is_contiguous() and out.dtype == torch.float32
    check(lib.ls_syncnet_mel(_p(wav), wav.numel(), _p(filters), _p(out), _stream()), "ls_syncnet_mel")
    return out


def syncnet_pack_frames(faces_u8, starts, num_frames, out=None):
    """uint8 faces (n, R, R, 3) on the device + frame starts (host ints) -> the visual
    encoder's input (B, R/2, R, 3 num_frames) bf16: lower half, channel 3 f + c, (x / 255 -
    0.5) / 0.5 (ls_syncnet_pack_frames).  A window outside the frames raises here."""
    lib = _lib.load()
    if faces_u8.dtype != torch.uint8 or faces_u8.dim() != 4 or faces_u8.shape[3] != 3 or \
            faces_u8.shape[1] != faces_u8.shape[2] or not faces_u8.is_cuda or not faces_u8.is_contiguous():
        raise ValueError(f"syncnet_pack_frames: contiguous uint8 (n, R, R, 3) on the device expected, got "
                         f"{faces_u8.dtype} {tuple(faces_u8.shape)} on {faces_u8.device}")
    n, R = faces_u8.shape[0], faces_u8.shape[1]
    starts = [int(s) for s in starts]
    F_ = int(num_frames)
    if not starts or min(starts) < 0 or max(starts) + F_ > n:
        raise ValueError(f"syncnet_pack_frames: windows {starts} of {F_} frames do not lie in {n} frames")
    if R % 2 or F_ < 1 or (3 * F_) % 8:
        raise ValueError(f"syncnet_pack_frames: R = {R} must be even and 3 * num_frames = {3 * F_} a multiple of 8")
    B = len(starts)
    st = torch.tensor(starts, dtype=torch.int32, device=faces_u8.device)
    if out is None:
        out = torch.empty((B, R // 2, R, 3 * F_), dtype=torch.bfloat16, device=faces_u8.device)
    assert tuple(out.shape) == (B, R // 2, R, 3 * F_) and out.is_contiguous() and out.dtype == torch.bfloat16
    check(lib.ls_syncnet_pack_frames(_p(faces_u8), n, R, _p(st), B, F_, _p(out), _stream()), "ls_syncnet_pack_frames")
    return out


def syncnet_pack_mel(mel, cols, mel_len=52, out=None):
    """mel fp32 (T, 80) on the device + window columns (host ints) -> the audio encoder's
    input (B, 80, mel_len, 8) bf16, channel 0 = mel[cols[b] + j][m], channels 1..7 zero
    (ls_syncnet_pack_mel).  A window past the end of the mel raises here."""
    lib = _lib.load()
    if mel.dtype != torch.float32 or mel.dim() != 2 or mel.shape[1] != 80 or not mel.is_cuda or not mel.is_contiguous():
        raise ValueError(f"syncnet_pack_mel: contiguous fp32 (T, 80) on the device expected, got {mel.dtype} "
                         f"{tuple(mel.shape)} on {mel.device}")
    T, L = mel.shape[0], int(mel_len)
    cols = [int(c) for c in cols]
    if not cols or L < 1 or min(cols) < 0 or max(cols) + L > T:
        raise ValueError(f"syncnet_pack_mel: windows {cols} of {L} columns do not lie in {T} mel frames")
    B = len(cols)
    ct = torch.tensor(cols, dtype=torch.int32, device=mel.device)
    if out is None:
        out = torch.empty((B, 80, L, 8), dtype=torch.bfloat16, device=mel.device)
    assert tuple(out.shape) == (B, 80, L, 8) and out.is_contiguous() and out.dtype == torch.bfloat16
    check(lib.ls_syncnet_pack_mel(_p(mel), T, _p(ct), B, L, _p(out), _stream()), "ls_syncnet_pack_mel")
    return out


def sync_score(v_in, a_in, v=None, a=None, score=None):
    """ReLU + F.normalize of both embeddings and their cosine (ls_sync_score): v_in, a_in
    bf16 (B, D) rows (row-strided views allowed) -> (v, a fp32 (B, D), score fp32 (B,))."""
    lib = _lib.load()
    B, D = v_in.shape
    assert tuple(a_in.shape) == (B, D) and v_in.dtype == a_in.dtype == torch.bfloat16
    assert v_in.stride(1) == 1 and a_in.stride(1) == 1
    if v is None:
        v = torch.empty((B, D), dtype=torch.float32, device=v_in.device)
    if a is None:
        a = torch.empty((B, D), dtype=torch.float32, device=v_in.device)
    if score is None:
        score = torch.empty((B,), dtype=torch.float32, device=v_in.device)
    assert v.stride(1) == 1 and a.stride(1) == 1 and v.stride(0) == a.stride(0) and score.is_contiguous()
    check(lib.ls_sync_score(_p(v_in), v_in.stride(0) if B > 1 else D, _p(a_in), a_in.stride(0) if B > 1 else D, B, D,
                            _p(v), _p(a), v.stride(0) if B > 1 else D, _p(score), _stream()), "ls_sync_score")
    return v, a, score


def add_rows(x2d, table, out=None):
    lib = _lib.load()
    rows, C_ = x2d.shape
    if out is None:
        out = torch.empty_like(x2d)
    check(lib.ls_add_rows(_p(x2d), rows, C_, x2d.stride(0), _p(table), table.shape[0], _p(out), out.stride(0),
                          _stream()), "ls_add_rows")
    return out


# ---- GIF thumbnail (thumbnail.py; csrc/ls_thumb.hip) ----------------------------------


def _rgb_frames(frames_u8, what):
    if (not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or
            frames_u8.shape[-1] != 3 or not frames_u8.is_cuda):
        raise ValueError(f"{what}: uint8 (n, H, W, 3) on the device expected, got "
                         f"{getattr(frames_u8, 'dtype', type(frames_u8))} {tuple(getattr(frames_u8, 'shape', ()))}")
    if not frames_u8.is_contiguous():
        raise ValueError(f"{what}: frames must be contiguous")
    return frames_u8.shape[:3]


def resize_area_u8(frames_u8, out_h, out_w):
    """cv2.resize(frame, (out_w, out_h), interpolation=INTER_AREA) of uint8 RGB frames
    (n, H, W, 3) on the device -> (n, out_h, out_w, 3) (ls_resize_area_u8; downscale only)."""
    lib = _lib.load()
    n, H, W = _rgb_frames(frames_u8, "resize_area_u8")
    out_h, out_w = int(out_h), int(out_w)
    out = torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device=frames_u8.device)
    if n:
        with torch.cuda.device(frames_u8.device):
            check(lib.ls_resize_area_u8(_p(frames_u8), n, H, W, _p(out), out_h, out_w, _stream()), "ls_resize_area_u8")
    return out


def overlay_blend_u8(frames_u8, layers):
    """Blends ``layers`` -- a sequence of (x0, y0, alpha uint8 (h, w) array, (r, g, b)), at
    most 16, applied in order -- into uint8 RGB frames (n, H, W, 3) on the device, in place
    (ls_overlay_blend_u8: Pillow's blend per channel).  Returns the frames."""
    import numpy as np
    lib = _lib.load()
    n, H, W = _rgb_frames(frames_u8, "overlay_blend_u8")
    layers = list(layers)
    desc, maps, off = [], [], 0
    for x0, y0, a, ink in layers:
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError(f"overlay_blend_u8: an alpha map must be 2-D, got shape {a.shape}")
        desc.append([int(x0), int(y0), a.shape[1], a.shape[0], off, int(ink[0]), int(ink[1]), int(ink[2])])
        maps.append(a.reshape(-1))
        off += a.size
    if n == 0:
        return frames_u8
    alpha = None
    if off:
        alpha = torch.from_numpy(np.concatenate(maps)).to(frames_u8.device)
    d = (C.c_int32 * (8 * len(desc)))(*[v for row in desc for v in row]) if desc else None
    with torch.cuda.device(frames_u8.device):
        check(lib.ls_overlay_blend_u8(_p(frames_u8), n, H, W, d, len(desc), _p(alpha), off, _stream()),
              "ls_overlay_blend_u8")
    return frames_u8


def rgb555_hist(frames_u8):
    """uint8 RGB frames (n, H, W, 3) on the device -> int64 (32768,) on the device: the pixel
    count of every 5-5-5 bin r >> 3 << 10 | g >> 3 << 5 | b >> 3 (ls_rgb555_hist; the kernel
    counts in uint32)."""
    lib = _lib.load()
    n, H, W = _rgb_frames(frames_u8, "rgb555_hist")
    hist = torch.zeros(32768, dtype=torch.int32, device=frames_u8.device)
    if n:
        with torch.cuda.device(frames_u8.device):
            check(lib.ls_rgb555_hist(_p(frames_u8), n, H, W, _p(hist), _stream()), "ls_rgb555_hist")
    return hist.to(torch.int64) & 0xffffffff


def palette_map(frames_u8, lut):
    """uint8 RGB frames (n, H, W, 3) -> uint8 (n, H, W): lut[5-5-5 bin] per pixel, with lut a
    uint8 (32768,) tensor on the frames' device (ls_palette_map)."""
    lib = _lib.load()
    n, H, W = _rgb_frames(frames_u8, "palette_map")
    if (not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (32768,) or
            lut.device != frames_u8.device or not lut.is_contiguous()):
        raise ValueError("palette_map: lut must be a contiguous uint8 (32768,) tensor on the frames' device")
    idx = torch.empty((n, H, W), dtype=torch.uint8, device=frames_u8.device)
    if n:
        with torch.cuda.device(frames_u8.device):
            check(lib.ls_palette_map(_p(frames_u8), n, H, W, _p(lut), _p(idx), _stream()), "ls_palette_map")
    return idx


def gif_lzw(idx_u8, workspace=None, capacity=None):
    """GIF LZW code bytes (minimum code size 8) of uint8 index frames (n, H, W) on the device
    (ls_gif_lzw) -> (bytes uint8 (total,), offsets int64 (n + 1,)), both on the device; frame
    f's codes are bytes[offsets[f]:offsets[f + 1]], not yet split into sub-blocks.  The output
    buffer starts at ``capacity`` bytes (default: the raw size) and the call is repeated once
    with the exact size when the codes are larger.  There is no CPU path."""
    lib = _lib.load()
    if (not isinstance(idx_u8, torch.Tensor) or idx_u8.dtype != torch.uint8 or idx_u8.dim() != 3 or
            not idx_u8.is_cuda or not idx_u8.is_contiguous()):
        raise ValueError("gif_lzw: contiguous uint8 (n, H, W) on the device expected, got "
                         f"{getattr(idx_u8, 'dtype', type(idx_u8))} {tuple(getattr(idx_u8, 'shape', ()))}")
    n, H, W = idx_u8.shape
    device = idx_u8.device
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=device), offsets
    with torch.cuda.device(device):
        need = lib.ls_gif_lzw_workspace_bytes(n, H, W)
        if workspace is None:
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != device:
            raise ValueError("gif_lzw: workspace must be a contiguous uint8 tensor on the frames' device")
        capacity = n * H * W + 64 if capacity is None else int(capacity)
        for _ in range(2):
            out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=device)
            check(lib.ls_gif_lzw(_p(idx_u8), n, H, W, _p(out), capacity, _p(offsets), _p(workspace),
                                 workspace.numel(), _stream()), "ls_gif_lzw")
            total = int(offsets[-1].item())
            if total <= capacity:
                return out[:total], offsets
            capacity = total
    raise RuntimeError("gif_lzw: the coded size changed between two runs on the same frames")


# ---- classic SyncNet evaluation (synceval.py; csrc/ls_synceval.hip) ---------------------


class PackedGeneral:
    """An operand of ls_conv_general: w bf16 (N, K) (packing.pack_weight_general), bias fp32
    (N,) or None, the window (kt, kh, kw) and the padded input channel count."""

    def __init__(self, w, bias, cin, window):
        self.w, self.bias, self.cin, self.window = w, bias, cin, tuple(window)
        self.N, self.K = w.shape


def mfcc(audio_i16scale, filters, out=None):
    """python_speech_features.mfcc's defaults (ls_mfcc): fp32 (n,) mono 16 kHz samples on the
    int16 scale, filters fp32 (26, 257), both on the device -> fp32 (13, T)."""
    lib = _lib.load()
    a = audio_i16scale
    if a.dim() != 1 or a.dtype != torch.float32 or not a.is_cuda or not a.is_contiguous() or a.numel() < 1:
        raise ValueError(f"mfcc: a non-empty contiguous fp32 1-D device tensor expected, got {a.dtype} "
                         f"{tuple(a.shape)} on {a.device}")
    assert tuple(filters.shape) == (26, 257) and filters.dtype == torch.float32 and filters.is_contiguous()
    n = a.numel()
    T = 1 + -(-(n - 400) // 160) if n > 400 else 1
    if out is None:
        out = torch.empty((13, T), dtype=torch.float32, device=a.device)
    assert tuple(out.shape) == (13, T) and out.is_contiguous() and out.dtype == torch.float32
    check(lib.ls_mfcc(_p(a), n, _p(filters), _p(out), _stream()), "ls_mfcc")
    return out


def conv_out_hw(H, W, window, stride, pad):
    return (H + 2 * pad[0] - window[-2]) // stride[0] + 1, (W + 2 * pad[1] - window[-1]) // stride[1] + 1


def conv_general(x, pw: PackedGeneral, stride=(1, 1), pad=(0, 0), relu=False, out=None, out_f32=False):
    """ls_conv_general: x (T, H, W, Cin) bf16 NHWC -> (T - kt + 1, Ho, Wo, N) bf16 (fp32 with
    out_f32), the window of ``pw`` over (time, y, x), ReLU on request.  ``out`` may be a
    pitched NHWC view."""
    lib = _lib.load()
    T, H, W, Cin = x.shape
    kt, kh, kw = pw.window
    assert pw.cin == Cin and x.dtype == torch.bfloat16, (pw.cin, Cin, x.dtype)
    Ho, Wo = conv_out_hw(H, W, pw.window, stride, pad)
    dt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty((T - kt + 1, Ho, Wo, pw.N), dtype=dt, device=x.device)
    assert tuple(out.shape) == (T - kt + 1, Ho, Wo, pw.N) and out.dtype == dt, (tuple(out.shape), out.dtype)
    check(lib.ls_conv_general(_p(x), _ld(x), T, H, W, Cin, _p(pw.w), pw.K, pw.N, _p(pw.bias), kt, kh, kw, stride[0],
                              stride[1], pad[0], pad[1], int(bool(relu)), _p(out), _ld(out), int(out_f32), _stream()),
          "ls_conv_general")
    return out


def maxpool2d(x, window, stride, pad=(0, 0), out=None):
    """ls_maxpool2d: x (n, H, W, C) bf16 NHWC -> (n, Ho, Wo, C); the padding is -inf."""
    lib = _lib.load()
    n, H, W, C_ = x.shape
    Ho, Wo = conv_out_hw(H, W, window, stride, pad)
    if out is None:
        out = torch.empty((n, Ho, Wo, C_), dtype=torch.bfloat16, device=x.device)
    assert tuple(out.shape) == (n, Ho, Wo, C_) and out.dtype == x.dtype == torch.bfloat16
    check(lib.ls_maxpool2d(_p(x), _ld(x), n, H, W, C_, window[0], window[1], stride[0], stride[1], pad[0], pad[1],
                           _p(out), _ld(out), _stream()), "ls_maxpool2d")
    return out


def sync_offset(im_feat, cc_feat, vshift, dists=None, mean_dists=None):
    """calc_pdist and its mean (ls_sync_offset): im_feat, cc_feat fp32 (n, D) contiguous ->
    (dists fp32 (n, 2 vshift + 1), mean_dists fp32 (2 vshift + 1,))."""
    lib = _lib.load()
    n, D = im_feat.shape
    assert tuple(cc_feat.shape) == (n, D) and im_feat.dtype == cc_feat.dtype == torch.float32
    assert im_feat.is_contiguous() and cc_feat.is_contiguous()
    win = 2 * int(vshift) + 1
    if dists is None:
        dists = torch.empty((n, win), dtype=torch.float32, device=im_feat.device)
    if mean_dists is None:
        mean_dists = torch.empty((win,), dtype=torch.float32, device=im_feat.device)
    assert tuple(dists.shape) == (n, win) and dists.is_contiguous() and mean_dists.is_contiguous()
    check(lib.ls_sync_offset(_p(im_feat), _p(cc_feat), n, D, int(vshift), _p(dists), _p(mean_dists), _stream()),
          "ls_sync_offset")
    return dists, mean_dists


def crop_track(frames_u8, plan, out=None):
    """ls_crop_track: frames uint8 (n, H, W, 3) and plan int32 (n, 5) = (y0, y1, x0, x1, bsi),
    both on the device -> uint8 (n, 224, 224, 3)."""
    lib = _lib.load()
    n, H, W = _rgb_frames(frames_u8, "crop_track")
    assert tuple(plan.shape) == (n, 5) and plan.dtype == torch.int32 and plan.is_cuda and plan.is_contiguous()
    if out is None:
        out = torch.empty((n, 224, 224, 3), dtype=torch.uint8, device=frames_u8.device)
    assert tuple(out.shape) == (n, 224, 224, 3) and out.dtype == torch.uint8 and out.is_contiguous()
    check(lib.ls_crop_track(_p(frames_u8), n, H, W, _p(plan), _p(out), _stream()), "ls_crop_track")
    return out


# ---- S3FD face detector (s3fd.py; csrc/ls_s3fd.hip) --------------------------------------


def s3fd_prep_size(H, W, scale):
    """cvRound(H s), cvRound(W s): round half to even, as Python's round() does on a float."""
    return int(round(H * float(scale))), int(round(W * float(scale)))


def s3fd_prep(frames_u8, scale, out=None):
    """ls_s3fd_prep: frames uint8 (n, H, W, 3) RGB on the device -> bf16 (n, h, w, 8): resized by
    ``scale`` as cv2.resize(., (0, 0), fx=s, fy=s) does, minus the means; channels R, G, B, 0.."""
    lib = _lib.load()
    n, H, W = _rgb_frames(frames_u8, "s3fd_prep")
    s = float(scale)
    if not 0.0 < s <= 1.0:
        raise ValueError(f"s3fd_prep: the scale must be in (0, 1], got {scale}")
    if s == 0.5:
        raise ValueError("s3fd_prep: scale 0.5 is refused: cv2.resize switches to its 2 x 2 area path there, which "
                         "ls_s3fd_prep does not restate")
    h, w = s3fd_prep_size(H, W, s)
    if h < 1 or w < 1:
        raise ValueError(f"s3fd_prep: a {H} x {W} frame at scale {s} is empty")
    if out is None:
        out = torch.empty((n, h, w, 8), dtype=torch.bfloat16, device=frames_u8.device)
    assert tuple(out.shape) == (n, h, w, 8) and out.dtype == torch.bfloat16 and out.is_contiguous()
    check(lib.ls_s3fd_prep(_p(frames_u8), n, H, W, s, _p(out), _stream()), "ls_s3fd_prep")
    return out


def conv3x3_relu(x, pw: PackedGeneral, dilation=1, out=None):
    """ls_conv3x3_relu: x (n, H, W, Cin) bf16 NHWC -> (n, H, W, N) bf16: 3 x 3, stride 1, padding =
    dilation, bias, ReLU.  ``pw`` is the operand ls_conv_general takes for the same weight."""
    lib = _lib.load()
    n, H, W, Cin = x.shape
    assert pw.window == (1, 3, 3) and pw.cin == Cin and pw.K == 9 * Cin and x.dtype == torch.bfloat16, \
        (pw.window, pw.cin, Cin, pw.K, x.dtype)
    if out is None:
        out = torch.empty((n, H, W, pw.N), dtype=torch.bfloat16, device=x.device)
    assert tuple(out.shape) == (n, H, W, pw.N) and out.dtype == torch.bfloat16
    check(lib.ls_conv3x3_relu(_p(x), _ld(x), n, H, W, Cin, _p(pw.w), pw.N, _p(pw.bias), int(dilation), _p(out),
                              _ld(out), _stream()), "ls_conv3x3_relu")
    return out


def maxpool2x2_ceil(x, out=None):
    """ls_maxpool2x2_ceil: MaxPool2d(2, 2, ceil_mode=True) on bf16 NHWC."""
    lib = _lib.load()
    n, H, W, C_ = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if out is None:
        out = torch.empty((n, Ho, Wo, C_), dtype=torch.bfloat16, device=x.device)
    assert tuple(out.shape) == (n, Ho, Wo, C_) and out.dtype == x.dtype == torch.bfloat16
    check(lib.ls_maxpool2x2_ceil(_p(x), _ld(x), n, H, W, C_, _p(out), _ld(out), _stream()), "ls_maxpool2x2_ceil")
    return out


def l2norm_scale(x, weight, out=None):
    """ls_l2norm_scale: x (n, H, W, C) bf16 NHWC, weight fp32 (C,) -> L2Norm.forward, bf16."""
    lib = _lib.load()
    n, H, W, C_ = x.shape
    assert x.dtype == torch.bfloat16 and weight.dtype == torch.float32 and tuple(weight.shape) == (C_,)
    assert weight.is_contiguous()
    if out is None:
        out = torch.empty((n, H, W, C_), dtype=torch.bfloat16, device=x.device)
    assert tuple(out.shape) == tuple(x.shape) and out.dtype == torch.bfloat16
    check(lib.ls_l2norm_scale(_p(x), _ld(x), n * H * W, C_, _p(weight), _p(out), _ld(out), _stream()),
          "ls_l2norm_scale")
    return out


S3FD_TOP_K = 750
S3FD_MAX_PRIORS = 65536


def s3fd_detect(maps, priors, want_idx=False):
    """ls_s3fd_detect: the six head maps fp32 (n, h_l, w_l, 8 | 6) contiguous (loc | conf) and the
    priors fp32 (P, 4), all on the device -> (out fp32 (n, 750, 5) = score, x1, y1, x2, y2,
    counts int32 (n,)[, keep_idx int32 (n, 750)])."""
    lib = _lib.load()
    assert len(maps) == 6
    n = maps[0].shape[0]
    hw = []
    for l, m in enumerate(maps):
        assert m.dim() == 4 and m.shape[0] == n and m.shape[3] == (8 if l == 0 else 6), (l, tuple(m.shape))
        assert m.dtype == torch.float32 and m.is_contiguous() and m.is_cuda
        hw += [m.shape[1], m.shape[2]]
    P = sum(hw[2 * l] * hw[2 * l + 1] for l in range(6))
    if P > S3FD_MAX_PRIORS:
        raise ValueError(f"s3fd_detect: {P} priors per frame exceed the kernel's {S3FD_MAX_PRIORS}: detect at a "
                         "smaller scale")
    assert tuple(priors.shape) == (P, 4) and priors.dtype == torch.float32 and priors.is_contiguous(), \
        (tuple(priors.shape), P)
    dev = maps[0].device
    out = torch.empty((n, S3FD_TOP_K, 5), dtype=torch.float32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    idx = torch.empty((n, S3FD_TOP_K), dtype=torch.int32, device=dev) if want_idx else None
    nbytes = lib.ls_s3fd_detect_workspace_bytes(n, P)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * 6)(*[m.data_ptr() for m in maps])
    sizes = (C.c_int32 * 12)(*hw)
    check(lib.ls_s3fd_detect(ptrs, sizes, n, _p(priors), P, _p(out), _p(counts), _p(idx), _p(ws), nbytes, _stream()),
          "ls_s3fd_detect")
    return (out, counts, idx) if want_idx else (out, counts)


def nms_boxes(det, conf_th, frame_w, frame_h, thresh=0.1, want_idx=False):
    """ls_nms_boxes: det fp32 (n, R, 5) = score, x1, y1, x2, y2 -> (out fp32 (n, R, 5) = x1, y1, x2,
    y2, score in frame coordinates and nms_'s keep order, counts int32 (n,)[, keep_idx])."""
    lib = _lib.load()
    assert det.dim() == 3 and det.shape[2] == 5 and det.dtype == torch.float32 and det.is_contiguous() and det.is_cuda
    n, R = det.shape[:2]
    out = torch.empty((n, R, 5), dtype=torch.float32, device=det.device)
    counts = torch.empty((n,), dtype=torch.int32, device=det.device)
    idx = torch.empty((n, R), dtype=torch.int32, device=det.device) if want_idx else None
    check(lib.ls_nms_boxes(_p(det), n, R, float(conf_th), float(frame_w), float(frame_h), float(thresh), _p(out),
                           _p(counts), _p(idx), _stream()), "ls_nms_boxes")
    return (out, counts, idx) if want_idx else (out, counts)
