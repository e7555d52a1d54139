"""ls_conv2d per element at tile edges (tests/parity.py): the smallest shapes that still
cross every tile boundary, on every compiled tile, the register-staged kernel, split-K, the
row-block and halo kernels, the scalar (N % 8 != 0) epilogue and every epilogue operand --
each output inside a sentinel guard band (pitch above N, extra rows), inputs checked
unchanged, acceptance |got - ref| <= gemm_bound per element against fp64 on the same
bf16-rounded inputs.  Every test prints its worst err/bound ratio.  (The LayerNorm fold, row
statistics out, GroupNorm column sums out and the row-block kernel's other instances and steady
state: tests/test_gpu_edges_conv_fused.py.)"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import parity as P
from latentsync_amd import _lib, ops
from latentsync_amd.packing import geglu_interleave, pack_weight

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
FRAG = dict(rows=16, cols=16)  # the MFMA fragment: what the failure report names tiles by


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev_bf(t):
    return t.to(BF).to(DEV).contiguous()


def packed(w, b, ksize, geglu=False):
    n_out = w.shape[0]
    if geglu:
        w, b = geglu_interleave(w, b)
    wp = pack_weight(w)
    cin = (w.shape[1] + 7) // 8 * 8
    return ops.Packed(wp.to(BF).to(DEV), None if b is None else b.float().to(DEV), cin, ksize, n_out, geglu)


def wide(t, ld):
    """t (..., C) as a view of a (..., ld) device buffer: a pitch above the channel count."""
    buf = torch.full(t.shape[:-1] + (ld,), 7.0, dtype=BF, device=DEV)
    buf[..., :t.shape[-1]] = t.to(BF).to(DEV)
    return buf[..., :t.shape[-1]]


class tuning:
    """ls_set_tuning keys for the duration of a block, restored in the finally of __exit__."""
    DEFAULTS = {1: 0, 2: 0, 3: 0, 6: 1, 8: 1, 15: 1, 16: 1, 18: 1, 19: 1}

    def __init__(self, **keys):
        self.keys = {int(k[1:]): v for k, v in keys.items()}
        self.lib = _lib.load()

    def __enter__(self):
        try:
            for k, v in self.keys.items():
                assert self.lib.ls_set_tuning(k, v) == 0, \
                    f"ls_set_tuning({k}, {v}) refused: {self.lib.ls_last_error().decode()}"
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k in self.keys:
            self.lib.ls_set_tuning(k, self.DEFAULTS[k])
        return False


def conv_reference(x1, x2, w, b, ksize, *, stride=1, pad=None, upsample=False, vae_down=False, aff=None,
                   rowvec=None, res=None, out_scale=1.0):
    """fp64 (ref, mag, prod_mag), each (n, Ho, Wo, N): ref = out_scale (sum a w + bias + rowvec +
    res), mag the same with absolute values, prod_mag = out_scale sum |a'| |w| for the prologue
    term, where |a'| = |a| + 1.1 2^-12 (|x scale| + |shift|): the kernel's a is the bf16 rounding
    (2^-8, gemm_bound's factor) of an fp32 evaluation of silu(x scale + shift) -- the product,
    the add and silu's 6 operations, 8 2^-23 relative to |x scale| + |shift|, through silu's
    slope <= 1.1 -- and 8 2^-23 1.1 = 2^-8 (1.1 2^-12)."""
    x = P.f64(x1 if x2 is None else torch.cat([x1, x2], -1)).permute(0, 3, 1, 2)
    w64 = P.f64(w)
    if w64.dim() == 2:
        w64 = w64[:, :, None, None]
    a, a_abs = x, x.abs()
    if aff is not None:
        sc, sh, ips, silu = aff
        sc = P.f64(sc).repeat_interleave(ips, 0)[:, :, None, None]
        sh = P.f64(sh).repeat_interleave(ips, 0)[:, :, None, None]
        a = x * sc + sh
        pre = (x * sc).abs() + sh.abs()
        if silu:
            a = a * torch.sigmoid(a)
        a_abs = a.abs() + 1.1 * 2.0 ** -12 * pre
    if upsample:
        a, a_abs = (F.interpolate(t, scale_factor=2.0, mode="nearest") for t in (a, a_abs))
    if vae_down:  # the SD-VAE downsampler: F.pad(0, 1, 0, 1), stride 2, no padding
        a, a_abs = (F.pad(t, (0, 1, 0, 1)) for t in (a, a_abs))
        stride, pad = 2, 0
    if pad is None:
        pad = 1 if ksize == 3 else 0
    acc = F.conv2d(a, w64, None, stride=stride, padding=pad).permute(0, 2, 3, 1)
    prod = F.conv2d(a_abs, w64.abs(), None, stride=stride, padding=pad).permute(0, 2, 3, 1)
    mag = prod.clone()
    M, N = acc.numel() // acc.shape[-1], acc.shape[-1]
    if b is not None:
        acc, mag = acc + P.f64(b), mag + P.f64(b).abs()
    if rowvec is not None:
        t, rpv, mod = rowvec
        r = torch.arange(M) // rpv
        rows = P.f64(t)[(r % mod) if mod else r][:, :N].reshape(acc.shape)
        acc, mag = acc + rows, mag + rows.abs()
    if res is not None:
        acc, mag = acc + P.f64(res), mag + P.f64(res).abs()
    return acc * out_scale, mag * abs(out_scale), prod * abs(out_scale)


def finish(name, g, ref, bound, inputs):
    torch.cuda.synchronize()
    worst = P.assert_elementwise(g.view.reshape(ref.shape), ref, bound, where=FRAG, name=name)
    P.assert_guard_intact(g, name)
    for i, (t, snap) in enumerate(inputs):
        P.assert_unchanged(t, snap, f"{name} input {i}")
    return worst


def snaps(*ts):
    return [(t, P.snapshot(t)) for t in ts if t is not None]


# ---------------------------------------------------------------- ksize 1: every tile, M edge, split
@functools.lru_cache(maxsize=None)
def linear_case(M, Cin, N):
    x = P.bf16_round(rnd(M, Cin, seed=M + Cin))
    w = P.bf16_round(rnd(N, Cin, seed=N + Cin + 1, scale=1 / math.sqrt(Cin)))
    b = rnd(N, seed=N + 2, scale=0.1)
    res = P.bf16_round(rnd(M, N, seed=M + N + 3))
    ref, mag, _ = conv_reference(x[None, None], None, w, b, 1, res=res[None, None])
    return x, w, b, res, ref.reshape(M, N), P.gemm_bound(ref, mag, Cin, BF).reshape(M, N)


CONFIGS = [(f"tile{t}", dict(k2=t)) for t in (1, 2, 3, 4, 5, 6, 9)] + [("regstage", dict(k1=1)),
           ("split2", dict(k2=1, k3=2)), ("split3", dict(k2=1, k3=3))]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
@pytest.mark.parametrize("Cin,K,N", P.EDGE_KN)
def test_linear_tiles(gpu, Cin, K, N, cfg):
    """M in {1, 127, 129, 257, 300} on every compiled forced tile (128x128, 128x64, 64x64,
    128x32, 256x256, 256x128, 128x160), the register-staged kernel and split-K 2 / 3, with
    bias and a residual of pitch N + 8.  K = 64 has one K-tile (split-K degenerates to 1)."""
    worst = 0.0
    with tuning(**cfg[1]):
        for M in P.EDGE_M:
            x, w, b, res, ref, bound = linear_case(M, Cin, N)
            pw = packed(w, b, 1)
            assert pw.K == K
            xd, rd = dev_bf(x), wide(res, N + 8)
            g = P.guarded((M, N), pitch=N + 16, pad_rows=3, dtype=BF, device=DEV)
            inputs = snaps(xd, pw.w, pw.bias, rd)
            assert ops.conv_path(xd[None, None], pw, res=rd[None, None], out=g.view[None, None]) == (2 if "k1" in cfg[1] else 0)
            ops.linear(xd, pw, res=rd, out=g.view)
            worst = max(worst, finish(f"linear {cfg[0]} {M}x{K}x{N}", g, ref, bound, inputs))
    print(f"linear {cfg[0]} K {K} N {N}: worst err/bound {worst:.3f}")


# ---------------------------------------------------------------- row-block kernel
@pytest.mark.parametrize("K,M,fm2,res,path", [
    (320, 256, 1, False, 1), (320, 512, 1, True, 1), (320, 384, 1, False, 0), (320, 130, 1, False, 0),
    (640, 256, 1, False, 1), (640, 128, 0, False, 1), (640, 384, 0, False, 1), (640, 128, 1, False, 0),
    (640, 384, 1, False, 0), (640, 130, 0, False, 0), (640, 384, 0, True, 0)])
def test_rowblock(gpu, K, M, fm2, res, path):
    """gemm_rowblock_kernel at its smallest grids: K = 320 takes M % 256 == 0; K = 640 takes
    M % 256 == 0 with two fragments per wave (tuning key 15, the default) and M % 128 == 0 with
    one, and no residual.  The other M (and K = 640 with a residual) fall to the tiled kernels:
    the same call must stay right there (path 0)."""
    N = 192
    x = P.bf16_round(rnd(M, K, seed=K + M))
    w = P.bf16_round(rnd(N, K, seed=K + 1, scale=1 / math.sqrt(K)))
    b = rnd(N, seed=5, scale=0.1)
    r = P.bf16_round(rnd(M, N, seed=6)) if res else None
    ref, mag, _ = conv_reference(x[None, None], None, w, b, 1, res=None if r is None else r[None, None])
    pw = packed(w, b, 1)
    xd, rd = dev_bf(x), (wide(r, N + 8) if res else None)
    g = P.guarded((M, N), pitch=N + 8, pad_rows=3, dtype=BF, device=DEV)
    inputs = snaps(xd, pw.w, pw.bias, rd)
    with tuning(k15=fm2):
        kw = dict(res=None if rd is None else rd[None, None], out=g.view[None, None])
        assert ops.conv_path(xd[None, None], pw, **kw) == path
        ops.linear(xd, pw, res=rd, out=g.view)
        worst = finish(f"rowblock K {K} M {M}", g, ref.reshape(M, N), P.gemm_bound(ref, mag, K, BF).reshape(M, N), inputs)
    print(f"rowblock K {K} M {M} fm2 {fm2} res {res} (path {path}): worst err/bound {worst:.3f}")


# ---------------------------------------------------------------- scalar epilogue (N % 8 != 0)
@pytest.mark.parametrize("out_dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("split", [0, 2])
def test_scalar_epilogue(gpu, out_dtype, split):
    """N = 20, output pitch 28, residual pitch 36: epi_chunk's element-by-element side (vec ==
    false in store_tile and splitk_reduce_kernel).  Read before the first run: the weight rows
    past N come from the zero page (brow < a.N), bias / rowvec / residual / y are indexed below
    column N only, the split-K slab has pitch N -- in bounds for any N."""
    M, Cin, N = 129, 72, 20
    x = P.bf16_round(rnd(M, Cin, seed=1))
    w = P.bf16_round(rnd(N, Cin, seed=2, scale=1 / math.sqrt(Cin)))
    b = rnd(N, seed=3, scale=0.1)
    res = P.bf16_round(rnd(M, N, seed=4))
    tv = rnd(3, N, seed=5)
    ref, mag, _ = conv_reference(x[None, None], None, w, b, 1, rowvec=(tv, 50, 0), res=res[None, None], out_scale=0.5)
    pw = packed(w, b, 1)
    xd, rd, td = dev_bf(x), wide(res, 36), tv.to(DEV)
    g = P.guarded((M, N), pitch=28, pad_rows=3, dtype=out_dtype, device=DEV)
    inputs = snaps(xd, pw.w, pw.bias, rd, td)
    ops.linear(xd, pw, rowvec=(td, 50, N), res=rd, out_scale=0.5, out=g.view, split_k=split)
    worst = finish(f"scalar epilogue {out_dtype}", g, ref.reshape(M, N), P.gemm_bound(ref, mag, Cin, out_dtype).reshape(M, N),
                   inputs)
    print(f"scalar epilogue N 20 {out_dtype} split {split}: worst err/bound {worst:.3f}")


# ---------------------------------------------------------------- epilogue operands
EPI_CASES = ["nobias", "rowvec50", "rowvec_ld", "rowvec_mod3", "res_ldr", "scale", "gelu", "silu", "geglu", "all"]


@pytest.mark.parametrize("case", EPI_CASES)
def test_epilogue_operands(gpu, case):
    """One epilogue operand each, then all together (with SiLU): no bias; a row vector whose
    rows_per_vec = 50 does not divide the tile height; rowvec_ld > N; rowvec_mod 3; a residual
    with ldr > N; out_scale 0.5; GELU, SiLU, GEGLU (bias only: anything else is
    LS_ERR_INVALID) with the activation bounds of parity.act_bound / geglu_bound."""
    M, Cin, N = 300, 320, (64 if case == "geglu" else 72)
    every = case == "all"
    x = P.bf16_round(rnd(M, Cin, seed=11))
    w = P.bf16_round(rnd(N, Cin, seed=12, scale=1 / math.sqrt(Cin)))
    b = None if case == "nobias" else rnd(N, seed=13, scale=0.1)
    kw, rkw = {}, {}
    if case.startswith("rowvec") or every:
        ld = 80 if case == "rowvec_ld" or every else N
        mod = 3 if case == "rowvec_mod3" or every else 0
        tv = rnd(3 if mod else 6, ld, seed=14)
        td = tv.to(DEV)
        kw["rowvec"], rkw["rowvec"] = (td, 50, ld, mod), (tv, 50, mod)
    if case == "res_ldr" or every:
        res = P.bf16_round(rnd(M, N, seed=15))
        kw["res"], rkw["res"] = wide(res, N + 24), res[None, None]
    if case == "scale" or every:
        kw["out_scale"] = rkw["out_scale"] = 0.5
    act = {"gelu": ops.ACT_GELU, "silu": ops.ACT_SILU, "geglu": ops.ACT_GEGLU, "all": ops.ACT_SILU}.get(case, 0)
    pre, mag, _ = conv_reference(x[None, None], None, w, b, 1, **rkw)
    pre, mag = pre.reshape(M, N), mag.reshape(M, N)
    if act == ops.ACT_GEGLU:
        b_pre = P.gemm_bound(pre, mag, Cin, None)
        ref, bound = P.geglu_bound(pre[:, :32], b_pre[:, :32], pre[:, 32:], b_pre[:, 32:], BF)
    elif act:
        ref, bound = P.act_bound("gelu" if act == ops.ACT_GELU else "silu", pre, P.gemm_bound(pre, mag, Cin, None), BF)
    else:
        ref, bound = pre, P.gemm_bound(pre, mag, Cin, BF)
    pw = packed(w, b, 1, geglu=act == ops.ACT_GEGLU)
    xd = dev_bf(x)
    n_out = ref.shape[1]
    g = P.guarded((M, n_out), pitch=n_out + 8, pad_rows=3, dtype=BF, device=DEV)
    inputs = snaps(xd, pw.w, pw.bias, kw.get("res"), kw["rowvec"][0] if "rowvec" in kw else None)
    ops.linear(xd, pw, act=act, out=g.view, **kw)
    worst = finish(f"epilogue {case}", g, ref, bound, inputs)
    print(f"epilogue {case}: worst err/bound {worst:.3f}")


def test_geglu_rejects_other_epilogue_operands(gpu):
    """The GEGLU epilogues add the bias only; a rowvec, a residual or an out_scale with GEGLU is
    refused by the argument check (nothing launched) instead of being silently dropped."""
    M, Cin, N = 32, 64, 64
    pw = packed(rnd(N, Cin, seed=1), rnd(N, seed=2), 1, geglu=True)
    xd = dev_bf(rnd(M, Cin, seed=3))
    g = P.guarded((M, N // 2), pitch=40, dtype=BF, device=DEV)
    for kw in (dict(res=dev_bf(rnd(M, N // 2, seed=4))), dict(out_scale=0.5), dict(rowvec=(rnd(1, 32).to(DEV), M, 32))):
        assert ops.conv_path(xd[None, None], pw, act=ops.ACT_GEGLU, out=g.view[None, None],
                             **{k: (v[None, None] if k == "res" else v) for k, v in kw.items()}) == -1
        with pytest.raises(RuntimeError, match="GEGLU"):
            ops.linear(xd, pw, act=ops.ACT_GEGLU, out=g.view, **kw)
    torch.cuda.synchronize()
    P.assert_guard_intact(g)
    assert bool((g.view.contiguous().view(torch.int16) == 0x7FC1).all())  # nothing was written


# ---------------------------------------------------------------- ksize 3: the tiled gather
IMAGES = ((5, 7), (12, 9))
CONV_VARIANTS = {"s1": {}, "s2p1": dict(stride=2, pad=1), "vae_down": dict(vae_down=True), "up2": dict(upsample=True)}


def run_conv3(name, x1, x2, w, b, N, variant, aff=None, ld1=None, ld2=None, expect_path=None, tune=None, res=False,
              upsample_hw=None):
    """One 3x3 call: reference, guarded output of pitch N + 8, parity, guards, inputs."""
    n, H, W, _ = x1.shape
    rkw = dict(CONV_VARIANTS[variant])
    kw = {k: v for k, v in rkw.items() if k != "vae_down"}
    if variant == "vae_down":
        kw.update(stride=2, pad=0, out_hw=((H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1))
    sc = sh = None
    if aff is not None:
        sc, sh, ips, silu = aff
        rkw["aff"] = aff
    ref, mag, prod = conv_reference(x1, x2, w, b, 3, **rkw)
    Ho, Wo = ref.shape[1:3]
    r = P.bf16_round(rnd(n, Ho, Wo, N, seed=77)) if res else None
    if res:
        ref, mag = ref + P.f64(r), mag + P.f64(r).abs()
    Cin = x1.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
    bound = P.gemm_bound(ref, mag, 9 * Cin, BF, prologue=aff is not None, prod_mag=prod)
    pw = packed(w, b, 3)
    x1d = wide(x1, ld1) if ld1 else dev_bf(x1)
    x2d = None if x2 is None else (wide(x2, ld2) if ld2 else dev_bf(x2))
    if aff is not None:
        scd, shd = sc.float().to(DEV), sh.float().to(DEV)
        kw["aff"] = (scd, shd, ips, silu)
    if res:
        kw["res"] = wide(r, N + 8)
    g = P.guarded((n, Ho, Wo, N), pitch=N + 8, pad_rows=3, dtype=BF, device=DEV)
    inputs = snaps(x1d, x2d, pw.w, pw.bias, kw.get("res"), *(kw["aff"][:2] if aff is not None else ()))
    with tuning(**(tune or {})):
        if expect_path is not None:
            assert ops.conv_path(x1d, pw, x2=x2d, out=g.view, **kw) == expect_path, name
        ops.conv(x1d, pw, x2=x2d, out=g.view, **kw)
        return finish(name, g, ref, bound, inputs)


@pytest.mark.parametrize("variant", list(CONV_VARIANTS))
@pytest.mark.parametrize("Cin", [8, 24, 72, 64, 128])
def test_conv3x3_gather(gpu, Cin, variant):
    """5 x 7 and 12 x 9 images, n_img 3 (M = 105 / 324 and their strided / upsampled forms: odd
    sizes, more than one 128-row tile): Cin 8 / 24 / 72 tap-major K with a padded tail, Cin
    64 / 128 chunk-major K through the buffer-descriptor DMA; stride 1, stride 2 + pad 1 on odd
    H, the VAE's stride-2 pad-0 downsampler, nearest x2 upsample."""
    N, worst = 40, 0.0
    for H, W in IMAGES:
        x = P.bf16_round(rnd(3, H, W, Cin, seed=H + Cin))
        w = P.bf16_round(rnd(N, Cin, 3, 3, seed=Cin + 1, scale=1 / math.sqrt(9 * Cin)))
        b = rnd(N, seed=2, scale=0.1)
        worst = max(worst, run_conv3(f"conv3x3 {variant} Cin {Cin} {H}x{W}", x, None, w, b, N, variant, expect_path=0))
    print(f"conv3x3 {variant} Cin {Cin}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("prologue", [False, True])
def test_conv3x3_concat_wide_buffers(gpu, prologue):
    """The fused concat with C1 = 40, C2 = 24 read from wider buffers (ld1 = 48, ld2 = 32);
    with and without the affine + SiLU prologue over both sources."""
    N, worst = 40, 0.0
    for H, W in IMAGES:
        x1 = P.bf16_round(rnd(3, H, W, 40, seed=H))
        x2 = P.bf16_round(rnd(3, H, W, 24, seed=H + 1))
        w = P.bf16_round(rnd(N, 64, 3, 3, seed=3, scale=1 / 24))
        b = rnd(N, seed=4, scale=0.1)
        aff = (1 + 0.2 * rnd(3, 64, seed=5), 0.5 + 0.3 * rnd(3, 64, seed=6), 1, True) if prologue else None
        worst = max(worst, run_conv3(f"concat {H}x{W} prologue {prologue}", x1, x2, w, b, N, "s1", aff=aff, ld1=48, ld2=32,
                                     expect_path=2 if prologue else 0))
    print(f"conv3x3 concat prologue {prologue}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("Cin", [24, 64])
@pytest.mark.parametrize("variant", ["s1", "s2p1"])
def test_conv3x3_prologue_padding_stays_zero(gpu, Cin, variant):
    """The GroupNorm affine + SiLU prologue with a shift of about +2: silu(shift) is far from 0,
    so a padding tap (or the padded K tail) put through the prologue instead of staying zero
    moves every border pixel far outside the bound.  One affine per image (3 samples)."""
    N, worst = 40, 0.0
    for H, W in IMAGES:
        x = P.bf16_round(rnd(3, H, W, Cin, seed=H + Cin))
        w = P.bf16_round(rnd(N, Cin, 3, 3, seed=Cin + 1, scale=1 / math.sqrt(9 * Cin)))
        b = rnd(N, seed=2, scale=0.1)
        aff = (1 + 0.2 * rnd(3, Cin, seed=7), 2.0 + 0.3 * rnd(3, Cin, seed=8), 1, True)
        worst = max(worst, run_conv3(f"prologue {variant} Cin {Cin} {H}x{W}", x, None, w, b, N, variant, aff=aff,
                                     expect_path=2))
    print(f"conv3x3 prologue {variant} Cin {Cin}: worst err/bound {worst:.3f}")


# ---------------------------------------------------------------- halo kernel
HALO = [(Cin, N, aff, th8) for Cin in (64, 128) for N in (128, 160, 16, 8) for aff in (False, True) for th8 in (1, 0)
        if th8 == 1 or N == 128]  # key 16 picks the patch form of the 128-column tiles only


@pytest.mark.parametrize("Cin,N,aff,th8", HALO)
def test_halo_edges(gpu, Cin, N, aff, th8):
    """conv3x3_halo_kernel (path 3) on one 16 x 16 patch and on 32 x 16 (an inner patch edge),
    n_img 2: 128- / 160-column tiles, the narrow 16-column tile (N 16 / 8), with and without
    the affine + SiLU input transform, without and with a residual of pitch N + 8, both patch
    forms of tuning key 16."""
    worst = 0.0
    for H, W in ((16, 16), (32, 16)):
        x = P.bf16_round(rnd(2, H, W, Cin, seed=H + Cin) * 2 + 0.5)
        w = P.bf16_round(rnd(N, Cin, 3, 3, seed=N + 1, scale=1 / math.sqrt(9 * Cin)))
        b = rnd(N, seed=2, scale=0.1)
        a = (1 + 0.2 * rnd(2, Cin, seed=7), 0.5 + 0.3 * rnd(2, Cin, seed=8), 1, True) if aff else None
        for res in (False, True):
            worst = max(worst, run_conv3(f"halo Cin {Cin} N {N} aff {aff} th8 {th8} {H}x{W} res {res}", x, None, w, b, N,
                                         "s1", aff=a, expect_path=3, tune=dict(k16=th8), res=res))
    print(f"halo Cin {Cin} N {N} aff {aff} th8 {th8}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("Cin,N", [(64, 128), (128, 160), (128, 128), (64, 16), (128, 8)])
def test_halo_upsample_edge(gpu, Cin, N):
    """The upsample form at its smallest: 8 x 8 -> 16 x 16, one patch per image (two 16 x 8
    patches on the 128-column and the narrow tiles).  Read before the first run of narrow +
    upsample: the halo pixels come through per-image buffer descriptors with (y >> 1, x >> 1)
    of in-image (y, x) only, and the launch tiles the OUTPUT image, whose sides halo_tw requires
    to be multiples of 16."""
    x = P.bf16_round(rnd(2, 8, 8, Cin, seed=Cin))
    w = P.bf16_round(rnd(N, Cin, 3, 3, seed=N, scale=1 / math.sqrt(9 * Cin)))
    b = rnd(N, seed=2, scale=0.1)
    worst = run_conv3(f"halo upsample Cin {Cin} N {N}", x, None, w, b, N, "up2", expect_path=3, res=True)
    print(f"halo upsample Cin {Cin} N {N}: worst err/bound {worst:.3f}")


def test_forced_big_tile_with_prologue(gpu):
    """A forced 256-row tile (tuning key 2 = 5 / 6) on a call with the affine prologue: the
    256-row kernels have no register-staged form, so the call runs a 128-row kernel, and the grid
    must be that kernel's: on the 256-row grid a smaller tile leaves most rows unwritten."""
    M, Cin, N = 300, 64, 72
    x = P.bf16_round(rnd(1, 1, M, Cin, seed=1))
    w = P.bf16_round(rnd(N, Cin, seed=2, scale=1 / 8))
    b = rnd(N, seed=3, scale=0.1)
    aff = (1 + 0.2 * rnd(1, Cin, seed=4), 0.3 * rnd(1, Cin, seed=5), 1, True)
    ref, mag, prod = conv_reference(x, None, w, b, 1, aff=aff)
    bound = P.gemm_bound(ref, mag, Cin, BF, prologue=True, prod_mag=prod)
    pw = packed(w, b, 1)
    xd = dev_bf(x)
    for tile in (5, 6):
        g = P.guarded((1, 1, M, N), pitch=N + 8, pad_rows=3, dtype=BF, device=DEV)
        with tuning(k2=tile):
            ops.conv(xd, pw, aff=(aff[0].to(DEV), aff[1].to(DEV), 1, True), out=g.view)
            worst = finish(f"forced tile {tile} with prologue", g, ref, bound, snaps(xd, pw.w))
        print(f"forced tile {tile} with prologue: worst err/bound {worst:.3f}")
