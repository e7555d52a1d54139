"""The UNet's audio conditioning per element (tests/parity.py): ls_log_mel, and every call of the
Whisper encoder (audio._DeviceWhisper.encode) on its own at the encoder's real shapes.

ls_log_mel is called through the C ABI: the bf16 output inside a sentinel guard band, the
workspace filled with 0xA5 and followed by a sentinel tail.  Both of its results are checked per
element against the fp64 STFT oracle with parity.log_mel_bound: the fp32 log10 mel rows the first
kernel leaves in the workspace (T x n_mels floats at byte offset 256, include/ls_hip.h) -- the bf16
rounding of the output hides about 4e-3 of error by itself -- and the normalised bf16 output, whose
rows T .. t_pad must be +0.0 bit for bit.

The encoder's calls run at n_seg = 2 (3000 rows of 11 x 128 + 92 per segment) with the weights of
Audio2Feature.random and operands passed as encode passes them: row-strided views X[:, l] of one
stacked X[rows][5][384] that starts as sentinels and sits in a guard band; after each call every
layer slot it must not write is compared bit for bit.  References are fp64 on the bf16-rounded
operands, bounds the helpers of parity.py.  Every case first asserts the kernel family ops.conv_plan
reports (all six GEMMs plan onto the tiled kernels, family 0: the LayerNorm fold is the epilogue
form), so a dispatch change fails here rather than testing another kernel silently."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import parity as P
import test_gpu_edges_gemm as E
from latentsync_amd import _lib, ops
from latentsync_amd.audio import Audio2Feature, mel_filters

pytestmark = pytest.mark.gpu
DEV, BF, F32, U8 = "cuda", torch.bfloat16, torch.float32, torch.uint8
WS_HEAD, WS_TAIL = 256, 4096  # bytes in front of the log-mel rows; sentinel bytes behind the workspace


# ---------------------------------------------------------------- ls_log_mel
@functools.lru_cache(maxsize=None)
def filters(n_mels):
    return torch.from_numpy(mel_filters(n_mels=n_mels))


@functools.lru_cache(maxsize=None)
def oracle(n, kind, n_mels, t_pad):
    return P.log_mel_bound(P.mel_signal(n, kind), filters(n_mels), t_pad)


def call_log_mel(wd, fd, n_mels, t_pad, out, ws, nbytes):
    lib = _lib.load()
    rc = lib.ls_log_mel(wd.data_ptr(), wd.numel(), fd.data_ptr(), n_mels, t_pad, out.data_ptr(), ws.data_ptr(), nbytes,
                        ops._stream())
    assert rc == 0, lib.ls_last_error().decode()
    torch.cuda.synchronize()


def run_log_mel(n, kind, n_mels, t_pad):
    """One call: both results per element, the zero rows, the guard band, the workspace's unused
    head (bytes 4 .. 255) and its tail, the inputs.  Returns (l fp32, v bf16 as fp32, worst ratios)."""
    lib = _lib.load()
    T = n // P.MEL_HOP
    wave = P.mel_signal(n, kind)
    wd, fd = wave.to(DEV).contiguous(), filters(n_mels).to(DEV).contiguous()
    nbytes = lib.ls_log_mel_workspace_bytes(n, n_mels)
    assert nbytes == WS_HEAD + T * n_mels * 4
    ws = torch.full((nbytes + WS_TAIL,), 0xA5, dtype=U8, device=DEV)
    g = P.guarded((t_pad, n_mels), dtype=BF, device=DEV)
    inputs = E.snaps(wd, fd)
    call_log_mel(wd, fd, n_mels, t_pad, g.view, ws, nbytes)
    name = f"log_mel n {n} {kind} mels {n_mels} t_pad {t_pad}"
    l_ref, l_b, v_ref, v_b = oracle(n, kind, n_mels, t_pad)
    l = ws[WS_HEAD:nbytes].view(F32).reshape(T, n_mels).cpu()
    v = g.view.float().cpu()
    wl = P.assert_elementwise(l, l_ref, l_b, where=dict(rows=P.MEL_BLOCK, cols=n_mels), name=name + " fp32 log-mel")
    wv = P.assert_elementwise(v, v_ref, v_b, where=dict(rows=P.MEL_BLOCK, cols=n_mels), name=name + " output")
    if t_pad > T:
        assert int(g.view[T:].contiguous().view(torch.int16).abs().max()) == 0, f"{name}: rows T .. t_pad are not +0.0"
    P.assert_guard_intact(g, name)
    assert bool((ws[4:WS_HEAD] == 0xA5).all()), f"{name}: workspace bytes 4 .. 255 were written"
    assert bool((ws[nbytes:] == 0xA5).all()), f"{name}: bytes past ls_log_mel_workspace_bytes were written"
    for i, (t, snap) in enumerate(inputs):
        P.assert_unchanged(t, snap, f"{name} input {i}")
    print(f"{name}: worst err/bound fp32 log-mel {wl:.3f}, bf16 output {wv:.3f}")
    return l, v, wl, wv


@pytest.mark.parametrize("pad3000", [False, True], ids=["t_pad_T", "t_pad_3000"])
@pytest.mark.parametrize("n", P.MEL_N)
def test_log_mel_frame_edges(gpu, n, pad3000):
    """T = 1 (n 201, 319) and 2 (320); T % 8 = 7 (1279), 0 (1319, 1320), 1 (4000, 4159) and 2 (40000, the
    golden clip's length: 31 blocks and two frames); n % 160 below 40 (201, 1320, 4000, 40000: the last
    frame reflects at the end of the clip) and above (319, 1279, 1319, 4159: it does not); t_pad = T
    and the encoder's 3000."""
    T = n // P.MEL_HOP
    run_log_mel(n, "mix", 80, 3000 if pad3000 else T)


def test_log_mel_128_bands(gpu):
    """n_mels = 128 (the limit): 8 x 128 = 1024 band sums over 256 threads."""
    run_log_mel(4159, "mix", 128, 4159 // P.MEL_HOP + 5)


@pytest.mark.parametrize("kind", P.MEL_FLOOR_KINDS)
def test_log_mel_floor(gpu, kind):
    """The clip-wide max - 8 floor: loud then exact zeros, loud then -60 dB, the loudest frame
    first / last (the last in the partial block of T = 25), all zeros (every output exactly -1.5),
    and noise of 1e-3 (every log value negative: the negative branch of ord_enc / ord_dec)."""
    n = P.MEL_FLOOR_N
    T = n // P.MEL_HOP
    l_ref = oracle(n, kind, 80, T + 3)[0]
    if kind in ("zeros_after", "loud_first", "loud_last"):  # the floor is in force somewhere, and not everywhere
        clamped = l_ref < l_ref.max() - 8.0
        assert bool(clamped.any()) and not bool(clamped.all())
    if kind == "loud_first":
        assert int(l_ref.amax(1).argmax()) == 0
    if kind == "loud_last":
        assert int(l_ref.amax(1).argmax()) == T - 1 and (T - 1) % P.MEL_BLOCK == 0
    if kind == "noise1e-3":
        assert float(l_ref.max()) < 0
    l, v, _, _ = run_log_mel(n, kind, 80, T + 3)
    if kind == "zeros":
        assert bool((v[:T] == -1.5).all())


def test_log_mel_twice_on_a_dirty_workspace(gpu):
    """The same call twice on one workspace (dirty from the first call: the maximum slot holds the
    last clip's value) and then once more after a louder clip used it: bit-identical results."""
    lib = _lib.load()
    n, n_mels = P.MEL_N[0], 80
    T = n // P.MEL_HOP
    fd = filters(n_mels).to(DEV).contiguous()
    wd = P.mel_signal(n, "mix").to(DEV).contiguous()
    loud = (100.0 * P.mel_signal(n, "mix")).to(DEV).contiguous()
    nbytes = lib.ls_log_mel_workspace_bytes(n, n_mels)
    ws = torch.full((nbytes + WS_TAIL,), 0xA5, dtype=U8, device=DEV)
    outs, works = [], []
    for w in (wd, wd, loud, wd):
        g = P.guarded((T + 2, n_mels), dtype=BF, device=DEV)
        call_log_mel(w, fd, n_mels, T + 2, g.view, ws, nbytes)
        P.assert_guard_intact(g, "log_mel twice")
        outs.append(g.view.contiguous().view(torch.int16).cpu())
        works.append(ws[WS_HEAD:nbytes].clone().cpu())
    for i in (1, 3):
        assert torch.equal(outs[0], outs[i]) and torch.equal(works[0], works[i]), f"call {i} differs from the first"
    assert not torch.equal(outs[0], outs[2])
    assert bool((ws[nbytes:] == 0xA5).all()) and bool((ws[4:WS_HEAD] == 0xA5).all())


# ---------------------------------------------------------------- the encoder's calls
NSEG, FRAMES, CTX, C, SLOTS, HEADS, D = 2, 3000, 1500, 384, 5, 6, 64
ROWS = NSEG * CTX
LI = 1  # the layer the GEMM cases stand in for: x = X[:, 1], y = X[:, 2], weights of blocks[1]
EPS = 1e-5
ENC_NEEDLE_KEYS = (0, 63, 64, 127, 128, 1407, 1408, 1498, 1499)  # 1408 = 11 x 128: the partial last tile
WORST = {}


@functools.lru_cache(maxsize=1)
def whisper():
    a = Audio2Feature.random(seed=0, device=DEV)
    return a, a._require()


def stacked():
    """The guarded X[rows][5][384], every element a sentinel."""
    g = P.guarded((ROWS, SLOTS, C), dtype=BF, device=DEV)
    assert g.view.stride() == (SLOTS * C, C, 1)
    return g, g.view


def assert_slots_untouched(g, before, written, name):
    for l in range(SLOTS):
        if l != written:
            P.assert_unchanged(g.view[:, l], before[:, l], f"{name}: layer slot {l}")
    P.assert_guard_intact(g, name)


def planned_conv(name, x4, pw, **kw):
    """ops.conv with the whole split-K workspace, as encode's calls have it, after asserting that the
    plan for exactly this call is the tiled family.  Returns the plan."""
    kw["workspace_bytes"] = ops.workspace(x4.device).gemm.numel()
    plan = ops.conv_plan(x4, pw, **kw)
    assert plan is not None, f"{name}: {_lib.load().ls_last_error().decode()}"
    assert plan["family"] == 0, f"{name}: planned on family {plan['family']}, the case was written for the tiled kernels ({plan})"
    ops.conv(x4, pw, **kw)
    return plan


def as4(t):
    return t.unsqueeze(0).unsqueeze(0)  # ops.linear's view of a (rows, C) operand


def done(name, worst, plan=None):
    WORST[name] = worst
    extra = "" if plan is None else f" (tile {plan['bm']}x{plan['bn']}, split {plan['split']}, grid {plan['grid']})"
    print(f"{name}: worst err/bound {worst:.3f}{extra}")


def conv1d_reference(x, w, b, stride):
    """fp64 (ref, mag), each (n, Wo, N), of the k = 3, padding 1 conv1d per segment: x (n, W, Cin)
    bf16-rounded, w (N, Cin, 3) bf16-rounded, b (N,) fp32.  (The kernel runs it as a 3x3 conv on
    a one-row image whose other two kernel rows are zero: those products are exact zeros.)"""
    xt = P.f64(x).transpose(1, 2)
    ref = F.conv1d(xt, P.f64(w), P.f64(b), stride=stride, padding=1)
    mag = F.conv1d(xt.abs(), P.f64(w).abs(), P.f64(b).abs(), stride=stride, padding=1)
    return ref.transpose(1, 2), mag.transpose(1, 2)


def boundary_x8(x):
    """The rows either side of the segment boundary times 8: a tap that reads the neighbouring
    segment where it should read the zero padding is then far outside the bound."""
    x[0, -1] *= 8.0
    x[1, 0] *= 8.0
    return P.bf16_round(x)


@pytest.mark.parametrize("which", ["conv1", "conv2"])
def test_encoder_conv(gpu, which):
    """conv1: (2, 1, 3000, 80) -> 384, GELU (Cin = 80 is no multiple of 64: the tap-major packing);
    conv2: stride 2 -> (2, 1, 1500, 384), GELU (channel-chunk-major; split over K with the workspace)."""
    a, dev = whisper()
    cin, stride, pw = (80, 1, dev.conv1) if which == "conv1" else (C, 2, dev.conv2)
    w = P.bf16_round(a.sd[f"encoder.{which}.weight"])
    b = a.sd[f"encoder.{which}.bias"].float()
    assert tuple(w.shape) == (C, cin, 3)
    x = boundary_x8(E.rnd(NSEG, FRAMES, cin, seed=3 + cin))
    xd = E.dev_bf(x).view(NSEG, 1, FRAMES, cin)
    wo = FRAMES // stride
    g = P.guarded((NSEG, 1, wo, C), pad_rows=3, dtype=BF, device=DEV)
    inputs = E.snaps(xd, pw.w, pw.bias)
    name = f"encoder {which}"
    plan = planned_conv(name, xd, pw, stride=stride, act=ops.ACT_GELU, out=g.view)
    ref, mag = conv1d_reference(x, w, b, stride)
    ref, bound = P.act_bound("gelu", ref, P.gemm_bound(ref, mag, 3 * cin, None), BF)
    done(name, E.finish(name, g, ref.reshape(NSEG, 1, wo, C), bound.reshape(NSEG, 1, wo, C), inputs), plan)


def test_encoder_add_rows(gpu):
    """h2 + positional embedding into X[:, 0] (pitch 1920): the 1500-row table wraps once."""
    a, dev = whisper()
    h2 = P.bf16_round(E.rnd(ROWS, C, seed=11))
    hd = E.dev_bf(h2)
    g, X = stacked()
    before = P.snapshot(X)
    inputs = E.snaps(hd, dev.pos)
    ops.add_rows(hd, dev.pos, out=X[:, 0])
    torch.cuda.synchronize()
    t = P.f64(dev.pos)[torch.arange(ROWS) % CTX]
    ref = P.f64(h2) + t
    name = "encoder add_rows"
    worst = P.assert_elementwise(X[:, 0], ref, P.elem_bound(ref, P.f64(h2).abs() + t.abs(), BF), where=E.FRAG, name=name)
    assert_slots_untouched(g, before, 0, name)
    for i, (t_, s) in enumerate(inputs):
        P.assert_unchanged(t_, s, f"{name} input {i}")
    done(name, worst)


def residual_rows(seed):
    """A residual stream: rows of deviation 0.5 .. 2 around a mean of one deviation."""
    return P.ln_case(ROWS, C, 1, seed)[0]


def row_stats_of(x_view, name):
    """ls_row_stats of a strided view into a guarded (rows, 2), checked per row."""
    lib = _lib.load()
    g_st = P.guarded((ROWS, 2), pad_rows=8, dtype=F32, device=DEV)
    rc = lib.ls_row_stats(x_view.data_ptr(), x_view.stride(0), ROWS, C, EPS, g_st.view.data_ptr(), ops._stream())
    assert rc == 0, lib.ls_last_error().decode()
    torch.cuda.synchronize()
    sref, sb = P.row_stats_bound(x_view.float().cpu(), EPS)
    worst = P.assert_elementwise(g_st.view, sref, sb, where=dict(rows=16, cols=2), name=name + " row_stats")
    P.assert_guard_intact(g_st, name + " row_stats")
    return g_st.view, worst


def fold_form(plan):
    return "rows" if plan["family"] == 1 else "epilogue"


def test_encoder_row_stats_qkv(gpu):
    """ls_row_stats of X[:, 1] (rows 1920 apart) and the fused q|k|v GEMM with attn_ln folded in,
    N = 1152, from those statistics."""
    a, dev = whisper()
    pw = dev.blocks[LI].qkv
    x = residual_rows(21)
    g, X = stacked()
    X[:, LI].copy_(x)
    before = P.snapshot(X)
    name = "encoder qkv"
    st, w_st = row_stats_of(X[:, LI], name)
    gy = P.guarded((ROWS, 3 * C), pad_rows=3, dtype=BF, device=DEV)
    inputs = E.snaps(pw.w, pw.bias, pw.colsum, st)
    plan = planned_conv(name, as4(X[:, LI]), pw, ln_stats=st, out=as4(gy.view))
    ref, bound = P.ln_fold_bound(x, st.cpu(), pw.w.float().cpu(), pw.colsum.cpu(), pw.bias.cpu(), form=fold_form(plan))
    worst = E.finish(name, gy, ref, bound, inputs)
    assert_slots_untouched(g, before, None, name)
    done(name + " row_stats", w_st)
    done(name, worst, plan)


def test_encoder_attention(gpu):
    """batch 2, 6 heads of d = 64 over 1500 keys (11 full 128-key tiles and one of 92), q / k / v read
    out of one (3000, 1152) fused-qkv buffer.  d = 64 with nk > 32 dispatches to attn3_kernel
    (launch_attn3<2, 4, 0>, "case 4" of ls_attention's switch), which multiplies Q by scale log2(e) and
    rounds it to bf16 again ("f[e] *= c2; qf[g][kc] = ... pack8(f)"): q_prescaled=True."""
    q, k, v = P.needle_qkv(NSEG, HEADS, CTX, CTX, D, seed=31, keys=ENC_NEEDLE_KEYS)
    assert not torch.equal(q[0], q[1]) and not torch.equal(v[0], v[1])  # the segments differ
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(ROWS, C)
    qkv = torch.cat([rows(q), rows(k), rows(v)], 1).to(BF).to(DEV).contiguous()
    g = P.guarded((ROWS, C), pad_rows=3, dtype=BF, device=DEV)
    snap = P.snapshot(qkv)
    qs = (CTX * 3 * C, 0, 3 * C, D)
    ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], g.view, batch=NSEG, z2=1, heads=HEADS, nq=CTX, nk=CTX, head_dim=D,
                  qs=qs, ks=qs, vs=qs, os_=(CTX * C, 0, C, D))
    torch.cuda.synchronize()
    got = g.view.float().cpu().reshape(NSEG, CTX, HEADS, D).permute(0, 2, 1, 3)
    name = "encoder attention"
    worst = 0.0
    for s in range(NSEG):  # one segment at a time: the fp64 score matrices are 6 x 1500 x 1500 each
        ref, bound = P.attn_bound(q[s], k[s], v[s], 1 / math.sqrt(D), q_prescaled=True)
        worst = max(worst, P.assert_elementwise(got[s], ref, bound, where=dict(rows=16, cols=16), name=f"{name} segment {s}"))
    P.assert_guard_intact(g, name)
    P.assert_unchanged(qkv, snap, name + " qkv")
    done(name, worst)


def test_encoder_out_projection(gpu):
    """o W^T + b + x with the residual x = X[:, 1] and the output y = X[:, 2], both of pitch 1920."""
    a, dev = whisper()
    pw = dev.blocks[LI].out
    o, x = P.bf16_round(E.rnd(ROWS, C, seed=41)), residual_rows(42)
    od = E.dev_bf(o)
    g, X = stacked()
    X[:, LI].copy_(x)
    before = P.snapshot(X)
    inputs = E.snaps(od, pw.w, pw.bias)
    name = "encoder out projection"
    plan = planned_conv(name, as4(od), pw, res=as4(X[:, LI]), out=as4(X[:, LI + 1]))
    torch.cuda.synchronize()
    ref, mag = P._linear(o, pw.w.float().cpu(), pw.bias.cpu(), x)
    worst = P.assert_elementwise(X[:, LI + 1], ref, P.gemm_bound(ref, mag, C, BF), where=E.FRAG, name=name)
    assert_slots_untouched(g, before, LI + 1, name)
    for i, (t, s) in enumerate(inputs):
        P.assert_unchanged(t, s, f"{name} input {i}")
    done(name, worst, plan)


def test_encoder_mlp1(gpu):
    """mlp_ln folded into mlp.0, N = 1536, GELU, from the row statistics of y = X[:, 2]."""
    a, dev = whisper()
    pw = dev.blocks[LI].mlp1
    y = residual_rows(51)
    g, X = stacked()
    X[:, LI + 1].copy_(y)
    before = P.snapshot(X)
    name = "encoder mlp1"
    st, w_st = row_stats_of(X[:, LI + 1], name)
    gm = P.guarded((ROWS, 4 * C), pad_rows=3, dtype=BF, device=DEV)
    inputs = E.snaps(pw.w, pw.bias, pw.colsum, st)
    plan = planned_conv(name, as4(X[:, LI + 1]), pw, act=ops.ACT_GELU, ln_stats=st, out=as4(gm.view))
    pre, b_pre = P.ln_fold_bound(y, st.cpu(), pw.w.float().cpu(), pw.colsum.cpu(), pw.bias.cpu(), out_dtype=None,
                                 form=fold_form(plan))
    ref, bound = P.act_bound("gelu", pre, b_pre, BF)
    worst = E.finish(name, gm, ref, bound, inputs)
    assert_slots_untouched(g, before, None, name)
    done(name + " row_stats", w_st)
    done(name, worst, plan)


def test_encoder_mlp2_in_place(gpu):
    """m W^T + b + y with K = 1536 and res = out = the same strided view X[:, 2] (split over K with
    the workspace: the reduce pass reads the residual it overwrites); the reference is taken from a
    copy of y made before the call."""
    a, dev = whisper()
    pw = dev.blocks[LI].mlp2
    m, y = P.bf16_round(E.rnd(ROWS, 4 * C, seed=61)), residual_rows(62)
    md = E.dev_bf(m)
    g, X = stacked()
    X[:, LI + 1].copy_(y)
    before = P.snapshot(X)
    inputs = E.snaps(md, pw.w, pw.bias)
    name = "encoder mlp2"
    plan = planned_conv(name, as4(md), pw, res=as4(X[:, LI + 1]), out=as4(X[:, LI + 1]))
    torch.cuda.synchronize()
    ref, mag = P._linear(m, pw.w.float().cpu(), pw.bias.cpu(), before[:, LI + 1].float().cpu())
    worst = P.assert_elementwise(X[:, LI + 1], ref, P.gemm_bound(ref, mag, 4 * C, BF), where=E.FRAG, name=name)
    assert_slots_untouched(g, before, LI + 1, name)
    for i, (t, s) in enumerate(inputs):
        P.assert_unchanged(t, s, f"{name} input {i}")
    done(name, worst, plan)
