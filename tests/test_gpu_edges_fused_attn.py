"""ls_cross_attention_block (ls_xattn.hip) and ls_temporal_attention (ls_motion.hip) per element.
The fp64 references are built from the logical tensors (to_q with norm2 folded and rounded once as
ops.pack_cross_attention does; wq / wk / wv rounded as ops.pack_temporal rounds them, the q
pre-scale divided out again in fp64), the bounds are composed stage by stage (parity.xattn_bound,
parity.tattn_bound).  x, kv and the outputs sit in NaN guard bands with pitches wider than the
row, so a masked key slot >= L, a frame >= F or a pitch gap that is read and multiplied by zero
shows up as a NaN.  tests/test_parity_bounds.py has the CPU proof for these shapes and data."""
import ctypes

import pytest
import torch

import parity as P
from latentsync_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded_input(x, pitch):
    g = P.guarded(tuple(x.shape), pitch=pitch, dtype=BF, device=DEV)
    g.view.copy_(x.to(BF))
    return g


@pytest.mark.parametrize("L", P.XA_L)
def test_cross_attention_block(gpu, L):
    lib = _lib.load()
    C, hw, M = 320, P.XA_HW, P.XA_IMGS * P.XA_HW
    c = P.xattn_case(L)
    pk = ops.pack_cross_attention(c["wq"], c["gamma"], c["beta"], c["wo"], c["bo"], 8, DEV)
    gx, gkv = guarded_input(c["x"], 328), guarded_input(c["kv"], 648)
    gy = P.guarded((M, C), pitch=324, dtype=BF, device=DEV)
    gst = P.guarded((M, 2), dtype=F32, device=DEV)
    st = c["stats"].to(DEV)
    ins = [(t, P.snapshot(t)) for t in (gx.buf, gkv.buf, st, pk.wq, pk.bq, pk.wo, pk.bo)]
    d = _lib.XAttnDesc()
    d.x, d.ln_rowstats, d.wq, d.bq, d.kv, d.wo, d.bo = _p(gx.view), _p(st), _p(pk.wq), _p(pk.bq), _p(gkv.view), \
        _p(pk.wo), _p(pk.bo)
    d.y, d.stats_out = _p(gy.view), _p(gst.view)
    d.M, d.ldx, d.ldy, d.ldkv, d.C, d.heads, d.L, d.hw, d.eps = M, 328, 324, 648, C, 8, L, hw, 1e-5
    _lib.check(lib.ls_cross_attention_block(ctypes.byref(d), _stream()), "ls_cross_attention_block")
    torch.cuda.synchronize()
    name = f"cross_attention_block L {L}"
    P.assert_guard_intact(gy, f"{name} y")
    P.assert_guard_intact(gst, f"{name} stats_out")
    for i, (t, s) in enumerate(ins):
        P.assert_unchanged(t, s, f"{name} input {i}")
    ref, bound = P.xattn_bound(c["x"], c["stats"], c["wqr"], c["bqf"], c["bq_mag"], c["kv"], L, hw, c["wor"], c["bo"])
    worst = P.assert_elementwise(gy.view, ref, bound, where=dict(rows=16, cols=16), name=f"{name} y")
    ws = P.assert_elementwise(gst.view, *P.stored_row_stats_bound(gy.view.float().cpu(), 1e-5), where=dict(rows=16, cols=2),
                              name=f"{name} stats_out")
    print(f"{name}: worst err/bound y {worst:.3f}, stats_out {ws:.3f}")


@pytest.mark.parametrize("C,S", P.TA_CASES)
@pytest.mark.parametrize("Fr", P.TA_F)
def test_temporal_attention(gpu, C, S, Fr):
    lib = _lib.load()
    B = P.TA_SAMPLES
    c = P.tattn_case(C, S, Fr)
    pk = ops.pack_temporal(c["wq"], c["wk"], c["wv"], c["gamma"], c["beta"], c["pe"], 8, DEV)
    rows = B * Fr * S
    gx = guarded_input(c["x"], C + 8)
    go = P.guarded((rows, C), pitch=C + 8, dtype=BF, device=DEV)
    ins = [(t, P.snapshot(t)) for t in (gx.buf, pk.w, pk.gamma, pk.bpe)]
    d = _lib.TAttnDesc()
    d.x, d.ldx, d.gamma, d.bpe, d.w = _p(gx.view), C + 8, _p(pk.gamma), _p(pk.bpe), _p(pk.w)
    d.o, d.ldo = _p(go.view), C + 8
    d.C, d.heads, d.n_samples, d.F, d.S, d.eps = C, 8, B, Fr, S, 1e-5
    _lib.check(lib.ls_temporal_attention(ctypes.byref(d), _stream()), "ls_temporal_attention")
    torch.cuda.synchronize()
    name = f"temporal_attention C {C} F {Fr}"
    P.assert_guard_intact(go, name)
    for i, (t, s) in enumerate(ins):
        P.assert_unchanged(t, s, f"{name} input {i}")
    ref, bound = P.tattn_bound(c["x"], c["gamma"], c["bpe"], c["wqp"], c["wkr"], c["wvr"], B, Fr, S, 8, 1e-5)
    worst = P.assert_elementwise(go.view, ref, bound, where=dict(rows=S, cols=C // 8), name=name)
    print(f"{name}: worst err/bound {worst:.3f}")
