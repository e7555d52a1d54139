"""ls_feedforward and ls_ff_chain (ls_ff.hip) per element.  The fp64 reference is built from the
LOGICAL tensors (W1 with gamma folded and rounded once as unet._Dev.packed_ln does, b1 + W1 beta,
W2, to_out, proj_out) and never touches a packed layout, so an error in packing.pack_ff_w2,
permute_k_acc or geglu_interleave is caught like one in the kernel.  The bound is composed stage
by stage (parity.ff_bound, parity.ff_chain_bound); needle columns (inner columns of W2 and
k-columns of W1 scaled by 8, parity.FF_W2_NEEDLES / FF_W1_NEEDLES) sit at the chunk and tile
edges.  Outputs and activation inputs live in NaN guard bands with pitches wider than the row;
tests/test_parity_bounds.py has the CPU proof for these shapes and data."""
import ctypes

import pytest
import torch

import parity as P
from latentsync_amd import _lib, ops
from latentsync_amd.packing import pack_ff_w2
from latentsync_amd.unet import _Dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
C, INNER = P.FF_C, P.FF_INNER
LS_ERR_INVALID = 1


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded_input(x, pitch):
    g = P.guarded(tuple(x.shape), pitch=pitch, dtype=BF, device=DEV)
    g.view.copy_(x.to(BF))
    return g


def pack_ff(c):
    """(ff1, ff2 bias, w2 packed) on the device from the logical tensors, the model's way."""
    dv = _Dev({"w2": c["w2"], "b2": c["b2"]}, DEV)
    ff1 = dv.packed_ln(c["w1"], c["b1"], (c["gamma"], c["beta"]), geglu=True)
    ff2 = dv.packed("w2", "b2")
    return ff1, ff2, pack_ff_w2(c["w2"]).to(BF).to(DEV)


def ff_desc(gx, st, ff1, ff2, w2p, gy, M, ldx, ldy):
    d = _lib.FFDesc()
    d.x, d.ln_rowstats, d.w1, d.b1 = _p(gx.view), _p(st), _p(ff1.w), _p(ff1.bias)
    d.w2, d.b2, d.y = _p(w2p), _p(ff2.bias), _p(gy.view)
    d.M, d.ldx, d.ldy, d.C, d.inner = M, ldx, ldy, C, INNER
    return d


@pytest.mark.parametrize("M", P.FF_M)
def test_feedforward(gpu, M):
    lib = _lib.load()
    c = P.ff_case(M)
    ff1, ff2, w2p = pack_ff(c)
    gx, gy = guarded_input(c["x"], 328), P.guarded((M, C), pitch=324, dtype=BF, device=DEV)
    st = c["stats"].to(DEV)
    ins = [(t, P.snapshot(t)) for t in (gx.buf, st, ff1.w, ff1.bias, w2p, ff2.bias)]
    d = ff_desc(gx, st, ff1, ff2, w2p, gy, M, 328, 324)
    _lib.check(lib.ls_feedforward(ctypes.byref(d), _stream()), "ls_feedforward")
    torch.cuda.synchronize()
    name = f"feedforward M {M}"
    P.assert_guard_intact(gy, name)
    for i, (t, s) in enumerate(ins):
        P.assert_unchanged(t, s, f"{name} input {i}")
    ref, bound = P.ff_bound(c["x"], c["stats"], c["w1g"], c["b1f"], c["b1_mag"], c["w2r"], c["b2"])
    worst = P.assert_elementwise(gy.view, ref, bound, where=dict(rows=16, cols=16), name=name)
    print(f"{name}: worst err/bound {worst:.3f}")


def chain_setup(M):
    c = P.ff_chain_case(M)
    dv = _Dev({k: c[k] for k in ("wo", "bo", "w2", "b2", "wp", "bp")}, DEV)
    ff1 = dv.packed_ln(c["w1"], c["b1"], (c["gamma"], c["beta"]), geglu=True)
    pk = ops.pack_ff_chain(dv.packed("wo", "bo"), ff1, dv.packed("w2", "b2"), dv.packed("wp", "bp"))
    g = dict(o=guarded_input(c["o"], 328), h1=guarded_input(c["h1"], 324), xb=guarded_input(c["xb"], 332),
             z=P.guarded((M, C), pitch=336, dtype=BF, device=DEV),
             cs=P.guarded((M // 128, 2, C), dtype=F32, device=DEV))
    d = _lib.FFChainDesc()
    d.o, d.wo, d.bo, d.h1 = _p(g["o"].view), _p(pk.wo), _p(pk.bo), _p(g["h1"].view)
    d.w1, d.b1, d.w2, d.b2, d.wp, d.bp = _p(pk.w1), _p(pk.b1), _p(pk.w2), _p(pk.b2), _p(pk.wp), _p(pk.bp)
    d.xb, d.z, d.cs_out = _p(g["xb"].view), _p(g["z"].view), _p(g["cs"].view)
    d.M, d.ldo, d.ldh, d.ldxb, d.ldz, d.C, d.inner, d.eps = M, 328, 324, 332, 336, C, INNER, 1e-5
    return c, pk, g, d


@pytest.mark.parametrize("fmr", [1])  # 16 rows per wave, the only form
@pytest.mark.parametrize("M", P.FF_CHAIN_M)
def test_ff_chain(gpu, M, fmr):
    lib = _lib.load()
    c, pk, g, d = chain_setup(M)
    ins = [(t, P.snapshot(t)) for t in (g["o"].buf, g["h1"].buf, g["xb"].buf, pk.wo, pk.w1, pk.w2, pk.wp, pk.b1)]
    _lib.check(lib.ls_ff_chain(ctypes.byref(d), _stream()), "ls_ff_chain")
    torch.cuda.synchronize()
    name = f"ff_chain M {M} fmr {fmr}"
    P.assert_guard_intact(g["z"], f"{name} z")
    P.assert_guard_intact(g["cs"], f"{name} cs_out")
    for i, (t, s) in enumerate(ins):
        P.assert_unchanged(t, s, f"{name} input {i}")
    ref, bound = P.ff_chain_bound(c["o"], c["h1"], c["xb"], c["wor"], c["bo"], c["w1g"], c["b1f"], c["b1_mag"],
                                  c["w2r"], c["b2"], c["wpr"], c["bp"], 1e-5)
    worst = P.assert_elementwise(g["z"].view, ref, bound, where=dict(rows=16, cols=16), name=f"{name} z")
    wcs = P.assert_elementwise(g["cs"].view, *P.colsum_bound(g["z"].view.float().cpu()), where=dict(rows=1, cols=4),
                               name=f"{name} cs_out")
    print(f"{name}: worst err/bound z {worst:.3f}, cs_out {wcs:.4f}")


def test_feedforward_argument_checks(gpu):
    """Every fail(LS_ERR_INVALID ...) branch of ls_feedforward returns its status before anything
    is launched: the guarded output keeps its sentinel in every element."""
    lib = _lib.load()
    M = 129
    c = P.ff_case(M)
    ff1, ff2, w2p = pack_ff(c)
    gx, gy = guarded_input(c["x"], 328), P.guarded((M, C), pitch=324, dtype=BF, device=DEV)
    st = c["stats"].to(DEV)
    bad = [("x", None), ("ln_rowstats", None), ("w1", None), ("b1", None), ("w2", None), ("b2", None),  # null pointer
           ("C", 640), ("inner", 2560),                                                                   # shape
           ("M", 0), ("ldx", 312), ("ldy", 316), ("ldx", 324), ("ldy", 326),                              # rows / pitches
           ("x", _p(gx.view) + 2), ("w1", _p(ff1.w) + 8), ("w2", _p(w2p) + 4), ("b1", _p(ff1.bias) + 4),  # alignment
           ("b2", _p(ff2.bias) + 8), ("y", _p(gy.view) + 2), ("ln_rowstats", _p(st) + 4),
           ("M", 128 * 2 ** 31)]                                                                          # too many rows
    for field, value in bad:
        d = ff_desc(gx, st, ff1, ff2, w2p, gy, M, 328, 324)
        setattr(d, field, value)
        assert lib.ls_feedforward(ctypes.byref(d), _stream()) == LS_ERR_INVALID, (field, value)
    assert lib.ls_feedforward(None, _stream()) == LS_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((gy.buf.view(torch.int16) == 0x7FC1).all()), "a rejected call wrote to y"


def test_ff_chain_argument_checks(gpu):
    lib = _lib.load()
    c, pk, g, d0 = chain_setup(128)
    ptrs = ("o", "wo", "bo", "h1", "w1", "b1", "w2", "b2", "wp", "bp", "xb")
    bad = [(f, None) for f in ptrs]                                                        # null pointer
    bad += [("C", 640), ("inner", 2560)]                                                   # shape
    bad += [("M", 0), ("M", 127), ("M", 128 * 2 ** 31)]                                    # rows
    bad += [("ldo", 312), ("ldh", 316), ("ldxb", 316), ("ldz", 312), ("ldo", 324), ("ldh", 322), ("ldxb", 326),
            ("ldz", 324)]                                                                  # pitches
    bad += [(f, getattr(d0, f) + 8) for f in ("o", "wo", "w1", "w2", "wp", "b1", "b2", "bo", "bp", "z", "cs_out")]
    bad += [(f, getattr(d0, f) + 4) for f in ("h1", "xb")]                                 # alignment
    for field, value in bad:
        d = _lib.FFChainDesc.from_buffer_copy(d0)
        setattr(d, field, value)
        assert lib.ls_ff_chain(ctypes.byref(d), _stream()) == LS_ERR_INVALID, (field, value)
    assert lib.ls_ff_chain(None, _stream()) == LS_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((g["z"].buf.view(torch.int16) == 0x7FC1).all()), "a rejected call wrote to z"
    assert bool((g["cs"].buf.view(torch.int32) == 0x7FC0A5A5).all()), "a rejected call wrote to cs_out"
