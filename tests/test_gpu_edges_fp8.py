"""ls_attention_fp8 (vt8_quant_kernel + attn8_kernel, ls_attn.hip) per element, at the edges of
its 128-query block, 128-key tile, 64-key halves and depth-2 LDS ring: the bound of
tests/parity.py attn_fp8_bound against the fp64 softmax, `o` and the V^T workspace inside
sentinel guard bands, the inputs bit for bit unchanged, and the workspace bit for bit equal to
oracle.fp8_cpu.quant_vt -- the zero codes of the keys past nk, the 0x38 sum row and the zero rows
above it included.  tests/test_parity_bounds.py walks every case on the CPU (a tile-order
emulation passes the bound, planted defects leave it); tests/test_gpu_fp8.py keeps the large
shapes (2^31 offsets, long key sets) under its Frobenius ratios."""
import math

import pytest
import torch

import parity as P
from latentsync_amd import ops
from oracle import fp8_cpu as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def guarded_workspace(batch, heads, nk, d):
    n = ops.attention_fp8_workspace_bytes(batch=batch, heads=heads, nk=nk, head_dim=d)
    return P.guarded((1, n), dtype=torch.uint8, device=DEV)


def check_workspace(ws, v, name):
    """v (batch, heads, nk, d) bf16 values; ws the guarded workspace after the call."""
    P.assert_guard_intact(ws, f"{name} workspace")
    batch, heads, nk, d = v.shape
    codes, e8 = Q.decode_workspace(ws.view.reshape(-1).cpu(), batch * heads, nk, d)
    for b in range(batch):
        for h in range(heads):
            c_ref, e_ref = Q.quant_vt(v[b, h])  # the keys past nk of the last tile: zero codes
            p = b * heads + h
            assert torch.equal(e8[p, :, :d], e_ref), (name, b, h)
            assert torch.equal(codes[p, :, :d], c_ref), (name, b, h, int((codes[p, :, :d] != c_ref).sum()))
            assert bool((codes[p, :, d] == 0x38).all()) and bool((e8[p, :, d:] == 127).all()), (name, b, h)
            assert bool((codes[p, :, d + 1:] == 0).all()), (name, b, h)


def check_output(name, g, got, q, k, v, ws, snaps):
    """got (batch, heads, nq, d) fp32 on the CPU, read from the guarded output g."""
    d = q.shape[-1]
    ref, bound = P.attn_fp8_bound(q, k, v, 1 / math.sqrt(d))
    worst = P.assert_elementwise(got, ref, bound, where=dict(rows=16, cols=16), name=name)
    P.assert_guard_intact(g, name)
    for i, (t, s) in enumerate(snaps):
        P.assert_unchanged(t, s, f"{name} input {i}")
    check_workspace(ws, v, name)
    print(f"fp8 {name}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("name,d,batch,heads,nq,nk,kind", P.FP8_CASES, ids=[c[0] for c in P.FP8_CASES])
def test_attention_fp8_edges(gpu, name, d, batch, heads, nq, nk, kind):
    """q / k / v rows [batch][n][heads * d], o rows of pitch heads * d + 8 inside the guard band."""
    q, k, v = P.fp8_qkv(d, batch, heads, nq, nk, kind)
    C = heads * d
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(batch, t.shape[2], C).to(BF).to(DEV).contiguous()
    qd, kd, vd = rows(q), rows(k), rows(v)
    pitch = C + 8
    g = P.guarded((batch, nq, C), pitch=pitch, dtype=BF, device=DEV)
    ws = guarded_workspace(batch, heads, nk, d)
    snaps = [(t, P.snapshot(t)) for t in (qd, kd, vd)]
    ops.attention(qd, kd, vd, g.view, batch=batch, z2=1, heads=heads, nq=nq, nk=nk, head_dim=d,
                  qs=(nq * C, 0, C, d), ks=(nk * C, 0, C, d), vs=(nk * C, 0, C, d), os_=(nq * pitch, 0, pitch, d),
                  fp8=True, fp8_workspace=ws.view)
    torch.cuda.synchronize()
    got = g.view.float().cpu().reshape(batch, nq, heads, d).permute(0, 2, 1, 3)
    check_output(name, g, got, q, k, v, ws, snaps)


def test_attention_fp8_fused_qkv_view_edges(gpu):
    """The UNet's call at N = 130: q, k, v as column slices of one q|k|v buffer (row stride 3 C,
    k and v as column offsets), as in tests/test_gpu_fp8.py test_attention_fp8_fused_qkv_view."""
    batch, N, heads, d = 2, 130, 8, 40
    C = heads * d
    q, k, v = P.fp8_qkv(d, batch, heads, N, N, "needle")
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(batch * N, C)
    qkv = torch.cat([rows(q), rows(k), rows(v)], 1).to(BF).to(DEV).contiguous()
    pitch = C + 8
    g = P.guarded((batch, N, C), pitch=pitch, dtype=BF, device=DEV)
    ws = guarded_workspace(batch, heads, N, d)
    snaps = [(qkv, P.snapshot(qkv))]
    st = (N * 3 * C, 0, 3 * C, d)
    ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], g.view, batch=batch, z2=1, heads=heads, nq=N, nk=N, head_dim=d,
                  qs=st, ks=st, vs=st, os_=(N * pitch, 0, pitch, d), fp8=True, fp8_workspace=ws.view)
    torch.cuda.synchronize()
    got = g.view.float().cpu().reshape(batch, N, heads, d).permute(0, 2, 1, 3)
    check_output("fused q|k|v 130x130 d40", g, got, q, k, v, ws, snaps)


def test_attention_fp8_temporal_strides(gpu):
    """z2 = 2 with the "(b f) s c -> (b s) f c" strides of tests/test_gpu_edges_attn.py
    test_attention_seqm_temporal: memory rows (bb, f, s), logical batch index bb * S + s."""
    Bb, S, heads, d, n = 2, 2, 2, 80, 130
    C = heads * d
    q, k, v = P.fp8_qkv(d, Bb * S, heads, n, n, "needle")
    mem = lambda t: t.reshape(Bb, S, heads, n, d).permute(0, 3, 1, 2, 4).reshape(Bb * n * S, C).to(BF).to(DEV).contiguous()
    qd, kd, vd = mem(q), mem(k), mem(v)
    pitch = C + 8
    g = P.guarded((Bb * n * S, C), pitch=pitch, dtype=BF, device=DEV)
    ws = guarded_workspace(Bb * S, heads, n, d)
    snaps = [(t, P.snapshot(t)) for t in (qd, kd, vd)]
    st = (n * S * C, C, S * C, d)
    ops.attention(qd, kd, vd, g.view, batch=Bb * S, z2=S, heads=heads, nq=n, nk=n, head_dim=d, qs=st, ks=st, vs=st,
                  os_=(n * S * pitch, pitch, S * pitch, d), fp8=True, fp8_workspace=ws.view)
    torch.cuda.synchronize()
    got = g.view.float().cpu().reshape(Bb, n, S, heads, d).permute(0, 2, 3, 1, 4).reshape(Bb * S, heads, n, d)
    check_output("temporal z2 = 2 130x130 d80", g, got, q, k, v, ws, snaps)


def test_attention_fp8_rejects_4_byte_output_pitch(gpu):
    """attn8_kernel stores 8 bytes at orow + d: an o pitch of C + 2 elements (4-byte aligned rows)
    is refused with LS_ERR_INVALID (status 1) before anything is launched -- o, its guard band and
    the workspace keep their sentinels."""
    batch, heads, nq, nk, d = 1, 2, 17, 77, 40
    C = heads * d
    q, k, v = P.fp8_qkv(d, batch, heads, nq, nk, "needle")
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(batch, t.shape[2], C).to(BF).to(DEV).contiguous()
    qd, kd, vd = rows(q), rows(k), rows(v)
    ws = guarded_workspace(batch, heads, nk, d)
    for name, pitch, sh in (("o_si", C + 2, d), ("o_sh", C + 8, d + 2)):
        g = P.guarded((batch, nq, C), pitch=pitch, dtype=BF, device=DEV)
        assert g.view.data_ptr() % 8 == 0  # the pointer itself passes: the stride is what is refused
        with pytest.raises(RuntimeError, match=r"status 1\).*o rows 8-B"):
            ops.attention(qd, kd, vd, g.view, batch=batch, z2=1, heads=heads, nq=nq, nk=nk, head_dim=d,
                          qs=(nq * C, 0, C, d), ks=(nk * C, 0, C, d), vs=(nk * C, 0, C, d), os_=(nq * pitch, 0, pitch, sh),
                          fp8=True, fp8_workspace=ws.view)
        torch.cuda.synchronize()
        for t in (g, ws):
            assert bool((t.buf.view(t.bits_dtype).cpu().to(torch.int64) & 0xFFFF == t.sentinel & 0xFFFF).all()), name
