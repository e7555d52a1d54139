"""ls_attention, one case per dispatch branch, per element: needle inputs (a tile-boundary
key carries most of a row's weight, so one dropped key or a row sum without it shows),
the bound of tests/parity.py attn_bound, and `o` inside a sentinel guard band.

Which kernel a case reaches is read from the dispatch in ls_attention (ls_attn.hip):
  nq == nk <= 16, heads packed, 16-B aligned, d in {40, 80, 160}, heads 8 -> attn_seqm_kernel
  nk > 32, d % 8 == 0, d <= 160: d == 40 and nk > 128 -> attn5_kernel, else attn3_kernel
      (nk <= 64: its single-tile ONE form; d picks the <KC, ND> instance)
  d == 512, 16-B aligned rows -> attnw_kernel (launch_attnw512)
  everything else -> attn_kernel<DPV, NKF>: NKF 2 for nk <= 32 ("generic small"), 4 otherwise;
      DPV = d rounded up to 64 / 96 / 160 / 256 / 512; d % 8 != 0 takes its load_partial path
attn3 / attn5 / attnw multiply Q by scale log2(e) and round it to bf16 again (q_prescaled in
attn_bound); attn_kernel and attn_seqm_kernel scale the fp32 score."""
import math

import pytest
import torch

import parity as P
from latentsync_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def run_case(name, d, heads, nq, nk, pre, offset=0, batch=2):
    """q / k / v rows [batch][n][heads * d] (fused-projection style), o rows of pitch
    heads * d + 8 inside the guard band."""
    q, k, v = P.needle_qkv(batch, heads, nq, nk, d, seed=21)
    C = heads * d
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(batch, t.shape[2], C).to(BF).to(DEV).contiguous()
    qd, kd, vd = rows(q), rows(k), rows(v)
    pitch = C + 8
    g = P.guarded((batch, nq, C), pitch=pitch, dtype=BF, device=DEV, offset=offset)
    snaps = [(t, P.snapshot(t)) for t in (qd, kd, vd)]
    ops.attention(qd, kd, vd, g.view, batch=batch, z2=1, heads=heads, nq=nq, nk=nk, head_dim=d,
                  qs=(nq * C, 0, C, d), ks=(nk * C, 0, C, d), vs=(nk * C, 0, C, d), os_=(nq * pitch, 0, pitch, d))
    torch.cuda.synchronize()
    scale = 1 / math.sqrt(d)
    ref, bound = P.attn_bound(q, k, v, scale, q_prescaled=pre)
    got = g.view.float().cpu().reshape(batch, nq, heads, d).permute(0, 2, 1, 3)
    worst = P.assert_elementwise(got, ref, bound, where=dict(rows=16, cols=16), name=name)
    P.assert_guard_intact(g, name)
    for i, (t, s) in enumerate(snaps):
        P.assert_unchanged(t, s, f"{name} input {i}")
    print(f"{name} offset {offset}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("name,d,heads,nq,nk,pre", P.ATTN_CASES, ids=[c[0] for c in P.ATTN_CASES])
def test_attention_branch(gpu, name, d, heads, nq, nk, pre):
    run_case(name, d, heads, nq, nk, pre)


@pytest.mark.parametrize("name", ["attn3_d64_17x77", "generic_d40_65x7"])
def test_attention_unaligned_output(gpu, name):
    """o shifted by 2 elements (4 bytes): a.o16 is false, attn3 takes its 8-byte / scalar
    store fallback instead of the 16-byte lane-swapped stores."""
    case = next(c for c in P.ATTN_CASES if c[0] == name)
    run_case(*case, offset=2)


@pytest.mark.parametrize("d,n", P.SEQM_CASES)
def test_attention_seqm_temporal(gpu, d, n):
    """attn_seqm_kernel (d = 40 all heads in a block, d = 80 / 160 heads split over two
    blocks) with the temporal "(b f) s c -> (b s) f c" strides: z2 = S > 1."""
    Bb, S, heads = 2, 3, 8
    C = heads * d
    q, k, v = P.needle_qkv(Bb * S, heads, n, n, d, seed=22)  # logical batch index bb * S + s
    # memory rows (bb, f, s) of C channels
    mem = lambda t: t.reshape(Bb, S, heads, n, d).permute(0, 3, 1, 2, 4).reshape(Bb * n * S, C).to(BF).to(DEV).contiguous()
    qd, kd, vd = mem(q), mem(k), mem(v)
    pitch = C + 8
    g = P.guarded((Bb * n * S, C), pitch=pitch, dtype=BF, device=DEV)
    snaps = [(t, P.snapshot(t)) for t in (qd, kd, vd)]
    st = (n * S * C, C, S * C, d)
    ops.attention(qd, kd, vd, g.view, batch=Bb * S, z2=S, heads=heads, nq=n, nk=n, head_dim=d, qs=st, ks=st, vs=st,
                  os_=(n * S * pitch, pitch, S * pitch, d))
    torch.cuda.synchronize()
    ref, bound = P.attn_bound(q, k, v, 1 / math.sqrt(d), q_prescaled=False)
    got = g.view.float().cpu().reshape(Bb, n, S, heads, d).permute(0, 2, 3, 1, 4).reshape(Bb * S, heads, n, d)
    name = f"seqm d {d} n {n}"
    worst = P.assert_elementwise(got, ref, bound, where=dict(rows=16, cols=16), name=name)
    P.assert_guard_intact(g, name)
    for i, (t, s) in enumerate(snaps):
        P.assert_unchanged(t, s, f"{name} input {i}")
    print(f"{name}: worst err/bound {worst:.3f}")
