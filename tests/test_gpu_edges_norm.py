"""ls_norm.hip (and ls_gn_colsum of ls_conv.hip) per element: every entry point is called through
the C ABI so that its outputs sit in sentinel guard bands (bf16 outputs in the bf16 NaN, scale /
shift / statistics in the fp32 NaN), its activation inputs sit in guarded buffers too -- NaN rows
behind the last valid row and NaNs in every pitch gap, so a read past the input shows up in the
output -- and every element is held to the bound tests/parity.py derives from the kernel's
arithmetic.  tests/test_parity_bounds.py proves on the CPU, for these very shapes, that the
kernels' arithmetic passes the bounds and that planted defects do not.

Which kernel a case reaches is read from the launchers in ls_norm.hip:
  ls_layernorm / ls_row_stats: layernorm_kernel<NCH>, NCH from cdiv(C / 8, 16) rounded up to
      one of 1, 2, 3, 5, 8, 10, 12, 16 (parity.LN_C has one C per instance);
  ls_groupnorm: gn_stats_kernel on a (gn_nsplit, n_samples) grid; C / 8 > 256 -> nchunk > 1,
      groups > 32 -> L = 4 lanes per group;
  ls_groupnorm_apply: gn_apply_u_kernel<4> when ppb = 256 / (C / 8) >= 2 and 4 ppb <= pps,
      else the grid-stride gn_apply_kernel."""
import pytest
import torch

import parity as P
from latentsync_amd import _lib
from latentsync_amd._lib import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded_input(x, pitch=None):
    """x (rows, cols) fp32 values -> a bf16 device view of that pitch inside a NaN-filled buffer."""
    g = P.guarded(tuple(x.shape), pitch=pitch, dtype=BF, device=DEV)
    g.view.copy_(x.to(BF))
    return g


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def finish(outs, ins, name):
    torch.cuda.synchronize()
    for i, g in enumerate(outs):
        P.assert_guard_intact(g, f"{name} output {i}")
    for i, (t, s) in enumerate(ins):
        P.assert_unchanged(t, s, f"{name} input {i}")


# ---------------------------------------------------------------- LayerNorm, row statistics
@pytest.mark.parametrize("C", P.LN_C)
@pytest.mark.parametrize("mean_sigmas", [0, 30])
@pytest.mark.parametrize("with_pe", [False, True])
def test_layernorm(gpu, C, mean_sigmas, with_pe):
    lib = _lib.load()
    worst = 0.0
    for rows in P.LN_ROWS:
        x, gamma, beta, pe = P.ln_case(rows, C, mean_sigmas)
        gx = guarded_input(x, pitch=C + 8)
        gd, bd, ped = dev(gamma), dev(beta), dev(pe) if with_pe else None
        gy = P.guarded((rows, C), dtype=BF, device=DEV)  # (y has no pitch in the ABI: dense rows)
        ins = [(t, P.snapshot(t)) for t in (gx.buf, gd, bd) + ((ped,) if with_pe else ())]
        check(lib.ls_layernorm(_p(gx.view), C + 8, rows, C, P.LN_EPS, _p(gd), _p(bd), _p(ped), P.LN_PE_RPF,
                               P.LN_PE_FRAMES, _p(gy.view), _stream()), "ls_layernorm")
        name = f"layernorm C {C} rows {rows} mean {mean_sigmas} pe {with_pe}"
        finish([gy], ins, name)
        ref, bound = P.ln_bound(x, gamma, beta, P.ln_pe_rows(pe, rows) if with_pe else None, P.LN_EPS, BF)
        worst = max(worst, P.assert_elementwise(gy.view, ref, bound, where=dict(rows=16, cols=128), name=name))
    print(f"layernorm C {C} mean {mean_sigmas} pe {with_pe}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("C", P.LN_C)
@pytest.mark.parametrize("mean_sigmas", [0, 30])
def test_row_stats(gpu, C, mean_sigmas):
    lib = _lib.load()
    worst = 0.0
    for rows in P.LN_ROWS:
        x, _, _, _ = P.ln_case(rows, C, mean_sigmas)
        gx = guarded_input(x, pitch=C + 8)
        gs = P.guarded((rows, 2), dtype=F32, device=DEV)
        ins = [(gx.buf, P.snapshot(gx.buf))]
        check(lib.ls_row_stats(_p(gx.view), C + 8, rows, C, P.LN_EPS, _p(gs.view), _stream()), "ls_row_stats")
        name = f"row_stats C {C} rows {rows} mean {mean_sigmas}"
        finish([gs], ins, name)
        ref, bound = P.row_stats_bound(x, P.LN_EPS)
        worst = max(worst, P.assert_elementwise(gs.view, ref, bound, where=dict(rows=16, cols=2), name=name))
    print(f"row_stats C {C} mean {mean_sigmas}: worst err/bound {worst:.3f}")


# ---------------------------------------------------------------- GroupNorm statistics (read pass)
@pytest.mark.parametrize("name,C1,C2,groups,n_samples,pps", P.GN_CASES, ids=[c[0] for c in P.GN_CASES])
@pytest.mark.parametrize("mean_sigmas", P.GN_MEANS)
def test_groupnorm_stats(gpu, name, C1, C2, groups, n_samples, pps, mean_sigmas):
    lib = _lib.load()
    C = C1 + C2
    x, gamma, beta = P.gn_case(C1, C2, n_samples, pps, mean_sigmas)
    g1 = guarded_input(x[:, :, :C1].reshape(n_samples * pps, C1))
    g2 = guarded_input(x[:, :, C1:].reshape(n_samples * pps, C2)) if C2 else None
    gd, bd = dev(gamma), dev(beta)
    nbytes = lib.ls_groupnorm_workspace_bytes(n_samples, groups)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    ref, bound = P.gn_stats_bound(x, groups, P.GN_EPS, gamma, beta, P.gn_nsplit(n_samples, pps, C), P.gn_R(C))
    ins = [(t, P.snapshot(t)) for t in (g1.buf, gd, bd) + ((g2.buf,) if C2 else ())]
    worst = 0.0
    for run in (0, 1):  # the second call finds the tickets re-armed and the accumulators re-zeroed
        gsc = P.guarded((n_samples, C), dtype=F32, device=DEV)
        gsh = P.guarded((n_samples, C), dtype=F32, device=DEV)
        check(lib.ls_groupnorm(_p(g1.view), _p(g2.view) if C2 else None, C1, C2, n_samples, pps, groups, P.GN_EPS,
                               _p(gd), _p(bd), _p(gsc.view), _p(gsh.view), _p(ws), nbytes, _stream()), "ls_groupnorm")
        finish([gsc, gsh], ins, f"{name} run {run}")
        assert int(ws.count_nonzero()) == 0, f"{name} run {run}: the workspace is not back to zero"
        worst = max(worst, P.assert_elementwise(gsc.view, ref[0], bound[0], where=dict(rows=1, cols=C // groups),
                                                name=f"{name} run {run} scale"))
        worst = max(worst, P.assert_elementwise(gsh.view, ref[1], bound[1], where=dict(rows=1, cols=C // groups),
                                                name=f"{name} run {run} shift"))
    print(f"groupnorm {name} mean {mean_sigmas}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("cpg,slots,C1,C2", P.GN_COLSUM_CASES)
def test_groupnorm_colsum(gpu, cpg, slots, C1, C2):
    lib = _lib.load()
    cs1, cs2, gamma, beta = P.gn_colsum_case(cpg, slots, C1, C2)
    C = 32 * cpg
    d1, d2, gd, bd = dev(cs1), dev(cs2), dev(gamma), dev(beta)
    gsc = P.guarded((3, C), dtype=F32, device=DEV)
    gsh = P.guarded((3, C), dtype=F32, device=DEV)
    ins = [(t, P.snapshot(t)) for t in (d1, gd, bd) + ((d2,) if d2 is not None else ())]
    check(lib.ls_groupnorm_colsum(_p(d1), _p(d2), C1, C - C1, 3, slots * 128, 32, P.GN_EPS, _p(gd), _p(bd),
                                  _p(gsc.view), _p(gsh.view), _stream()), "ls_groupnorm_colsum")
    name = f"groupnorm_colsum cpg {cpg} slots {slots} C1 {C1}"
    finish([gsc, gsh], ins, name)
    cs = cs1 if cs2 is None else torch.cat([cs1, cs2], 2)
    ref, bound = P.gn_colsum_bound(cs, slots, 32, P.GN_EPS, gamma, beta)
    worst = P.assert_elementwise(gsc.view, ref[0], bound[0], where=dict(rows=1, cols=cpg), name=f"{name} scale")
    worst = max(worst, P.assert_elementwise(gsh.view, ref[1], bound[1], where=dict(rows=1, cols=cpg), name=f"{name} shift"))
    print(f"{name}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("M", [128, 384])
@pytest.mark.parametrize("N", [8, 40, 320])
def test_gn_colsum(gpu, M, N):
    lib = _lib.load()
    y = P.bf16_round(torch.randn(M, N, generator=torch.Generator().manual_seed(M + N)) + 2.0)
    gy = guarded_input(y, pitch=N + 8)
    go = P.guarded((M // 128, 2, N), dtype=F32, device=DEV)
    ins = [(gy.buf, P.snapshot(gy.buf))]
    check(lib.ls_gn_colsum(_p(gy.view), N + 8, M, N, _p(go.view), _stream()), "ls_gn_colsum")
    name = f"gn_colsum {M}x{N}"
    finish([go], ins, name)
    ref, bound = P.colsum_bound(y)
    worst = P.assert_elementwise(go.view, ref, bound, where=dict(rows=1, cols=8), name=name)
    print(f"{name}: worst err/bound {worst:.4f}")


# ---------------------------------------------------------------- GroupNorm apply
@pytest.mark.parametrize("name,C1,C2,S,pps", P.GN_APPLY_CASES, ids=[c[0] for c in P.GN_APPLY_CASES])
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_apply(gpu, name, C1, C2, S, pps, silu):
    """scale / shift are exactly (S, C) floats at the END of their guarded buffers' views, so
    the rows a thread without pixels would address (sample index S) are the NaN band: reading
    them is harmless to the output, which is why gn_apply_u_kernel's early return for such
    threads is verified by reading the kernel, not here."""
    lib = _lib.load()
    C = C1 + C2
    x, gamma, beta = P.gn_case(C1, C2, S, pps, 2)
    (sc, sh), _ = P.gn_stats_bound(x, 32, P.GN_EPS, gamma, beta, 1, 1)
    sc, sh = sc.float(), sh.float()
    g1 = guarded_input(x[:, :, :C1].reshape(S * pps, C1))
    g2 = guarded_input(x[:, :, C1:].reshape(S * pps, C2)) if C2 else None
    gsc = P.guarded((S, C), dtype=F32, device=DEV)
    gsh = P.guarded((S, C), dtype=F32, device=DEV)
    gsc.view.copy_(sc)
    gsh.view.copy_(sh)
    gy = P.guarded((S * pps, C), dtype=BF, device=DEV)
    ins = [(g.buf, P.snapshot(g.buf)) for g in (g1, gsc, gsh) + ((g2,) if C2 else ())]
    check(lib.ls_groupnorm_apply(_p(g1.view), _p(g2.view) if C2 else None, C1, C2, S * pps, pps, _p(gsc.view),
                                 _p(gsh.view), int(silu), _p(gy.view), _stream()), "ls_groupnorm_apply")
    finish([gy], ins, name)
    ref, bound = P.gn_apply_bound(x, sc, sh, silu)
    worst = P.assert_elementwise(gy.view, ref.reshape(S * pps, C), bound.reshape(S * pps, C),
                                 where=dict(rows=max(1, 256 // (C // 8)), cols=8), name=name)
    print(f"groupnorm_apply {name} silu {silu}: worst err/bound {worst:.3f}")
