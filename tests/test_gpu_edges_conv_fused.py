"""The fused features of ls_conv2d per element (tests/parity.py): the LayerNorm fold in both
of its arithmetics (the row-block kernel's normalised A rows, the tiled kernels' epilogue fold),
the row-block GEMM in every compiled instance and in its steady state, row statistics out
(row_stats_out), GroupNorm column sums out (gn_colsum_out) from every producer and per slot,
the GroupNorm affine folded into the row-block A rows, and the ragged grouped raster.

The harness is that of test_gpu_edges_gemm.py: fp64 references on the operands handed to the
kernel, bounds derived from the arithmetic, every output (y, stats_out, the column-sum buffer)
inside a sentinel guard band, output pitches above N, A read from a wider buffer (ld1 = K + 8),
inputs checked unchanged, the worst err/bound ratio printed.  Every case first reads
ops.conv_plan and asserts the family, instance and trailing passes it was written for, so a
planner change cannot empty a test silently.

Read before the first run (rowblock_ok, halo_ok, cs_tile_fits): the row-block cases have K = Cin
in {320, 640}, M % 256 == 0 (% 128 at one fragment per wave), N % 64 == 0, 16-byte aligned
operands, ldy % 4 == 0, ldr % 8 == 0, rowvec_ld % 4 == 0 and rows_per_vec % 256 == 0; samples of
the affine are 256 (K 320) / 128 (K 640) rows; the halo cases are 16 x 16 / 32 x 16 images with
Cin % 64 == 0; the column-sum buffer is (M / 128, 2, N) with M % 128 == 0 and N % 8 == 0."""
import functools
import math

import pytest
import torch

import parity as P
import test_gpu_edges_gemm as E
from latentsync_amd import _lib, ops
from latentsync_amd.packing import pack_phase_weight

pytestmark = pytest.mark.gpu
DEV, BF, F32 = "cuda", torch.bfloat16, torch.float32
EPS = 1e-5
WS = 64 << 20  # the split-K workspace named in the plan query and the call alike: one plan

RB_LN, RB_RES, RB_RV, RB_GEGLU, RB_STATS, RB_GNCS, RB_AFF = 1, 2, 4, 8, 16, 32, 64
# RowblockInstances of ls_conv_rowblock.hip: a flag set added there gains its cases here
RB_FLAG_SETS = (0, RB_LN, RB_LN | RB_RV, RB_RES, RB_LN | RB_RES, RB_LN | RB_GEGLU, RB_GEGLU, RB_STATS, RB_RES | RB_STATS,
                RB_RES | RB_GNCS, RB_AFF, RB_AFF | RB_STATS)
RB_FM1 = RB_STATS | RB_GNCS | RB_AFF  # one fragment per wave only
# ... at K 640 also with a residual: <20, 2> with RB_RES needs 170 KB of LDS, and every launch of it
# was refused (this file's first run: "gemm_rowblock_kernel: invalid argument" under tuning keys 20
# and 15); the planner now gives such a call <20, 1>, and the two instances are no longer compiled
RB_FM1_K640 = RB_FM1 | RB_RES
RB_INSTANCES = {(kt, fm, f) for f in RB_FLAG_SETS for kt, fm in ((10, 2), (20, 1), (20, 2))
                if (kt, fm) != (20, 2) or not f & RB_FM1_K640}
SEEN = set()  # (rb_kt, rb_fm, rb_flags) of every row-block plan sections a to c asserted
WORST = {}    # section -> worst err/bound


class tuning(E.tuning):
    """E.tuning that also knows keys 7 (K = 640 on the row-block kernel) and 20 (with a residual)."""
    DEFAULTS = {**E.tuning.DEFAULTS, 7: 1, 20: 0}


def geglu_logical(t):
    """Rows in packing.geglu_interleave's order (16 h rows, 16 g rows, ...) -> [h; g]."""
    n2 = t.shape[0] // 2
    return t.reshape(n2 // 16, 2, 16, *t.shape[1:]).transpose(0, 1).reshape(t.shape)


def note(section, *ratios):
    WORST[section] = max([WORST.get(section, 0.0)] + [r for r in ratios if r is not None])


@functools.lru_cache(maxsize=4)
def operands(M, K, N, ln, seed):
    """bf16-rounded x (M, K) (P.ln_case rows at `ln` mean_sigmas with their fp32 statistics, or
    plain random rows), the packed bf16 weight (N, K) in logical order (sparse: see
    parity.sparse_weight, the bound stays a few bf16 steps wide) and an fp32 bias."""
    if ln is None:
        x, st = P.bf16_round(E.rnd(M, K, seed=seed + M + K)), None
    else:
        x = P.ln_case(M, K, ln, seed)[0]
        st = P.host_row_stats(x, EPS)
    w = P.bf16_round(P.sparse_weight(N, K, 8, seed + N + K))
    return x, st, w, E.rnd(N, seed=seed + N + 2, scale=0.1)


def run_linear(name, M, K, N, *, ln=None, geglu=False, res=False, rowvec=None, out_scale=1.0, aff=None, stats=False,
               gn=False, out_dtype=BF, split=0, form="rows", tune=None, expect=None, chunks=None, record=False, seed=0):
    """One ksize-1 call: plan asserted, run, y / stats_out / column sums checked per element.
    rowvec = (rows_per_vec, mod, ld); aff = (rows per sample, mean shift).  Returns the worst
    err/bound of (y, stats_out, column sums), None where not requested."""
    x, st, w, b = operands(M, K, N, ln, seed)
    n2 = N // 2
    n_out = n2 if geglu else N
    pw = E.packed(w, b, 1, geglu=geglu)
    colsum = None
    if ln is not None:
        cs_packed = pw.w.float().cpu().sum(1)  # fp32 row sums of the packed bf16 weight (unet._Dev.packed_ln)
        pw.colsum = cs_packed.to(DEV).contiguous()
        colsum = geglu_logical(cs_packed) if geglu else cs_packed
    pps = aff[0] if aff else M
    lead = (M // pps, 1, pps)  # (images, H, W): one sample of the affine per image
    xd = E.wide(x, K + 8)
    # no workspace unless the case asks for a split: with one the planner splits K on its own where
    # the grid is small (K 640 at M 384 takes split 2 on the tiled kernels, not the row-block one)
    kw, rows, r, sc, sh = dict(out_scale=out_scale, split_k=split, workspace_bytes=WS if split else 0), None, None, None, None
    if geglu:
        kw["act"] = ops.ACT_GEGLU
    if ln is not None:
        kw["ln_stats"] = st.to(DEV).contiguous()
    if res:
        r = P.bf16_round(E.rnd(M, n_out, seed=seed + 15))
        rd = E.wide(r, n_out + (16 if N % 8 else 8))
        kw["res"] = rd.unflatten(0, lead)
    if rowvec is not None:
        rpv, mod, ld = rowvec
        tv = E.rnd(mod if mod else -(-M // rpv), ld, seed=seed + 14)
        kw["rowvec"] = (tv.to(DEV), rpv, ld, mod)
        idx = torch.arange(M) // rpv
        rows = tv[(idx % mod) if mod else idx][:, :N]
    if aff is not None:
        S = M // pps
        sc, sh = 1 + 0.2 * E.rnd(S, K, seed=seed + 7), aff[1] + 0.3 * E.rnd(S, K, seed=seed + 8)
        kw["aff"] = (sc.to(DEV), sh.to(DEV), 1, False)
    g = P.guarded((M, n_out), pitch=n_out + 8, pad_rows=3, dtype=out_dtype, device=DEV)
    g_st = g_cs = None
    if stats:
        g_st = P.guarded((M, 2), pad_rows=8, dtype=F32, device=DEV)
        kw["stats_out"] = g_st.view
    if gn:
        g_cs = P.guarded((M // 128, 2, N), pad_rows=2, dtype=F32, device=DEV)
        kw["gn_out"] = g_cs.view
    inputs = E.snaps(xd, pw.w, pw.bias, pw.colsum, kw.get("ln_stats"), kw.get("res"),
                     kw["rowvec"][0] if rowvec is not None else None, *(kw["aff"][:2] if aff is not None else ()))
    x4, y4 = xd.unflatten(0, lead), g.view.unflatten(0, lead)
    with tuning(**(tune or {})):
        plan = ops.conv_plan(x4, pw, out=y4, **kw)
        assert plan is not None, f"{name}: {_lib.load().ls_last_error().decode()}"
        for k, v in (expect or {}).items():
            assert plan[k] == v, f"{name}: plan {k} = {plan[k]}, the case was written for {v} ({plan})"
        if chunks is not None:
            assert P.rb_chunk_counts(plan, N, M) == chunks, (name, P.rb_chunk_counts(plan, N, M))
        if record:
            assert plan["family"] == 1, (name, plan)
            SEEN.add((plan["rb_kt"], plan["rb_fm"], plan["rb_flags"]))
        ops.conv(x4, pw, out=y4, **kw)
    # ---- the fp64 reference and the bound of y
    pre_dtype = None if geglu else out_dtype
    if aff is not None:
        ref, mag, prod = E.conv_reference(x.reshape(*lead, K), None, w, b, 1, aff=(sc, sh, 1, False),
                                          res=None if r is None else r.reshape(*lead, N), out_scale=out_scale)
        ref, bound = ref.reshape(M, N), P.gemm_bound(ref, mag, K, pre_dtype, prologue=True, prod_mag=prod).reshape(M, N)
    elif ln is not None:
        ref, bound = P.ln_fold_bound(x, st, w, colsum, b, rowvec=rows, res=r, out_scale=out_scale, out_dtype=pre_dtype,
                                     form=form)
    else:
        ref, mag, _ = E.conv_reference(x[None, None], None, w, b, 1, rowvec=None if rowvec is None else (tv, rpv, mod),
                                       res=None if r is None else r[None, None], out_scale=out_scale)
        ref, bound = ref.reshape(M, N), P.gemm_bound(ref, mag, K, pre_dtype).reshape(M, N)
    if geglu:
        ref, bound = P.geglu_bound(ref[:, :n2], bound[:, :n2], ref[:, n2:], bound[:, n2:], out_dtype)
    wy = E.finish(name, g, ref, bound, inputs)
    # ---- statistics and column sums of the STORED output
    ys = g.view.float().cpu()
    ws = wc = None
    if stats:
        sref, sb = P.row_stats_bound(ys, EPS) if plan["row_stats"] else P.stored_row_stats_bound(ys, EPS, chain=8)
        ws = P.assert_elementwise(g_st.view, sref, sb, where=dict(rows=16, cols=2), name=name + " stats_out")
        P.assert_guard_intact(g_st, name + " stats_out")
    if gn:
        cref, cb = P.colsum_bound(ys)
        wc = P.assert_elementwise(g_cs.view, cref, cb, where=dict(rows=2, cols=16), name=name + " column sums")
        P.assert_guard_intact(g_cs, name + " column sums")
    return wy, ws, wc


def fmt(t):
    return " / ".join("-" if v is None else f"{v:.3f}" for v in t)


# ---------------------------------------------------------------- a. row-block: every instance, one chunk
RB_SHAPE = {(10, 2): (320, 512), (20, 1): (640, 384), (20, 2): (640, 512)}  # (KT, FM) -> (K, M)


def rb_request(flags, K, N):
    """What a caller asks for to get the flag set (where the planner can fuse it)."""
    return dict(ln=None, geglu=bool(flags & RB_GEGLU), res=bool(flags & RB_RES),
                rowvec=(256, 0, N + 8) if flags & RB_RV else None, stats=bool(flags & RB_STATS), gn=bool(flags & RB_GNCS),
                aff=((256 if K == 320 else 128), 0.5) if flags & RB_AFF else None)


def rb_tune(K, fm, res):
    return dict(k15=int(fm == 2), k20=int(bool(res) and K == 640)) if K == 640 else {}


CASES_A = [(f, kt, fm, ms) for f in RB_FLAG_SETS for kt, fm in RB_SHAPE if (kt, fm) != (20, 2) or not f & RB_FM1
           for ms in ((0, 30) if f & RB_LN else (None,))]


@pytest.mark.parametrize("flags,kt,fm,ms", CASES_A)
def test_rowblock_instances(gpu, flags, kt, fm, ms):
    """Each of the 12 compiled flag sets at <KT 10, FM 2> (K 320, M 512) and <20, 1> (K 640, M 384,
    tuning key 15 = 0), the 7 without statistics / sums / affine also at K 640, M 512 with key 15 = 1:
    <20, 2>, but <20, 1> for the two with a residual (RB_FM1_K640 above).
    N = 192 (128 packed for GEGLU), K = 640 with a residual through tuning key 20.  At these M a
    block owns one 32-column chunk (ntn = N / 32), so statistics and column sums cannot be fused:
    the plan is the flag set without them plus the trailing pass, and the outputs are checked
    with that pass's bound (section c has the fused forms)."""
    K, M = RB_SHAPE[(kt, fm)]
    N = 128 if flags & RB_GEGLU else 192
    req = rb_request(flags, K, N)
    req["ln"] = ms
    fm_plan = 1 if kt == 20 and flags & RB_RES else fm
    expect = dict(family=1, rb_kt=kt, rb_fm=fm_plan, rb_flags=flags & ~(RB_STATS | RB_GNCS),
                  row_stats=int(bool(flags & RB_STATS)), colsum_rows=M if flags & RB_GNCS else 0)
    name = f"rowblock K {K} M {M} <{kt}, {fm_plan}> flags {flags} mean {ms}"
    w = run_linear(name, M, K, N, tune=rb_tune(K, fm, req["res"]), expect=expect, chunks={1}, record=True, **req)
    note("a", *w)
    print(f"{name}: worst err/bound y / stats / sums {fmt(w)}")


def test_rowblock_out_scale(gpu):
    """out_scale = 0.5 with a residual: the epilogue's "(acc[i][j][r] + r4[r]) * a.out_scale" side."""
    w = run_linear("rowblock out_scale", 512, 320, 192, res=True, out_scale=0.5, chunks={1}, record=True,
                   expect=dict(family=1, rb_kt=10, rb_fm=2, rb_flags=RB_RES))
    note("a", *w)
    print(f"rowblock out_scale 0.5: worst err/bound {fmt(w)}")


@pytest.mark.parametrize("ms", [0, 30])
def test_rowblock_ln_rowvec_mod(gpu, ms):
    """RB_LN | RB_RV with rows_per_vec 256, rowvec_mod 3 and rowvec_ld = N + 8 on M = 1024: the
    four row blocks take table rows 0, 1, 2, 0."""
    N = 192
    w = run_linear(f"rowblock ln rowvec mod 3 mean {ms}", 1024, 320, N, ln=ms, rowvec=(256, 3, N + 8), record=True,
                   expect=dict(family=1, rb_kt=10, rb_fm=2, rb_flags=RB_LN | RB_RV))
    note("a", *w)
    print(f"rowblock ln rowvec mod 3 mean {ms}: worst err/bound {fmt(w)}")


# ---------------------------------------------------------------- b. row-block steady state
# (M, N, K, key 15, flags, planned FM, chunks per block); K 640 with a residual is planned at FM 1
# whatever key 15 says, so its 256 row blocks own all 6 chunks
STEADY = [(21760, 192, 320, 1, RB_RES, 2, {1, 2}), (32768, 192, 320, 1, RB_RES, 2, {3}), (65536, 192, 320, 1, RB_RES, 2, {6}),
          (32768, 64, 640, 0, RB_RES, 1, {2}), (32768, 192, 640, 1, RB_RES, 1, {6}),
          (21760, 192, 320, 1, RB_LN, 2, {1, 2}), (32768, 192, 320, 1, RB_LN, 2, {3}), (65536, 192, 320, 1, RB_LN, 2, {6}),
          (32768, 64, 640, 0, RB_LN, 1, {2}), (32768, 192, 640, 1, RB_LN, 2, {3})]


@pytest.mark.parametrize("M,N,K,k15,flags,fm,chunks", STEADY)
def test_rowblock_steady_state(gpu, M, N, K, k15, flags, fm, chunks):
    """More than one chunk per block: the odd tail (2 chunks), one steady-state pair (3), the
    3-stage ring wrapping with both accumulator sets and the past-the-end DMA reload (5, 6), and
    uneven N ranges ({1, 2}).  The smallest M that give these counts: ntn = min(N / 32,
    ceil(256 / ntm)) falls only as M grows.  RB_RES moves the residual tile through the ring."""
    req = rb_request(flags, K, N)
    req["ln"] = 30 if flags & RB_LN else None
    w = run_linear(f"rowblock steady M {M} N {N} K {K} flags {flags}", M, K, N, tune=rb_tune(K, 1 + k15, req["res"]),
                   expect=dict(family=1, rb_kt=K // 32, rb_fm=fm, rb_flags=flags), chunks=chunks, record=True, **req)
    note("b", *w)
    print(f"rowblock steady M {M} N {N} K {K} flags {flags} chunks {sorted(chunks)}: worst err/bound {fmt(w)}")


def test_rowblock_steady_state_geglu(gpu):
    """RB_LN | RB_GEGLU at N = 2560 packed, M = 4096: 16 N ranges of 5 chunks."""
    w = run_linear("rowblock steady geglu", 4096, 320, 2560, ln=30, geglu=True, chunks={5}, record=True,
                   expect=dict(family=1, rb_kt=10, rb_fm=2, rb_flags=RB_LN | RB_GEGLU))
    note("b", *w)
    print(f"rowblock steady M 4096 N 2560 ln geglu chunks [5]: worst err/bound {fmt(w)}")


# ---------------------------------------------------------------- c. row-block fused statistics and sums
# (name, request, fused flags, trailing row_stats, trailing column-sum pass)
FUSED = [("stats", dict(stats=True), RB_STATS, 0, False),
         ("res_stats", dict(res=True, stats=True), RB_RES | RB_STATS, 0, False),
         ("res_gn", dict(res=True, gn=True), RB_RES | RB_GNCS, 0, False),
         ("aff_stats", dict(aff=True, stats=True), RB_AFF | RB_STATS, 0, False),
         ("res_stats_gn", dict(res=True, stats=True, gn=True), RB_RES | RB_STATS, 0, True),  # no instance has both
         ("gn", dict(gn=True), 0, 0, True)]                                                # nor the sums alone


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("K", [320, 640])
@pytest.mark.parametrize("name,req,flags,row_stats,cs_pass", FUSED, ids=[f[0] for f in FUSED])
def test_rowblock_fused_stats_and_sums(gpu, name, req, flags, row_stats, cs_pass, K, N):
    """row_stats_out and gn_colsum_out from the row-block epilogue need one N range per block
    (ntn == 1): 256 row blocks, M = 65536 at K 320 and 32768 at K 640 with one fragment per wave;
    N = 64 and 128 (2 and 4 chunks: merge_cs both in the loop and after it).  The affine has 256
    samples of 256 / 128 rows.  stats_out is checked per row against the stored rows
    (stored_row_stats_bound, chain 8), the sums per slot and column (colsum_bound), both inside
    guard bands: exactly M rows and M / 128 slots are written."""
    M = 65536 if K == 320 else 32768
    fm = 2 if K == 320 or not flags & RB_FM1_K640 else 1
    req = dict(req)
    if req.get("aff"):
        req["aff"] = (256 if K == 320 else 128, 0.5)
    # (the sums alone at K 640 run the plain two-fragment instance: 128 row blocks, two N ranges)
    chunks = {N // 64} if K == 640 and fm == 2 else {N // 32}
    w = run_linear(f"rowblock fused {name} K {K} N {N}", M, K, N, tune=rb_tune(K, fm, req.get("res")), record=True,
                   expect=dict(family=1, rb_kt=K // 32, rb_fm=fm, rb_flags=flags, row_stats=row_stats,
                               colsum_rows=M if cs_pass else 0), chunks=chunks, **req)
    note("c", *w)
    print(f"rowblock fused {name} K {K} N {N}: worst err/bound y / stats / sums {fmt(w)}")


# ---------------------------------------------------------------- d. RB_AFF per element
@pytest.mark.parametrize("K,samples,pps", [(320, 3, 256), (640, 5, 128)])
def test_rowblock_affine_sample_boundaries(gpu, K, samples, pps):
    """The GroupNorm affine folded into the A rows ("v[e] = (__bf16)fmaf((float)v[e], sc[e],
    sh[e])") against fp64 with gemm_bound's prologue term: per-sample scale and a shift near 2,
    one block per sample (K 320) -- a block that reads its neighbour's sample is far outside."""
    M = samples * pps
    w = run_linear(f"rowblock affine K {K}", M, K, 192, aff=(pps, 2.0), tune=rb_tune(K, 1, False),
                   expect=dict(family=1, rb_kt=K // 32, rb_fm=2 if K == 320 else 1, rb_flags=RB_AFF))
    note("d", *w)
    print(f"rowblock affine K {K} {samples} samples of {pps}: worst err/bound {fmt(w)}")


# ---------------------------------------------------------------- e. the tiled LN fold
TILE = {1: (128, 128), 2: (128, 64), 4: (128, 32), 5: (256, 256), 9: (128, 160)}
FOLD_CFG = [(f"tile{t}", dict(k2=t), t, 0) for t in TILE] + [("regstage", dict(k1=1), 0, 0), ("split2", dict(k2=1, k3=2), 1, 2)]
FOLD_N = [("plain72", 72, False), ("scalar20", 20, False), ("geglu64", 64, True)]


@pytest.mark.parametrize("ms", [0, 30])
@pytest.mark.parametrize("kind,N,geglu", FOLD_N, ids=[k[0] for k in FOLD_N])
@pytest.mark.parametrize("cfg,tune,tile,split", FOLD_CFG, ids=[c[0] for c in FOLD_CFG])
def test_tiled_ln_fold(gpu, cfg, tune, tile, split, kind, N, geglu, ms):
    """rstd * (acc - mean * colsum[c]) in all five places of the tiled kernels: store_tile_plain_pre
    (N 72, bf16), store_tile_geglu (N 64 packed), ln_fold8 / epi_chunk (N 20: the scalar side),
    epi_geglu8 and the split-K reduce (split 2), plus the general epilogue (fp32 out) and the
    register-staged kernel; M in P.EDGE_M, K = 320, bf16 and fp32 out, alone and with rowvec
    (rows_per_vec 50, mod 3, ld N + 8) + residual + out_scale 0.5 together.  form="epilogue": the
    bound charges the cancellation of a large row mean and the host's fp32 colsum."""
    worst = 0.0
    for M in P.EDGE_M:
        for out_dtype in (BF, F32):
            for extras in ((False,) if geglu else (False, True)):
                general = split or N % 8 or out_dtype == F32
                expect = dict(family=2 if cfg == "regstage" else 0, split=2 if split else 1, reduce=int(bool(split)))
                if tile:
                    expect.update(bm=TILE[tile][0], bn=TILE[tile][1])
                if cfg != "regstage":
                    expect["epi"] = 2 if general else 1 if geglu else 0
                kw = dict(rowvec=(50, 3, N + 8), res=True, out_scale=0.5) if extras else {}
                w = run_linear(f"tiled ln fold {cfg} {kind} M {M} {out_dtype} extras {extras} mean {ms}", M, 320, N, ln=ms,
                               geglu=geglu, out_dtype=out_dtype, split=split, form="epilogue", tune=tune, expect=expect, **kw)
                worst = max(worst, w[0])
    note("e", worst)
    print(f"tiled ln fold {cfg} {kind} mean {ms}: worst err/bound {worst:.3f}")


# ---------------------------------------------------------------- f. column sums from every producer
def run_conv_sums(name, H, W, Cin, N, ksize, *, res=False, aff=False, upsample=False, tune=None, expect=None, n=2):
    """One conv with gn_out into a guarded buffer: y per element, then every 128-row slot (the
    plan's numbering, P.halo_slot_rows) and column of the sums against the stored y."""
    x = P.bf16_round(E.rnd(n, H, W, Cin, seed=H + Cin) * 2 + 0.5)
    w = P.bf16_round(E.rnd(*((N, Cin, 3, 3) if ksize == 3 else (N, Cin)), seed=N + 1, scale=1 / math.sqrt(ksize * ksize * Cin)))
    b = E.rnd(N, seed=2, scale=0.1) + 0.5
    a = (1 + 0.2 * E.rnd(n, Cin, seed=7), 0.5 + 0.3 * E.rnd(n, Cin, seed=8), 1, True) if aff else None
    ref, mag, prod = E.conv_reference(x, None, w, b, ksize, aff=a, upsample=upsample)
    Ho, Wo = ref.shape[1:3]
    M = n * Ho * Wo
    r = P.bf16_round(E.rnd(n, Ho, Wo, N, seed=77)) if res else None
    if res:
        ref, mag = ref + P.f64(r), mag + P.f64(r).abs()
    pw = E.packed(w, b, ksize)
    if upsample:  # the phase form: 4 taps of summed, re-rounded weights (gemm_bound's prologue term)
        pw.phase = pack_phase_weight(w).to(BF).to(DEV).contiguous()
        bound = P.gemm_bound(ref, mag, 4 * Cin, BF, prologue=True, prod_mag=prod)
    else:
        bound = P.gemm_bound(ref, mag, ksize * ksize * Cin, BF, prologue=aff, prod_mag=prod)
    xd = E.dev_bf(x)
    kw = dict(upsample=upsample, workspace_bytes=WS)
    if aff:
        kw["aff"] = (a[0].to(DEV), a[1].to(DEV), 1, True)
    if res:
        kw["res"] = E.wide(r, N + 8)
    g = P.guarded((n, Ho, Wo, N), pitch=N + 8, pad_rows=3, dtype=BF, device=DEV)
    g_cs = P.guarded((M // 128, 2, N), pad_rows=2, dtype=F32, device=DEV)
    inputs = E.snaps(xd, pw.w, pw.phase, pw.bias, kw.get("res"), *(kw["aff"][:2] if aff else ()))
    with tuning(**(tune or {})):
        plan = ops.conv_plan(xd, pw, out=g.view, gn_out=g_cs.view, **kw)
        assert plan is not None, f"{name}: {_lib.load().ls_last_error().decode()}"
        for k, v in (expect or {}).items():
            assert plan[k] == (M if v == "M" else v), f"{name}: plan {k} = {plan[k]}, the case was written for {v} ({plan})"
        ops.conv(xd, pw, out=g.view, gn_out=g_cs.view, **kw)
    wy = E.finish(name, g, ref, bound, inputs)
    ys = g.view.float().cpu().reshape(M, N)
    cref, cb = P.colsum_bound(ys[P.halo_slot_rows(plan, n, Ho, Wo).reshape(-1)])
    wc = P.assert_elementwise(g_cs.view, cref, cb, where=dict(rows=2, cols=16), name=name + " column sums")
    P.assert_guard_intact(g_cs, name + " column sums")
    return wy, wc


IMAGES = ((16, 16), (32, 16))
# forced tile -> whether its epilogue has the sums (cs_tile_fits and the planner's cs_epi)
SUM_TILES = [(1, True), (2, True), (9, True), (3, False), (4, False), (5, False), (6, False)]


@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("tile,fused", SUM_TILES)
def test_column_sums_tiled(gpu, tile, fused, ksize):
    """The tiled epilogue's per-pass sums (tiles 1, 2, 9) and the read pass behind the tiles
    without them (3, 4, 5, 6), on a 3x3 conv with a residual and on a 1x1; N = 160 (a partial
    column tile on all but tile 9), y of pitch N + 8."""
    worst = (0.0, 0.0)
    for H, W in IMAGES:
        w = run_conv_sums(f"sums tile {tile} ksize {ksize} {H}x{W}", H, W, 64, 160, ksize, res=ksize == 3, tune=dict(k2=tile),
                          expect=dict(family=0, colsum_rows=0 if fused else "M"))
        worst = tuple(max(a, b) for a, b in zip(worst, w))
    note("f", *worst)
    print(f"column sums tile {tile} ksize {ksize}: worst err/bound y / sums {fmt(worst)}")


def test_column_sums_split_k(gpu):
    """Split-K 2 (3x3, Cin 64: 9 K-tiles): the reduce stores y, the read pass sums it."""
    worst = (0.0, 0.0)
    for H, W in IMAGES:
        w = run_conv_sums(f"sums split2 {H}x{W}", H, W, 64, 160, 3, res=True, tune=dict(k2=1, k3=2),
                          expect=dict(family=0, split=2, reduce=1, colsum_rows="M"))
        worst = tuple(max(a, b) for a, b in zip(worst, w))
    note("f", *worst)
    print(f"column sums split-K 2: worst err/bound y / sums {fmt(worst)}")


HALO_SUMS = [(128, 1, 128, 8), (128, 0, 128, 16), (160, 1, 160, 16), (16, 1, 16, 8), (8, 1, 16, 8)]  # (N, key 16, halo_bn, halo_th)


@pytest.mark.parametrize("aff", [False, True])
@pytest.mark.parametrize("N,th8,bn,th", HALO_SUMS)
def test_column_sums_halo(gpu, N, th8, bn, th, aff):
    """The halo kernel's register partials (CSG = 2), every slot: 128-column tiles on 16 x 8 and
    16 x 16 patches, 160 columns, the narrow tile (N 16 and 8); with a residual, without and with
    the input affine; 16 x 16 (one patch) and 32 x 16 (two patch rows) images."""
    worst = (0.0, 0.0)
    for H, W in IMAGES:
        w = run_conv_sums(f"sums halo N {N} th8 {th8} aff {aff} {H}x{W}", H, W, 64, N, 3, res=True, aff=aff, tune=dict(k16=th8),
                          expect=dict(family=3, halo_bn=bn, halo_th=th, halo_cs=1, halo_gn=int(aff), colsum_rows=0))
        worst = tuple(max(a, b) for a, b in zip(worst, w))
    note("f", *worst)
    print(f"column sums halo N {N} th8 {th8} aff {aff}: worst err/bound y / sums {fmt(worst)}")


@pytest.mark.parametrize("N,th8,bn,th", HALO_SUMS[:3])
def test_column_sums_halo_phase(gpu, N, th8, bn, th):
    """The halo phase form (path 4): 16 x 16 and 32 x 16 INPUT images, slots numbered (parity,
    patch), each 128 stored pixels of one output parity."""
    worst = (0.0, 0.0)
    for H, W in IMAGES:
        w = run_conv_sums(f"sums halo phase N {N} th8 {th8} {H}x{W}", H, W, 64, N, 3, res=True, upsample=True, tune=dict(k16=th8),
                          expect=dict(family=4, halo_bn=bn, halo_th=th, halo_cs=1, halo_ph=1, colsum_rows=0))
        worst = tuple(max(a, b) for a, b in zip(worst, w))
    note("f", *worst)
    print(f"column sums halo phase N {N} th8 {th8}: worst err/bound y / sums {fmt(worst)}")


def test_column_sums_tiled_phase(gpu):
    """The tiled phase form (path 5; 8 x 8 and 16 x 8 inputs, below a halo patch): the read pass
    over the 16 x 16 / 32 x 16 output."""
    worst = (0.0, 0.0)
    for H, W in ((8, 8), (16, 8)):
        w = run_conv_sums(f"sums tiled phase {H}x{W}", H, W, 64, 160, 3, res=True, upsample=True,
                          expect=dict(family=5, epi=3, colsum_rows="M"))
        worst = tuple(max(a, b) for a, b in zip(worst, w))
    note("f", *worst)
    print(f"column sums tiled phase: worst err/bound y / sums {fmt(worst)}")


# ---------------------------------------------------------------- g. the ragged grouped raster
def test_ragged_grouped_raster(gpu):
    """Forced 256 x 256 tile on a 1x1 with K = 64: gm = 4 row bands per group, M = 1100 gives
    ntm = 5, so the last group has ONE band (tile_of's "rows = min(a.ntm - first, a.gm)"), and
    N = 264 a second, 8-column-wide column tile."""
    M, K, N = 1100, 64, 264
    w = run_linear("ragged raster", M, K, N, res=True, tune=dict(k2=5), expect=dict(family=0, bm=256, bn=256, grid=10, epi=0))
    note("g", *w)
    print(f"ragged grouped raster: worst err/bound {fmt(w)}")


# ---------------------------------------------------------------- the instances sections a to c ran
def test_every_rowblock_instance_ran(gpu):
    """The (rb_kt, rb_fm, rb_flags) of the plans that sections a to c asserted (and then ran) are
    all compiled instances of gemm_rowblock_kernel: 12 flag sets at <10, 2> and <20, 1>, the 5
    without statistics, sums, affine or residual at <20, 2> -- 29, since the two <20, 2> residual
    instances that could not be launched are gone.  Runs after them, in the same process."""
    assert len(RB_INSTANCES) == 29
    assert SEEN == RB_INSTANCES, f"never planned: {sorted(RB_INSTANCES - SEEN)}; not compiled: {sorted(SEEN - RB_INSTANCES)}"
    print("worst err/bound per section: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
