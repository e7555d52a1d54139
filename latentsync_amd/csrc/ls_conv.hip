// Host side of the conv / linear layer: the plan of a call (plan_conv), the split-K reduce and
// GroupNorm column-sum passes, and the C entry points.  The kernels are in ls_conv_tiled.hip,
// ls_conv_big.hip, ls_conv_rowblock.hip and ls_conv_halo.hip.
#include <algorithm>

#include "ls_conv.h"

namespace ls {

ConvTuning g_tune;

struct TileCfg { int bm, bn, split; };

// Tile + split-K choice by a small cost model. A CU runs up to R blocks of a tile
// at once (LDS-limited: 2 for the 4-wave 128-row tiles, 1 for the 8-wave 256x256);
// the grid takes ceil(blocks / CUs) block-durations per CU, and a 4-wave tile alone
// on a CU runs at ~0.75 of its throughput with a second block beside it (measured,
// scripts/splitk_sweep.py: 128x160 at 256 blocks 685 TF/s, at 512 blocks 838).
// eff = relative MFMA throughput of the tile; split-K adds its fp32 slab write + read
// (~1.5 MAC-units per slab element, calibrated on the 4x4-level convs and FF2).
static TileCfg pick_tile(long M, int N, int ktiles, bool allow_split, bool big_ok, int ksize) {
  struct Cand { int bm, bn; double eff; int waves, resident; };
  const Cand cands[] = {{128, 128, 1.0, 4, 2}, {128, 160, 1.2, 4, 2}, {128, 64, 0.72, 4, 2}, {64, 64, 0.42, 4, 4},
                        {128, 32, 0.36, 4, 4}, {256, 256, 1.5, 8, 1}};
  TileCfg best{128, 128, 1};
  double best_t = 1e300;
  for (const Cand& c : cands) {
    if (c.bn == 32 && N > 32) continue;
    if (N <= 32 && c.bn != 32) continue;
    if (c.bm == 256) {
      if (!big_ok || N < 256) continue;
      // linears: 256x256 only on wide N (GEGLU W1, fused q|k|v, and N = 1280: the 8x8 / 4x4
      // levels' projections, FF2 and shortcuts, 7-16 % faster than 128x160 on every one of
      // them, profiles/r05c_n1280.txt) or when 160 does not divide N (the VAE's 512); 3x3
      // convs: the cost model decides
      if (ksize == 1 && ((N % 256 != 0 && N < 1920) || (N < 1280 && N % 160 == 0))) continue;
    }
    if (c.bn == 160 && N % 160 != 0) continue;  // the UNet's widths are all multiples of 160
    const long tiles = (long)cdiv(M, c.bm) * cdiv(N, c.bn);
    for (int split = 1; split <= 16; ++split) {
      // split-K only to fill the chip (grids of fewer tiles than CUs)
      if (split > 1 && (!allow_split || ktiles / split < 4 || tiles >= 256)) break;
      const long blocks = tiles * split;
      const long per_cu = (blocks + 255) / 256;
      const long conc = std::min<long>(c.resident, per_cu);
      const double f = (c.waves * conc >= 8) ? 1.0 : 0.75;
      const double per_block = (double)c.bm * c.bn * 64.0 * cdiv(ktiles, split) / c.eff;
      double t = per_cu * per_block / f;
      if (split > 1) t += (double)M * N * split * 1.5;
      if (t < best_t * 0.97) { best_t = t; best = {c.bm, c.bn, split}; }
    }
  }
  return best;
}

// split-K slabs of whole K-tiles: at most `split` of them, none empty
static void set_split(ConvArgs& a, int split) {
  a.kt_per_split = cdiv(a.ktiles, std::max(1, std::min(split, a.ktiles)));
  a.split = cdiv(a.ktiles, a.kt_per_split);
}

// epilogue variant of a launch (see store_tile)
static int epi_kind(const ConvArgs& a) {
  if (a.phase) return EPI_PLAINP;  // (tiled_phase_ok: the plain epilogue's conditions hold)
  if (a.split != 1 || !vec_ok(a) || a.y_f32) return EPI_ANY;
  if (a.act == LS_ACT_NONE) return EPI_PLAIN;
  if (a.act == LS_ACT_GEGLU) return EPI_GEGLU;
  return EPI_ANY;
}

// operand DMA through buffer descriptors: 1x1 with K == Cin, Cin % 64 == 0; tap-major 3x3,
// stride 1 or 2, pad 0 or 1, or nearest-x2 upsample with pad 1; C1 % 64 == 0 (a K-tile never straddles the
// concat); byte offsets of a tile's window must fit 31 bits (they do: < 16 MB)
static bool buf_dma_ok(const ConvArgs& a, int ks) {
  if (a.aff_scale) return false;
  if (ks == 1) return a.Cin % 64 == 0 && a.C1 % 64 == 0 && a.K == a.Cin;
  if (a.upsample) return a.Cin % 64 == 0 && a.C1 % 64 == 0 && a.stride == 1 && a.pad == 1;
  return a.Cin % 64 == 0 && a.C1 % 64 == 0 && (a.stride == 1 || a.stride == 2) && (a.pad == 0 || a.pad == 1);
}

// The phase form of an upsample conv (upsample == 2) on the tiled kernels, for what the halo
// kernel does not take (N > 640, images its patches do not divide): per output parity a plain
// pad-1 conv in input space over 4 of the 9 tap positions (BufDma's border masks and tap_of
// as for any 3x3), the parity a grid slice, rows mapped to the strided output pixels in the
// plain epilogue (EPI_PLAINP); GroupNorm column sums by the read pass over the stored output.
static bool tiled_phase_ok(const ConvArgs& a) {
  return a.upsample == 2 && vec_ok(a) && !a.y_f32 && a.act == LS_ACT_NONE && !a.rowvec && !a.C2 && !g_tune.force_regstage &&
         buf_dma_ok(a, 3);
}

static void to_tiled_phase(ConvArgs& a, int bm) {
  a.phase = 1;  // (the kernel sets 1 + ph)
  a.upsample = 0;
  a.Ho = a.H;
  a.Wo = a.W;
  a.M = a.n_img * a.H * a.W;
  a.ntm = cdiv(a.M, bm);
  a.gm = std::max(1, std::min(a.gm, a.ntm));
}

// The position-major form of a 3x3 / stride 1 / pad 1 conv on the 256-row tiles (ConvArgs::pm,
// conv_gemm_big_kernel<PM>): buffer DMA over channel-chunk-major K (Cin % 64 == 0, K == 9 Cin,
// no affine prologue), the single-pass 16-byte epilogue (no split-K, no GEGLU), images with an
// interior (pm_tile_of).  A row vector must not change inside a standard 256-row tile, so that
// both forms add it to the bias first and round alike (store_tile_plain_pre).  A frame group's
// window (256 images) must fit the 31-bit byte offsets of the A descriptor.
static bool posmajor_ok(const ls_conv_desc* d, const ConvArgs& a) {
  const long span = 256L * a.H * a.W * std::max(a.ld1, a.C2 ? a.ld2 : 0) * 2;
  return d->ksize == 3 && a.stride == 1 && a.pad == 1 && !a.upsample && !a.phase && a.Ho == a.H && a.Wo == a.W &&
         a.H >= 3 && a.W >= 3 && buf_dma_ok(a, 3) && !g_tune.force_regstage && a.K == 9 * a.Cin && a.split == 1 &&
         vec_ok(a) && a.act != LS_ACT_GEGLU && (!a.rowvec || a.rows_per_vec % 256 == 0) &&
         span < (1L << 30);
}

// Tap-units on the critical path of the position-major launch: every XCD (32 CUs, one block
// each) hands its blocks, in index order, to the CU that is free first.  (The standard raster
// costs ceil(tiles / 256) * 9 in the same unit.)
static int posmajor_cost(int H, int W, int G, int ntn) {
  struct Memo { int H, W, G, ntn, cost; };  // (a model's few shapes recur on every call)
  static thread_local Memo memo[8];
  static thread_local int memo_next = 0;
  for (const Memo& m : memo)
    if (m.H == H && m.W == W && m.G == G && m.ntn == ntn) return m.cost;
  const int nb = H * W * G * ntn;
  int worst = 0;
  for (int x = 0; x < 8; ++x) {
    int load[32] = {0};
    for (int b = x; b < nb; b += 8) {
      int pos, g, tn;
      pm_tile_of(b, H, W, G, ntn, pos, g, tn);
      int* lo = std::min_element(load, load + 32);
      *lo += __builtin_popcount(pm_tap_mask(H, W, pos));
    }
    worst = std::max(worst, *std::max_element(load, load + 32));
  }
  memo[memo_next++ % 8] = Memo{H, W, G, ntn, worst};
  return worst;
}

// split-K reduction + epilogue: one thread per 8 output columns
__global__ void splitk_reduce_kernel(ConvArgs a) {
  const bool geglu = a.act == LS_ACT_GEGLU;
  const int nout = geglu ? a.N / 2 : a.N;
  const int cpr = (nout + 7) / 8;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)a.M * cpr) return;
  const int row = idx / cpr, o8 = (int)(idx - (long)row * cpr) * 8;
  const long MN = (long)a.M * a.N;
  const bool vec = (a.N % 8 == 0) && (a.ldy % 8 == 0) && (!a.res || a.ldr % 8 == 0);
  if (geglu) {
    const int ph = (o8 >> 4) * 32 + (o8 & 15);
    float h[8], g[8], t[8];
    for (int j = 0; j < 8; ++j) { h[j] = 0.f; g[j] = 0.f; }
    for (int z = 0; z < a.split; ++z) {
      load8f(a.partial + z * MN + (long)row * a.N + ph, t);
      for (int j = 0; j < 8; ++j) h[j] += t[j];
      load8f(a.partial + z * MN + (long)row * a.N + ph + 16, t);
      for (int j = 0; j < 8; ++j) g[j] += t[j];
    }
    epi_geglu8(a, row, ph, h, g, vec);
  } else {
    float v[8];
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    for (int z = 0; z < a.split; ++z) {
      const float* p = a.partial + z * MN + (long)row * a.N + o8;
      if (vec) {
        float t[8];
        load8f(p, t);
        for (int j = 0; j < 8; ++j) v[j] += t[j];
      } else {
        for (int j = 0; j < 8 && o8 + j < a.N; ++j) v[j] += p[j];
      }
    }
    epi_chunk(a, row, o8, v, vec && o8 + 8 <= a.N);
  }
}

// GroupNorm column sums of a stored bf16 [M][ldy] tensor by a separate read pass
// (producers whose epilogue does not emit them: split-K, the row-block kernel, the
// small tiles).  Block = (slot, 32 column chunks of 8); thread = (chunk, row lane of
// 8); same fp32-per-slot sums as the epilogue (the order of the adds differs).
__global__ void __launch_bounds__(256) colsum_pass_kernel(const u16* __restrict__ y, long ldy, int N,
                                                          float* __restrict__ out) {
  __shared__ float red[8][32][17];
  const int lane = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const long slot = blockIdx.x;
  const int cc = blockIdx.y * 32 + lane;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  if (cc * 8 < N) {
    const u16* src = y + slot * CS_ROWS * ldy + cc * 8;
#pragma unroll 4
    for (int r = rl; r < CS_ROWS; r += 8) {
      float f[8];
      unpack8(*(const uint4*)(src + (long)r * ldy), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1[j] += f[j]; s2[j] = fmaf(f[j], f[j], s2[j]); }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[rl][lane][j] = s1[j]; red[rl][lane][8 + j] = s2[j]; }
  __syncthreads();
  if (rl == 0 && cc * 8 < N) {
    float t[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) t[j] = red[0][lane][j];
    for (int k = 1; k < 8; ++k)
#pragma unroll
      for (int j = 0; j < 16; ++j) t[j] += red[k][lane][j];
    float* o = out + slot * 2 * N + cc * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) { o[j] = t[j]; o[N + j] = t[8 + j]; }
  }
}

static int launch_colsum_pass(const u16* y, long ldy, long M, int N, float* out, hipStream_t s) {
  if (!y || !out || M <= 0 || M % CS_ROWS || N <= 0 || N % 8 || ldy % 8)
    return fail(LS_ERR_INVALID, "gn column sums: M % 128 == 0, N % 8 == 0, ldy % 8 == 0");
  colsum_pass_kernel<<<dim3((unsigned)(M / CS_ROWS), cdiv(N / 8, 32)), 256, 0, s>>>(y, ldy, N, out);
  return check_launch("colsum_pass_kernel");
}

// ---- the plan
static int plan_conv(const ls_conv_desc* d, ConvPlan& p) {
  if (!d || !d->x1 || !d->w || !d->y) return fail(LS_ERR_INVALID, "ls_conv2d: null pointer");
  if (d->ksize != 1 && d->ksize != 3) return fail(LS_ERR_INVALID, "ls_conv2d: ksize must be 1 or 3");
  const int Cin = d->C1 + d->C2;
  if (d->C1 % 8 || d->C2 % 8 || Cin <= 0) return fail(LS_ERR_INVALID, "ls_conv2d: channels must be multiples of 8");
  if (d->C2 && !d->x2) return fail(LS_ERR_INVALID, "ls_conv2d: C2 > 0 needs x2");
  if (d->ld1 % 8 || (d->C2 && d->ld2 % 8)) return fail(LS_ERR_INVALID, "ls_conv2d: pixel pitch must be a multiple of 8");
  if (d->upsample < 0 || d->upsample > 2) return fail(LS_ERR_INVALID, "ls_conv2d: upsample must be 0, 1 or 2");
  if (d->upsample == 2 && (d->ksize != 3 || Cin % 64 || d->K != 4 * Cin || d->aff_scale || d->stride != 1 ||
                           d->pad != 1 || d->Ho != 2 * d->H || d->Wo != 2 * d->W))
    return fail(LS_ERR_INVALID, "ls_conv2d: upsample 2 (phase-packed weights) needs ksize 3, Cin % 64 == 0, K == 4 Cin, "
                                "no affine prologue, stride 1, pad 1, Ho x Wo = 2H x 2W");
  const long Kneed = (d->upsample == 2 ? 4L : (long)d->ksize * d->ksize) * Cin;
  if (d->K % 64 || d->K < Kneed || d->K - Kneed >= 64)
    return fail(LS_ERR_INVALID, "ls_conv2d: K must be ksize^2*Cin rounded up to 64");
  if (d->ksize == 1 && (d->Ho != d->H || d->Wo != d->W || d->stride != 1 || d->upsample))
    return fail(LS_ERR_INVALID, "ls_conv2d: ksize 1 must be stride 1 with no resampling");
  if (d->act == LS_ACT_GEGLU && (d->N % 32)) return fail(LS_ERR_INVALID, "ls_conv2d: GEGLU needs N % 32 == 0");
  // (the GEGLU epilogues -- epi_geglu8, store_tile_geglu, the row-block kernel's -- add the bias only)
  if (d->act == LS_ACT_GEGLU && (d->rowvec || d->res || (d->out_scale != 0.f && d->out_scale != 1.f)))
    return fail(LS_ERR_INVALID, "ls_conv2d: GEGLU takes no rowvec, residual or out_scale");
  if (d->aff_scale && (!d->aff_shift || d->imgs_per_sample <= 0))
    return fail(LS_ERR_INVALID, "ls_conv2d: affine prologue needs shift and imgs_per_sample");
  if (d->rowvec && d->rows_per_vec <= 0) return fail(LS_ERR_INVALID, "ls_conv2d: rowvec needs rows_per_vec");
  const long M = (long)d->n_img * d->Ho * d->Wo;
  if (M <= 0 || M >= (1L << 31)) return fail(LS_ERR_INVALID, "ls_conv2d: bad M");
  p = ConvPlan{};
  ConvArgs& a = p.a;
  a.x1 = d->x1; a.x2 = d->x2; a.C1 = d->C1; a.C2 = d->C2; a.Cin = Cin; a.ld1 = d->ld1; a.ld2 = d->ld2;
  a.n_img = d->n_img; a.H = d->H; a.W = d->W; a.Ho = d->Ho; a.Wo = d->Wo;
  a.stride = d->stride; a.pad = d->pad; a.upsample = d->upsample;
  a.aff_scale = d->aff_scale; a.aff_shift = d->aff_shift;
  a.pix_per_sample = d->imgs_per_sample * d->H * d->W; a.silu_in = d->silu_in;
  a.w = d->w; a.K = d->K; a.N = d->N; a.M = (int)M; a.Mo = (int)M; a.phase = 0; a.CC = Cin / 8;
  a.bias = d->bias; a.rowvec = d->rowvec; a.rows_per_vec = d->rows_per_vec; a.rowvec_mod = d->rowvec_mod;
  a.ln_mr = d->ln_rowstats; a.ln_cs = d->ln_colsum;
  if (a.ln_mr && (!a.ln_cs || d->ksize != 1)) return fail(LS_ERR_INVALID, "ls_conv2d: ln_rowstats needs ln_colsum, ksize 1");
  a.rowvec_ld = d->rowvec_ld > 0 ? d->rowvec_ld : d->N;
  a.res = d->res; a.ldr = d->ldr; a.out_scale = d->out_scale == 0.f ? 1.f : d->out_scale; a.act = d->act;
  a.y = d->y; a.ldy = d->ldy; a.y_f32 = d->y_f32;
  a.stats_out = d->row_stats_out;
  a.stats_eps = d->row_stats_eps > 0.f ? d->row_stats_eps : 1e-5f;
  if (a.stats_out && (d->ksize != 1 || d->act == LS_ACT_GEGLU || d->y_f32))
    return fail(LS_ERR_INVALID, "ls_conv2d: row_stats_out needs ksize 1, bf16 output, no GEGLU");
  a.cs_out = d->gn_colsum_out;
  if (a.cs_out && (M % CS_ROWS || d->N % 8 || d->ldy % 8 || d->act == LS_ACT_GEGLU || d->y_f32))
    return fail(LS_ERR_INVALID, "ls_conv2d: gn_colsum_out needs M % 128 == 0, N % 8 == 0, bf16 output, no GEGLU");
  a.ablate = g_tune.ablate;
  a.ccm = (d->ksize == 3 && Cin % 64 == 0) ? 1 : 0;
  a.ktiles = d->K / 64;
  // (automatic split-K only with a workspace; the phase forms have none)
  TileCfg t = pick_tile(M, d->N, a.ktiles, d->split_k <= 0 && d->workspace != nullptr && d->upsample != 2,
                        !d->aff_scale && !g_tune.force_regstage && (d->ksize == 1 || Cin % 64 == 0), d->ksize);
  if (g_tune.force_tile) {
    // (ids 7 and 8 were rejected 256-row variants; ls_set_tuning refuses them)
    static const int tb[10][2] = {{0, 0}, {128, 128}, {128, 64}, {64, 64}, {128, 32}, {256, 256}, {256, 128},
                                  {0, 0}, {0, 0}, {128, 160}};
    t.bm = tb[g_tune.force_tile][0]; t.bn = tb[g_tune.force_tile][1]; t.split = g_tune.force_split ? g_tune.force_split : 1;
    // the 256-row kernels have no register-staged form (affine prologue, tuning key 1): such a
    // call runs a 128-row kernel, and the grid below must be the one of the kernel launched
    if (t.bm >= 256 && (d->aff_scale || g_tune.force_regstage)) { t.bm = 128; t.bn = 128; }
  }
  a.ntm = cdiv(M, t.bm); a.ntn = cdiv(d->N, t.bn);
  // grouped raster (g row-bands per group): it cuts the wide linears' L2-miss
  // fetch (GEGLU W1 at 8x8 3.6 -> 1.3 GB per call) but measured +0.4 ms per 32-window step
  // against the column-fastest order over three alternated same-box rounds
  // (profiles/r03i_locality_sweep.txt), so the default stays column-fastest (gm = 1)
  a.gm = 1;
  // round 5: 4 row bands per group for 256x256 1x1 tiles with K <= 1920 (out2 181 -> 173 us,
  // sc2b -1 %, profiles/r05s_gm_ab.txt; at K = 5120 the grouping loses)
  if (t.bm == 256 && t.bn == 256 && d->ksize == 1 && d->K <= 1920) a.gm = 4;
  a.gm = std::max(1, std::min(a.gm, a.ntm));
  set_split(a, d->upsample == 2 ? 1 : d->split_k > 0 ? d->split_k : t.split);
  const size_t slab = (size_t)a.M * a.N * sizeof(float);
  ls_conv_plan_info& i = p.i;
  i.bm = i.bn = i.ks = i.tapu = i.buf = i.epi = i.rb_kt = i.rb_fm = i.rb_flags = -1;
  i.halo_bn = i.halo_th = i.halo_gn = i.halo_cs = i.halo_ph = i.posmajor = -1;
  i.workspace_bytes = a.split > 1 ? (int64_t)(a.split * slab) : 0;
  // fewer splits where the workspace does not hold them all
  if (a.split > 1 && (!d->workspace || d->workspace_bytes < a.split * slab))
    set_split(a, d->workspace ? (int)std::min<size_t>(d->workspace_bytes / slab, a.split) : 1);
  if (a.split > 1) a.partial = (float*)d->workspace;

  // ---- the kernel: the order of these rounds is the behaviour
  float* const cs = a.cs_out;        // GroupNorm column sums: a kernel's epilogue, else a read pass over y
  float* const stats = a.stats_out;  // LayerNorm row statistics: the row-block epilogue, else ls_row_stats over y
  bool planned = false;
  if (halo_ok(d, a)) {  // 3x3 from an LDS halo tile: input affine and column sums fused; its phase form
    plan_halo(p);
    planned = true;
  } else if (a.upsample == 2) {  // the phase form on the tiled kernels
    if (!tiled_phase_ok(a))
      return fail(LS_ERR_INVALID, "ls_conv2d: no phase-form kernel for this shape (ls_conv_path -1): use upsample = 1");
    to_tiled_phase(a, t.bm);
  } else if (rowblock_ok(d, a)) {
    // (statistics, column sums) in the row-block epilogue: both, then the sums by the read
    // pass, then the statistics by ls_row_stats with the sums fused, then neither
    for (int round = 0; round < 4 && !planned; ++round) {
      const bool fuse_stats = round < 2, fuse_cs = round % 2 == 0;
      if ((!fuse_stats && !stats) || (!fuse_cs && !cs)) continue;  // (an earlier round already asked this)
      a.stats_out = fuse_stats ? stats : nullptr;
      a.cs_out = fuse_cs ? cs : nullptr;
      planned = plan_rowblock(p);
    }
    if (planned) {
      p.cs_pass = a.cs_out ? nullptr : cs;
      p.row_stats = a.stats_out ? nullptr : stats;
    }
  }
  if (!planned) {  // the tiled kernels
    // position-major 256-row tiles (tuning key 22): by the cost model only where the standard
    // raster would run a 256-row tile, on that tile's width; forced (2), on 256 x 256, or 256 x 128
    // for N < 256 or under tuning key 2 = 6
    i.posmajor = 0;
    if (g_tune.posmajor && posmajor_ok(d, a)) {
      const int bn = t.bm == 256 ? t.bn : d->N >= 256 ? 256 : 128, G = cdiv(a.n_img, 256), ntn = cdiv(d->N, bn);
      // (equal critical paths: the form with fewer tap-units in all -- the 4x4 level at 768 frames,
      // 240 blocks either way, ran 6 % faster position-major, profiles/posmajor_kernel_ab.txt)
      const long tiles = (long)cdiv(M, 256) * ntn;
      const long units = ((a.H - 2L) * (a.W - 2) * 9 + (2L * (a.H - 2) + 2 * (a.W - 2)) * 6 + 16) * G * ntn;
      const int c_pm = g_tune.posmajor == 1 && t.bm == 256 ? posmajor_cost(a.H, a.W, G, ntn) : 0;
      const int c_std = cdiv(tiles, 256) * 9;
      const bool take = g_tune.posmajor == 2 || (t.bm == 256 && (c_pm < c_std || (c_pm == c_std && units < tiles * 9)));
      if (take) {
        i.posmajor = 1;
        t.bm = 256;
        t.bn = bn;
        a.pm = G;
        a.ntm = G;
        a.ntn = ntn;
        a.gm = 1;
      }
    }
    const bool regstage = a.aff_scale || g_tune.force_regstage;  // the prologue needs the register path
    // epilogue column sums: single-pass vectorised epilogue and a tile whose staging
    // buffer holds the per-thread partials (cs_tile_fits; not 128x32 / 64x64)
    // (not the 256-row kernels: compiled in, the sums cost their main loop ~12 % -- they run
    // at the 256-VGPR limit -- against a ~15 us read pass; same-box A/B, scripts/ab_lib.sh)
    const bool cs_epi = cs && !a.phase && a.split == 1 && vec_ok(a) && !(t.bm == 128 && t.bn == 32) && t.bm != 64 && t.bm < 256;
    a.cs_out = cs_epi ? cs : nullptr;
    a.stats_out = nullptr;
    p.cs_pass = cs_epi ? nullptr : cs;
    p.row_stats = stats;
    i.family = a.phase ? 5 : regstage ? 2 : 0;
    i.bm = t.bm;
    i.bn = t.bn;
    i.ks = d->ksize;
    i.tapu = d->ksize == 3 && Cin % 64 == 0;
    i.buf = !regstage && buf_dma_ok(a, d->ksize);
    i.epi = regstage ? -1 : epi_kind(a);
    i.grid = a.pm ? a.H * a.W * a.pm * a.ntn : a.ntm * a.ntn * (a.phase ? 4 : a.split);
    i.threads = t.bm == 256 ? 512 : 256;
    i.lds_bytes = regstage ? 0 : (int)tiled_lds(t.bm, t.bn, t.bn == 32 ? 4 : 2);
    i.reduce = a.split > 1;
  }
  i.split = a.split;
  i.colsum_rows = p.cs_pass ? a.Mo : 0;
  i.row_stats = p.row_stats != nullptr;
  return LS_OK;
}

}  // namespace ls

using namespace ls;

extern "C" int ls_set_tuning(int32_t key, int32_t value) {
  switch (key) {
    case 18: g_tune.halo_ups = value != 0; return LS_OK;
    case 19: g_tune.halo_narrow = value != 0; return LS_OK;
    case 20: g_tune.rb640_res = value != 0; return LS_OK;
    case 22:
      if (value < 0 || value > 2) return fail(LS_ERR_INVALID, "position-major 3x3 conv: 0 never, 1 by the cost model, 2 wherever legal");
      g_tune.posmajor = value;
      return LS_OK;
    case 17:
      // (2, 32 rows per wave, was measured and rejected: DESIGN.md section 3)
      if (value != 1) return fail(LS_ERR_INVALID, "ls_ff_chain rows per wave: 1 (16) only");
      return LS_OK;
    case 1: g_tune.force_regstage = value != 0; return LS_OK;
    case 2:
      if (value < 0 || value > 9 || value == 7 || value == 8) return fail(LS_ERR_INVALID, "tile id 0..6 or 9");
      g_tune.force_tile = value;
      return LS_OK;
    case 3: g_tune.force_split = value; return LS_OK;
    case 4: g_tune.ablate = value; return LS_OK;
    case 6: g_tune.rowblock = value != 0; return LS_OK;
    case 7: g_tune.rowblock640 = value != 0; return LS_OK;
    case 8: g_tune.halo = value != 0; return LS_OK;
    case 12:  // (the padded-row halo image is gone since the compact image, round 5)
      if (!value) return fail(LS_ERR_INVALID, "key 12 = 0 (padded halo rows) no longer exists");
      return LS_OK;
    case 13: g_tune.halo_bn128 = value != 0; return LS_OK;
    case 15: g_tune.rb640_fm2 = value != 0; return LS_OK;
    case 16: g_tune.halo_th8 = value != 0; return LS_OK;
    case 9:
      // (the attn6 kernel was measured and rejected: DESIGN.md section 3)
      if (value) return fail(LS_ERR_INVALID, "attention variant: 0 only");
      return LS_OK;
    default: return fail(LS_ERR_INVALID, "ls_set_tuning: unknown key");
  }
}

extern "C" int ls_gemm_occupancy(int32_t which) {
  switch (which) {
    case 1: return tiled_occupancy(160);
    case 2: return big_occupancy();
    case 3: return tiled_occupancy(128);
    default: return fail(LS_ERR_INVALID, "ls_gemm_occupancy: which 1..3");
  }
}

extern "C" int ls_conv_plan(const ls_conv_desc* d, ls_conv_plan_info* out) {
  ConvPlan p;
  if (!out) return fail(LS_ERR_INVALID, "ls_conv_plan: null out");
  const int rc = plan_conv(d, p);
  if (rc == LS_OK) *out = p.i;
  return rc;
}

extern "C" int ls_conv_posmajor_tile(int32_t H, int32_t W, int32_t groups, int32_t ntn, int32_t block, int32_t* out) {
  if (!out || H < 3 || W < 3 || groups < 1 || ntn < 1 || block < 0 || (long)block >= (long)H * W * groups * ntn)
    return fail(LS_ERR_INVALID, "ls_conv_posmajor_tile: H, W >= 3, groups, ntn >= 1, 0 <= block < H W groups ntn");
  pm_tile_of(block, H, W, groups, ntn, out[0], out[1], out[2]);
  out[3] = __builtin_popcount(pm_tap_mask(H, W, out[0]));
  return LS_OK;
}

extern "C" int ls_conv_path(const ls_conv_desc* d) {
  ConvPlan p;
  return plan_conv(d, p) == LS_OK ? p.i.family : -1;
}

extern "C" size_t ls_conv_workspace_bytes(const ls_conv_desc* d) {
  ConvPlan p;  // (the bytes are taken before the split is fitted: the plan of an unlimited workspace)
  return plan_conv(d, p) == LS_OK ? (size_t)p.i.workspace_bytes : 0;
}

extern "C" int ls_conv2d(const ls_conv_desc* d, void* stream) {
  ConvPlan p;
  int rc = plan_conv(d, p);
  if (rc != LS_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const ConvArgs& a = p.a;
  const int f = p.i.family;
  if (f == 1) launch_rowblock(p, s);
  else if (f == 3 || f == 4) launch_halo(p, s);
  else launch_tiled(p, s);
  rc = check_launch(f == 1 ? "gemm_rowblock_kernel" : f == 3 || f == 4 ? "conv3x3_halo_kernel" : "conv_gemm_kernel");
  if (rc != LS_OK) return rc;
  if (p.i.reduce) {
    const long nchunk = (long)a.M * ((((a.act == LS_ACT_GEGLU) ? a.N / 2 : a.N) + 7) / 8);
    splitk_reduce_kernel<<<cdiv(nchunk, 256), 256, 0, s>>>(a);
    if ((rc = check_launch("splitk_reduce_kernel")) != LS_OK) return rc;
  }
  if (p.cs_pass && (rc = launch_colsum_pass((const u16*)a.y, a.ldy, p.i.colsum_rows, a.N, p.cs_pass, s)) != LS_OK) return rc;
  if (p.row_stats) return ls_row_stats((const uint16_t*)a.y, a.ldy, a.Mo, a.N, a.stats_eps, p.row_stats, stream);
  return LS_OK;
}

extern "C" int ls_gn_colsum(const uint16_t* y, int64_t ldy, int64_t M, int32_t N, float* out, void* stream) {
  return launch_colsum_pass(y, ldy, M, N, out, (hipStream_t)stream);
}
