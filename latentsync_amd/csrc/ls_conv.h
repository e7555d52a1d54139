// Fused implicit-GEMM convolution / linear layer for gfx950 (bf16 MFMA 16x16x32).
//
// One kernel family covers every dense contraction of the UNet / SD-VAE / Whisper
// path: InflatedConv3d 3x3 (s1, s2, fused nearest-x2 upsample), 1x1 convs and
// nn.Linear (ksize 1).  The A operand is gathered straight from the NHWC
// activation (optionally two tensors = fused torch.cat, optionally through the
// GroupNorm affine + SiLU prologue); W is pre-packed [N][K] K-contiguous.
//
// This header: what every kernel family needs -- the kernel arguments, the epilogue, the plan
// and the tuning state.  One translation unit per family (a kernel template is instantiated
// only where it is defined): ls_conv_tiled.hip, ls_conv_big.hip, ls_conv_rowblock.hip,
// ls_conv_halo.hip; ls_conv.hip holds the planner, the two small passes and the C entry points.
#pragma once
#include <type_traits>

#include "ls_common.h"

namespace ls {

struct ConvArgs {
  const u16* x1; const u16* x2;
  int C1, C2, Cin, ld1, ld2;
  int n_img, H, W, Ho, Wo, stride, pad, upsample;
  const float* aff_scale; const float* aff_shift; int pix_per_sample; int silu_in;
  const u16* w; int K, N, M, CC;
  const float* bias; const float* rowvec; int rows_per_vec, rowvec_ld, rowvec_mod;
  const float* ln_mr; const float* ln_cs;
  const u16* res; int ldr; float out_scale; int act;
  void* y; int ldy; int y_f32;
  int ktiles, kt_per_split, split; float* partial;
  int ntm, ntn;
  float* stats_out; float stats_eps;  // row (mean, rstd) of y (row-block epilogue or a trailing row_stats)
  float* cs_out;  // GroupNorm column sums of y: [M / CS_ROWS][2][N] fp32 (sum, sum of squares per slot)
  int ablate;  // tuning only (bits): 2 = skip operand DMA, 4 = skip epilogue stores, 8 = skip epilogue,
               // 16 = skip MFMAs (DMA kernel)
  int ccm;     // 3x3 with Cin % 64 == 0: K is channel-chunk-major, taps innermost (see tap_of)
  int gm;      // tile raster: groups of gm row-blocks x all column tiles, row-block fastest (tile_of)
  int Mo;      // rows of y (== M except in the tiled phase form, where M counts one parity's rows)
  // tiled phase form of an upsample conv (ls_conv_desc.upsample == 2 off the halo kernel): 0, or
  // 1 + ph for output parity ph = 2 py + px.  The launch is a plain pad-1 conv in INPUT space
  // (Ho x Wo = H x W, M = n_img H W) over the parity's 4 taps with its [N][4 Cin] weights; the
  // host passes 1 and a 4 x larger grid, the kernel sets ph (EPI_PLAINP, tile_phase)
  int phase;
  // position-major form of a 3x3 / stride 1 / pad 1 conv on the 256-row tiles: 0, or the number of
  // 256-frame groups.  A tile is 256 frames at ONE pixel position (pm_tile_of), so all its rows
  // have the same valid taps and the K loop leaves the padding taps' K-tiles out
  int pm;
};

// Logical tile index -> (row-block, column-block), grouped: gm row-blocks x all ntn column
// tiles per group, the row-block index fastest.  Tiles running together on an XCD (xcd_remap
// gives every XCD a contiguous logical range) then share gm A row-bands and ~(concurrent /
// gm) W column panels instead of one A band and a W panel per tile: the wide linears
// (GEGLU W1, fused q|k|v) re-fetched their whole W per row-band (profiles/r03e_pmc_per_kernel.txt).
// gm = 1 is the plain column-fastest order.
__device__ __forceinline__ void tile_of(const ConvArgs& a, int bid, int& tm, int& tn) {
  const int gsz = a.gm * a.ntn, g = bid / gsz, r = bid - g * gsz;
  const int first = g * a.gm, rows = min(a.ntm - first, a.gm);
  tm = first + r % rows;
  tn = r / rows;
}

// ---- position-major tiles (ConvArgs::pm): launch order.  Block b runs on XCD b % 8, and an XCD
// hands its blocks to its CUs in index order.  The positions fall into three classes by their
// valid taps -- 9 inside, 6 on an edge, 4 at a corner; every XCD gets a contiguous eighth of each
// class (the remainders of the classes dealt to the XCDs in turn, so the XCDs' tap totals differ
// by less than one tile) and runs its 9-tap tiles first, its 4-tap tiles last.  Within a class
// the column tiles of a (frame group, position) are adjacent, then the positions of a frame
// group: tiles running together share the A lines of neighbouring positions and the W panels in
// the XCD's L2.  The same function is the planner's host twin (posmajor_cost, ls_conv_posmajor_tile).
__host__ __device__ inline unsigned pm_tap_mask(int H, int W, int pos) {
  const int yo = pos / W, xo = pos - yo * W;
  unsigned mk = 0;
  for (int kh = 0; kh < 3; ++kh)
    for (int kw = 0; kw < 3; ++kw)
      if ((unsigned)(yo - 1 + kh) < (unsigned)H && (unsigned)(xo - 1 + kw) < (unsigned)W) mk |= 1u << (kh * 3 + kw);
  return mk;
}

// block -> (pos, frame group g, column tile tn); H, W >= 3; G frame groups, ntn column tiles
__host__ __device__ inline void pm_tile_of(int b, int H, int W, int G, int ntn, int& pos, int& g, int& tn) {
  const int x = b % 8;
  int s = b / 8, off = 0;  // slot on the XCD; the XCD the class's first remainder tile goes to
  const int pc[3] = {(H - 2) * (W - 2), 2 * (H - 2) + 2 * (W - 2), 4};
  for (int c = 0; c < 3; ++c) {
    const int n = pc[c] * G * ntn, q = n / 8, r = n % 8, e0 = off, e1 = off + r;  // remainders: XCDs [e0, e1) mod 8
    const int lo = x - e0 < 0 ? 0 : x - e0;
    const int before = e1 <= 8 ? (lo < r ? lo : r) : (x < e1 - 8 ? x : e1 - 8) + lo;
    const int cnt = q + ((e1 <= 8 ? (x >= e0 && x < e1) : (x >= e0 || x < e1 - 8)) ? 1 : 0);
    if (s < cnt || c == 2) {
      const int j = x * q + before + s, t = j / ntn, qi = t % pc[c];
      tn = j - t * ntn;
      g = t / pc[c];
      int yo, xo;
      if (c == 0) {
        yo = 1 + qi / (W - 2);
        xo = 1 + qi % (W - 2);
      } else if (c == 2) {
        yo = (qi >> 1) ? H - 1 : 0;
        xo = (qi & 1) ? W - 1 : 0;
      } else if (qi < 2 * (W - 2)) {  // top, then bottom row
        yo = qi < W - 2 ? 0 : H - 1;
        xo = 1 + qi % (W - 2);
      } else {  // left, then right column
        const int e = qi - 2 * (W - 2);
        yo = 1 + e % (H - 2);
        xo = e < H - 2 ? 0 : W - 1;
      }
      pos = yo * W + xo;
      return;
    }
    s -= cnt;
    off = e1 % 8;
  }
}

// K order of a 3x3 weight with Cin % 64 == 0 (packing.py): k = (ci / 64) * 576 + tap * 64 +
// ci % 64 -- the 9 taps of one 64-channel chunk are consecutive K-tiles, so a block reads
// a pixel chunk's 3x3 neighbourhood in 9 back-to-back K-tiles and the re-reads hit L2
// (tap-major, the 9 re-reads of a pixel were Cin / 64 K-tiles apart and, with 64 blocks
// per XCD streaming operands in between, missed: profiles/r03e_pmc_per_kernel.txt).
// Returns the tap and sets c0 = the K-tile's first input channel (k0 = a 64-aligned K offset).
__device__ __forceinline__ int tap_of(const ConvArgs& a, int k0, int& c0) {
  if (a.phase) {  // k = (ci / 64) * 256 + t * 64 + ci % 64: 3x3 tap (py + t / 2, px + t % 2)
    const int t = (k0 >> 6) & 3, ph = a.phase - 1;
    c0 = (k0 >> 8) * 64 + (k0 & 63);
    return ((ph >> 1) + (t >> 1)) * 3 + (ph & 1) + (t & 1);
  }
  if (a.ccm) {
    const int chunk = k0 / 576, rem = k0 - chunk * 576;
    c0 = chunk * 64 + (rem & 63);
    return rem >> 6;
  }
  const int tap = k0 / a.Cin;
  c0 = k0 - tap * a.Cin;
  return tap;
}
// ---------------------------------------------------------------- epilogue
// Vectorised epilogue on 8 consecutive output columns (16-B bf16 / 32-B fp32
// stores).  All global loads of a chunk are issued before its stores.
struct Chunk8 { float v[8]; };


__device__ __forceinline__ float act_fn(int act, float v) {
  if (act == LS_ACT_GELU) return gelu_erf(v);
  if (act == LS_ACT_SILU) return silu(v);
  return v;
}

// v[8] = accumulators of packed columns [col, col+8) of `row`; applies bias,
// rowvec, residual, scale, activation and stores.  vec = all 8 in range and aligned.
__device__ __forceinline__ long rv_row(const ConvArgs& a, int row) {
  const int r = row / a.rows_per_vec;
  return (long)(a.rowvec_mod ? r % a.rowvec_mod : r) * a.rowvec_ld;
}

// LayerNorm fold: acc = rstd * (acc - mean * colsum[c])
__device__ __forceinline__ void ln_fold8(const ConvArgs& a, int row, int col, float* v, bool vec) {
  const float2 mr = *(const float2*)(a.ln_mr + 2L * row);
  if (vec) {
    float cs[8];
    load8f(a.ln_cs + col, cs);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = mr.y * (v[j] - mr.x * cs[j]);
  } else {
    for (int j = 0; j < 8 && col + j < a.N; ++j) v[j] = mr.y * (v[j] - mr.x * a.ln_cs[col + j]);
  }
}

__device__ __forceinline__ void epi_chunk(const ConvArgs& a, int row, int col, float* v, bool vec) {
  if (row >= a.M) return;
  if (a.ln_mr) ln_fold8(a, row, col, v, vec);
  if (vec) {
    float b[8], rv[8], rs[8];
    if (a.bias) load8f(a.bias + col, b); else for (int j = 0; j < 8; ++j) b[j] = 0.f;
    if (a.rowvec) load8f(a.rowvec + rv_row(a, row) + col, rv);
    else for (int j = 0; j < 8; ++j) rv[j] = 0.f;
    if (a.res) unpack8(*(const uint4*)(a.res + (long)row * a.ldr + col), rs);
    else for (int j = 0; j < 8; ++j) rs[j] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = act_fn(a.act, (v[j] + b[j] + rv[j] + rs[j]) * a.out_scale);
    if (a.y_f32) {
      float* y = (float*)a.y + (long)row * a.ldy + col;
      *(float4*)y = make_float4(v[0], v[1], v[2], v[3]);
      *(float4*)(y + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      *(uint4*)((u16*)a.y + (long)row * a.ldy + col) = pack8(v);
    }
  } else {
    for (int j = 0; j < 8; ++j) {
      const int c = col + j;
      if (c >= a.N) break;
      float t = v[j];
      if (a.bias) t += a.bias[c];
      if (a.rowvec) t += a.rowvec[rv_row(a, row) + c];
      if (a.res) t += bf2f(a.res[(long)row * a.ldr + c]);
      t = act_fn(a.act, t * a.out_scale);
      if (a.y_f32) ((float*)a.y)[(long)row * a.ldy + c] = t;
      else ((u16*)a.y)[(long)row * a.ldy + c] = f2bf(t);
    }
  }
}

// GEGLU chunk: h[8] = packed cols [ph, ph+8), g[8] = [ph+16, ph+24) -> out cols [oc, oc+8)
__device__ __forceinline__ void epi_geglu8(const ConvArgs& a, int row, int ph, float* h, float* g, bool vec) {
  if (row >= a.M) return;
  const int oc = (ph >> 5) * 16 + (ph & 15);
  if (a.ln_mr) {
    ln_fold8(a, row, ph, h, true);
    ln_fold8(a, row, ph + 16, g, true);
  }
  float bh[8], bg[8];
  if (a.bias) { load8f(a.bias + ph, bh); load8f(a.bias + ph + 16, bg); }
  else for (int j = 0; j < 8; ++j) { bh[j] = 0.f; bg[j] = 0.f; }
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (h[j] + bh[j]) * gelu_erf(g[j] + bg[j]);
  if (vec && !a.y_f32) *(uint4*)((u16*)a.y + (long)row * a.ldy + oc) = pack8(h);
  else
    for (int j = 0; j < 8; ++j) {
      if (a.y_f32) ((float*)a.y)[(long)row * a.ldy + oc + j] = h[j];
      else ((u16*)a.y)[(long)row * a.ldy + oc + j] = f2bf(h[j]);
    }
}

__device__ __forceinline__ int swz(int row, int ch) { return row * 8 + (ch ^ ((row >> 1) & 7)); }

// Accumulators of wave-row p -> LDS staging (fp32, pitch BN + 4).
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void stage_acc(f32x4 (&acc)[BM / WM / 16][BN / WN / 16], float* st, int p, int tid) {
  constexpr int WTM = BM / WM, WTN = BN / WN, FM = WTM / 16, FN = WTN / 16, SP = BN + 4;
  const int lane = tid & 63, wid = tid >> 6;
  if (wid / WN != p) return;
  const int wn = wid % WN;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        st[(i * 16 + (lane >> 4) * 4 + r) * SP + wn * WTN + j * 16 + (lane & 15)] = acc[i][j][r];
}

// Vectorised single-pass epilogue (N % 8 == 0, no split-K).  Every thread owns
// ONE 8-column chunk of the tile for the whole epilogue, so the per-column side
// inputs (bias, LayerNorm colsum) are loaded once, before the first barrier; the
// per-row side inputs (residual, row vector, LayerNorm row stats) of all of a
// thread's rows in a wave-row pass are issued together before any is consumed --
// one L2/HBM round trip per pass instead of one per chunk.
// GroupNorm statistics from the producer (a.cs_out): per CS_ROWS-row slot and column,
// the sum and the sum of squares of the STORED (bf16-rounded) values, fp32 over the
// slot -- what gn_stats_kernel would read back; ls_groupnorm_colsum merges the slots
// of a sample in fp64.  The store loop writes the rounded values back over its fp32
// staging; after the pass barrier one thread per column adds the pass's rows from LDS
// (2 registers across passes), then a barrier before the next pass re-stages.  A
// slot's sums go out with its last pass.  128-row tiles only (cs_tile_fits).
constexpr int CS_ROWS = LS_GN_SLOT_ROWS;

template <int BM, int BN, int WM, int WN>
__host__ __device__ constexpr bool cs_tile_fits() {
  return BM != 256 && BM % CS_ROWS == 0 && CS_ROWS % (BM / WM) == 0 && WM * WN * 64 >= BN;
}

// Thread geometry of the single-pass epilogue: a thread owns one 8-column chunk of the
// tile (CPRW chunk columns per row), RPI rows per iteration, ITER iterations per wave-row pass.
template <int BM, int BN, int WM, int WN>
struct EpiGeo {
  static constexpr int NT = WM * WN * 64, WTM = BM / WM, CPRW = BN / 8, RPI = NT / CPRW;
  static constexpr int ITER = (WTM + RPI - 1) / RPI;
};
// the residual chunks of one wave-row pass (the per-row side input worth prefetching; the
// LayerNorm row statistics of a folded GEMM are loaded in the pass)
template <int ITER>
struct EpiSide {
  uint4 rs[ITER];
};

// tile-local row -> output row (RW: see store_tile_plain)
constexpr int RW_PHASE = -(1 << 20);  // the tiled phase form: rows are one parity's pixels in input space
constexpr int RW_POS = RW_PHASE - 1;  // the position-major form: rows are the frames from m0 at pixel m0r
template <int RW>
__device__ __forceinline__ int epi_out_row(const ConvArgs& a, int m0, long m0r, int lr) {
  if constexpr (RW == RW_POS) {  // (frames past the last: not stored)
    const int n = m0 + lr;
    return n < a.n_img ? (int)((long)n * (a.H * a.W) + m0r) : a.Mo;
  } else if constexpr (RW == RW_PHASE) {  // input pixel (n, y, x) of parity (py, px) -> (n Ho + 2y + py) Wo + 2x + px
    const int m = m0 + lr;
    if (m >= a.M) return a.Mo;  // (past the parity's rows: not stored)
    const int hw = a.H * a.W, n = m / hw, r = m - n * hw;
    const int y = r / a.W, x = r - y * a.W, ph = a.phase - 1;
    return ((n * 2 * a.H + 2 * y + (ph >> 1)) * 2 * a.W + 2 * x + (ph & 1));
  } else if constexpr (RW > 0) return (int)(m0r + (long)(lr / RW) * a.Wo + lr % RW);
  else if constexpr (RW < 0) return (int)(m0r + (long)(lr / -RW) * 2 * a.Wo + 2 * (lr % -RW));
  else return m0 + lr;
}

// issue the residual loads of wave-row pass p (global loads into registers; the consumer's
// s_waitcnt is the compiler's): one HBM round trip per pass, issued a pass (or, from the
// DMA kernel's last K-tile, the whole final K-tile) before it is consumed
template <int BM, int BN, int WM, int WN, int RW = 0>
__device__ __forceinline__ void epi_side_load(const ConvArgs& a, int m0, int n0, long m0r, int tid, int p,
                                              EpiSide<EpiGeo<BM, BN, WM, WN>::ITER>& sd) {
  using G = EpiGeo<BM, BN, WM, WN>;
  const int c8 = (tid % G::CPRW) * 8, r0 = tid / G::CPRW;
  const int col = n0 + c8;
  const bool cok = (r0 < G::RPI) && col < a.N;
#pragma unroll
  for (int it = 0; it < G::ITER; ++it) {
    const int rl = r0 + it * G::RPI, row = epi_out_row<RW>(a, m0, m0r, p * G::WTM + rl);
    const bool ok = cok && rl < G::WTM && row < a.Mo;
    sd.rs[it] = make_uint4(0, 0, 0, 0);
    if (ok && a.res) sd.rs[it] = *(const uint4*)(a.res + (long)row * a.ldr + col);
  }
}

// CSF: the column sums also for a 256-row tile whose wave rows are 64 (the halo conv);
// RW > 0: the tile's rows are BM / RW segments of RW consecutive output pixels, one per
// image row (the halo conv's TH x TW tiles); m0 is then the tile's VIRTUAL first row
// (GroupNorm slots) and m0r the real first row.  RW < 0 (the phase form of an upsample conv):
// the segments are -RW INPUT pixels of one input row, i.e. every second pixel of every second
// output row from m0r (one output parity).  PRE: pass 0's side inputs were loaded by
// the caller (epi_side_load during its last K-tile) into `pre`.  Pass p + 1's side inputs
// are issued right after pass p's staging barrier, so only the first pass waits on HBM.
// CSG > 1 (round 6, the halo convs): the column sums are kept per thread in registers -- its
// 8-column chunk summed over the rows it stores, across the passes of a 128-row slot -- and
// only at the slot's end do the RPI threads of a chunk column meet through LDS (the staging
// image; a fixed order).  The per-pass form wrote every stored value back to the staging image
// and had BN threads re-read all WTM rows: 10-14 % of the 16x16 halo conv (scripts/cs_cost.py).
// (The caller guarantees (NT / (BN / 8)) x BN x 2 floats of LDS at st.)
template <int BM, int BN, int WM, int WN, bool GEN, bool CSF = false, int RW = 0, bool PRE = false, bool PIPE = true,
          int CSG = 1>
__device__ __forceinline__ void store_tile_plain_pre(const ConvArgs& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16],
                                                     float* st, int m0, int n0, long m0r, int tid_in,
                                                     const EpiSide<EpiGeo<BM, BN, WM, WN>::ITER>& pre) {
  constexpr int NT = WM * WN * 64, WTM = BM / WM, SP = BN + 4;
  constexpr int CPRW = BN / 8;                 // chunk columns per tile row
  constexpr int RPI = NT / CPRW;               // rows per iteration
  constexpr int ITER = (WTM + RPI - 1) / RPI;  // iterations per wave-row pass
  constexpr bool CSOK = CSF || cs_tile_fits<BM, BN, WM, WN>();
  static_assert(!CSF || (CS_ROWS % WTM == 0 && NT >= BN), "column-sum slots of whole wave rows");
  // tile-local row -> output row
  auto out_row = [&](int lr) -> int { return epi_out_row<RW>(a, m0, m0r, lr); };
  const int tid = tid_in >= 0 ? tid_in : (int)threadIdx.x;  // (a caller in a loop passes an opaque copy)
  const int c8 = (tid % CPRW) * 8, r0 = tid / CPRW;
  const int col = n0 + c8;
  const bool cok = (r0 < RPI) && col < a.N;
  const bool cs_on = CSOK && a.cs_out != nullptr;
  float g1 = 0.f, g2 = 0.f;  // column tid's sums over the slot's passes so far
  float q1[8], q2[8];        // (CSG > 1) this thread's chunk sums over its stored rows of the slot
#pragma unroll
  for (int j = 0; j < 8; ++j) { q1[j] = 0.f; q2[j] = 0.f; }
  // row vector (per-frame temb / positional-encoding rows): one row for the whole
  // tile in the common case (rows_per_vec >= the tile's row span), folded into
  // the per-column constants; otherwise looked up per row.
  const int last_row = RW == RW_POS ? out_row(min(BM, a.n_img - m0) - 1) : RW != 0 ? out_row(BM - 1) : min(m0 + BM, a.M) - 1;
  const bool rv_tile = a.rowvec && out_row(0) / a.rows_per_vec == last_row / a.rows_per_vec;
  float bb[8], cs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { bb[j] = 0.f; cs[j] = 0.f; }
  if (cok && a.bias) load8f(a.bias + col, bb);
  if (cok && rv_tile) {
    float rv[8];
    load8f(a.rowvec + rv_row(a, out_row(0)) + col, rv);
#pragma unroll
    for (int j = 0; j < 8; ++j) bb[j] += rv[j];
  }
  if (cok && a.ln_mr) load8f(a.ln_cs + col, cs);
  // no LayerNorm fold, no per-row row vector, unit output scale: the short path
  // (position-major: a row vector per row is added to the column constants first, as the
  // standard raster does for its tile -- there a 256-row tile never straddles two row vectors,
  // posmajor_ok -- so both forms round alike)
  const bool plain = !a.ln_mr && !(RW != RW_POS && a.rowvec && !rv_tile) && a.out_scale == 1.f && !(a.ablate & 8);
  EpiSide<ITER> cur;
  if constexpr (PRE) cur = pre;
  else if constexpr (PIPE) epi_side_load<BM, BN, WM, WN, RW>(a, m0, n0, m0r, tid, 0, cur);
#pragma unroll 1
  for (int p = 0; p < WM; ++p) {
    stage_acc<BM, BN, WM, WN>(acc, st, p, tid);
    // (no pipelining: this pass's residual after its staging writes, as the accumulators
    // it staged are dead -- the 256 x 256 tile has no registers to spare before that)
    if constexpr (!PIPE && !PRE) epi_side_load<BM, BN, WM, WN, RW>(a, m0, n0, m0r, tid, p, cur);
    float2 mr[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int rl = r0 + it * RPI, row = out_row(p * WTM + rl);
      mr[it] = make_float2(0.f, 1.f);
      if (cok && rl < WTM && row < a.Mo && a.ln_mr) mr[it] = *(const float2*)(a.ln_mr + 2L * row);
    }
    __syncthreads();
    EpiSide<ITER> nxt;
    if (PIPE && p + 1 < WM) epi_side_load<BM, BN, WM, WN, RW>(a, m0, n0, m0r, tid, p + 1, nxt);
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int rl = r0 + it * RPI, row = out_row(p * WTM + rl);
      if (!(cok && rl < WTM && row < a.Mo)) continue;
      const float* s = st + rl * SP + c8;
      const float4 s0 = *(const float4*)s, s1 = *(const float4*)(s + 4);
      float v[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
      float r8[8];
      unpack8(cur.rs[it], r8);
      if (RW == RW_POS && a.rowvec && !rv_tile) {  // (block-uniform)
        float rv[8];
        load8f(a.rowvec + rv_row(a, row) + col, rv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float b = bb[j] + rv[j];
          v[j] = plain ? (v[j] + b) + r8[j] : (v[j] + b + 0.f + r8[j]) * a.out_scale;
        }
      } else if (plain) {  // (block-uniform) bias (+ the tile's row vector) + residual: 2 VALU per value
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (v[j] + bb[j]) + r8[j];
      } else {
        float rv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) rv[j] = 0.f;
        if (a.rowvec && !rv_tile) load8f(a.rowvec + rv_row(a, row) + col, rv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x = mr[it].y * (v[j] - mr[it].x * cs[j]);
          v[j] = (x + bb[j] + rv[j] + r8[j]) * a.out_scale;
        }
      }
      if (GEN) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = act_fn(a.act, v[j]);
      }
      if (a.ablate & 4) {
        if (v[0] == 12345.f) ((float*)a.y)[0] = v[1];
      } else if (GEN && a.y_f32) {
        float* y = (float*)a.y + (long)row * a.ldy + col;
        *(float4*)y = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(y + 4) = make_float4(v[4], v[5], v[6], v[7]);
      } else {
        const uint4 pk = pack8(v);
        *(uint4*)((u16*)a.y + (long)row * a.ldy + col) = pk;
        if (cs_on) {
          float b[8];
          unpack8(pk, b);
          if constexpr (CSG > 1) {  // sums of the stored (bf16) values, in registers
#pragma unroll
            for (int j = 0; j < 8; ++j) { q1[j] += b[j]; q2[j] = fmaf(b[j], b[j], q2[j]); }
          } else {  // the stored values replace their fp32 staging
            float* sw = st + rl * SP + c8;
            *(float4*)sw = make_float4(b[0], b[1], b[2], b[3]);
            *(float4*)(sw + 4) = make_float4(b[4], b[5], b[6], b[7]);
          }
        }
      }
    }
    __syncthreads();
    if (cs_on && CSG > 1) {  // (block-uniform) the slot's end: the RPI chunk partials of a column meet
      if (((p + 1) * WTM) % CS_ROWS == 0) {
        float2* const part = (float2*)st;  // [RPI][BN] (sum, sum of squares)
        if (cok) {
#pragma unroll
          for (int j = 0; j < 8; ++j) part[r0 * BN + c8 + j] = make_float2(q1[j], q2[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { q1[j] = 0.f; q2[j] = 0.f; }
        __syncthreads();
        if (tid < BN && n0 + tid < a.N) {
          float t1 = 0.f, t2 = 0.f;
#pragma unroll 5
          for (int r = 0; r < RPI; ++r) {
            const float2 v = part[r * BN + tid];
            t1 += v.x;
            t2 += v.y;
          }
          float* o = a.cs_out + (m0 + (long)p * WTM) / CS_ROWS * 2 * a.N + n0 + tid;
          o[0] = t1;
          o[a.N] = t2;
        }
        __syncthreads();  // the next pass stages into st
      }
    } else if (cs_on) {  // (block-uniform)
      const bool mine = tid < BN && n0 + tid < a.N;
      if (mine) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll 8
        for (int r = 0; r < WTM; ++r) {
          const float x = st[r * SP + tid];
          t1 += x;
          t2 = fmaf(x, x, t2);
        }
        g1 += t1;
        g2 += t2;
      }
      if (((p + 1) * WTM) % CS_ROWS == 0) {  // the slot is complete
        if (mine) {
          float* o = a.cs_out + (m0 + (long)p * WTM) / CS_ROWS * 2 * a.N + n0 + tid;
          o[0] = g1;
          o[a.N] = g2;
        }
        g1 = 0.f;
        g2 = 0.f;
      }
      __syncthreads();
    }
    if constexpr (PIPE) {
      if (p + 1 < WM) cur = nxt;
    }
  }
}

template <int BM, int BN, int WM, int WN, bool GEN, bool CSF = false, int RW = 0, int CSG = 1>
__device__ __forceinline__ void store_tile_plain(const ConvArgs& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16],
                                                 float* st, int m0, int n0, long m0r = 0, int tid_in = -1) {
  // (the 8-wave 256 x 256 tile runs at the 256-VGPR limit: its next pass's residual loads
  // would spill, so they stay in the pass)
  EpiSide<EpiGeo<BM, BN, WM, WN>::ITER> none;
  store_tile_plain_pre<BM, BN, WM, WN, GEN, CSF, RW, false, !(BM == 256 && WM == 2), CSG>(a, acc, st, m0, n0, m0r,
                                                                                          tid_in, none);
}

// GEGLU variant: a thread owns one 8-wide OUTPUT chunk, i.e. packed columns
// [ph, ph+8) (h) and [ph+16, ph+24) (g) of the 16-row-interleaved W1.
template <int BM, int BN, int WM, int WN, bool GEN>
__device__ __forceinline__ void store_tile_geglu(const ConvArgs& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16],
                                                 float* st, int m0, int n0) {
  constexpr int NT = WM * WN * 64, WTM = BM / WM, SP = BN + 4;
  constexpr int CPRW = BN / 16;
  constexpr int RPI = NT / CPRW;
  constexpr int ITER = (WTM + RPI - 1) / RPI;
  const int tid = threadIdx.x;
  const int o8 = (tid % CPRW) * 8, r0 = tid / CPRW;
  const int ph = (o8 >> 4) * 32 + (o8 & 15);
  const int col = n0 + ph;                       // packed column of h
  const int oc = (col >> 5) * 16 + (col & 15);   // output column
  const bool cok = (r0 < RPI) && col < a.N;
  float bh[8], bg[8], ch[8], cg[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { bh[j] = 0.f; bg[j] = 0.f; ch[j] = 0.f; cg[j] = 0.f; }
  if (cok && a.bias) { load8f(a.bias + col, bh); load8f(a.bias + col + 16, bg); }
  if (cok && a.ln_mr) { load8f(a.ln_cs + col, ch); load8f(a.ln_cs + col + 16, cg); }
#pragma unroll 1
  for (int p = 0; p < WM; ++p) {
    stage_acc<BM, BN, WM, WN>(acc, st, p, tid);
    const int rbase = m0 + p * WTM;
    float2 mr[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int rl = r0 + it * RPI, row = rbase + rl;
      mr[it] = make_float2(0.f, 1.f);
      if (cok && rl < WTM && row < a.M && a.ln_mr) mr[it] = *(const float2*)(a.ln_mr + 2L * row);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int rl = r0 + it * RPI, row = rbase + rl;
      if (!(cok && rl < WTM && row < a.M)) continue;
      const float* s = st + rl * SP + ph;
      float h[8], g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        h[j] = mr[it].y * (s[j] - mr[it].x * ch[j]) + bh[j];
        g[j] = mr[it].y * (s[16 + j] - mr[it].x * cg[j]) + bg[j];
        h[j] *= gelu_erf(g[j]);
      }
      if (GEN && a.y_f32) {
        float* y = (float*)a.y + (long)row * a.ldy + oc;
        *(float4*)y = make_float4(h[0], h[1], h[2], h[3]);
        *(float4*)(y + 4) = make_float4(h[4], h[5], h[6], h[7]);
      } else {
        *(uint4*)((u16*)a.y + (long)row * a.ldy + oc) = pack8(h);
      }
    }
    __syncthreads();
  }
}

// Stage the accumulator tile through LDS one wave-row (WTM rows) at a time, then
// each thread handles whole 8-column chunks (split-K slab / GEGLU / plain).
// EPI selects the epilogue compiled into a kernel instance (host: epi_kind()), so
// the common instances carry only the code they run -- the fully general
// epilogue is ~40 KB of code, and fetching it per tile cost more than the
// MFMAs of a K = 320 tile.
//   EPI_PLAIN: vectorised, no split-K, no activation, bf16 out (bias / rowvec /
//              residual / LayerNorm fold as runtime options);
//   EPI_GEGLU: the same for the GEGLU epilogue;
//   EPI_ANY:   everything (split-K slabs, GELU/SiLU, fp32 out, ragged N).
//   EPI_PLAINP: EPI_PLAIN for the tiled phase form of an upsample conv: the block's parity is
//              its grid slice (tile_phase) and the rows go through epi_out_row<RW_PHASE>.
enum { EPI_PLAIN = 0, EPI_GEGLU = 1, EPI_ANY = 2, EPI_PLAINP = 3 };

// EPI_PLAINP: the grid is 4 x ntm x ntn (no split-K), the slice index z is the parity: point the
// kernel's own copy of the arguments at the parity's weights and rows
template <int EPI>
__device__ __forceinline__ void tile_phase(ConvArgs& a, int& z) {
  if constexpr (EPI == EPI_PLAINP) {
    a.w += (long)z * a.N * a.K;
    a.phase = 1 + z;
    z = 0;
  }
}

// RW = RW_POS (the position-major form; the plan has no split-K, 16-B rows, no GEGLU): m0 is the
// tile's first frame and m0r its pixel position.
template <int BM, int BN, int WM, int WN, int EPI = EPI_ANY, int RW = 0>
__device__ __forceinline__ void store_tile(const ConvArgs& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16], float* st,
                                           int m0, int n0, int z, long m0r = 0) {
  if constexpr (EPI == EPI_PLAIN) {
    // (the 4 x 2-wave 256-row tile keeps 64-row wave rows: column sums in its epilogue too)
    store_tile_plain<BM, BN, WM, WN, false, BM == 256 && WM == 4, RW>(a, acc, st, m0, n0, m0r);
    return;
  } else if constexpr (RW == RW_POS) {
    static_assert(EPI == EPI_ANY, "position-major: the plain or the general epilogue");
    store_tile_plain<BM, BN, WM, WN, true, false, RW>(a, acc, st, m0, n0, m0r);
    return;
  } else if constexpr (EPI == EPI_GEGLU) {
    store_tile_geglu<BM, BN, WM, WN, false>(a, acc, st, m0, n0);
    return;
  } else if constexpr (EPI == EPI_PLAINP) {  // (no column sums: the host runs the read pass)
    store_tile_plain<BM, BN, WM, WN, false, false, RW_PHASE>(a, acc, st, m0, n0);
    return;
  }
  constexpr int NT = WM * WN * 64;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr int SP = BN + 4;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const bool vec = (a.N % 8 == 0) && (a.ldy % 8 == 0) && (!a.res || a.ldr % 8 == 0);
  const bool geglu = a.act == LS_ACT_GEGLU;
  if (a.split == 1 && vec) {
    if (geglu) store_tile_geglu<BM, BN, WM, WN, true>(a, acc, st, m0, n0);
    else store_tile_plain<BM, BN, WM, WN, true>(a, acc, st, m0, n0);
    return;
  }
#pragma unroll 1
  for (int p = 0; p < WM; ++p) {
    if (wm == p) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            st[(i * 16 + (lane >> 4) * 4 + r) * SP + wn * WTN + j * 16 + (lane & 15)] = acc[i][j][r];
    }
    __syncthreads();
    const int rbase = m0 + p * WTM;
    if (a.split > 1) {
      float* P = a.partial + (long)z * a.M * a.N;
      for (int q = tid; q < WTM * (BN / 8); q += NT) {
        const int r = q / (BN / 8), c8 = (q - r * (BN / 8)) * 8;
        const int row = rbase + r, col = n0 + c8;
        if (row >= a.M || col >= a.N) continue;
        const float* s = st + r * SP + c8;
        if (vec) {
          *(float4*)(P + (long)row * a.N + col) = *(const float4*)s;
          *(float4*)(P + (long)row * a.N + col + 4) = *(const float4*)(s + 4);
        } else {
          for (int j = 0; j < 8 && col + j < a.N; ++j) P[(long)row * a.N + col + j] = s[j];
        }
      }
    } else if (geglu) {
      for (int q = tid; q < WTM * (BN / 16); q += NT) {
        const int r = q / (BN / 16), o8 = (q - r * (BN / 16)) * 8;
        const int ph = (o8 >> 4) * 32 + (o8 & 15);
        const int row = rbase + r, col = n0 + ph;
        if (col >= a.N) continue;
        float h[8], g[8];
        const float* s = st + r * SP + ph;
#pragma unroll
        for (int j = 0; j < 8; ++j) { h[j] = s[j]; g[j] = s[16 + j]; }
        epi_geglu8(a, row, col, h, g, vec);
      }
    } else {
      for (int q = tid; q < WTM * (BN / 8); q += NT) {
        const int r = q / (BN / 8), c8 = (q - r * (BN / 8)) * 8;
        const int row = rbase + r, col = n0 + c8;
        if (col >= a.N) continue;
        float v[8];
        const float* s = st + r * SP + c8;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s[j];
        epi_chunk(a, row, col, v, vec && col + 8 <= a.N);
      }
    }
    __syncthreads();
  }
}

// XCD-aware block order: blocks b and b+8 share an XCD under round-robin
// dispatch, so give every XCD a contiguous range of tiles (shared A rows /
// 3x3 halos / weight panels stay in one L2).  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = b % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + b / 8;
}

// buffer_load_dwordx4 into registers (the LDS-DMA form is ls_common.h's ls_raw_buffer_load_lds)
__device__ i32x4 ls_raw_buffer_load_v4(i32x4 rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.buffer.load.v4i32");

// Out-of-range / padding operand pieces of the global -> LDS DMA read this zero page.  One copy
// per translation unit: without relocatable device code a kernel only sees its own unit's.
// `inline`, not `static`: the host shadow symbols of the units merge at the link, and the device
// symbol stays protected, addressed PC-relative (a static one is externalised with default
// visibility and every use loads its address through the GOT).
inline __device__ uint4 ls_zero_page[2];

// ---------------------------------------------------------------- host side
// The tuning switches of ls_set_tuning: ONE object (g_tune, defined in ls_conv.hip), so that a
// key acts in whichever translation unit reads it.
struct ConvTuning {
  bool force_regstage = false;  // tuning key 1
  int force_tile = 0, force_split = 0;  // tuning keys 2, 3
  // ablation bits (diagnostics; tuning key 4): 1 no MFMA, 2 no operand DMA,
  // 4 no output store, 8 the general epilogue arithmetic even where the short path applies
  int ablate = 0;
  // ---- row-block GEMM (gemm_rowblock_kernel)
  bool rowblock = true;     // tuning key 6
  bool rowblock640 = true;  // tuning key 7
  bool rb640_res = false;   // tuning key 20: K = 640 residual GEMMs too
  // K = 640 with two 16-row fragments per wave (256-row blocks, half the W-fragment LDS reads
  // per MFMA, 160 A registers): default since r04x (step 215.3 -> 212.2 ms at 48 windows, three
  // same-box alternations); tuning key 15 = 0: one fragment per wave
  bool rb640_fm2 = true;
  // ---- halo-tile 3x3 conv (conv3x3_halo_kernel)
  bool halo = true;  // tuning key 8
  // the nearest-x2 upsample convs on the halo kernel too (tuning key 18; off: the tiled gather)
  bool halo_ups = true;
  // tuning key 13: 128-channel tiles where both divide N (3-slot weight ring instead of 2 at
  // BN 160)
  bool halo_bn128 = false;
  // the narrow 16-column tile for N <= 16 (tuning key 19; off: the tiled GEMM's 128 x 32 tile)
  bool halo_narrow = true;
  // 16 x 8 patches, two blocks per CU for the 128-column tiles of convs with at most 4 input
  // chunks (Cin <= 256), where a block's halo prologue and epilogue are a large share of its
  // time: VAE 128 ch at 256^2 17.67 -> 17.23 ms, 128 -> 256 at 128^2 8.74 -> 8.43 ms, 256 at
  // 128^2 a tie; at Cin 512 (8 chunks) the 2-slot weight ring loses to the 1-block form's 3
  // slots (13.12 -> 13.55 ms at 64^2), profiles/r05k_halo_ab.txt.  Tuning key 16 = 0: off.
  bool halo_th8 = true;
  // ---- position-major 3x3 conv on the 256-row tiles (tuning key 22): 0 never, 1 where the
  // cost model prefers it (posmajor_cost), 2 wherever it is legal (posmajor_ok)
  int posmajor = 1;
};
extern ConvTuning g_tune;

// The plan of one ls_conv2d call.  plan_conv takes every decision once -- the kernel family,
// the instance within it, the launch geometry and the passes that follow -- and ls_conv2d,
// ls_conv_path, ls_conv_plan and ls_conv_workspace_bytes all read that one answer.
struct ConvPlan {
  ConvArgs a;           // exactly as the kernel receives it
  ls_conv_plan_info i;  // family, instance, geometry, trailing passes (ls_hip.h)
  float* cs_pass;       // launch_colsum_pass over the stored y (i.colsum_rows rows) into this, or null
  float* row_stats;     // ls_row_stats of the stored y into this, or null
};

template <int V>
using IC = std::integral_constant<int, V>;

// launches the plan's kernel instance with the plan's geometry
template <void (*KERN)(ConvArgs)>
static void launch_plan(const ConvPlan& p, hipStream_t s) {
  if (p.i.lds_bytes) LS_SET_MAX_DYN_SHM(KERN, p.i.lds_bytes);
  KERN<<<p.i.grid, p.i.threads, p.i.lds_bytes, s>>>(p.a);
}

// 16-B rows in the epilogue (else the tiled kernels store element by element)
static bool vec_ok(const ConvArgs& a) { return a.N % 8 == 0 && a.ldy % 8 == 0 && (!a.res || a.ldr % 8 == 0); }

// ---- tiled kernels (conv_gemm_kernel, conv_gemm_dma_kernel, conv_gemm_big_kernel)
// dynamic LDS of the DMA kernels: two stages of 64-deep K-tiles; staging for the epilogue
// (the bm / wm rows of a wave row; 128 in the 8-wave 256-row kernels) must fit too
constexpr size_t tiled_lds(int bm, int bn, int wm) {
  return std::max<size_t>((size_t)2 * (bm + bn) * 8 * 16, (size_t)(bm / wm) * (bn + 4) * 4);
}

template <typename K>
static int occ(K kern, int threads, size_t shm) {
  int n = 0;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, threads, shm) != hipSuccess) return -1;
  return n;
}

// ---- what each family's translation unit gives the planner (ls_conv.hip)
bool rowblock_ok(const ls_conv_desc* d, const ConvArgs& a);  // ls_conv_rowblock.hip
bool plan_rowblock(ConvPlan& p);
void launch_rowblock(const ConvPlan& p, hipStream_t s);
bool halo_ok(const ls_conv_desc* d, const ConvArgs& a);  // ls_conv_halo.hip
void plan_halo(ConvPlan& p);
void launch_halo(const ConvPlan& p, hipStream_t s);
void launch_tiled(const ConvPlan& p, hipStream_t s);  // ls_conv_tiled.hip (forwards the 256-row tiles)
int tiled_occupancy(int bn);                          // ... of the 128 x bn 1x1 EPI_PLAIN instance
void launch_big(const ConvPlan& p, hipStream_t s);    // ls_conv_big.hip
int big_occupancy();                                  // ... of the 256 x 256 1x1 EPI_PLAIN instance

}  // namespace ls
