// The 256 x 256 and 256 x 128 tiles of the implicit-GEMM conv / linear (conv_gemm_big_kernel).
#include "ls_conv_tiled.h"

namespace ls {

// 256-row tile, 8 waves (2 M x 4 N), each wave 128 x BN/4 (FM = 8 fragments of
// 16 rows x FN of 16 cols): 1.5x the MFMAs per LDS fragment read of the 4-wave
// 64 x 64 wave tile.  One block per CU (128 KB of LDS: two 64-KB stages at
// BN = 256), glds operand DMA into XOR-swizzled lane-linear images, one raw
// barrier per K-tile; the next tile's DMA is issued right after the barrier so
// it has a whole K-tile of MFMAs to land.  MFMA runs are bracketed by
// s_setprio(1) so the co-resident wave's fragment reads interleave.
// PM: the position-major form of a 3x3 / stride 1 / pad 1 conv (ConvArgs::pm).  The tile is 256
// frames at one pixel position, block -> (position, frame group, column tile) by pm_tile_of; the
// K loop runs the K-tiles of the position's valid taps only (BufDma<PM>::next) -- the ones left
// out added products with a zero A, so the accumulators are bit-identical to the standard raster's.
template <int BN, int KS, bool TAPU, int EPI, bool BUF = false, bool PM = false>
__global__ void __launch_bounds__(512) conv_gemm_big_kernel(ConvArgs a) {
  static_assert(!PM || (KS == 3 && TAPU && BUF), "position-major: channel-chunk-major 3x3 through buffer DMA");
  constexpr int BM = 256, BK = 64, WM = 2, WN = 4;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int FM = WTM / 16, FN = WTN / 16, FH = FM / 2;
  constexpr int CPR = BK / 8;
  constexpr int AI = BM * CPR / 512, BI = BN * CPR / 512;
  constexpr int STAGE = (BM + BN) * CPR;
  extern __shared__ __attribute__((aligned(16))) uint4 lds_dyn[];
  uint4* lds = lds_dyn;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int nt = a.ntm * a.ntn;
  int bid = xcd_remap(blockIdx.x, nt * (EPI == EPI_PLAINP ? 4 : a.split));
  int z = bid / nt;
  bid -= z * nt;
  tile_phase<EPI>(a, z);
  int tm, tn, pos = 0;
  if constexpr (PM) {  // (no split-K; the grid is positions x frame groups x column tiles)
    z = 0;
    pm_tile_of(blockIdx.x, a.H, a.W, a.pm, a.ntn, pos, tm, tn);  // (m0: the tile's first frame)
  } else {
    tile_of(a, bid, tm, tn);
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int kt0 = z * a.kt_per_split;
  int kt1 = min(a.ktiles, kt0 + a.kt_per_split);

  int arow[AI], ach[AI], brow[BI], bch[BI];
  RowGeo geo[AI];
#pragma unroll
  for (int p = 0; p < AI; ++p) {
    const int q = (wid * AI + p) * 64 + lane;
    const int row = q / CPR;
    arow[p] = m0 + row;
    ach[p] = swz64(row, q % CPR) - row * CPR;
    if (KS == 3) {
      const int m = m0 + row;
      const int hw = a.Ho * a.Wo;
      const int n = m / hw, r = m - n * hw;
      const int yo = r / a.Wo, xo = r - yo * a.Wo;
      geo[p].pb = n * a.H * a.W;
      geo[p].yb = (m < a.M) ? (a.upsample ? yo - a.pad : yo * a.stride - a.pad) : -(1 << 28);
      geo[p].xb = a.upsample ? xo - a.pad : xo * a.stride - a.pad;
    } else {
      geo[p].pb = 0; geo[p].yb = 0; geo[p].xb = 0;
    }
  }
#pragma unroll
  for (int p = 0; p < BI; ++p) {
    const int q = (wid * BI + p) * 64 + lane;
    const int row = q / CPR;
    brow[p] = n0 + row;
    bch[p] = swz64(row, q % CPR) - row * CPR;
  }
  static_assert(!BUF || KS == 1 || TAPU, "buffer DMA: 1x1 or tap-major 3x3");
  BufDma<BM, BN, AI, BI, KS, PM> bd;  // BUF (dead code otherwise)
  if constexpr (BUF) {
    int ar[AI], br[BI];
#pragma unroll
    for (int p = 0; p < AI; ++p) ar[p] = arow[p] - m0;
#pragma unroll
    for (int p = 0; p < BI; ++p) br[p] = brow[p] - n0;
    bd.init(a, m0, n0, ar, ach, br, bch, pos);
    if constexpr (PM) kt1 = a.ktiles / 9 * __builtin_popcount(bd.tmask);  // (no split-K: kt0 = 0)
  }
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  auto issue = [&](int kt, int stage) {
    uint4* base = lds + stage * STAGE;
    if constexpr (BUF) {
      bd.issue(a, kt, base, base + BM * CPR, wid_u);
      return;
    }
#pragma unroll
    for (int p = 0; p < AI; ++p)
      glds16(a_src<KS, TAPU>(a, kt, ach[p], arow[p], geo[p]), base + (wid * AI + p) * 64);
#pragma unroll
    for (int p = 0; p < BI; ++p) {
      const void* src = brow[p] < a.N ? (const void*)(a.w + (long)brow[p] * a.K + kt * BK + bch[p] * 8)
                                      : (const void*)ls_zero_page;
      glds16(src, base + BM * CPR + (wid * BI + p) * 64);
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (kt0 < kt1) issue(kt0, 0);
  int stage = 0;
  for (int kt = kt0; kt < kt1; ++kt) {
    wait_vm<0>();  // this wave's share of tile kt has landed
    __builtin_amdgcn_s_barrier();  // ... everyone's, and stage^1 is no longer read
    asm volatile("" ::: "memory");
    if (kt + 1 < kt1) issue(kt + 1, stage ^ 1);
    const uint4* cur = lds + stage * STAGE;
    bf16x8 bfr[2][FN], af[2][FH];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + (lane >> 4);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        bfr[ks][j] = __builtin_bit_cast(bf16x8, cur[BM * CPR + swz64(wn * WTN + j * 16 + (lane & 15), c)]);
#pragma unroll
      for (int i = 0; i < FH; ++i)
        af[ks][i] = __builtin_bit_cast(bf16x8, cur[swz64(wm * WTM + i * 16 + (lane & 15), c)]);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bf16x8 an[2][FH];
      if (h == 0) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int c = ks * 4 + (lane >> 4);
#pragma unroll
          for (int i = 0; i < FH; ++i)
            an[ks][i] = __builtin_bit_cast(bf16x8, cur[swz64(wm * WTM + (FH + i) * 16 + (lane & 15), c)]);
        }
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < FH; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[h * FH + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][i], bfr[ks][j], acc[h * FH + i][j],
                                                                          0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      if (h == 0) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < FH; ++i) af[ks][i] = an[ks][i];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    stage ^= 1;
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  store_tile<BM, BN, WM, WN, EPI, PM ? RW_POS : 0>(a, acc, (float*)lds, m0, n0, z, pos);
}

template <int BN>
static void launch_big1(const ConvPlan& p, hipStream_t s) {
  with_gather(p.i, [&](auto ks, auto tapu) {
    constexpr int KS = decltype(ks)::value;
    constexpr bool TAPU = decltype(tapu)::value;
    with_epi_buf<KS, TAPU>(p.i, [&](auto epi, auto buf) {
      constexpr int EPI = decltype(epi)::value;
      constexpr bool BUF = decltype(buf)::value;
      if constexpr (KS == 3 && TAPU && BUF && (EPI == EPI_PLAIN || EPI == EPI_ANY)) {  // (posmajor_ok)
        if (p.a.pm) return launch_plan<conv_gemm_big_kernel<BN, KS, TAPU, EPI, BUF, true>>(p, s);
      }
      launch_plan<conv_gemm_big_kernel<BN, KS, TAPU, EPI, BUF>>(p, s);
    });
  });
}

void launch_big(const ConvPlan& p, hipStream_t s) {
  if (p.i.bn == 256) launch_big1<256>(p, s);
  else launch_big1<128>(p, s);
}

int big_occupancy() { return occ(conv_gemm_big_kernel<256, 1, false, EPI_PLAIN>, 512, tiled_lds(256, 256, 2)); }

}  // namespace ls
