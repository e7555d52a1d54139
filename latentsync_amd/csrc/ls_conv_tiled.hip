// The 128- and 64-row tiles of the implicit-GEMM conv / linear: conv_gemm_kernel (operands
// staged through registers: the GroupNorm affine prologue) and conv_gemm_dma_kernel.
//
// Tile: BM x BN x 64, 4 waves (256 threads) of (BM/WM) x (BN/WN) each, fp32
// accumulators in registers, register-staged double-buffered LDS (one barrier
// per K-tile: the next tile's global loads are issued before the MFMAs of the
// current one).  LDS rows are 128 B (64 bf16) and XOR-swizzled at 16-B chunk
// granularity (chunk ^ ((row >> 1) & 7)) so the ds_read_b128 fragment reads of
// a 16-lane group hit 16 distinct 4-bank slots.
#include "ls_conv_tiled.h"

namespace ls {

template <int KS, bool TAPU>
__device__ __forceinline__ uint4 load_a_chunk(const ConvArgs& a, int kt, int ch, int m, const RowGeo& g) {
  int c, tap = 0;
  if (KS == 1) {
    c = kt * 64 + ch * 8;
    if (m >= a.M || c >= a.Cin) return make_uint4(0, 0, 0, 0);
  } else if (TAPU) {
    tap = tap_of(a, kt * 64, c);
    c += ch * 8;
  } else {
    const int kc = kt * 8 + ch;
    tap = kc / a.CC;
    c = (kc - tap * a.CC) * 8;
    if (tap >= 9) return make_uint4(0, 0, 0, 0);
  }
  long pix;
  if (KS == 1) {
    pix = m;
  } else {
    const int kh = tap / 3, kw = tap - kh * 3;
    int yy = g.yb + kh, xx = g.xb + kw;
    if (a.upsample) {
      if ((unsigned)yy >= (unsigned)(2 * a.H) || (unsigned)xx >= (unsigned)(2 * a.W)) return make_uint4(0, 0, 0, 0);
      yy >>= 1; xx >>= 1;
    } else {
      if ((unsigned)yy >= (unsigned)a.H || (unsigned)xx >= (unsigned)a.W) return make_uint4(0, 0, 0, 0);
    }
    pix = (long)g.pb + yy * a.W + xx;
  }
  uint4 v;
  if (c < a.C1) v = *(const uint4*)(a.x1 + pix * a.ld1 + c);
  else v = *(const uint4*)(a.x2 + pix * a.ld2 + (c - a.C1));
  if (a.aff_scale) {
    const long s = pix / a.pix_per_sample;
    float scl[8], shf[8], f[8];
    load8f(a.aff_scale + s * a.Cin + c, scl);
    load8f(a.aff_shift + s * a.Cin + c, shf);
    unpack8(v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = f[j] * scl[j] + shf[j];
      f[j] = a.silu_in ? silu(t) : t;
    }
    v = pack8(f);
  }
  return v;
}

template <int BM, int BN, int WM, int WN, int KS, bool TAPU>
__global__ void __launch_bounds__(256) conv_gemm_kernel(ConvArgs a) {
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr int AL = BM / 32, BL = BN / 32;  // 16-B chunks per thread per K-tile
  constexpr int SP = BN + 4;                 // epilogue staging pitch (floats)
  static_assert(WTM * SP * 4 <= 2 * (BM + BN) * 8 * 16, "staging must fit the LDS ring");
  __shared__ uint4 lds[2][(BM + BN) * 8];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  int bid = blockIdx.x;
  const int nt = a.ntm * a.ntn;
  const int z = bid / nt;
  bid -= z * nt;
  int tm, tn;
  tile_of(a, bid, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int kt0 = z * a.kt_per_split;
  const int kt1 = min(a.ktiles, kt0 + a.kt_per_split);

  const int ch = tid & 7;
  int rm[AL];
  RowGeo geo[AL];
#pragma unroll
  for (int i = 0; i < AL; ++i) {
    const int m = m0 + (tid >> 3) + 32 * i;
    rm[i] = m;
    if (KS == 3) {
      const int hw = a.Ho * a.Wo;
      const int n = m / hw, r = m - n * hw;
      const int yo = r / a.Wo, xo = r - yo * a.Wo;
      geo[i].pb = n * a.H * a.W;
      geo[i].yb = (m < a.M) ? (a.upsample ? yo - a.pad : yo * a.stride - a.pad) : -(1 << 28);
      geo[i].xb = a.upsample ? xo - a.pad : xo * a.stride - a.pad;
    } else {
      geo[i].pb = 0; geo[i].yb = 0; geo[i].xb = 0;
    }
  }

  uint4 ra[AL], rb[BL];
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < AL; ++i) ra[i] = load_a_chunk<KS, TAPU>(a, kt, ch, rm[i], geo[i]);
#pragma unroll
    for (int j = 0; j < BL; ++j) {
      const int n = n0 + (tid >> 3) + 32 * j;
      rb[j] = (n < a.N) ? *(const uint4*)(a.w + (long)n * a.K + kt * 64 + ch * 8) : make_uint4(0, 0, 0, 0);
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AL; ++i) lds[buf][swz((tid >> 3) + 32 * i, ch)] = ra[i];
#pragma unroll
    for (int j = 0; j < BL; ++j) lds[buf][BM * 8 + swz((tid >> 3) + 32 * j, ch)] = rb[j];
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (kt0 < kt1) {
    gload(kt0);
    sstore(0);
    __syncthreads();
    int cur = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
      const bool more = kt + 1 < kt1;
      if (more) gload(kt + 1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int c = ks * 4 + (lane >> 4);
        bf16x8 af[FM], bfr[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i)
          af[i] = __builtin_bit_cast(bf16x8, lds[cur][swz(wm * WTM + i * 16 + (lane & 15), c)]);
#pragma unroll
        for (int j = 0; j < FN; ++j)
          bfr[j] = __builtin_bit_cast(bf16x8, lds[cur][BM * 8 + swz(wn * WTN + j * 16 + (lane & 15), c)]);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
      if (more) sstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }

  store_tile<BM, BN, WM, WN>(a, acc, (float*)&lds[0][0], m0, n0, z);
}

// ------------------------------------------------------------------ DMA path
// Same tiles / LDS image / epilogue, but both operands stream global -> LDS with
// global_load_lds_dwordx4 (no VGPR staging, no ds_write).  The LDS image is
// written lane-linearly, so the XOR swizzle is applied on the per-lane SOURCE
// address (logical chunk = physical chunk ^ ((row >> 1) & 7)).  Out-of-range /
// padding taps read a zero page.  Two LDS buffers: tile k+1's DMA overlaps tile
// k's MFMAs; counted vmcnt + raw s_barrier so the in-flight tile is not drained.
// BUF: operand DMA through buffer descriptors (host: buf_dma_ok) -- every per-thread
// byte offset is computed once; a K-tile only changes the uniform soffset (and, for
// a 3x3 tap, one select per piece between the precomputed window offset and an
// out-of-range offset that reads zeros), so the K loop carries no 64-bit address
// arithmetic: ~90-125 VALU per K-tile less than the global_load_lds path, which
// competes with the MFMAs for vector issue.  1x1: A rows of the tile from a
// descriptor at row m0 (rows past M read zeros), B rows from one at column n0.
// 3x3 (stride 1 / 2, pad 0 / 1, C1 % 64 == 0): the descriptor starts pad (W + 1)
// pixels before the tile's first input image, so every window's top-left pixel has
// a non-negative offset; the tap's (kh W + kw) pixel shift and channel offset go in
// soffset, taps outside the image select an offset past the descriptor (zeros).
template <int BM, int BN, int WM, int WN, int KS, bool TAPU, int EPI, bool BUF = false>
__global__ void __launch_bounds__(WM * WN * 64) conv_gemm_dma_kernel(ConvArgs a) {
  constexpr int NST = 2, BK = 64;                     // LDS stages, K-tile depth (what ships)
  constexpr int NT = WM * WN * 64;                    // 256 (4 waves) or 512 (8 waves, 256-row tiles)
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr int CPR = BK / 8;                         // 16-B chunks per row
  constexpr int AI = BM * CPR / NT, BI = BN * CPR / NT;  // DMA wave-instructions per wave per K-tile
  static_assert((BM * CPR) % NT == 0 && (BN * CPR) % NT == 0, "operand pieces must divide over the threads");
  constexpr int L = AI + BI;
  constexpr int KSTEPS = BK / 32;
  constexpr int STAGE = (BM + BN) * CPR;              // uint4 per stage
  extern __shared__ __attribute__((aligned(16))) uint4 lds_dyn[];
  uint4* lds = lds_dyn;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int nt = a.ntm * a.ntn;
  int bid = xcd_remap(blockIdx.x, nt * (EPI == EPI_PLAINP ? 4 : a.split));
  int z = bid / nt;
  bid -= z * nt;
  tile_phase<EPI>(a, z);
  int tm, tn;
  tile_of(a, bid, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int ktiles = a.K / BK;
  const int kps = a.kt_per_split * (64 / BK);
  const int kt0 = z * kps;
  const int kt1 = min(ktiles, kt0 + kps);

  int arow[AI], ach[AI], brow[BI], bch[BI];
  RowGeo geo[AI];
#pragma unroll
  for (int p = 0; p < AI; ++p) {
    const int q = (wid * AI + p) * 64 + lane;
    const int row = q / CPR;
    const int pc = q % CPR;
    arow[p] = m0 + row;
    ach[p] = swz64(row, pc) - row * CPR;  // logical chunk stored at physical chunk pc (involution)
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
  BufDma<BM, BN, AI, BI, KS> bd;  // BUF (dead code otherwise)
  if constexpr (BUF) {
    int ar[AI], br[BI];
#pragma unroll
    for (int p = 0; p < AI; ++p) ar[p] = arow[p] - m0;
#pragma unroll
    for (int p = 0; p < BI; ++p) br[p] = brow[p] - n0;
    bd.init(a, m0, n0, ar, ach, br, bch);
  }
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  auto issue = [&](int kt, int stage) {
    uint4* base = lds + stage * STAGE;
    if constexpr (BUF) {
      bd.issue(a, kt, base, base + BM * CPR, wid_u);
    } else {
#pragma unroll
      for (int p = 0; p < AI; ++p)
        glds16(a_src<KS, TAPU>(a, kt, ach[p], arow[p], geo[p]), base + (wid * AI + p) * 64);
#pragma unroll
      for (int p = 0; p < BI; ++p) {
        const void* src = brow[p] < a.N ? (const void*)(a.w + (long)brow[p] * a.K + kt * BK + bch[p] * 8)
                                        : (const void*)ls_zero_page;
        glds16(src, base + BM * CPR + (wid * BI + p) * 64);
      }
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const bool do_dma = !(a.ablate & 2);
#pragma unroll
  for (int t = 0; t < NST - 1; ++t)
    if (kt0 + t < kt1 && do_dma) issue(kt0 + t, t);
  // ILV: the next K-tile's DMA issued after this K-tile's barrier instead of in one burst before
  // the wait; measured and rejected.  The constant and its dead second
  // issue() call site stay: without them the compiler orders two v_mov of the EPI_ANY instances'
  // epilogue differently, and the shipped instructions are held fixed.
  constexpr bool ILV = false;
  int stage = 0;
  // the plain epilogue's first-pass side inputs (residual / LayerNorm rows), loaded during
  // the last K-tile so their HBM latency hides under its MFMAs
  EpiSide<EpiGeo<BM, BN, WM, WN>::ITER> pre;
  // one K-tile; IS: issue the next K-tile's DMA inside it (ILV).  (Peeling the last K-tile so
  // that the DMA and the MFMAs share one basic block made the register allocator rotate the
  // accumulators through AGPR moves, ~90 per K-tile: not kept.)
  auto ktile = [&](int kt, auto is_tag) {
    constexpr bool IS = decltype(is_tag)::value;
    if (!ILV && kt + NST - 1 < kt1 && do_dma) issue(kt + NST - 1, (stage + NST - 1) % NST);
    const int ahead = ILV ? 0 : min(NST - 1, kt1 - 1 - kt);
    if (ahead >= 1) wait_vm<L>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (EPI == EPI_PLAIN) {
      if (kt == kt1 - 1) epi_side_load<BM, BN, WM, WN>(a, m0, n0, 0, tid, 0, pre);
    }
    const uint4* cur = lds + stage * STAGE;
    bf16x8 af[KSTEPS][FM], bfr[KSTEPS][FN];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int c = ks * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < FM; ++i)
        af[ks][i] = __builtin_bit_cast(bf16x8, cur[swz64(wm * WTM + i * 16 + (lane & 15), c)]);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        bfr[ks][j] = __builtin_bit_cast(bf16x8, cur[BM * CPR + swz64(wn * WTN + j * 16 + (lane & 15), c)]);
    }
    if (ILV && IS && kt + 1 < kt1 && do_dma) issue(kt + 1, stage ^ 1);
#ifdef LS_GEMM_ABLATE
    if (!(a.ablate & 16))
#endif
    {
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][i], bfr[ks][j], acc[i][j], 0, 0, 0);
    }
#ifdef LS_GEMM_ABLATE
    if (a.ablate & 32) {
      acc[0][0][0] += (float)af[0][0][0] + (float)bfr[0][0][0];
    }
#endif
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stage = stage + 1 == NST ? 0 : stage + 1;
  };
  for (int kt = kt0; kt < kt1; ++kt) ktile(kt, std::true_type{});
#ifdef LS_GEMM_ABLATE  // diagnostic build only (hipcc -DLS_GEMM_ABLATE): it costs registers
  if (a.ablate & 8) {  // tuning: no epilogue at all (keep the accumulators live)
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) t += acc[i][j][0] + acc[i][j][3];
    if (t == 12345.f) ((float*)a.y)[tid] = t;
    return;
  }
#endif
  if constexpr (EPI == EPI_PLAIN) {
    if (kt0 < kt1) {
      store_tile_plain_pre<BM, BN, WM, WN, false, BM == 256 && WM == 4, 0, true>(a, acc, (float*)lds, m0, n0, 0, -1,
                                                                                 pre);
      return;
    }
  }
  store_tile<BM, BN, WM, WN, EPI>(a, acc, (float*)lds, m0, n0, z);
}

template <int BM, int BN, int WM, int WN>
static void launch_tiled1(const ConvPlan& p, hipStream_t s) {
  with_gather(p.i, [&](auto ks, auto tapu) {
    constexpr int KS = decltype(ks)::value;
    constexpr bool TAPU = decltype(tapu)::value;
    if (p.i.family == 2) return launch_plan<conv_gemm_kernel<BM, BN, WM, WN, KS, TAPU>>(p, s);
    with_epi_buf<KS, TAPU>(p.i, [&](auto epi, auto buf) {
      constexpr int EPI = decltype(epi)::value;
      constexpr bool BUF = decltype(buf)::value;
      launch_plan<conv_gemm_dma_kernel<BM, BN, WM, WN, KS, TAPU, EPI, BUF>>(p, s);
    });
  });
}

void launch_tiled(const ConvPlan& p, hipStream_t s) {
  const int bm = p.i.bm, bn = p.i.bn;
  if (bm == 256) launch_big(p, s);  // (the 256-row kernels have no register-staged form)
  else if (bm == 128 && bn == 128) launch_tiled1<128, 128, 2, 2>(p, s);
  else if (bm == 128 && bn == 160) launch_tiled1<128, 160, 2, 2>(p, s);
  else if (bm == 128 && bn == 64) launch_tiled1<128, 64, 2, 2>(p, s);
  else if (bm == 128 && bn == 32) launch_tiled1<128, 32, 4, 1>(p, s);
  else launch_tiled1<64, 64, 2, 2>(p, s);
}

int tiled_occupancy(int bn) {
  if (bn == 160) return occ(conv_gemm_dma_kernel<128, 160, 2, 2, 1, false, EPI_PLAIN>, 256, tiled_lds(128, 160, 2));
  return occ(conv_gemm_dma_kernel<128, 128, 2, 2, 1, false, EPI_PLAIN>, 256, tiled_lds(128, 128, 2));
}

}  // namespace ls
