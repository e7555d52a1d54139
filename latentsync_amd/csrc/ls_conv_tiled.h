// What the two translation units of the tiled GEMMs share (ls_conv_tiled.hip: the 128- and
// 64-row tiles; ls_conv_big.hip: the 256-row tiles): the operand gather and the choice of the
// compiled instance from a plan.
#pragma once
#include "ls_conv.h"

namespace ls {

// ---------------------------------------------------------------- A gather
// Per-row geometry precomputed once per thread: pixel base of the image, and
// the top-left input coordinate of the 3x3 window (or a sentinel for m >= M).
struct RowGeo { int pb, yb, xb; };

template <int KS, bool TAPU>
__device__ __forceinline__ const void* a_src(const ConvArgs& a, int kt, int c, int m, const RowGeo& g) {
  // branch-free: compute the candidate address, then select it or the zero page
  int cg, tap = 0;
  bool ok;
  if (KS == 1) {
    cg = kt * 64 + c * 8;
    ok = (m < a.M) & (cg < a.Cin);
  } else if (TAPU) {
    tap = tap_of(a, kt * 64, cg);
    cg += c * 8;
    ok = true;
  } else {
    const int kc = kt * 8 + c;
    tap = kc / a.CC;
    cg = (kc - tap * a.CC) * 8;
    ok = tap < 9;
  }
  int pix;
  if (KS == 1) {
    pix = m;
  } else {
    const int kh = tap / 3, kw = tap - kh * 3;
    int yy = g.yb + kh, xx = g.xb + kw;
    const int lim_y = a.upsample ? 2 * a.H : a.H, lim_x = a.upsample ? 2 * a.W : a.W;
    ok &= ((unsigned)yy < (unsigned)lim_y) & ((unsigned)xx < (unsigned)lim_x);
    yy >>= a.upsample;
    xx >>= a.upsample;
    pix = g.pb + yy * a.W + xx;
  }
  const bool second = cg >= a.C1;
  const u16* base = second ? a.x2 : a.x1;
  const long off = (long)pix * (second ? a.ld2 : a.ld1) + (second ? cg - a.C1 : cg);
  return ok ? (const void*)(base + off) : (const void*)ls_zero_page;
}

// Operand DMA through buffer descriptors for a BM x BN x 64 tile whose threads each
// move AI A pieces and BI B pieces of 16 B per K-tile (LDS images lane-linear per
// wave, 64 pieces per wave-instruction; the XOR swizzle is folded into the chunk
// offsets ach / bch).  See conv_gemm_dma_kernel's BUF note.
// PM: the position-major form (ConvArgs::pm) -- tile row r is frame m0 + r at pixel `pos`, and
// next() walks only the K-tiles of the taps valid at that pixel (tmask, block-uniform).
template <int BM, int BN, int AI, int BI, int KS, bool PM = false>
struct BufDma {
  i32x4 rs_a1, rs_a2, rs_b;
  int avo1[AI], avo2[AI], bvo[BI];
  unsigned amask[AI];
  int tap = 0, c0 = 0;  // 3x3: tap / channel offset of the next K-tile (next())
  unsigned tmask = 0x1FF;  // PM: the taps inside the image at the tile's pixel

  // arow / brow: tile-relative row of each piece; ach / bch: its logical 16-B chunk
  __device__ __forceinline__ void init(const ConvArgs& a, int m0, int n0, const int* arow, const int* ach,
                                       const int* brow, const int* bch, int pos = 0) {
    const long cap = 0x7FFFFFFFL;
    if (PM) {  // stride 1, pad 1: frame m0 + row, output pixel pos = (yo, xo), window top-left (yo - 1, xo - 1)
      const int HWi = a.H * a.W;
      const long base_pix = (long)m0 * HWi - a.W - 1;
      const long tot_pix = (long)a.n_img * HWi;
      rs_a1 = buffer_rsrc(a.x1 + base_pix * a.ld1, (uint32_t)min((tot_pix - base_pix) * a.ld1 * 2, cap));
      rs_a2 = a.C2 ? buffer_rsrc(a.x2 + base_pix * a.ld2, (uint32_t)min((tot_pix - base_pix) * a.ld2 * 2, cap))
                   : rs_a1;
      tmask = pm_tap_mask(a.H, a.W, pos);
      tap = __builtin_ctz(tmask);
#pragma unroll
      for (int p = 0; p < AI; ++p) {
        const int win = arow[p] * HWi + pos;  // = frame * HWi + (yo - 1) W + xo - 1 - base_pix
        avo1[p] = (win * a.ld1 + ach[p] * 8) * 2;
        avo2[p] = (win * a.ld2 + ach[p] * 8) * 2;
        amask[p] = m0 + arow[p] < a.n_img ? tmask : 0u;
      }
    } else if (KS == 1) {  // (rows of one tile: the concat halves share the row index)
      rs_a1 = buffer_rsrc(a.x1 + (long)m0 * a.ld1, (uint32_t)min((long)(a.M - m0) * a.ld1 * 2, cap));
      rs_a2 = a.C2 ? buffer_rsrc(a.x2 + (long)m0 * a.ld2, (uint32_t)min((long)(a.M - m0) * a.ld2 * 2, cap)) : rs_a1;
#pragma unroll
      for (int p = 0; p < AI; ++p) {
        avo1[p] = (arow[p] * a.ld1 + ach[p] * 8) * 2;
        avo2[p] = (arow[p] * a.ld2 + ach[p] * 8) * 2;
        amask[p] = 0x1FF;
      }
    } else if (a.upsample) {
      // nearest x2 then 3x3 pad 1: upsampled (yo - 1 + kh, xo - 1 + kw) reads input
      // (i - 1 + r, j - 1 + c), i = yo >> 1, r = (py + kh + 1) >> 1 (py = yo & 1), likewise
      // c: the tap's uniform shift r0 W + c0 (py = px = 0) plus W / 1 pixel for the odd
      // rows / columns of taps kh / kw != 1 (parity bits 9 / 10 of amask)
      const int HWi = a.H * a.W, HWo = a.Ho * a.Wo;
      const long base_pix = (long)(m0 / HWo) * HWi - a.W - 1;
      const long tot_pix = (long)a.n_img * HWi;
      rs_a1 = buffer_rsrc(a.x1 + base_pix * a.ld1, (uint32_t)min((tot_pix - base_pix) * a.ld1 * 2, cap));
      rs_a2 = a.C2 ? buffer_rsrc(a.x2 + base_pix * a.ld2, (uint32_t)min((tot_pix - base_pix) * a.ld2 * 2, cap))
                   : rs_a1;
#pragma unroll
      for (int p = 0; p < AI; ++p) {
        const int m = m0 + arow[p];
        const int n = m / HWo, r = m - n * HWo;
        const int yo = r / a.Wo, xo = r - yo * a.Wo;
        const int win = (int)((long)n * HWi + (long)((yo >> 1) - 1) * a.W + ((xo >> 1) - 1) - base_pix);
        avo1[p] = (win * a.ld1 + ach[p] * 8) * 2;
        avo2[p] = (win * a.ld2 + ach[p] * 8) * 2;
        unsigned mk = ((unsigned)(yo & 1) << 9) | ((unsigned)(xo & 1) << 10);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const bool ok = m < a.M && (unsigned)(yo - 1 + kh) < (unsigned)a.Ho && (unsigned)(xo - 1 + kw) < (unsigned)a.Wo;
            mk |= (ok ? 1u : 0u) << (kh * 3 + kw);
          }
        amask[p] = mk;
      }
    } else {  // output pixel (yo, xo) reads input (yo s - pad + kh, xo s - pad + kw)
      const int HWi = a.H * a.W, HWo = a.Ho * a.Wo;
      const long base_pix = (long)(m0 / HWo) * HWi - (long)a.pad * a.W - a.pad;
      const long tot_pix = (long)a.n_img * HWi;
      rs_a1 = buffer_rsrc(a.x1 + base_pix * a.ld1, (uint32_t)min((tot_pix - base_pix) * a.ld1 * 2, cap));
      rs_a2 = a.C2 ? buffer_rsrc(a.x2 + base_pix * a.ld2, (uint32_t)min((tot_pix - base_pix) * a.ld2 * 2, cap))
                   : rs_a1;
#pragma unroll
      for (int p = 0; p < AI; ++p) {
        const int m = m0 + arow[p];
        const int n = m / HWo, r = m - n * HWo;
        const int yo = r / a.Wo, xo = r - yo * a.Wo;
        const int yt = yo * a.stride - a.pad, xt = xo * a.stride - a.pad;  // window top-left
        const int win = (int)((long)n * HWi + (long)yt * a.W + xt - base_pix);
        avo1[p] = (win * a.ld1 + ach[p] * 8) * 2;
        avo2[p] = (win * a.ld2 + ach[p] * 8) * 2;
        unsigned mk = 0;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const bool ok = m < a.M && (unsigned)(yt + kh) < (unsigned)a.H && (unsigned)(xt + kw) < (unsigned)a.W;
            mk |= (ok ? 1u : 0u) << (kh * 3 + kw);
          }
        amask[p] = mk;
      }
    }
    rs_b = buffer_rsrc(a.w + (long)n0 * a.K, (uint32_t)min((long)(a.N - n0) * a.K * 2, cap));
#pragma unroll
    for (int p = 0; p < BI; ++p) bvo[p] = (brow[p] * a.K + bch[p] * 8) * 2;
  }

  // uniform per-K-tile offsets.  next(): K-tiles requested in increasing order from the
  // first (3x3: the tap / channel offset advance; the first of a split divides once)
  struct KTile { int soff_a, soff_b, tap, dy, dx; bool two; };
  __device__ __forceinline__ KTile next(const ConvArgs& a, int kt) {
    KTile k;
    k.soff_b = kt * 128;
    k.dy = 0;
    k.dx = 0;
    if (KS == 1) {
      k.tap = 0;
      k.two = a.C2 && kt * 64 >= a.C1;  // concat: a K-tile lies in one source (host: C1 % 64 == 0)
      k.soff_a = k.two ? (kt * 64 - a.C1) * 2 : kt * 128;
    } else if (PM) {  // the valid taps of each chunk in turn (kt only counts them)
      const int kh = tap / 3, kw = tap - kh * 3;
      k.tap = tap;
      k.two = c0 >= a.C1;
      const int ld = k.two ? a.ld2 : a.ld1;
      k.soff_a = ((kh * a.W + kw) * ld + (k.two ? c0 - a.C1 : c0)) * 2;
      k.soff_b = ((c0 >> 6) * 9 + tap) * 128;
      const unsigned rest = tmask & (0x1FEu << tap);  // the chunk's valid taps after this one
      if (rest) tap = __builtin_ctz(rest);
      else { tap = __builtin_ctz(tmask); c0 += 64; }
    } else if (a.phase) {  // (uniform) the parity's 4 taps per chunk: tap and channel straight from kt
      int cc;
      k.tap = tap_of(a, kt * 64, cc);
      const int kh = k.tap / 3, kw = k.tap - kh * 3;
      k.two = cc >= a.C1;
      const int ld = k.two ? a.ld2 : a.ld1;
      k.soff_a = ((kh * a.W + kw) * ld + (k.two ? cc - a.C1 : cc)) * 2;
    } else {
      if (c0 == 0 && tap == 0 && kt != 0) tap = tap_of(a, kt * 64, c0);
      const int kh = tap / 3, kw = tap - kh * 3;
      k.tap = tap;
      k.two = c0 >= a.C1;
      const int ld = k.two ? a.ld2 : a.ld1;
      if (a.upsample) {
        k.soff_a = ((((kh + 1) >> 1) * a.W + ((kw + 1) >> 1)) * ld + (k.two ? c0 - a.C1 : c0)) * 2;
        k.dy = kh != 1 ? a.W * ld * 2 : 0;
        k.dx = kw != 1 ? ld * 2 : 0;
      } else {
        k.soff_a = ((kh * a.W + kw) * ld + (k.two ? c0 - a.C1 : c0)) * 2;
      }
      if (a.ccm) {
        if (++tap == 9) { tap = 0; c0 += 64; }
      } else {
        c0 += 64;
        if (c0 == a.Cin) { c0 = 0; ++tap; }
      }
    }
    return k;
  }

  __device__ __forceinline__ void load_a(int p, uint4* dst, const KTile& k, bool ups = false) const {
    int v = k.two ? avo2[p] : avo1[p];
    if (KS == 3 && ups) v += ((amask[p] >> 9) & 1u ? k.dy : 0) + ((amask[p] >> 10) & 1u ? k.dx : 0);
    const int vo = KS == 1 ? v : (((amask[p] >> k.tap) & 1u) ? v : (int)0x80000000);
    ls_raw_buffer_load_lds(k.two ? rs_a2 : rs_a1, (__attribute__((address_space(3))) void*)dst, 16, vo, k.soff_a, 0, 0);
  }
  __device__ __forceinline__ void load_b(int p, uint4* dst, const KTile& k) const {
    ls_raw_buffer_load_lds(rs_b, (__attribute__((address_space(3))) void*)dst, 16, bvo[p], k.soff_b, 0, 0);
  }
  // the same pieces into registers (register-staged variant: buffer_load_dwordx4 + ds_write_b128)
  __device__ __forceinline__ uint4 reg_a(int p, const KTile& k, bool ups = false) const {
    int v = k.two ? avo2[p] : avo1[p];
    if (KS == 3 && ups) v += ((amask[p] >> 9) & 1u ? k.dy : 0) + ((amask[p] >> 10) & 1u ? k.dx : 0);
    const int vo = KS == 1 ? v : (((amask[p] >> k.tap) & 1u) ? v : (int)0x80000000);
    return __builtin_bit_cast(uint4, ls_raw_buffer_load_v4(k.two ? rs_a2 : rs_a1, vo, k.soff_a, 0));
  }
  __device__ __forceinline__ uint4 reg_b(int p, const KTile& k) const {
    return __builtin_bit_cast(uint4, ls_raw_buffer_load_v4(rs_b, bvo[p], k.soff_b, 0));
  }

  // the whole K-tile kt into the A / B images of a stage (pieces lane-linear per wave)
  __device__ __forceinline__ void issue(const ConvArgs& a, int kt, uint4* a_img, uint4* b_img, int wid_u) {
    const KTile k = next(a, kt);
    if (KS == 3 && a.upsample) {  // (uniform branch: the parity adds only where they apply)
#pragma unroll
      for (int p = 0; p < AI; ++p) load_a(p, a_img + (wid_u * AI + p) * 64, k, true);
    } else {
#pragma unroll
      for (int p = 0; p < AI; ++p) load_a(p, a_img + (wid_u * AI + p) * 64, k);
    }
#pragma unroll
    for (int p = 0; p < BI; ++p) load_b(p, b_img + (wid_u * BI + p) * 64, k);
  }
};

template <class B, class F>
static void with_epi(int epi, B buf, F f) {
  switch (epi) {
    case EPI_PLAIN: return f(IC<EPI_PLAIN>{}, buf);
    case EPI_GEGLU: return f(IC<EPI_GEGLU>{}, buf);
    default: return f(IC<EPI_ANY>{}, buf);
  }
}

// f(EPI, BUF) for the plan's epilogue and DMA form, over the instances compiled for a (KS,
// TAPU) gather: buffer-descriptor DMA only for 1x1 and channel-chunk-major 3x3, EPI_PLAINP
// (the tiled phase form) only for the latter and always with it
template <int KS, bool TAPU, class F>
static void with_epi_buf(const ls_conv_plan_info& i, F f) {
  if constexpr (KS == 3 && TAPU) {
    if (i.epi == EPI_PLAINP) return f(IC<EPI_PLAINP>{}, std::true_type{});
  }
  if constexpr (KS == 1 || TAPU) {
    if (i.buf) return with_epi(i.epi, std::true_type{}, f);
  }
  with_epi(i.epi, std::false_type{}, f);
}

// f(KS, TAPU) for the plan's gather
template <class F>
static void with_gather(const ls_conv_plan_info& i, F f) {
  if (i.ks == 1) f(IC<1>{}, std::false_type{});
  else if (i.tapu) f(IC<3>{}, std::true_type{});
  else f(IC<3>{}, std::false_type{});
}

}  // namespace ls
