#include "ls_conv.h"

namespace ls {

// ------------------------------------------------------------ row-block GEMM
// The short-K linears of the 32x32 level (K = Cin = 320: Transformer/motion
// proj_in/out, fused q|k|v, q, out-proj, GEGLU W1) are epilogue/bandwidth bound
// on the tiled kernels: every 128x160 tile pays a full prologue + LDS-staged
// epilogue for only 5 K-tiles of MFMAs, and re-reads its A rows once per N tile.
// Here one workgroup (8 waves, 2 per SIMD) owns 256 rows x a range of N:
//   * each wave keeps its 32 A rows x K in registers for the whole kernel
//     (2 x KT bf16x8 fragments = 80 VGPRs at K = 320): A is read once;
//   * W streams through LDS in 64-column chunks (all of K per chunk, 2-stage
//     ring, global_load_lds DMA into the XOR-swizzled 64-wide images);
//   * the product is computed transposed, C^T = W A^T (MFMA A operand = W rows,
//     B operand = A rows), so a lane's accumulator holds 4 consecutive output
//     columns of one row and the epilogue stores 8 B per lane straight from
//     registers -- no LDS staging, no barrier -- and runs in the same basic
//     block as the next chunk's MFMAs (double-buffered accumulators), so its
//     VALU work and stores overlap the matrix pipe.
// FLAGS: RB_LN LayerNorm fold (ln_rowstats/ln_colsum), RB_RES residual,
// RB_RV row vector (positional-encoding rows), RB_GEGLU GEGLU epilogue.  With RB_LN the
// register-resident A rows are normalised in place (the host folds gamma / beta).
// Host contract (rowblock_ok): ksize 1, no x2 / affine prologue, K = 32*KT = Cin
// (320 with FM = 2: 256 rows per block; 640 with FM = 1: 128 rows, A still 80 VGPRs),
// M % BM == 0, N % 64 == 0, no split-K, bf16 output with 4-aligned pitches.
enum { RB_LN = 1, RB_RES = 2, RB_RV = 4, RB_GEGLU = 8, RB_STATS = 16, RB_GNCS = 32, RB_AFF = 64 };

// sum over the 16 lanes of a DPP row (all 16 receive it): quad butterflies, then
// rotations by 4 and 8 within the row
__device__ __forceinline__ float row16_sum(float v) {
  auto dpp = [](float x, int ctrl) -> float {
    switch (ctrl) {  // dpp_ctrl must be a constant
      case 0: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, false));
      case 1: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, false));
      case 2: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xF, 0xF, false));
      default: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xF, 0xF, false));
    }
  };
  v += dpp(v, 0);
  v += dpp(v, 1);
  v += dpp(v, 2);
  v += dpp(v, 3);
  return v;
}

template <int KT, int FM, int FN, int FLAGS>
__global__ void __launch_bounds__(512) gemm_rowblock_kernel(ConvArgs a) {
  constexpr int BN = 16 * FN;
  constexpr int BM = 8 * 16 * FM;             // rows per workgroup (8 waves x FM fragments of 16)
  constexpr int KTILES = KT / 2;              // 64-wide LDS images per chunk
  constexpr int WIMG = BN * KTILES * 8;       // uint4 of the W images of a chunk
  constexpr bool LN = FLAGS & RB_LN, RES = FLAGS & RB_RES, RV = FLAGS & RB_RV, GG = FLAGS & RB_GEGLU;
  // residual tile of a chunk (BM rows x BN columns bf16) DMA'd with its W images, so it is
  // in flight two chunks ahead of its epilogue with no registers held (the register
  // residual, one chunk ahead, left the short-K residual GEMMs latency-bound on HBM)
  constexpr int RIMG = RES ? BM * BN / 8 : 0;  // uint4
  constexpr int RPT = RIMG / 512;
  constexpr int STAGE = WIMG + 48 + RIMG;     // + bias / colsum / row-vector columns (3 x 64 fp32) + residual
  constexpr bool AF = FLAGS & RB_AFF;  // GroupNorm affine (+SiLU) prologue on the register-resident A rows
  constexpr bool ST = (FLAGS & RB_STATS) && !GG;  // row statistics of the output (host: one N range per block)
  // GroupNorm column sums (a.cs_out): per chunk a wave's 16 FM rows are summed over its
  // lanes (DPP) into LDS; after the chunk's barrier the CS_ROWS / (16 FM) waves of a
  // slot are added in a fixed order and written (host: BM % CS_ROWS == 0)
  constexpr bool CS = (FLAGS & RB_GNCS) && !GG;
  constexpr int WPS = CS_ROWS / (16 * FM);  // waves per 128-row slot
  constexpr int NSTORE = GG ? FM * FN / 2 : FM * FN;
  constexpr int PPT = (WIMG + 511) / 512;     // 16-B DMA pieces per thread per chunk
  static_assert(KT % 2 == 0 && WIMG % 256 == 0, "K must be a multiple of 64");
  extern __shared__ __attribute__((aligned(16))) uint4 lds_dyn[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l16 = lane & 15, lg = lane >> 4;
  const int rb = blockIdx.x / a.ntn, ns = blockIdx.x - rb * a.ntn;
  const int nch = a.N / BN;
  const int c0 = (int)((long)nch * ns / a.ntn), c1 = (int)((long)nch * (ns + 1) / a.ntn);
  const int mw = rb * BM + wid * 16 * FM;  // this wave's first row

  // chunk c -> LDS stage: W rows [64c, 64c + 64) x all K as KTILES swizzled 64-wide
  // images, then the chunk's 64 bias, colsum and row-vector values (wave 0).
  // piece q = p * 512 + tid of a chunk's images: image t = q / (8 BN), row (q / 8) % BN, chunk q % 8
  const long rv_base = RV ? rv_row(a, rb * BM) : 0;  // host: rows_per_vec % BM == 0
  constexpr int abl = 0;
  // W / residual DMA through buffer descriptors (round 6): the per-thread byte offsets are
  // fixed over the chunks, a chunk moves only the uniform soffset, and the LDS destinations
  // are LDS-space addresses -- one s_add to M0 per DMA instead of a 64-bit global address,
  // a readfirstlane and the M0 copy (the same change took the ff_chain kernel 5-8 % faster)
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  __builtin_assume(wid_u >= 0 && wid_u < 8);
  const uint32_t cap = 0x7FFFFFFFu;
  const i32x4 rs_w = buffer_rsrc(a.w, (uint32_t)min((long)a.N * a.K * 2, (long)cap));
  const i32x4 rs_r = RES ? buffer_rsrc(a.res + (long)rb * BM * a.ldr, (uint32_t)min((long)BM * a.ldr * 2, (long)cap)) : rs_w;
  int wvo[PPT], rvo[RPT > 0 ? RPT : 1];
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int q = p * 512 + tid, t = q / (8 * BN), row = (q >> 3) % BN, pc = q & 7;
    const int lc = pc ^ ((row >> 1) & 7);  // logical 16-B chunk stored at physical chunk pc
    wvo[p] = (row * a.K + t * 64 + lc * 8) * 2;
  }
#pragma unroll
  for (int p = 0; p < RPT; ++p) {  // residual piece q: row q / (BN / 8), 16-B column chunk q % (BN / 8)
    const int q = p * 512 + tid, row = q / (BN / 8), ch = q % (BN / 8);
    rvo[p] = (row * a.ldr + ch * 8) * 2;
  }
  lds_u4* const lbase = (lds_u4*)lds_dyn;
  auto issue = [&](int c, int stage) {
    if ((abl & 2) && c > c0 + 1) return;
    lds_u4* const dst = lbase + stage * STAGE;
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      if (WIMG % 512 == 0 || p * 512 + wid_u * 64 < WIMG)  // (wave-uniform)
        ls_raw_buffer_load_lds(rs_w, (__attribute__((address_space(3))) void*)(dst + p * 512 + wid_u * 64), 16, wvo[p],
                               c * BN * a.K * 2, 0, 0);
    }
    if (wid == 0 && lane < 48 && (lane & 15) * 4 < BN) {
      const int q = lane >> 4, e = (lane & 15) * 4;
      const float* base = q == 0 ? a.bias : q == 1 ? nullptr : (RV ? a.rowvec + rv_base : nullptr);
      const void* ps = base ? (const void*)(base + c * BN + e) : (const void*)ls_zero_page;
      glds16(ps, lds_dyn + stage * STAGE + WIMG);
    }
#pragma unroll
    for (int p = 0; p < RPT; ++p)
      ls_raw_buffer_load_lds(rs_r, (__attribute__((address_space(3))) void*)(dst + WIMG + 48 + p * 512 + wid_u * 64), 16,
                             rvo[p], c * BN * 2, 0, 0);
  };

  if (c0 >= c1) return;
  float2 mrow[FM];  // LayerNorm (mean, rstd) of this lane's two rows
  if (LN) {
#pragma unroll
    for (int i = 0; i < FM; ++i) mrow[i] = *(const float2*)(a.ln_mr + 2L * (mw + i * 16 + l16));
  }
  issue(c0, 0);
  // A rows -> registers (B operand of C^T = W A^T: lane = row l16, k = 8 lg .. + 7 of each 32-wide step)
  bf16x8 ar[FM][KT];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const u16* src = a.x1 + (long)(mw + i * 16 + l16) * a.ld1 + lg * 8;
#pragma unroll
    for (int s = 0; s < KT; ++s) ar[i][s] = (abl & 64) ? bf16x8{} : *(const bf16x8*)(src + s * 32);
  }
  if (LN) {
    // LayerNorm applied to the register-resident A rows once ((x - mean) * rstd, rounded
    // to bf16 like the reference's normalised activations); gamma / beta are folded
    // into W and the bias on the host, so the epilogue needs no per-column colsum.
    wait_vm<0>();
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const float rstd = mrow[i].y, nmr = -mrow[i].x * mrow[i].y;
#pragma unroll
      for (int s = 0; s < KT; ++s) {
        bf16x8 v = ar[i][s];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (__bf16)fmaf((float)v[e], rstd, nmr);
        ar[i][s] = v;
      }
    }
  }
  if (AF) {
    // x * scale[s][c] + shift[s][c], rounded to bf16 like ls_groupnorm_apply's materialised
    // output; the block's rows lie in one sample (host: pix_per_sample % BM == 0).  A SiLU
    // after the affine goes to the register-staged kernel (rowblock_ok): beside the 80 A
    // registers its unrolled form spills.
    const long sb = (long)((rb * BM) / a.pix_per_sample) * a.Cin + lg * 8;
    wait_vm<0>();
#pragma unroll
    for (int s = 0; s < KT; ++s) {
      float sc[8], sh[8];
      load8f(a.aff_scale + sb + s * 32, sc);
      load8f(a.aff_shift + sb + s * 32, sh);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        bf16x8 v = ar[i][s];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (__bf16)fmaf((float)v[e], sc[e], sh[e]);
        // pin the result here: sunk past the barrier, every step's scale / shift would
        // stay live beside the A rows and spill
        asm volatile("" : "+v"(v));
        ar[i][s] = v;
      }
    }
  }
  wait_vm<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  f32x4 acc0[FM][FN], acc1[FM][FN];
  // column parameters (bias + row vector) of chunk c from its LDS stage, read before
  // the next DMA is issued (an LDS read after it would wait for the DMA); the chunk's
  // accumulators start at them
  auto load_prm = [&](int stage, float4 (&bb)[FN]) {
    const float4* prm = (const float4*)(lds_dyn + stage * STAGE + WIMG);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      bb[j] = prm[lg + 4 * j];
      if (RV) {
        const float4 r4 = prm[32 + lg + 4 * j];  // (FN 2 uses the first 8 of each 16)
        bb[j].x += r4.x; bb[j].y += r4.y; bb[j].z += r4.z; bb[j].w += r4.w;
      }
    }
  };
  const bool unit_scale = a.out_scale == 1.f;
  double S1[FM], S2[FM];  // running row sums of the output (ST), per lane: its 4-column slices
#pragma unroll
  for (int i = 0; i < FM; ++i) { S1[i] = 0.0; S2[i] = 0.0; }
  auto epilogue = [&](int c, f32x4 (&acc)[FM][FN], int stage) {
    const int nb = c * BN + 4 * lg;  // packed column of fragment j: nb + 16 j
    const u16* rtile = (const u16*)(lds_dyn + stage * STAGE + WIMG + 48);  // [BM][BN] residual of chunk c
    float cs1[FM], cs2[FM];  // this chunk's partial sums (fp32 over 4*FN values), folded into S in fp64
    float gcs[FM][FN][4];    // stored values of this chunk (CS)
#pragma unroll
    for (int i = 0; i < FM; ++i) { cs1[i] = 0.f; cs2[i] = 0.f; }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      u16* yrow = (u16*)a.y + (long)(mw + i * 16 + l16) * a.ldy;
      if (GG) {
#pragma unroll
        for (int p = 0; p < FN / 2; ++p) {
          float h[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) h[r] = acc[i][2 * p][r] * gelu_erf(acc[i][2 * p + 1][r]);
          *(uint2*)(yrow + c * (BN / 2) + 16 * p + 4 * lg) = make_uint2(pack2(h[0], h[1]), pack2(h[2], h[3]));
        }
      } else {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          float o[4];
          float r4[4] = {0.f, 0.f, 0.f, 0.f};
          if (RES) {
            const uint2 rs = *(const uint2*)(rtile + (wid * 16 * FM + i * 16 + l16) * BN + 4 * lg + 16 * j);
            r4[0] = __uint_as_float(rs.x << 16); r4[1] = __uint_as_float(rs.x & 0xffff0000u);
            r4[2] = __uint_as_float(rs.y << 16); r4[3] = __uint_as_float(rs.y & 0xffff0000u);
          }
          if (unit_scale) {  // (block-uniform)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = acc[i][j][r] + r4[r];
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (acc[i][j][r] + r4[r]) * a.out_scale;
          }
          const uint2 pk = make_uint2(pack2(o[0], o[1]), pack2(o[2], o[3]));
          if (!(abl & 4) || pk.x == 0x12345u) *(uint2*)(yrow + nb + 16 * j) = pk;
          if (CS) {
            gcs[i][j][0] = __uint_as_float(pk.x << 16); gcs[i][j][1] = __uint_as_float(pk.x & 0xffff0000u);
            gcs[i][j][2] = __uint_as_float(pk.y << 16); gcs[i][j][3] = __uint_as_float(pk.y & 0xffff0000u);
          }
          if (ST) {  // statistics of the stored (bf16-rounded) values, like ls_row_stats reads them:
            // v_dot2c_f32_bf16 on the packed pairs (4 instructions for 4 values instead of 11)
            typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
            const bf2 one2 = {(__bf16)1.0f, (__bf16)1.0f};
            const bf2 px = __builtin_bit_cast(bf2, pk.x), py = __builtin_bit_cast(bf2, pk.y);
            cs1[i] = __builtin_amdgcn_fdot2_f32_bf16(py, one2, __builtin_amdgcn_fdot2_f32_bf16(px, one2, cs1[i], false), false);
            cs2[i] = __builtin_amdgcn_fdot2_f32_bf16(py, py, __builtin_amdgcn_fdot2_f32_bf16(px, px, cs2[i], false), false);
          }
        }
      }
    }
    if (ST) {
#pragma unroll
      for (int i = 0; i < FM; ++i) { S1[i] += (double)cs1[i]; S2[i] += (double)cs2[i]; }
    }
    if (CS) {  // column sums of this wave's rows -> LDS part[c & 1][wave][64]
      float* part = (float*)(lds_dyn + 3 * STAGE) + (c & 1) * 512 + wid * 64;
      float mine = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {  // v = kind * 8 + j * 4 + r
        const int j = (v >> 2) & 1, r = v & 3;
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const float b = gcs[i][j][r];
          t += (v >> 3) ? b * b : b;
        }
        t = row16_sum(t);
        mine = (l16 == v) ? t : mine;
      }
      // lane (lg, l16): column 4 lg + 16 j + r of the chunk, value kind
      const int v = l16, col = 4 * lg + 16 * ((v >> 2) & 1) + (v & 3);
      part[col * 2 + (v >> 3)] = mine;
    }
  };
  // slots of this block's rows: add the WPS waves of each for chunk cc and write them
  auto merge_cs = [&](int cc) {
    const float* part = (const float*)(lds_dyn + 3 * STAGE) + (cc & 1) * 512;
    for (int q = tid; q < (BM / CS_ROWS) * 64; q += 512) {
      const int sl = q >> 6, e = q & 63;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WPS; ++w) t += part[(sl * WPS + w) * 64 + e];
      const long slot = (long)rb * (BM / CS_ROWS) + sl;
      a.cs_out[slot * 2 * a.N + (e & 1) * a.N + cc * BN + (e >> 1)] = t;
    }
  };
  // b0: the chunk's bias (+ row vector), read by the caller before its DMA issue; the
  // accumulators start there, so the epilogue has no bias add
  auto mfma_chunk = [&](int stage, f32x4 (&acc)[FM][FN], const float4 (&b0)[FN]) {
    const uint4* cur = lds_dyn + stage * STAGE;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){b0[j].x, b0[j].y, b0[j].z, b0[j].w};
#pragma unroll
    for (int s = 0; s < KT; ++s) {
      bf16x8 bw[FN];
      const int ch = (s & 1) * 4 + lg;
#pragma unroll
      for (int j = 0; j < FN; ++j)
        bw[j] = __builtin_bit_cast(bf16x8, cur[(s >> 1) * (8 * BN) + swz64(j * 16 + l16, ch)]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[j], ar[i][s], acc[i][j], 0, 0, 0);
    }
  };
  auto sync = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // 3-stage ring: chunk c computes from stage c%3 while chunk c-1's parameters stay in
  // (c-1)%3 for its epilogue and chunk c+1 lands in (c+1)%3.  Past the last chunk the DMA
  // re-loads the last chunk into the spare stage, so the steady-state body is branch-free.
  // The residual tile of chunk c travels with the chunk's W images (stage c % 3).
  auto body = [&](int c, f32x4 (&acc)[FM][FN], f32x4 (&prev)[FM][FN]) {
    const int st = (c - c0) % 3;
    const int sp = st == 0 ? 2 : st - 1;
    float4 bn[FN];
    load_prm(st, bn);
    issue(min(c + 1, c1 - 1), st == 2 ? 0 : st + 1);
    if (CS && c - 2 >= c0) merge_cs(c - 2);  // written two epilogues ago, past a barrier
    mfma_chunk(st, acc, bn);
    epilogue(c - 1, prev, sp);
    wait_vm<NSTORE>();                                       // the DMA (older than the stores) landed
    sync();
  };
  // first chunk: no epilogue
  {
    float4 bn[FN];
    load_prm(0, bn);
    issue(min(c0 + 1, c1 - 1), 1);
    mfma_chunk(0, acc0, bn);
  }
  wait_vm<0>();
  sync();
  int c = c0 + 1;
  for (; c + 1 < c1; c += 2) {
    body(c, acc1, acc0);
    body(c + 1, acc0, acc1);
  }
  if (c < c1) {
    body(c, acc1, acc0);
    epilogue(c, acc1, (c - c0) % 3);
  } else {
    epilogue(c1 - 1, acc0, (c1 - 1 - c0) % 3);
  }
  if (CS) {  // the last two chunks' column sums
    __syncthreads();
    for (int cc = max(c0, c1 - 2); cc < c1; ++cc) merge_cs(cc);
  }
  if (ST) {  // the 4 lane groups of a row hold disjoint column slices: combine, then lane group 0 writes
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      double s1 = S1[i], s2 = S2[i];
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
      }
      if (lg == 0) {
        const double n = (double)a.N, mean = s1 / n;
        const double var = fmax(s2 / n - mean * mean, 0.0);
        *(float2*)(a.stats_out + 2L * (mw + i * 16 + l16)) =
            make_float2((float)mean, (float)(1.0 / sqrt(var + (double)a.stats_eps)));
      }
    }
  }
}

bool rowblock_ok(const ls_conv_desc* d, const ConvArgs& a) {
  if (!g_tune.rowblock || g_tune.force_tile || g_tune.force_regstage || d->ksize != 1 || a.C2) return false;
  // GroupNorm affine prologue: one sample per block, and not together with the LayerNorm fold
  if (a.aff_scale && (a.ln_mr || a.silu_in || a.pix_per_sample % (a.Cin == 320 ? 256 : 128) ||
                      ((uintptr_t)a.aff_scale | (uintptr_t)a.aff_shift) & 15))
    return false;
  // K = 640 only without a residual (the tiled kernel is faster there: 48 vs 53 us at 16x16)
  if (!((a.Cin == 320 && a.K == 320 && a.M % 256 == 0) ||
        (g_tune.rowblock640 && a.Cin == 640 && a.K == 640 && a.M % 128 == 0 && (!a.res || g_tune.rb640_res))))
    return false;
  if (a.N % 64 || a.split != 1 || a.y_f32) return false;
  if (a.act != LS_ACT_NONE && a.act != LS_ACT_GEGLU) return false;
  if (a.ldy % 4 || (a.res && a.ldr % 8) || (a.rowvec && (a.rowvec_ld % 4 || a.rows_per_vec % 256))) return false;
  if (((uintptr_t)a.y & 7) || ((uintptr_t)a.res & 15)) return false;  // 8-B output pieces, 16-B residual DMA
  return (((uintptr_t)a.x1 | (uintptr_t)a.bias | (uintptr_t)a.ln_cs | (uintptr_t)a.rowvec) & 15) == 0;
}

// the compiled FLAGS combinations, each at <KT 10, FM 2>, <20, 1> and, without RB_FM1_K640, <20, 2>.
// Every flag set added here needs its per-element cases in tests/test_gpu_edges_conv_fused.py
// (RB_FLAG_SETS there; test_every_rowblock_instance_ran counts the instances the plans reported)
using RowblockInstances =
    std::integer_sequence<int, 0, RB_LN, RB_LN | RB_RV, RB_RES, RB_LN | RB_RES, RB_LN | RB_GEGLU, RB_GEGLU, RB_STATS,
                          RB_RES | RB_STATS, RB_RES | RB_GNCS, RB_AFF, RB_AFF | RB_STATS>;
// one fragment per wave only: the statistics epilogues spill at FM 2, and with the GroupNorm
// affine a block looks its sample up once (rowblock_ok only guarantees pix_per_sample % 128
// == 0 at K = 640)
constexpr int RB_FM1 = RB_STATS | RB_GNCS | RB_AFF;
// ... and at K = 640 also with a residual (tuning key 20): three stages of 40 KB of W images and a
// 256-row residual tile of 16 KB are 170 KB, more LDS than a workgroup can have.  <20, 2> was
// planned for it under tuning key 15 and every such launch refused ("invalid argument");
// tests/test_gpu_edges_conv_fused.py found it.
constexpr int RB_FM1_K640 = RB_FM1 | RB_RES;
constexpr size_t RB_LDS_MAX = 160 << 10;  // LDS of a gfx950 workgroup

// FN = 2 (32-column chunks): the FN = 4 variant needs > 256 VGPRs and spills, and a
// spill's scratch traffic would break the kernel's counted vmcnt waits.
constexpr size_t rowblock_lds(int kt, int fm, int flags) {
  return (size_t)3 * (16 * 2 * (kt / 2) * 8 + 48 + ((flags & RB_RES) ? 128 * fm * 16 * 2 / 8 : 0)) * 16 +
         ((flags & RB_GNCS) ? 4096 : 0);
}

template <int... F>
static bool rowblock_compiled(int flags, std::integer_sequence<int, F...>) {
  return ((flags == F) || ...);
}

// Plans the row-block instance for a.stats_out / a.cs_out as they stand; false when there is
// none (fused statistics and column sums need whole rows in a block).
bool plan_rowblock(ConvPlan& p) {
  ConvArgs& a = p.a;
  const int flags = (a.ln_mr ? RB_LN : 0) | (a.res ? RB_RES : 0) | (a.rowvec ? RB_RV : 0) |
                    (a.act == LS_ACT_GEGLU ? RB_GEGLU : 0) | (a.stats_out ? RB_STATS : 0) | (a.cs_out ? RB_GNCS : 0) |
                    (a.aff_scale ? RB_AFF : 0);
  const int fm = a.K == 320 || (g_tune.rb640_fm2 && !(flags & RB_FM1_K640)) ? 2 : 1, bm = 128 * fm;
  if (a.M % bm || !rowblock_compiled(flags, RowblockInstances{})) return false;
  const int ntm = a.M / bm, nch = a.N / 32;
  const int ntn = std::max(1, std::min(nch, (256 + ntm - 1) / ntm));
  if ((a.stats_out || a.cs_out) && ntn != 1) return false;
  a.ntm = ntm;
  a.ntn = ntn;
  p.i.family = 1;
  p.i.rb_kt = a.K / 32;
  p.i.rb_fm = fm;
  p.i.rb_flags = flags;
  p.i.grid = ntm * ntn;
  p.i.threads = 512;
  p.i.lds_bytes = (int)rowblock_lds(p.i.rb_kt, fm, flags);
  return true;
}

template <int FLAGS>
static void launch_rowblock1(const ConvPlan& p, hipStream_t s) {
  static_assert(rowblock_lds(10, 2, FLAGS) <= RB_LDS_MAX && rowblock_lds(20, 1, FLAGS) <= RB_LDS_MAX, "row-block LDS");
  if (p.i.rb_kt == 10) return launch_plan<gemm_rowblock_kernel<10, 2, 2, FLAGS>>(p, s);
  if constexpr (!(FLAGS & RB_FM1_K640)) {
    static_assert(rowblock_lds(20, 2, FLAGS) <= RB_LDS_MAX, "row-block LDS");
    if (p.i.rb_fm == 2) return launch_plan<gemm_rowblock_kernel<20, 2, 2, FLAGS>>(p, s);
  }
  launch_plan<gemm_rowblock_kernel<20, 1, 2, FLAGS>>(p, s);
}

template <int... F>
static void launch_rowblock(const ConvPlan& p, hipStream_t s, std::integer_sequence<int, F...>) {
  ((p.i.rb_flags == F ? launch_rowblock1<F>(p, s) : void()), ...);
}

void launch_rowblock(const ConvPlan& p, hipStream_t s) { launch_rowblock(p, s, RowblockInstances{}); }

}  // namespace ls
