#include "ls_conv.h"

namespace ls {

// ------------------------------------------------------------- halo-tile 3x3 conv
// conv3x3_halo_kernel: 3x3 / stride 1 / pad 1 convolutions with Cin % 64 == 0 whose A
// operand comes from an LDS HALO TILE.  The implicit-GEMM kernels (ls_conv_tiled.hip) gather A per tap:
// a 64-channel chunk of every output pixel's 3x3 window is DMA'd 9 times (9 K-tiles), so
// at N = 128 / 160 the operand DMA -- about 60 issue cycles per 1-KB wave-instruction --
// outweighs the MFMAs it feeds (the VAE's 128-channel convs at 256^2 ran at 0.34 of the
// bf16 peak), and a GroupNorm affine + SiLU on the input had to be materialised by its
// own pass (ls_groupnorm_apply) because applying it in the gather would repeat it 9 times.
// Here a block owns a TH x TW patch of one image (256 output pixels; 128 in the 16 x 8
// form below) x BN output channels:
//   * per 64-channel chunk, the (TH + 2) x (TW + 2) input pixels of the patch are loaded
//     ONCE (buffer loads into registers; pixels outside the image read zeros), optionally
//     put through y = silu?(x * scale + shift) (the GroupNorm affine of the pixel's sample)
//     and stored to a halo image in LDS: 128 B per pixel, the 16-B chunks XOR-swizzled by
//     (pixel & 7) -- conflict-free ds_read_b128 fragment reads at ANY pixel offset, which
//     the 9 taps need (brute-forced over the lane groups; the GEMMs' ((row >> 1) & 7)
//     swizzle is 2-way there).  Halo rows are TW + 8 pixels long (== 0 mod 8), so the
//     swizzle phase of every fragment of a wave equals its first fragment's: one address
//     computation per (tap, k-step) and lane, fragment offsets are immediates (the compact
//     TW + 2 row with a column-based swizzle frees 28 KB of LDS, but the third weight slot
//     at BN 160 that room was for spills 30 VGPRs; the 16 x 8 form uses it to fit 2 blocks);
//   * the 9 taps of the chunk then run from that image: tap (kh, kw) shifts the read by
//     kh P + kw pixels (P the row pitch); the weight K-tile of each tap ([BN][64], channel-chunk-major
//     packing) streams through an NSW-slot LDS ring by LDS-DMA, NSW - 1 taps ahead;
//   * the halo of chunk c + 1 is loaded into registers in three batches at taps 0 / 3 / 6 of
//     chunk c and written to the other halo image at taps 3 / 6 / 8, each batch BEHIND the
//     MFMAs of its tap (the `tap` lambda pins the order), so the input affine's VALU work
//     never stands between a barrier and the MFMAs whose operands are already resident;
//     every wait is one constant vmcnt (padded dummy DMAs).
// 8 waves as 4 (pixels) x 2 (channels), 64 x BN/2 per wave; the epilogue is
// store_tile_plain (bias, per-frame row vector, residual, scale, GroupNorm column sums
// of the output) with the patch's rows mapped back to image rows.
// TH = 256 / TW: 16 x 16 patches, 8 waves, one block per CU (the shipped UNet form).
// TH = 8 (round 5, BN 128: the VAE's convs): 16 x 8 patches, 4 waves as 2 (pixels) x 2
// (channels), compact halo rows (TW + 2 pixels, chunks swizzled by the halo COLUMN & 7 --
// conflict-free at any row / column offset, brute-forced -- so fragments one patch row
// apart still share the swizzle phase) and a 2-slot weight ring: 80 KB of LDS, TWO blocks
// per CU, so one block's halo prologue, chunk transitions and epilogue overlap the other's
// MFMAs (the 1-block form waited 44.5 % of its wave time, profiles/r05a_h128_summary.txt).
template <int TW, int BN, int TH_ = 256 / TW>
struct HaloCfg {
  static constexpr int TH = TH_;
  // channel waves: 2 (BN / 2 columns each); 1 for the narrow tile (BN 16: the VAE decoder's
  // conv_out, 3 used output channels, where the conv is bound by the halo transform and HBM)
  static constexpr int WNW = BN >= 64 ? 2 : 1;
  static constexpr int NT = (TH / 4) * WNW * 64;         // threads: (TH / 4) pixel waves x WNW channel waves
  static constexpr bool COMPACT = TH < 16;
  static constexpr int P = COMPACT ? TW + 2 : TW + 8;    // halo row pitch (pixels); padded: 0 mod 8
  static constexpr int HALO = (TH + 2) * P * 8;          // uint4 per halo image
  static constexpr int WSLOT = BN * 8;                   // uint4 per weight ring slot (BN x 64 k)
  // weight ring slots (3 at BN 160 spills 30 VGPRs; the 2-block form has LDS for 2)
  static constexpr int NSW = COMPACT ? 2 : BN <= 128 ? 3 : 2;
  static constexpr int DPT = (WSLOT + NT - 1) / NT;      // weight DMAs per thread per tap
  static constexpr int FN = BN / WNW / 16;               // 16-column fragments per wave
  static constexpr size_t SHM = ((size_t)2 * HALO + (size_t)NSW * WSLOT + 64 + 64) * 16;  // + dummy, affine
  static_assert(SHM <= (COMPACT ? 81920 : 163840), "halo conv LDS (compact: two blocks per CU)");
  static_assert((size_t)64 * (BN + 4) * 4 <= (size_t)2 * HALO * 16, "epilogue staging fits the halo images");
  static_assert(TW == 16 && (TH == 16 || TH == 8), "16-pixel patch rows, 16 or 8 of them");
  static_assert(BN % (16 * WNW) == 0, "whole 16-column fragments per wave");
  static constexpr int MINB = BN >= 64 ? 16 / TH : 2;    // launch bounds: blocks per CU
};


// halo loads of a chunk in 3 batches (pieces [hb_lo(b), hb_lo(b + 1))): loaded at taps 0 /
// 3 / 6 of the previous chunk and stored at taps 3 / 6 / 8, so at most 3 pieces (12 VGPRs)
// are in flight per thread
__host__ __device__ constexpr int hb_lo(int b, int nhl) { return b == 0 ? 0 : b == 1 ? (nhl + 2) / 3 : b == 2 ? (2 * nhl + 2) / 3 : nhl; }
// VMEM instructions a thread issues after the weight DMA at tap t (0..8) of a chunk:
// the halo batch loaded there (+ at tap 0 the chunk's affine parameters, one float4 per thread)
// (ts: taps between two batches -- 3 with 9 taps per chunk, 1 with the phase form's 4)
__host__ __device__ constexpr int halo_issue(int t, int nhl, bool gn, int ts = 3) {
  return t == 0 ? hb_lo(1, nhl) + (gn ? 1 : 0) : t == ts ? hb_lo(2, nhl) - hb_lo(1, nhl) : t == 2 * ts ? nhl - hb_lo(2, nhl) : 0;
}

// Halo pieces: the (TH + 2) x (TW + 2) pixels the taps read x 8 16-B chunks (2592 pieces at
// 16 x 16: 5.06 per thread); piece j of a thread has its own LDS slot hdst[j].
// PH (the phase form of a nearest-x2 upsample conv, ls_conv_desc.upsample == 2): the block
// owns a TH x TW patch of the INPUT image and one output parity ph = 2 py + px (a grid
// dimension).  The 2 x 2 output pixels of an input pixel read the same 3 x 3 input
// neighbourhood, and the three row (column) taps of parity py (px) land on two input rows
// (columns), so the parity's outputs are a 2 x 2 conv over the plain input-space halo image:
// 4 taps per chunk, tap t at halo offset (py + t / 2, px + t % 2), with the phase's own
// summed weights ([4][N][4 Cin], K-tile 4 ci + t; packing.pack_phase_weight); the epilogue
// stores patch pixel (r, c) at output pixel (2 (y0 + r) + py, 2 (x0 + c) + px).
template <int TW, int BN, bool GN, bool CSF, int TH_ = 256 / TW, bool PH = false>
__global__ void __launch_bounds__((HaloCfg<TW, BN, TH_>::NT), (HaloCfg<TW, BN, TH_>::MINB)) conv3x3_halo_kernel(ConvArgs a) {
  using HC = HaloCfg<TW, BN, TH_>;
  static_assert(!(PH && GN), "the phase form takes no input affine");
  constexpr int NTAP = PH ? 4 : 9;  // taps per chunk
  constexpr int TS = PH ? 1 : 3;    // taps between two halo batches
  constexpr int TH = HC::TH, P = HC::P, HALO = HC::HALO, WSLOT = HC::WSLOT, NSW = HC::NSW, NT = HC::NT;
  constexpr int WNW = HC::WNW;
  constexpr bool COMPACT = HC::COMPACT;
  constexpr int NPC = (TH + 2) * (TW + 2) * 8;  // pieces per chunk (the read pixels)
  constexpr int NHL = (NPC + NT - 1) / NT, DPT = HC::DPT, FM = 4, FN = HC::FN, WTN = BN / WNW;
  constexpr int HB = (NHL + 2) / 3;  // largest batch
  extern __shared__ __attribute__((aligned(16))) uint4 lds_dyn[];
  uint4* const hbuf = lds_dyn;                 // [2][HALO]
  uint4* const wbuf = lds_dyn + 2 * HALO;      // [NSW][WSLOT]
  uint4* const dummy = wbuf + NSW * WSLOT;     // 1 KB: padding DMAs land here
  float4* const gpar = (float4*)(dummy + 64);  // [2 chunk parities][scale 16 | shift 16] float4

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WNW, wn = wid % WNW;
  const int l16 = lane & 15, lg = lane >> 4;
  const int ntn = (a.N + BN - 1) / BN, tpr = a.W / TW, tpc = a.H / TH;
  // (measured, not kept: a persistent grid issuing the next tile's weights and halo loads
  // before this tile's epilogue -- 30-90 VGPRs of spills in every instance)
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tn = bid % ntn;
  bid /= ntn;
  int ph = 0;  // (the four parities of a patch run next to each other: they read the same input)
  if constexpr (PH) {
    ph = bid & 3;
    bid >>= 2;
  }
  const int py = ph >> 1, px = ph & 1;
  const int txb = bid % tpr;
  bid /= tpr;
  const int tyb = bid % tpc;
  const int img = bid / tpc;
  const int y0 = tyb * TH, x0 = txb * TW, n0 = tn * BN;
  // the image the patches tile: the output image (for a 9-tap upsample conv the launch passes the
  // output dims); in the phase form the INPUT image (H x W as given, upsample zeroed by the launch)
  const long HW = (long)a.H * a.W;
  // nearest x2 upsample (round 6): halo pixel (y, x) of the output image reads input pixel
  // (y >> 1, x >> 1) -- the LDS halo image, the taps and the epilogue are those of a plain conv
  const int ups = a.upsample;
  const int Wi = a.W >> ups;
  const long HWi = HW >> (2 * ups);
  const int nchunk = a.Cin / 64;
  const int G = NTAP * nchunk;  // taps in all

  // ---- this thread's halo pieces: q = j*NT + tid -> read pixel q / 8 (row-major over the
  // (TH + 2) x (TW + 2) pixels the taps read), logical 16-B chunk tid & 7; its slot in the
  // padded image: row hr, column hcol + 3, the chunk swizzled by (slot & 7); compact: row
  // hr, column hcol, swizzled by (hcol & 7)
  const int hc8 = tid & 7;
  int hpix[NHL];  // pixel index within the image, or -1 (outside: zeros)
  int hdst[NHL];
#pragma unroll
  for (int j = 0; j < NHL; ++j) {
    const int q = j * NT + tid, hp = q >> 3;
    const int hr = hp / (TW + 2), hcol = hp - hr * (TW + 2);
    if constexpr (COMPACT) {  // row hr, column hcol, the chunk swizzled by the column
      hdst[j] = (hr * P + hcol) * 8 + (hc8 ^ (hcol & 7));
    } else {
      const int slot = hr * P + hcol + 3;
      hdst[j] = slot * 8 + (hc8 ^ (slot & 7));
    }
  }
  const uint32_t cap = 0x7FFFFFFFu;
#pragma unroll
  for (int j = 0; j < NHL; ++j) {
    const int q = j * NT + tid, hp = q >> 3;
    const int hr = hp / (TW + 2), hcol = hp - hr * (TW + 2);
    const int y = y0 - 1 + hr, x = x0 - 1 + hcol;
    hpix[j] = q < NPC && y >= 0 && y < a.H && x >= 0 && x < a.W ? (y >> ups) * Wi + (x >> ups) : -1;
  }
  const i32x4 rs1 = buffer_rsrc(a.x1 + img * HWi * a.ld1, (uint32_t)min((long)HWi * a.ld1 * 2, (long)cap));
  const i32x4 rs2 = a.C2 ? buffer_rsrc(a.x2 + img * HWi * a.ld2, (uint32_t)min((long)HWi * a.ld2 * 2, (long)cap)) : rs1;
  const long aff0 = (long)img * HW / a.pix_per_sample * a.Cin;
  // weight descriptor from column n0 (rows n0 + BN > N -- the narrow tile over N = 8 -- lie
  // past it and read zeros)
  // (phase form: the parity's [N][K] matrix)
  const i32x4 rs_w = buffer_rsrc(a.w + ((long)ph * a.N + n0) * a.K, (uint32_t)min((long)min(BN, a.N - n0) * a.K * 2, (long)cap));
  uint4 hreg[HB];
  float4 gp;
  // the affine parameters of chunk ci (64 scales, 64 shifts): every thread loads one float4
  // (the same count per wave), threads 0..31 keep theirs in LDS for store_halo
  auto load_par = [&](int ci) {
    const int k = tid & 31;
    gp = *(const float4*)((k < 16 ? a.aff_scale : a.aff_shift) + aff0 + ci * 64 + (k & 15) * 4);
  };
  auto store_par = [&](int ci) {  // scale and shift times log2(e): store_halo applies silu_log2
    constexpr float L2E = 1.4426950408889634f;
    if (tid < 32) gpar[(ci & 1) * 32 + tid] = make_float4(gp.x * L2E, gp.y * L2E, gp.z * L2E, gp.w * L2E);
  };
  auto load_halo = [&](int ci, int b) {
    const bool two = ci * 64 >= a.C1;
    const int ld = two ? a.ld2 : a.ld1;
    const int soff = (two ? ci * 64 - a.C1 : ci * 64) * 2;
    const int j0 = hb_lo(b, NHL), j1 = hb_lo(b + 1, NHL);
#pragma unroll
    for (int j = j0; j < j1; ++j) {
      const int vo = hpix[j] >= 0 ? hpix[j] * ld * 2 + hc8 * 16 : (int)0x80000000;
      hreg[j - j0] = __builtin_bit_cast(uint4, ls_raw_buffer_load_v4(two ? rs2 : rs1, vo, soff, 0));
    }
    if constexpr (GN) {
      if (b == 0 && ci > 0) load_par(ci);
    }
  };
  // pieces [j0, j1) of a chunk's halo image buf from v[j - j0] (+ the affine + SiLU)
  auto put_halo = [&](int buf, int j0, int j1, const uint4* v_in) __attribute__((always_inline)) {
    uint4* const hb0 = hbuf + buf * HALO;
    float4 gsc[2], gsh[2];
    if constexpr (GN) {  // this thread's 8 channels (chunk parity buf)
      const float4* gq = gpar + buf * 32 + hc8 * 2;
      gsc[0] = gq[0]; gsc[1] = gq[1]; gsh[0] = gq[16]; gsh[1] = gq[17];
    }
#pragma unroll
    for (int j = j0; j < j1; ++j) {
      if (j * NT + tid >= NPC) continue;
      uint4 v = v_in[j - j0];
      if constexpr (GN) {
        if (hpix[j] >= 0) {  // zero padding stays zero: the conv pads the ACTIVATED input
          float f[8];
          unpack8(v, f);
          const float scl[8] = {gsc[0].x, gsc[0].y, gsc[0].z, gsc[0].w, gsc[1].x, gsc[1].y, gsc[1].z, gsc[1].w};
          const float shf[8] = {gsh[0].x, gsh[0].y, gsh[0].z, gsh[0].w, gsh[1].x, gsh[1].y, gsh[1].z, gsh[1].w};
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = silu_log2(fmaf(f[e], scl[e], shf[e]));  // (host: GN implies SiLU)
          v = pack8(f);
        }
      }
      hb0[hdst[j]] = v;
    }
  };
  auto store_halo = [&](int buf, int b) { put_halo(buf, hb_lo(b, NHL), hb_lo(b + 1, NHL), hreg); };

  // ---- weight DMA: tap g = NTAP ci + t is K-tile g of the channel-chunk-major packing
  // (buffer-descriptor DMA from column n0: per thread one byte offset, per tap the uniform
  // soffset g * 128 -- no 64-bit address arithmetic in the tap loop)
  int wvo[DPT];
#pragma unroll
  for (int j = 0; j < DPT; ++j) {
    const int q = j * NT + tid, row = q >> 3, pc = q & 7;
    const int lc = pc ^ ((row >> 1) & 7);
    wvo[j] = ((q < WSLOT ? row : 0) * a.K + lc * 8) * 2;
  }
  // ring slot of tap g: with 3 slots, (9 ci + t) % 3 == t % 3 is known per tap at compile time
  // (2 slots: (9 ci + t) % 2 == (ci + t) % 2, so with the chunk parity par = ci & 1 computed
  // once per chunk the slot of every tap is one of two per-chunk values -- no per-tap g % 2)
  // (phase form, 4 taps per chunk: 2 slots t % 2; 3 slots (4 ci + t) % 3 = (ci + t) % 3 from
  // the per-chunk par = ci % 3)
  auto wslot = [&](int par, int t) { return PH ? (NSW == 3 ? (par + t) % 3 : t & 1) : NSW == 3 ? t % 3 : (t & 1) ^ par; };
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  __builtin_assume(wid_u >= 0 && wid_u < NT / 64);
  // (LDS destinations as 32-bit LDS-space addresses: a generic-pointer select cast to LDS
  // costs a null check per DMA, and with WSLOT % NT == 0 no DMA is a padding one)
  lds_u4* const wbuf_l = (lds_u4*)lds_dyn + 2 * HALO;
  lds_u4* const dummy_l = wbuf_l + NSW * WSLOT;
  auto issue_w = [&](int g, int sl) {
    lds_u4* slot = wbuf_l + sl * WSLOT + wid_u * 64;
#pragma unroll
    for (int j = 0; j < DPT; ++j) {
      const bool live = WSLOT % NT == 0 || j * NT + wid_u * 64 < WSLOT;  // wave-uniform
      ls_raw_buffer_load_lds(rs_w, (__attribute__((address_space(3))) void*)(live ? slot + j * NT : dummy_l), 16, wvo[j],
                             g * 128, 0, 0);
    }
  };

  // ---- A fragment addressing: output pixel p = 64 wm + 16 i + l16 of the patch (TW 16:
  // fragment i is patch row 4 wm + i, column l16)
  static_assert(TW == 16, "fragment i = one patch row");
  const int p0 = 64 * wm + l16;
  // halo pixel of fragment 0 at tap (0, 0) (phase form: at the parity's first tap (py, px))
  const int hp0 = (p0 / TW) * P + (p0 % TW) + (COMPACT ? 0 : 3) + py * P + px;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // prologue: weights of taps 0 .. NSW - 2, the chunk-0 affine row, and every chunk-0 halo
  // piece into registers at once (one HBM round trip, not one per batch), then the image
  // (chunk 0 reads source 1: host C1 % 64 == 0, C1 > 0)
  for (int g = 0; g < NSW - 1 && g < G; ++g) issue_w(g, g % NSW);
  {
    uint4 hpre[NHL];
    if constexpr (GN) load_par(0);
#pragma unroll
    for (int j = 0; j < NHL; ++j) {
      const int vo = hpix[j] >= 0 ? hpix[j] * a.ld1 * 2 + hc8 * 16 : (int)0x80000000;
      hpre[j] = __builtin_bit_cast(uint4, ls_raw_buffer_load_v4(rs1, vo, 0, 0));
    }
    if constexpr (GN) {
      store_par(0);
      __syncthreads();
    }
    put_halo(0, 0, NHL, hpre);  // (the compiler waits for the loads)
  }

  bf16x8 apf[2][FM];  // A fragments of the current tap (both k-steps)
  auto read_a = [&](const uint4* hb, int tt, int ks) {  // (tt, ks compile-time after inlining)
    constexpr int TPR = PH ? 2 : 3;  // taps per kernel row
    const int hpt = hp0 + (tt / TPR) * P + tt % TPR;
    // the swizzle phase, shared by the wave's fragments: padded rows (P == 0 mod 8) the
    // pixel's, compact rows the halo column's (l16 + kw)
    const int sw = COMPACT ? (l16 + px + tt % TPR) & 7 : hpt & 7;
    const int base = hpt * 8 + ((ks * 4 + lg) ^ sw);
#pragma unroll
    for (int i = 0; i < FM; ++i)  // fragment i: + ((16 i) / TW) rows, + (16 i) % TW pixels
      apf[ks][i] = __builtin_bit_cast(bf16x8, hb[base + 8 * (((16 * i) / TW) * P + (16 * i) % TW)]);
  };
  // One tap.  The order within it keeps the matrix pipe fed across the per-tap barrier:
  //   barrier | weight fragment reads of k-step 0 | weight DMA of a later tap (under their LDS
  //   round trip) | MFMAs of k-step 0 | A fragments of the NEXT tap's k-step 0 (into the
  //   registers k-step 0 just released) | MFMAs of k-step 1
  //   | the halo batch of this tap (store_halo: the GroupNorm affine + SiLU, ds_writes; then the
  //   next batch's loads) | A fragments of the next tap's k-step 1 | next barrier
  // sched_barrier(0) pins the seams: hipcc otherwise sinks all eight A reads behind the
  // last MFMA, where the wave then sat out their LDS round trip in front of the barrier, and
  // hoists the transform's VALU block in front of the MFMAs (where the source had it before).
  // The k-step 1 A reads are the wave's last LDS instructions of the tap and need not land before the
  // barrier (the halo image is stable within a chunk and nothing else reads their registers):
  // the tap's closing wait is lgkmcnt(FM), not 0.  LDS instructions of a wave complete in order, so
  // with at most FM outstanding every older one -- the weight fragment reads of the slot a later
  // DMA overwrites, store_halo's and store_par's writes the barrier publishes -- has completed;
  // the compiler's own counted lgkmcnt in front of the next tap's k-step 1 MFMAs covers the rest.
  auto tap = [&](int ci, int par, auto t_tag, auto last_tag) {
    constexpr int t = decltype(t_tag)::value;
    constexpr bool LAST = decltype(last_tag)::value;  // no next chunk
    const int g = NTAP * ci + t;
    const int hpar = ci & 1;  // the chunk's halo image (par: the weight ring's per-chunk value)
    // the weight DMA of tap g landed: VMEM instructions younger than it are the weights
    // of the NSW - 2 later taps and the halo batches issued at taps t - NSW + 1 .. t - 1
    // (HY only counts what may stay in flight behind the weights.  The halo registers themselves
    // are plain buffer loads: store_halo's use of them gets the compiler's own vmcnt wait -- in
    // the phase form already one tap after the load -- so no counted wait has to cover them.
    // A batch's loads now stand at the end of their tap instead of behind its weight DMA; they are
    // still younger than that DMA and older than the next tap's, so the counts are what they were)
    constexpr int HY = LAST ? 0 : (t - 1 >= 0 ? halo_issue(t - 1, NHL, GN, TS) : 0) +
                                  (NSW >= 3 && t - 2 >= 0 ? halo_issue(t - 2, NHL, GN, TS) : 0);
    if (g + NSW - 2 >= G) wait_vm<0>();  // the ring's tail
    else wait_vm<(NSW - 2) * DPT + HY>();
    // (t = 0 follows tap NTAP - 1, the prologue or nothing: no A reads in flight, all of it waited for)
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(t > 0 ? FM : 0) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const uint4* hb = hbuf + hpar * HALO;
    const uint4* wb = wbuf + wslot(par, t) * WSLOT;
    // A fragments of tap t: at t = 0 read here (the barrier above published the chunk's image);
    // for t > 0 read during tap t - 1, so after this tap's barrier only the k-step 0 weight
    // fragments stand between the wave and its MFMAs
    if constexpr (t == 0) {
      read_a(hb, 0, 0);
      read_a(hb, 0, 1);
    }
    auto read_b = [&](bf16x8* bfr, int ks) {
#pragma unroll
      for (int j = 0; j < FN; ++j)
        bfr[j] = __builtin_bit_cast(bf16x8, wb[swz64(wn * WTN + j * 16 + l16, ks * 4 + lg)]);
    };
    auto mfmas = [&](const bf16x8* bfr, int ks, int i0, int i1) {
#pragma unroll
      for (int i = i0; i < i1; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(apf[ks][i], bfr[j], acc[i][j], 0, 0, 0);
    };
    {
      bf16x8 bfr0[FN], bfr1[FN];
      read_b(bfr0, 0);
      // the weight DMA of a later tap (about 60 issue cycles per wave instruction) under the
      // LDS round trip of the fragment reads above, not in front of them
      __builtin_amdgcn_sched_barrier(0);
      if (g + NSW - 1 < G) issue_w(g + NSW - 1, wslot(par, t + NSW - 1));
      if constexpr (!LAST) {
        if constexpr (GN && t == 1) store_par(ci + 1);  // read at taps 3 / 6 / 8, past a barrier
        if constexpr (t == 0) load_halo(ci + 1, 0);     // (nothing to store yet: two loads, no VALU)
      }
      __builtin_amdgcn_sched_barrier(0);
      mfmas(bfr0, 0, 0, FM - 1);
      read_b(bfr1, 1);  // (under the last FN MFMAs of k-step 0, in front of the seam)
      mfmas(bfr0, 0, FM - 1, FM);
      if constexpr (t < NTAP - 1) {
        __builtin_amdgcn_sched_barrier(0);
        read_a(hb, t + 1, 0);
      }
      mfmas(bfr1, 1, 0, FM);
    }
    if constexpr (!LAST && (t == TS || t == 2 * TS || t == NTAP - 1)) {
      __builtin_amdgcn_sched_barrier(0);
      store_halo(hpar ^ 1, t == NTAP - 1 ? 2 : t / TS - 1);
      if constexpr (t < NTAP - 1) load_halo(ci + 1, t / TS);
    }
    if constexpr (t < NTAP - 1) {
      __builtin_amdgcn_sched_barrier(0);
      read_a(hb, t + 1, 1);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
  using I4 = std::integral_constant<int, 4>; using I5 = std::integral_constant<int, 5>;
  using I6 = std::integral_constant<int, 6>; using I7 = std::integral_constant<int, 7>;
  using I8 = std::integral_constant<int, 8>;
  auto chunk = [&](int ci, auto last) {
    const int par = PH && NSW == 3 ? ci % 3 : ci & 1;
    tap(ci, par, I0{}, last); tap(ci, par, I1{}, last); tap(ci, par, I2{}, last);
    tap(ci, par, I3{}, last);
    if constexpr (!PH) {
      tap(ci, par, I4{}, last); tap(ci, par, I5{}, last);
      tap(ci, par, I6{}, last); tap(ci, par, I7{}, last); tap(ci, par, I8{}, last);
    }
  };
  for (int ci = 0; ci + 1 < nchunk; ++ci) chunk(ci, std::false_type{});
  chunk(nchunk - 1, std::true_type{});
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  // epilogue: virtual rows (GroupNorm slots) = the patch's index within its image x 256
  // (phase form: the output image has 4 HW pixels; the block's TH x TW stored pixels fill the
  // slots of patch (ph, tyb, txb) -- every output pixel once, every slot 128 stored rows)
  const int m0v = PH ? (int)(img * 4 * HW) + ((ph * tpc + tyb) * tpr + txb) * (TH * TW)
                     : (int)(img * HW) + (tyb * tpr + txb) * (TH * TW);
  const long m0r = PH ? img * 4 * HW + (long)(2 * y0 + py) * a.Wo + 2 * x0 + px : img * HW + (long)y0 * a.W + x0;
  // column sums from per-thread register partials (CSG = 2: store_tile_plain_pre's slot-end form)
  static_assert((size_t)(NT / (BN / 8)) * BN * 2 * 4 <= (size_t)2 * HALO * 16, "column-sum partials fit the halo images");
  store_tile_plain<TH * TW, BN, TH / 4, WNW, false, CSF, PH ? -TW : TW, 2>(a, acc, (float*)lds_dyn, m0v, n0, m0r);
}

// whether the halo conv takes this call
bool halo_ok(const ls_conv_desc* d, const ConvArgs& a) {
  if (!g_tune.halo || g_tune.force_tile || g_tune.force_regstage || d->ksize != 3 || a.stride != 1 || a.pad != 1 ||
      !a.ccm || a.Cin % 64 || a.C1 % 64 || a.K != (a.upsample == 2 ? 4 : 9) * a.Cin || a.y_f32 || a.act != LS_ACT_NONE ||
      a.ln_mr || a.stats_out || a.ldy % 8 || (a.res && a.ldr % 8))
    return false;
  // nearest x2 upsample (Upsample3D, resnet.py:53-71; round 6): no input affine (the UNet's
  // upsampler conv has none); the halo image is built in output space from the input pixels
  if (a.upsample ? (!g_tune.halo_ups || a.aff_scale || a.Ho != 2 * a.H || a.Wo != 2 * a.W) : (a.Ho != a.H || a.Wo != a.W))
    return false;
  // N <= 640: with more output channels the patch is re-loaded and re-transformed per N tile
  // and the tiled 256x256 kernel wins (VAE 512 channels at 32^2: 3667 vs 3409 us; 128 at
  // 256^2: 18660 vs 23610 us incl. the materialised GroupNorm; profiles/r04f_ab_t256_halo.txt)
  // (N = 8 / 16: the narrow tile -- conv_out of the VAE decoder / encoder, N padded to 8)
  const bool narrow = a.N % 8 == 0 && a.N <= 16 && a.H % 8 == 0 && g_tune.halo_narrow;
  if (((a.N % 160 && a.N % 128) || a.N > 640) && !narrow) return false;
  if (a.aff_scale && (!a.silu_in || a.pix_per_sample % (a.H * a.W) || ((uintptr_t)a.aff_scale | (uintptr_t)a.aff_shift) & 15))
    return false;  // (the kernel's input transform is the GroupNorm affine + SiLU of a ResnetBlock)
  if (((uintptr_t)a.x1 | (uintptr_t)a.x2 | (uintptr_t)a.w) & 15 || a.ld1 % 8 || (a.C2 && a.ld2 % 8)) return false;
  // 16 x 16 patches everywhere (the only patch width compiled): the smallest halo overhead
  // ((16 + 2)^2 / 256 = 1.27 input pixels per output pixel; 32 x 8: 1.33, 64 x 4: 1.55) and no
  // register spills (the phase form of an upsample conv, upsample == 2, patches the INPUT image)
  if (a.upsample == 2 ? a.W % 16 || a.H % 16 : a.Wo % 16 || a.Ho % 16) return false;
  if (a.upsample == 2 && (a.N <= 16 || a.C2)) return false;  // (no narrow tile, one source)
  if ((long)a.H * a.W * a.ld1 * 2 >= (1L << 31) || (a.C2 && (long)a.H * a.W * a.ld2 * 2 >= (1L << 31)))
    return false;  // per-image buffer descriptors
  return true;
}

// f(BN, TH) over the compiled halo tiles
template <class F>
static void with_halo_tile(const ls_conv_plan_info& i, F f) {
  if (i.halo_bn == 16) f(IC<16>{}, IC<8>{});
  else if (i.halo_bn == 160) f(IC<160>{}, IC<16>{});
  else if (i.halo_th == 8) f(IC<128>{}, IC<8>{});
  else f(IC<128>{}, IC<16>{});
}

// The halo kernel's arguments, tile and grid (halo_ok holds).  One tile choice for the plain
// and the phase form (upsample == 2: input-space patches, the output parity a grid dimension).
void plan_halo(ConvPlan& p) {
  ConvArgs& a = p.a;
  ls_conv_plan_info& i = p.i;
  i.halo_ph = a.upsample == 2;
  i.family = i.halo_ph ? 4 : 3;
  if (i.halo_ph) {
    a.upsample = 0;  // (the kernel's halo image is the plain input-space one)
  } else if (a.upsample) {  // the kernel works in output space: H, W = the output image
    a.H = a.Ho;
    a.W = a.Wo;
  }
  i.halo_bn = a.N <= 16 ? 16 : (a.N % 160 == 0 && !(g_tune.halo_bn128 && a.N % 128 == 0)) ? 160 : 128;
  i.halo_th = i.halo_bn == 16 || (i.halo_bn == 128 && g_tune.halo_th8 && a.Cin <= 256) ? 8 : 16;  // (H % 16 == 0)
  i.halo_gn = a.aff_scale != nullptr;
  i.halo_cs = a.cs_out != nullptr;
  with_halo_tile(i, [&](auto bn, auto th) {
    using HC = HaloCfg<16, decltype(bn)::value, decltype(th)::value>;
    i.threads = HC::NT;
    i.lds_bytes = (int)HC::SHM;
  });
  i.grid = a.n_img * (a.H / i.halo_th) * (a.W / 16) * cdiv(a.N, i.halo_bn) * (i.halo_ph ? 4 : 1);
}

template <int BN, int TH, bool PH>
static void launch_halo2(const ConvPlan& p, hipStream_t s) {
  if constexpr (!PH) {  // (the phase form takes no input affine)
    if (p.i.halo_gn)
      return p.i.halo_cs ? launch_plan<conv3x3_halo_kernel<16, BN, true, true, TH>>(p, s)
                         : launch_plan<conv3x3_halo_kernel<16, BN, true, false, TH>>(p, s);
  }
  p.i.halo_cs ? launch_plan<conv3x3_halo_kernel<16, BN, false, true, TH, PH>>(p, s)
              : launch_plan<conv3x3_halo_kernel<16, BN, false, false, TH, PH>>(p, s);
}

void launch_halo(const ConvPlan& p, hipStream_t s) {
  with_halo_tile(p.i, [&](auto bn, auto th) {
    constexpr int BN = decltype(bn)::value, TH = decltype(th)::value;
    if constexpr (BN != 16) {  // (halo_ok: the phase form has no narrow tile)
      if (p.i.halo_ph) return launch_halo2<BN, TH, true>(p, s);
    }
    launch_halo2<BN, TH, false>(p, s);
  });
}

}  // namespace ls
