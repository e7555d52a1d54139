// Motion-JPEG encoder on gfx950: the restored clip, uint8 RGB (n, H, W, 3) on the device,
// becomes the entropy-coded scan of one baseline JPEG per frame (what ffmpeg's encoder does
// for the reference's write_video, util.py:140-160).  The host wraps each scan in its JFIF
// headers (latentsync_amd/video.py); only compressed bytes and offsets cross to the host.
//
// Format: baseline sequential, 8-bit, YCbCr 4:2:0 (16x16 MCUs: Y0 Y1 Y2 Y3 Cb Cr), the
// Annex K quantisation tables scaled by the libjpeg quality rule, the Annex K Huffman
// tables, a restart interval of MJ_RI MCUs.  All arithmetic is integer and equals libjpeg's
// (jccolor.c rgb_ycc_convert, jcsample.c h2v2_downsample, jfdctint.c jpeg_fdct_islow,
// jcdctmgr.c forward_DCT's quantiser); DESIGN.md section 4.2 holds the exact definition.
// Pixels past the right / bottom edge of the frame replicate the last column / row up to
// the MCU boundary; chroma rows past the last one of the subsampled plane replicate it.
//
//  * mjpeg_transform_kernel: one workgroup owns MJ_G horizontally adjacent MCUs.  The 16
//    interleaved RGB row segments are read as aligned dwords into LDS (coalesced whatever
//    3 * W and the frame's byte offset are modulo 4), one thread per 2x2 pixel quad
//    converts to Y / Cb / Cr and averages the chroma, then 8 threads per 8x8 block run
//    the row pass and the column pass of the DCT through LDS, quantise, and the zigzag
//    int16 coefficients leave as one coalesced run.
//  * mjpeg_entropy_kernel: one wave per (frame, restart interval), one lane per block.
//    Each lane counts its block's bits, a wave scan gives bit offsets, the lanes OR their
//    codes into an LDS bit buffer (ds_or_b32: neighbouring blocks share words), the last
//    byte is padded with 1 bits, and a second scan over the bytes inserts the 0x00 after
//    every 0xFF on the way to the interval's slot of the workspace.  The slot is sized
//    from the worst case (every block 22 + 63 * 26 = 1660 bits, every byte stuffed), so it
//    cannot overflow.
//  * mjpeg_offsets_kernel: prefix sums of the interval sizes (+ 2 for each RSTm marker)
//    -> the absolute position of every interval and offsets[f + 1].
//  * mjpeg_pack_kernel: copies every interval to its position and appends RSTm (m = the
//    interval index modulo 8; none after the last).  Writes past `out_capacity` are
//    dropped, offsets stay exact, so the caller can detect a short buffer and retry.
// Frames go through in batches of a fixed workspace budget: the workspace does not grow
// with n.  Every pixel and byte index is 64-bit.
#include "ls_common.h"

namespace ls {

constexpr int MJ_RI = 10;                     // MCUs per restart interval
constexpr int MJ_BLK = MJ_RI * 6;             // blocks per interval <= 64 lanes
constexpr int MJ_BLOCK_BITS = 22 + 63 * 26;   // DC cat 11 (11 + 11) + 63 x (16-bit code + 10 bits)
constexpr int MJ_IV_BYTES = (MJ_BLK * MJ_BLOCK_BITS + 7) / 8;  // 12450 before stuffing
constexpr int MJ_BITBUF_DW = (MJ_IV_BYTES + 3) / 4 + 2;        // + the spill word of the last flush
constexpr int MJ_SLOT = (2 * MJ_IV_BYTES + 63) / 64 * 64;      // every byte stuffed: 24960
constexpr int MJ_G = 4;                       // MCUs per transform workgroup
constexpr int MJ_TW = 16 * MJ_G;              // its width in pixels
constexpr int MJ_ROW_DW = MJ_TW * 3 / 4 + 2;  // dwords of one staged row segment (+ misalignment)
constexpr int MJ_MCU_COEF = 6 * 64;
constexpr int MJ_CF_LD = 66;                  // int16 per block in LDS: 33 dwords, conflict-free
constexpr size_t MJ_WS_BUDGET = (size_t)96 << 20;
constexpr int MJ_MAX_BATCH = 1024;
static_assert(MJ_BLK <= 64, "one lane per block of an interval");

__device__ const uint8_t MJ_QBASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// natural (row-major) index -> zigzag position
__device__ const uint8_t MJ_ZZ_OF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                         3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                         10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                         21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// Annex K.3 Huffman tables as (BITS, HUFFVAL); entry [symbol] = length << 16 | code
struct MjHuff {
  uint32_t e[256];
};
struct MjSpec {
  uint8_t bits[16];
  uint8_t vals[162];
};
constexpr MjSpec MJ_DC_L = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr MjSpec MJ_DC_C = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr MjSpec MJ_AC_L = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr MjSpec MJ_AC_C = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

constexpr MjHuff mj_make_huff(const MjSpec& s) {
  MjHuff h{};
  int k = 0;
  uint32_t code = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.bits[len - 1]; ++i) h.e[s.vals[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
  return h;
}
// [0] DC luma, [1] DC chroma, [2] AC luma, [3] AC chroma
__device__ const MjHuff MJ_HT[4] = {mj_make_huff(MJ_DC_L), mj_make_huff(MJ_DC_C), mj_make_huff(MJ_AC_L),
                                    mj_make_huff(MJ_AC_C)};

// jfdctint.c: CONST_BITS 13, PASS1_BITS 2
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633,
              F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 8-point pass of jpeg_fdct_islow.  PASS2 = false: the row pass (even outputs scaled
// up by PASS1_BITS, odd ones descaled by CONST_BITS - PASS1_BITS); true: the column pass.
template <bool PASS2>
__device__ __forceinline__ void fdct8(const int* d, int* o) {
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int SH = PASS2 ? 13 + 2 : 13 - 2;
  if (PASS2) {
    o[0] = descale(tmp10 + tmp11, 2);
    o[4] = descale(tmp10 - tmp11, 2);
  } else {
    o[0] = (tmp10 + tmp11) << 2;
    o[4] = (tmp10 - tmp11) << 2;
  }
  int z1 = (tmp12 + tmp13) * F_0_541;
  o[2] = descale(z1 + tmp13 * F_0_765, SH);
  o[6] = descale(z1 - tmp12 * F_1_847, SH);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * F_1_175;
  const int t4 = tmp4 * F_0_298, t5 = tmp5 * F_2_053, t6 = tmp6 * F_3_072, t7 = tmp7 * F_1_501;
  z1 *= -F_0_899;
  z2 *= -F_2_562;
  z3 = z3 * -F_1_961 + z5;
  z4 = z4 * -F_0_390 + z5;
  o[7] = descale(t4 + z1 + z3, SH);
  o[5] = descale(t5 + z2 + z4, SH);
  o[3] = descale(t6 + z2 + z3, SH);
  o[1] = descale(t7 + z1 + z4, SH);
}

__global__ void __launch_bounds__(256)
mjpeg_transform_kernel(const uint8_t* __restrict__ frames, int H, int W, int mcux, int qscale,
                       int16_t* __restrict__ coef) {
  __shared__ uint32_t rgb[16][MJ_ROW_DW];
  __shared__ uint8_t ypl[16][MJ_TW];
  __shared__ uint8_t cpl[2][8][MJ_TW / 2];
  __shared__ int ws[MJ_G * 6][8][9];
  __shared__ uint16_t qt8[2][64];  // divisors: 8 * the quantisation step (the DCT's output scale)
  __shared__ uint32_t outz[MJ_G * MJ_MCU_COEF / 2];
  const int tid = threadIdx.x;
  const int g = blockIdx.x, my = blockIdx.y, f = blockIdx.z;
  const int nmcu_y = gridDim.y;
  const int x0 = g * MJ_TW, y0 = my * 16;
  const int wvalid = min(MJ_TW, W - x0);  // >= 1: the grid covers cdiv(mcux, MJ_G) groups
  const uint8_t* fr = frames + (long)f * H * W * 3;

  if (tid < 128) {
    int q = ((int)MJ_QBASE[tid >> 6][tid & 63] * qscale + 50) / 100;
    q = q < 1 ? 1 : (q > 255 ? 255 : q);
    qt8[tid >> 6][tid & 63] = (uint16_t)(q << 3);
  }
  // Stage the row segments as the aligned dwords that contain them.  The first and the
  // last dword of a segment may reach up to 3 bytes outside the tensor, never outside
  // the aligned dword (hence the page) that holds a byte of it.
  for (int i = tid; i < 16 * MJ_ROW_DW; i += 256) {
    const int r = i / MJ_ROW_DW, d = i - r * MJ_ROW_DW;
    const int y = min(y0 + r, H - 1);
    const uintptr_t a = (uintptr_t)(fr + ((long)y * W + x0) * 3);
    const int ndw = ((int)(a & 3) + wvalid * 3 + 3) >> 2;
    if (d < ndw) rgb[r][d] = *(const uint32_t*)((a & ~(uintptr_t)3) + 4 * (uintptr_t)d);
  }
  __syncthreads();
  {  // one 2x2 quad per thread: jccolor.c rgb_ycc_convert + jcsample.c h2v2_downsample
    const int qx = tid & 31, qy = tid >> 5;
    int cb = 0, cr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int r = 2 * qy + dy;
      const int y = min(y0 + r, H - 1);
      const int mis = (int)((uintptr_t)(fr + ((long)y * W + x0) * 3) & 3);
      const uint8_t* row = (const uint8_t*)rgb[r] + mis;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int x = 2 * qx + dx;
        const uint8_t* p = row + 3 * min(x, wvalid - 1);
        const int R = p[0], G = p[1], B = p[2];
        ypl[r][x] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
        cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
        cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
      }
    }
    const int bias = 1 + (qx & 1);  // 1, 2, 1, 2, ... along a chroma row (x0 / 2 is even)
    cpl[0][qy][qx] = (uint8_t)((cb + bias) >> 2);
    cpl[1][qy][qx] = (uint8_t)((cr + bias) >> 2);
  }
  __syncthreads();
  const int b = tid >> 3, l = tid & 7;  // block of the group, row (pass 1) / column (pass 2)
  const int m = b / 6, c = b - m * 6;
  if (b < MJ_G * 6) {
    int d[8], o[8];
    // chroma rows below the plane's last one, (H - 1) / 2, replicate it (libjpeg pads the
    // downsampled rows, not the full-resolution ones)
    const int lastc = min(7, ((H - 1) >> 1) - (y0 >> 1));
    const uint8_t* src = c < 4 ? &ypl[(c >> 1) * 8 + l][m * 16 + (c & 1) * 8] : &cpl[c - 4][min(l, lastc)][m * 8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = (int)src[k] - 128;
    fdct8<false>(d, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) ws[b][l][k] = o[k];
  }
  __syncthreads();
  if (b < MJ_G * 6) {
    int d[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = ws[b][k][l];
    fdct8<true>(d, o);
    int16_t* oz = (int16_t*)outz + b * 64;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int nat = k * 8 + l;
      const unsigned q8 = qt8[c < 4 ? 0 : 1][nat];
      const int v = o[k];
      // jcdctmgr.c: round half away from zero; AC clamped to +-1023 (category 10)
      int a = (int)(((unsigned)(v < 0 ? -v : v) + (q8 >> 1)) / q8);
      if (nat != 0 && a > 1023) a = 1023;
      oz[MJ_ZZ_OF[nat]] = (int16_t)(v < 0 ? -a : a);
    }
  }
  __syncthreads();
  const int nv = min(MJ_G, mcux - g * MJ_G);  // MCUs of this group inside the frame
  const long nmcu = (long)mcux * nmcu_y;
  uint32_t* dst = (uint32_t*)(coef + ((long)f * nmcu + (long)my * mcux + (long)g * MJ_G) * MJ_MCU_COEF);
  for (int i = tid; i < nv * (MJ_MCU_COEF / 2); i += 256) dst[i] = outz[i];
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ int mj_nbits(int v) { return 32 - __clz(v < 0 ? -v : v); }  // 0 for v == 0 (clz(0) = 32)

// MSB-first bit writer of one lane into the shared LDS bit buffer
struct MjBits {
  uint32_t* buf;
  uint64_t acc;
  int nacc, w;
  __device__ __forceinline__ void put(uint32_t v, int n) {  // 1 <= n <= 26, nacc < 32
    acc |= (uint64_t)v << (64 - nacc - n);
    nacc += n;
    if (nacc >= 32) {
      atomicOr(&buf[w++], (uint32_t)(acc >> 32));
      acc <<= 32;
      nacc -= 32;
    }
  }
};

__global__ void __launch_bounds__(64)
mjpeg_entropy_kernel(const int16_t* __restrict__ coef, int nmcu, int nint, uint8_t* __restrict__ slots,
                     int* __restrict__ sizes) {
  __shared__ uint32_t ht[4][256];
  __shared__ uint32_t cf[MJ_BLK * MJ_CF_LD / 2];
  __shared__ uint32_t bits[MJ_BITBUF_DW];
  const int lane = threadIdx.x;
  const int k = blockIdx.x, f = blockIdx.y;
  const int mcu0 = k * MJ_RI;
  const int nb = min(MJ_RI, nmcu - mcu0) * 6;
  for (int i = lane; i < 4 * 256; i += 64) (&ht[0][0])[i] = (&MJ_HT[0].e[0])[i];
  const uint32_t* src = (const uint32_t*)(coef + ((long)f * nmcu + mcu0) * MJ_MCU_COEF);
  for (int i = lane; i < nb * 32; i += 64) cf[(i >> 5) * (MJ_CF_LD / 2) + (i & 31)] = src[i];
  __syncthreads();
  const bool active = lane < nb;
  const int comp = lane % 6;
  const int16_t* c = (const int16_t*)cf + lane * MJ_CF_LD;
  const uint32_t* dct = ht[comp < 4 ? 0 : 1];
  const uint32_t* act = ht[comp < 4 ? 2 : 3];
  int diff = 0, total = 0;
  if (active) {
    // DC predictor: the previous block of the same component in the interval, 0 at its start
    const int16_t* all = (const int16_t*)cf;
    int pred;
    if (comp == 0) pred = lane >= 6 ? all[(lane - 3) * MJ_CF_LD] : 0;
    else if (comp < 4) pred = all[(lane - 1) * MJ_CF_LD];
    else pred = lane >= 6 ? all[(lane - 6) * MJ_CF_LD] : 0;
    diff = (int)c[0] - pred;
    diff = diff < -2047 ? -2047 : (diff > 2047 ? 2047 : diff);
    const int cat = mj_nbits(diff);
    total = (int)(dct[cat] >> 16) + cat;
    int run = 0;
    for (int i = 1; i < 64; ++i) {
      const int v = c[i];
      if (v == 0) {
        ++run;
      } else {
        total += (run >> 4) * (int)(act[0xF0] >> 16);
        const int n = mj_nbits(v);
        total += (int)(act[((run & 15) << 4) | n] >> 16) + n;
        run = 0;
      }
    }
    if (run) total += (int)(act[0] >> 16);
  }
  const int incl = wave_incl_scan(total, lane);
  const int total_bits = __shfl(incl, 63, 64);
  const int start = incl - total;
  const int nbytes = (total_bits + 7) >> 3;
  for (int i = lane; i < (nbytes + 3) / 4 + 2; i += 64) bits[i] = 0;  // <= MJ_BITBUF_DW: nbytes <= MJ_IV_BYTES
  __syncthreads();
  if (active) {
    MjBits bw{bits, 0, start & 31, start >> 5};
    const int cat = mj_nbits(diff);
    const uint32_t e = dct[cat];
    bw.put(((e & 0xffff) << cat) | ((uint32_t)(diff + (diff >> 31)) & ((1u << cat) - 1)), (int)(e >> 16) + cat);
    int run = 0;
    for (int i = 1; i < 64; ++i) {
      const int v = c[i];
      if (v == 0) {
        ++run;
      } else {
        for (; run >= 16; run -= 16) bw.put(act[0xF0] & 0xffff, (int)(act[0xF0] >> 16));
        const int n = mj_nbits(v);
        const uint32_t a = act[(run << 4) | n];
        bw.put(((a & 0xffff) << n) | ((uint32_t)(v + (v >> 31)) & ((1u << n) - 1)), (int)(a >> 16) + n);
        run = 0;
      }
    }
    if (run) bw.put(act[0] & 0xffff, (int)(act[0] >> 16));
    if (bw.nacc) atomicOr(&bits[bw.w], (uint32_t)(bw.acc >> 32));
  }
  if (lane == 0) {  // pad the last byte with 1 bits
    const int pad = (8 - (total_bits & 7)) & 7;
    if (pad) atomicOr(&bits[total_bits >> 5], ((1u << pad) - 1) << (32 - (total_bits & 31) - pad));
  }
  __syncthreads();
  // byte stuffing: lane l owns bytes [l * chunk, (l + 1) * chunk), chunk a multiple of 4
  const int chunk = (((nbytes + 63) >> 6) + 3) & ~3;
  const int b0 = lane * chunk, b1 = min(nbytes, b0 + chunk);
  int nff = 0;
  for (int i = b0; i < b1; i += 4) {
    const uint32_t w = bits[i >> 2];
#pragma unroll
    for (int j = 0; j < 4; ++j) nff += (i + j < b1) && ((w >> (24 - 8 * j)) & 0xff) == 0xff;
  }
  const int ffi = wave_incl_scan(nff, lane);
  uint8_t* dst = slots + ((long)f * nint + k) * MJ_SLOT + b0 + (ffi - nff);
  for (int i = b0; i < b1; i += 4) {
    const uint32_t w = bits[i >> 2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < b1) {
        const uint8_t v = (uint8_t)(w >> (24 - 8 * j));
        *dst++ = v;
        if (v == 0xff) *dst++ = 0;
      }
    }
  }
  if (lane == 63) sizes[(long)f * nint + k] = nbytes + ffi;
}

// One workgroup: pos[f][k] = offsets[0] + bytes of everything before interval k of frame f
// (each interval but the last of a frame is followed by a 2-byte RSTm), offsets[f + 1].
__global__ void __launch_bounds__(256)
mjpeg_offsets_kernel(const int* __restrict__ sizes, int nint, int nf, long* __restrict__ pos,
                     long* __restrict__ offsets) {
  __shared__ long wsum[4];
  __shared__ long carry;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry = offsets[0];
  __syncthreads();
  for (int f = 0; f < nf; ++f) {
    for (int base = 0; base < nint; base += 256) {
      const int i = base + tid;
      const int v = i < nint ? sizes[(long)f * nint + i] + (i < nint - 1 ? 2 : 0) : 0;
      const int incl = wave_incl_scan(v, lane);
      if (lane == 63) wsum[wv] = incl;
      __syncthreads();
      long before = carry;
      for (int w = 0; w < wv; ++w) before += wsum[w];
      if (i < nint) pos[(long)f * nint + i] = before + incl - v;
      __syncthreads();
      if (tid == 255) carry = before + incl;
      __syncthreads();
    }
    if (tid == 0) offsets[f + 1] = carry;
  }
}

__global__ void __launch_bounds__(64)
mjpeg_pack_kernel(const uint8_t* __restrict__ slots, const int* __restrict__ sizes, const long* __restrict__ pos,
                  int nint, uint8_t* __restrict__ out, long capacity) {
  const int k = blockIdx.x, f = blockIdx.y;
  const long iv = (long)f * nint + k;
  const uint8_t* src = slots + iv * MJ_SLOT;
  const int n = sizes[iv];
  const long p = pos[iv];
  for (int i = threadIdx.x; i < n; i += 64)
    if (p + i < capacity) out[p + i] = src[i];
  if (k < nint - 1 && threadIdx.x < 2 && p + n + threadIdx.x < capacity)
    out[p + n + threadIdx.x] = threadIdx.x == 0 ? 0xff : (uint8_t)(0xd0 + (k & 7));
}

struct MjGeom {
  int mcux, mcuy, nint, batch;
  long nmcu;
  size_t coef_b, slot_b, size_b, pos_b;  // per frame, each a multiple of 256
};

static bool mj_geom(int n, int H, int W, MjGeom* g) {
  if (n < 1 || H < 1 || W < 1 || H > 65535 || W > 65535) return false;  // SOF0 holds 16-bit sizes
  g->mcux = (W + 15) / 16;
  g->mcuy = (H + 15) / 16;
  g->nmcu = (long)g->mcux * g->mcuy;
  if (g->nmcu > 800000) return false;  // one frame's worst case stays below 2^31 bytes
  g->nint = (int)((g->nmcu + MJ_RI - 1) / MJ_RI);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  g->coef_b = up((size_t)g->nmcu * MJ_MCU_COEF * 2);
  g->slot_b = up((size_t)g->nint * MJ_SLOT);
  g->size_b = up((size_t)g->nint * 4);
  g->pos_b = up((size_t)g->nint * 8);
  const size_t per = g->coef_b + g->slot_b + g->size_b + g->pos_b;
  size_t b = MJ_WS_BUDGET / per;
  b = b < 1 ? 1 : b;
  b = b > (size_t)MJ_MAX_BATCH ? MJ_MAX_BATCH : b;
  g->batch = (int)(b > (size_t)n ? n : b);
  return true;
}

}  // namespace ls

using namespace ls;

extern "C" int ls_mjpeg_restart_interval(void) { return MJ_RI; }

extern "C" size_t ls_mjpeg_workspace_bytes(int32_t n, int32_t H, int32_t W) {
  MjGeom g;
  if (!mj_geom(n, H, W, &g)) return 0;
  return (size_t)g.batch * (g.coef_b + g.slot_b + g.size_b + g.pos_b) + 256;
}

extern "C" int ls_mjpeg_encode(const uint8_t* frames, int32_t n, int32_t H, int32_t W, int32_t quality, uint8_t* out,
                               int64_t out_capacity, int64_t* offsets, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (!frames || !out || !offsets) return fail(LS_ERR_INVALID, "ls_mjpeg_encode: null pointer");
  if (quality < 1 || quality > 100)
    return fail(LS_ERR_INVALID, "ls_mjpeg_encode: quality " + std::to_string(quality) + " outside 1..100");
  if (out_capacity < 0) return fail(LS_ERR_INVALID, "ls_mjpeg_encode: negative out_capacity");
  MjGeom g;
  if (!mj_geom(n, H, W, &g))
    return fail(LS_ERR_INVALID, "ls_mjpeg_encode: need n >= 1, 1 <= H, W <= 65535 and at most 800000 MCUs per frame");
  if (!workspace || workspace_bytes < ls_mjpeg_workspace_bytes(n, H, W))
    return fail(LS_ERR_WORKSPACE, "ls_mjpeg_encode: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  int16_t* coef = (int16_t*)ws;
  uint8_t* slots = (uint8_t*)(ws + (size_t)g.batch * g.coef_b);
  int* sizes = (int*)((char*)slots + (size_t)g.batch * g.slot_b);
  long* pos = (long*)((char*)sizes + (size_t)g.batch * g.size_b);
  const int qscale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  if (hipMemsetAsync(offsets, 0, sizeof(int64_t), s) != hipSuccess)
    return fail(LS_ERR_LAUNCH, "ls_mjpeg_encode: memset");
  const size_t frame_bytes = (size_t)H * W * 3;
  for (int f0 = 0; f0 < n; f0 += g.batch) {
    const int nf = std::min(g.batch, n - f0);
    mjpeg_transform_kernel<<<dim3((g.mcux + MJ_G - 1) / MJ_G, g.mcuy, nf), 256, 0, s>>>(
        frames + (size_t)f0 * frame_bytes, H, W, g.mcux, qscale, coef);
    if (int rc = check_launch("mjpeg_transform_kernel")) return rc;
    mjpeg_entropy_kernel<<<dim3(g.nint, nf), 64, 0, s>>>(coef, (int)g.nmcu, g.nint, slots, sizes);
    if (int rc = check_launch("mjpeg_entropy_kernel")) return rc;
    mjpeg_offsets_kernel<<<1, 256, 0, s>>>(sizes, g.nint, nf, pos, (long*)offsets + f0);
    if (int rc = check_launch("mjpeg_offsets_kernel")) return rc;
    mjpeg_pack_kernel<<<dim3(g.nint, nf), 64, 0, s>>>(slots, sizes, pos, g.nint, out, (long)out_capacity);
    if (int rc = check_launch("mjpeg_pack_kernel")) return rc;
  }
  return LS_OK;
}
