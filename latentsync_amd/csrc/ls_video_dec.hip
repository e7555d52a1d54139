// Motion-JPEG decoder on gfx950: the inverse of ls_video.hip.  The entropy-coded scans of n
// baseline JPEG frames, already on the device, become uint8 RGB (n, H, W, 3).  The host
// (latentsync_amd/video.py parse_jpeg) reads only the segments in front of each scan and
// builds the per-frame descriptors and the deduplicated quantiser / Huffman tables; only
// compressed bytes cross to the device.
//
// Subset: 8-bit baseline, one interleaved scan, greyscale or YCbCr with chroma 1x1 and luma
// 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0), any restart interval, any Huffman tables.  All
// arithmetic is integer and equals libjpeg's (jdhuff.c decode_mcu, jidctint.c
// jpeg_idct_islow with a saturating range limit, jdsample.c h2v1 / h2v2 fancy upsampling,
// jdcolor.c ycc_rgb_convert); DESIGN.md section 4.3 holds the exact definition.
//
//  * mjd_markers_kernel: one workgroup per frame walks the scan in tiles and finds the
//    FF D0..D7 pairs (inside entropy-coded data an FF is followed only by 00, FF or a
//    marker), writing the byte after each pair in stream order: the segment starts.  The
//    count must be ceil(MCUs / Ri) - 1 and the k-th marker RST(k mod 8), else the frame's
//    status is set.
//  * mjd_entropy_kernel: one lane per (frame, restart segment) -- the DC predictors reset
//    at every marker, so segments are independent.  A frame gets up to MJD_MAX_WAVES waves,
//    each with the frame's table set in LDS; a lane loops when there are more segments
//    than lanes.  jdhuff.c's decode: an 8-bit lookahead table, maxcode / valoffset for
//    longer codes.  Only non-zero coefficients are stored, into the zero-filled int16
//    buffer in natural order.  Every byte index is checked against the segment's end
//    before the load and bytes past the end are zero bits; a code longer than 16 bits, a
//    coefficient index past 63 or a segment that runs out before its MCUs sets the frame's
//    status and stops the lane.  This kernel is divergent and serial by nature: its
//    parallelism is frames x segments, one lane per frame for a file without DRI.
//  * mjd_idct_kernel: 8 threads per block, dequantise + column pass + row pass through LDS,
//    + 128, clamp, one 8-byte store per row into the component's uint8 plane.
//  * mjd_colour_kernel: one workgroup per 256 pixels of an output row: chroma upsampled
//    from the planes, YCbCr -> RGB, staged in LDS and written as aligned dwords whatever
//    3 * W and the row's byte offset are modulo 4.
// Frames go through in batches of a fixed workspace budget: the workspace does not grow
// with n.  Every pixel and byte index is 64-bit.
#include "ls_common.h"

namespace ls {

constexpr size_t MJD_WS_BUDGET = (size_t)512 << 20;
constexpr int MJD_MAX_BATCH = 1024;
constexpr int MJD_MAX_WAVES = 16;     // entropy waves per frame: 1024 lanes before a lane loops
constexpr int MJD_DESC = 8;           // int64 per frame descriptor
constexpr int MJD_HT_LOOK = 0;        // uint16 [256]: length << 8 | symbol of every code up to 8 bits, 0 = longer
constexpr int MJD_HT_MAXCODE = 128;   // int32 [18]: largest code of length l, -1 = none, [17] = sentinel
constexpr int MJD_HT_VALOFF = 146;    // int32 [18]: huffval index of the first code of length l, minus that code
constexpr int MJD_HT_VAL = 164;       // uint8 [256]
constexpr int MJD_HT_INTS = 228;
constexpr int MJD_TILE = 2048;        // bytes of a scan one marker-search step covers (8 per thread)

enum { MJD_ST_DESC = 1, MJD_ST_MARKERS = 2, MJD_ST_CODE = 3, MJD_ST_INDEX = 4, MJD_ST_SHORT = 5 };

// zigzag position -> natural (row-major) index
__device__ const uint8_t MJD_NAT_OF[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                           12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                           58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Geometry of one frame for a sampling mode: 0 grey, 1 4:4:4, 2 4:2:2 (luma 2x1), 3 4:2:0 (luma 2x2)
struct MjdLayout {
  int ncomp, hs, vs;       // components; luma blocks per MCU across / down
  int mcux, mcuy;          // MCUs per row / column
  int bw[3], bh[3];        // blocks per row / column of each component's padded plane
  long off[3];             // first block of each component in the frame's buffers
  long nblocks;
  __host__ __device__ int bwc(int c) const { return c ? bw[1] : bw[0]; }  // selects: indexing by c would go through scratch
  __host__ __device__ long offc(int c) const { return c == 0 ? 0 : (c == 1 ? off[1] : off[2]); }
};

__host__ __device__ inline MjdLayout mjd_layout(int mode, int H, int W) {
  MjdLayout g;
  g.ncomp = mode == 0 ? 1 : 3;
  g.hs = mode >= 2 ? 2 : 1;
  g.vs = mode == 3 ? 2 : 1;
  g.mcux = (W + 8 * g.hs - 1) / (8 * g.hs);
  g.mcuy = (H + 8 * g.vs - 1) / (8 * g.vs);
  g.bw[0] = g.mcux * g.hs;
  g.bh[0] = g.mcuy * g.vs;
  g.bw[1] = g.bw[2] = g.mcux;
  g.bh[1] = g.bh[2] = g.mcuy;
  g.off[0] = 0;
  g.off[1] = (long)g.bw[0] * g.bh[0];
  g.off[2] = g.off[1] + (long)g.mcux * g.mcuy;
  g.nblocks = g.ncomp == 1 ? g.off[1] : g.off[2] + (long)g.mcux * g.mcuy;
  return g;
}

// What a kernel needs of a frame's descriptor (int64 [8], built by the host):
// [0] first byte of the scan in `data`, [1] its length, [2] restart interval (0 = none),
// [3] sampling mode, [4] quantiser index of component c in bits 16c..16c+15,
// [5] DC table index likewise, [6] AC table index likewise, [7] reserved.
struct MjdFrame {
  long scan_off, scan_len;
  int ri, mode, nseg;
  long nmcu;
  bool ok;
};

__device__ inline MjdFrame mjd_frame(const long* __restrict__ desc, int f, int H, int W, long data_bytes) {
  const long* d = desc + (long)f * MJD_DESC;
  MjdFrame fr;
  fr.scan_off = d[0];
  fr.scan_len = d[1];
  const long ri = d[2];
  const long mode = d[3];
  fr.ok = fr.scan_off >= 0 && fr.scan_len >= 0 && fr.scan_len <= 0x7fffffffL && fr.scan_off <= data_bytes &&
          fr.scan_len <= data_bytes - fr.scan_off && ri >= 0 && ri <= 65535 && mode >= 0 && mode <= 3;
  fr.mode = fr.ok ? (int)mode : 0;
  const MjdLayout g = mjd_layout(fr.mode, H, W);
  fr.nmcu = (long)g.mcux * g.mcuy;
  fr.ri = fr.ok && ri > 0 && ri < fr.nmcu ? (int)ri : (int)fr.nmcu;  // Ri = 0 or >= MCUs: one segment
  fr.nseg = (int)((fr.nmcu + fr.ri - 1) / fr.ri);
  if (!fr.ok) fr.scan_len = 0;
  return fr;
}

__device__ __forceinline__ int wave_incl_scan_i(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// ---------------------------------------------------------------------- stage 1: markers
// segstart[f][k] = offset in the scan of the byte after the (k + 1)-th RSTm, k < nseg - 1.
__global__ void __launch_bounds__(256)
mjd_markers_kernel(const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ desc, int H, int W,
                   int* __restrict__ segstart, long seg_ld, int* __restrict__ status) {
  __shared__ int wsum[4];
  __shared__ int carry_s, bad_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int f = blockIdx.x;
  const MjdFrame fr = mjd_frame(desc, f, H, W, data_bytes);
  if (!fr.ok) {
    if (tid == 0) status[f] = MJD_ST_DESC;
    return;
  }
  if (tid == 0) {
    carry_s = 0;
    bad_s = 0;
  }
  __syncthreads();
  const uint8_t* p = data + fr.scan_off;
  const long len = fr.scan_len;
  int* out = segstart + (long)f * seg_ld;
  const int want = fr.nseg - 1;
  for (long base = 0; base < len; base += MJD_TILE) {
    // 8 bytes per thread plus the first byte of the next thread's run
    const long i0 = base + (long)tid * 8;
    uint8_t b[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) b[j] = i0 + j < len ? p[i0 + j] : 0;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) cnt += b[j] == 0xff && (b[j + 1] & 0xf8) == 0xd0;
    const int incl = wave_incl_scan_i(cnt, lane);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int k = carry_s + incl - cnt;
    for (int w = 0; w < wv; ++w) k += wsum[w];
    if (cnt) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (b[j] == 0xff && (b[j + 1] & 0xf8) == 0xd0) {
          if (k < want) out[k] = (int)(i0 + j + 2);
          if (k >= want || (b[j + 1] & 7) != (k & 7)) bad_s = 1;  // benign race: every writer stores 1
          ++k;
        }
      }
    }
    __syncthreads();
    if (tid == 255) carry_s = k;
    __syncthreads();
  }
  if (tid == 0 && (bad_s || carry_s != want)) status[f] = MJD_ST_MARKERS;
}

// ---------------------------------------------------------------------- stage 2: entropy
// MSB-first bit reader of one lane over [pos, end) of the scan.  0xFF 0x00 is the data byte
// 0xFF; an 0xFF followed by anything else (a marker, a fill byte, the end) ends the data.
// Past the end the reader supplies zero bits and counts them in `fake`; the zero bits are
// always the tail of `acc`, so n < fake means real bits ran out.
struct MjdBits {
  const uint8_t* p;
  long pos, end;
  uint64_t acc;
  int n, fake;
  __device__ __forceinline__ void fill() {  // -> n >= 57
    while (n <= 56) {
      uint32_t b = 0;
      if (pos < end) {
        b = p[pos++];
        if (b == 0xff) {
          if (pos < end && p[pos] == 0) {
            ++pos;
          } else {
            pos = end;
            b = 0;
            fake += 8;
          }
        }
      } else {
        fake += 8;
      }
      acc |= (uint64_t)b << (56 - n);
      n += 8;
    }
  }
  __device__ __forceinline__ uint32_t peek(int k) const { return (uint32_t)(acc >> (64 - k)); }  // 1 <= k <= 32
  __device__ __forceinline__ void skip(int k) {
    acc <<= k;
    n -= k;
  }
  __device__ __forceinline__ bool short_of_bits() const { return n < fake; }
};

// jdhuff.c: one Huffman symbol, at most 16 bits; -1 for a code longer than 16 bits.  Needs n >= 16.
__device__ __forceinline__ int mjd_symbol(MjdBits& br, const int* __restrict__ t) {
  const uint32_t lk = ((const uint16_t*)(t + MJD_HT_LOOK))[br.peek(8)];
  if (lk) {
    br.skip((int)(lk >> 8));
    return (int)(lk & 0xff);
  }
  int l = 9;
  int code = (int)br.peek(9);
  while (l <= 16 && code > t[MJD_HT_MAXCODE + l]) {
    ++l;
    code = (int)br.peek(l);
  }
  if (l > 16) return -1;
  br.skip(l);
  return ((const uint8_t*)(t + MJD_HT_VAL))[(code + t[MJD_HT_VALOFF + l]) & 0xff];
}

// s magnitude bits, 1 <= s <= 15 -> the signed value (T.81 F.2.2.1 EXTEND)
__device__ __forceinline__ int mjd_receive_extend(MjdBits& br, int s) {
  const int v = (int)br.peek(s);
  br.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block: DC difference + run-length AC into coef[64] (natural order).  0 or a status.
__device__ __forceinline__ int mjd_block(MjdBits& br, const int* __restrict__ dct, const int* __restrict__ act, int& pred,
                                         int16_t* __restrict__ coef) {
  br.fill();
  int s = mjd_symbol(br, dct);
  if (s < 0 || s > 15) return MJD_ST_CODE;
  if (s) pred += mjd_receive_extend(br, s);
  if (pred) coef[0] = (int16_t)pred;
  for (int k = 1; k < 64; ++k) {  // k grows by at least 1: at most 63 symbols
    br.fill();
    const int rs = mjd_symbol(br, act);
    if (rs < 0) return MJD_ST_CODE;
    const int r = rs >> 4;
    s = rs & 15;
    if (s) {
      k += r;
      if (k > 63) return MJD_ST_INDEX;
      coef[MJD_NAT_OF[k]] = (int16_t)mjd_receive_extend(br, s);
    } else {
      if (r != 15) break;  // EOB
      k += 15;             // ZRL
    }
  }
  return br.short_of_bits() ? MJD_ST_SHORT : 0;
}

__global__ void __launch_bounds__(64)
mjd_entropy_kernel(const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ desc, int H, int W,
                   const int* __restrict__ huff, int n_huff, const int* __restrict__ segstart, long seg_ld,
                   int16_t* __restrict__ coef, long coef_ld, int* __restrict__ status) {
  __shared__ int tab[6][MJD_HT_INTS];  // [c] DC of component c, [3 + c] AC
  const int lane = threadIdx.x;
  const int f = blockIdx.y;
  if (status[f] != 0) return;  // stage 1 refused the frame (uniform: read before any lane of this launch writes)
  const MjdFrame fr = mjd_frame(desc, f, H, W, data_bytes);
  const MjdLayout g = mjd_layout(fr.mode, H, W);
  const long* d = desc + (long)f * MJD_DESC;
  for (int c = 0; c < g.ncomp; ++c) {
    const int di = (int)((d[5] >> (16 * c)) & 0xffff) % n_huff, ai = (int)((d[6] >> (16 * c)) & 0xffff) % n_huff;
    for (int i = lane; i < MJD_HT_INTS; i += 64) {
      tab[c][i] = huff[(long)di * MJD_HT_INTS + i];
      tab[3 + c][i] = huff[(long)ai * MJD_HT_INTS + i];
    }
  }
  __syncthreads();
  const uint8_t* p = data + fr.scan_off;
  const int* ss = segstart + (long)f * seg_ld;
  int16_t* cf = coef + (long)f * coef_ld;
  const int stride = gridDim.x * 64;
  for (int k = blockIdx.x * 64 + lane; k < fr.nseg; k += stride) {
    long begin = k ? ss[k - 1] : 0;
    long end = k < fr.nseg - 1 ? (long)ss[k] - 2 : fr.scan_len;
    // stage 1 wrote increasing in-range offsets; clamp all the same
    end = end < 0 ? 0 : (end > fr.scan_len ? fr.scan_len : end);
    begin = begin < 0 ? 0 : (begin > end ? end : begin);
    MjdBits br{p, begin, end, 0, 0, 0};
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const long m0 = (long)k * fr.ri, m1 = m0 + fr.ri < fr.nmcu ? m0 + fr.ri : fr.nmcu;
    int st = 0;
    for (long m = m0; m < m1 && !st; ++m) {
      const int my = (int)(m / g.mcux), mx = (int)(m - (long)my * g.mcux);
      for (int c = 0; c < g.ncomp && !st; ++c) {
        const int nh = c ? 1 : g.hs, nv = c ? 1 : g.vs;
        for (int b = 0; b < nh * nv && !st; ++b) {
          const int by = my * nv + b / nh, bx = mx * nh + b % nh;
          int16_t* blk = cf + (g.offc(c) + (long)by * g.bwc(c) + bx) * 64;
          st = mjd_block(br, tab[c], tab[3 + c], c == 0 ? pred0 : (c == 1 ? pred1 : pred2), blk);
        }
      }
    }
    if (st) {
      atomicMax(&status[f], st);
      break;  // the lane stops for this frame
    }
  }
}

// ---------------------------------------------------------------------- stage 3: IDCT
// jidctint.c: CONST_BITS 13, PASS1_BITS 2
constexpr int I_0_298 = 2446, I_0_390 = 3196, I_0_541 = 4433, I_0_765 = 6270, I_0_899 = 7373, I_1_175 = 9633,
              I_1_501 = 12299, I_1_847 = 15137, I_1_961 = 16069, I_2_053 = 16819, I_2_562 = 20995, I_3_072 = 25172;

// One 8-point pass of jpeg_idct_islow: SH = 11 for the column pass, 18 for the row pass.
template <int SH>
__device__ __forceinline__ void idct8(const int* d, int* o) {
  int z2 = d[2], z3 = d[6];
  int z1 = (z2 + z3) * I_0_541;
  int tmp2 = z1 - z3 * I_1_847;
  int tmp3 = z1 + z2 * I_0_765;
  int tmp0 = (d[0] + d[4]) << 13;
  int tmp1 = (d[0] - d[4]) << 13;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d[7];
  tmp1 = d[5];
  tmp2 = d[3];
  tmp3 = d[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * I_1_175;
  tmp0 *= I_0_298;
  tmp1 *= I_2_053;
  tmp2 *= I_3_072;
  tmp3 *= I_1_501;
  z1 *= -I_0_899;
  z2 *= -I_2_562;
  z3 = z3 * -I_1_961 + z5;
  z4 = z4 * -I_0_390 + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  constexpr int R = 1 << (SH - 1);
  o[0] = (tmp10 + tmp3 + R) >> SH;
  o[7] = (tmp10 - tmp3 + R) >> SH;
  o[1] = (tmp11 + tmp2 + R) >> SH;
  o[6] = (tmp11 - tmp2 + R) >> SH;
  o[2] = (tmp12 + tmp1 + R) >> SH;
  o[5] = (tmp12 - tmp1 + R) >> SH;
  o[3] = (tmp13 + tmp0 + R) >> SH;
  o[4] = (tmp13 - tmp0 + R) >> SH;
}

__global__ void __launch_bounds__(256)
mjd_idct_kernel(const long* __restrict__ desc, int H, int W, const uint16_t* __restrict__ quant, int n_quant,
                const int16_t* __restrict__ coef, long coef_ld, uint8_t* __restrict__ planes, long plane_ld) {
  __shared__ int ws[32][8][9];
  const int tid = threadIdx.x, g8 = tid >> 3, l = tid & 7;
  const int f = blockIdx.y;
  const long* d = desc + (long)f * MJD_DESC;
  const long mode_l = d[3];
  const MjdLayout g = mjd_layout(mode_l >= 0 && mode_l <= 3 ? (int)mode_l : 0, H, W);
  const long blk = (long)blockIdx.x * 32 + g8;
  const bool active = blk < g.nblocks;  // the grid covers the 4:4:4 count; uniform per 8-thread group
  int c = 0;
  if (active) c = blk >= g.off[1] ? (blk >= g.off[2] && g.ncomp == 3 ? 2 : 1) : 0;
  if (active) {
    const int qi = (int)((d[4] >> (16 * c)) & 0xffff) % n_quant;
    const int16_t* src = coef + (long)f * coef_ld + blk * 64;
    const uint16_t* q = quant + (long)qi * 64;
    int v[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (int)src[k * 8 + l] * (int)q[k * 8 + l];  // column l
    idct8<11>(v, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) ws[g8][k][l] = o[k];
  }
  __syncthreads();
  if (active) {
    int v[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = ws[g8][l][k];  // row l
    idct8<18>(v, o);
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int s = o[k] + 128;
      s = s < 0 ? 0 : (s > 255 ? 255 : s);
      w[k >> 2] |= (uint32_t)s << (8 * (k & 3));
    }
    const long b = blk - g.offc(c);
    const int bwc = g.bwc(c);
    const int by = (int)(b / bwc), bx = (int)(b - (long)by * bwc);
    // plane c starts at 64 * off[c]; its rows are 8 * bw[c] bytes: the store is 8-byte aligned
    uint8_t* dst = planes + (long)f * plane_ld + g.offc(c) * 64 + ((long)by * 8 + l) * ((long)bwc * 8) + bx * 8;
    *(uint2*)dst = make_uint2(w[0], w[1]);
  }
}

// ---------------------------------------------------------------------- stage 4: colour
__global__ void __launch_bounds__(256)
mjd_colour_kernel(const long* __restrict__ desc, int H, int W, const uint8_t* __restrict__ planes, long plane_ld,
                  uint8_t* __restrict__ out) {
  __shared__ uint32_t stage[256 * 3 / 4 + 2];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * 256, y = blockIdx.y, f = blockIdx.z;
  const long* d = desc + (long)f * MJD_DESC;
  const long mode_l = d[3];
  const int mode = mode_l >= 0 && mode_l <= 3 ? (int)mode_l : 0;
  const MjdLayout g = mjd_layout(mode, H, W);
  const int wvalid = min(256, W - x0);  // >= 1
  uint8_t* row = out + (((long)f * H + y) * W + x0) * 3;
  const int mis = (int)((uintptr_t)row & 3);
  const int x = x0 + tid;
  if (tid < wvalid) {
    const uint8_t* pl = planes + (long)f * plane_ld;
    const long ldy = (long)g.bw[0] * 8;
    const int yy = pl[(long)y * ldy + x];
    int R = yy, G = yy, B = yy;
    if (mode != 0) {
      const long ldc = (long)g.bw[1] * 8;
      const uint8_t* p1 = pl + g.off[1] * 64;
      const uint8_t* p2 = pl + g.off[2] * 64;
      int cb, cr;
      if (mode == 1) {
        cb = p1[(long)y * ldc + x];
        cr = p2[(long)y * ldc + x];
      } else {
        const int dw = (W + 1) >> 1, c = x >> 1;
        const bool odd = x & 1;
        const int cn = odd ? c + 1 : c - 1;            // the horizontal neighbour
        const bool edge = odd ? c == dw - 1 : c == 0;  // the plane's first / last real column
        if (dw <= 2) {  // jdsample.c uses the fancy filters only for planes wider than 2: replicate
          const long o = (long)(mode == 3 ? y >> 1 : y) * ldc + c;
          cb = p1[o];
          cr = p2[o];
        } else if (mode == 2) {  // h2v1 fancy: 3/4 nearer + 1/4 further, the two end samples copied
          const uint8_t* a = p1 + (long)y * ldc;
          const uint8_t* b = p2 + (long)y * ldc;
          const int rnd = odd ? 2 : 1;
          cb = edge ? a[c] : (3 * a[c] + a[cn] + rnd) >> 2;
          cr = edge ? b[c] : (3 * b[c] + b[cn] + rnd) >> 2;
        } else {  // h2v2 fancy: 3/4 nearer + 1/4 further row, then the same across
          const int dh = (H + 1) >> 1, r = y >> 1;
          int rn = (y & 1) ? r + 1 : r - 1;
          if (rn < 0 || rn > dh - 1) rn = r;
          const uint8_t* a0 = p1 + (long)r * ldc;
          const uint8_t* a1 = p1 + (long)rn * ldc;
          const uint8_t* b0 = p2 + (long)r * ldc;
          const uint8_t* b1 = p2 + (long)rn * ldc;
          const int rnd = odd ? 7 : 8;
          const int sa = 3 * a0[c] + a1[c], sb = 3 * b0[c] + b1[c];
          if (edge) {
            cb = (4 * sa + rnd) >> 4;
            cr = (4 * sb + rnd) >> 4;
          } else {
            cb = (3 * sa + 3 * a0[cn] + a1[cn] + rnd) >> 4;
            cr = (3 * sb + 3 * b0[cn] + b1[cn] + rnd) >> 4;
          }
        }
      }
      cb -= 128;
      cr -= 128;
      R = yy + ((91881 * cr + 32768) >> 16);
      G = yy + ((-22554 * cb - 46802 * cr + 32768) >> 16);
      B = yy + ((116130 * cb + 32768) >> 16);
      R = R < 0 ? 0 : (R > 255 ? 255 : R);
      G = G < 0 ? 0 : (G > 255 ? 255 : G);
      B = B < 0 ? 0 : (B > 255 ? 255 : B);
    }
    uint8_t* s = (uint8_t*)stage + mis + 3 * tid;
    s[0] = (uint8_t)R;
    s[1] = (uint8_t)G;
    s[2] = (uint8_t)B;
  }
  __syncthreads();
  // the staged bytes [mis, mis + 3 * wvalid) leave as the aligned dwords that hold them; a
  // dword that is only partly inside the row segment is written byte by byte
  const int nbytes = 3 * wvalid, ndw = (mis + nbytes + 3) >> 2;
  if (tid < ndw) {
    uint8_t* base = row - mis + 4 * tid;
    const int lo = 4 * tid, hi = lo + 4;
    if (lo >= mis && hi <= mis + nbytes) {
      *(uint32_t*)base = stage[tid];
    } else {
      const uint8_t* s = (const uint8_t*)stage + lo;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (lo + j >= mis && lo + j < mis + nbytes) base[j] = s[j];
    }
  }
}

struct MjdGeom {
  int batch;
  long blocks;                         // 8x8 blocks of a 4:4:4 frame: the most any mode needs
  size_t coef_b, plane_b, seg_b, per;  // per frame, each a multiple of 256
};

static bool mjd_geom(int n, int H, int W, MjdGeom* g) {
  if (n < 1 || H < 3 || W < 3 || H > 65535 || W > 65535) return false;
  // every mode's planes fit 3 planes padded to 16 x 16 (4:2:0 pads luma to 16, 4:4:4 has 3 full planes)
  const long bw = (long)((W + 15) / 16) * 2, bh = (long)((H + 15) / 16) * 2;
  g->blocks = 3 * bw * bh;
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  g->coef_b = up((size_t)g->blocks * 64 * 2);
  g->plane_b = up((size_t)g->blocks * 64);
  g->seg_b = up((size_t)(bw * bh + 1) * 4);  // at most one segment per MCU, at most bw * bh MCUs
  g->per = g->coef_b + g->plane_b + g->seg_b;
  size_t b = MJD_WS_BUDGET / g->per;
  b = b < 1 ? 1 : b;
  b = b > (size_t)MJD_MAX_BATCH ? MJD_MAX_BATCH : b;
  g->batch = (int)(b > (size_t)n ? n : b);
  return true;
}

}  // namespace ls

using namespace ls;

extern "C" size_t ls_mjpeg_decode_workspace_bytes(int32_t n, int32_t H, int32_t W) {
  MjdGeom g;
  if (!mjd_geom(n, H, W, &g)) return 0;
  return (size_t)g.batch * g.per + 256;
}

extern "C" int ls_mjpeg_decode(const uint8_t* data, int64_t data_bytes, const int64_t* frames, int32_t n, int32_t H,
                               int32_t W, const uint16_t* quant, int32_t n_quant, const int32_t* huff, int32_t n_huff,
                               int32_t max_segments, uint8_t* out, int32_t* status, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if ((!data && data_bytes > 0) || !frames || !quant || !huff || !out || !status)
    return fail(LS_ERR_INVALID, "ls_mjpeg_decode: null pointer");
  if (data_bytes < 0 || n_quant < 1 || n_huff < 1 || n_quant > 65535 || n_huff > 65535)
    return fail(LS_ERR_INVALID, "ls_mjpeg_decode: need data_bytes >= 0 and 1..65535 quantiser and Huffman tables");
  MjdGeom g;
  if (!mjd_geom(n, H, W, &g)) return fail(LS_ERR_INVALID, "ls_mjpeg_decode: need n >= 1 and 3 <= H, W <= 65535");
  if (!workspace || workspace_bytes < ls_mjpeg_decode_workspace_bytes(n, H, W))
    return fail(LS_ERR_WORKSPACE, "ls_mjpeg_decode: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  int16_t* coef = (int16_t*)ws;
  uint8_t* planes = (uint8_t*)(ws + (size_t)g.batch * g.coef_b);
  int* segstart = (int*)((char*)planes + (size_t)g.batch * g.plane_b);
  const long coef_ld = (long)(g.coef_b / 2), plane_ld = (long)g.plane_b, seg_ld = (long)(g.seg_b / 4);
  int waves = max_segments < 1 ? 1 : (max_segments + 63) / 64;
  waves = waves > MJD_MAX_WAVES ? MJD_MAX_WAVES : waves;
  if (hipMemsetAsync(status, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess)
    return fail(LS_ERR_LAUNCH, "ls_mjpeg_decode: memset");
  const size_t frame_bytes = (size_t)H * W * 3;
  for (int f0 = 0; f0 < n; f0 += g.batch) {
    const int nf = std::min(g.batch, n - f0);
    const long* desc = (const long*)frames + (size_t)f0 * MJD_DESC;
    if (hipMemsetAsync(coef, 0, (size_t)nf * g.coef_b, s) != hipSuccess)
      return fail(LS_ERR_LAUNCH, "ls_mjpeg_decode: memset");
    mjd_markers_kernel<<<nf, 256, 0, s>>>(data, (long)data_bytes, desc, H, W, segstart, seg_ld, status + f0);
    if (int rc = check_launch("mjd_markers_kernel")) return rc;
    mjd_entropy_kernel<<<dim3(waves, nf), 64, 0, s>>>(data, (long)data_bytes, desc, H, W, huff, n_huff, segstart,
                                                       seg_ld, coef, coef_ld, status + f0);
    if (int rc = check_launch("mjd_entropy_kernel")) return rc;
    mjd_idct_kernel<<<dim3((unsigned)((g.blocks + 31) / 32), nf), 256, 0, s>>>(desc, H, W, quant, n_quant, coef,
                                                                                coef_ld, planes, plane_ld);
    if (int rc = check_launch("mjd_idct_kernel")) return rc;
    mjd_colour_kernel<<<dim3((W + 255) / 256, H, nf), 256, 0, s>>>(desc, H, W, planes, plane_ld,
                                                                   out + (size_t)f0 * frame_bytes);
    if (int rc = check_launch("mjd_colour_kernel")) return rc;
  }
  return LS_OK;
}
