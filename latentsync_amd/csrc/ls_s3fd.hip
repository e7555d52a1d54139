// The S3FD face detector of the reference's sync gate (eval/detectors/s3fd: S3FD.detect_faces,
// S3FDNet, Detect, nms_) on gfx950: what it needs beyond ls_conv_general and ls_maxpool2d.
//
//  * s3fd_prep_kernel: detect_faces' cv2.resize(image, (0, 0), fx = s, fy = s, INTER_LINEAR) for
//    uint8 and the mean subtraction.  The destination is cvRound(W s) x cvRound(H s) (round half
//    to even) and the source step is 1 / s on both axes -- not the ratio of the sizes, which is
//    what cv2 uses when a dsize is given (ls_crop_track).  Coefficients and the two rounding
//    passes are crop_track_kernel's (ls_synceval.hip).  The two [2, 1, 0] swaps cancel: the
//    network sees R - 123, G - 117, B - 104, integers below 256 in magnitude, exact in bf16.
//    cv2 switches to the 2 x 2 area mean at exactly s = 0.5; that path is not restated here and
//    the entry point refuses s = 0.5.
//  * conv3x3_relu_kernel: the VGG trunk's conv, 3 x 3, stride 1, padding = dilation (1 or 6), on
//    v_mfma_f32_16x16x32_bf16.  A block of 4 waves owns 128 consecutive pixels (of the n_img H W
//    pixels, images back to back) x 64 output channels; a wave owns 32 pixels x 64 channels = 8
//    accumulator tiles.  Per (tap, 64-channel chunk) the block stages the 64 x 64 weight tile in
//    LDS (8 KiB, two buffers, swz64 image: the 16-lane groups of a ds_read_b128 fragment read
//    hit distinct bank slots), so a weight byte fetched from L2 serves 128 pixels, against 16 in
//    conv_general_kernel; the pixel operand is gathered from memory in MFMA fragment order (lane
//    (r, g) holds channels 8 g .. 8 g + 7 of its k-step for pixel r), one 16-byte load, and a
//    tap in the padding is a zero register, never a load.  The operands of step s + 1 are
//    fetched into registers while step s runs on the MFMAs; one barrier per step.  The block
//    first ORs the live taps of its pixels: a tap that is padding for all 128 is skipped with
//    its weights (at dilation 6 on a map of at most 6 x 6 that leaves the centre tap alone).
//    Skipping adds no rounding (a zero operand adds +0), and a pixel's sum runs over taps and
//    chunks in one fixed order, so a frame's result does not depend on what it is batched with.
//    One form for every (Cin, N, dilation).
//  * maxpool2x2_ceil_kernel: MaxPool2d(2, 2, ceil_mode = True), the last window clipped.  Exact.
//  * l2norm_scale_kernel: L2Norm.forward per pixel in fp32, x / (sqrt(sum x^2) + 1e-10) w[c].
//  * s3fd_detect_kernel: the tail of S3FDNet.forward and Detect.forward, one frame per block:
//    max-out background label at level 0, two-class softmax, decode() with variances (0.1,
//    0.2) in the reference's operation order, the candidates above 0.05 sorted by descending
//    score (bitonic on 64-bit keys score | ~index in the workspace), the 5000 highest, greedy
//    NMS at IoU <= 0.3, the first 750 kept.
//  * nms_boxes_kernel: the rest of detect_faces: the rows above conf_th scaled to the frame,
//    nms_ in fp32 (the reference runs it in float64 on the same fp32 values).
#include "ls_common.h"

namespace ls {

// --------------------------------------------------------------------------------- prep
// cv2's linear coefficients of destination index d (crop_track_kernel's ct_coef)
__device__ __forceinline__ void s3_coef(int d, double scale, int size, bool horizontal, int* s, int* w0, int* w1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int i = (int)floorf(f);
  f -= (float)i;
  if (horizontal) {
    if (i < 0) f = 0.f, i = 0;
    if (i >= size - 1) f = 0.f, i = size - 1;
  }
  *s = i;
  *w0 = (int)rintf((1.0f - f) * 2048.0f);
  *w1 = (int)rintf(f * 2048.0f);
}

__global__ void __launch_bounds__(256)
s3fd_prep_kernel(const uint8_t* __restrict__ frames, int n, int H, int W, double scale, int h, int w,
                 u16* __restrict__ out) {
  const long total = (long)n * h * w;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int dx = (int)(i % w);
    const long q = i / w;
    const int dy = (int)(q % h), fi = (int)(q / h);
    const uint8_t* f = frames + (long)fi * H * W * 3;
    int sx, a0, ax, sy, b0, by;
    s3_coef(dx, scale, W, true, &sx, &a0, &ax);
    s3_coef(dy, scale, H, false, &sy, &b0, &by);
    const int xa = sx, xb = min(sx + 1, W - 1);
    const int ya = min(max(sy, 0), H - 1), yb = min(max(sy + 1, 0), H - 1);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float mean[3] = {123.f, 117.f, 104.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int r0 = (int)f[((long)ya * W + xa) * 3 + c] * a0 + (int)f[((long)ya * W + xb) * 3 + c] * ax;
      const int r1 = (int)f[((long)yb * W + xa) * 3 + c] * a0 + (int)f[((long)yb * W + xb) * 3 + c] * ax;
      const int p = (((b0 * (r0 >> 4)) >> 16) + ((by * (r1 >> 4)) >> 16) + 2) >> 2;
      v[c] = (float)min(max(p, 0), 255) - mean[c];
    }
    *(uint4*)(out + i * 8) = pack8(v);
  }
}

// ------------------------------------------------------------------------- 3 x 3 trunk conv
constexpr int C3_BM = 128, C3_BN = 64;

struct conv3_args {
  const u16* x;
  const u16* w;
  const float* bias;
  u16* y;
  long M;
  int ldx, ldy, H, W, Cin, N, dil;
};

__device__ __forceinline__ void c3_pixel(long p, int hw, int W, long& pix, int& y, int& x) {
  const long img = p / hw;
  const int rem = (int)(p - img * hw);
  y = rem / W;
  x = rem - y * W;
  pix = img * hw;
}

// the taps of pixel (y, x) that fall inside the image, one bit per tap
__device__ __forceinline__ int c3_live(const conv3_args& a, int y, int x) {
  int mask = 0;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = y + (tap / 3 - 1) * a.dil, xx = x + (tap % 3 - 1) * a.dil;
    if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) mask |= 1 << tap;
  }
  return mask;
}

// channels c .. c + 7 and c + 32 .. c + 39 of input pixel (yy, xx) of the image at pixel offset
// pix: the lane's operand of the two k-steps of a 64-channel chunk; zeros in the padding
__device__ __forceinline__ void c3_gather(const conv3_args& a, long pix, int yy, int xx, bool pv, int c, uint4& lo,
                                          uint4& hi) {
  lo = hi = make_uint4(0u, 0u, 0u, 0u);
  if (pv && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
    const u16* xp = a.x + (pix + (long)yy * a.W + xx) * a.ldx + c;
    lo = *(const uint4*)xp;
    hi = *(const uint4*)(xp + 32);
  }
}

// the accumulator lane holds channels n + 16 j .. + 3 of pixel p
__device__ __forceinline__ void c3_store(const conv3_args& a, long p, int n, const f32x4 (&acc)[4]) {
  u16* yp = a.y + p * a.ldy;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[j][i] + (a.bias ? a.bias[n + j * 16 + i] : 0.f), 0.f);
    *(uint2*)(yp + n + j * 16) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
  }
}

__global__ void __launch_bounds__(256) conv3x3_relu_kernel(const conv3_args a) {
  __shared__ uint4 wl[2][C3_BN * 8];  // [buffer][swz64(row, 16-byte chunk)]
  __shared__ int live_mask;
  __shared__ int taps[9];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * C3_BN;
  const long m0 = (long)blockIdx.x * C3_BM;
  const int K = 9 * a.Cin;

  // this lane's two pixels (pixel r of each of the wave's two 16-pixel tiles)
  const int hw = a.H * a.W;
  long pix0, pix1;
  int py0, px0, py1, px1;
  const long p0 = m0 + wave * 32 + r, p1 = p0 + 16;
  const bool pv0 = p0 < a.M, pv1 = p1 < a.M;
  c3_pixel(pv0 ? p0 : 0, hw, a.W, pix0, py0, px0);
  c3_pixel(pv1 ? p1 : 0, hw, a.W, pix1, py1, px1);
  const int mask = (pv0 ? c3_live(a, py0, px0) : 0) | (pv1 ? c3_live(a, py1, px1) : 0);
  if (tid == 0) live_mask = 0;
  __syncthreads();
  if (mask) atomicOr(&live_mask, mask);
  __syncthreads();
  const int bm = live_mask;  // never 0: the centre tap of a valid pixel is live
  if (tid == 0) {
    int c = 0;
    for (int tap = 0; tap < 9; ++tap)
      if (bm >> tap & 1) taps[c++] = tap;
  }
  __syncthreads();
  const int ntaps = __builtin_popcount(bm);
  const int nch = a.Cin / 64;
  const int nsteps = ntaps * nch;

  // weight staging: thread -> rows wr, wr + 32 of the 64 x 64 tile, 16-byte chunk wc
  const int wr = tid >> 3, wc = tid & 7;
  const u16* wbase = a.w + (long)(n0 + wr) * K + wc * 8;

  uint4 wreg0, wreg1, b00, b01, b10, b11;  // scalars, not arrays: nothing here may be indexed through memory
#define C3_FETCH(s_)                                                                             \
  do {                                                                                           \
    const int tap_ = taps[(s_) / nch], c0_ = ((s_) % nch) * 64;                                  \
    const u16* wp_ = wbase + (long)tap_ * a.Cin + c0_;                                           \
    wreg0 = *(const uint4*)wp_;                                                                  \
    wreg1 = *(const uint4*)(wp_ + (long)32 * K);                                                 \
    const int dy_ = (tap_ / 3 - 1) * a.dil, dx_ = (tap_ % 3 - 1) * a.dil;                        \
    c3_gather(a, pix0, py0 + dy_, px0 + dx_, pv0, c0_ + g * 8, b00, b01);                        \
    c3_gather(a, pix1, py1 + dy_, px1 + dx_, pv1, c0_ + g * 8, b10, b11);                        \
  } while (0)
#define C3_STAGE(buf_)                           \
  do {                                           \
    wl[buf_][swz64(wr, wc)] = wreg0;             \
    wl[buf_][swz64(wr + 32, wc)] = wreg1;        \
  } while (0)

  f32x4 acc0[4], acc1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc0[j] = acc1[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  C3_FETCH(0);
  C3_STAGE(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const bf16x8 f00 = __builtin_bit_cast(bf16x8, b00), f01 = __builtin_bit_cast(bf16x8, b01);
    const bf16x8 f10 = __builtin_bit_cast(bf16x8, b10), f11 = __builtin_bit_cast(bf16x8, b11);
    const bool more = s + 1 < nsteps;
    if (more) C3_FETCH(s + 1);
    const uint4* cur = wl[s & 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8 af = __builtin_bit_cast(bf16x8, cur[swz64(j * 16 + r, g)]);
      acc0[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, f00, acc0[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, f10, acc1[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8 af = __builtin_bit_cast(bf16x8, cur[swz64(j * 16 + r, 4 + g)]);
      acc0[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, f01, acc0[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, f11, acc1[j], 0, 0, 0);
    }
    if (more) C3_STAGE((s + 1) & 1);  // last read in step s - 1, before the barrier that ended it
    __syncthreads();
  }
#undef C3_FETCH
#undef C3_STAGE

  if (pv0) c3_store(a, p0, n0 + g * 4, acc0);
  if (pv1) c3_store(a, p1, n0 + g * 4, acc1);
}

// --------------------------------------------------------------------- ceil-mode 2 x 2 pool
__global__ void __launch_bounds__(256)
maxpool2x2_ceil_kernel(const u16* __restrict__ x, int ldx, long n_img, int H, int W, int C8, int Ho, int Wo,
                       u16* __restrict__ y, int ldy) {
  const long total = n_img * Ho * Wo * C8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % C8);
    const long p = i / C8;
    const int ox = (int)(p % Wo);
    const long q = p / Wo;
    const int oy = (int)(q % Ho);
    const long img = q / Ho;
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
    for (int dy = 0; dy < 2; ++dy) {
      const int yy = oy * 2 + dy;
      if (yy >= H) continue;  // the clipped last window
      for (int dx = 0; dx < 2; ++dx) {
        const int xx = ox * 2 + dx;
        if (xx >= W) continue;
        float v[8];
        unpack8(*(const uint4*)(x + ((img * H + yy) * W + xx) * ldx + c8 * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = (v[j] > m[j] || v[j] != v[j]) ? v[j] : m[j];  // a NaN wins, as in torch
      }
    }
    *(uint4*)(y + p * ldy + c8 * 8) = pack8(m);
  }
}

// ----------------------------------------------------------------------------------- L2Norm
__global__ void __launch_bounds__(256)
l2norm_scale_kernel(const u16* __restrict__ x, int ldx, long M, int C8, const float* __restrict__ weight,
                    u16* __restrict__ y, int ldy) {
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= M) return;
  const u16* xp = x + p * ldx;
  float s = 0.f;
  for (int c = lane; c < C8; c += 64) {
    float v[8];
    unpack8(*(const uint4*)(xp + c * 8), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) s = fmaf(v[j], v[j], s);
  }
  s = wave_sum(s);
  const float norm = sqrtf(s) + 1e-10f;
  for (int c = lane; c < C8; c += 64) {
    float v[8], wv[8];
    unpack8(*(const uint4*)(xp + c * 8), v);
    load8f(weight + c * 8, wv);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] / norm * wv[j];
    *(uint4*)(y + p * ldy + c * 8) = pack8(v);
  }
}

// ------------------------------------------------------------------- SSD post-processing
constexpr int DET_TOPK = 750, DET_NMS_TOPK = 5000, DET_MAX_P = 65536, DET_THREADS = 1024;
constexpr float DET_CONF = 0.05f, DET_NMS = 0.3f, DET_VAR0 = 0.1f, DET_VAR1 = 0.2f;

struct det_args {
  const float* map[6];
  int npix[6];  // pixels of each level's map, per frame
  const float* priors;
  float* out;        // [n][750][5]
  int* counts;       // [n]
  int* keep_idx;     // [n][750] or NULL
  unsigned long long* keys;  // [n][P2]
  float4* boxes;     // [n][P]
  float4* sbox;      // [n][5000]
  int P, P2;
};

// IoU in Detect's nms(): the reference's operation order, no contraction into fma
__device__ __forceinline__ float det_area(const float4 b) { return __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y)); }

__device__ __forceinline__ float det_iou(const float4 bi, const float4 bj) {
  const float w = fmaxf(__fsub_rn(fminf(bj.z, bi.z), fmaxf(bj.x, bi.x)), 0.f);
  const float h = fmaxf(__fsub_rn(fminf(bj.w, bi.w), fmaxf(bj.y, bi.y)), 0.f);
  const float inter = __fmul_rn(w, h);
  const float uni = __fadd_rn(__fsub_rn(det_area(bj), inter), det_area(bi));  // (rem_areas - inter) + area[i]
  return __fdiv_rn(inter, uni);
}

__global__ void __launch_bounds__(DET_THREADS) s3fd_detect_kernel(const det_args a) {
  __shared__ int cnt_s;
  __shared__ unsigned char alive[DET_NMS_TOPK];
  const int f = blockIdx.x, tid = threadIdx.x;
  unsigned long long* keys = a.keys + (long)f * a.P2;
  float4* boxes = a.boxes + (long)f * a.P;
  float4* sbox = a.sbox + (long)f * DET_NMS_TOPK;
  float* out = a.out + (long)f * DET_TOPK * 5;
  if (tid == 0) cnt_s = 0;
  for (int i = tid; i < DET_TOPK * 5; i += DET_THREADS) out[i] = 0.f;
  if (a.keep_idx)
    for (int i = tid; i < DET_TOPK; i += DET_THREADS) a.keep_idx[(long)f * DET_TOPK + i] = -1;
  __syncthreads();

  // softmax, decode, candidates
  for (int i = tid; i < a.P; i += DET_THREADS) {
    int lvl = 0, q = i;
    while (lvl < 5 && q >= a.npix[lvl]) q -= a.npix[lvl], ++lvl;
    const int ch = lvl == 0 ? 8 : 6;
    const float* m = a.map[lvl] + ((long)f * a.npix[lvl] + q) * ch;
    const float bg = lvl == 0 ? fmaxf(fmaxf(m[4], m[5]), m[6]) : m[4];
    const float fc = lvl == 0 ? m[7] : m[5];
    const float mx = fmaxf(bg, fc);
    const float e0 = expf(__fsub_rn(bg, mx)), e1 = expf(__fsub_rn(fc, mx));
    const float score = __fdiv_rn(e1, __fadd_rn(e0, e1));
    const float4 pr = *(const float4*)(a.priors + (long)i * 4);
    // decode(): priors[:, :2] + loc[:, :2] * 0.1 * priors[:, 2:]; priors[:, 2:] * exp(loc[:, 2:] * 0.2)
    const float cx = __fadd_rn(pr.x, __fmul_rn(__fmul_rn(m[0], DET_VAR0), pr.z));
    const float cy = __fadd_rn(pr.y, __fmul_rn(__fmul_rn(m[1], DET_VAR0), pr.w));
    const float bw = __fmul_rn(pr.z, expf(__fmul_rn(m[2], DET_VAR1)));
    const float bh = __fmul_rn(pr.w, expf(__fmul_rn(m[3], DET_VAR1)));
    const float x1 = __fsub_rn(cx, __fdiv_rn(bw, 2.f)), y1 = __fsub_rn(cy, __fdiv_rn(bh, 2.f));
    boxes[i] = make_float4(x1, y1, __fadd_rn(bw, x1), __fadd_rn(bh, y1));
    if (score > DET_CONF) {
      const int slot = atomicAdd(&cnt_s, 1);  // the slot order is arbitrary, the keys are unique: the sort is not
      keys[slot] = ((unsigned long long)__float_as_uint(score) << 32) | (unsigned)(~i);
    }
  }
  __syncthreads();
  const int cnt = cnt_s;
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;
  for (int i = cnt + tid; i < n2; i += DET_THREADS) keys[i] = 0ull;
  __syncthreads();
  // bitonic sort, descending (a score ties towards the lower prior index)
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += DET_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long x = keys[i], y = keys[l];
          if (((i & k) == 0) ? (x < y) : (x > y)) keys[i] = y, keys[l] = x;
        }
      }
      __syncthreads();
    }
  }
  const int m = min(cnt, DET_NMS_TOPK);  // idx[-top_k:]: exactly the 5000 highest
  for (int i = tid; i < m; i += DET_THREADS) {
    sbox[i] = boxes[~(unsigned)keys[i]];
    alive[i] = 1;
  }
  __syncthreads();
  int kept = 0, i = 0;
  while (true) {
    while (i < m && !alive[i]) ++i;  // uniform: every thread reads the same flags
    if (i >= m || kept >= DET_TOPK) break;
    const float4 bi = sbox[i];
    if (tid == 0) {
      const unsigned long long key = keys[i];
      float* o = out + kept * 5;
      o[0] = __uint_as_float((unsigned)(key >> 32)), o[1] = bi.x, o[2] = bi.y, o[3] = bi.z, o[4] = bi.w;
      if (a.keep_idx) a.keep_idx[(long)f * DET_TOPK + kept] = (int)~(unsigned)key;
    }
    ++kept;
    for (int j = i + 1 + tid; j < m; j += DET_THREADS)
      if (alive[j] && !(det_iou(bi, sbox[j]) <= DET_NMS)) alive[j] = 0;
    ++i;
    __syncthreads();
  }
  if (tid == 0) a.counts[f] = kept;
}

constexpr int NB_MAX_ROWS = 4096, NB_THREADS = 256;

// nms_ of box_utils.py: areas (x2 - x1) (y2 - y1), ovr = inter / (areas[i] + areas[j] - inter)
__device__ __forceinline__ float nb_iou(const float4 bi, const float4 bj) {
  const float w = fmaxf(0.f, __fsub_rn(fminf(bi.z, bj.z), fmaxf(bi.x, bj.x)));
  const float h = fmaxf(0.f, __fsub_rn(fminf(bi.w, bj.w), fmaxf(bi.y, bj.y)));
  const float inter = __fmul_rn(w, h);
  return __fdiv_rn(inter, __fsub_rn(__fadd_rn(det_area(bi), det_area(bj)), inter));
}

__global__ void __launch_bounds__(NB_THREADS)
nms_boxes_kernel(const float* __restrict__ det, int R, float conf_th, float fw, float fh, float thresh,
                 float* __restrict__ out, int* __restrict__ counts, int* __restrict__ keep_idx) {
  __shared__ unsigned short sel[NB_MAX_ROWS], order[NB_MAX_ROWS];
  __shared__ unsigned char alive[NB_MAX_ROWS];
  __shared__ int m_s;
  const int f = blockIdx.x, tid = threadIdx.x;
  const float* d = det + (long)f * R * 5;
  float* o = out + (long)f * R * 5;
  for (int i = tid; i < R * 5; i += NB_THREADS) o[i] = 0.f;
  if (keep_idx)
    for (int i = tid; i < R; i += NB_THREADS) keep_idx[(long)f * R + i] = -1;
  for (int i = tid; i < R; i += NB_THREADS) alive[i] = d[i * 5] > conf_th ? 1 : 0;
  __syncthreads();
  if (tid == 0) {  // the rows above conf_th, in row order
    int m = 0;
    for (int i = 0; i < R; ++i)
      if (alive[i]) sel[m++] = (unsigned short)i;
    m_s = m;
  }
  __syncthreads();
  const int m = m_s;
  auto box = [&](int s) {  // detections[0, i, j, 1:] * scale
    const float* r = d + (int)sel[s] * 5;
    return make_float4(__fmul_rn(r[1], fw), __fmul_rn(r[2], fh), __fmul_rn(r[3], fw), __fmul_rn(r[4], fh));
  };
  // descending score order by counting (equal scores: the later row first, argsort()[::-1] of a stable sort)
  for (int i = tid; i < m; i += NB_THREADS) {
    const float si = d[(int)sel[i] * 5];
    int rank = 0;
    for (int j = 0; j < m; ++j) {
      const float sj = d[(int)sel[j] * 5];
      rank += (sj > si || (sj == si && j > i)) ? 1 : 0;
    }
    order[rank] = (unsigned short)i;
    alive[i] = 1;
  }
  __syncthreads();
  int kept = 0, i = 0;
  while (true) {
    while (i < m && !alive[order[i]]) ++i;
    if (i >= m) break;
    const int si = order[i];
    const float4 bi = box(si);
    if (tid == 0) {
      float* r = o + kept * 5;
      r[0] = bi.x, r[1] = bi.y, r[2] = bi.z, r[3] = bi.w, r[4] = d[(int)sel[si] * 5];
      if (keep_idx) keep_idx[(long)f * R + kept] = si;
    }
    ++kept;
    for (int j = i + 1 + tid; j < m; j += NB_THREADS) {
      const int sj = order[j];
      if (alive[sj] && !(nb_iou(bi, box(sj)) <= thresh)) alive[sj] = 0;
    }
    ++i;
    __syncthreads();
  }
  if (tid == 0) counts[f] = kept;
}

static bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

static long pow2_ceil(long v) {
  long p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace ls

using namespace ls;

static long s3_round_half_even(double v) { return (long)nearbyint(v); }  // cvRound, default rounding mode

extern "C" int ls_s3fd_prep(const uint8_t* frames, int32_t n, int32_t H, int32_t W, double s, uint16_t* out,
                            void* stream) {
  if (!frames || !out) return fail(LS_ERR_INVALID, "ls_s3fd_prep: null pointer");
  if (n < 1 || H < 1 || W < 1 || H > 32768 || W > 32768)
    return fail(LS_ERR_INVALID, "ls_s3fd_prep: need n >= 1 and a frame size in 1..32768");
  if (!(s > 0.0) || !(s <= 1.0)) return fail(LS_ERR_INVALID, "ls_s3fd_prep: the scale must be in (0, 1]");
  if (s == 0.5)
    return fail(LS_ERR_INVALID, "ls_s3fd_prep: scale 0.5 is refused: cv2.resize takes its 2 x 2 area path there, "
                                "which this kernel does not restate");
  if (misaligned16(out)) return fail(LS_ERR_INVALID, "ls_s3fd_prep: out must be 16-byte aligned");
  const long h = s3_round_half_even((double)H * s), w = s3_round_half_even((double)W * s);
  if (h < 1 || w < 1) return fail(LS_ERR_INVALID, "ls_s3fd_prep: the scaled frame is empty");
  const long total = (long)n * h * w;
  s3fd_prep_kernel<<<(int)std::min<long>(cdiv(total, 256), 16384), 256, 0, (hipStream_t)stream>>>(
      frames, n, H, W, 1.0 / s, (int)h, (int)w, out);
  return check_launch("s3fd_prep_kernel");
}

extern "C" int ls_conv3x3_relu(const uint16_t* x, int32_t ldx, int32_t n_img, int32_t H, int32_t W, int32_t Cin,
                               const uint16_t* w, int32_t N, const float* bias, int32_t dilation, uint16_t* y,
                               int32_t ldy, void* stream) {
  if (!x || !w || !y) return fail(LS_ERR_INVALID, "ls_conv3x3_relu: null pointer");
  if (dilation != 1 && dilation != 6) return fail(LS_ERR_INVALID, "ls_conv3x3_relu: dilation must be 1 or 6");
  if (Cin < 64 || Cin > 1024 || Cin % 64 || N < 64 || N % 64 || N > 65535 * 64)
    return fail(LS_ERR_INVALID, "ls_conv3x3_relu: Cin must be a multiple of 64 in 64..1024 and N a multiple of 64");
  if (ldx % 8 || ldx < Cin || ldy % 8 || ldy < N)
    return fail(LS_ERR_INVALID, "ls_conv3x3_relu: ldx and ldy must be multiples of 8, ldx >= Cin, ldy >= N");
  if (n_img < 1 || H < 1 || W < 1) return fail(LS_ERR_INVALID, "ls_conv3x3_relu: need n_img, H, W >= 1");
  if (misaligned16(x) || misaligned16(w) || misaligned16(y) || (bias && ((uintptr_t)bias & 3)))
    return fail(LS_ERR_INVALID, "ls_conv3x3_relu: x, w and y must be 16-byte aligned");
  const long M = (long)n_img * H * W;
  if ((long)H * W > 0x7fffffffL / 2 || (M + C3_BM - 1) / C3_BM > 0x7fffffffL)
    return fail(LS_ERR_INVALID, "ls_conv3x3_relu: shape too large for one grid");
  conv3_args a;
  a.x = x, a.w = w, a.bias = bias, a.y = y, a.M = M, a.ldx = ldx, a.ldy = ldy, a.H = H, a.W = W, a.Cin = Cin, a.N = N;
  a.dil = dilation;
  const dim3 grid((unsigned)((M + C3_BM - 1) / C3_BM), (unsigned)(N / C3_BN));
  conv3x3_relu_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return check_launch("conv3x3_relu_kernel");
}

extern "C" int ls_maxpool2x2_ceil(const uint16_t* x, int32_t ldx, int32_t n_img, int32_t H, int32_t W, int32_t C,
                                  uint16_t* y, int32_t ldy, void* stream) {
  if (!x || !y) return fail(LS_ERR_INVALID, "ls_maxpool2x2_ceil: null pointer");
  if (C < 8 || C % 8 || ldx % 8 || ldy % 8 || ldx < C || ldy < C)
    return fail(LS_ERR_INVALID, "ls_maxpool2x2_ceil: C, ldx and ldy must be multiples of 8 and the pitches at least C");
  if (n_img < 1 || H < 1 || W < 1) return fail(LS_ERR_INVALID, "ls_maxpool2x2_ceil: need n_img, H, W >= 1");
  if (misaligned16(x) || misaligned16(y))
    return fail(LS_ERR_INVALID, "ls_maxpool2x2_ceil: x and y must be 16-byte aligned");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long total = (long)n_img * Ho * Wo * (C / 8);
  maxpool2x2_ceil_kernel<<<(int)std::min<long>(cdiv(total, 256), 16384), 256, 0, (hipStream_t)stream>>>(
      x, ldx, n_img, H, W, C / 8, Ho, Wo, y, ldy);
  return check_launch("maxpool2x2_ceil_kernel");
}

extern "C" int ls_l2norm_scale(const uint16_t* x, int32_t ldx, int64_t M, int32_t C, const float* weight, uint16_t* y,
                               int32_t ldy, void* stream) {
  if (!x || !weight || !y) return fail(LS_ERR_INVALID, "ls_l2norm_scale: null pointer");
  if (C < 8 || C % 8 || C > 8192 || ldx % 8 || ldy % 8 || ldx < C || ldy < C)
    return fail(LS_ERR_INVALID, "ls_l2norm_scale: C (8..8192), ldx and ldy must be multiples of 8 and the pitches at "
                                "least C");
  if (M < 1 || (M + 3) / 4 > 0x7fffffffL) return fail(LS_ERR_INVALID, "ls_l2norm_scale: M must be in 1 .. 2^33");
  if (misaligned16(x) || misaligned16(y) || misaligned16(weight))
    return fail(LS_ERR_INVALID, "ls_l2norm_scale: x, y and weight must be 16-byte aligned");
  l2norm_scale_kernel<<<(unsigned)((M + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, ldx, M, C / 8, weight, y, ldy);
  return check_launch("l2norm_scale_kernel");
}

extern "C" size_t ls_s3fd_detect_workspace_bytes(int32_t n, int32_t P) {
  if (n < 1 || P < 1 || P > DET_MAX_P) return 0;
  return (size_t)n * ((size_t)pow2_ceil(P) * 8 + (size_t)P * 16 + (size_t)DET_NMS_TOPK * 16);
}

extern "C" int ls_s3fd_detect(const float* const* maps, const int32_t* map_hw, int32_t n, const float* priors,
                              int32_t P, float* out, int32_t* counts, int32_t* keep_idx, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!maps || !map_hw || !priors || !out || !counts) return fail(LS_ERR_INVALID, "ls_s3fd_detect: null pointer");
  if (n < 1 || n > 65535) return fail(LS_ERR_INVALID, "ls_s3fd_detect: n must be in 1..65535");
  if (P < 1 || P > DET_MAX_P)
    return fail(LS_ERR_INVALID, "ls_s3fd_detect: the prior count must be in 1..65536 (detect at a smaller scale)");
  det_args a;
  long total = 0;
  for (int l = 0; l < 6; ++l) {
    if (!maps[l] || ((uintptr_t)maps[l] & 3)) return fail(LS_ERR_INVALID, "ls_s3fd_detect: null or misaligned head map");
    const long h = map_hw[2 * l], w = map_hw[2 * l + 1];
    if (h < 1 || w < 1 || h * w > DET_MAX_P) return fail(LS_ERR_INVALID, "ls_s3fd_detect: a head map size is out of range");
    a.map[l] = maps[l];
    a.npix[l] = (int)(h * w);
    total += h * w;
  }
  if (total != P) return fail(LS_ERR_INVALID, "ls_s3fd_detect: the head maps do not hold one pixel per prior");
  if (misaligned16(priors)) return fail(LS_ERR_INVALID, "ls_s3fd_detect: priors must be 16-byte aligned");
  const size_t need = ls_s3fd_detect_workspace_bytes(n, P);
  if (!workspace || workspace_bytes < need || misaligned16(workspace))
    return fail(LS_ERR_WORKSPACE, "ls_s3fd_detect: workspace null, misaligned or smaller than "
                                  "ls_s3fd_detect_workspace_bytes");
  a.priors = priors, a.out = out, a.counts = counts, a.keep_idx = keep_idx, a.P = P, a.P2 = (int)pow2_ceil(P);
  char* ws = (char*)workspace;
  a.keys = (unsigned long long*)ws;
  ws += (size_t)n * a.P2 * 8;
  a.boxes = (float4*)ws;
  ws += (size_t)n * P * 16;
  a.sbox = (float4*)ws;
  s3fd_detect_kernel<<<n, DET_THREADS, 0, (hipStream_t)stream>>>(a);
  return check_launch("s3fd_detect_kernel");
}

extern "C" int ls_nms_boxes(const float* det, int32_t n, int32_t R, float conf_th, float frame_w, float frame_h,
                            float thresh, float* out, int32_t* counts, int32_t* keep_idx, void* stream) {
  if (!det || !out || !counts) return fail(LS_ERR_INVALID, "ls_nms_boxes: null pointer");
  if (n < 1 || n > 65535 || R < 1 || R > NB_MAX_ROWS)
    return fail(LS_ERR_INVALID, "ls_nms_boxes: n must be in 1..65535 and the rows per frame in 1..4096");
  if (!(conf_th >= 0.f) || !(thresh >= 0.f) || !(frame_w > 0.f) || !(frame_h > 0.f))
    return fail(LS_ERR_INVALID, "ls_nms_boxes: conf_th and thresh must be >= 0 and the frame size positive");
  nms_boxes_kernel<<<n, NB_THREADS, 0, (hipStream_t)stream>>>(det, R, conf_th, frame_w, frame_h, thresh, out, counts,
                                                               keep_idx);
  return check_launch("nms_boxes_kernel");
}
