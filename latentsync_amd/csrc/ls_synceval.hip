// The classic SyncNet evaluation (eval/eval_sync_conf.py of the reference: eval/syncnet/syncnet.py
// class S, eval/syncnet/syncnet_eval.py class SyncNetEval, eval/syncnet_detect.py crop_video) on
// gfx950: what AV offset, LSE-D and LSE-C need beyond the kernels the UNet and StableSyncNet use.
//
//  * mfcc_kernel: python_speech_features.mfcc(audio_int16, 16000) with that library's defaults,
//    from its published definition (the library is not a dependency): pre-emphasis 0.97, frames
//    of 400 every 160 with a zero-padded tail and a RECTANGULAR window, |rfft(., 512)|^2 / 512,
//    26 triangular mel filters, log, orthonormal DCT-II, coefficients 0..12, lifter 22,
//    coefficient 0 = log(frame energy).  One block owns MF_FR frames: the samples and a 512-entry
//    twiddle table in LDS, a direct DFT per (frame, bin) over the 400 live samples, the power
//    spectrum to LDS, one thread per (frame, filter), then one per (frame, coefficient).  fp32,
//    every sum in a fixed order.  One launch, no workspace.
//  * conv_general_kernel: S's convolutions -- 5x7x7 over (time, y, x), 5x5, 3x3, the 6x6 and 5x4
//    valid convs and the heads' linears -- as ONE implicit GEMM on v_mfma_f32_16x16x32_bf16.  The
//    form is conv3x3_strided_kernel's (ls_syncnet.hip): a wave owns 16 output pixels x 16 NT
//    channels and reads both operands straight from memory in MFMA fragment order; lane (r, g) =
//    (lane % 16, lane / 16) holds the 8 k-values 32 s + 8 g .. + 7 of pixel r and of weight row
//    r of each channel tile.  k = ((it kh + iy) kw + ix) Cin + ci, so 8 consecutive k are 8
//    consecutive channels of one tap: one 16-byte load, and a tap in the padding is a zero
//    register, never a load.  A lane walks its taps with carries instead of dividing per step.
//    From K = 2048 on the four waves of a block split the K range of one tile and wave 0 adds the
//    partials in wave order through LDS.  Which form runs depends on K and N alone, never on the
//    number of steps, so a step's result does not depend on what it is computed with.
//  * maxpool2d_kernel: bf16 NHWC max-pool, padding = -inf, 8 channels a thread.  Exact.
//  * sync_dist_kernel / sync_mean_kernel: calc_pdist (F.pairwise_distance, eps 1e-6 inside the
//    norm, against the feature rows shifted by -vshift .. vshift with zero rows past the ends)
//    and the mean over the windows, lane-strided sums and a butterfly: a fixed order.
//  * crop_track_kernel: crop_video's per-frame pad(110) / crop / cv2.resize(., (224, 224)).  cv2
//    is not a dependency and was not available to compare with: the yardstick is the CPU
//    restatement in tests/synceval_ref.py, written from OpenCV's published definition of
//    INTER_LINEAR for uint8 (resize.cpp: coefficients (float)((d + 0.5) scale - 0.5) split into
//    floor and fraction, rounded to 11-bit fixed point; the horizontal pass keeps 32-bit sums,
//    the vertical pass is ((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2 >> 2; a source
//    exactly twice the target on both axes is the 2x2 area mean (s00 + s01 + s10 + s11 + 2) >> 2).
#include "ls_common.h"

namespace ls {

// ------------------------------------------------------------------------------------ MFCC
constexpr int MF_WIN = 400, MF_HOP = 160, MF_FFT = 512, MF_BINS = MF_FFT / 2 + 1, MF_FILT = 26, MF_CEP = 13,
              MF_FR = 4;
constexpr float MF_EPS = 2.220446049250313e-16f;  // numpy.finfo(float).eps = 2^-52, exact in fp32

__global__ void __launch_bounds__(256)
mfcc_kernel(const float* __restrict__ audio, long n, int T, const float* __restrict__ filters,
            float* __restrict__ out) {
  __shared__ float xw[MF_FR][MF_WIN];
  __shared__ float cs[MF_FFT], sn[MF_FFT];
  __shared__ float pw[MF_FR][MF_BINS + 3];
  __shared__ float lf[MF_FR][MF_FILT];
  __shared__ float le[MF_FR];
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * MF_FR;
  for (int i = tid; i < MF_FFT; i += 256) {
    float s, c;
    sincospif(2.0f * (float)i / (float)MF_FFT, &s, &c);
    cs[i] = c;
    sn[i] = s;
  }
  for (int i = tid; i < MF_FR * MF_WIN; i += 256) {
    const int f = i / MF_WIN, k = i - f * MF_WIN;
    const long j = (long)(t0 + f) * MF_HOP + k;
    float v = 0.f;  // the zero-padded tail (and frames past T, never stored)
    if (t0 + f < T && j < n) v = j > 0 ? audio[j] - 0.97f * audio[j - 1] : audio[0];
    xw[f][k] = v;
  }
  __syncthreads();
  for (int p = tid; p < MF_FR * MF_BINS; p += 256) {
    const int f = p / MF_BINS, k = p - f * MF_BINS;
    float re = 0.f, im = 0.f;
    int idx = 0;
    const float* x = xw[f];
#pragma unroll 8
    for (int i = 0; i < MF_WIN; ++i) {
      re = fmaf(x[i], cs[idx], re);
      im = fmaf(x[i], sn[idx], im);
      idx = (idx + k) & (MF_FFT - 1);
    }
    pw[f][k] = (re * re + im * im) * (1.0f / MF_FFT);
  }
  __syncthreads();
  for (int p = tid; p < MF_FR * (MF_FILT + 1); p += 256) {
    const int f = p / (MF_FILT + 1), b = p - f * (MF_FILT + 1);
    float s = 0.f;
    if (b == MF_FILT) {  // the frame energy
      for (int k = 0; k < MF_BINS; ++k) s += pw[f][k];
      le[f] = logf(s == 0.f ? MF_EPS : s);
    } else {
      const float* fr = filters + b * MF_BINS;
      for (int k = 0; k < MF_BINS; ++k) s = fmaf(fr[k], pw[f][k], s);
      lf[f][b] = logf(s == 0.f ? MF_EPS : s);
    }
  }
  __syncthreads();
  for (int p = tid; p < MF_FR * MF_CEP; p += 256) {
    const int f = p / MF_CEP, c = p - f * MF_CEP;
    const int t = t0 + f;
    if (t >= T) continue;
    float v;
    if (c == 0) {
      v = le[f];
    } else {
      float s = 0.f;
      for (int m = 0; m < MF_FILT; ++m) s = fmaf(lf[f][m], cospif((float)(c * (2 * m + 1)) / (2.0f * MF_FILT)), s);
      // DCT-II, norm = "ortho": sqrt(2 / N) for c > 0; lifter 1 + (L / 2) sin(pi c / L), L = 22
      v = s * 0.27735009811261457f * (1.0f + 11.0f * sinpif((float)c / 22.0f));
    }
    out[(long)c * T + t] = v;
  }
}

// ---------------------------------------------------------------------- general convolution
struct gconv_args {
  const u16* x;
  const u16* w;
  const float* bias;
  void* y;
  long M, frame;  // frame = H W ldx
  int ldx, ldy, H, W, Cin, K, N, Ho, Wo, kt, kh, kw, sh, sw, ph, pw, relu, f32;
};

constexpr int GCONV_SPLIT_K = 2048;  // K from which the four waves of a block split one tile's K range

template <int NT, bool SPLIT>
__global__ void __launch_bounds__(256) conv_general_kernel(const gconv_args a) {
  __shared__ f32x4 red[SPLIT ? 3 * NT * 64 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const long mt = SPLIT ? (long)blockIdx.x : (long)blockIdx.x * 4 + wave;
  if (!SPLIT && mt * 16 >= a.M) return;
  const int n0 = blockIdx.y * (16 * NT);
  const long p = mt * 16 + r;
  const bool pv = p < a.M;
  long t = 0;
  int oy = 0, ox = 0;
  if (pv) {
    const int hw = a.Ho * a.Wo;
    t = p / hw;
    const int rem = (int)(p - t * hw);
    oy = rem / a.Wo;
    ox = rem - oy * a.Wo;
  }
  const int iy0 = oy * a.sh - a.ph, ix0 = ox * a.sw - a.pw;
  const u16* xt = a.x + t * a.frame;
  const int ksteps = a.K / 32;
  const int s0 = SPLIT ? ksteps * wave / 4 : 0, s1 = SPLIT ? ksteps * (wave + 1) / 4 : ksteps;
  // this lane's first k = 32 s0 + 8 g as (it, iy, ix, ci); every step adds 32 to ci with carries
  int ci, ix, iy, it;
  {
    const int k = s0 * 32 + g * 8;
    int tap = k / a.Cin;
    ci = k - tap * a.Cin;
    ix = tap % a.kw;
    tap /= a.kw;
    iy = tap % a.kh;
    it = tap / a.kh;
  }
  const u16* wrow[NT];
  bool wok[NT];
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + j * 16 + r;
    wok[j] = n < a.N;
    wrow[j] = a.w + (long)(wok[j] ? n : 0) * a.K;
    acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  for (int s = s0; s < s1; ++s) {
    const int k = s * 32 + g * 8;
    uint4 xv = make_uint4(0u, 0u, 0u, 0u);
    if (pv && it < a.kt) {  // it == kt: the zero columns that round K up to 64
      const int yy = iy0 + iy, xx = ix0 + ix;
      if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W)
        xv = *(const uint4*)(xt + (long)it * a.frame + ((long)yy * a.W + xx) * a.ldx + ci);
    }
    const bf16x8 xf = __builtin_bit_cast(bf16x8, xv);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const uint4 wv = wok[j] ? *(const uint4*)(wrow[j] + k) : make_uint4(0u, 0u, 0u, 0u);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wv), xf, acc[j], 0, 0, 0);
    }
    ci += 32;
    while (ci >= a.Cin && it < a.kt) {
      ci -= a.Cin;
      if (++ix == a.kw) {
        ix = 0;
        if (++iy == a.kh) {
          iy = 0;
          ++it;
        }
      }
    }
  }
  if (SPLIT) {
    if (wave > 0) {
#pragma unroll
      for (int j = 0; j < NT; ++j) red[((wave - 1) * NT + j) * 64 + lane] = acc[j];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] += red[(w * NT + j) * 64 + lane];
  }
  if (!pv) return;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + j * 16 + g * 4;  // the accumulator lane: channels n .. n + 3 of pixel r
    if (n >= a.N) continue;
    float v[4] = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (a.bias && n + i < a.N) v[i] += a.bias[n + i];
      if (a.relu) v[i] = fmaxf(v[i], 0.f);
    }
    if (a.f32) {
      float* yp = (float*)a.y + p * a.ldy;
      for (int i = 0; i < 4 && n + i < a.N; ++i) yp[n + i] = v[i];
    } else {
      u16* yp = (u16*)a.y + p * a.ldy;
      if (n + 3 < a.N) {
        *(uint2*)(yp + n) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
      } else {
        for (int i = 0; n + i < a.N; ++i) yp[n + i] = f2bf(v[i]);
      }
    }
  }
}

template <int NT>
static void gconv_launch(const gconv_args& a, bool split, hipStream_t s) {
  const long mtiles = (a.M + 15) / 16;
  const dim3 grid((unsigned)(split ? mtiles : (mtiles + 3) / 4), (unsigned)cdiv(a.N, 16 * NT));
  if (split)
    conv_general_kernel<NT, true><<<grid, 256, 0, s>>>(a);
  else
    conv_general_kernel<NT, false><<<grid, 256, 0, s>>>(a);
}

// --------------------------------------------------------------------------------- max-pool
__global__ void __launch_bounds__(256)
maxpool2d_kernel(const u16* __restrict__ x, int ldx, long n_img, int H, int W, int C8, int kh, int kw, int sh,
                 int sw, int ph, int pw, int Ho, int Wo, u16* __restrict__ y, int ldy) {
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
    for (int dy = 0; dy < kh; ++dy) {
      const int yy = oy * sh - ph + dy;
      if (yy < 0 || yy >= H) continue;
      for (int dx = 0; dx < kw; ++dx) {
        const int xx = ox * sw - pw + dx;
        if (xx < 0 || xx >= W) continue;
        float v[8];
        unpack8(*(const uint4*)(x + ((img * H + yy) * W + xx) * ldx + c8 * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = (v[j] > m[j] || v[j] != v[j]) ? v[j] : m[j];  // a NaN wins, as in torch
      }
    }
    *(uint4*)(y + p * ldy + c8 * 8) = pack8(m);  // bf16 -> fp32 -> bf16 of the same value: exact
  }
}

// ------------------------------------------------------------------- offset search distances
// dists[i][j] = | im[i] - ccp[i + j] + 1e-6 |_2, ccp = cc with vshift zero rows at each end
__global__ void __launch_bounds__(64)
sync_dist_kernel(const float* __restrict__ im, const float* __restrict__ cc, int n, int D, int vshift,
                 float* __restrict__ dists) {
  const int i = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
  const int win = 2 * vshift + 1;
  const int rr = i + j - vshift;
  const bool live = rr >= 0 && rr < n;
  const float* a = im + (long)i * D;
  const float* b = cc + (long)(live ? rr : 0) * D;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float e = a[d] - (live ? b[d] : 0.f) + 1e-6f;
    s = fmaf(e, e, s);
  }
  s = wave_sum(s);
  if (lane == 0) dists[(long)i * win + j] = sqrtf(s);
}

__global__ void __launch_bounds__(64)
sync_mean_kernel(const float* __restrict__ dists, int n, int win, float* __restrict__ mean_dists) {
  const int j = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s += dists[(long)i * win + j];
  s = wave_sum(s);
  if (lane == 0) mean_dists[j] = s / (float)n;
}

// ------------------------------------------------------------------------ face-track crop
constexpr int CT_OUT = 224, CT_PAD = 110;

__device__ __forceinline__ int ct_src(const uint8_t* __restrict__ f, int H, int W, int bsi, int py, int px, int c) {
  const int y = py - bsi, x = px - bsi;  // padded-frame -> frame coordinates
  return (y >= 0 && y < H && x >= 0 && x < W) ? (int)f[((long)y * W + x) * 3 + c] : CT_PAD;
}

// cv2's linear coefficients of destination index d: the source index (clamped the way the
// horizontal table is) and the 11-bit weights of it and of its right / lower neighbour
__device__ __forceinline__ void ct_coef(int d, double scale, int size, bool horizontal, int* s, int* w0, int* w1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int i = (int)floorf(f);
  f -= (float)i;
  if (horizontal) {
    if (i < 0) f = 0.f, i = 0;
    if (i >= size - 1) f = 0.f, i = size - 1;
  }
  *s = i;
  *w0 = (int)rintf((1.0f - f) * 2048.0f);  // saturate_cast<short>: round half to even
  *w1 = (int)rintf(f * 2048.0f);
}

__global__ void __launch_bounds__(256)
crop_track_kernel(const uint8_t* __restrict__ frames, int n, int H, int W, const int* __restrict__ plan,
                  uint8_t* __restrict__ out) {
  const long total = (long)n * CT_OUT * CT_OUT;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int dx = (int)(i % CT_OUT);
    const long q = i / CT_OUT;
    const int dy = (int)(q % CT_OUT), fi = (int)(q / CT_OUT);
    const int y0 = plan[fi * 5], y1 = plan[fi * 5 + 1], x0 = plan[fi * 5 + 2], x1 = plan[fi * 5 + 3],
              bsi = plan[fi * 5 + 4];
    const int sh = y1 - y0, sw = x1 - x0;
    const uint8_t* f = frames + (long)fi * H * W * 3;
    uint8_t* o = out + i * 3;
    if (sh < 1 || sw < 1) {  // the host refuses an empty crop; never read
      o[0] = o[1] = o[2] = 0;
      continue;
    }
    if (sh == 2 * CT_OUT && sw == 2 * CT_OUT) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int py = y0 + 2 * dy, px = x0 + 2 * dx;
        o[c] = (uint8_t)((ct_src(f, H, W, bsi, py, px, c) + ct_src(f, H, W, bsi, py, px + 1, c) +
                          ct_src(f, H, W, bsi, py + 1, px, c) + ct_src(f, H, W, bsi, py + 1, px + 1, c) + 2) >> 2);
      }
      continue;
    }
    const double scx = 1.0 / ((double)CT_OUT / (double)sw), scy = 1.0 / ((double)CT_OUT / (double)sh);
    int sx, a0, ax, sy, b0, by;
    ct_coef(dx, scx, sw, true, &sx, &a0, &ax);
    ct_coef(dy, scy, sh, false, &sy, &b0, &by);
    const int xa = x0 + sx, xb = x0 + min(sx + 1, sw - 1);
    const int ya = y0 + min(max(sy, 0), sh - 1), yb = y0 + min(max(sy + 1, 0), sh - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int r0 = ct_src(f, H, W, bsi, ya, xa, c) * a0 + ct_src(f, H, W, bsi, ya, xb, c) * ax;
      const int r1 = ct_src(f, H, W, bsi, yb, xa, c) * a0 + ct_src(f, H, W, bsi, yb, xb, c) * ax;
      o[c] = (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((by * (r1 >> 4)) >> 16) + 2) >> 2);
    }
  }
}

static bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace ls

using namespace ls;

extern "C" int ls_mfcc(const float* audio, int64_t n, const float* filters, float* out, void* stream) {
  if (!audio || !filters || !out) return fail(LS_ERR_INVALID, "ls_mfcc: null pointer");
  // the frame count and the grid stay in int32: 2^38 samples are 200 days of audio
  if (n < 1 || n > ((int64_t)1 << 38)) return fail(LS_ERR_INVALID, "ls_mfcc: n must be in 1 .. 2^38");
  const long T = n > MF_WIN ? 1 + (n - MF_WIN + MF_HOP - 1) / MF_HOP : 1;
  mfcc_kernel<<<(unsigned)cdiv(T, MF_FR), 256, 0, (hipStream_t)stream>>>(audio, n, (int)T, filters, out);
  return check_launch("mfcc_kernel");
}

extern "C" int ls_conv_general(const uint16_t* x, int32_t ldx, int32_t T, int32_t H, int32_t W, int32_t Cin,
                               const uint16_t* w, int32_t K, int32_t N, const float* bias, int32_t kt, int32_t kh,
                               int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                               int32_t act, void* y, int32_t ldy, int32_t y_f32, void* stream) {
  if (!x || !w || !y) return fail(LS_ERR_INVALID, "ls_conv_general: null pointer");
  if (kt < 1 || kt > 5 || kh < 1 || kh > 7 || kw < 1 || kw > 7)
    return fail(LS_ERR_INVALID, "ls_conv_general: the window must be 1..5 x 1..7 x 1..7");
  if (stride_h < 1 || stride_h > 2 || stride_w < 1 || stride_w > 2)
    return fail(LS_ERR_INVALID, "ls_conv_general: strides must be 1 or 2");
  if (pad_h < 0 || pad_h > 1 || pad_w < 0 || pad_w > 1)
    return fail(LS_ERR_INVALID, "ls_conv_general: pads must be 0 or 1");
  if (act != 0 && act != 1) return fail(LS_ERR_INVALID, "ls_conv_general: act must be 0 (none) or 1 (ReLU)");
  if (y_f32 != 0 && y_f32 != 1) return fail(LS_ERR_INVALID, "ls_conv_general: y_f32 must be 0 or 1");
  if (Cin < 8 || Cin % 8 || Cin > (1 << 16) || ldx % 8 || ldx < Cin || N < 1 || ldy < N || (!y_f32 && ldy % 8))
    return fail(LS_ERR_INVALID, "ls_conv_general: Cin and ldx (and a bf16 ldy) must be multiples of 8, ldx >= Cin, "
                                "ldy >= N >= 1");
  if (K != (kt * kh * kw * Cin + 63) / 64 * 64)
    return fail(LS_ERR_INVALID, "ls_conv_general: K must be kt kh kw Cin rounded up to 64 (packing.pack_weight_general)");
  if (T < kt || H < 1 || W < 1 || H + 2 * pad_h < kh || W + 2 * pad_w < kw)
    return fail(LS_ERR_INVALID, "ls_conv_general: the window does not fit into the input");
  if (misaligned16(x) || misaligned16(w) || (!y_f32 && misaligned16(y)) || (y_f32 && ((uintptr_t)y & 3)))
    return fail(LS_ERR_INVALID, "ls_conv_general: x, w and a bf16 y must be 16-byte aligned");
  const int Ho = (H + 2 * pad_h - kh) / stride_h + 1, Wo = (W + 2 * pad_w - kw) / stride_w + 1;
  const long M = (long)(T - kt + 1) * Ho * Wo;
  const long mtiles = (M + 15) / 16;
  if (mtiles > 0x7fffffffL || (long)H * W * ldx > 0x7fffffffL || N > 65535 * 16)
    return fail(LS_ERR_INVALID, "ls_conv_general: shape too large for one grid");
  gconv_args a;
  a.x = x, a.w = w, a.bias = bias, a.y = y, a.M = M, a.frame = (long)H * W * ldx;
  a.ldx = ldx, a.ldy = ldy, a.H = H, a.W = W, a.Cin = Cin, a.K = K, a.N = N, a.Ho = Ho, a.Wo = Wo;
  a.kt = kt, a.kh = kh, a.kw = kw, a.sh = stride_h, a.sw = stride_w, a.ph = pad_h, a.pw = pad_w;
  a.relu = act, a.f32 = y_f32;
  const bool split = K >= GCONV_SPLIT_K;
  hipStream_t s = (hipStream_t)stream;
  if (N <= 16)
    gconv_launch<1>(a, split, s);
  else if (N <= 32)
    gconv_launch<2>(a, split, s);
  else
    gconv_launch<4>(a, split, s);
  return check_launch("conv_general_kernel");
}

extern "C" int ls_maxpool2d(const uint16_t* x, int32_t ldx, int32_t n_img, int32_t H, int32_t W, int32_t C,
                            int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                            uint16_t* y, int32_t ldy, void* stream) {
  if (!x || !y) return fail(LS_ERR_INVALID, "ls_maxpool2d: null pointer");
  if (kh < 1 || kh > 3 || kw < 1 || kw > 3 || stride_h < 1 || stride_h > 2 || stride_w < 1 || stride_w > 2)
    return fail(LS_ERR_INVALID, "ls_maxpool2d: the window must be 1..3 and the strides 1..2 per axis");
  if (pad_h < 0 || pad_h > 1 || pad_w < 0 || pad_w > 1 || 2 * pad_h > kh || 2 * pad_w > kw)
    return fail(LS_ERR_INVALID, "ls_maxpool2d: pads must be 0 or 1 and at most half the window");
  if (C < 8 || C % 8 || ldx % 8 || ldy % 8 || ldx < C || ldy < C)
    return fail(LS_ERR_INVALID, "ls_maxpool2d: C, ldx and ldy must be multiples of 8 and the pitches at least C");
  if (n_img < 1 || H < 1 || W < 1 || H + 2 * pad_h < kh || W + 2 * pad_w < kw)
    return fail(LS_ERR_INVALID, "ls_maxpool2d: the window does not fit into the input");
  if (misaligned16(x) || misaligned16(y)) return fail(LS_ERR_INVALID, "ls_maxpool2d: x and y must be 16-byte aligned");
  const int Ho = (H + 2 * pad_h - kh) / stride_h + 1, Wo = (W + 2 * pad_w - kw) / stride_w + 1;
  const long total = (long)n_img * Ho * Wo * (C / 8);
  maxpool2d_kernel<<<(int)std::min<long>(cdiv(total, 256), 16384), 256, 0, (hipStream_t)stream>>>(
      x, ldx, n_img, H, W, C / 8, kh, kw, stride_h, stride_w, pad_h, pad_w, Ho, Wo, y, ldy);
  return check_launch("maxpool2d_kernel");
}

extern "C" int ls_sync_offset(const float* im_feat, const float* cc_feat, int32_t n, int32_t D, int32_t vshift,
                              float* dists, float* mean_dists, void* stream) {
  if (!im_feat || !cc_feat || !dists || !mean_dists) return fail(LS_ERR_INVALID, "ls_sync_offset: null pointer");
  if (n < 1 || n > (1 << 24) || D < 1 || vshift < 0 || vshift > 15)
    return fail(LS_ERR_INVALID, "ls_sync_offset: need 1 <= n <= 2^24, D >= 1 and 0 <= vshift <= 15");
  const int win = 2 * vshift + 1;
  hipStream_t s = (hipStream_t)stream;
  sync_dist_kernel<<<dim3(n, win), 64, 0, s>>>(im_feat, cc_feat, n, D, vshift, dists);
  sync_mean_kernel<<<win, 64, 0, s>>>(dists, n, win, mean_dists);
  return check_launch("sync_dist_kernel");
}

extern "C" int ls_crop_track(const uint8_t* frames, int32_t n, int32_t H, int32_t W, const int32_t* plan,
                             uint8_t* out, void* stream) {
  if (!frames || !plan || !out) return fail(LS_ERR_INVALID, "ls_crop_track: null pointer");
  if (n < 1 || H < 1 || W < 1 || H > 32768 || W > 32768)
    return fail(LS_ERR_INVALID, "ls_crop_track: need n >= 1 and a frame size in 1..32768");
  const long total = (long)n * CT_OUT * CT_OUT;
  crop_track_kernel<<<(int)std::min<long>(cdiv(total, 256), 16384), 256, 0, (hipStream_t)stream>>>(
      frames, n, H, W, plan, out);
  return check_launch("crop_track_kernel");
}
