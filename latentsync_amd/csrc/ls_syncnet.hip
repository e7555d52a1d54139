// StableSyncNet (latentsync/models/stable_syncnet.py) on gfx950: what the sync-confidence
// score needs beyond the conv / norm / attention kernels the UNet already uses.
//
//  * syncnet_mel_kernel: the Wav2Lip-style mel front end (latentsync/utils/audio.py:59-65,
//    configs/audio.yaml): pre-emphasis 0.97, STFT n_fft = win = 800, hop 200, periodic Hann,
//    centred with ZERO padding, magnitude, 80-band filterbank, 20 log10(max(1e-5, .)) - 20,
//    clip(8 (S + 100) / 100 - 4, -4, 4).  One block owns SM_FR frames: windowed samples and an
//    800-entry twiddle table in LDS, a direct DFT per (frame, bin) (800 x 401 fp32 MACs per
//    frame at 80 frames per second of audio), the magnitudes to LDS, then one thread per
//    (frame, band).  One launch, no workspace.
//  * syncnet_pack_frames_kernel / syncnet_pack_mel_kernel: uint8 faces -> the visual
//    encoder's (B, R/2, R, 3F) window tensor; mel columns -> the audio encoder's
//    channel-padded (B, 80, L, 8) image.
//  * conv3x3_strided_kernel: the three anisotropic downsamplers (strides [1,2], [2,1],
//    [2,3] after a one-sided F.pad, stable_syncnet.py:95-109, 129-131) as an implicit GEMM
//    on v_mfma_f32_16x16x32_bf16.  A wave owns 16 output pixels x 16 NT channels and reads
//    both operands straight from memory in MFMA fragment order: lane (r, g) = (lane % 16,
//    lane / 16) holds the 8 k-values 32 s + 8 g .. + 7 of pixel r (B operand) and of weight
//    row r of each channel tile (A operand); 8 consecutive k are 8 consecutive channels of one
//    tap in both of pack_weight's orders, so each is one 16-byte load, and a tap outside the
//    image is a zero register, never a load.  The accumulator lane then holds channels
//    4 g .. 4 g + 3 of pixel r: one 8-byte store.  From K = 2048 on (the 512-channel layers
//    and deeper, where an image has a handful of pixels) the four waves of a block split the
//    K range of ONE tile and wave 0 adds the partials in wave order through LDS.  Which form
//    runs depends on K and N alone, never on the number of images, so a window's result does
//    not depend on its batch.
//  * sync_score_kernel: ReLU, F.normalize (eps 1e-12) of both embeddings and their
//    cosine (eps 1e-8), one wave per window.
#include "ls_common.h"

namespace ls {

constexpr int SM_FFT = 800, SM_HOP = 200, SM_FREQ = SM_FFT / 2 + 1, SM_MELS = 80, SM_FR = 4;

__global__ void __launch_bounds__(256)
syncnet_mel_kernel(const float* __restrict__ audio, long n, int T, const float* __restrict__ filters,
                   float* __restrict__ out) {
  __shared__ float xw[SM_FR][SM_FFT];
  __shared__ float cs[SM_FFT], sn[SM_FFT];
  __shared__ float mg[SM_FR][SM_FREQ + 3];
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * SM_FR;
  for (int i = tid; i < SM_FFT; i += 256) {
    float s, c;
    sincospif(2.0f * (float)i / (float)SM_FFT, &s, &c);
    cs[i] = c;
    sn[i] = s;
  }
  __syncthreads();
  for (int i = tid; i < SM_FR * SM_FFT; i += 256) {
    const int f = i / SM_FFT, k = i - f * SM_FFT;
    const int t = t0 + f;
    float v = 0.f;
    const long j = (long)t * SM_HOP + k - SM_FFT / 2;  // centre padding, zeros
    if (t < T && j >= 0 && j < n) {
      const float y = j > 0 ? audio[j] - 0.97f * audio[j - 1] : audio[0];  // pre-emphasis
      v = y * (0.5f - 0.5f * cs[k]);                                      // periodic Hann
    }
    xw[f][k] = v;
  }
  __syncthreads();
  for (int p = tid; p < SM_FR * SM_FREQ; p += 256) {
    const int f = p / SM_FREQ, k = p - f * SM_FREQ;
    float re = 0.f, im = 0.f;
    int idx = 0;
    const float* x = xw[f];
#pragma unroll 8
    for (int i = 0; i < SM_FFT; ++i) {
      re = fmaf(x[i], cs[idx], re);
      im = fmaf(x[i], sn[idx], im);
      idx += k;
      if (idx >= SM_FFT) idx -= SM_FFT;
    }
    mg[f][k] = sqrtf(re * re + im * im);
  }
  __syncthreads();
  for (int p = tid; p < SM_FR * SM_MELS; p += 256) {
    const int f = p / SM_MELS, b = p - f * SM_MELS;
    const int t = t0 + f;
    if (t >= T) continue;
    const float* fr = filters + (long)b * SM_FREQ;
    float s = 0.f;
    for (int k = 0; k < SM_FREQ; ++k) s = fmaf(fr[k], mg[f][k], s);
    const float db = 20.0f * log10f(fmaxf(1e-5f, s)) - 20.0f;
    const float v = 8.0f * ((db + 100.0f) / 100.0f) - 4.0f;
    out[(long)t * SM_MELS + b] = fminf(fmaxf(v, -4.0f), 4.0f);
  }
}

// out[b][y][x][3 f + c] = (faces[starts[b] + f][R/2 + y][x][c] / 255 - 0.5) / 0.5; 8 channels a thread
__global__ void syncnet_pack_frames_kernel(const uint8_t* __restrict__ faces, int n, int R,
                                           const int* __restrict__ starts, int B, int F, u16* __restrict__ out) {
  const int C8 = 3 * F / 8, hr = R / 2;
  const long total = (long)B * hr * R * C8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % C8);
    long p = i / C8;
    const int x = (int)(p % R);
    p /= R;
    const int y = (int)(p % hr), b = (int)(p / hr);
    const int s = starts[b];
    const bool ok = s >= 0 && s + F <= n;  // the host raises for such a window; never read past the end
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ch = c8 * 8 + j;
      const int f = ch / 3, c = ch - f * 3;
      float u = 0.f;
      if (ok) u = (float)faces[(((long)(s + f) * R + hr + y) * R + x) * 3 + c];
      v[j] = ok ? (u / 255.0f - 0.5f) / 0.5f : 0.f;
    }
    *(uint4*)(out + i * 8) = pack8(v);
  }
}

// out[b][m][j][0] = mel[cols[b] + j][m], channels 1..7 zero
__global__ void syncnet_pack_mel_kernel(const float* __restrict__ mel, int T, const int* __restrict__ cols, int B,
                                        int L, u16* __restrict__ out) {
  const long total = (long)B * SM_MELS * L;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i % L);
    const long p = i / L;
    const int m = (int)(p % SM_MELS), b = (int)(p / SM_MELS);
    const long t = (long)cols[b] + j;
    const float v = (t >= 0 && t < T) ? mel[t * SM_MELS + m] : 0.f;
    *(uint4*)(out + i * 8) = make_uint4(pack2(v, 0.f), 0u, 0u, 0u);
  }
}

struct sconv_args {
  const u16* x;
  const u16* w;
  const float* bias;
  u16* y;
  long M;
  int ldx, ldy, H, W, Cin, K, N, Ho, Wo, sh, sw, pt, pl, chunk_major;
};

constexpr int SCONV_SPLIT_K = 2048;  // K from which the four waves of a block split one tile's K range

template <int NT, bool SPLIT>
__global__ void __launch_bounds__(256) conv3x3_strided_kernel(const sconv_args a) {
  __shared__ f32x4 red[SPLIT ? 3 * NT * 64 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const long mt = SPLIT ? (long)blockIdx.x : (long)blockIdx.x * 4 + wave;
  if (!SPLIT && mt * 16 >= a.M) return;
  const int n0 = blockIdx.y * (16 * NT);
  const long p = mt * 16 + r;
  const bool pv = p < a.M;
  int img = 0, oy = 0, ox = 0;
  if (pv) {
    const int hw = a.Ho * a.Wo;
    img = (int)(p / hw);
    const int rem = (int)(p - (long)img * hw);
    oy = rem / a.Wo;
    ox = rem - oy * a.Wo;
  }
  const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;
  const u16* ximg = a.x + (long)img * a.H * a.W * a.ldx;
  const int ksteps = a.K / 32;
  const int s0 = SPLIT ? ksteps * wave / 4 : 0, s1 = SPLIT ? ksteps * (wave + 1) / 4 : ksteps;
  const int kreal = 9 * a.Cin;
  const u16* wrow[NT];
  bool wok[NT];
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + t * 16 + r;
    wok[t] = n < a.N;
    wrow[t] = a.w + (long)(wok[t] ? n : 0) * a.K;
    acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  for (int s = s0; s < s1; ++s) {
    const int k = s * 32 + g * 8;
    uint4 xv = make_uint4(0u, 0u, 0u, 0u);
    if (pv && k < kreal) {
      int tap, ci;
      if (a.chunk_major) {  // k = (ci / 64) * 576 + tap * 64 + ci % 64
        const int c64 = k / 576, rem = k - c64 * 576;
        tap = rem >> 6;
        ci = c64 * 64 + (rem & 63);
      } else {  // k = tap * Cin + ci
        tap = k / a.Cin;
        ci = k - tap * a.Cin;
      }
      const int ky = tap / 3, kx = tap - ky * 3;
      const int iy = iy0 + ky, ix = ix0 + kx;
      if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) xv = *(const uint4*)(ximg + ((long)iy * a.W + ix) * a.ldx + ci);
    }
    const bf16x8 xf = __builtin_bit_cast(bf16x8, xv);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint4 wv = wok[t] ? *(const uint4*)(wrow[t] + k) : make_uint4(0u, 0u, 0u, 0u);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wv), xf, acc[t], 0, 0, 0);
    }
  }
  if (SPLIT) {
    if (wave > 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) red[((wave - 1) * NT + t) * 64 + lane] = acc[t];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] += red[(w * NT + t) * 64 + lane];
  }
  if (!pv) return;
  u16* yp = a.y + p * a.ldy;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + t * 16 + g * 4;  // the accumulator lane: channels n .. n + 3 of pixel r
    if (n >= a.N) continue;
    float v[4] = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
    if (a.bias) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (n + i < a.N) v[i] += a.bias[n + i];
    }
    if (n + 3 < a.N) {
      *(uint2*)(yp + n) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    } else {
      for (int i = 0; n + i < a.N; ++i) yp[n + i] = f2bf(v[i]);
    }
  }
}

template <int NT>
static void sconv_launch(const sconv_args& a, bool split, hipStream_t s) {
  const long mtiles = (a.M + 15) / 16;
  const dim3 grid((unsigned)(split ? mtiles : (mtiles + 3) / 4), (unsigned)cdiv(a.N, 16 * NT));
  if (split)
    conv3x3_strided_kernel<NT, true><<<grid, 256, 0, s>>>(a);
  else
    conv3x3_strided_kernel<NT, false><<<grid, 256, 0, s>>>(a);
}

// v = relu(vin) / max(|relu(vin)|, 1e-12), a likewise, score = v . a / (max(|v|, 1e-8) max(|a|, 1e-8))
__global__ void __launch_bounds__(64)
sync_score_kernel(const u16* __restrict__ vin, int ldv, const u16* __restrict__ ain, int lda, int D,
                  float* __restrict__ v, float* __restrict__ a, int ldo, float* __restrict__ score) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const u16* vr = vin + (long)b * ldv;
  const u16* ar = ain + (long)b * lda;
  float sv = 0.f, sa = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float x = fmaxf(bf2f(vr[d]), 0.f), y = fmaxf(bf2f(ar[d]), 0.f);
    sv = fmaf(x, x, sv);
    sa = fmaf(y, y, sa);
  }
  const float iv = 1.0f / fmaxf(sqrtf(wave_sum(sv)), 1e-12f), ia = 1.0f / fmaxf(sqrtf(wave_sum(sa)), 1e-12f);
  float dot = 0.f, nv = 0.f, na = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float x = fmaxf(bf2f(vr[d]), 0.f) * iv, y = fmaxf(bf2f(ar[d]), 0.f) * ia;
    v[(long)b * ldo + d] = x;
    a[(long)b * ldo + d] = y;
    dot = fmaf(x, y, dot);
    nv = fmaf(x, x, nv);
    na = fmaf(y, y, na);
  }
  dot = wave_sum(dot);
  nv = sqrtf(wave_sum(nv));
  na = sqrtf(wave_sum(na));
  if (lane == 0) score[b] = dot / (fmaxf(nv, 1e-8f) * fmaxf(na, 1e-8f));
}

static bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace ls

using namespace ls;

extern "C" int ls_syncnet_mel(const float* audio, int64_t n, const float* filters, float* out, void* stream) {
  if (!audio || !filters || !out) return fail(LS_ERR_INVALID, "ls_syncnet_mel: null pointer");
  // T = 1 + n / 200 frames and the grid (T / 4 blocks) stay in int32: 2^38 samples are 200 days of audio
  if (n < 1 || n > ((int64_t)1 << 38)) return fail(LS_ERR_INVALID, "ls_syncnet_mel: n must be in 1 .. 2^38");
  const long T = 1 + n / SM_HOP;
  syncnet_mel_kernel<<<(unsigned)cdiv(T, SM_FR), 256, 0, (hipStream_t)stream>>>(audio, n, (int)T, filters, out);
  return check_launch("syncnet_mel_kernel");
}

extern "C" int ls_syncnet_pack_frames(const uint8_t* faces, int32_t n, int32_t R, const int32_t* starts, int32_t B,
                                      int32_t F, uint16_t* out, void* stream) {
  if (!faces || !starts || !out) return fail(LS_ERR_INVALID, "ls_syncnet_pack_frames: null pointer");
  if (n < 1 || B < 1 || R < 2 || R % 2 || R > 32768 || F < 1 || F > n || (3 * F) % 8 || misaligned16(out))
    return fail(LS_ERR_INVALID, "ls_syncnet_pack_frames: need n, B >= 1, an even R, 1 <= F <= n, 3 F % 8 == 0 and a "
                                "16-byte aligned output");
  const long total = (long)B * (R / 2) * R * (3 * F / 8);
  syncnet_pack_frames_kernel<<<(int)std::min<long>(cdiv(total, 256), 8192), 256, 0, (hipStream_t)stream>>>(
      faces, n, R, starts, B, F, out);
  return check_launch("syncnet_pack_frames_kernel");
}

extern "C" int ls_syncnet_pack_mel(const float* mel, int32_t T, const int32_t* cols, int32_t B, int32_t L,
                                   uint16_t* out, void* stream) {
  if (!mel || !cols || !out) return fail(LS_ERR_INVALID, "ls_syncnet_pack_mel: null pointer");
  if (T < 1 || B < 1 || L < 1 || L > T || misaligned16(out))
    return fail(LS_ERR_INVALID, "ls_syncnet_pack_mel: need B >= 1, 1 <= L <= T and a 16-byte aligned output");
  const long total = (long)B * SM_MELS * L;
  syncnet_pack_mel_kernel<<<(int)std::min<long>(cdiv(total, 256), 8192), 256, 0, (hipStream_t)stream>>>(
      mel, T, cols, B, L, out);
  return check_launch("syncnet_pack_mel_kernel");
}

extern "C" int ls_conv3x3_strided(const uint16_t* x, int32_t ldx, int32_t n_img, int32_t H, int32_t W, int32_t Cin,
                                  const uint16_t* w, int32_t K, int32_t N, const float* bias, int32_t stride_h,
                                  int32_t stride_w, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo,
                                  uint16_t* y, int32_t ldy, void* stream) {
  if (!x || !w || !y) return fail(LS_ERR_INVALID, "ls_conv3x3_strided: null pointer");
  if (stride_h < 1 || stride_h > 3 || stride_w < 1 || stride_w > 3)
    return fail(LS_ERR_INVALID, "ls_conv3x3_strided: strides must be 1, 2 or 3");
  if (pad_top < 0 || pad_top > 1 || pad_left < 0 || pad_left > 1)
    return fail(LS_ERR_INVALID, "ls_conv3x3_strided: pad_top and pad_left must be 0 or 1");
  if (Cin < 8 || Cin % 8 || ldx % 8 || ldy % 8 || ldx < Cin || ldy < N || N < 1)
    return fail(LS_ERR_INVALID, "ls_conv3x3_strided: Cin, ldx and ldy must be multiples of 8, ldx >= Cin, ldy >= N >= 1");
  if (Cin > (1 << 20) || K != (9 * Cin + 63) / 64 * 64)
    return fail(LS_ERR_INVALID, "ls_conv3x3_strided: K must be 9 Cin rounded up to 64 (packing.pack_weight)");
  if (n_img < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || (long)(Ho - 1) * stride_h - pad_top >= H ||
      (long)(Wo - 1) * stride_w - pad_left >= W)
    return fail(LS_ERR_INVALID, "ls_conv3x3_strided: every output pixel's first tap row and column must lie in the image");
  if (misaligned16(x) || misaligned16(w) || misaligned16(y))
    return fail(LS_ERR_INVALID, "ls_conv3x3_strided: x, w and y must be 16-byte aligned");
  const long M = (long)n_img * Ho * Wo;
  const long mtiles = (M + 15) / 16;
  if (mtiles > 0x7fffffffL || (long)Ho * Wo > 0x7fffffffL || (long)H * W > 0x7fffffffL || N > 65535 * 16)
    return fail(LS_ERR_INVALID, "ls_conv3x3_strided: shape too large for one grid");
  sconv_args a;
  a.x = x, a.w = w, a.bias = bias, a.y = y, a.M = M;
  a.ldx = ldx, a.ldy = ldy, a.H = H, a.W = W, a.Cin = Cin, a.K = K, a.N = N, a.Ho = Ho, a.Wo = Wo;
  a.sh = stride_h, a.sw = stride_w, a.pt = pad_top, a.pl = pad_left, a.chunk_major = Cin % 64 == 0;
  const bool split = K >= SCONV_SPLIT_K;
  hipStream_t s = (hipStream_t)stream;
  if (N <= 16)
    sconv_launch<1>(a, split, s);
  else if (N <= 32)
    sconv_launch<2>(a, split, s);
  else
    sconv_launch<4>(a, split, s);
  return check_launch("conv3x3_strided_kernel");
}

extern "C" int ls_sync_score(const uint16_t* v_in, int32_t ldv, const uint16_t* a_in, int32_t lda, int32_t B,
                             int32_t D, float* v, float* a, int32_t ldo, float* score, void* stream) {
  if (!v_in || !a_in || !v || !a || !score) return fail(LS_ERR_INVALID, "ls_sync_score: null pointer");
  if (B < 1 || D < 1 || ldv < D || lda < D || ldo < D)
    return fail(LS_ERR_INVALID, "ls_sync_score: need B, D >= 1 and pitches of at least D");
  sync_score_kernel<<<B, 64, 0, (hipStream_t)stream>>>(v_in, ldv, a_in, lda, D, v, a, ldo, score);
  return check_launch("sync_score_kernel");
}
