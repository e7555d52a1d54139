// GIF thumbnail of a result on gfx950 (the reference's create_video_thumbnail_gif,
// latentsync/utils/thumbnail.py, which runs on the host with cv2, Pillow and imageio): the
// selected frames, uint8 RGB (n, H, W, 3) on the device, are area-resized, the overlay is
// blended in, a 5-5-5 colour histogram goes to the host (which designs the palette), pixels
// are mapped through the resulting table and LZW-coded.  Only the histogram, the table and
// the compressed bytes cross to the host (latentsync_amd/thumbnail.py); DESIGN.md section
// 4.6 holds the exact definitions.
//
//  * resize_area_kernel: cv2.resize(..., INTER_AREA) for a downscale.  One thread per
//    output pixel derives the (source index, weight) entries of its column and its row in
//    fp64 as OpenCV's computeResizeAreaTab does, then sums in fp32 in OpenCV's order:
//    columns of one source row first, rows second, one rounding per multiply and per add
//    (no contraction), round half to even at the end.  Integer factors on both axes take
//    the integer path (sum, one multiply by 1 / area; (s + 2) >> 2 for 2 x 2).
//  * overlay_blend_kernel: one thread per pixel walks the layers in order; the layer
//    descriptors travel as a kernel argument.
//  * rgb555_hist_kernel: block-private LDS table of the 8192 bins of one quarter of the red
//    range (blockIdx.y picks the quarter), flushed with global atomics; counts are exact.
//  * palette_map_kernel: one table lookup per pixel.
//  * gif_lzw_strip_kernel: one wave per (frame, strip of GIF_STRIP_ROWS rows).  LZW is
//    serial: lane 0 codes, the whole wave stages the pixels and clears the dictionary (an
//    LDS hash table of (prefix << 8 | byte) << 12 | code words).  Every strip is a
//    self-contained piece of one ordinary stream: it ends with CLEAR (EOI for the last) at
//    the width a decoder has reached, so the next strip starts from a fresh dictionary.
//  * gif_lzw_scan_kernel / gif_lzw_merge_kernel: prefix sums of the strips' bit lengths,
//    then one lane per output byte gathers its 8 bits, LSB first, from the one or two
//    strips that hold them.  Writes past `out_capacity` are dropped, offsets stay exact.
// Every pixel, bit and byte index is 64-bit.
#include "ls_common.h"

// No a * b + c of this file may be fused: the resize must round every product and every sum
// as OpenCV's scalar code (and numpy) does.  Plain operators are used throughout, because
// the __fmul_rn / __fadd_rn wrappers are defined before this pragma, carry the default
// contraction flag into the kernel when inlined and are fused all the same.
#pragma clang fp contract(off)

namespace ls {

constexpr int TH_MAX_LAYERS = 16;
constexpr int TH_MAX_GRID = 1 << 16;           // blocks of a grid-stride launch
constexpr int GIF_STRIP_ROWS = 8;
constexpr int LZ_TAB = 8192;                   // hash slots: at most 3838 live entries
constexpr int LZ_CHUNK = 4096;                 // pixels staged in LDS at a time
constexpr uint32_t LZ_EMPTY = 0xffffffffu;
constexpr int LZ_CLEAR = 256, LZ_EOI = 257, LZ_FIRST = 258, LZ_LAST = 4095;
enum { LZ_EV_DONE = 0, LZ_EV_CLEAR = 1, LZ_EV_DATA = 2 };

// ------------------------------------------------------------------ INTER_AREA resize

// computeResizeAreaTab for one destination index: an optional partial cell (first, a_first)
// on the left, the full cells [s1, s2) at a_full, an optional partial cell s2 at a_last.
struct AreaTaps {
  int s1, s2, first, last;
  float a_first, a_full, a_last;
  __device__ __forceinline__ int count() const { return first + (s2 - s1) + last; }
  __device__ __forceinline__ void entry(int k, int smax, int* si, float* a) const {
    int s;
    if (first && k == 0) {
      s = s1 - 1;
      *a = a_first;
    } else if (k - first < s2 - s1) {
      s = s1 + k - first;
      *a = a_full;
    } else {
      s = s2;
      *a = a_last;
    }
    *si = s < 0 ? 0 : (s > smax ? smax : s);
  }
};

__device__ __forceinline__ AreaTaps area_taps(int d, double scale, int ssize) {
  AreaTaps t;
  const double f1 = (double)d * scale;
  const double f2 = f1 + scale;
  const double cw = fmin(scale, (double)ssize - f1);
  int s1 = (int)ceil(f1), s2 = (int)floor(f2);
  s2 = min(s2, ssize - 1);
  s1 = min(s1, s2);
  t.s1 = s1;
  t.s2 = s2;
  t.first = ((double)s1 - f1 > 1e-3) ? 1 : 0;
  t.a_first = (float)(((double)s1 - f1) / cw);
  t.a_full = (float)(1.0 / cw);
  t.last = (f2 - (double)s2 > 1e-3) ? 1 : 0;
  t.a_last = (float)(fmin(fmin(f2 - (double)s2, 1.0), cw) / cw);
  return t;
}

__device__ __forceinline__ uint8_t sat_u8(float v) {
  const float r = rintf(v);  // round half to even
  return (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

__global__ void __launch_bounds__(256)
resize_area_kernel(const uint8_t* __restrict__ src, long total, int H, int W, int dh, int dw, double sy, double sx,
                   int iy, int ix, float inv_area, uint8_t* __restrict__ dst) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % dw);
    const long r = i / dw;
    const int y = (int)(r % dh);
    const long f = r / dh;
    const uint8_t* fr = src + f * H * W * 3;
    uint8_t o[3];
    if (ix > 0) {  // integer factors on both axes
      int s[3] = {0, 0, 0};
      for (int j = 0; j < iy; ++j) {
        const uint8_t* p = fr + ((long)(y * iy + j) * W + (long)x * ix) * 3;
        for (int k = 0; k < ix; ++k, p += 3) {
          s[0] += p[0];
          s[1] += p[1];
          s[2] += p[2];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
        o[c] = (ix == 2 && iy == 2) ? (uint8_t)((s[c] + 2) >> 2) : sat_u8((float)s[c] * inv_area);
    } else {
      const AreaTaps tx = area_taps(x, sx, W), ty = area_taps(y, sy, H);
      const int nx = tx.count(), ny = ty.count();
      float sum[3] = {0.f, 0.f, 0.f};
      for (int j = 0; j < ny; ++j) {
        int yy;
        float beta;
        ty.entry(j, H - 1, &yy, &beta);
        const uint8_t* row = fr + (long)yy * W * 3;
        float buf[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < nx; ++k) {
          int xx;
          float alpha;
          tx.entry(k, W - 1, &xx, &alpha);
          const uint8_t* p = row + (long)xx * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) buf[c] = buf[c] + (float)p[c] * alpha;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
          sum[c] = j == 0 ? beta * buf[c] : sum[c] + beta * buf[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = sat_u8(sum[c]);
    }
    uint8_t* q = dst + i * 3;
    q[0] = o[0];
    q[1] = o[1];
    q[2] = o[2];
  }
}

// ------------------------------------------------------------------ overlay

struct ThLayers {
  int n;
  int d[TH_MAX_LAYERS][8];  // x0, y0, w, h, alpha-map offset, r, g, b
};

// Pillow's blend of an ink at alpha a over dst: (ink a + dst (255 - a)) / 255, rounded
__device__ __forceinline__ int blend255(int ink, int dst, int a) {
  const int t = ink * a + dst * (255 - a) + 128;
  return ((t >> 8) + t) >> 8;
}

__global__ void __launch_bounds__(256)
overlay_blend_kernel(uint8_t* __restrict__ frames, long total, int H, int W, const uint8_t* __restrict__ alpha,
                     ThLayers L) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    uint8_t* p = frames + i * 3;
    int r = p[0], g = p[1], b = p[2];
    bool touched = false;
    for (int l = 0; l < L.n; ++l) {
      const int lx = x - L.d[l][0], ly = y - L.d[l][1];
      if (lx < 0 || ly < 0 || lx >= L.d[l][2] || ly >= L.d[l][3]) continue;
      const int a = alpha[(long)L.d[l][4] + (long)ly * L.d[l][2] + lx];
      if (a == 0) continue;
      r = blend255(L.d[l][5], r, a);
      g = blend255(L.d[l][6], g, a);
      b = blend255(L.d[l][7], b, a);
      touched = true;
    }
    if (touched) {
      p[0] = (uint8_t)r;
      p[1] = (uint8_t)g;
      p[2] = (uint8_t)b;
    }
  }
}

// ------------------------------------------------------------------ histogram, palette map

__device__ __forceinline__ int key555(const uint8_t* p) { return ((p[0] >> 3) << 10) | ((p[1] >> 3) << 5) | (p[2] >> 3); }

__global__ void __launch_bounds__(256)
rgb555_hist_kernel(const uint8_t* __restrict__ frames, long total, uint32_t* __restrict__ hist) {
  __shared__ uint32_t part[8192];
  const int q = blockIdx.y;  // the quarter of the red range this block counts
  for (int i = threadIdx.x; i < 8192; i += 256) part[i] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int k = key555(frames + i * 3);
    if ((k >> 13) == q) atomicAdd(&part[k & 8191], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 8192; i += 256) {
    const uint32_t v = part[i];
    if (v) atomicAdd(&hist[q * 8192 + i], v);
  }
}

__global__ void __launch_bounds__(256)
palette_map_kernel(const uint8_t* __restrict__ frames, long total, const uint8_t* __restrict__ lut,
                   uint8_t* __restrict__ idx) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256)
    idx[i] = lut[key555(frames + i * 3)];
}

// ------------------------------------------------------------------ LZW

__device__ __forceinline__ int th_wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// LSB-first bit writer of lane 0 into the strip's slot
struct LzBits {
  uint32_t* dst;
  uint64_t acc;
  int nacc, w, total;
  __device__ __forceinline__ void put(uint32_t code, int n) {  // n <= 12, nacc < 32
    acc |= (uint64_t)code << nacc;
    nacc += n;
    total += n;
    if (nacc >= 32) {
      dst[w++] = (uint32_t)acc;
      acc >>= 32;
      nacc -= 32;
    }
  }
};

__global__ void __launch_bounds__(64)
gif_lzw_strip_kernel(const uint8_t* __restrict__ idx, int H, int W, int nstrips, long slot_dw,
                     uint32_t* __restrict__ slots, int* __restrict__ nbits) {
  __shared__ uint32_t tab[LZ_TAB];
  __shared__ uint8_t px[LZ_CHUNK];
  __shared__ int ev;
  const int lane = threadIdx.x;
  const int s = blockIdx.x, f = blockIdx.y;
  const int r0 = s * GIF_STRIP_ROWS;
  const int npx = min(GIF_STRIP_ROWS, H - r0) * W;  // <= 8 * 65535
  const uint8_t* in = idx + ((long)f * H + r0) * W;
  const long strip = (long)f * nstrips + s;
  LzBits bw{slots + strip * slot_dw, 0, 0, 0, 0};
  int width = 9, next = LZ_FIRST, prefix = 0, pos = 0, chunk0 = 0;
  bool need_clear = true, need_data = true;
  for (;;) {
    if (need_clear)
      for (int i = lane; i < LZ_TAB; i += 64) tab[i] = LZ_EMPTY;
    if (need_data) {
      const int n = min(LZ_CHUNK, npx - chunk0);
      for (int i = lane; i < n; i += 64) px[i] = in[chunk0 + i];
    }
    __syncthreads();
    if (lane == 0) {
      int e = LZ_EV_DONE;
      if (pos == 0) {
        if (s == 0) bw.put(LZ_CLEAR, 9);
        prefix = px[0];
        pos = 1;
      }
      for (;;) {
        if (pos == npx) {
          // the last code of the strip, the width bump a decoder makes after it, the terminator
          bw.put((uint32_t)prefix, width);
          const int code = next++;
          if (code == (1 << width) && width < 12) ++width;
          bw.put(s == nstrips - 1 ? LZ_EOI : LZ_CLEAR, width);
          if (bw.nacc) bw.dst[bw.w++] = (uint32_t)bw.acc;
          nbits[strip] = bw.total;
          break;
        }
        if (pos - chunk0 == LZ_CHUNK) {
          e = LZ_EV_DATA;
          break;
        }
        const uint32_t c = px[pos - chunk0];
        const uint32_t key = ((uint32_t)prefix << 8) | c;
        uint32_t h = (key * 2654435761u) >> 19;
        bool hit = false;
        for (;;) {
          const uint32_t t = tab[h];
          if (t == LZ_EMPTY) break;
          if ((t >> 12) == key) {
            prefix = (int)(t & 4095u);
            hit = true;
            break;
          }
          h = (h + 1) & (LZ_TAB - 1);
        }
        ++pos;
        if (hit) continue;
        bw.put((uint32_t)prefix, width);
        prefix = (int)c;
        const int code = next++;
        if (code == LZ_LAST) {  // the dictionary is full: CLEAR at width 12 and start over
          bw.put(LZ_CLEAR, width);
          width = 9;
          next = LZ_FIRST;
          e = LZ_EV_CLEAR;
          break;
        }
        tab[h] = (key << 12) | (uint32_t)code;
        if (code == (1 << width)) ++width;
      }
      ev = e;
    }
    __syncthreads();
    const int e = ev;
    if (e == LZ_EV_DONE) break;
    need_clear = e == LZ_EV_CLEAR;
    need_data = e == LZ_EV_DATA;
    if (need_data) chunk0 += LZ_CHUNK;
  }
}

// One wave: bitoff[f][k] = bits of the strips of frame f before strip k (k = nstrips: all of
// them), offsets[f + 1] = bytes of the frames up to f, each frame padded to a whole byte.
__global__ void __launch_bounds__(64)
gif_lzw_scan_kernel(const int* __restrict__ nbits, int nstrips, int n, long* __restrict__ bitoff,
                    long* __restrict__ offsets) {
  const int lane = threadIdx.x;
  long bytes = 0;
  if (lane == 0) offsets[0] = 0;
  for (int f = 0; f < n; ++f) {
    long carry = 0;
    long* bo = bitoff + (long)f * (nstrips + 1);
    for (int base = 0; base < nstrips; base += 64) {
      const int i = base + lane;
      const int v = i < nstrips ? nbits[(long)f * nstrips + i] : 0;
      const int incl = th_wave_incl_scan(v, lane);  // 64 strips x at most 6.3 Mbit
      if (i < nstrips) bo[i] = carry + incl - v;
      carry += __shfl(incl, 63, 64);
    }
    bytes += (carry + 7) >> 3;
    if (lane == 0) {
      bo[nstrips] = carry;
      offsets[f + 1] = bytes;
    }
  }
}

__global__ void __launch_bounds__(256)
gif_lzw_merge_kernel(const uint32_t* __restrict__ slots, long slot_dw, const long* __restrict__ bitoff,
                     const long* __restrict__ offsets, int nstrips, uint8_t* __restrict__ out, long capacity) {
  const int f = blockIdx.y;
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  const long* bo = bitoff + (long)f * (nstrips + 1);
  if (b >= ((bo[nstrips] + 7) >> 3)) return;
  const long p = b * 8;
  int lo = 0, hi = nstrips - 1;  // the last strip that starts at or before bit p
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bo[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  uint32_t byte = 0;
  int got = 0;
  for (int k = lo; got < 8 && k < nstrips; ++k) {
    const long q = p + got - bo[k];
    const long len = bo[k + 1] - bo[k];
    const int take = (int)min((long)(8 - got), len - q);
    // the slot has a spare dword past its worst case, so byte (q >> 3) + 1 is inside it
    const uint8_t* sb = (const uint8_t*)(slots + ((long)f * nstrips + k) * slot_dw);
    const uint32_t two = (uint32_t)sb[q >> 3] | ((uint32_t)sb[(q >> 3) + 1] << 8);
    byte |= ((two >> (q & 7)) & ((1u << take) - 1u)) << got;
    got += take;
  }
  const long at = offsets[f] + b;
  if (at < capacity) out[at] = (uint8_t)byte;
}

struct LzGeom {
  int nstrips;
  long slot_dw;
  size_t slots_b, nbits_b, bitoff_b;
};

static bool lz_geom(int n, int H, int W, LzGeom* g) {
  if (n < 1 || n > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535) return false;  // 16-bit sizes in the descriptor
  g->nstrips = (H + GIF_STRIP_ROWS - 1) / GIF_STRIP_ROWS;
  // worst case: every pixel its own code plus the two CLEAR / EOI, 12 bits each (the CLEAR of a
  // full dictionary is paid for by that cycle's 9..11-bit codes), and one spare dword
  const long bits = ((long)GIF_STRIP_ROWS * W + 2) * 12;
  g->slot_dw = (bits + 31) / 32 + 1;
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t ns = (size_t)n * g->nstrips;
  g->slots_b = up(ns * g->slot_dw * 4);
  g->nbits_b = up(ns * 4);
  g->bitoff_b = up((size_t)n * (g->nstrips + 1) * 8);
  return true;
}

static int th_grid(long total) { return (int)std::min<long>((total + 255) / 256, TH_MAX_GRID); }

}  // namespace ls

using namespace ls;

extern "C" int ls_resize_area_u8(const uint8_t* src, int32_t n, int32_t H, int32_t W, uint8_t* dst, int32_t dh,
                                 int32_t dw, void* stream) {
  if (!src || !dst) return fail(LS_ERR_INVALID, "ls_resize_area_u8: null pointer");
  if (n < 1 || H < 1 || W < 1 || dh < 1 || dw < 1 || H > 65535 || W > 65535)
    return fail(LS_ERR_INVALID, "ls_resize_area_u8: need n >= 1 and sizes in 1..65535");
  if (dh > H || dw > W)
    return fail(LS_ERR_INVALID, "ls_resize_area_u8: " + std::to_string(H) + "x" + std::to_string(W) + " -> " +
                                    std::to_string(dh) + "x" + std::to_string(dw) + " is not a downscale");
  // cv::resize: scale = 1 / (dst / src) in fp64; the integer path when both are integers
  const double sx = 1.0 / ((double)dw / (double)W), sy = 1.0 / ((double)dh / (double)H);
  const int ix = (int)lrint(sx), iy = (int)lrint(sy);
  const bool fast = fabs(sx - ix) < 2.220446049250313e-16 && fabs(sy - iy) < 2.220446049250313e-16;
  const float inv_area = 1.0f / (float)(ix * iy);
  const long total = (long)n * dh * dw;
  resize_area_kernel<<<th_grid(total), 256, 0, (hipStream_t)stream>>>(src, total, H, W, dh, dw, sy, sx, fast ? iy : 0,
                                                                      fast ? ix : 0, inv_area, dst);
  return check_launch("resize_area_kernel");
}

extern "C" int ls_overlay_blend_u8(uint8_t* frames, int32_t n, int32_t H, int32_t W, const int32_t* layers,
                                   int32_t n_layers, const uint8_t* alpha, int64_t alpha_bytes, void* stream) {
  if (!frames) return fail(LS_ERR_INVALID, "ls_overlay_blend_u8: null pointer");
  if (n < 1 || H < 1 || W < 1) return fail(LS_ERR_INVALID, "ls_overlay_blend_u8: need n, H, W >= 1");
  if (n_layers < 0 || n_layers > TH_MAX_LAYERS)
    return fail(LS_ERR_INVALID, "ls_overlay_blend_u8: " + std::to_string(n_layers) + " layers outside 0..16");
  if (n_layers == 0) return LS_OK;
  if (!layers || alpha_bytes < 0) return fail(LS_ERR_INVALID, "ls_overlay_blend_u8: null layers or negative alpha_bytes");
  ThLayers L;
  L.n = n_layers;
  bool any = false;
  for (int l = 0; l < n_layers; ++l) {
    const int32_t* d = layers + 8 * l;
    const int64_t area = (int64_t)d[2] * d[3];
    if (d[2] < 0 || d[3] < 0 || d[4] < 0 || (int64_t)d[4] + area > alpha_bytes || (d[5] | d[6] | d[7]) < 0 ||
        d[5] > 255 || d[6] > 255 || d[7] > 255)
      return fail(LS_ERR_INVALID, "ls_overlay_blend_u8: layer " + std::to_string(l) +
                                      ": negative size, alpha map outside alpha_bytes or ink outside 0..255");
    any = any || area > 0;
    for (int k = 0; k < 8; ++k) L.d[l][k] = d[k];
  }
  if (!any) return LS_OK;
  if (!alpha) return fail(LS_ERR_INVALID, "ls_overlay_blend_u8: null alpha");
  const long total = (long)n * H * W;
  overlay_blend_kernel<<<th_grid(total), 256, 0, (hipStream_t)stream>>>(frames, total, H, W, alpha, L);
  return check_launch("overlay_blend_kernel");
}

extern "C" int ls_rgb555_hist(const uint8_t* frames, int32_t n, int32_t H, int32_t W, uint32_t* hist, void* stream) {
  if (!frames || !hist) return fail(LS_ERR_INVALID, "ls_rgb555_hist: null pointer");
  if (n < 1 || H < 1 || W < 1) return fail(LS_ERR_INVALID, "ls_rgb555_hist: need n, H, W >= 1");
  const long total = (long)n * H * W;
  if (total > 0xffffffffL) return fail(LS_ERR_INVALID, "ls_rgb555_hist: more than 2^32 - 1 pixels");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, 32768 * sizeof(uint32_t), s) != hipSuccess)
    return fail(LS_ERR_LAUNCH, "ls_rgb555_hist: memset");
  const int gx = (int)std::min<long>((total + 256 * 16 - 1) / (256 * 16), 1024);
  rgb555_hist_kernel<<<dim3(gx, 4), 256, 0, s>>>(frames, total, hist);
  return check_launch("rgb555_hist_kernel");
}

extern "C" int ls_palette_map(const uint8_t* frames, int32_t n, int32_t H, int32_t W, const uint8_t* lut, uint8_t* idx,
                              void* stream) {
  if (!frames || !lut || !idx) return fail(LS_ERR_INVALID, "ls_palette_map: null pointer");
  if (n < 1 || H < 1 || W < 1) return fail(LS_ERR_INVALID, "ls_palette_map: need n, H, W >= 1");
  const long total = (long)n * H * W;
  palette_map_kernel<<<th_grid(total), 256, 0, (hipStream_t)stream>>>(frames, total, lut, idx);
  return check_launch("palette_map_kernel");
}

extern "C" int ls_gif_strip_rows(void) { return GIF_STRIP_ROWS; }

extern "C" size_t ls_gif_lzw_workspace_bytes(int32_t n, int32_t H, int32_t W) {
  LzGeom g;
  if (!lz_geom(n, H, W, &g)) return 0;
  return g.slots_b + g.nbits_b + g.bitoff_b + 256;
}

extern "C" int ls_gif_lzw(const uint8_t* idx, int32_t n, int32_t H, int32_t W, uint8_t* out, int64_t out_capacity,
                          int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream) {
  if (!idx || !out || !offsets) return fail(LS_ERR_INVALID, "ls_gif_lzw: null pointer");
  if (out_capacity < 0) return fail(LS_ERR_INVALID, "ls_gif_lzw: negative out_capacity");
  LzGeom g;
  if (!lz_geom(n, H, W, &g)) return fail(LS_ERR_INVALID, "ls_gif_lzw: need 1 <= n, H, W <= 65535");
  if (!workspace || workspace_bytes < ls_gif_lzw_workspace_bytes(n, H, W))
    return fail(LS_ERR_WORKSPACE, "ls_gif_lzw: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  uint32_t* slots = (uint32_t*)ws;
  int* nbits = (int*)(ws + g.slots_b);
  long* bitoff = (long*)(ws + g.slots_b + g.nbits_b);
  gif_lzw_strip_kernel<<<dim3(g.nstrips, n), 64, 0, s>>>(idx, H, W, g.nstrips, g.slot_dw, slots, nbits);
  if (int rc = check_launch("gif_lzw_strip_kernel")) return rc;
  gif_lzw_scan_kernel<<<1, 64, 0, s>>>(nbits, g.nstrips, n, bitoff, (long*)offsets);
  if (int rc = check_launch("gif_lzw_scan_kernel")) return rc;
  const long worst = (long)g.nstrips * g.slot_dw * 4;  // bytes of a frame whose every strip is worst case
  gif_lzw_merge_kernel<<<dim3((unsigned)((worst + 255) / 256), n), 256, 0, s>>>(slots, g.slot_dw, bitoff,
                                                                                 (const long*)offsets, g.nstrips, out,
                                                                                 (long)out_capacity);
  return check_launch("gif_lzw_merge_kernel");
}
