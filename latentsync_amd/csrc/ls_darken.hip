// Face brightness restore on gfx950: what the reference's write_video does to every output
// frame of a use_darken request (darken_restore.enhance_face_brightness), on the restored
// frames where they already are -- uint8 RGB (n, H, W, 3) on the device, in place.
// DESIGN.md section 4.4 holds the exact arithmetic; the host half (latentsync_amd/darken.py)
// turns the caller's landmarks into convex hulls, a per-frame plan and one region of
// interest (ROI) for the clip.  Every pixel of a processed frame goes through the 8-bit
// RGB -> HSV -> RGB round trip; inside the ROI V is scaled by the feathered face mask.
//
//  * darken_fill_kernel: one thread per ROI pixel and frame; the pixel is set iff it lies
//    inside or on the boundary of hull A or hull B (int64 cross products against every
//    edge, plus the hull's bounding box so a hull of one or two vertices works too).
//  * darken_dilate_kernel: k x k box maximum, anchor k / 2, pixels outside the frame ignored.
//  * darken_hblur_kernel / darken_vblur_kernel: the separable Gaussian with
//    BORDER_REFLECT_101 at the frame edge.  A row segment / a column tile is staged in LDS
//    (zeros outside the ROI, which is where the mask is exactly zero), every thread then
//    adds its taps in the fixed order j = 0 .. n_taps - 1, each product and each sum rounded
//    to float32 (no contraction in this file).
//  * darken_apply_kernel: one thread per 4 pixels (12 bytes, three aligned dwords when the
//    frames allow it) that loops over the frames of the batch; the temporal recurrence is
//    elementwise, so `last` stays in registers and touches the carried plane only at batch
//    boundaries.
// Frames go through in batches of a fixed workspace budget: the workspace holds one batch of
// ROI planes plus the carried `last` and `first_valid` planes and does not grow with n.
#include "ls_common.h"

#pragma clang fp contract(off)

namespace ls {

constexpr size_t DK_WS_BUDGET = (size_t)96 << 20;
constexpr int DK_MAX_TAPS = 129;  // the column tile of the vertical pass stays below 64 KiB of LDS
constexpr int DK_VT = 64;         // vertical pass: 64 x 64 output tile per workgroup
// plan modes (darken.py: MODE_*)
constexpr int DK_SKIP = 0, DK_FIRST = 1, DK_BLEND = 2, DK_DECAY = 3, DK_FIRST_VALID = 4;

struct DkRoi {
  int x, y, w, h;
};
struct __attribute__((aligned(4))) DkU3 {  // four packed RGB pixels
  uint32_t a, b, c;
};

// plan row of frame f: {mode, first vertex, vertices of hull A, vertices of hull B}
__device__ __forceinline__ bool dk_detected(const int* __restrict__ plan, int f) {
  const int m = plan[4 * f];
  return m == DK_FIRST || m == DK_BLEND;
}

__device__ __forceinline__ bool dk_in_hull(const int* __restrict__ v, int nv, int px, int py) {
  if (nv < 1) return false;
  int x0 = v[0], x1 = v[0], y0 = v[1], y1 = v[1];
  bool ok = true;
  for (int i = 0; i < nv; ++i) {
    const int j = i + 1 == nv ? 0 : i + 1;
    const long ax = v[2 * i], ay = v[2 * i + 1], bx = v[2 * j], by = v[2 * j + 1];
    ok = ok && ((bx - ax) * (py - ay) - (by - ay) * (px - ax) >= 0);
    x0 = min(x0, (int)ax); x1 = max(x1, (int)ax);
    y0 = min(y0, (int)ay); y1 = max(y1, (int)ay);
  }
  return ok && px >= x0 && px <= x1 && py >= y0 && py <= y1;
}

__global__ void __launch_bounds__(256)
darken_fill_kernel(const int* __restrict__ plan, const int* __restrict__ verts, int n_verts, DkRoi roi,
                   uint8_t* __restrict__ fill, size_t plane) {
  const int f = blockIdx.z;
  if (!dk_detected(plan, f)) return;
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= roi.w) return;
  const int off = plan[4 * f + 1], na = plan[4 * f + 2], nb = plan[4 * f + 3];
  bool in = false;
  if (off >= 0 && na >= 0 && nb >= 0 && (long)off + na + nb <= n_verts) {  // a plan pointing outside: empty mask
    const int* v = verts + 2 * (size_t)off;
    in = dk_in_hull(v, na, roi.x + x, roi.y + y) || dk_in_hull(v + 2 * na, nb, roi.x + x, roi.y + y);
  }
  fill[f * plane + (size_t)y * roi.w + x] = in ? 1 : 0;
}

__global__ void __launch_bounds__(256)
darken_dilate_kernel(const int* __restrict__ plan, const uint8_t* __restrict__ fill, DkRoi roi, int k,
                     uint8_t* __restrict__ dil, size_t plane) {
  const int f = blockIdx.z;
  if (!dk_detected(plan, f)) return;
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= roi.w) return;
  const uint8_t* src = fill + f * plane;
  const int a = k / 2;
  uint8_t m = 0;
  // the ROI holds every set pixel, so a source outside it (in the frame or not) adds nothing
  for (int dy = -a; dy < k - a; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= roi.h) continue;
    for (int dx = -a; dx < k - a; ++dx) {
      const int xx = x + dx;
      if (xx >= 0 && xx < roi.w) m |= src[(size_t)yy * roi.w + xx];
    }
  }
  dil[f * plane + (size_t)y * roi.w + x] = m;
}

// BORDER_REFLECT_101 (cv2.borderInterpolate): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...
__device__ __forceinline__ int dk_reflect(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

__global__ void __launch_bounds__(256)
darken_hblur_kernel(const int* __restrict__ plan, const uint8_t* __restrict__ dil, DkRoi roi, int W,
                    const float* __restrict__ taps, int n_taps, float* __restrict__ tmp, size_t plane_u8,
                    size_t plane) {
  extern __shared__ float dk_lds[];  // taps [n_taps], then the row segment [256 + n_taps - 1]
  const int f = blockIdx.z;
  if (!dk_detected(plan, f)) return;
  float* tp = dk_lds;
  float* seg = dk_lds + n_taps;
  const int r = n_taps / 2, x0 = blockIdx.x * 256, y = blockIdx.y;
  const uint8_t* src = dil + f * plane_u8 + (size_t)y * roi.w;
  for (int i = threadIdx.x; i < n_taps; i += 256) tp[i] = taps[i];
  for (int i = threadIdx.x; i < 256 + n_taps - 1; i += 256) {
    const int xs = dk_reflect(roi.x + x0 + i - r, W) - roi.x;  // frame column -> ROI column
    seg[i] = xs >= 0 && xs < roi.w ? (float)src[xs] : 0.0f;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= roi.w) return;
  float acc = 0.0f;
  for (int j = 0; j < n_taps; ++j) acc = acc + tp[j] * seg[threadIdx.x + j];
  tmp[f * plane + (size_t)y * roi.w + x] = acc;
}

__global__ void __launch_bounds__(256)
darken_vblur_kernel(const int* __restrict__ plan, const float* __restrict__ tmp, DkRoi roi, int H,
                    const float* __restrict__ taps, int n_taps, float* __restrict__ mask, size_t plane) {
  extern __shared__ float dk_lds[];  // taps [n_taps], then the column tile [DK_VT + n_taps - 1][DK_VT]
  const int f = blockIdx.z;
  if (!dk_detected(plan, f)) return;
  float* tp = dk_lds;
  float* tile = dk_lds + n_taps;
  const int r = n_taps / 2, x0 = blockIdx.x * DK_VT, y0 = blockIdx.y * DK_VT;
  const int cx = threadIdx.x & (DK_VT - 1), ry = threadIdx.x / DK_VT;  // 64 columns x 4 rows of threads
  const float* src = tmp + f * plane;
  for (int i = threadIdx.x; i < n_taps; i += 256) tp[i] = taps[i];
  const int x = x0 + cx;
  for (int i = ry; i < DK_VT + n_taps - 1; i += 4) {
    const int ys = dk_reflect(roi.y + y0 + i - r, H) - roi.y;
    tile[i * DK_VT + cx] = x < roi.w && ys >= 0 && ys < roi.h ? src[(size_t)ys * roi.w + x] : 0.0f;
  }
  __syncthreads();
  if (x >= roi.w) return;
  for (int i = ry; i < DK_VT; i += 4) {
    const int y = y0 + i;
    if (y >= roi.h) break;
    float acc = 0.0f;
    for (int j = 0; j < n_taps; ++j) acc = acc + tp[j] * tile[(i + j) * DK_VT + cx];
    mask[f * plane + (size_t)y * roi.w + x] = acc;
  }
}

// OpenCV's 8-bit scalar RGB2HSV_b (hue range 180) and HSV2RGB_b around the scaled V
__device__ __forceinline__ void dk_pixel(uint32_t& r8, uint32_t& g8, uint32_t& b8, float factor, float vmax,
                                         const int* __restrict__ sdiv, const int* __restrict__ hdiv) {
  const int r = (int)r8, g = (int)g8, b = (int)b8;
  const int v = max(r, max(g, b)), d = v - min(r, min(g, b));
  const int s = (d * sdiv[v] + 2048) >> 12;
  int h = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
  h = (h * hdiv[d] + 2048) >> 12;
  if (h < 0) h += 180;
  const int v2 = (int)fminf(fmaxf((float)v * factor, 0.0f), vmax);  // truncated, as astype(uint8)
  const float vv = (float)v2 * (1.0f / 255.0f);
  float fr = vv, fg = vv, fb = vv;
  if (s != 0) {
    const float hh = (float)h * (6.0f / 180.0f), ss = (float)s * (1.0f / 255.0f);
    const float sec = floorf(hh), q = hh - sec;
    const float t1 = vv * (1.0f - ss), t2 = vv * (1.0f - ss * q), t3 = vv * (1.0f - ss * (1.0f - q));
    switch ((int)sec) {
      case 0: fb = t1; fg = t3; fr = vv; break;
      case 1: fb = t1; fg = vv; fr = t2; break;
      case 2: fb = t3; fg = vv; fr = t1; break;
      case 3: fb = vv; fg = t2; fr = t1; break;
      case 4: fb = vv; fg = t1; fr = t3; break;
      default: fb = t2; fg = t1; fr = vv; break;
    }
  }
  r8 = (uint32_t)fminf(fmaxf(rintf(fr * 255.0f), 0.0f), 255.0f);
  g8 = (uint32_t)fminf(fmaxf(rintf(fg * 255.0f), 0.0f), 255.0f);
  b8 = (uint32_t)fminf(fmaxf(rintf(fb * 255.0f), 0.0f), 255.0f);
}

// frames: the first frame of the batch; plan: its plan row; masks: the batch's blurred planes
template <bool ALIGNED>
__global__ void __launch_bounds__(256)
darken_apply_kernel(uint8_t* __restrict__ frames, int nf, const int* __restrict__ plan, uint32_t npix, int W, DkRoi roi,
                    const float* __restrict__ masks, size_t plane, float* __restrict__ last_plane,
                    const float* __restrict__ fv_plane, float c, int brighten, float vmax) {
  __shared__ int sdiv[256], hdiv[256];
  {
    const int i = threadIdx.x;  // cv2's tables: cvRound of the double quotient
    sdiv[i] = i ? (int)rint((double)(255 << 12) / (double)i) : 0;
    hdiv[i] = i ? (int)rint((double)(180 << 12) / (6.0 * (double)i)) : 0;
  }
  __syncthreads();
  const uint64_t q0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
  if (q0 >= npix) return;
  const uint32_t p0 = (uint32_t)q0;
  const int cnt = (int)min(4u, npix - p0);
  long ridx[4];  // ROI index of each pixel, -1 outside the ROI
  float last[4];
  {
    int y = (int)(p0 / (uint32_t)W), x = (int)(p0 - (uint32_t)y * (uint32_t)W);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rx = x - roi.x, ry = y - roi.y;
      ridx[i] = i < cnt && rx >= 0 && rx < roi.w && ry >= 0 && ry < roi.h ? (long)ry * roi.w + rx : -1;
      last[i] = ridx[i] >= 0 ? last_plane[ridx[i]] : 0.0f;
      if (++x == W) { x = 0; ++y; }
    }
  }
  const size_t frame_bytes = (size_t)npix * 3;
  bool dirty = false;
  for (int f = 0; f < nf; ++f) {
    const int mode = plan[4 * f];
    if (mode < DK_FIRST || mode > DK_FIRST_VALID) continue;
    uint8_t* px = frames + (size_t)f * frame_bytes + (size_t)p0 * 3;
    const bool wide = ALIGNED && cnt == 4;
    uint32_t ch[12];
    if (wide) {
      const DkU3 w = *(const DkU3*)px;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ch[i] = (w.a >> (8 * i)) & 255;
        ch[4 + i] = (w.b >> (8 * i)) & 255;
        ch[8 + i] = (w.c >> (8 * i)) & 255;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) ch[i] = i < 3 * cnt ? px[i] : 0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= cnt) break;
      float g = 0.0f;
      if (ridx[i] >= 0) {
        if (mode == DK_FIRST_VALID) {
          g = (fv_plane[ridx[i]] * c) * 0.8f;
        } else {
          float cur = last[i];
          if (mode == DK_DECAY) {
            last[i] = last[i] * 0.8f;
          } else {
            const float m = masks[(size_t)f * plane + ridx[i]];
            cur = mode == DK_BLEND ? 0.7f * last[i] + 0.3f * m : m;
            last[i] = cur;
          }
          dirty = true;
          g = cur * c;
        }
      }
      const float factor = brighten ? 1.0f + g : 1.0f - g;
      dk_pixel(ch[3 * i], ch[3 * i + 1], ch[3 * i + 2], factor, vmax, sdiv, hdiv);
    }
    if (wide) {
      DkU3 w;
      w.a = ch[0] | ch[1] << 8 | ch[2] << 16 | ch[3] << 24;
      w.b = ch[4] | ch[5] << 8 | ch[6] << 16 | ch[7] << 24;
      w.c = ch[8] | ch[9] << 8 | ch[10] << 16 | ch[11] << 24;
      *(DkU3*)px = w;
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * cnt) px[i] = (uint8_t)ch[i];
    }
  }
  if (dirty) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (ridx[i] >= 0) last_plane[ridx[i]] = last[i];
  }
}

struct DkGeom {
  int batch;
  size_t u8_b, f32_b;  // one ROI plane of bytes / of floats, each a multiple of 256
};

static bool dk_geom(int n, int roi_h, int roi_w, int frames_per_batch, DkGeom* g) {
  if (n < 1 || roi_h < 1 || roi_w < 1 || roi_h > 65535 || roi_w > 65535) return false;
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t px = (size_t)roi_h * roi_w;
  g->u8_b = up(px);
  g->f32_b = up(px * 4);
  size_t b = frames_per_batch > 0 ? (size_t)frames_per_batch : DK_WS_BUDGET / (2 * g->u8_b + 2 * g->f32_b);
  b = b < 1 ? 1 : b;
  b = b > 65535 ? 65535 : b;  // a grid's z extent
  g->batch = (int)(b > (size_t)n ? n : b);
  return true;
}

}  // namespace ls

using namespace ls;

extern "C" size_t ls_face_brighten_workspace_bytes(int32_t n, int32_t roi_h, int32_t roi_w, int32_t frames_per_batch) {
  DkGeom g;
  if (!dk_geom(n, roi_h, roi_w, frames_per_batch, &g)) return 0;
  return (size_t)g.batch * (2 * g.u8_b + 2 * g.f32_b) + 2 * g.f32_b + 256;
}

extern "C" int ls_face_brighten(uint8_t* frames, int32_t n, int32_t H, int32_t W, const int32_t* plan,
                                const int32_t* verts, int32_t n_verts, int32_t first_valid, int32_t roi_x,
                                int32_t roi_y, int32_t roi_w, int32_t roi_h, const float* taps, int32_t n_taps,
                                int32_t dilate, float c, int32_t brighten, int32_t max_value,
                                int32_t frames_per_batch, void* workspace, size_t workspace_bytes, void* stream) {
  if (!frames || !plan || !verts || !taps) return fail(LS_ERR_INVALID, "ls_face_brighten: null pointer");
  if (n < 1 || H < 1 || W < 1 || H > 65535 || W > 65535)
    return fail(LS_ERR_INVALID, "ls_face_brighten: need n >= 1 and 1 <= H, W <= 65535");
  if (n_taps < 1 || n_taps % 2 == 0 || n_taps > DK_MAX_TAPS)
    return fail(LS_ERR_INVALID, "ls_face_brighten: the tap count " + std::to_string(n_taps) +
                                    " must be odd and within 1.." + std::to_string(DK_MAX_TAPS));
  if (dilate < 1) return fail(LS_ERR_INVALID, "ls_face_brighten: dilate size " + std::to_string(dilate) + " below 1");
  if (n_verts < 0 || first_valid < -1 || first_valid >= n || max_value < 0 || max_value > 255)
    return fail(LS_ERR_INVALID, "ls_face_brighten: need n_verts >= 0, -1 <= first_valid < n, 0 <= max_value <= 255");
  if (roi_x < 0 || roi_y < 0 || roi_w < 1 || roi_h < 1 || roi_w > W - roi_x || roi_h > H - roi_y)
    return fail(LS_ERR_INVALID, "ls_face_brighten: the region of interest must be non-empty and inside the frame");
  DkGeom g;
  if (!dk_geom(n, roi_h, roi_w, frames_per_batch, &g)) return fail(LS_ERR_INVALID, "ls_face_brighten: bad sizes");
  if (!workspace || workspace_bytes < ls_face_brighten_workspace_bytes(n, roi_h, roi_w, frames_per_batch))
    return fail(LS_ERR_WORKSPACE, "ls_face_brighten: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* last = (float*)ws;
  float* fv = (float*)(ws + g.f32_b);
  uint8_t* fill = (uint8_t*)(ws + 2 * g.f32_b);
  uint8_t* dil = fill + (size_t)g.batch * g.u8_b;
  float* tmp = (float*)(dil + (size_t)g.batch * g.u8_b);
  float* mask = (float*)((char*)tmp + (size_t)g.batch * g.f32_b);
  const DkRoi roi = {roi_x, roi_y, roi_w, roi_h};
  const size_t h_lds = (size_t)(n_taps + 256 + n_taps - 1) * 4;
  const size_t v_lds = (size_t)(n_taps + (DK_VT + n_taps - 1) * DK_VT) * 4;
  // the blurred mask of frames plan[0 .. nf) into `out` (plane strides in elements)
  auto masks_of = [&](const int32_t* pl, int nf, float* out) -> int {
    const dim3 rows(cdiv(roi_w, 256), roi_h, nf);
    darken_fill_kernel<<<rows, 256, 0, s>>>(pl, verts, n_verts, roi, fill, g.u8_b);
    if (int rc = check_launch("darken_fill_kernel")) return rc;
    darken_dilate_kernel<<<rows, 256, 0, s>>>(pl, fill, roi, dilate, dil, g.u8_b);
    if (int rc = check_launch("darken_dilate_kernel")) return rc;
    darken_hblur_kernel<<<rows, 256, h_lds, s>>>(pl, dil, roi, W, taps, n_taps, tmp, g.u8_b, g.f32_b / 4);
    if (int rc = check_launch("darken_hblur_kernel")) return rc;
    darken_vblur_kernel<<<dim3(cdiv(roi_w, DK_VT), cdiv(roi_h, DK_VT), nf), 256, v_lds, s>>>(
        pl, tmp, roi, H, taps, n_taps, out, g.f32_b / 4);
    return check_launch("darken_vblur_kernel");
  };
  if (first_valid >= 0)
    if (int rc = masks_of(plan + 4 * (size_t)first_valid, 1, fv)) return rc;
  const uint32_t npix = (uint32_t)H * (uint32_t)W;
  const size_t frame_bytes = (size_t)npix * 3;
  const bool aligned = (((uintptr_t)frames | frame_bytes) & 3) == 0;
  const int blocks = cdiv(cdiv(npix, 4), 256);
  const float vmax = brighten ? (float)max_value : 255.0f;  // the darkening form clips at 255
  for (int f0 = 0; f0 < n; f0 += g.batch) {
    const int nf = std::min(g.batch, n - f0);
    const int32_t* pl = plan + 4 * (size_t)f0;
    if (int rc = masks_of(pl, nf, mask)) return rc;
    uint8_t* fr = frames + (size_t)f0 * frame_bytes;
    if (aligned)
      darken_apply_kernel<true><<<blocks, 256, 0, s>>>(fr, nf, pl, npix, W, roi, mask, g.f32_b / 4, last, fv, c,
                                                        brighten, vmax);
    else
      darken_apply_kernel<false><<<blocks, 256, 0, s>>>(fr, nf, pl, npix, W, roi, mask, g.f32_b / 4, last, fv, c,
                                                         brighten, vmax);
    if (int rc = check_launch("darken_apply_kernel")) return rc;
  }
  return LS_OK;
}
