"""CPU restatement of the face brightness restore: numpy, float32
wherever the reference (latentsync/utils/darken_restore.py) is float32, whole frames (no
region of interest), one frame after the other as the reference loops.  cv2 is not
installed, so its steps (fillConvexPoly, dilate, GaussianBlur, the 8-bit HSV conversions)
are restated here; the device kernels must equal this file bit for bit.

Only the convex hull is shared with the package (latentsync_amd.darken.convex_hull, pinned
against a brute-force test in tests/test_darken_host.py)."""
import numpy as np

from latentsync_amd.darken import convex_hull

BOUNDARY = [*range(0, 17), *range(100, 110), *range(127, 137), 46, 55, 276, 285, *range(10, 108, 8)]
F32 = np.float32


def taps(feather=40):
    k = 2 * feather + 1
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    i = np.arange(k, dtype=np.float64) - feather
    t = np.exp(-(i * i) / (2 * sigma * sigma))
    return (t / t.sum()).astype(F32)


def fill_hull(mask, hull):
    """Set every integer pixel inside or on the boundary of the hull (int64 cross products)."""
    H, W = mask.shape
    if not hull:
        return
    hx = np.array([p[0] for p in hull], np.int64)
    hy = np.array([p[1] for p in hull], np.int64)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    ok = (xs >= hx.min()) & (xs <= hx.max()) & (ys >= hy.min()) & (ys <= hy.max())
    for i in range(len(hull)):
        j = (i + 1) % len(hull)
        ok &= (hx[j] - hx[i]) * (ys - hy[i]) - (hy[j] - hy[i]) * (xs - hx[i]) >= 0
    mask[ok] = 1


def dilate(mask, k):
    H, W = mask.shape
    a = k // 2
    out = np.zeros_like(mask)
    for dy in range(-a, k - a):
        for dx in range(-a, k - a):
            ys0, ys1 = max(0, -dy), min(H, H - dy)  # destination rows whose source y + dy is in the frame
            xs0, xs1 = max(0, -dx), min(W, W - dx)
            if ys0 < ys1 and xs0 < xs1:
                np.maximum(out[ys0:ys1, xs0:xs1], mask[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx],
                           out=out[ys0:ys1, xs0:xs1])
    return out


def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = p.copy()
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def blur_axis(x, t, axis):
    """acc = 0; for j: acc = acc + t[j] * x[reflect(i + j - r)]: float32 products and sums."""
    n, r = x.shape[axis], len(t) // 2
    acc = np.zeros_like(x, dtype=F32)
    for j in range(len(t)):
        idx = reflect101(np.arange(n) + j - r, n)
        acc = acc + t[j] * np.take(x, idx, axis=axis)
        assert acc.dtype == F32
    return acc


def face_mask(row, H, W, feather=40):
    """create_natural_face_mask (darken_restore.py:8-96) with expansion_factor 1.2."""
    x = np.trunc(row[:, 0].astype(np.float64) * W)
    y = np.trunc(row[:, 1].astype(np.float64) * H)
    pts = np.stack([x, y], axis=1).astype(np.int32)
    centre = np.trunc(pts.mean(axis=0)).astype(np.int32)
    exp = centre + np.trunc((pts - centre) * 1.2).astype(np.int32)
    exp[:, 0] = np.clip(exp[:, 0], 0, W - 1)
    exp[:, 1] = np.clip(exp[:, 1], 0, H - 1)
    mask = np.zeros((H, W), np.uint8)
    fill_hull(mask, convex_hull(exp))
    b = [pts[i] for i in BOUNDARY if i < len(pts)]
    if len(b) > 3:
        fill_hull(mask, convex_hull(b))
    mask = dilate(mask, max(1, int(min(W, H) * 0.01)))
    m = mask.astype(F32)
    if feather > 0:
        t = taps(feather)
        m = blur_axis(blur_axis(m, t, 1), t, 0)
    return m


SDIV = np.array([0] + [int(np.rint((255 << 12) / i)) for i in range(1, 256)], np.int32)
HDIV = np.array([0] + [int(np.rint((180 << 12) / (6.0 * i))) for i in range(1, 256)], np.int32)


def rgb_to_hsv(rgb):
    """OpenCV's scalar RGB2HSV_b, hue range 180: uint8 (..., 3) -> int32 h, s, v."""
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = (d * SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * HDIV[d] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv_to_rgb(h, s, v):
    """OpenCV's scalar HSV2RGB_b in float32: int h, s, v -> uint8 (..., 3)."""
    hh = h.astype(F32) * (F32(6) / F32(180))
    ss = s.astype(F32) * (F32(1) / F32(255))
    vv = v.astype(F32) * (F32(1) / F32(255))
    sec = np.floor(hh)
    fr = hh - sec
    one = F32(1)
    t0, t1, t2, t3 = vv, vv * (one - ss), vv * (one - ss * fr), vv * (one - ss * (one - fr))
    order = [(t1, t3, t0), (t1, t0, t2), (t3, t0, t1), (t0, t2, t1), (t0, t1, t3), (t2, t1, t0)]  # (b, g, r)
    k = sec.astype(np.int32)
    out = np.empty(h.shape + (3,), F32)
    for ch, pos in ((2, 0), (1, 1), (0, 2)):  # order[k][ch] -> RGB position
        out[..., pos] = np.choose(k, [o[ch] for o in order])
    grey = s == 0
    out[grey] = vv[grey][..., None]
    assert out.dtype == F32
    return np.clip(np.rint(out * F32(255)), 0, 255).astype(np.uint8)


def scale_v(frame, g, brighten, max_value=235):
    """The HSV round trip of one RGB frame with V' = clip(V (1 +- g), 0, max), truncated."""
    h, s, v = rgb_to_hsv(frame)
    vf = v.astype(F32)
    if brighten:
        v2 = np.clip(vf * (F32(1) + g), 0, max_value)
    else:
        v2 = np.clip(vf * (F32(1) - g), 0, 255)
    assert v2.dtype == F32
    return hsv_to_rgb(h, s, v2.astype(np.uint8).astype(np.int32))


def enhance_face_brightness(frames, landmarks, brightness_factor, feather=40, max_value=235):
    """darken_restore.py:150-317 on uint8 RGB frames (N, H, W, 3) -> a new array."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    out = frames.copy()
    det = [not np.isnan(landmarks[i]).all() for i in range(n)]
    f = float(brightness_factor)
    brighten = f > 1.0
    c = F32(f - 1.0) if brighten else F32(1.0 - f)
    first_valid = None
    for i in range(0, min(100, n + 1), 5):
        if i < n and det[i]:
            first_valid = face_mask(landmarks[i], H, W, feather)
            break
    last = None
    for i in range(n):
        cur = None
        if det[i]:
            cur = face_mask(landmarks[i], H, W, feather)
            if last is not None:
                cur = F32(0.7) * last + F32(0.3) * cur
            last = cur.copy()
        elif last is not None:
            cur = last.copy()
            last = last * F32(0.8)
        if cur is not None:
            g = cur * c
        elif first_valid is not None:
            g = (first_valid * c) * F32(0.8)
        else:
            continue
        assert g.dtype == F32
        out[i] = scale_v(frames[i], g, brighten, max_value)
    return out


# ---------------------------------------------------------------- test inputs


def noise_gradient_frames(n, H, W, seed):
    """Seeded noise on a colour gradient: every hue sector, greys and bright pixels."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    base = np.stack([xs * 255.0 / max(W - 1, 1), ys * 255.0 / max(H - 1, 1),
                     255.0 - (xs + ys) * 255.0 / max(W + H - 2, 1)], axis=-1)
    fr = base[None] + rng.normal(0, 40, (n, H, W, 3))
    fr = np.clip(fr, 0, 255).astype(np.uint8)
    fr[:, : H // 8, : W // 8] = fr[:, : H // 8, : W // 8, :1]  # a grey patch
    return fr


def ellipse_landmarks(n, P, cx, cy, rx, ry, missing=(), seed=0, drift=(0.01, 0.006)):
    """P points on a jittered ellipse (normalised coordinates) that drifts a few pixels a
    frame; frames in ``missing`` are all NaN."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, 2 * np.pi, P)
    rad = rng.uniform(0.2, 1.0, P)
    lm = np.empty((n, P, 2), F32)
    for i in range(n):
        jit = rng.normal(0, 0.004, (P, 2))
        lm[i, :, 0] = cx + drift[0] * i + rad * rx * np.cos(t) + jit[:, 0]
        lm[i, :, 1] = cy + drift[1] * i + rad * ry * np.sin(t) + jit[:, 1]
    for i in missing:
        lm[i] = np.nan
    return lm
