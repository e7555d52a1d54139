"""Face brightness restore of ``use_darken`` requests: the host half.

The reference darkens the clip before lip-sync and, after paste-back, write_video runs
``enhance_face_brightness`` over every output frame (latentsync/utils/util.py:150-151,
latentsync/utils/darken_restore.py:99-376): a PNG round trip through the disk per frame
and cv2 on the host.  Here the restored frames are already on the device and stay there
(csrc/ls_darken.hip, ops.face_brighten).  This module turns the landmarks into what the
kernels need -- convex hulls, a per-frame plan, the Gaussian taps and one region of
interest -- all of it tiny (at most 478 points a frame) and in exact integers.

Landmarks are this module's input, as in align.py: the FaceMesh model is not carried.
They are float32 (N, P, 2), FaceMesh's normalised (x, y) as fractions of width and height;
a frame without a face is a row of NaN.  DESIGN.md section 4.4 is the definition of the
arithmetic; the cv2 steps are restated there and their parity is unpinned.
"""
import numpy as np

EXPANSION = 1.2
MODE_SKIP, MODE_FIRST, MODE_BLEND, MODE_DECAY, MODE_FIRST_VALID = 0, 1, 2, 3, 4
# darken_restore.py:57-66: jawline, ears, eyebrow ends, forehead samples
BOUNDARY = [*range(0, 17), *range(100, 110), *range(127, 137), 46, 55, 276, 285, *range(10, 108, 8)]
_COORD_LIMIT = 1 << 30  # the kernels' cross products stay inside int64


def load_landmarks(landmarks):
    """A path to a .npy, an array or a tensor -> float32 (N, P, 2) numpy.  ValueError for a
    wrong rank or dtype, P < 1, infinities, or a row that is only partly NaN."""
    if isinstance(landmarks, (str, bytes)) or hasattr(landmarks, "__fspath__"):
        landmarks = np.load(landmarks, allow_pickle=False)
    if hasattr(landmarks, "detach"):
        landmarks = landmarks.detach().cpu().numpy()
    lm = np.asarray(landmarks)
    if lm.dtype != np.float32 or lm.ndim != 3 or lm.shape[2] != 2 or lm.shape[1] < 1:
        raise ValueError(f"face_landmarks: float32 (N, P, 2) with P >= 1 expected, got {lm.dtype} {lm.shape}")
    nan = np.isnan(lm).reshape(lm.shape[0], -1)
    if (nan.any(axis=1) & ~nan.all(axis=1)).any():
        raise ValueError("face_landmarks: a frame's row is partly NaN (a frame without a face is all NaN)")
    if np.isinf(lm).any():
        raise ValueError("face_landmarks: infinite coordinates")
    return lm


def detected(landmarks):
    """Per frame: does it carry landmarks (a row that is not NaN)?"""
    return ~np.isnan(landmarks).reshape(landmarks.shape[0], -1).all(axis=1)


def convex_hull(points):
    """Andrew's monotone chain in exact integers: the strictly convex hull of integer
    points (n, 2) as a list of (x, y), ordered so that cross(b - a, p - a) >= 0 for
    consecutive vertices a, b and every inside point p.  Duplicates and collinear points are
    dropped: identical points give one vertex, collinear ones the two ends."""
    pts = sorted({(int(x), int(y)) for x, y in points})
    if len(pts) <= 2:
        return pts

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and ((h[-1][0] - h[-2][0]) * (p[1] - h[-2][1])
                                   - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0])) <= 0:
                h.pop()
            h.append(p)
        return h

    lower, upper = half(pts), half(reversed(pts))
    return lower[:-1] + upper[:-1]


def face_hulls(row, H, W):
    """darken_restore.py:22-81 for one frame's landmarks (P, 2): (hull A, hull B).  A is the
    hull of the points expanded by 1.2 about their centre and clipped to the frame, B the
    hull of the unexpanded boundary points (empty unless more than 3 of them exist)."""
    row = np.asarray(row, np.float64)
    pts = np.stack([np.trunc(row[:, 0] * W), np.trunc(row[:, 1] * H)], axis=1)
    if np.abs(pts).max() >= _COORD_LIMIT:
        raise ValueError("face_landmarks: coordinates beyond 2^30 pixels")
    pts = pts.astype(np.int32)
    centre = np.trunc(pts.mean(axis=0)).astype(np.int32)
    exp = centre + np.trunc((pts - centre) * EXPANSION).astype(np.int32)
    exp[:, 0] = np.clip(exp[:, 0], 0, W - 1)
    exp[:, 1] = np.clip(exp[:, 1], 0, H - 1)
    b = [pts[i] for i in BOUNDARY if i < len(pts)]
    return convex_hull(exp), (convex_hull(b) if len(b) > 3 else [])


def frame_plan(det):
    """darken_restore.py:150-317 as one mode per frame: (modes, first_valid).  first_valid is
    the first frame with landmarks among range(0, min(100, n + 1), 5) -- possibly later than
    the frames it serves -- or -1."""
    n = len(det)
    first_valid = next((i for i in range(0, min(100, n + 1), 5) if i < n and det[i]), -1)
    modes, have_last = [], False
    for d in det:
        if d:
            modes.append(MODE_BLEND if have_last else MODE_FIRST)
            have_last = True
        elif have_last:
            modes.append(MODE_DECAY)
        else:
            modes.append(MODE_FIRST_VALID if first_valid >= 0 else MODE_SKIP)
    return modes, first_valid


def gaussian_taps(feather_amount):
    """cv2.getGaussianKernel(2 f + 1, 0) in float32: sigma = 0.3 ((k - 1) 0.5 - 1) + 0.8, the
    taps normalised in float64 and then cast.  feather_amount 0 (no blur) is the one tap 1."""
    k = 2 * int(feather_amount) + 1
    if k == 1:
        return np.ones(1, np.float32)
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    i = np.arange(k, dtype=np.float64) - (k - 1) // 2
    t = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


def dilate_size(H, W):
    return max(1, int(min(W, H) * 0.01))


def gain_constant(brightness_factor):
    """(c, brighten): V' = clip(V (1 + g), 0, max_value) for f > 1, else clip(V (1 - g), 0, 255),
    g = mask c.  f = 1.0 is the reference's "no change" mode and still takes the second form."""
    f = float(brightness_factor)
    return (np.float32(f - 1.0), True) if f > 1.0 else (np.float32(1.0 - f), False)


def build_tables(landmarks, H, W, n_taps):
    """(plan int32 (N, 4), verts int32 (V, 2), first_valid, roi (x, y, w, h) or None).  roi is
    None when no frame has landmarks: then nothing is processed."""
    det = detected(landmarks)
    modes, first_valid = frame_plan(det)
    plan = np.zeros((len(det), 4), np.int32)
    plan[:, 0] = modes
    verts = []
    for i in np.flatnonzero(det):
        a, b = face_hulls(landmarks[i], H, W)
        plan[i, 1:] = len(verts), len(a), len(b)
        verts += a + b
    if not verts:
        return plan, np.zeros((1, 2), np.int32), -1, None
    verts = np.asarray(verts, np.int32).reshape(-1, 2)
    grow = dilate_size(H, W) + n_taps // 2
    # hull A is clipped into the frame, so the box meets the frame; hull B may leave it
    x0 = max(0, min(int(verts[:, 0].min()), W - 1) - grow)
    y0 = max(0, min(int(verts[:, 1].min()), H - 1) - grow)
    x1 = min(W - 1, max(int(verts[:, 0].max()), 0) + grow)
    y1 = min(H - 1, max(int(verts[:, 1].max()), 0) + grow)
    return plan, verts, first_valid, (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def enhance_face_brightness(frames_dev_u8, landmarks, brightness_factor, feather_amount=40, max_value=235,
                            frames_per_batch=0):
    """darken_restore.enhance_face_brightness on uint8 RGB frames (N, H, W, 3) on the device,
    in place; returns the tensor.  ``landmarks``: see load_landmarks, one row per frame.
    ``frames_per_batch`` bounds the frames whose masks are held at once (0: a fixed budget)."""
    import torch

    from . import ops
    fr = frames_dev_u8
    if not isinstance(fr, torch.Tensor) or fr.dtype != torch.uint8 or fr.dim() != 4 or fr.shape[-1] != 3:
        raise ValueError("enhance_face_brightness: uint8 (N, H, W, 3) frames expected, got "
                         f"{getattr(fr, 'dtype', type(fr))} {tuple(getattr(fr, 'shape', ()))}")
    lm = load_landmarks(landmarks)
    n, H, W, _ = fr.shape
    if lm.shape[0] != n:
        raise ValueError(f"enhance_face_brightness: {lm.shape[0]} landmark rows for {n} frames")
    taps = gaussian_taps(feather_amount)
    plan, verts, first_valid, roi = build_tables(lm, H, W, len(taps))
    if roi is None:
        return fr  # no face anywhere: every frame stays bit-identical
    c, brighten = gain_constant(brightness_factor)
    return ops.face_brighten(fr, plan, verts, first_valid, roi, taps, dilate_size(H, W), float(c), brighten,
                             int(max_value), frames_per_batch=frames_per_batch)
