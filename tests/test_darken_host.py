"""Host half of the face brightness restore (latentsync_amd/darken.py) and its CPU
restatement (tests/darken_cpu.py): the exact-integer convex hull against a brute-force
inside test, the per-frame plan, the Gaussian taps, known answers of the 8-bit HSV
conversions, an independent float64 yardstick, the option checks of
LipsyncPipeline.__call__, and serve.run_job passing the landmarks file.  No GPU."""
import itertools
import os

import numpy as np
import pytest
import torch

import darken_cpu as dc
from latentsync_amd import darken, serve
from latentsync_amd.pipeline import LipsyncPipeline


def _cross(a, b, p):
    return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])


def _inside_hull(hull, p):
    """The kernels' rule: inside the hull's bounding box and no negative cross product."""
    xs, ys = [q[0] for q in hull], [q[1] for q in hull]
    if not (min(xs) <= p[0] <= max(xs) and min(ys) <= p[1] <= max(ys)):
        return False
    return all(_cross(hull[i], hull[(i + 1) % len(hull)], p) >= 0 for i in range(len(hull)))


def _inside_brute(pts, p):
    """p in conv(pts) by Caratheodory: p is one of the points, on a segment between two of
    them, or in a triangle of three.  Uses no hull."""
    pts = sorted(set(pts))
    if p in pts:
        return True
    for a, b in itertools.combinations(pts, 2):
        if _cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and \
                min(a[1], b[1]) <= p[1] <= max(a[1], b[1]):
            return True
    for a, b, c in itertools.combinations(pts, 3):
        s = [_cross(a, b, p), _cross(b, c, p), _cross(c, a, p)]
        if _cross(a, b, c) != 0 and (all(v >= 0 for v in s) or all(v <= 0 for v in s)):
            return True
    return False


def _point_sets():
    rng = np.random.default_rng(11)
    sets = [[(3, 4)], [(3, 4)] * 5, [(1, 1), (6, 3)], [(0, 0), (2, 2), (4, 4), (6, 6), (2, 2)],  # < 3 points, collinear
            [(5, 1), (5, 7), (5, 3)], [(1, 5), (7, 5), (3, 5), (3, 5)]]
    for n in (3, 4, 5, 7, 9):
        for _ in range(4):
            p = rng.integers(0, 9, (n, 2))
            p = np.concatenate([p, p[: n // 2]])  # duplicates
            sets.append([tuple(int(v) for v in q) for q in p])
    return sets


@pytest.mark.parametrize("k", range(len(_point_sets())))
def test_convex_hull_against_brute_force(k):
    pts = _point_sets()[k]
    hull = darken.convex_hull(np.asarray(pts))
    assert hull and set(hull) <= set(pts) and len(set(hull)) == len(hull)
    if len(hull) >= 3:  # strictly convex, positive orientation
        m = len(hull)
        assert all(_cross(hull[i], hull[(i + 1) % m], hull[(i + 2) % m]) > 0 for i in range(m))
    for p in itertools.product(range(-1, 10), range(-1, 10)):
        assert _inside_hull(hull, p) == _inside_brute(pts, p), (pts, hull, p)


def test_face_hulls_follow_the_definition():
    lm = dc.ellipse_landmarks(1, 478, 0.3, 0.3, 0.2, 0.25, seed=3)[0]
    H, W = 96, 128
    a, b = darken.face_hulls(lm, H, W)
    pts = np.stack([np.trunc(lm[:, 0].astype(np.float64) * W), np.trunc(lm[:, 1].astype(np.float64) * H)], 1)
    pts = pts.astype(np.int32)
    c = np.trunc(pts.mean(0)).astype(np.int32)
    exp = c + np.trunc((pts - c) * 1.2).astype(np.int32)
    exp = np.stack([exp[:, 0].clip(0, W - 1), exp[:, 1].clip(0, H - 1)], 1)
    assert a == darken.convex_hull(exp) and b == darken.convex_hull(pts[dc.BOUNDARY])
    assert len(dc.BOUNDARY) == 17 + 10 + 10 + 4 + 13 and darken.BOUNDARY == dc.BOUNDARY
    # P = 3: only indices 0..2 exist, no more than 3 boundary points -> no hull B
    assert darken.face_hulls(lm[:3], H, W)[1] == []
    assert len(darken.face_hulls(lm[:4], H, W)[1]) >= 1


S, F, B, D, V = darken.MODE_SKIP, darken.MODE_FIRST, darken.MODE_BLEND, darken.MODE_DECAY, darken.MODE_FIRST_VALID


@pytest.mark.parametrize("det,modes,first_valid", [
    ([0, 0, 0, 0], [S, S, S, S], -1),              # none detected
    ([0, 0, 0, 1], [S, S, S, F], -1),              # only frame 3 of 4: frames 0-2 untouched
    ([0, 0, 1, 1, 1, 1, 1], [V, V, F, B, B, B, B], 5),   # frames 0-1 use frame 5's mask x 0.8
    ([1, 1, 0, 0, 1, 0], [F, B, D, D, B, D], 0),   # a gap after detections: the mask decays
    ([0] * 5 + [1], [V] * 5 + [F], 5),
    ([0] * 101 + [1], [S] * 101 + [F], -1),        # only frames 0, 5 .. 95 are searched
])
def test_frame_plan(det, modes, first_valid):
    assert darken.frame_plan([bool(d) for d in det]) == (modes, first_valid)


def test_build_tables_and_roi():
    H, W = 96, 128
    lm = dc.ellipse_landmarks(4, 50, 0.2, 0.25, 0.12, 0.15, missing=(0, 2), seed=1)
    plan, verts, fv, roi = darken.build_tables(lm, H, W, 81)
    assert plan.dtype == np.int32 and plan[:, 0].tolist() == [S, F, D, B] and fv == -1
    assert plan[0, 1:].tolist() == [0, 0, 0] and plan[1, 1] == 0 and plan[3, 1] == plan[1, 2] + plan[1, 3]
    assert verts.shape == (plan[3, 1:].sum(), 2)
    x, y, w, h = roi
    assert x == 0 and y == 0 and x + w <= W and y + h <= H  # the face sits near the corner
    # the region holds everything that is not exactly zero in the restatement's masks
    for i in (1, 3):
        m = dc.face_mask(lm[i], H, W)
        ys, xs = np.nonzero(m)
        assert xs.min() >= x and xs.max() < x + w and ys.min() >= y and ys.max() < y + h
    assert darken.build_tables(np.full((3, 5, 2), np.nan, np.float32), H, W, 81)[3] is None


def test_taps():
    t = darken.gaussian_taps(40)
    i = np.arange(81, dtype=np.float64) - 40
    ref = np.exp(-i * i / (2 * 12.5 ** 2))
    ref /= ref.sum()
    assert t.dtype == np.float32 and t.shape == (81,) and np.array_equal(t, t[::-1])
    assert np.array_equal(t, ref.astype(np.float32)) and np.array_equal(t, dc.taps(40))
    assert abs(t.astype(np.float64).sum() - 1) < 1e-6
    assert darken.gaussian_taps(0).tolist() == [1.0]


def test_hsv_known_answers():
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    h, s, v = dc.rgb_to_hsv(rgb)
    assert h.tolist() == [0, 60, 120] and s.tolist() == [255] * 3 and v.tolist() == [255] * 3
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    assert np.array_equal(dc.hsv_to_rgb(*dc.rgb_to_hsv(grey)), grey)
    # a grey pixel above 235 under f > 1 and mask 0 comes out as 235
    g0 = np.zeros((1, 256), np.float32)
    out = dc.scale_v(grey[None], g0, True)
    assert np.array_equal(out[0, :, 0], np.minimum(np.arange(256), 235)) and (out[..., 0] == out[..., 2]).all()
    rng = np.random.default_rng(5)
    col = rng.integers(0, 256, (400, 1000, 3), dtype=np.uint8)
    h, s, v = dc.rgb_to_hsv(col)
    assert h.min() >= 0 and h.max() <= 179 and s.max() <= 255
    back = dc.hsv_to_rgb(h, s, v)
    assert np.abs(back.astype(int) - col.astype(int)).max() <= 5


@pytest.mark.parametrize("f,bound", [(1.25, 5.175 + 1), (0.8, 5.067 + 1)])
def test_restatement_against_proportional_scaling(f, bound):
    """Scaling V scales R, G and B proportionally, so the restatement must be near
    input * V' / V computed in float64.  Measured maximum deviation over these inputs
    (400 x 1000 seeded random colours, random mask values in [0, 1]): 5.175 levels at
    f = 1.25 and 5.067 at f = 0.8 -- the cost of 2-degree hue steps and 8-bit S.  The bound
    is that maximum plus 1 level for rounding."""
    rng = np.random.default_rng(17)
    col = rng.integers(0, 256, (400, 1000, 3), dtype=np.uint8)
    m = rng.uniform(0, 1, (400, 1000)).astype(np.float32)
    brighten = f > 1
    c = np.float32(f - 1.0) if brighten else np.float32(1.0 - f)
    got = dc.scale_v(col, m * c, brighten).astype(np.float64)
    v = col.max(axis=-1).astype(np.float64)
    g = m.astype(np.float64) * float(c)
    v2 = np.floor(np.clip(v * (1 + g), 0, 235)) if brighten else np.floor(np.clip(v * (1 - g), 0, 255))
    want = col.astype(np.float64) * np.where(v > 0, v2 / np.maximum(v, 1), 0)[..., None]
    dev = np.abs(got - want).max()
    print(f"f = {f}: maximum deviation from proportional scaling {dev:.3f} levels")
    assert dev <= bound


def test_restatement_schedule_passthrough():
    """Frames the schedule does not process are bit-identical; processed ones are not."""
    fr = dc.noise_gradient_frames(4, 40, 48, 2)
    lm = dc.ellipse_landmarks(4, 30, 0.5, 0.5, 0.2, 0.2, missing=(0, 1, 2), seed=2)
    out = dc.enhance_face_brightness(fr, lm, 1.25, feather=4)
    assert np.array_equal(out[:3], fr[:3]) and (out[3] != fr[3]).any()
    assert np.array_equal(dc.enhance_face_brightness(fr, np.full_like(lm, np.nan), 1.25, feather=4), fr)


# ---------------------------------------------------------------- __call__ option checks

CALL = dict(video_path="v.npy", audio_path="a.wav", video_out_path="o.npz")
LM = np.zeros((4, 5, 2), np.float32)


def test_call_with_landmarks_passes_the_option_check(tmp_path):
    pipe = LipsyncPipeline.__new__(LipsyncPipeline)
    with pytest.raises(FileNotFoundError):
        pipe(data_path=str(tmp_path / "d.pth"), use_darken=True, brightness_factor=1.25, face_landmarks=LM, **CALL)
    np.save(tmp_path / "lm.npy", LM)
    with pytest.raises(FileNotFoundError):
        pipe(data_path=str(tmp_path / "d.pth"), use_darken=True, brightness_factor=1.25,
             face_landmarks=str(tmp_path / "lm.npy"), **CALL)
    with pytest.raises(NotImplementedError, match="face_landmarks"):
        pipe(data_path=str(tmp_path / "d.pth"), use_darken=True, brightness_factor=1.25, **CALL)


def test_call_refuses_darken_with_faces_only(tmp_path):
    pipe = LipsyncPipeline.__new__(LipsyncPipeline)
    with pytest.raises(ValueError, match="faces_only"):
        pipe(data_path=str(tmp_path / "d.pth"), use_darken=True, brightness_factor=1.25, face_landmarks=LM,
             faces_only=True, **CALL)


def _partly_nan():
    lm = LM.copy()
    lm[1, 2, 0] = np.nan
    return lm


@pytest.mark.parametrize("bad", [LM.astype(np.float64), LM[0], LM[:, :, :1], np.zeros((4, 0, 2), np.float32),
                                 _partly_nan(), torch.zeros((4, 5, 2), dtype=torch.float16)])
def test_call_refuses_malformed_landmarks(bad, tmp_path):
    pipe = LipsyncPipeline.__new__(LipsyncPipeline)
    with pytest.raises(ValueError, match="face_landmarks"):
        pipe(data_path=str(tmp_path / "d.pth"), use_darken=True, brightness_factor=1.25, face_landmarks=bad, **CALL)


def test_landmark_count_must_match_the_faces(tmp_path):
    """Checked after data.pth is read and before anything else is."""
    pipe = LipsyncPipeline.__new__(LipsyncPipeline)
    torch.save({"faces": torch.zeros((3, 3, 8, 8), dtype=torch.uint8), "boxes": [[0, 0, 8, 8]] * 3,
                "affine_matrices": [np.eye(2, 3)] * 3}, tmp_path / "d.pth")
    with pytest.raises(ValueError, match="4 landmark rows for 3 faces"):
        pipe(data_path=str(tmp_path / "d.pth"), use_darken=True, brightness_factor=1.25, face_landmarks=LM, **CALL)


# ---------------------------------------------------------------- serve


class StubPipeline:
    """Records each call and writes an output file, as the real __call__ does."""

    def __init__(self):
        self.calls = []

    def __call__(self, **kw):
        self.calls.append(kw)
        open(kw["video_out_path"], "wb").close()


@pytest.mark.parametrize("with_file", [False, True])
def test_run_job_passes_the_landmarks_file_iff_it_exists(tmp_path, with_file):
    data, results = tmp_path / "data", tmp_path / "results"
    data.mkdir()
    for name in ("vid_darken.mp4", "vid_darken.pth", "vid.mp4", "vid.pth", "req.wav"):
        (data / name).write_bytes(b"x")
    if with_file:
        np.save(data / "vid_darken.landmarks.npy", LM)
    (data / "vid.landmarks.npy").write_bytes(b"x")  # belongs to the plain clip: never passed
    pipe = StubPipeline()
    payload = dict(id="req", video_id="vid", audio_url="unused", use_darken=True, brightness_factor=0.8)
    serve.run_job(pipe, payload, str(data), str(results), 256)
    kw = pipe.calls[0]
    assert kw["use_darken"] is True and kw["brightness_factor"] == 1.25
    assert kw["data_path"] == str(data / "vid_darken.pth")
    if with_file:
        assert kw["face_landmarks"] == str(data / "vid_darken.landmarks.npy")
    else:
        assert "face_landmarks" not in kw
    serve.run_job(pipe, dict(payload, use_darken=False), str(data), str(results), 256)
    assert "face_landmarks" not in pipe.calls[1] and os.path.exists(pipe.calls[1]["video_out_path"])
