"""The project's own restatement of the S3FD detector (eval/detectors/s3fd of the reference), for
the tests.

  * resize_fx_u8 / prep: cv2.resize(image, (0, 0), fx=s, fy=s, INTER_LINEAR) for uint8 from
    OpenCV's published definition (destination cvRound(size s), source step 1 / s, 11-bit
    fixed-point coefficients, two rounding passes) and detect_faces' mean subtraction.  cv2 is
    not a dependency: parity with it is unpinned.
  * forward(sd, x, bf16=False): S3FDNet's trunk and heads in fp32 torch on the CPU from a
    reference-named state dict.  bf16=True rounds every weight to bf16 once and rounds to bf16
    wherever the device path stores bf16 (the input, every ReLU output, the L2Norm outputs); the
    head maps stay fp32, so only the accumulation order differs from the device.
  * detect_ref / nms_ref: the tail of S3FDNet.forward, Detect.forward and detect_faces' nms_ in
    float64 numpy on fp32 inputs, with the margins the exact tests rest on: the distance of the
    closest score to its threshold and of the closest compared IoU to its threshold.
  * the seeded weights, frames, synthetic head maps and tracker cases.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from latentsync_amd import s3fd

WORK_HW = (304, 432)      # the working frame; at scale 0.25 a 76 x 108 network input, 697 priors
WORK_SCALE = 0.25
BIG_INPUT = (192, 336)    # the network input whose 5373 priors all become candidates
SUBSAMPLE = 3072          # stage outputs above 2 * SUBSAMPLE elements are stored at SUBSAMPLE fixed positions
NET_SEED, FRAME_SEED = 31, 32
N_RELU = 19               # 13 trunk convs, fc6, fc7, four extras
MARGIN_SCORE, MARGIN_IOU = 1e-4, 1e-4


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def subsample_index(numel, seed):
    if numel <= 2 * SUBSAMPLE:
        return None
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(numel, generator=g)[:SUBSAMPLE].sort().values


# ---------------------------------------------------------------- seeded weights and frames
# gain on top of He's sqrt(2 / fan_in): conv1_1 sees mean-subtracted pixels (RMS about 40 after
# the 4-to-1 resize of uniform noise), every conv behind a max-pool sees the maximum of four,
# and on the working size's smallest maps most taps of fc6 and of the stride-2 extras are padding
_GAIN = {0: 1.0 / 32.0, 5: 0.7, 10: 0.7, 17: 0.7, 24: 0.7, 31: 2.0}
_GAIN_EXTRAS = {1: 1.5, 3: 2.0}


def case_weights(seed=NET_SEED):
    """The seeded state dict: conv weights N(0, 2 / fan_in) times _GAIN, biases 0.1 N(0, 1) (0.02
    in the heads), L2Norm weights (10, 8, 5) (1 + 0.1 N(0, 1)).  The head weights are N(0, 1 /
    fan_in): logits of order one."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {}
    l2 = {"L2Norm3_3.weight": 10.0, "L2Norm4_3.weight": 8.0, "L2Norm5_3.weight": 5.0}
    for k, s in s3fd.param_shapes().items():
        if k in l2:
            sd[k] = l2[k] * (1.0 + 0.1 * rn(*s))
        elif k.endswith(".weight"):
            fan_in = int(np.prod(s[1:]))
            mod, idx = k.split(".")[:2]
            if mod in ("loc", "conf"):
                sd[k] = rn(*s) * math.sqrt(1.0 / fan_in)
            else:
                sd[k] = rn(*s) * math.sqrt(2.0 / fan_in) * (_GAIN if mod == "vgg" else _GAIN_EXTRAS).get(int(idx), 1.0)
        else:
            sd[k] = (0.02 if k.startswith(("loc", "conf")) else 0.1) * rn(*s)
    return sd


def case_frames(n=2, hw=WORK_HW, seed=FRAME_SEED):
    """uint8 (n, H, W, 3) RGB, uniform random."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, hw[0], hw[1], 3), generator=g, dtype=torch.uint8)


# ---------------------------------------------------------------- cv2.resize(fx, fy), prep
def cv_round(v):
    """cvRound: to nearest, halves to even."""
    return int(np.rint(v))


def _fx_table(dst, src, scale, horizontal):
    idx = np.zeros(dst, np.int64)
    w = np.zeros((dst, 2), np.int64)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if horizontal:
            if s < 0:
                f, s = np.float32(0), 0
            if s >= src - 1:
                f, s = np.float32(0), src - 1
        idx[d] = s
        w[d] = (int(np.rint(np.float32((np.float32(1) - f) * np.float32(2048)))), int(np.rint(np.float32(f * np.float32(2048)))))
    return idx, w


def resize_fx_u8(img, s):
    """cv2.resize(img, (0, 0), fx=s, fy=s, interpolation=INTER_LINEAR) for uint8 (H, W, C), s in
    (0, 1] and not 0.5 (cv2's 2 x 2 area path, which the project refuses)."""
    img = np.asarray(img)
    assert 0.0 < s <= 1.0 and s != 0.5
    H, W = img.shape[:2]
    dh, dw = cv_round(H * s), cv_round(W * s)
    scale = 1.0 / s
    v = img.astype(np.int64)
    xi, xw = _fx_table(dw, W, scale, True)
    yi, yw = _fx_table(dh, H, scale, False)
    x1 = np.minimum(xi + 1, W - 1)
    rows = v[:, xi] * xw[:, 0][None, :, None] + v[:, x1] * xw[:, 1][None, :, None]
    y0, y1 = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
    out = (((yw[:, 0][:, None, None] * (rows[y0] >> 4)) >> 16) + ((yw[:, 1][:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def prep(frames, s):
    """detect_faces lines 35-42 per frame: uint8 (n, H, W, 3) RGB -> fp32 (n, 3, h, w): the resized
    frame minus the means; channel order R, G, B (the two [2, 1, 0] swaps cancel)."""
    mean = np.array([123.0, 117.0, 104.0], dtype=np.float32)
    out = [resize_fx_u8(f, s).astype(np.float32) - mean for f in np.asarray(frames)]
    return torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------- the network
@torch.no_grad()
def forward(sd, x, bf16=False):
    """x fp32 (n, 3, h, w) -> dict(relu=[19 NCHW], l2norm=[3 NCHW], heads=[6 x (n, h_l, w_l, 8 | 6)
    loc | conf])."""
    r = bf16_round if bf16 else (lambda t: t)
    w = lambda k: r(sd[k + ".weight"].float())
    b = lambda k: sd[k + ".bias"].float()
    relu, l2, sources = [], [], []
    h = r(x.float())
    for s in s3fd._VGG:
        if s == "P":
            h = F.max_pool2d(h, 2, 2)
        elif s == "C":
            h = F.max_pool2d(h, 2, 2, ceil_mode=True)
        else:
            i, _, _, dil = s
            h = r(F.relu(F.conv2d(h, w(f"vgg.{i}"), b(f"vgg.{i}"), padding=dil, dilation=dil)))
            relu.append(h)
            if i in s3fd._L2NORM:
                norm = h.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10
                l2.append(r(sd[s3fd._L2NORM[i][0] + ".weight"].float()[None, :, None, None] * (h / norm)))
                sources.append(l2[-1])
    h = r(F.relu(F.conv2d(h, w("vgg.33"), b("vgg.33"))))
    relu.append(h)
    sources.append(h)
    for i, (_, _, k) in enumerate(s3fd._EXTRAS):
        h = r(F.relu(F.conv2d(h, w(f"extras.{i}"), b(f"extras.{i}"), stride=2 if k == 3 else 1, padding=1 if k == 3 else 0)))
        relu.append(h)
        if i % 2 == 1:
            sources.append(h)
    heads = []
    for i, src in enumerate(sources):
        loc = F.conv2d(src, w(f"loc.{i}"), b(f"loc.{i}"), padding=1)
        conf = F.conv2d(src, w(f"conf.{i}"), b(f"conf.{i}"), padding=1)
        heads.append(torch.cat([loc, conf], 1).permute(0, 2, 3, 1).contiguous())
    return dict(relu=relu, l2norm=l2, heads=heads)


# ---------------------------------------------------------------- post-processing, float64
def _greedy(boxes, order, thresh, union_first):
    """Greedy NMS over `order` (descending score).  -> (keep, margin): the smallest |IoU -
    thresh| over every comparison made."""
    x1, y1, x2, y2 = boxes.T
    area = (x2 - x1) * (y2 - y1)
    keep, margin = [], np.inf
    order = np.asarray(order)
    while order.size:
        i = order[0]
        keep.append(int(i))
        rest = order[1:]
        if not rest.size:
            break
        w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]))
        h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]))
        inter = w * h
        iou = inter / ((area[rest] - inter) + area[i] if union_first else (area[i] + area[rest] - inter))
        margin = min(margin, float(np.abs(iou - thresh).min()))
        order = rest[iou <= thresh]
    return keep, margin


def detect_ref(heads, priors, frame=0):
    """The tail of S3FDNet.forward + Detect.forward for one frame in float64 on the fp32 head
    maps: -> dict(idx (k,) prior indices of the kept boxes in order, k <= 750; scores; boxes (k,
    4); n_cand; score_margin; iou_margin)."""
    loc, conf = [], []
    for l, m in enumerate(heads):
        m = np.asarray(m[frame], dtype=np.float64).reshape(-1, m.shape[-1])
        loc.append(m[:, :4])
        c = m[:, 4:]
        conf.append(np.stack([c[:, :3].max(1), c[:, 3]], 1) if l == 0 else c)
    loc, conf = np.concatenate(loc), np.concatenate(conf)
    pr = np.asarray(priors, dtype=np.float64)
    assert pr.shape == loc.shape, (pr.shape, loc.shape)
    e = np.exp(conf - conf.max(1, keepdims=True))
    score = e[:, 1] / e.sum(1)
    cxy = pr[:, :2] + loc[:, :2] * 0.1 * pr[:, 2:]
    wh = pr[:, 2:] * np.exp(loc[:, 2:] * 0.2)
    x1y1 = cxy - wh / 2
    boxes = np.concatenate([x1y1, wh + x1y1], 1)
    cand = np.nonzero(score > 0.05)[0]
    order = cand[np.argsort(-score[cand], kind="stable")][:5000]
    keep, iou_margin = _greedy(boxes, order, 0.3, True)
    keep = np.asarray(keep[:750], dtype=np.int64)
    return dict(idx=keep, scores=score[keep], boxes=boxes[keep].reshape(-1, 4), n_cand=int(cand.size),
                score_margin=float(np.abs(score - 0.05).min()), iou_margin=iou_margin,
                score_gap=float(np.diff(np.sort(score)).min()) if score.size > 1 else np.inf)


def nms_ref(det, conf_th, frame_w, frame_h, thresh=0.1):
    """detect_faces lines 46-59 for one frame: det (R, 5) fp32 = score, x1, y1, x2, y2 -> dict(idx:
    nms_'s keep (indices into the rows above conf_th), boxes (k, 5) = x1, y1, x2, y2, score,
    score_margin, iou_margin).  The products with (w, h, w, h) are fp32, as torch's are."""
    det = np.asarray(det, dtype=np.float32)
    sel = np.nonzero(det[:, 0] > np.float32(conf_th))[0]
    scale = np.array([frame_w, frame_h, frame_w, frame_h], dtype=np.float32)
    b = (det[sel, 1:] * scale).astype(np.float64)
    sc = det[sel, 0].astype(np.float64)
    nz = det[:, 0][det[:, 0] > 0]
    order = np.argsort(-sc, kind="stable")
    keep, margin = _greedy(b, order, thresh, False)
    keep = np.asarray(keep, dtype=np.int64)
    return dict(idx=keep, boxes=np.concatenate([b[keep].reshape(-1, 4), sc[keep].reshape(-1, 1)], 1),
                score_margin=float(np.abs(nz.astype(np.float64) - conf_th).min()) if nz.size else np.inf,
                iou_margin=margin)


# ---------------------------------------------------------------- synthetic head maps
def synthetic_heads(seed, sizes, n=1, lo=0.001, hi=0.999, loc_scale=1.0):
    """Seeded fp32 head maps (n, h_l, w_l, 8 | 6) whose face probabilities are a permutation of
    an evenly spaced grid in [lo, hi] (no two closer than (hi - lo) / P), the logits from its
    inverse; level 0 gets three distinct background logits of which the largest is the real
    one; the loc channels are loc_scale N(0, 1)."""
    rng = np.random.RandomState(seed)
    P = sum(h * w for h, w in sizes)
    maps = [np.zeros((n, h, w, 8 if l == 0 else 6), dtype=np.float32) for l, (h, w) in enumerate(sizes)]
    for f in range(n):
        p = np.linspace(lo, hi, P)[rng.permutation(P)]
        _fill_heads(maps, f, sizes, loc_scale * rng.randn(P, 4), np.log(p / (1.0 - p)), rng)
    return [torch.from_numpy(m) for m in maps]


def _fill_heads(maps, f, sizes, loc, logit, rng):
    off = 0
    for l, (h, w) in enumerate(sizes):
        m = maps[l][f].reshape(h * w, -1)
        k = h * w
        m[:, :4] = loc[off:off + k]
        lg = logit[off:off + k]
        bg = rng.randn(k)
        if l == 0:
            below = np.abs(rng.randn(k, 2)) + 0.5
            trio = np.stack([bg, bg - below[:, 0], bg - below[:, 1]], 1)
            for q in range(k):
                trio[q] = trio[q][rng.permutation(3)]
            m[:, 4:7] = trio
            m[:, 7] = bg + lg
        else:
            m[:, 4] = bg
            m[:, 5] = bg + lg
        off += k


CLUSTER_CELL, CLUSTER_BOX, CLUSTER_FORCED = 16, 12.0, 3


def clustered_heads(seed, hw, lo=0.06, hi=0.999):
    """Head maps for the top-5000 cut on an h x w input (one frame): every prior's loc decodes to
    a CLUSTER_BOX-pixel box about the centre of the CLUSTER_CELL-pixel cell its own centre lies
    in, jittered by up to 0.3 pixels and 2 % in size, so boxes of one cell overlap almost fully
    and boxes of different cells not at all: far fewer than 750 boxes survive the NMS.  The
    probabilities are a seeded permutation of the evenly spaced grid in [lo, hi], chosen so that
    CLUSTER_FORCED whole cells hold only probabilities from the lowest P - 5000: with the exact
    cut those cells yield no box, without it one each."""
    rng = np.random.RandomState(seed)
    h, w = hw
    sizes = s3fd.feature_map_sizes(h, w)
    pr = s3fd.prior_boxes(h, w, sizes).astype(np.float64)
    P = pr.shape[0]
    assert P > 5000
    cell = (np.floor(pr[:, 1] * h / CLUSTER_CELL).clip(0, h // CLUSTER_CELL - 1).astype(np.int64) * (w // CLUSTER_CELL) +
            np.floor(pr[:, 0] * w / CLUSTER_CELL).clip(0, w // CLUSTER_CELL - 1).astype(np.int64))
    cy = (cell // (w // CLUSTER_CELL) + 0.5) * CLUSTER_CELL + rng.uniform(-0.3, 0.3, P)
    cx = (cell % (w // CLUSTER_CELL) + 0.5) * CLUSTER_CELL + rng.uniform(-0.3, 0.3, P)
    bw = CLUSTER_BOX * np.exp(rng.uniform(-0.02, 0.02, P))
    bh = CLUSTER_BOX * np.exp(rng.uniform(-0.02, 0.02, P))
    loc = np.stack([(cx / w - pr[:, 0]) / (0.1 * pr[:, 2]), (cy / h - pr[:, 1]) / (0.1 * pr[:, 3]),
                    np.log(bw / w / pr[:, 2]) / 0.2, np.log(bh / h / pr[:, 3]) / 0.2], 1)
    grid = np.linspace(lo, hi, P)
    forced = rng.choice(np.unique(cell), CLUSTER_FORCED, replace=False)
    low = np.nonzero(np.isin(cell, forced))[0]
    assert low.size <= P - 5000, (low.size, P)
    rest = np.setdiff1d(np.arange(P), low)
    p = np.zeros(P)
    p[low] = grid[rng.permutation(P - 5000)[:low.size]]
    used = np.isin(grid, p[low])
    p[rest] = grid[~used][rng.permutation(rest.size)]
    maps = [np.zeros((1, a, b, 8 if l == 0 else 6), dtype=np.float32) for l, (a, b) in enumerate(sizes)]
    _fill_heads(maps, 0, sizes, loc, np.log(p / (1.0 - p)), rng)
    return [torch.from_numpy(m) for m in maps], forced.size


# ---------------------------------------------------------------- tracker cases
def _face(frame, box):
    return {"frame": int(frame), "bbox": [float(v) for v in box], "conf": 0.99}


def tracker_cases():
    """{name: per-frame detection lists}: what SyncNetDetector.detect_face would hand track_face."""
    def drift(i, x0=200.0, y0=100.0, size=160.0):
        return (x0 + 0.5 * i, y0 + 0.25 * i, x0 + 0.5 * i + size, y0 + 0.25 * i + size + 8.0)

    cases = {}
    # gaps of at most 25 frames are interpolated
    miss = set(range(20, 30)) | set(range(60, 84))
    cases["short_gaps"] = [[] if i in miss else [_face(i, drift(i))] for i in range(140)]
    # a gap of more than 25 frames splits the track
    miss = set(range(70, 97))
    cases["long_gap"] = [[] if i in miss else [_face(i, drift(i))] for i in range(170)]
    # two faces, listed in alternating order
    two = []
    for i in range(80):
        a, b = _face(i, drift(i)), _face(i, drift(i, x0=700.0, y0=300.0, size=200.0))
        two.append([a, b] if i % 2 == 0 else [b, a])
    cases["two_faces"] = two
    # a track of at most 50 detections is dropped
    cases["too_short"] = [[_face(i, drift(i))] for i in range(50)]
    # a small face is dropped, the large one beside it stays
    cases["small_face"] = [[_face(i, drift(i, size=60.0)), _face(i, drift(i, x0=600.0, size=150.0))] for i in range(70)]
    return cases


# ---------------------------------------------------------------- comparing with a golden
def golden_errors(g, relu, l2norm, heads):
    """{label: max |got - golden| / RMS(golden)} of the 19 ReLU outputs and 3 L2Norm outputs
    (NCHW) and the 6 head maps (NHWC) against tests/golden/s3fd_net.npz."""
    errs = {}
    assert len(relu) == N_RELU and len(l2norm) == 3 and len(heads) == 6
    for kind, ts in (("relu", relu), ("l2norm", l2norm), ("head", heads)):
        for j, t in enumerate(ts):
            label = f"{kind}_{j}"
            assert tuple(t.shape) == tuple(g[label + "_shape"]), (label, tuple(t.shape), tuple(g[label + "_shape"]))
            flat = torch.as_tensor(t).reshape(-1).cpu().double()
            if label + "_idx" in g.files:
                flat = flat[torch.from_numpy(g[label + "_idx"]).long()]
            ref = torch.from_numpy(g[label]).double().reshape(-1)
            errs[label] = float((flat - ref).abs().max()) / float(g[label + "_rms"])
    return errs
