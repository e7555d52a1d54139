"""The face detector and tracker of the reference's sync gate (eval/syncnet_detect.py
SyncNetDetector: eval/detectors/s3fd S3FD + track_face) on the HIP path.

`S3FDNet` keeps the reference's state-dict keys (vgg.N, L2Norm3_3 / 4_3 / 5_3, extras.N, loc.N,
conf.N) and its forward signature; `S3FD` keeps detect_faces and adds the batched `detect`;
`track_faces` restates SyncNetDetector.track_face on the host.  The trunk runs on
csrc/ls_s3fd.hip (ls_s3fd_prep, ls_conv3x3_relu, ls_maxpool2x2_ceil, ls_l2norm_scale) and on
ls_conv_general / ls_maxpool2d for the layers those do not cover (conv1_1, the 1 x 1 and
stride-2 convs, the heads); the SSD post-processing is ls_s3fd_detect and ls_nms_boxes.  NHWC
bf16 storage with fp32 accumulation, head maps and everything after them in fp32; inference
only.

Documented deviations from the reference:
  * scene detection (scenedetect's ContentDetector) is not carried: a clip is treated as ONE
    shot, so a track may run across a cut;
  * the JPEG round trip of the frames (ffmpeg -f image2, cv2.imread) is not reproduced, as in
    synceval.py: the detector sees the decoded frames as they are;
  * cv2.resize is restated from OpenCV's definition (ls_s3fd_prep); at scale 0.5, where cv2
    takes a 2 x 2 area path, the call is refused;
  * nms_ runs in fp32 on the device (the reference: float64 on the same fp32 values).
Unpinned: parity with cv2 itself, and the boxes carry meaning only with the real sfd_face.pth
checkpoint (the tests pin the network on seeded weights).
"""
import math
from itertools import product

import numpy as np
import torch

from . import ops
from .packing import pack_weight_general

PATH_WEIGHT = "checkpoints/auxiliary/sfd_face.pth"
IMG_MEAN_RGB = (123.0, 117.0, 104.0)
# detect() processes frames in chunks whose largest activation, the conv1_2 output (h w 64 bf16
# a frame), stays below this many bytes
ACT_BUDGET_BYTES = 256 << 20

# vgg: (module index, cin, cout, dilation) of the 3 x 3 convs, "P" floor pool, "C" ceil pool;
# fc7 (index 33) is the 1 x 1 conv after fc6 (index 31, dilation 6)
_VGG = ((0, 3, 64, 1), (2, 64, 64, 1), "P", (5, 64, 128, 1), (7, 128, 128, 1), "P",
        (10, 128, 256, 1), (12, 256, 256, 1), (14, 256, 256, 1), "C",
        (17, 256, 512, 1), (19, 512, 512, 1), (21, 512, 512, 1), "P",
        (24, 512, 512, 1), (26, 512, 512, 1), (28, 512, 512, 1), "P", (31, 512, 1024, 6))
_L2NORM = {14: ("L2Norm3_3", 256), 21: ("L2Norm4_3", 512), 28: ("L2Norm5_3", 512)}
_EXTRAS = ((1024, 256, 1), (256, 512, 3), (512, 128, 1), (128, 256, 3))  # (cin, cout, k); k 3: stride 2, pad 1
_HEAD_CIN = (256, 512, 512, 1024, 512, 256)
MIN_SIZES = (16, 32, 64, 128, 256, 512)
STEPS = (4, 8, 16, 32, 64, 128)

# Which kernel a trunk conv with Cin >= 64 runs on, by (Cin, N, dilation) alone: True =
# ls_conv3x3_relu, False = ls_conv_general.  Set from scripts/s3fd_bench.py.
CONV3X3_ON_NEW = {(64, 64, 1): True, (64, 128, 1): True, (128, 128, 1): True, (128, 256, 1): True,
                  (256, 256, 1): True, (256, 512, 1): True, (512, 512, 1): True, (512, 1024, 6): True}


def param_shapes():
    """{state-dict key: shape} of the reference's S3FDNet, in its order."""
    sh = {}
    for s in _VGG:
        if isinstance(s, tuple):
            i, cin, cout, _ = s
            sh[f"vgg.{i}.weight"], sh[f"vgg.{i}.bias"] = (cout, cin, 3, 3), (cout,)
    sh["vgg.33.weight"], sh["vgg.33.bias"] = (1024, 1024, 1, 1), (1024,)
    for name, c in _L2NORM.values():
        sh[name + ".weight"] = (c,)
    for i, (cin, cout, k) in enumerate(_EXTRAS):
        sh[f"extras.{i}.weight"], sh[f"extras.{i}.bias"] = (cout, cin, k, k), (cout,)
    for i, cin in enumerate(_HEAD_CIN):
        sh[f"loc.{i}.weight"], sh[f"loc.{i}.bias"] = (4, cin, 3, 3), (4,)
    for i, cin in enumerate(_HEAD_CIN):
        n = 4 if i == 0 else 2
        sh[f"conf.{i}.weight"], sh[f"conf.{i}.bias"] = (n, cin, 3, 3), (n,)
    return sh


def feature_map_sizes(h, w):
    """The six source map sizes of an h x w network input: two floor pools, the ceil pool, two
    floor pools (fc6 / fc7 keep the size), then two 3 x 3 stride-2 pad-1 convs."""
    out = []
    h, w = h // 2 // 2, w // 2 // 2
    out.append((h, w))
    h, w = (h + 1) // 2, (w + 1) // 2
    out.append((h, w))
    for _ in range(2):
        h, w = h // 2, w // 2
        out.append((h, w))
    for _ in range(2):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out.append((h, w))
    return out


def prior_boxes(imh, imw, fmaps):
    """PriorBox.forward: float64 arithmetic in the reference's order, rounded to fp32 once:
    (P, 4) = (cx, cy, w, h), level-major, row-major within a level."""
    mean = []
    for k, (feath, featw) in enumerate(fmaps):
        for i, j in product(range(feath), range(featw)):
            f_kw = imw / STEPS[k]
            f_kh = imh / STEPS[k]
            mean += [(j + 0.5) / f_kw, (i + 0.5) / f_kh, MIN_SIZES[k] / imw, MIN_SIZES[k] / imh]
    return np.asarray(mean, dtype=np.float64).astype(np.float32).reshape(-1, 4)


class S3FDNet(torch.nn.Module):
    """The reference's S3FDNet.  Weights live as an fp32 state dict on the host and as packed
    bf16 operands on the device after .to(device)."""

    def __init__(self, device="cpu"):
        super().__init__()
        self._shapes = param_shapes()
        self._state = None
        self._dev = None
        self._device = torch.device("cpu")
        self._priors = {}
        self.eval()
        self.to(device)

    # -- weights
    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in self._shapes if k not in state_dict]
        extra = [k for k in state_dict if k not in self._shapes]
        if missing or (strict and extra):
            raise RuntimeError(f"S3FDNet.load_state_dict: missing keys {missing[:4]}"
                               f"{'...' if len(missing) > 4 else ''}, unexpected keys {extra[:4]}")
        for k, s in self._shapes.items():
            if tuple(state_dict[k].shape) != tuple(s):
                raise RuntimeError(f"S3FDNet.load_state_dict: {k} has shape {tuple(state_dict[k].shape)}, "
                                   f"expected {tuple(s)}")
        self._state = {k: state_dict[k].detach().float().cpu().clone() for k in self._shapes}
        self._dev = None
        if self._device.type == "cuda":
            self._pack()
        return self

    def state_dict(self, *a, **k):
        if self._state is None:
            raise RuntimeError("S3FDNet has no weights: load_state_dict first")
        return dict(self._state)

    def _pack(self):
        sd, dev = self._state, self._device

        def packed(w, b, cin_pad=None):
            pw = pack_weight_general(w, cin_pad).to(torch.bfloat16).to(dev).contiguous()
            return ops.PackedGeneral(pw, b.float().to(dev).contiguous(), cin_pad or w.shape[1], (1,) + tuple(w.shape[2:]))

        d = {"vgg": {}, "l2": {}, "extras": [], "heads": []}
        for s in _VGG:
            if isinstance(s, tuple):
                i, cin, _, _ = s
                d["vgg"][i] = packed(sd[f"vgg.{i}.weight"], sd[f"vgg.{i}.bias"], 8 if cin == 3 else None)
        d["vgg"][33] = packed(sd["vgg.33.weight"], sd["vgg.33.bias"])
        for i, (name, _) in _L2NORM.items():
            d["l2"][i] = sd[name + ".weight"].float().to(dev).contiguous()
        for i in range(len(_EXTRAS)):
            d["extras"].append(packed(sd[f"extras.{i}.weight"], sd[f"extras.{i}.bias"]))
        for i in range(6):  # loc | conf as one conv: N = 8 at level 0, 6 elsewhere
            d["heads"].append(packed(torch.cat([sd[f"loc.{i}.weight"], sd[f"conf.{i}.weight"]], 0),
                                     torch.cat([sd[f"loc.{i}.bias"], sd[f"conf.{i}.bias"]], 0)))
        self._dev = d

    def to(self, device=None, dtype=None, *a, **k):
        if device is not None and not isinstance(device, torch.dtype):
            device = torch.device(device)
            if device.type == "cuda" and device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            if device != self._device:
                self._device = device
                self._dev = None
                self._priors = {}
                if device.type == "cuda" and self._state is not None:
                    self._pack()
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("S3FDNet on the HIP path is inference only")
        return super().train(False)

    @property
    def device(self):
        return self._device

    def _require(self):
        if self._dev is None:
            if self._state is not None and self._device.type == "cuda":
                self._pack()
            else:
                raise RuntimeError("S3FDNet runs on the HIP device only: load weights and call .to('cuda') "
                                   "(there is no CPU path)")
        return self._dev

    def priors(self, h, w):
        """The prior table of an h x w network input on the device, computed once per size."""
        key = (int(h), int(w))
        if key not in self._priors:
            p = prior_boxes(key[0], key[1], feature_map_sizes(*key))
            self._priors[key] = torch.from_numpy(p).to(self._device).contiguous()
        return self._priors[key]

    # -- the network
    def _conv3(self, h, pw, dil):
        if CONV3X3_ON_NEW[(pw.cin, pw.N, dil)]:
            return ops.conv3x3_relu(h, pw, dil)
        if dil != 1:
            raise RuntimeError("the dilated conv has no other kernel than ls_conv3x3_relu")
        return ops.conv_general(h, pw, (1, 1), (1, 1), relu=True)

    def head_maps(self, x, taps=None):
        """x bf16 (n, h, w, 8) as ls_s3fd_prep writes it -> the six head maps, fp32 (n, h_l, w_l,
        8 | 6) = loc | conf.  taps: a dict that receives "relu" (every ReLU output, in network
        order), "l2norm" (the three L2Norm outputs) and "heads"."""
        d = self._require()
        if x.dim() != 4 or x.shape[3] != 8 or x.dtype != torch.bfloat16:
            raise ValueError(f"S3FDNet: a bf16 (n, h, w, 8) input expected, got {x.dtype} {tuple(x.shape)}")
        if min(feature_map_sizes(x.shape[1], x.shape[2])[3]) < 1:
            raise ValueError(f"S3FDNet: a {x.shape[1]} x {x.shape[2]} input is too small (at least 32 x 32)")
        relu, l2, sources = [], [], []
        h = x
        for s in _VGG:
            if s == "P":
                h = ops.maxpool2d(h, (2, 2), (2, 2))
            elif s == "C":
                h = ops.maxpool2x2_ceil(h)
            else:
                i, cin, _, dil = s
                if cin == 3:
                    h = ops.conv_general(h, d["vgg"][i], (1, 1), (1, 1), relu=True)
                else:
                    h = self._conv3(h, d["vgg"][i], dil)
                relu.append(h)
                if i in d["l2"]:  # the trunk continues from the un-normalised tensor
                    l2.append(ops.l2norm_scale(h, d["l2"][i]))
                    sources.append(l2[-1])
        h = ops.conv_general(h, d["vgg"][33], relu=True)
        relu.append(h)
        sources.append(h)
        for i, (_, _, k) in enumerate(_EXTRAS):
            h = ops.conv_general(h, d["extras"][i], (2, 2) if k == 3 else (1, 1), (1, 1) if k == 3 else (0, 0), relu=True)
            relu.append(h)
            if i % 2 == 1:
                sources.append(h)
        heads = [ops.conv_general(src, d["heads"][i], (1, 1), (1, 1), out_f32=True) for i, src in enumerate(sources)]
        if taps is not None:
            taps["relu"], taps["l2norm"], taps["heads"] = relu, l2, heads
        return heads

    @torch.no_grad()
    def detections(self, x, taps=None, want_idx=False):
        """x bf16 (n, h, w, 8) -> (det fp32 (n, 750, 5) = score, x1, y1, x2, y2, counts int32 (n,))
        : output[:, 1] of the reference's forward."""
        with torch.cuda.device(self._device):
            heads = self.head_maps(x, taps)
            return ops.s3fd_detect(heads, self.priors(x.shape[1], x.shape[2]), want_idx=want_idx)

    @torch.no_grad()
    def forward(self, x):
        """S3FDNet.forward: x fp32 (n, 3, h, w), mean-subtracted -> fp32 (n, 2, 750, 5); class 0 is
        all zeros, class 1 holds (score, x1, y1, x2, y2) rows."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"S3FDNet.forward: (n, 3, h, w) expected, got {tuple(x.shape)}")
        self._require()
        with torch.cuda.device(self._device):
            xin = torch.zeros((x.shape[0], x.shape[2], x.shape[3], 8), dtype=torch.bfloat16, device=self._device)
            xin[..., :3] = x.to(self._device).permute(0, 2, 3, 1).to(torch.bfloat16)
            det, _ = self.detections(xin)
            out = torch.zeros((x.shape[0], 2, ops.S3FD_TOP_K, 5), dtype=torch.float32, device=self._device)
            out[:, 1] = det
        return out


class S3FD:
    """The reference's S3FD: detect_faces(image) on one RGB frame, plus the batched detect()."""

    def __init__(self, device="cuda", weights=None):
        self.device = torch.device(device)
        self.net = S3FDNet(device=self.device)
        if weights is None:
            weights = PATH_WEIGHT
        if not isinstance(weights, dict):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        self.net.load_state_dict(weights)

    def chunk_frames(self, h, w):
        """Frames per pass: the conv1_2 output (h w 64 bf16 a frame) stays under ACT_BUDGET_BYTES."""
        return max(1, ACT_BUDGET_BYTES // (h * w * 64 * 2))

    def _frames(self, frames_u8):
        f = torch.as_tensor(frames_u8)
        if f.dim() != 4 or f.shape[3] != 3 or f.dtype != torch.uint8:
            raise ValueError(f"S3FD: uint8 (n, H, W, 3) RGB frames expected, got {f.dtype} {tuple(f.shape)}")
        return f.to(self.net.device).contiguous()

    def _detections(self, frames, scale):
        """frames uint8 (n, H, W, 3) on the device -> det fp32 (n, 750, 5) at one scale."""
        n, H, W = frames.shape[:3]
        h, w = ops.s3fd_prep_size(H, W, scale)
        step = self.chunk_frames(h, w)
        out = []
        for s in range(0, n, step):
            out.append(self.net.detections(ops.s3fd_prep(frames[s:s + step], scale))[0])
        return torch.cat(out, 0)

    @staticmethod
    def _rows(out, counts):
        out, counts = out.cpu().numpy().astype(np.float64), counts.cpu().numpy()
        return [out[i, :int(c)] for i, c in enumerate(counts)]

    @torch.no_grad()
    def detect(self, frames_u8, conf_th=0.9, scale=0.25):
        """The detector over a clip, as SyncNetDetector.detect_face runs it: frames uint8 (n, H,
        W, 3) RGB -> a list of n float64 arrays (k_i, 5) = x1, y1, x2, y2, score in frame
        coordinates."""
        frames = self._frames(frames_u8)
        with torch.cuda.device(self.net.device):
            det = self._detections(frames, scale)
            out, counts = ops.nms_boxes(det, conf_th, frames.shape[2], frames.shape[1], 0.1)
        return self._rows(out, counts)

    @torch.no_grad()
    def detect_faces(self, image, conf_th=0.8, scales=[1]):
        """S3FD.detect_faces: image uint8 (H, W, 3) RGB -> float64 (k, 5) = x1, y1, x2, y2, score."""
        frames = self._frames(torch.as_tensor(np.ascontiguousarray(image))[None])
        with torch.cuda.device(self.net.device):
            det = torch.cat([self._detections(frames, s) for s in scales], 1).contiguous()
            out, counts = ops.nms_boxes(det, conf_th, frames.shape[2], frames.shape[1], 0.1)
        return self._rows(out, counts)[0]


def faces_from_detections(dets):
    """detect()'s per-frame arrays -> SyncNetDetector.detect_face's structure: per frame a list
    of {"frame", "bbox" (x1, y1, x2, y2 as a list), "conf"}."""
    return [[{"frame": i, "bbox": np.asarray(b[:4], dtype=np.float64).tolist(), "conf": float(b[4])} for b in boxes]
            for i, boxes in enumerate(dets)]


def bounding_box_iou(a, b):
    xa, ya, xb, yb = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    inter = max(0, xb - xa) * max(0, yb - ya)
    return inter / float((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def track_faces(dets, num_failed_det=25, min_track=50, min_face_size=100):
    """SyncNetDetector.track_face on the host: dets is detect_face's per-frame list of {"frame",
    "bbox", ...} (faces_from_detections); the result is [{"frame": int array, "bbox": float64
    (len, 4)}], the boxes interpolated linearly over the frames a track skipped (np.interp for
    the reference's interp1d).  The same greedy order: a track starts at the first unused face,
    takes a later face when it is at most num_failed_det frames after the track's last one and
    their IoU is > 0.5, and stops looking at a frame's faces at the first one further away
    than that.  The reference removes a taken face from the very list it is iterating, which
    makes it pass over the face that follows in that frame until the next track; that is kept.
    A track needs more than min_track detections and a mean interpolated width or height above
    min_face_size.  The whole clip is one shot: scene detection is not carried."""
    faces = [list(f) for f in dets]
    tracks = []
    while True:
        track = []
        for framefaces in faces:
            k = 0
            while k < len(framefaces):
                face = framefaces[k]
                k += 1  # not taken back after a removal: the reference's iterator does not either
                if not track:
                    track.append(face)
                    framefaces.remove(face)
                elif face["frame"] - track[-1]["frame"] <= num_failed_det:
                    if bounding_box_iou(face["bbox"], track[-1]["bbox"]) > 0.5:
                        track.append(face)
                        framefaces.remove(face)
                else:
                    break
        if not track:
            break
        if len(track) > min_track:
            framenum = np.array([f["frame"] for f in track])
            bboxes = np.array([np.array(f["bbox"], dtype=np.float64) for f in track])
            frame_i = np.arange(framenum[0], framenum[-1] + 1)
            bboxes_i = np.stack([np.interp(frame_i, framenum, bboxes[:, j]) for j in range(4)], axis=1)
            if max(np.mean(bboxes_i[:, 2] - bboxes_i[:, 0]), np.mean(bboxes_i[:, 3] - bboxes_i[:, 1])) > min_face_size:
                tracks.append({"frame": frame_i, "bbox": bboxes_i})
    return tracks
