"""The classic SyncNet evaluation (eval/eval_sync_conf.py of the reference) on the HIP path: AV
offset, LSE-D (min_dist) and LSE-C (conf) of a 224 x 224 face-crop track against its audio.

`SyncNetEval` keeps the reference's constructor, `loadParameters`, state-dict keys
(eval/syncnet/syncnet.py class S: netcnnaud / netfcaud / netfclip / netcnnlip) and
`evaluate` signature.  Both towers run on csrc/ls_synceval.hip: ls_mfcc (the
python_speech_features front end S was trained on), ls_conv_general (every conv and linear, the
eval-mode BatchNorm folded in and the ReLU in the epilogue), ls_maxpool2d and ls_sync_offset;
`crop_track` is SyncNetDetector.crop_video's crop (ls_crop_track).  NHWC bf16 storage with fp32
accumulation; inference only.

Two documented deviations from the reference:
  * its JPEG round trip of the frames (ffmpeg -f image2 to .jpg, cv2.imread) is not reproduced:
    the network sees the decoded frames as they are;
  * the visual tower runs once over the clip as a temporal convolution (kt = 5) instead of once
    per 5-frame window.  ls_conv_general's kernel form depends on K and N alone, so this cannot
    change a result; it is a fifth of the work.
Unpinned: parity with python_speech_features and with cv2.resize themselves (neither library is a
dependency; both are restated from their definitions), and the scores carry meaning only with
the real syncnet_v2.model checkpoint.
"""
import math

import numpy as np
import torch

from . import ops
from .packing import pack_weight_general

SAMPLE_RATE = 16000
BN_EPS = 1e-5
STEPS_PER_CHUNK = 32   # visual steps per pass: conv1's output is 2.3 MB a step
WINDOWS_PER_CHUNK = 256  # audio windows per pass

# (kind, ...) per module of S, in nn.Sequential order.  conv: (cin, cout, window, stride, pad)
_AUD = (("conv", 1, 64, (1, 3, 3), (1, 1), (1, 1)), ("pool", (1, 1), (1, 1), (0, 0)),
        ("conv", 64, 192, (1, 3, 3), (1, 1), (1, 1)), ("pool", (3, 3), (1, 2), (0, 0)),
        ("conv", 192, 384, (1, 3, 3), (1, 1), (1, 1)),
        ("conv", 384, 256, (1, 3, 3), (1, 1), (1, 1)),
        ("conv", 256, 256, (1, 3, 3), (1, 1), (1, 1)), ("pool", (3, 3), (2, 2), (0, 0)),
        ("conv", 256, 512, (1, 5, 4), (1, 1), (0, 0)))
_LIP = (("conv", 3, 96, (5, 7, 7), (2, 2), (0, 0)), ("pool", (3, 3), (2, 2), (0, 0)),
        ("conv", 96, 256, (1, 5, 5), (2, 2), (1, 1)), ("pool", (3, 3), (2, 2), (1, 1)),
        ("conv", 256, 256, (1, 3, 3), (1, 1), (1, 1)),
        ("conv", 256, 256, (1, 3, 3), (1, 1), (1, 1)),
        ("conv", 256, 256, (1, 3, 3), (1, 1), (1, 1)), ("pool", (3, 3), (2, 2), (0, 0)),
        ("conv", 256, 512, (1, 6, 6), (1, 1), (0, 0)))


def _seq_layout(spec):
    """[(sequential index of the conv, index of its BatchNorm, spec entry)] and the pools, as
    nn.Sequential numbers them: conv, BN, ReLU, then an optional pool."""
    out, i = [], 0
    for s in spec:
        if s[0] == "conv":
            out.append((i, s))
            i += 3
        else:
            out.append((i, s))
            i += 1
    return out


def param_shapes(num_layers_in_fc_layers=1024):
    """{state-dict key: shape} of S, in the reference's order (buffers included)."""
    sh = {}

    def bn(p, c):
        sh[p + ".weight"], sh[p + ".bias"] = (c,), (c,)
        sh[p + ".running_mean"], sh[p + ".running_var"], sh[p + ".num_batches_tracked"] = (c,), (c,), ()

    def tower(name, spec, three_d):
        for i, s in _seq_layout(spec):
            if s[0] != "conv":
                continue
            _, cin, cout, win, _, _ = s
            sh[f"{name}.{i}.weight"] = (cout, cin) + (tuple(win) if three_d else tuple(win[1:]))
            sh[f"{name}.{i}.bias"] = (cout,)
            bn(f"{name}.{i + 1}", cout)

    def head(name):
        sh[name + ".0.weight"], sh[name + ".0.bias"] = (512, 512), (512,)
        bn(name + ".1", 512)
        sh[name + ".3.weight"], sh[name + ".3.bias"] = (num_layers_in_fc_layers, 512), (num_layers_in_fc_layers,)

    tower("netcnnaud", _AUD, False)
    head("netfcaud")
    head("netfclip")
    tower("netcnnlip", _LIP, True)
    return sh


def fold_batchnorm(w, b, gamma, beta, mean, var, eps=BN_EPS):
    """Eval-mode BatchNorm after a conv / linear, folded into it in fp32:
    scale = gamma / sqrt(var + eps); w' = w scale[o], b' = (b - mean) scale + beta."""
    w, b = w.float(), b.float()
    scale = gamma.float() / torch.sqrt(var.float() + eps)
    return w * scale.reshape((-1,) + (1,) * (w.dim() - 1)), (b - mean.float()) * scale + beta.float()


# ---------------------------------------------------------------- host: MFCC filters, plans
def mfcc_filters():
    """float32 (26, 257): python_speech_features.get_filterbanks(26, 512, 16000, 0, 8000) from
    its definition -- 28 points equally spaced in mel = 2595 log10(1 + f / 700) between 0 and
    8000 Hz, bin = floor(513 hz / 16000), triangles between consecutive bins."""
    mel = np.linspace(0.0, 2595.0 * np.log10(1.0 + 8000.0 / 700.0), 28)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    b = np.floor(513 * hz / 16000.0)
    fb = np.zeros((26, 257))
    for j in range(26):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb.astype(np.float32)


def mfcc_frames(n):
    """Frames python_speech_features cuts n samples into: 400 every 160, the tail padded."""
    n = int(n)
    return 1 + -(-(n - 400) // 160) if n > 400 else 1


def window_plan(n_frames, n_samples):
    """syncnet_eval.py:110-133 -> lastframe, the number of windows: min_length = min(frames,
    floor(samples / 640)), lastframe = min_length - 5; window i holds frames i .. i + 4 and
    MFCC columns 4 i .. 4 i + 19.  Fewer than 6 usable frames leave no window: ValueError."""
    min_length = min(int(n_frames), int(n_samples) // 640)
    lastframe = min_length - 5
    if lastframe < 1:
        raise ValueError(f"evaluate: {n_frames} frames and {n_samples} samples at 16 kHz give {min_length} usable "
                         "frames; at least 6 are needed for one 5-frame window")
    return lastframe


def offset_from_means(mean_dists, vshift):
    """syncnet_eval.py:145-148 on the host: (av_offset, min_dist, conf) from the 2 vshift + 1
    means: the first minimum, av_offset = vshift - argmin, conf = median - min with torch's
    median (the lower middle of an even count)."""
    m = np.asarray(mean_dists, dtype=np.float32).reshape(-1)
    if m.size != 2 * int(vshift) + 1:
        raise ValueError(f"offset_from_means: {2 * int(vshift) + 1} means expected for vshift {vshift}, got {m.size}")
    idx = int(np.argmin(m))
    median = np.sort(m)[(m.size - 1) // 2]
    return int(vshift) - idx, float(m[idx]), float(np.float32(median) - m[idx])


def pcm16(audio):
    """Float mono samples in [-1, 1) -> the values of the reference's extracted pcm_s16le file,
    as fp32: x 32768, rounded to nearest (ties to even), clipped to the int16 range."""
    a = torch.as_tensor(audio).to(torch.float32)
    return torch.clamp(torch.round(a * 32768.0), -32768.0, 32767.0)


def crop_plan(boxes, crop_scale=0.4):
    """The host side of SyncNetDetector.crop_video (syncnet_detect.py:176-202): boxes float
    (n, 4) x1, y1, x2, y2 -> int32 (n, 5) = (y0, y1, x0, x1, bsi) in the frame padded by bsi.
    An interior all-NaN row is interpolated linearly from its neighbours (track_face's
    interp1d); a leading or trailing one is a ValueError.  s = max(w, h) / 2 and the centre are
    median-filtered over 13 frames as scipy.signal.medfilt(., 13) does (zeros past both ends)."""
    def medfilt(v, kernel_size):
        h = kernel_size // 2
        p = np.concatenate([np.zeros(h), v, np.zeros(h)])
        return np.median(np.lib.stride_tricks.sliding_window_view(p, kernel_size), axis=1)

    b = np.array(boxes, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] < 1:
        raise ValueError(f"crop_track: boxes must be (n, 4) x1, y1, x2, y2, got {b.shape}")
    nan = np.isnan(b)
    if (nan.any(1) != nan.all(1)).any():
        raise ValueError("crop_track: a box row must be all numbers or all NaN")
    miss = nan.all(1)
    if miss[0] or miss[-1]:
        raise ValueError("crop_track: the first and the last box must be given (NaN rows are interpolated between "
                         "their neighbours only)")
    if miss.any():
        have = np.nonzero(~miss)[0]
        for j in range(4):
            b[:, j] = np.interp(np.arange(b.shape[0]), have, b[have, j])
    if not np.isfinite(b).all():
        raise ValueError("crop_track: boxes must be finite")
    cs = float(crop_scale)
    s = medfilt(np.maximum(b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]) / 2, kernel_size=13)
    cx = medfilt((b[:, 0] + b[:, 2]) / 2, kernel_size=13)
    cy = medfilt((b[:, 1] + b[:, 3]) / 2, kernel_size=13)
    plan = np.zeros((b.shape[0], 5), dtype=np.int64)
    for i in range(b.shape[0]):
        bs = s[i]
        bsi = int(bs * (1 + 2 * cs))
        my, mx = cy[i] + bsi, cx[i] + bsi
        plan[i] = (int(my - bs), int(my + bs * (1 + 2 * cs)), int(mx - bs * (1 + cs)), int(mx + bs * (1 + cs)), bsi)
    return plan


def _check_plan(plan, H, W):
    """numpy's slice of the padded frame must be the whole requested box: a start below 0 or an
    end past the padded frame would wrap or clip there, which a track never means."""
    for i, (y0, y1, x0, x1, bsi) in enumerate(plan.tolist()):
        if bsi < 0 or y0 < 0 or x0 < 0 or y1 <= y0 or x1 <= x0 or y1 > H + 2 * bsi or x1 > W + 2 * bsi:
            raise ValueError(f"crop_track: frame {i}: crop rows {y0}:{y1}, columns {x0}:{x1} do not lie in the "
                             f"{H + 2 * bsi} x {W + 2 * bsi} padded frame (box too large or degenerate)")


def crop_track(frames_u8, boxes, crop_scale=0.4):
    """frames uint8 (n, H, W, 3) RGB on the device + detector boxes (n, 4) -> the 224 x 224 crop
    track uint8 (n, 224, 224, 3) the evaluation runs on (crop_plan on the host, ls_crop_track)."""
    if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
        raise ValueError("crop_track: frames must be a uint8 (n, H, W, 3) tensor on the HIP device")
    plan = crop_plan(boxes, crop_scale)
    n, H, W = frames_u8.shape[:3]
    if plan.shape[0] != n:
        raise ValueError(f"crop_track: {plan.shape[0]} boxes for {n} frames")
    _check_plan(plan, H, W)
    with torch.cuda.device(frames_u8.device):
        return ops.crop_track(frames_u8.contiguous(), torch.from_numpy(plan.astype(np.int32)).to(frames_u8.device))


# ---------------------------------------------------------------- device towers
class _Tower:
    """One conv tower and its head, packed: BatchNorm folded in fp32, rounded to bf16 once."""

    def __init__(self, sd, cnn, fc, spec, three_d, device):
        def packed(w, b, window, cin_pad=None):
            pw = pack_weight_general(w, cin_pad).to(torch.bfloat16).to(device).contiguous()
            return ops.PackedGeneral(pw, b.float().to(device).contiguous(), cin_pad or w.shape[1], window)

        def bn(p):
            return (sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"])

        self.layers = []
        for i, s in _seq_layout(spec):
            if s[0] == "pool":
                if s[1] != (1, 1):  # MaxPool2d(1, 1) is the identity
                    self.layers.append(s)
                continue
            _, cin, cout, win, stride, pad = s
            w, b = fold_batchnorm(sd[f"{cnn}.{i}.weight"], sd[f"{cnn}.{i}.bias"], *bn(f"{cnn}.{i + 1}"))
            if not three_d:
                w = w[:, :, None]
            self.layers.append(("conv", packed(w, b, win, (cin + 7) // 8 * 8), stride, pad))
        w, b = fold_batchnorm(sd[fc + ".0.weight"], sd[fc + ".0.bias"], *bn(fc + ".1"))
        self.fc0 = packed(w, b, (1, 1, 1))
        self.fc1 = packed(sd[fc + ".3.weight"], sd[fc + ".3.bias"], (1, 1, 1))
        self.cin_pad = self.layers[0][1].cin
        self.kt = self.layers[0][1].window[0]

    def features(self, x, taps=None):
        """x bf16 (T, H, W, cin_pad) -> the tower's 512 values per step, bf16 (steps, 512)."""
        h = x
        for layer in self.layers:
            if layer[0] == "conv":
                h = ops.conv_general(h, layer[1], layer[2], layer[3], relu=True)
                if taps is not None:
                    taps.append(h)
            else:
                h = ops.maxpool2d(h, layer[1], layer[2], layer[3])
        if h.shape[1] != 1 or h.shape[2] != 1:
            raise ValueError(f"the tower must end at 1 x 1, got {h.shape[1]} x {h.shape[2]}: wrong input size")
        return h

    def head(self, feat, taps=None):
        """feat bf16 (steps, 1, 1, 512) -> fp32 (steps, num_layers_in_fc_layers)."""
        h = ops.conv_general(feat, self.fc0, relu=True)
        if taps is not None:
            taps.append(h)
        return ops.conv_general(h, self.fc1, out_f32=True).reshape(feat.shape[0], -1)


class SyncNetEval(torch.nn.Module):
    """The reference's SyncNetEval: constructor, loadParameters, evaluate.  Weights live as an
    fp32 state dict on the host and as packed bf16 operands on the device after .to(device)."""

    def __init__(self, dropout=0, num_layers_in_fc_layers=1024, device="cpu"):
        super().__init__()
        self.num_layers_in_fc_layers = int(num_layers_in_fc_layers)
        self._shapes = param_shapes(self.num_layers_in_fc_layers)
        self._state = None
        self._dev = None
        self._device = torch.device("cpu")
        self._filters = None
        self.eval()
        self.to(device)

    # -- weights
    def loadParameters(self, path):
        loaded = torch.load(path, map_location="cpu", weights_only=True)
        return self.load_state_dict(loaded)

    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in self._shapes if k not in state_dict]
        extra = [k for k in state_dict if k not in self._shapes]
        if missing or (strict and extra):
            raise RuntimeError(f"SyncNetEval.load_state_dict: missing keys {missing[:4]}"
                               f"{'...' if len(missing) > 4 else ''}, unexpected keys {extra[:4]}")
        for k, s in self._shapes.items():
            if tuple(state_dict[k].shape) != tuple(s):
                raise RuntimeError(f"SyncNetEval.load_state_dict: {k} has shape {tuple(state_dict[k].shape)}, "
                                   f"expected {tuple(s)}")
        self._state = {k: (state_dict[k].detach().cpu().clone() if k.endswith("num_batches_tracked")
                           else state_dict[k].detach().float().cpu().clone()) for k in self._shapes}
        self._dev = None
        if self._device.type == "cuda":
            self._pack()
        return self

    def state_dict(self, *a, **k):
        if self._state is None:
            raise RuntimeError("SyncNetEval has no weights: loadParameters / load_state_dict first")
        return dict(self._state)

    def _pack(self):
        self._dev = (_Tower(self._state, "netcnnlip", "netfclip", _LIP, True, self._device),
                     _Tower(self._state, "netcnnaud", "netfcaud", _AUD, False, self._device))
        self._filters = torch.from_numpy(mfcc_filters()).to(self._device).contiguous()

    def to(self, device=None, dtype=None, *a, **k):
        if device is not None and not isinstance(device, torch.dtype):
            device = torch.device(device)
            if device.type == "cuda" and device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            if device != self._device:
                self._device = device
                self._dev = None
                if device.type == "cuda" and self._state is not None:
                    self._pack()
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("SyncNetEval on the HIP path is inference only")
        return super().train(False)

    @property
    def device(self):
        return self._device

    def _require(self):
        if self._dev is None:
            if self._state is not None and self._device.type == "cuda":
                self._pack()
            else:
                raise RuntimeError("SyncNetEval runs on the HIP device only: load weights and call .to('cuda') "
                                   "(there is no CPU path)")
        return self._dev

    # -- the towers
    def _lip_clip(self, clip, taps=None, head=True):
        """clip bf16 (n, 224, 224, 8) B, G, R, 0.. -> one row per 5-frame window (n - 4 rows),
        in chunks of STEPS_PER_CHUNK steps; taps only for a single chunk."""
        lip = self._require()[0]
        n = clip.shape[0]
        out = []
        for s in range(0, n - 4, STEPS_PER_CHUNK):
            e = min(n - 4, s + STEPS_PER_CHUNK)
            f = lip.features(clip[s:e + 4], taps)
            out.append(lip.head(f, taps) if head else f.reshape(e - s, -1).float())
        return torch.cat(out, 0)

    def _aud_windows(self, x, taps=None):
        """x bf16 (B, 13, 20, 8) -> fp32 (B, D), in chunks of WINDOWS_PER_CHUNK windows."""
        aud = self._require()[1]
        out = []
        for s in range(0, x.shape[0], WINDOWS_PER_CHUNK):
            out.append(aud.head(aud.features(x[s:s + WINDOWS_PER_CHUNK], taps), taps))
        return torch.cat(out, 0)

    def _pad8(self, x_nhwc):
        y = torch.zeros(x_nhwc.shape[:-1] + (8,), dtype=torch.bfloat16, device=self._device)
        y[..., :x_nhwc.shape[-1]] = x_nhwc.to(torch.bfloat16)
        return y

    def _lip_input(self, x):
        if x.dim() != 5 or x.shape[1] != 3 or x.shape[2] != 5:
            raise ValueError(f"forward_lip: (N, 3, 5, H, W) expected, got {tuple(x.shape)}")
        return self._pad8(x.to(self._device).permute(0, 2, 3, 4, 1))  # (N, 5, H, W, 8)

    @torch.no_grad()
    def forward_lip(self, x):
        """S.forward_lip: x fp32 (N, 3, 5, 224, 224) -> fp32 (N, num_layers_in_fc_layers)."""
        with torch.cuda.device(self._device):
            return torch.cat([self._lip_clip(w) for w in self._lip_input(x)], 0)

    @torch.no_grad()
    def forward_lipfeat(self, x):
        """S.forward_lipfeat: the 512 values in front of netfclip, fp32 (N, 512)."""
        with torch.cuda.device(self._device):
            return torch.cat([self._lip_clip(w, head=False) for w in self._lip_input(x)], 0)

    @torch.no_grad()
    def forward_aud(self, x):
        """S.forward_aud: x fp32 (N, 1, 13, 20) -> fp32 (N, num_layers_in_fc_layers)."""
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"forward_aud: (N, 1, 13, 20) expected, got {tuple(x.shape)}")
        with torch.cuda.device(self._device):
            return self._aud_windows(self._pad8(x.to(self._device).permute(0, 2, 3, 1)))

    # -- the evaluation
    @torch.no_grad()
    def features(self, frames, audio_i16, taps=None):
        """frames uint8 (n, 224, 224, 3) RGB and fp32 int16-scale 16 kHz samples, both on the
        device -> (im_feat, cc_feat) fp32 (windows, D).  taps: a dict that receives the MFCC and
        every conv / linear output of both towers ({"mfcc", "lip": [...], "aud": [...]})."""
        self._require()
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (224, 224, 3) or frames.dtype != torch.uint8:
            raise ValueError(f"evaluate: frames must be uint8 (n, 224, 224, 3), got {frames.dtype} {tuple(frames.shape)}")
        lastframe = window_plan(frames.shape[0], audio_i16.numel())
        tl = [] if taps is not None else None
        ta = [] if taps is not None else None
        with torch.cuda.device(self._device):
            mf = ops.mfcc(audio_i16.to(self._device, torch.float32).contiguous(), self._filters)
            if 4 * (lastframe - 1) + 20 > mf.shape[1]:
                raise ValueError(f"evaluate: the audio gives {mf.shape[1]} MFCC columns, window {lastframe - 1} needs "
                                 f"{4 * (lastframe - 1) + 20}")
            # cv2.imread order: the network is fed B, G, R as raw 0..255 values
            clip = self._pad8(frames[:lastframe + 4].to(self._device).flip(-1))
            im = self._lip_clip(clip, tl)
            cols = (4 * torch.arange(lastframe, device=self._device)[:, None] +
                    torch.arange(20, device=self._device)[None, :])
            win = mf[:, cols].permute(1, 0, 2)[..., None]  # (B, 13, 20, 1)
            cc = self._aud_windows(self._pad8(win), ta)
        if taps is not None:
            taps["mfcc"], taps["lip"], taps["aud"] = mf, tl, ta
        return im.contiguous(), cc.contiguous()

    @torch.no_grad()
    def evaluate(self, video_path=None, temp_dir="temp", batch_size=20, vshift=15, *, frames=None, audio=None,
                 sample_rate=SAMPLE_RATE, details=None):
        """syncnet_eval.py:46-157 -> (av_offset int, min_dist float, conf float).  Either
        `video_path`, an .avi of the 224 x 224 crop track at 25 frames/s with its audio, or
        `frames` (uint8 (n, 224, 224, 3) RGB on the device) plus `audio` (float mono in [-1, 1)
        at `sample_rate`).  temp_dir and batch_size are accepted and ignored.  details: a dict
        that receives im_feat, cc_feat, dists and mean_dists (device tensors)."""
        self._require()
        if (video_path is None) == (frames is None):
            raise ValueError("evaluate: give either video_path or frames= and audio=")
        if video_path is not None:
            from . import video
            frames, fps, audio, sample_rate = video.read_avi_auto(video_path, self._device)
            if abs(float(fps) - 25.0) > 1e-6:
                raise ValueError(f"evaluate: {video_path} runs at {fps} frames/s; the evaluation is defined at 25")
            if audio is None:
                raise ValueError(f"evaluate: {video_path} has no audio stream")
        if audio is None:
            raise ValueError("evaluate: frames= needs audio=")
        frames = torch.as_tensor(frames).to(self._device)
        a = torch.as_tensor(audio).reshape(-1).to(torch.float32)
        with torch.cuda.device(self._device):
            if int(sample_rate) != SAMPLE_RATE:
                a = ops.resample(a, int(sample_rate), SAMPLE_RATE)
            im, cc = self.features(frames, pcm16(a.to(self._device)))
            dists, means = ops.sync_offset(im, cc, vshift)
        if details is not None:
            details.update(im_feat=im, cc_feat=cc, dists=dists, mean_dists=means)
        return offset_from_means(means.cpu().numpy(), vshift)
