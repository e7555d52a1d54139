"""StableSyncNet (latentsync/models/stable_syncnet.py) on the HIP path: the reference's own
measure of lip-sync -- the cosine between an embedding of 16 aligned face frames (lower
half) and an embedding of the matching 52 columns of a Wav2Lip-style mel spectrogram;
above 0.5 counts as in sync (eval/eval_syncnet_acc.py).

The two DownEncoder2D towers run on the kernels the UNet and the VAE use (ops.conv,
ops.group_norm, ops.layer_norm, ops.attention, the GEGLU GEMM), NHWC bf16 storage with fp32
accumulation, plus ls_syncnet.hip: the mel front end, the input packing, the anisotropic
downsample convolutions and the score.  Inference only: dropout is ignored and there is no
gradient checkpointing.  State-dict keys are the reference's.
"""
import math

import numpy as np
import torch

from . import ops
from .unet import _Dev
from .weights import fill_state_dict

SAMPLE_RATE, N_FFT, HOP, N_MELS, FMIN, FMAX = 16000, 800, 200, 80, 55.0, 7600.0
MEL_STEPS_PER_SECOND = 80.0  # SAMPLE_RATE / HOP


# ---------------------------------------------------------------- host: filters, window plan
def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    logstep = np.log(6.4) / 27.0
    lin = f / f_sp
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_band_edges():
    """The 82 band edges in Hz of mel_filters(): equal steps on the Slaney mel scale."""
    return _mel_to_hz(np.linspace(_hz_to_mel(FMIN), _hz_to_mel(FMAX), N_MELS + 2))


def mel_filters():
    """float32 (80, 401): a restatement of librosa.filters.mel(sr=16000, n_fft=800,
    n_mels=80, fmin=55, fmax=7600) -- Slaney mel scale (htk=False), triangles between
    consecutive band edges evaluated at the FFT bin frequencies, Slaney norm (each row times
    2 / (f[i + 2] - f[i]), unit area).  librosa is not installed here: parity unpinned."""
    fft_f = np.fft.rfftfreq(N_FFT, 1.0 / SAMPLE_RATE)
    mel_f = mel_band_edges()
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.zeros((N_MELS, fft_f.size))
    for i in range(N_MELS):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:N_MELS + 2] - mel_f[:N_MELS]))[:, None]
    return w.astype(np.float32)


def window_plan(n_frames, T, fps=25, num_frames=16, stride=16, mel_len=None):
    """(frame starts, mel columns) of the windows sync_scores scores: starts 0, stride, ...
    with start + num_frames <= n_frames, column int(80.0 * (start / float(fps)))
    (syncnet_dataset.py:57-60); a window whose mel slice would be shorter than mel_len
    (default ceil(num_frames / 5 * 16) = 52 for 16 frames) is dropped, as the dataset
    `continue`s (:120-121).  T = mel frames."""
    if mel_len is None:
        mel_len = math.ceil(num_frames / 5 * 16)
    starts, cols = [], []
    for s in range(0, int(n_frames) - int(num_frames) + 1, int(stride)):
        c = int(MEL_STEPS_PER_SECOND * (s / float(fps)))
        if c + mel_len <= T:
            starts.append(s)
            cols.append(c)
    return starts, cols


# ---------------------------------------------------------------- parameters
def _pairs(f):
    return tuple(f) if isinstance(f, (list, tuple)) else (f, f)


def _encoder_shapes(prefix, cfg):
    sh = {}
    boc = list(cfg["block_out_channels"])

    def conv(p, o, i, k):
        sh[p + ".weight"], sh[p + ".bias"] = (o, i, k, k), (o,)

    def vec(p, c):
        sh[p + ".weight"], sh[p + ".bias"] = (c,), (c,)

    def lin(p, o, i):
        sh[p + ".weight"], sh[p + ".bias"] = (o, i), (o,)

    conv(prefix + ".conv_in", boc[0], cfg["in_channels"], 3)
    j, cin = 0, boc[0]
    for i, cout in enumerate(boc):
        p = f"{prefix}.down_blocks.{j}"
        vec(p + ".norm1", cin)
        conv(p + ".conv1", cout, cin, 3)
        vec(p + ".norm2", cout)
        conv(p + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(p + ".conv_shortcut", cout, cin, 1)
        if cfg["downsample_factors"][i] != 1:
            conv(p + ".downsample_conv", cout, cout, 3)
        j += 1
        if cfg["attn_blocks"][i] == 1:
            p = f"{prefix}.down_blocks.{j}"
            for nm in ("norm1", "norm2", "norm3"):
                vec(f"{p}.{nm}", cout)
            lin(p + ".ff.net.0.proj", 8 * cout, cout)
            lin(p + ".ff.net.2", cout, 4 * cout)
            conv(p + ".conv_in", cout, cout, 1)
            conv(p + ".conv_out", cout, cout, 1)
            for nm in ("to_q", "to_k", "to_v", "to_out.0"):
                lin(f"{p}.attn.{nm}", cout, cout)
            j += 1
        cin = cout
    vec(prefix + ".norm_out", boc[-1])
    return sh


def param_shapes(config):
    """{state-dict key: shape} of StableSyncNet(config), in the reference's order."""
    sh = {}
    for name in ("audio_encoder", "visual_encoder"):
        sh.update(_encoder_shapes(name, config[name]))
    return sh


# ---------------------------------------------------------------- device modules
GROUPS, GN_EPS, HEADS = 32, 1e-6, 8
WINDOWS_PER_BATCH = 48  # sync_scores embeds a clip's windows in batches of this many


def _conv(x, pw, **kw):
    # split_k = 1: no K range is split because few images share the call
    return ops.conv(x, pw, split_k=1, **kw)


class _Res:
    def __init__(self, dv, p, factor):
        sd = dv.sd
        self.n1 = (dv.f32(p + ".norm1.weight"), dv.f32(p + ".norm1.bias"))
        self.n2 = (dv.f32(p + ".norm2.weight"), dv.f32(p + ".norm2.bias"))
        self.c1 = dv.packed(p + ".conv1.weight", p + ".conv1.bias")
        self.c2 = dv.packed(p + ".conv2.weight", p + ".conv2.bias")
        self.sc = dv.packed(p + ".conv_shortcut.weight", p + ".conv_shortcut.bias") \
            if (p + ".conv_shortcut.weight") in sd else None
        self.factor = None if factor == 1 else _pairs(factor)
        self.ds = dv.packed(p + ".downsample_conv.weight", p + ".downsample_conv.bias") if self.factor else None
        # F.pad (left, right, top, bottom): (0,1,0,1); [1, w]: (0,1,1,1); [h, 1]: (1,1,0,1)
        self.pad = (0, 0)
        if self.factor and isinstance(factor, (list, tuple)):
            self.pad = (1, 0) if factor[0] == 1 else ((0, 1) if factor[1] == 1 else (0, 0))

    def __call__(self, x):
        n = x.shape[0]
        s1 = ops.group_norm(x, GROUPS, GN_EPS, *self.n1, n)
        h = _conv(ops.group_norm_apply(x, s1[0], s1[1], n, True), self.c1)
        s2 = ops.group_norm(h, GROUPS, GN_EPS, *self.n2, n)
        res = x if self.sc is None else _conv(x, self.sc)
        h = _conv(ops.group_norm_apply(h, s2[0], s2[1], n, True), self.c2, res=res)
        if self.factor is None:
            return h
        (sh, sw), (pt, pl) = self.factor, self.pad
        H, W = h.shape[1], h.shape[2]
        Ho, Wo = (H + pt + 1 - 3) // sh + 1, (W + pl + 1 - 3) // sw + 1
        if sh == sw == 2 and (pt, pl) == (0, 0):
            return _conv(h, self.ds, stride=2, pad=0, out_hw=(Ho, Wo))  # the VAE downsampler's form
        return ops.conv3x3_strided(h, self.ds, (sh, sw), (pt, pl), (Ho, Wo))


class _AttnBlock:
    def __init__(self, dv, p, c):
        sd = dv.sd
        self.c = c
        self.gn = (dv.f32(p + ".norm1.weight"), dv.f32(p + ".norm1.bias"))
        self.ln2 = (dv.f32(p + ".norm2.weight"), dv.f32(p + ".norm2.bias"))
        self.ln3 = (dv.f32(p + ".norm3.weight"), dv.f32(p + ".norm3.bias"))
        self.conv_in = dv.packed(p + ".conv_in.weight", p + ".conv_in.bias")
        self.conv_out = dv.packed(p + ".conv_out.weight", p + ".conv_out.bias")
        self.qkv = dv.packed(None, w=torch.cat([sd[p + f".attn.to_{n}.weight"] for n in "qkv"], 0),
                             b=torch.cat([sd[p + f".attn.to_{n}.bias"] for n in "qkv"], 0))
        self.o = dv.packed(p + ".attn.to_out.0.weight", p + ".attn.to_out.0.bias")
        self.ff1 = dv.packed(p + ".ff.net.0.proj.weight", p + ".ff.net.0.proj.bias", geglu=True)
        self.ff2 = dv.packed(p + ".ff.net.2.weight", p + ".ff.net.2.bias")

    def __call__(self, x):
        n, H, W, C = x.shape
        HW, rows, d = H * W, n * H * W, C // HEADS
        s = ops.group_norm(x, GROUPS, GN_EPS, *self.gn, n)
        h = _conv(ops.group_norm_apply(x, s[0], s[1], n, False), self.conv_in).view(rows, C)
        qkv = ops.linear(ops.layer_norm(h, *self.ln2), self.qkv, split_k=1)
        o = torch.empty((rows, C), dtype=torch.bfloat16, device=x.device)
        st = (HW * 3 * C, 0, 3 * C, d)
        ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], o, batch=n, z2=1, heads=HEADS, nq=HW, nk=HW, head_dim=d,
                      qs=st, ks=st, vs=st, os_=(HW * C, 0, C, d))
        h = ops.linear(o, self.o, res=h, split_k=1)
        g = ops.linear(ops.layer_norm(h, *self.ln3), self.ff1, act=ops.ACT_GEGLU, split_k=1)
        h = ops.linear(g, self.ff2, res=h, split_k=1)
        return _conv(h.view(n, H, W, C), self.conv_out, res=x)


class _Encoder:
    def __init__(self, dv, prefix, cfg):
        boc = list(cfg["block_out_channels"])
        if any(c % GROUPS for c in boc):
            raise ValueError(f"{prefix}: block_out_channels {boc} must be multiples of {GROUPS} (GroupNorm groups)")
        self.in_channels = cfg["in_channels"]
        self.cin_pad = (self.in_channels + 7) // 8 * 8
        self.conv_in = dv.packed(prefix + ".conv_in.weight", prefix + ".conv_in.bias", cin_pad=self.cin_pad)
        self.blocks = []
        j = 0
        for i, cout in enumerate(boc):
            self.blocks.append(_Res(dv, f"{prefix}.down_blocks.{j}", cfg["downsample_factors"][i]))
            j += 1
            if cfg["attn_blocks"][i] == 1:
                self.blocks.append(_AttnBlock(dv, f"{prefix}.down_blocks.{j}", cout))
                j += 1
        self.norm_out = (dv.f32(prefix + ".norm_out.weight"), dv.f32(prefix + ".norm_out.bias"))
        self.dim = boc[-1]

    def __call__(self, x, taps=None):
        """x NHWC bf16 (B, H, W, cin_pad) -> norm_out's output before the ReLU, bf16 (B, D)."""
        h = _conv(x, self.conv_in)
        for blk in self.blocks:
            h = blk(h)
            if taps is not None:
                taps.append(h)
        n = h.shape[0]
        if h.shape[1] != 1 or h.shape[2] != 1:
            raise ValueError(f"the encoder must end at 1 x 1, got {h.shape[1]} x {h.shape[2]}: input size and "
                             "downsample_factors do not match")
        s = ops.group_norm(h, GROUPS, GN_EPS, *self.norm_out, n)
        return ops.group_norm_apply(h, s[0], s[1], n, False).view(n, self.dim)


class StableSyncNet(torch.nn.Module):
    """The reference's constructor, state-dict keys and forward; weights live as an fp32
    state dict on the host and as packed bf16 operands on the device after .to(device)."""

    def __init__(self, config, gradient_checkpointing=False):
        super().__init__()
        self.config = {k: dict(config[k]) for k in ("audio_encoder", "visual_encoder")}
        self._shapes = param_shapes(self.config)
        self._state = None
        self._dev = None
        self._device = torch.device("cpu")
        self._filters = None
        self.resolution = None  # the face size the towers were built for (the config's data.resolution), if known
        self.eval()

    # -- weights
    def init_weights(self, seed: int):
        """Seeded random weights (weights.fill_state_dict), rounded to bf16 like the fixtures."""
        sd = fill_state_dict(self._shapes, seed)
        return self.load_state_dict({k: v.to(torch.bfloat16).float() for k, v in sd.items()})

    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in self._shapes if k not in state_dict]
        extra = [k for k in state_dict if k not in self._shapes]
        if missing or (strict and extra):
            raise RuntimeError(f"StableSyncNet.load_state_dict: missing keys {missing[:4]}"
                               f"{'...' if len(missing) > 4 else ''}, unexpected keys {extra[:4]}")
        for k, s in self._shapes.items():
            if tuple(state_dict[k].shape) != tuple(s):
                raise RuntimeError(f"StableSyncNet.load_state_dict: {k} has shape {tuple(state_dict[k].shape)}, "
                                   f"expected {tuple(s)}")
        self._state = {k: state_dict[k].detach().float().cpu().clone() for k in self._shapes}
        self._dev = None
        if self._device.type == "cuda":
            self._pack()
        return self

    def state_dict(self, *a, **k):
        if self._state is None:
            raise RuntimeError("StableSyncNet has no weights: load_state_dict / from_pretrained / init_weights first")
        return dict(self._state)

    @classmethod
    def from_pretrained(cls, config, ckpt_path, device="cpu"):
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        net = cls(config)
        net.load_state_dict(ckpt["state_dict"])
        return net.to(device)

    def _pack(self):
        dv = _Dev(self._state, self._device)
        self._dev = (_Encoder(dv, "visual_encoder", self.config["visual_encoder"]),
                     _Encoder(dv, "audio_encoder", self.config["audio_encoder"]))
        self._filters = torch.from_numpy(mel_filters()).to(self._device).contiguous()

    def to(self, device=None, dtype=None, *a, **k):
        if device is not None and not isinstance(device, torch.dtype):
            device = torch.device(device)
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
            raise NotImplementedError("StableSyncNet on the HIP path is inference only")
        return super().train(False)

    @property
    def device(self):
        return self._device

    @property
    def dim(self):
        return self.config["visual_encoder"]["block_out_channels"][-1]

    def _require(self):
        if self._dev is None:
            if self._state is not None and self._device.type == "cuda":
                self._pack()
            else:
                raise RuntimeError("StableSyncNet runs on the HIP device only: load weights and call .to('cuda') "
                                   "(there is no CPU path)")
        return self._dev

    # -- inference
    @torch.no_grad()
    def embed(self, vis, aud, taps=None):
        """vis NHWC bf16 (B, H, W, 3F), aud NHWC bf16 (B, 80, L, 8) (ops.syncnet_pack_*) ->
        (vision_embeds, audio_embeds fp32 (B, D) unit vectors, cosine fp32 (B,)).  taps: a dict
        that receives the outputs of every down block, {"visual": [...], "audio": [...]}."""
        venc, aenc = self._require()
        tv = [] if taps is not None else None
        ta = [] if taps is not None else None
        with torch.cuda.device(self._device):
            v, a, score = ops.sync_score(venc(vis, tv), aenc(aud, ta))
        if taps is not None:
            taps["visual"], taps["audio"] = tv, ta
        return v, a, score

    @torch.no_grad()
    def forward(self, image_sequences, audio_sequences):
        """image_sequences (B, 3F, H, W), audio_sequences (B, 1, 80, L) on the device ->
        (vision_embeds, audio_embeds), fp32 (B, D) unit vectors."""
        venc, aenc = self._require()
        def nhwc(x, enc):  # channels zero-padded to the multiple of 8 conv_in's weights are packed for
            if x.dim() != 4 or x.shape[1] != enc.in_channels:
                raise ValueError(f"StableSyncNet.forward: (B, {enc.in_channels}, H, W) expected, got {tuple(x.shape)}")
            x = x.to(self._device).permute(0, 2, 3, 1).to(torch.bfloat16)
            if enc.cin_pad == enc.in_channels:
                return x.contiguous()
            y = torch.zeros(x.shape[:3] + (enc.cin_pad,), dtype=torch.bfloat16, device=self._device)
            y[..., :x.shape[3]] = x
            return y

        v, a, _ = self.embed(nhwc(image_sequences, venc), nhwc(audio_sequences, aenc))
        return v, a


def melspectrogram(wav_16k, filters=None):
    """audio.py:59-65 on the device: fp32 mono 16 kHz samples (a tensor or array) ->
    (80, T) fp32, T = 1 + n // 200 (a view of the kernel's frame-major (T, 80))."""
    wav = torch.as_tensor(wav_16k)
    device = wav.device if wav.is_cuda else torch.device("cuda", torch.cuda.current_device())
    wav = wav.to(device, torch.float32).contiguous()
    if filters is None:
        filters = torch.from_numpy(mel_filters()).to(device)
    with torch.cuda.device(device):
        return ops.syncnet_mel(wav, filters).t()


@torch.no_grad()
def sync_scores(net, faces_u8, wav_16k, fps=25, num_frames=16, stride=16, resolution=None):
    """Sync confidence per window: faces_u8 uint8 (n, R, R, 3) aligned faces on the device
    (run_windows' out_u8), wav_16k the matching 16 kHz mono audio -> (scores fp32 (B,) on the
    device, frame starts).  Faces at another resolution than the network's (`resolution`,
    default: the faces' own) are resized first with ops.resize_faces_u8 (the dataset's
    ImageProcessor.resize)."""
    device = net.device
    faces_u8 = faces_u8.to(device)
    if resolution is None:
        resolution = net.resolution
    with torch.cuda.device(device):
        if resolution is not None and faces_u8.shape[1] != resolution:
            r = ops.resize_faces_u8(faces_u8.permute(0, 3, 1, 2).contiguous(), resolution, resolution)
            faces_u8 = r.permute(0, 2, 3, 1).contiguous()
        net._require()
        mel = ops.syncnet_mel(torch.as_tensor(wav_16k).to(device, torch.float32).contiguous(), net._filters)
        starts, cols = window_plan(faces_u8.shape[0], mel.shape[0], fps, num_frames, stride)
        if not starts:
            return torch.empty(0, dtype=torch.float32, device=device), starts
        mel_len = math.ceil(num_frames / 5 * 16)
        faces_u8 = faces_u8.contiguous()
        score = torch.empty(len(starts), dtype=torch.float32, device=device)
        for i in range(0, len(starts), WINDOWS_PER_BATCH):  # bounded activations whatever the clip length
            sl = slice(i, i + WINDOWS_PER_BATCH)
            vis = ops.syncnet_pack_frames(faces_u8, starts[sl], num_frames)
            aud = ops.syncnet_pack_mel(mel, cols[sl], mel_len)
            score[sl] = net.embed(vis, aud)[2]
    return score, starts
