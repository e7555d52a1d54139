"""The project's own restatement of StableSyncNet and of its mel front end, for the tests.

  * forward(sd, config, image, audio, bf16=False): the network in fp32 torch on the CPU from a
    reference-named state dict.  bf16=True rounds to bf16 at the points where the device path
    stores bf16 (every conv / linear output after its bias and residual, every materialised
    GroupNorm / LayerNorm output, the attention output, the GEGLU product); everything between
    two such points is fp32, as on the device, so only the accumulation order differs.
  * mel_oracle(wav): the mel front end (latentsync/utils/audio.py:59-65) in float64 numpy.
  * the two test configs, their seeded inputs and weights, and the chirp the mel tests use.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from latentsync_amd import syncnet
from latentsync_amd.weights import fill_state_dict, init_tensor

CONFIG_A = dict(
    audio_encoder=dict(in_channels=1, block_out_channels=[32, 32, 64, 64, 64],
                       downsample_factors=[[2, 1], 2, 1, 2, [2, 3]], attn_blocks=[0, 0, 1, 0, 0], dropout=0.0),
    visual_encoder=dict(in_channels=48, block_out_channels=[32, 32, 64, 64, 64],
                        downsample_factors=[[1, 2], 2, 2, 2, 2], attn_blocks=[0, 0, 1, 0, 0], dropout=0.0))
# the real model's spatial walk (configs/syncnet/syncnet_16_pixel_attn.yaml) at 32 channels
CONFIG_B = dict(
    audio_encoder=dict(in_channels=1, block_out_channels=[32] * 7,
                       downsample_factors=[[2, 1], 2, 2, 1, 2, 2, [2, 3]], attn_blocks=[0, 0, 0, 1, 1, 0, 0],
                       dropout=0.0),
    visual_encoder=dict(in_channels=48, block_out_channels=[32] * 8,
                        downsample_factors=[[1, 2], 2, 2, 2, 2, 2, 2, 2], attn_blocks=[0, 0, 0, 0, 1, 1, 0, 0],
                        dropout=0.0))
# a tail that depends on the input: 128 channels at the end, 4 per GroupNorm group
CONFIG_C = dict(
    audio_encoder=dict(in_channels=1, block_out_channels=[32, 64, 128], downsample_factors=[[2, 1], 2, [2, 3]],
                       attn_blocks=[0, 0, 0], dropout=0.0),
    visual_encoder=dict(in_channels=48, block_out_channels=[32, 64, 128, 128], downsample_factors=[[1, 2], 2, 2, 2],
                        attn_blocks=[0, 1, 0, 0], dropout=0.0))
CASES = {  # name -> (config, image shape (B, 3F, H, W), audio shape (B, 1, 80 or less, L), seed)
    "A": (CONFIG_A, (3, 48, 16, 32), (3, 1, 20, 13), 11),
    "B": (CONFIG_B, (2, 48, 128, 256), (2, 1, 80, 52), 12),
    "C": (CONFIG_C, (3, 48, 8, 16), (3, 1, 8, 6), 13),
}
SUBSAMPLE = 8192  # block outputs above 2 * SUBSAMPLE elements are stored at SUBSAMPLE fixed positions


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def case_weights(name):
    """The seeded state dict of a case, every tensor rounded to bf16 (GroupNorm / LayerNorm
    affines are drawn like any other 1-D weight: 1 + 0.1 N(0,1), biases 0.05 N(0,1))."""
    cfg, _, _, seed = CASES[name]
    return {k: bf16_round(v) for k, v in fill_state_dict(syncnet.param_shapes(cfg), seed).items()}


def case_inputs(name):
    """(image, audio) fp32, bf16-exact: pixels uniform on the (x / 255 - 0.5) / 0.5 grid rounded
    to bf16, mel values 1.5 N(0,1) clipped to [-4, 4]."""
    _, ishape, ashape, seed = CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    px = torch.randint(0, 256, ishape, generator=g).float()
    image = bf16_round((px / 255.0 - 0.5) / 0.5)
    audio = bf16_round((1.5 * torch.randn(ashape, generator=g)).clamp(-4, 4))
    return image, audio


def _gn(x, w, b, silu, r):
    y = F.group_norm(x, 32, w, b, eps=1e-6)
    return r(F.silu(y) if silu else y)


def _resnet(sd, p, x, factor, r):
    h = r(F.conv2d(_gn(x, sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], True, r), sd[p + ".conv1.weight"],
                   sd[p + ".conv1.bias"], padding=1))
    h = F.conv2d(_gn(h, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], True, r), sd[p + ".conv2.weight"],
                 sd[p + ".conv2.bias"], padding=1)
    if (p + ".conv_shortcut.weight") in sd:
        x = r(F.conv2d(x, sd[p + ".conv_shortcut.weight"], sd[p + ".conv_shortcut.bias"]))
    h = r(h + x)
    if factor == 1:
        return h
    pad = (0, 1, 0, 1)
    if isinstance(factor, (list, tuple)):
        factor = tuple(factor)
        if factor[0] == 1:
            pad = (0, 1, 1, 1)
        elif factor[1] == 1:
            pad = (1, 1, 0, 1)
    h = F.pad(h, pad, mode="constant", value=0)
    return r(F.conv2d(h, sd[p + ".downsample_conv.weight"], sd[p + ".downsample_conv.bias"], stride=factor))


def _attn_block(sd, p, x, r):
    b, c, hh, ww = x.shape
    lin = lambda t, k: F.linear(t, sd[f"{p}.{k}.weight"], sd[f"{p}.{k}.bias"])
    ln = lambda t, k: r(F.layer_norm(t, (c,), sd[f"{p}.{k}.weight"], sd[f"{p}.{k}.bias"]))
    h = r(F.conv2d(_gn(x, sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], False, r), sd[p + ".conv_in.weight"],
                   sd[p + ".conv_in.bias"]))
    h = h.permute(0, 2, 3, 1).reshape(b, hh * ww, c)
    n = ln(h, "norm2")
    heads = lambda t: t.reshape(b, hh * ww, 8, c // 8).permute(0, 2, 1, 3)
    q, k, v = (heads(r(lin(n, f"attn.to_{s}"))) for s in "qkv")
    o = r(F.scaled_dot_product_attention(q, k, v)).permute(0, 2, 1, 3).reshape(b, hh * ww, c)
    h = r(lin(o, "attn.to_out.0") + h)
    hid, gate = lin(ln(h, "norm3"), "ff.net.0.proj").chunk(2, dim=-1)
    h = r(lin(r(hid * F.gelu(gate)), "ff.net.2") + h)
    h = h.reshape(b, hh, ww, c).permute(0, 3, 1, 2)
    return r(F.conv2d(h, sd[p + ".conv_out.weight"], sd[p + ".conv_out.bias"]) + x)


def encoder(sd, prefix, cfg, x, r, blocks=None):
    h = r(F.conv2d(x, sd[prefix + ".conv_in.weight"], sd[prefix + ".conv_in.bias"], padding=1))
    j = 0
    for i in range(len(cfg["block_out_channels"])):
        h = _resnet(sd, f"{prefix}.down_blocks.{j}", h, cfg["downsample_factors"][i], r)
        j += 1
        if blocks is not None:
            blocks.append(h)
        if cfg["attn_blocks"][i] == 1:
            h = _attn_block(sd, f"{prefix}.down_blocks.{j}", h, r)
            j += 1
            if blocks is not None:
                blocks.append(h)
    h = r(F.group_norm(h, 32, sd[prefix + ".norm_out.weight"], sd[prefix + ".norm_out.bias"], eps=1e-6))
    return F.relu(h)


@torch.no_grad()
def forward(sd, config, image, audio, bf16=False):
    """-> dict(vision_embeds, audio_embeds (B, D), cosine (B,), visual_blocks, audio_blocks:
    the NCHW output of every down_blocks[i])."""
    r = bf16_round if bf16 else (lambda t: t)
    sd = {k: v.float() for k, v in sd.items()}
    vb, ab = [], []
    v = encoder(sd, "visual_encoder", config["visual_encoder"], image.float(), r, vb)
    a = encoder(sd, "audio_encoder", config["audio_encoder"], audio.float(), r, ab)
    v = F.normalize(v.reshape(v.shape[0], -1), p=2, dim=1)
    a = F.normalize(a.reshape(a.shape[0], -1), p=2, dim=1)
    return dict(vision_embeds=v, audio_embeds=a, cosine=F.cosine_similarity(v, a), visual_blocks=vb, audio_blocks=ab)


def subsample_index(numel, seed):
    """The fixed positions at which a large block output is stored (None: stored whole)."""
    if numel <= 2 * SUBSAMPLE:
        return None
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(numel, generator=g)[:SUBSAMPLE].sort().values


# ---------------------------------------------------------------- mel front end, float64
def chirp_signal(n, seed=0):
    """0.1 N(0,1) + 0.3 chirp(200 -> 3800 Hz over 2 s), float32, the first n samples of 2 s."""
    rng = np.random.RandomState(seed)
    t = np.arange(32000) / 16000.0
    phase = 2 * np.pi * (200.0 * t + 0.5 * (3800.0 - 200.0) / 2.0 * t * t)
    x = 0.1 * rng.randn(32000) + 0.3 * np.sin(phase)
    return x[:n].astype(np.float32)


def mel_oracle(wav, return_linear=False):
    """float64 (80, T), T = 1 + n // 200: pre-emphasis 0.97, centred zero-padded STFT (n_fft =
    win 800, hop 200, periodic Hann), magnitude, syncnet.mel_filters(), 20 log10(max(1e-5, .))
    - 20, clip(8 (S + 100) / 100 - 4, -4, 4).  return_linear: also the linear mel values."""
    x = np.asarray(wav, dtype=np.float64)
    n = x.size
    y = np.concatenate([x[:1], x[1:] - 0.97 * x[:-1]])
    y = np.concatenate([np.zeros(400), y, np.zeros(400)])
    T = 1 + n // 200
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(800) / 800.0)
    frames = np.stack([y[t * 200:t * 200 + 800] for t in range(T)]) * win
    mag = np.abs(np.fft.rfft(frames, axis=1))  # (T, 401)
    lin = syncnet.mel_filters().astype(np.float64) @ mag.T
    S = 20.0 * np.log10(np.maximum(1e-5, lin)) - 20.0
    out = np.clip(8.0 * ((S + 100.0) / 100.0) - 4.0, -4.0, 4.0)
    return (out, lin) if return_linear else out
