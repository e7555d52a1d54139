"""The project's own restatement of the classic SyncNet evaluation, for the tests.

  * mfcc_oracle(x): python_speech_features.mfcc(x, 16000) with its defaults, float64 numpy, from
    the library's definition (the library is not a dependency: parity with it is unpinned), plus a
    mask of the elements whose conditioning allows a judgement of an fp32 implementation.
  * forward(sd, frames_bgr, mfcc, bf16=False): S (eval/syncnet/syncnet.py) in fp32 torch on the
    CPU from a reference-named state dict.  bf16=True folds each eval-mode BatchNorm into its
    conv / linear in fp32, rounds the folded weight to bf16 once and rounds to bf16 wherever the
    device path stores bf16 (the inputs, every conv + ReLU output, the first linear's output);
    everything in between is fp32, so only the accumulation order differs from the device.
  * pdist(im, cc, vshift): calc_pdist and its mean in float64.
  * resize_linear_u8 / crop_video_ref: cv2.resize's default INTER_LINEAR for uint8 and
    crop_video's pad / crop / resize, restated from OpenCV's published definition (resize.cpp);
    cv2 is not a dependency: parity with it is unpinned.
  * the two cases, their seeded weights, frames and audio.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from latentsync_amd import synceval

CASES = {  # name -> frames, samples at 16 kHz, vshift, seed
    "A": dict(frames=12, samples=7680, vshift=15, seed=21),
    "B": dict(frames=7, samples=4480, vshift=2, seed=22),
}
SUBSAMPLE = 8192  # stage outputs above 2 * SUBSAMPLE elements are stored at SUBSAMPLE fixed positions
N_STAGES = 7      # six conv + BN + ReLU stages and the head's linear + BN + ReLU, per tower


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def subsample_index(numel, seed):
    if numel <= 2 * SUBSAMPLE:
        return None
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(numel, generator=g)[:SUBSAMPLE].sort().values


# ---------------------------------------------------------------- seeded weights and inputs
# (mean, variance) each layer's input is taken to have when its BatchNorm's running statistics
# are drawn: uniform 0..255 pixels; the MFCC of case_audio (coefficient 0 near 17, the others
# within a few tens); ReLU of a unit normal (0.40, 0.34); a 3 x 3 max-pool of those (1.3, 0.4).
_RELU, _POOL = (0.40, 0.34), (1.3, 0.4)
_MOMENTS = {
    "netcnnlip": {0: (127.5, 5461.25), 4: _POOL, 8: _POOL, 11: _RELU, 14: _RELU, 18: _POOL},
    "netcnnaud": {0: (0.0, 150.0), 4: _RELU, 8: _POOL, 11: _RELU, 14: _RELU, 18: _POOL},
}
HEAD_BIAS_SCALE = 8.0


def case_weights(name):
    """The seeded state dict of a case.  Conv / linear weights N(0, 2 / fan_in); BatchNorm gamma
    1 + 0.1 N, beta 0.1 N, running_mean = b + m sum(w) and running_var = v sum(w^2) for the
    input moments (m, v) above, so every stage comes out near unit scale with about half of
    its ReLU outputs alive.  Both heads' last bias is the SAME vector 8 N(0, 1): real feature
    rows then lie close together and far from calc_pdist's zero rows, which gives mean_dists a
    clear minimum (at full overlap) for the av_offset assertion to mean something."""
    seed = CASES[name]["seed"]
    g = torch.Generator().manual_seed(seed)
    shapes = synceval.param_shapes()
    sd = {}
    rn = lambda *s: torch.randn(*s, generator=g)
    common = HEAD_BIAS_SCALE * rn(shapes["netfcaud.3.bias"][0])
    for k, s in shapes.items():
        if not k.endswith(".weight") or len(s) < 2:
            continue
        p = k[:-len(".weight")]
        tower, idx = p.split(".")
        idx = int(idx)
        fan_in = int(np.prod(s[1:]))
        w = rn(*s) * math.sqrt(2.0 / fan_in)
        b = 0.1 * rn(s[0])
        sd[k], sd[p + ".bias"] = w, b
        if tower.startswith("netfc") and idx == 3:
            sd[p + ".bias"] = common.clone()
            continue
        m, v = _MOMENTS[tower][idx] if tower in _MOMENTS else _RELU
        q = f"{tower}.{idx + 1}"
        flat = w.reshape(s[0], -1)
        sd[q + ".weight"] = 1.0 + 0.1 * rn(s[0])
        sd[q + ".bias"] = 0.1 * rn(s[0])
        sd[q + ".running_mean"] = b + m * flat.sum(1)
        sd[q + ".running_var"] = v * (flat * flat).sum(1)
        sd[q + ".num_batches_tracked"] = torch.tensor(1, dtype=torch.int64)
    return {k: sd[k] for k in shapes}


def case_audio(name):
    """Float mono samples in [-1, 1) at 16 kHz: 0.05 N(0,1) + 0.3 chirp(200 -> 3800 Hz over 2 s)."""
    c = CASES[name]
    rng = np.random.RandomState(c["seed"])
    t = np.arange(c["samples"]) / 16000.0
    phase = 2 * np.pi * (200.0 * t + 0.5 * (3800.0 - 200.0) / 2.0 * t * t)
    return (0.05 * rng.randn(c["samples"]) + 0.3 * np.sin(phase)).astype(np.float32)


def case_frames(name):
    """uint8 (n, 224, 224, 3) RGB, uniform random."""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + c["seed"])
    return torch.randint(0, 256, (c["frames"], 224, 224, 3), generator=g, dtype=torch.uint8)


def pcm16(audio):
    """numpy: x 32768, rounded to nearest even, clipped to int16 -- synceval.pcm16 in float64."""
    return np.clip(np.rint(np.asarray(audio, dtype=np.float64) * 32768.0), -32768, 32767)


def case_network_inputs(name):
    """(imtv (1, 3, n, 224, 224) fp32 B, G, R as syncnet_eval.py builds it, mfcc float64 (13, T),
    lastframe)."""
    frames, audio = case_frames(name), pcm16(case_audio(name))
    mf, ok = mfcc_oracle(audio)
    assert ok.all()
    imtv = frames.flip(-1).permute(3, 0, 1, 2)[None].float()
    return imtv, mf, synceval.window_plan(frames.shape[0], audio.size)


# ---------------------------------------------------------------- MFCC, float64
def mfcc_frames(n):
    return 1 + int(math.ceil((n - 400) / 160.0)) if n > 400 else 1


def mfcc_filterbank():
    """float64 (26, 257): get_filterbanks(26, 512, 16000, 0, 8000)."""
    mel = np.linspace(0.0, 2595.0 * np.log10(1.0 + 8000.0 / 700.0), 28)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    b = np.floor(513 * hz / 16000.0)
    fb = np.zeros((26, 257))
    for j in range(26):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def mfcc_oracle(x, tol=2.0 ** -9):
    """-> (mfcc float64 (13, T), ok bool (13, T)).  x: samples on the int16 scale.

    ok marks the elements an fp32 implementation can be judged on at |got - ref| <= tol max(1,
    |ref|).  An fp32 direct DFT of 400 terms carries independent roundings (one per fma, one per
    twiddle, one for the pre-emphasis), each 2^-24 relative: the spectrum value X_k is off by
    about e = 2^-24 sqrt(sum y^2) (sqrt(400) + 2) at one sigma; 4 e is taken.  The power moves
    by (2 |X_k| 4e + 16 e^2) / 512, a filterbank energy by the filter's weighted sum of those,
    its log by that over the energy, and a coefficient by the root-sum-square of its DCT row
    times those (independent across filters) times the lifter.  An element whose figure exceeds
    tol max(1, |ref|) / 2 is too ill-conditioned to judge (log of a near-floor energy)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    y = np.concatenate([x[:1], x[1:] - 0.97 * x[:-1]])
    T = mfcc_frames(n)
    y = np.concatenate([y, np.zeros((T - 1) * 160 + 400 - n)]) if (T - 1) * 160 + 400 > n else y
    frames = np.stack([y[t * 160:t * 160 + 400] for t in range(T)])
    spec = np.fft.rfft(frames, 512, axis=1)
    power = (spec.real ** 2 + spec.imag ** 2) / 512.0
    energy = power.sum(1)
    energy_f = np.where(energy == 0, np.finfo(float).eps, energy)
    fbm = mfcc_filterbank()
    fb = power @ fbm.T
    fb_f = np.where(fb == 0, np.finfo(float).eps, fb)
    logfb = np.log(fb_f)
    m = np.arange(26)
    k = np.arange(13)
    dct = np.cos(np.pi * k[:, None] * (2 * m[None, :] + 1) / 52.0) * math.sqrt(2.0 / 26)
    dct[0] = math.sqrt(1.0 / 26)
    lift = 1 + 11.0 * np.sin(np.pi * k / 22.0)
    feat = (logfb @ dct.T) * lift
    feat[:, 0] = np.log(energy_f)
    # conditioning
    e4 = 4 * 2.0 ** -24 * np.sqrt((frames ** 2).sum(1)) * (math.sqrt(400) + 2)
    perr = (2 * np.abs(spec) * e4[:, None] + e4[:, None] ** 2) / 512.0
    log_err = (perr @ fbm.T) / fb_f
    cerr = np.sqrt((log_err ** 2) @ (dct.T ** 2)) * lift
    cerr[:, 0] = perr.sum(1) / energy_f
    # a floored energy is exact on both sides (0 -> eps): nothing to amplify
    cerr[:, 0] = np.where(energy == 0, 0.0, cerr[:, 0])
    silent = (fb == 0).all(1)
    cerr[silent, 1:] = 0.0
    ok = cerr <= tol * np.maximum(1.0, np.abs(feat)) / 2
    return feat.T.copy(), ok.T.copy()


def mfcc_test_signal(n, seed=3):
    """The first n of 8000 samples on the int16 scale: a chirp (200 -> 7000 Hz, amplitude 2000)
    plus noise that is white AFTER the pre-emphasis (500 N(0,1) through 1 / (1 - 0.97 z^-1)), so
    that every filter is energised at a level the fp32 DFT resolves: plain white noise leaves the
    lowest filters, which the pre-emphasis attenuates 30-fold, below what mfcc_oracle can judge."""
    rng = np.random.RandomState(seed)
    t = np.arange(8000) / 16000.0
    phase = 2 * np.pi * (200.0 * t + 0.5 * (7000.0 - 200.0) / 0.5 * t * t)
    w = 500.0 * rng.randn(8000)
    for i in range(1, 8000):
        w[i] += 0.97 * w[i - 1]
    return np.clip(np.rint(w + 2000.0 * np.sin(phase)), -32768, 32767)[:n]


# ---------------------------------------------------------------- the network
def _bn(sd, p):
    return sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"]


def _fold(w, b, gamma, beta, mean, var, eps=1e-5):
    s = gamma / torch.sqrt(var + eps)
    return w * s.reshape((-1,) + (1,) * (w.dim() - 1)), (b - mean) * s + beta


def _tower(sd, cnn, fc, spec, x, bf16, stages):
    """x (B, C, H, W) (the lip tower's first conv is applied by the caller)."""
    r = bf16_round if bf16 else (lambda t: t)
    i = 0
    for s in spec:
        if s[0] == "pool":
            if s[1] != (1, 1):
                x = F.max_pool2d(x, s[1], s[2], s[3])
            i += 1
            continue
        _, cin, cout, win, stride, pad = s
        w, b = sd[f"{cnn}.{i}.weight"], sd[f"{cnn}.{i}.bias"]
        if w.dim() == 5 and win[0] == 1:
            w = w[:, :, 0]
        if win[0] == 1:
            if bf16:
                wf, bfold = _fold(w, b, *_bn(sd, f"{cnn}.{i + 1}"))
                x = r(F.relu(F.conv2d(x, r(wf), bfold, stride=stride, padding=pad)))
            else:
                g, be, mu, var = _bn(sd, f"{cnn}.{i + 1}")
                x = F.relu(F.batch_norm(F.conv2d(x, w, b, stride=stride, padding=pad), mu, var, g, be, False, 0.0, 1e-5))
        else:  # the 5 x 7 x 7 conv over the whole clip: x (1, 3, n, H, W) -> (n - 4, 96, Ho, Wo)
            if bf16:
                wf, bfold = _fold(w, b, *_bn(sd, f"{cnn}.{i + 1}"))
                y = F.conv3d(x, r(wf), bfold, stride=(1,) + tuple(stride))
            else:
                g, be, mu, var = _bn(sd, f"{cnn}.{i + 1}")
                y = F.batch_norm(F.conv3d(x, w, b, stride=(1,) + tuple(stride)), mu, var, g, be, False, 0.0, 1e-5)
            x = r(F.relu(y[0].permute(1, 0, 2, 3)))
        stages.append(x)
        i += 3
    x = x.reshape(x.shape[0], -1)
    w, b = sd[fc + ".0.weight"], sd[fc + ".0.bias"]
    if bf16:
        wf, bfold = _fold(w, b, *_bn(sd, fc + ".1"))
        x = r(F.relu(F.linear(x, r(wf), bfold)))
        stages.append(x)
        return F.linear(x, r(sd[fc + ".3.weight"]), sd[fc + ".3.bias"])
    g, be, mu, var = _bn(sd, fc + ".1")
    x = F.relu(F.batch_norm(F.linear(x, w, b), mu, var, g, be, False, 0.0, 1e-5))
    stages.append(x)
    return F.linear(x, sd[fc + ".3.weight"], sd[fc + ".3.bias"])


@torch.no_grad()
def forward(sd, imtv, mfcc, lastframe, bf16=False):
    """imtv (1, 3, n, 224, 224) fp32 B, G, R; mfcc (13, T) -> dict(lip=[7 stage outputs, NCHW with
    one image per window], aud=[7], im_feat, cc_feat (lastframe, D))."""
    sd = {k: v.float() for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    r = bf16_round if bf16 else (lambda t: t)
    lip, aud = [], []
    im = _tower(sd, "netcnnlip", "netfclip", synceval._LIP, r(imtv[:, :, :lastframe + 4].float()), bf16, lip)
    mf = torch.as_tensor(np.asarray(mfcc)).float()
    win = torch.stack([mf[:, 4 * i:4 * i + 20] for i in range(lastframe)])[:, None]
    cc = _tower(sd, "netcnnaud", "netfcaud", synceval._AUD, r(win), bf16, aud)
    return dict(lip=lip, aud=aud, im_feat=im, cc_feat=cc)


def pdist(im, cc, vshift):
    """calc_pdist + mean in float64: (dists (n, 2 vshift + 1), mean_dists)."""
    im, cc = torch.as_tensor(im).double(), torch.as_tensor(cc).double()
    n, D = im.shape
    ccp = torch.cat([torch.zeros(vshift, D, dtype=torch.float64), cc, torch.zeros(vshift, D, dtype=torch.float64)])
    win = 2 * vshift + 1
    d = torch.stack([((im[i][None] - ccp[i:i + win] + 1e-6) ** 2).sum(1).sqrt() for i in range(n)])
    return d, d.mean(0)


# ---------------------------------------------------------------- cv2.resize, crop_video
def _linear_table(dst, src, horizontal):
    """OpenCV's INTER_LINEAR table for one axis: (index, 11-bit weights w0, w1)."""
    scale = 1.0 / (float(dst) / float(src))
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


def resize_linear_u8(img, dh, dw):
    """cv2.resize(img, (dw, dh)) for uint8 (H, W, C): INTER_LINEAR in 11-bit fixed point --
    the horizontal pass S0 w0 + S1 w1 in int32, the vertical pass ((b0 (r0 >> 4)) >> 16) +
    ((b1 (r1 >> 4)) >> 16) + 2 >> 2 -- and, for a source exactly twice the target on both axes,
    the 2 x 2 area mean (sum + 2) >> 2 that cv2 switches to."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    s = img.astype(np.int64)
    if H == 2 * dh and W == 2 * dw:
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xi, xw = _linear_table(dw, W, True)
    yi, yw = _linear_table(dh, H, False)
    x1 = np.minimum(xi + 1, W - 1)
    rows = s[:, xi] * xw[:, 0][None, :, None] + s[:, x1] * xw[:, 1][None, :, None]
    y0, y1 = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
    out = (((yw[:, 0][:, None, None] * (rows[y0] >> 4)) >> 16) + ((yw[:, 1][:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def crop_video_ref(frames, plan):
    """frames uint8 (n, H, W, 3), plan (n, 5) (y0, y1, x0, x1, bsi) -> (n, 224, 224, 3): np.pad
    with 110, the slice, resize_linear_u8."""
    out = []
    for f, (y0, y1, x0, x1, bsi) in zip(np.asarray(frames), np.asarray(plan).tolist()):
        p = np.pad(f, ((bsi, bsi), (bsi, bsi), (0, 0)), "constant", constant_values=110)
        out.append(resize_linear_u8(p[y0:y1, x0:x1], 224, 224))
    return np.stack(out)


# ---------------------------------------------------------------- comparing with a golden
def golden_errors(g, lip, aud, im_feat, cc_feat, dists, mean_dists):
    """{label: max |got - golden| / RMS(golden)} for the 14 stage outputs (NCHW, one image per
    window), both feature sets, dists and mean_dists against a synceval_*.npz fixture."""
    errs = {}

    def put(label, got, ref, rms):
        got, ref = torch.as_tensor(got).double().cpu().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
        assert got.shape == ref.shape, (label, got.shape, ref.shape)
        errs[label] = float((got - ref).abs().max()) / rms

    for tower, stages in (("lip", lip), ("aud", aud)):
        assert len(stages) == N_STAGES, (tower, len(stages))
        for j, t in enumerate(stages):
            label = f"{tower}_stage_{j}"
            assert tuple(t.shape) == tuple(g[label + "_shape"]), (label, tuple(t.shape), tuple(g[label + "_shape"]))
            flat = torch.as_tensor(t).reshape(-1).cpu()
            if label + "_idx" in g.files:
                flat = flat[torch.from_numpy(g[label + "_idx"]).long()]
            put(label, flat, g[label], float(g[label + "_rms"]))
    for label, got in (("im_feat", im_feat), ("cc_feat", cc_feat), ("dists", dists), ("mean_dists", mean_dists)):
        ref = torch.from_numpy(g[label])
        put(label, got, ref, float(ref.double().pow(2).mean().sqrt()))
    return errs
