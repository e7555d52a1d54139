"""Host side of the classic SyncNet evaluation (latentsync_amd/synceval.py) and the tests' own
oracles (tests/synceval_ref.py): no GPU needed."""
import math

import numpy as np
import pytest
import torch

import synceval_ref as R
from conftest import golden
from latentsync_amd import synceval
from latentsync_amd.packing import pack_weight_general, unpack_weight_general

# max |bf16 restatement - golden| / RMS(golden), measured on the CPU; the device is allowed 2 x
# (tests/test_gpu_synceval_model.py imports this table)
REF_ERR = {
    "A": dict(lip=[0.0225, 0.0363, 0.0504, 0.0728, 0.0999, 0.0985, 0.151],
              aud=[0.0192, 0.0258, 0.047, 0.0552, 0.0624, 0.0761, 0.0705],
              im_feat=0.0192, cc_feat=0.0152, dists=0.0013, mean_dists=0.000465),
    "B": dict(lip=[0.0274, 0.0528, 0.0642, 0.0764, 0.0912, 0.109, 0.125],
              aud=[0.0196, 0.0276, 0.0358, 0.0442, 0.0598, 0.0466, 0.0617],
              im_feat=0.0151, cc_feat=0.0105, dists=0.000663, mean_dists=0.000358),
}


def ref_err(name, label):
    e = REF_ERR[name]
    if label.startswith(("lip_stage_", "aud_stage_")):
        return e[label[:3]][int(label.rsplit("_", 1)[1])]
    return e[label]


# ---------------------------------------------------------------- MFCC oracle
@pytest.mark.parametrize("n,frames", ((1, 1), (400, 1), (401, 2), (560, 2), (561, 3), (8000, 49)))
def test_mfcc_frame_count(n, frames):
    assert R.mfcc_frames(n) == synceval.mfcc_frames(n) == frames
    mf, ok = R.mfcc_oracle(np.ones(n))
    assert mf.shape == ok.shape == (13, frames)


def test_mfcc_silence_hits_the_epsilon_floor():
    mf, ok = R.mfcc_oracle(np.zeros(800))
    eps = np.finfo(float).eps
    assert np.allclose(mf[0], math.log(eps), rtol=0, atol=1e-12)          # log(frame energy floor)
    assert np.abs(mf[1:]).max() < 1e-9                                     # the DCT of a constant: only c0
    assert ok.all()


def test_mfcc_filterbank_is_the_librarys_shape():
    fb = R.mfcc_filterbank()
    assert fb.shape == (26, 257) and np.array_equal(fb.astype(np.float32), synceval.mfcc_filters())
    assert fb.min() >= 0 and fb.max() <= 1.0
    peaks = fb.argmax(1)
    assert (np.diff(peaks) > 0).all()                                      # centres ascend
    mel = np.linspace(0, 2595 * math.log10(1 + 8000 / 700), 28)
    hz = 700 * (10 ** (mel / 2595) - 1)
    assert np.array_equal(peaks, np.floor(513 * hz[1:27] / 16000).astype(int))


def test_mfcc_single_bin_tone_lands_in_its_filter():
    """A tone on the FFT bin where filter 12's triangle peaks.  The frame is 400 of the 512
    samples, so the bin leaks into its neighbours, but filter 12 still holds the largest
    filterbank energy, and the coefficients are the liftered DCT of the log energies."""
    n, filt = 400, 12
    kbin = int(R.mfcc_filterbank()[filt].argmax())
    x = 1000.0 * np.sin(2 * np.pi * kbin * np.arange(n) / 512.0)  # x[0] = 0: no pre-emphasis start step
    y = np.concatenate([x[:1], x[1:] - 0.97 * x[:-1]])
    power = np.abs(np.fft.rfft(y, 512)) ** 2 / 512
    fb = R.mfcc_filterbank() @ power
    assert abs(int(power.argmax()) - kbin) <= 1
    assert int(fb.argmax()) == filt
    mf, ok = R.mfcc_oracle(x)
    assert ok.all()
    assert abs(mf[0, 0] - math.log(power.sum())) < 1e-9
    # coefficients 1..12 are the liftered orthonormal DCT-II of log(fb)
    m, k = np.arange(26), np.arange(1, 13)
    want = (np.cos(np.pi * k[:, None] * (2 * m[None] + 1) / 52) * math.sqrt(2 / 26)) @ np.log(fb)
    want = want * (1 + 11 * np.sin(np.pi * k / 22))
    assert np.allclose(mf[1:, 0], want, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name", tuple(R.CASES))
def test_oracle_skips_nothing_on_the_test_signals(name):
    for n in (400, 401, 560, 561, 8000):
        _, ok = R.mfcc_oracle(R.mfcc_test_signal(n))
        assert ok.all(), n
    _, ok = R.mfcc_oracle(R.pcm16(R.case_audio(name)))
    assert ok.all()


# ---------------------------------------------------------------- plans
def test_window_plan():
    assert synceval.window_plan(12, 7680) == 7
    assert synceval.window_plan(7, 4480) == 2
    assert synceval.window_plan(100, 6 * 640) == 1        # the audio is the shorter one
    assert synceval.window_plan(6, 6 * 640 + 639) == 1
    for frames, samples in ((5, 64000), (6, 6 * 640 - 1), (0, 0)):
        with pytest.raises(ValueError, match="at least 6"):
            synceval.window_plan(frames, samples)


def test_offset_from_means():
    m = np.array([5.0, 3.0, 1.0, 4.0, 2.0], dtype=np.float32)
    assert synceval.offset_from_means(m, 2) == (0, 1.0, 2.0)              # median 3
    m4 = torch.tensor([4.0, 1.0, 3.0, 2.0, 6.0, 5.0, 7.0])               # vshift 3, argmin 1 -> offset 2
    off, mn, conf = synceval.offset_from_means(m4.numpy(), 3)
    assert (off, mn) == (2, 1.0) and conf == float(torch.median(m4) - m4.min())
    # torch's median of an even count is the LOWER middle; an odd window never has one, but the
    # rule must be torch's: check on the helper's own sort
    even = torch.tensor([1.0, 2.0, 3.0, 4.0])
    assert float(torch.median(even)) == 2.0 == float(np.sort(even.numpy())[(4 - 1) // 2])
    tie = np.array([2.0, 1.0, 1.0], dtype=np.float32)                     # the first minimum, as torch.min
    assert synceval.offset_from_means(tie, 1)[0] == 1 - int(torch.min(torch.from_numpy(tie), 0)[1])
    with pytest.raises(ValueError):
        synceval.offset_from_means(m, 3)


def test_pcm16():
    a = torch.tensor([0.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -1.0, 0.99999, 1.5, -2.0])
    assert synceval.pcm16(a).tolist() == [0.0, 0.0, 2.0, 2.0, -32768.0, 32767.0, 32767.0, -32768.0]
    x = R.case_audio("A")
    assert np.array_equal(synceval.pcm16(x).numpy().astype(np.float64), R.pcm16(x))


# ---------------------------------------------------------------- weights
def test_state_dict_keys_equal_the_goldens():
    keys = list(synceval.param_shapes())
    for name in R.CASES:
        assert keys == [str(k) for k in golden(f"synceval_{name}.npz")["keys"]]
    net = synceval.SyncNetEval()
    sd = R.case_weights("B")
    assert list(net.load_state_dict(sd).state_dict()) == keys
    bad = dict(sd)
    del bad["netfclip.3.bias"]
    with pytest.raises(RuntimeError, match="missing"):
        net.load_state_dict(bad)
    with pytest.raises(RuntimeError, match="device only"):
        net.evaluate(frames=torch.zeros(6, 224, 224, 3, dtype=torch.uint8), audio=torch.zeros(6 * 640))


def test_load_parameters_round_trip(tmp_path):
    sd = R.case_weights("B")
    p = tmp_path / "syncnet_v2.model"
    torch.save(sd, p)
    net = synceval.SyncNetEval(device="cpu")
    net.loadParameters(str(p))
    got = net.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_batchnorm_fold_against_torch_fp64():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 9, 8, generator=g, dtype=torch.float64)
    w, b = torch.randn(7, 5, 3, 3, generator=g), torch.randn(7, generator=g)
    gamma, beta, mean = torch.randn(7, generator=g), torch.randn(7, generator=g), torch.randn(7, generator=g)
    var = torch.rand(7, generator=g) + 0.05
    ref = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, w.double(), b.double(), padding=1),
                                         mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    wf, bf = synceval.fold_batchnorm(w, b, gamma, beta, mean, var)
    assert wf.dtype == bf.dtype == torch.float32
    got = torch.nn.functional.conv2d(x, wf.double(), bf.double(), padding=1)
    # the fold is 4 fp32 operations per weight / bias: 2^-21 of the magnitude sum
    mag = torch.nn.functional.conv2d(x.abs(), wf.double().abs(), bf.double().abs(), padding=1)
    assert bool(((got - ref).abs() <= 2.0 ** -21 * mag + 1e-12).all())
    # a linear folds the same way
    wl, bl = synceval.fold_batchnorm(w[:, :, 0, 0], b, gamma, beta, mean, var)
    assert torch.equal(wl, wf[:, :, 0, 0]) and torch.equal(bl, bf)


def test_packer_k_order_round_trip():
    g = torch.Generator().manual_seed(5)
    for shape, cin_pad in (((6, 3, 5, 7, 7), 8), ((4, 96, 1, 5, 5), None), ((5, 16, 5, 4), None), ((3, 512), None)):
        w = torch.randn(*shape, generator=g)
        p = pack_weight_general(w, cin_pad)
        w5 = w if w.dim() == 5 else (w[:, :, None] if w.dim() == 4 else w[:, :, None, None, None])
        O, I, kt, kh, kw = w5.shape
        ip = cin_pad or (I + 7) // 8 * 8
        assert p.shape == (O, (kt * kh * kw * ip + 63) // 64 * 64)
        for (o, it, iy, ix, ci) in ((0, 0, 0, 0, 0), (O - 1, kt - 1, kh - 1, kw - 1, I - 1), (1, kt // 2, kh // 2, 0, I // 2)):
            assert p[o, ((it * kh + iy) * kw + ix) * ip + ci] == w5[o, ci, it, iy, ix]
        assert torch.equal(unpack_weight_general(p, I, (kt, kh, kw), cin_pad), w5)
        assert float(p.abs().sum()) == pytest.approx(float(w.abs().sum()), rel=1e-5)  # the padding is zero


# ---------------------------------------------------------------- crop plan
def test_crop_plan_medfilt_edges_and_integer_crop():
    from scipy.signal import medfilt
    n = 20
    rng = np.random.RandomState(0)
    boxes = np.stack([100 + rng.rand(n) * 6, 80 + rng.rand(n) * 6, 180 + rng.rand(n) * 6, 170 + rng.rand(n) * 6], 1)
    plan = synceval.crop_plan(boxes, 0.4)
    s = medfilt(np.maximum(boxes[:, 3] - boxes[:, 1], boxes[:, 2] - boxes[:, 0]) / 2, 13)
    cx, cy = medfilt((boxes[:, 0] + boxes[:, 2]) / 2, 13), medfilt((boxes[:, 1] + boxes[:, 3]) / 2, 13)
    # scipy's medfilt pads with zeros: the first 6 and last 6 values are pulled towards 0
    assert s[0] <= np.median(np.maximum(boxes[:7, 3] - boxes[:7, 1], boxes[:7, 2] - boxes[:7, 0]) / 2)
    for i in (0, 5, 10, n - 1):
        bs, bsi = s[i], int(s[i] * 1.8)
        my, mx = cy[i] + bsi, cx[i] + bsi
        assert plan[i].tolist() == [int(my - bs), int(my + bs * 1.8), int(mx - bs * 1.4), int(mx + bs * 1.4), bsi]
    # a short track: the zero padding wins the median everywhere -> an empty crop is refused
    with pytest.raises(ValueError, match="do not lie|degenerate"):
        synceval._check_plan(synceval.crop_plan(boxes[:5]), 300, 300)


def test_crop_plan_nan_rows():
    n = 30
    boxes = np.tile(np.array([[50.0, 40.0, 110.0, 100.0]]), (n, 1)) + np.arange(n)[:, None]
    holed = boxes.copy()
    holed[[7, 8, 15]] = np.nan
    assert np.array_equal(synceval.crop_plan(holed), synceval.crop_plan(boxes))  # linear track: exact
    for bad in (0, n - 1):
        h = boxes.copy()
        h[bad] = np.nan
        with pytest.raises(ValueError, match="first and the last"):
            synceval.crop_plan(h)
    h = boxes.copy()
    h[3, 1] = np.nan
    with pytest.raises(ValueError, match="all numbers or all NaN"):
        synceval.crop_plan(h)
    with pytest.raises(ValueError):
        synceval.crop_plan(np.zeros((4, 3)))


def test_resize_restatement_hand_cases():
    # identity size: every coefficient is (2048, 0)
    img = np.random.RandomState(1).randint(0, 256, (224, 224, 3)).astype(np.uint8)
    assert np.array_equal(R.resize_linear_u8(img, 224, 224), img)
    # a constant image stays constant through both rounding passes, upscaled or downscaled
    for h, w in ((37, 51), (300, 260), (448, 300)):
        assert np.array_equal(R.resize_linear_u8(np.full((h, w, 3), 110, np.uint8), 224, 224),
                              np.full((224, 224, 3), 110, np.uint8))
    # exactly twice the target: the 2 x 2 area mean, rounded half up
    big = np.random.RandomState(2).randint(0, 256, (448, 448, 3)).astype(np.uint8)
    want = (big.astype(int).reshape(224, 2, 224, 2, 3).sum((1, 3)) + 2) >> 2
    assert np.array_equal(R.resize_linear_u8(big, 224, 224), want.astype(np.uint8))
    # x2 upscale of a 2-pixel ramp: weights 0.25 / 0.75 in 11-bit fixed point
    ramp = np.array([[[0], [200]]], np.uint8)
    up = R.resize_linear_u8(ramp, 1, 4)[0, :, 0]
    assert up.tolist() == [0, 50, 150, 200]


# ---------------------------------------------------------------- the bf16 restatement
@pytest.mark.parametrize("name", tuple(R.CASES))
def test_bf16_restatement_against_golden(name):
    """Measures REF_ERR: the error of the bf16-rounding restatement against the reference's fp32
    golden, per tensor; the GPU test allows the device twice that.  The fp32 restatement must
    reproduce the golden to fp32 accuracy, which pins the restatement's structure."""
    g = golden(f"synceval_{name}.npz")
    c = R.CASES[name]
    imtv, mf, last = R.case_network_inputs(name)
    assert last == int(g["lastframe"]) and c["vshift"] == int(g["vshift"])
    sd = R.case_weights(name)
    for bf16 in (False, True):
        o = R.forward(sd, imtv, mf, last, bf16=bf16)
        d, m = R.pdist(o["im_feat"], o["cc_feat"], c["vshift"])
        errs = R.golden_errors(g, o["lip"], o["aud"], o["im_feat"], o["cc_feat"], d, m)
        for label, e in errs.items():
            print(f"{name} bf16={bf16} {label}: err / rms {e:.3g}")
            if bf16:
                want = ref_err(name, label)
                assert 0.5 * want <= e <= 1.05 * want, (label, e, want)  # REF_ERR is this figure
            else:
                assert e < 1e-4, (label, e)
        off = synceval.offset_from_means(m.float().numpy(), c["vshift"])
        assert off[0] == int(g["av_offset"])
        assert abs(off[1] - float(g["min_dist"])) <= 1e-2 * float(g["min_dist"])
        assert abs(off[2] - float(g["conf"])) <= 1e-2 * float(g["conf"])
    # the golden's own results follow from its mean_dists by the host rule
    assert synceval.offset_from_means(g["mean_dists"], c["vshift"]) == \
        (int(g["av_offset"]), pytest.approx(float(g["min_dist"])), pytest.approx(float(g["conf"]), rel=1e-5))
