"""The classic SyncNet on the device against the reference's fp32 golden (tests/golden/
synceval_*.npz, tests/make_synceval_golden.py): every conv / BN / ReLU stage of both towers,
both feature sets, dists, mean_dists and the three results.

Tolerance, per tensor, as max |got - golden| / RMS(golden): the error of the bf16-rounding
restatement (synceval_ref.forward(bf16=True), CPU) against the same golden is REF_ERR
(tests/test_synceval_host.py measures and pins it on the CPU); the device rounds at the same
points and only its accumulation order differs, so it is allowed 2 x that figure -- the rule of
tests/test_gpu_syncnet_model.py.  The device also computes its own MFCC (ls_mfcc) where the
golden was fed the float64 oracle's; both are rounded to bf16 at the tower's input."""
import numpy as np
import pytest
import torch

import synceval_ref as R
from conftest import golden
from latentsync_amd import synceval
from test_synceval_host import REF_ERR, ref_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEVICE_FACTOR = 2.0


def device_net(name):
    net = synceval.SyncNetEval()
    net.load_state_dict(R.case_weights(name))
    return net.to(DEV).eval()


@pytest.mark.parametrize("name", tuple(R.CASES))
def test_model_matches_golden(gpu, name):
    g = golden(f"synceval_{name}.npz")
    c = R.CASES[name]
    # the av_offset assertion means something only if the minimum is clear of the allowance
    md = np.sort(g["mean_dists"].astype(np.float64))
    rms = float(np.sqrt((md ** 2).mean()))
    allowance = DEVICE_FACTOR * REF_ERR[name]["mean_dists"] * rms
    assert md[1] - md[0] > 4 * allowance, (md[1] - md[0], allowance)

    net = device_net(name)
    frames, audio = R.case_frames(name).to(DEV), torch.from_numpy(R.case_audio(name))
    details = {}
    result = net.evaluate(frames=frames, audio=audio, vshift=c["vshift"], details=details)
    taps = {}
    im, cc = net.features(frames, synceval.pcm16(audio).to(DEV), taps=taps)
    torch.cuda.synchronize()
    assert torch.equal(im, details["im_feat"]) and torch.equal(cc, details["cc_feat"])
    nchw = lambda ts: [t.permute(0, 3, 1, 2).float() if t.dim() == 4 else t.float() for t in ts]
    lip, aud = nchw(taps["lip"]), nchw(taps["aud"])
    lip[6], aud[6] = lip[6].reshape(lip[6].shape[0], -1), aud[6].reshape(aud[6].shape[0], -1)
    errs = R.golden_errors(g, lip, aud, im, cc, details["dists"], details["mean_dists"])
    fails = []
    for label, e in errs.items():
        allowed = DEVICE_FACTOR * ref_err(name, label)
        print(f"{name} {label}: err / rms {e:.4g} (restatement {ref_err(name, label):.4g}, allowed {allowed:.4g})")
        if not (np.isfinite(e) and e <= allowed):
            fails.append((label, e, allowed))
    assert not fails, fails
    assert result[0] == int(g["av_offset"])
    assert abs(result[1] - float(g["min_dist"])) <= allowance
    assert abs(result[2] - float(g["conf"])) <= 2 * allowance
    assert isinstance(result[0], int) and isinstance(result[1], float) and isinstance(result[2], float)

    # the reference's NCDHW / NCHW interface gives the same features as the clip-wide path, bit for bit
    last = int(g["lastframe"])
    imtv = frames.flip(-1).permute(3, 0, 1, 2)[None].float()
    im_in = torch.cat([imtv[:, :, i:i + 5] for i in range(last)], 0)
    mf = taps["mfcc"]
    cc_in = torch.stack([mf[:, 4 * i:4 * i + 20] for i in range(last)])[:, None]
    im2, cc2 = net.forward_lip(im_in), net.forward_aud(cc_in)
    torch.cuda.synchronize()
    assert im2.dtype == torch.float32 and tuple(im2.shape) == tuple(g["im_feat"].shape)
    assert torch.equal(im2, im) and torch.equal(cc2, cc)
    feat = net.forward_lipfeat(im_in[:2])
    assert tuple(feat.shape) == (2, 512) and torch.equal(feat, taps["lip"][5].reshape(last, 512)[:2].float())


def test_evaluate_refusals(gpu):
    net = device_net("B")
    frames = R.case_frames("B").to(DEV)
    audio = torch.from_numpy(R.case_audio("B"))
    with pytest.raises(ValueError, match="at least 6"):
        net.evaluate(frames=frames[:5], audio=audio)
    with pytest.raises(ValueError, match="at least 6"):
        net.evaluate(frames=frames, audio=audio[:5 * 640])
    with pytest.raises(ValueError, match="either"):
        net.evaluate()
    with pytest.raises(ValueError, match="audio"):
        net.evaluate(frames=frames)
    with pytest.raises(ValueError, match="224"):
        net.evaluate(frames=frames[:, :200], audio=audio)
    # another sample rate goes through the device resampler and still yields a result
    a8 = audio[::2].contiguous()
    off, mn, conf = net.evaluate(frames=frames, audio=a8, sample_rate=8000, vshift=2)
    assert isinstance(off, int) and np.isfinite(mn) and np.isfinite(conf)
