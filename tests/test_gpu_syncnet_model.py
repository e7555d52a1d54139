"""StableSyncNet on the device against the reference's fp32 golden (tests/golden/syncnet_*.npz,
tests/make_syncnet_golden.py): every down_blocks[i] output, both embeddings and the cosine.

Tolerance, per tensor, as max |got - golden| / RMS(golden): the error of the bf16-rounding
restatement (syncnet_ref.forward(bf16=True), CPU) against the same golden is REF_ERR below; the
device rounds at the same points and only its accumulation order differs, so it is allowed
2 x that figure.  (Config A's vision embedding comes out of a GroupNorm over 2 channels at one
pixel -- a sign function of their difference -- so one bf16 rounding can flip an entry: 1.37.
Config B's embeddings come out of a GroupNorm over a single value and equal relu(beta).  Config
C ends at 128 channels, 4 per group: its embeddings and cosine depend on the input and are held
to the same rule, 0.10 and 0.07 of the RMS.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity as P
import syncnet_ref as R
from conftest import golden
from latentsync_amd import ops, syncnet

pytestmark = pytest.mark.gpu
DEV = "cuda"

# max |bf16 restatement - golden| / RMS(golden), measured on the CPU
REF_ERR = {
    "A": dict(visual=[0.0174, 0.0226, 0.0246, 0.0397, 0.0309, 0.0272],
              audio=[0.0197, 0.0215, 0.0273, 0.0275, 0.0233, 0.0203],
              vision_embeds=1.37, audio_embeds=0.00556, cosine=0.0455),
    "B": dict(visual=[0.0184, 0.0227, 0.0276, 0.0347, 0.0293, 0.0422, 0.0333, 0.0385, 0.0475, 0.0232],
              audio=[0.0172, 0.0171, 0.0194, 0.0264, 0.0286, 0.0251, 0.0354, 0.0316, 0.0208],
              vision_embeds=0.012, audio_embeds=0.0132, cosine=0.00374),
    # config C ends at 128 channels, 4 per group: its embeddings depend on the input, so they bite
    "C": dict(visual=[0.0165, 0.0229, 0.0295, 0.0259, 0.0271], audio=[0.0145, 0.0159, 0.0184],
              vision_embeds=0.0516, audio_embeds=0.0352, cosine=0.00229),
}
DEVICE_FACTOR = 2.0


def device_net(name):
    net = syncnet.StableSyncNet(R.CASES[name][0])
    net.load_state_dict(R.case_weights(name))
    return net.to(DEV).eval()


def nhwc_inputs(name):
    image, audio = R.case_inputs(name)
    vis = image.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous().to(DEV)
    aud = torch.zeros(audio.shape[0], audio.shape[2], audio.shape[3], 8, dtype=torch.bfloat16)
    aud[..., 0] = audio[:, 0].to(torch.bfloat16)
    return vis, aud.to(DEV)


@pytest.mark.parametrize("name", ("A", "B", "C"))
def test_model_matches_golden(gpu, name):
    g = golden(f"syncnet_{name}.npz")
    net = device_net(name)
    vis, aud = nhwc_inputs(name)
    taps = {}
    v, a, score = net.embed(vis, aud, taps=taps)
    torch.cuda.synchronize()
    fails = []

    def check(label, got, ref, rms, allowed):
        err = float((got.double() - ref.double()).abs().max()) / rms
        print(f"{name} {label}: err / rms {err:.4g} (restatement {allowed:.4g}, allowed {DEVICE_FACTOR * allowed:.4g})")
        if not (np.isfinite(err) and err <= DEVICE_FACTOR * allowed):
            fails.append((label, err, DEVICE_FACTOR * allowed))

    for enc in ("visual", "audio"):
        assert len(taps[enc]) == int(g[f"{enc}_n_blocks"]) == len(REF_ERR[name][enc])
        for i, t in enumerate(taps[enc]):
            got = t.permute(0, 3, 1, 2).float().cpu()
            assert tuple(got.shape) == tuple(g[f"{enc}_block_{i}_shape"])
            got = got.reshape(-1)
            if f"{enc}_block_{i}_idx" in g.files:
                got = got[torch.from_numpy(g[f"{enc}_block_{i}_idx"]).long()]
            check(f"{enc}_block_{i}", got, torch.from_numpy(g[f"{enc}_block_{i}"]), float(g[f"{enc}_block_{i}_rms"]),
                  REF_ERR[name][enc][i])
    for label, got in (("vision_embeds", v), ("audio_embeds", a), ("cosine", score)):
        ref = torch.from_numpy(g[label])
        check(label, got.cpu(), ref, float(ref.double().pow(2).mean().sqrt()), REF_ERR[name][label])
    assert not fails, fails
    # forward(): the reference's NCHW interface gives the same embeddings, bit for bit
    image, audio = R.case_inputs(name)
    v2, a2 = net(image.to(DEV), audio.to(DEV))
    assert torch.equal(v2, v) and torch.equal(a2, a)
    assert v2.dtype == torch.float32 and tuple(v2.shape) == tuple(g["vision_embeds"].shape)


@pytest.mark.parametrize("name", ("A", "B", "C"))
def test_batch_independence(gpu, name):
    """The windows of a case scored together equal each scored alone, bit for bit (every block
    output, both embeddings and the score) -- configs A and C at 3 windows, B (the real model's
    spatial sizes, where ls_conv2d's tile choice does change with the batch) at 2."""
    net = device_net(name)
    vis, aud = nhwc_inputs(name)
    taps = {}
    v, a, s = net.embed(vis, aud, taps=taps)
    for b in range(vis.shape[0]):
        tb = {}
        vb, ab, sb = net.embed(vis[b:b + 1].contiguous(), aud[b:b + 1].contiguous(), taps=tb)
        torch.cuda.synchronize()
        for enc in ("visual", "audio"):
            for i, (t1, tall) in enumerate(zip(tb[enc], taps[enc])):
                assert torch.equal(t1[0], tall[b]), (name, b, enc, i)
        assert torch.equal(vb[0], v[b]) and torch.equal(ab[0], a[b]) and torch.equal(sb[0], s[b]), (name, b)


def test_sync_score_matches_torch(gpu):
    B, D = 5, 200
    gen = torch.Generator().manual_seed(5)
    vin = P.bf16_round(torch.randn(B, D, generator=gen))
    ain = P.bf16_round(torch.randn(B, D, generator=gen))
    vin[1] = P.bf16_round(-vin[1].abs() - 0.5)  # an all-negative embedding: zero vector, score 0, no NaN
    ain[2] = vin[2]                             # identical embeddings: score 1
    gv = P.guarded((B, D), pitch=D + 8, dtype=torch.float32, device=DEV)
    ga = P.guarded((B, D), pitch=D + 8, dtype=torch.float32, device=DEV)
    gs = P.guarded((1, B), dtype=torch.float32, device=DEV)
    wide = lambda t: torch.cat([t, torch.full((B, 8), float("nan"))], 1).to(torch.bfloat16).to(DEV)[:, :D]
    ops.sync_score(wide(vin), wide(ain), v=gv.view, a=ga.view, score=gs.view[0])
    torch.cuda.synchronize()
    rv, ra = F.relu(P.f64(vin)), F.relu(P.f64(ain))
    nv, na = F.normalize(rv, dim=1), F.normalize(ra, dim=1)
    # x / |x|: the square sum (D terms), the root, the reciprocal and the product, each O(2^-24)
    # relative: elem_bound's 16 2^-24 on a magnitude of (D / 16 + 1) |ref| covers the sum
    P.assert_elementwise(gv.view, nv, P.elem_bound(nv, nv.abs() * (D / 16 + 1), torch.float32), name="v")
    P.assert_elementwise(ga.view, na, P.elem_bound(na, na.abs() * (D / 16 + 1), torch.float32), name="a")
    ref = F.cosine_similarity(nv, na, dim=1)
    # the dot's D accumulations plus both operands' errors above: (2 D + 48) 2^-24 sum |v a|
    mag = (nv.abs() * na.abs()).sum(1) * (D / 8 + 3)
    P.assert_elementwise(gs.view[0], ref, P.elem_bound(ref, mag, torch.float32), name="score")
    for g_, nm in ((gv, "v"), (ga, "a"), (gs, "score")):
        P.assert_guard_intact(g_, nm)
    got = gs.view[0].cpu()
    assert float(got[1]) == 0.0 and bool((gv.view[1] == 0).all()) and bool(torch.isfinite(gv.view).all())
    assert abs(float(got[2]) - 1.0) < 1e-6
