"""ls_syncnet_mel against the float64 oracle (tests/syncnet_ref.py), and the two packing
kernels bit for bit against torch doing the same fp32 arithmetic.  Outputs sit in guard bands.

Mel bound: 2^-10 on the [-4, 4] scale.  The only consumer stores the mel in bf16, whose
half-ulp in [2, 4) is 2^-7, so this is one eighth of what it can resolve.  Elements whose
float64 linear mel is below 1e-4 may be skipped (at most 1 %); on this signal there are none."""
import numpy as np
import pytest
import torch

import parity as P
import syncnet_ref as R
from latentsync_amd import ops, syncnet

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEL_BOUND = 2.0 ** -10


@pytest.mark.parametrize("n", (199, 200, 12345, 32000))
def test_mel_matches_float64_oracle(gpu, n):
    wav = R.chirp_signal(n)
    ref, lin = R.mel_oracle(wav, return_linear=True)
    T = 1 + n // 200
    assert ref.shape == (80, T)
    skip = lin < 1e-4
    assert skip.mean() <= 0.01
    assert not skip.any(), "the oracle skips no element on this signal"
    filters = torch.from_numpy(syncnet.mel_filters()).to(DEV)
    g = P.guarded((T, 80), dtype=torch.float32, device=DEV)
    ops.syncnet_mel(torch.from_numpy(wav).to(DEV), filters, out=g.view)
    torch.cuda.synchronize()
    got = g.view.cpu().double().numpy().T
    err = np.abs(got - ref)
    print(f"n = {n}: max |mel - oracle| = {err.max():.3g} (bound {MEL_BOUND:.3g})")
    assert np.isfinite(got).all()
    assert err[~skip].max() <= MEL_BOUND
    P.assert_guard_intact(g, "mel")
    got2 = syncnet.melspectrogram(wav)
    assert tuple(got2.shape) == (80, T) and torch.equal(got2.cpu(), g.view.cpu().t())


def test_pack_frames_bit_exact(gpu):
    R_, F_, n = 32, 16, 37
    starts = [0, 16, 21]
    faces = torch.randint(0, 256, (n, R_, R_, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    fd = faces.to(DEV)
    g = P.guarded((len(starts), R_ // 2, R_, 3 * F_), dtype=torch.bfloat16, device=DEV)
    ops.syncnet_pack_frames(fd, starts, F_, out=g.view)
    torch.cuda.synchronize()
    want = []
    for s in starts:
        w = faces[s:s + F_, R_ // 2:].float()                      # (F, R/2, R, 3)
        w = (w / 255.0 - 0.5) / 0.5
        want.append(w.permute(1, 2, 0, 3).reshape(R_ // 2, R_, 3 * F_))  # channel 3 f + c
    want = torch.stack(want).to(torch.bfloat16)
    assert torch.equal(g.view.cpu().view(torch.int16), want.view(torch.int16))
    P.assert_guard_intact(g, "pack_frames")
    for bad in ([22], [-1], [0, 37]):
        with pytest.raises(ValueError):
            ops.syncnet_pack_frames(fd, bad, F_)


def test_pack_mel_bit_exact(gpu):
    T, L = 161, 52
    mel = (torch.randn(T, 80, generator=torch.Generator().manual_seed(4)) * 1.5).clamp(-4, 4)
    cols = [0, 51, T - L]
    g = P.guarded((len(cols), 80, L, 8), dtype=torch.bfloat16, device=DEV)
    ops.syncnet_pack_mel(mel.to(DEV), cols, L, out=g.view)
    torch.cuda.synchronize()
    want = torch.zeros(len(cols), 80, L, 8)
    for b, c in enumerate(cols):
        want[b, :, :, 0] = mel[c:c + L].t()
    want = want.to(torch.bfloat16)
    assert torch.equal(g.view.cpu().view(torch.int16), want.view(torch.int16))
    P.assert_guard_intact(g, "pack_mel")
    for bad in ([T - L + 1], [-1]):
        with pytest.raises(ValueError):
            ops.syncnet_pack_mel(mel.to(DEV), bad, L)
