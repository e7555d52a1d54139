"""Host half of the sync-confidence score (latentsync_amd/syncnet.py): the window plan, the
mel filterbank, the state-dict layout and the float64 mel oracle's frame count.  No GPU."""
import numpy as np
import pytest
import torch

import syncnet_ref as R
from conftest import golden
from latentsync_amd import syncnet


def test_window_plan_known_answers():
    # 48 frames at 25 frames/s, 1.92 s of audio -> 154 mel frames: columns int(80 * s / 25)
    assert syncnet.window_plan(48, 154) == ([0, 16, 32], [0, 51, 102])
    # 102 + 52 = 154 just fits; one mel frame fewer drops the last window, as the dataset does
    assert syncnet.window_plan(48, 153) == ([0, 16], [0, 51])
    assert syncnet.window_plan(47, 1000) == ([0, 16], [0, 51])        # 32 + 16 > 47
    assert syncnet.window_plan(15, 1000) == ([], [])
    # stride != num_frames: overlapping windows
    assert syncnet.window_plan(40, 1000, stride=8) == ([0, 8, 16, 24], [0, 25, 51, 76])
    # another rate and window length: mel_len = ceil(5 / 5 * 16) = 16, columns int(80 * s / 30)
    assert syncnet.window_plan(12, 40, fps=30, num_frames=5, stride=5) == ([0, 5], [0, 13])
    assert syncnet.window_plan(48, 154, mel_len=60) == ([0, 16], [0, 51])


def test_mel_filters():
    f = syncnet.mel_filters()
    assert f.shape == (80, 401) and f.dtype == np.float32
    assert (f >= 0).all() and (f.max(axis=1) > 0).all()
    edges = syncnet.mel_band_edges()
    assert edges.shape == (82,) and abs(edges[0] - 55.0) < 1e-9 and abs(edges[-1] - 7600.0) < 1e-6
    assert (np.diff(edges) > 0).all()
    # a row is non-zero only between its outer band edges
    freqs = np.arange(401) * 20.0
    for i in range(80):
        outside = (freqs <= edges[i]) | (freqs >= edges[i + 2])
        assert not f[i, outside].any(), i
    # Slaney norm: each triangle has unit area.  The bins sample it every D = 20 Hz; the
    # Riemann sum of a piecewise-linear function misses its integral by at most D^2 / 8 per
    # kink times the slope change there: h/b1 at the first edge, h/b1 + h/b2 at the peak, h/b2
    # at the last (h = 2 / (b1 + b2) the peak, b1, b2 the two half-widths).
    b1, b2 = edges[1:81] - edges[:80], edges[2:82] - edges[1:81]
    h = 2.0 / (b1 + b2)
    bound = 20.0 ** 2 / 8 * 2 * (h / b1 + h / b2) + 1e-6
    integral = f.astype(np.float64).sum(axis=1) * 20.0
    assert (np.abs(integral - 1.0) <= bound).all(), np.abs(integral - 1.0).max()
    assert np.abs(integral[40:] - 1.0).max() < 0.02  # wide bands: many bins per triangle


@pytest.mark.parametrize("name", ("A", "B", "C"))
def test_state_dict_keys_match_the_reference(name):
    cfg = R.CASES[name][0]
    keys = [str(k) for k in golden(f"syncnet_{name}.npz")["keys"]]
    assert list(syncnet.param_shapes(cfg)) == keys
    net = syncnet.StableSyncNet(cfg)
    sd = R.case_weights(name)
    assert list(sd) == keys
    net.load_state_dict(sd)
    assert list(net.state_dict()) == keys
    assert all(torch.equal(net.state_dict()[k], sd[k]) for k in keys)
    missing = dict(sd)
    del missing["visual_encoder.norm_out.bias"]
    with pytest.raises(RuntimeError, match="missing"):
        syncnet.StableSyncNet(cfg).load_state_dict(missing)
    bad = dict(sd)
    bad["audio_encoder.conv_in.weight"] = torch.zeros(32, 2, 3, 3)
    with pytest.raises(RuntimeError, match="shape"):
        syncnet.StableSyncNet(cfg).load_state_dict(bad)
    extra = dict(sd, bogus=torch.zeros(1))
    with pytest.raises(RuntimeError, match="unexpected"):
        syncnet.StableSyncNet(cfg).load_state_dict(extra)


def test_from_pretrained_reads_the_reference_checkpoint_layout(tmp_path):
    cfg = R.CASES["A"][0]
    sd = R.case_weights("A")
    torch.save({"state_dict": sd, "global_step": 7}, tmp_path / "syncnet.pt")
    net = syncnet.StableSyncNet.from_pretrained(cfg, str(tmp_path / "syncnet.pt"))
    assert all(torch.equal(net.state_dict()[k], v) for k, v in sd.items())
    with pytest.raises(RuntimeError, match="HIP device"):
        net(torch.zeros(1, 48, 16, 32), torch.zeros(1, 1, 20, 13))  # no CPU path, and it says so


def test_forward_refuses_a_wrong_channel_count():
    net = syncnet.StableSyncNet(R.CASES["A"][0])
    net.load_state_dict(R.case_weights("A"))
    net._dev = (syncnet._Encoder.__new__(syncnet._Encoder), syncnet._Encoder.__new__(syncnet._Encoder))
    net._dev[0].in_channels, net._dev[0].cin_pad, net._dev[1].in_channels, net._dev[1].cin_pad = 48, 48, 1, 8
    with pytest.raises(ValueError, match="48"):
        net(torch.zeros(1, 45, 16, 32), torch.zeros(1, 1, 20, 13))


def test_dropout_is_accepted_and_ignored():
    cfg = {k: dict(v, dropout=0.3) for k, v in R.CASES["A"][0].items()}
    assert list(syncnet.param_shapes(cfg)) == list(syncnet.param_shapes(R.CASES["A"][0]))
    syncnet.StableSyncNet(cfg, gradient_checkpointing=True).load_state_dict(R.case_weights("A"))


@pytest.mark.parametrize("n", (199, 200, 12345, 32000))
def test_mel_oracle_frame_count(n):
    out, lin = R.mel_oracle(R.chirp_signal(n), return_linear=True)
    assert out.shape == lin.shape == (80, 1 + n // 200)
    assert np.isfinite(out).all() and (np.abs(out) <= 4).all()
