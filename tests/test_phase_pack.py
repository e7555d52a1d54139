"""Phase packing of a nearest-x2 upsample conv (packing.pack_phase_weight) and its dispatch
(ls_conv_desc.upsample == 2), without a GPU: the four 2x2 phase convs over the input image
equal conv3x3(nearest_x2(x), w, padding=1) to fp64 roundoff at every border; the K order
and the sizes are the ones conv3x3_halo_kernel indexes; ls_conv_path takes the phase form on
the halo-tile kernel (4) for the shapes it patches, on the tiled kernels (5) for the others
with a plain bf16 epilogue, and the callers keep the 9-tap form elsewhere."""
import pytest
import torch
import torch.nn.functional as F

from latentsync_amd import ops
from latentsync_amd.packing import pack_phase_weight, pack_weight, phase_tap_sums


def unpack(wp, cin):
    """(4, O, 4 cin) in the packed K order k = (ci / 64) * 256 + t * 64 + ci % 64, t = 2 dy + dx
    -> (4, O, cin, 2, 2)."""
    O = wp.shape[1]
    return wp.reshape(4, O, cin // 64, 2, 2, 64).permute(0, 1, 2, 5, 3, 4).reshape(4, O, cin, 2, 2)


def phase_conv(x, w4):
    """x (n, C, H, W), w4 (4, O, C, 2, 2) -> (n, O, 2H, 2W): every phase as a 2x2 conv over
    the zero-padded input, interleaved by output parity."""
    n, _, H, W = x.shape
    O = w4.shape[1]
    out = torch.zeros(n, O, 2 * H, 2 * W, dtype=x.dtype)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            w = w4[2 * py + px].to(x.dtype)
            # tap (dy, dx) reads input (y - 1 + py + dy, x - 1 + px + dx) = padded (y + py + dy, x + px + dx)
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], w)
    return out


@pytest.mark.parametrize("cin", [8, 64, 128])
@pytest.mark.parametrize("hw", [(4, 4), (5, 7), (16, 16)])
def test_phase_pack_equals_upsample_conv_fp64(hw, cin):
    """n_img 3; the difference to fp64 roundoff (the sums of up to 4 taps reorder the additions);
    checked whole and on each of the four border rows / columns.  Cin 64 / 128 through the
    packed K order, Cin 8 (no whole chunk, never packed) through the tap sums alone."""
    g = torch.Generator().manual_seed(cin + hw[0])
    x = torch.randn(3, cin, *hw, generator=g, dtype=torch.float64)
    w = torch.randn(24, cin, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, padding=1)
    got = phase_conv(x, unpack(pack_phase_weight(w), cin) if cin % 64 == 0 else phase_tap_sums(w))
    tol = 64 * 9 * cin * 2.0 ** -53 * float(ref.abs().max() + 1)
    for name, sl in (("all", (slice(None), slice(None))), ("top", (0, slice(None))), ("bottom", (-1, slice(None))),
                     ("left", (slice(None), 0)), ("right", (slice(None), -1))):
        d = float((got[(..., *sl)] - ref[(..., *sl)]).abs().max())
        assert d <= tol, (name, d, tol)


@pytest.mark.parametrize("cin", [64, 128])
def test_pack_phase_weight_layout_and_fp32_sums(cin):
    """The fp32 packing against the fp64 one: fp32 sums of <= 4 taps (3 roundings);
    shape (4, O, 4 cin) with no row or K padding (4 cin is whole 64-wide K-tiles; the kernel's
    weight descriptor covers min(BN, N - n0) rows of phase ph at (ph N + n0) K); element
    (ph, o, (ci / 64) 256 + t 64 + ci % 64) is the sum of the taps of PHASE_TAPS."""
    g = torch.Generator().manual_seed(cin)
    w = torch.randn(40, cin, 3, 3, generator=g)
    wp = pack_phase_weight(w)
    assert wp.shape == (4, 40, 4 * cin) and wp.dtype == torch.float32 and (4 * cin) % 64 == 0
    ref = pack_phase_weight(w.double())
    assert float((wp.double() - ref).abs().max()) <= 3 * 2.0 ** -24 * float(w.abs().max()) * 4
    # spot checks of the K order, written out
    ci, o = cin - 3, 7
    k = lambda t: (ci // 64) * 256 + t * 64 + ci % 64
    assert wp[0, o, k(0)] == w[o, ci, 0, 0]                                   # (py, px) = (0, 0), tap (0, 0)
    assert torch.isclose(wp[0, o, k(3)], w[o, ci, 1:, 1:].sum())              # tap (1, 1): 4 taps
    assert torch.isclose(wp[3, o, k(0)], w[o, ci, :2, :2].sum())              # (1, 1), tap (0, 0): 4 taps
    assert wp[3, o, k(3)] == w[o, ci, 2, 2]
    assert torch.isclose(wp[1, o, k(1)], w[o, ci, 0, 2])                      # (0, 1), tap (0, 1): w[0][2]
    assert wp[2, o, k(2)] == w[o, ci, 2, 0]                                   # (1, 0), tap (1, 0): w[2][0]
    assert torch.isclose(wp[2, o, k(0)], w[o, ci, :2, 0].sum())               # (1, 0), tap (0, 0): w[0][0] + w[1][0]


def test_pack_phase_weight_rejects_partial_chunks():
    with pytest.raises(AssertionError):
        pack_phase_weight(torch.zeros(8, 72, 3, 3))
    with pytest.raises(AssertionError):
        pack_phase_weight(torch.zeros(8, 8, 3, 3))


def _pw(n, cin, phase=True):
    w = torch.zeros(n, cin, 3, 3)
    pw = ops.Packed(pack_weight(w).to(torch.bfloat16), torch.zeros(n), (cin + 7) // 8 * 8, 3, n)
    if phase and cin % 64 == 0:
        pw.phase = pack_phase_weight(w).to(torch.bfloat16)
    return pw


def _x(n, H, W, C):
    return torch.zeros(n, H, W, C, dtype=torch.bfloat16)


@pytest.mark.parametrize("hw,c", [((16, 16), 640), ((32, 32), 512), ((64, 64), 512), ((128, 128), 256)])
def test_halo_upsamplers_take_the_phase_form(hw, c):
    """UNet 640 ch 16^2 -> 32^2 and the three VAE decoder upsamplers: path 4 with phase-packed
    weights, and the same call with an ordinary Packed stays on today's halo form (3)."""
    x = _x(2, *hw, c)
    assert ops.conv_path(x, _pw(c, c), upsample=True) == 4
    assert ops.conv_path(x, _pw(c, c, phase=False), upsample=True) == 3
    # (the fields the bench's FLOP probe reads keep describing the 9-tap layer)
    pw = _pw(c, c)
    assert (pw.N, pw.ksize, pw.cin, pw.K) == (c, 3, c, 9 * c) and pw.w.shape == (c, 9 * c)


@pytest.mark.parametrize("hw", [(4, 4), (8, 8)])
def test_wide_unet_upsamplers_take_the_tiled_phase_form(hw):
    """1280 channels at 4^2 / 8^2 (N > 640, images below a halo patch): the phase form on the
    tiled kernels (5); without phase weights the tiled 9-tap gather (0) as before."""
    x = _x(16, *hw, 1280)
    assert ops.conv_path(x, _pw(1280, 1280), upsample=True) == 5
    assert ops.conv_path(x, _pw(1280, 1280, phase=False), upsample=True) == 0


def test_shapes_the_phase_form_cannot_take_keep_the_present_path():
    # Cin = 72: no phase weights can be packed, the tap-major 9-tap gather
    assert _pw(40, 72).phase is None
    assert ops.conv_path(_x(3, 16, 16, 72), _pw(40, 72), upsample=True) == 0
    # a 5 x 7 image (the halo patches do not divide it), N = 40 (neither halo tile width divides
    # it), 8 x 8 (below a halo patch of the input image): the tiled phase form
    assert ops.conv_path(_x(3, 5, 7, 64), _pw(128, 64), upsample=True) == 5
    assert ops.conv_path(_x(3, 16, 16, 64), _pw(40, 64), upsample=True) == 5
    assert ops.conv_path(_x(2, 8, 8, 64), _pw(128, 64), upsample=True) == 5
    # N = 36 (not whole 16-B output rows), an fp32 output, an input affine:
    # no phase form, the 9-tap path as without phase weights
    assert ops.conv_path(_x(3, 8, 8, 64), _pw(36, 64), upsample=True) == 0
    y32 = torch.zeros(2, 16, 16, 128)
    assert ops.conv_path(_x(2, 8, 8, 64), _pw(128, 64), upsample=True, out=y32, out_f32=True) == \
        ops.conv_path(_x(2, 8, 8, 64), _pw(128, 64, phase=False), upsample=True, out=y32, out_f32=True)
    aff = (torch.ones(2, 64), torch.zeros(2, 64), 1, True)
    assert ops.conv_path(_x(2, 16, 16, 64), _pw(128, 64), upsample=True, aff=aff) == \
        ops.conv_path(_x(2, 16, 16, 64), _pw(128, 64, phase=False), upsample=True, aff=aff)
    # not an upsample call: phase weights are ignored
    assert ops.conv_path(_x(2, 16, 16, 64), _pw(128, 64)) == 3
