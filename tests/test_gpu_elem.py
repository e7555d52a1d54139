"""The elementwise entry points of ls_elem.hip, each on its own: per-element parity against
the fp64 formulas of include/ls_hip.h (tests/parity.py elem_bound), at sizes that are no
multiple of the 256-thread block, every pitch the kernels branch on, sentinel guard bands
around every output and inputs checked unchanged.  The whole-pipeline tests reach these
kernels at one pitch each and judge them by a Frobenius ratio.

Also the argument checks: non-positive sizes and a channel offset outside the destination
row return LS_ERR_INVALID with nothing launched.

The time embedding (ls_timestep_embed, ls_timestep_embed_f32, ls_small_linear -- temb of every
ResNet block) follows at the end, with the bounds parity.timestep_bound / dot_bound."""
import ctypes

import pytest
import torch

import parity as P
from latentsync_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
F_, R_, H_ = 3, 20, 10  # frames, pixel resolution, latent resolution: P = 300 latent pixels


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return t.to(DEV).contiguous()


def check(name, g, ref, bound, inputs):
    """Parity of the guarded output, the guard band, and every input bit for bit."""
    torch.cuda.synchronize()
    worst = P.assert_elementwise(g.view.reshape(ref.shape), ref, bound, name=name)
    P.assert_guard_intact(g, name)
    for i, (t, snap) in enumerate(inputs):
        P.assert_unchanged(t, snap, f"{name} input {i}")
    print(f"{name}: worst err/bound {worst:.3f}")
    return worst


def snaps(*ts):
    return [(t, P.snapshot(t)) for t in ts]


@pytest.mark.parametrize("ld", [8, 16, 4])
def test_prep_pixels(gpu, ld):
    """ld 8 = the 16-byte store path, 16 / 4 = the scalar path; channels 3.. exactly zero."""
    faces = torch.randint(0, 256, (F_, 3, R_, R_), generator=torch.Generator().manual_seed(1), dtype=U8)
    faces[0, :, 0, :3] = torch.tensor([[0, 255, 128]] * 3, dtype=U8)
    mask = (torch.rand(R_, R_, generator=torch.Generator().manual_seed(2)) > 0.4).float()
    mask[3, :5] = torch.tensor([0.25, 0.5, 0.75, 0.3, 0.9])  # a soft edge
    fd, md = dev(faces), dev(mask)
    gp = P.guarded((F_, R_, R_, ld), dtype=BF, device=DEV)
    gm = P.guarded((F_, R_, R_, ld), dtype=BF, device=DEV)
    inputs = snaps(fd, md)
    ops.prep_pixels(fd, md, ld=ld, pix=gp.view, masked=gm.view)
    u = P.f64(faces).permute(0, 2, 3, 1)  # (F, R, R, 3)
    p = (u / 255.0 - 0.5) / 0.5
    mag = 2 * (u / 255.0 + 0.5)
    pad = torch.zeros(F_, R_, R_, ld - 3, dtype=torch.float64)
    mk = P.f64(mask)[None, :, :, None]
    ref_p, ref_m = torch.cat([p, pad], -1), torch.cat([p * mk, pad], -1)
    check(f"prep_pixels ld {ld} pix", gp, ref_p, P.elem_bound(ref_p, torch.cat([mag, pad], -1), BF), inputs)
    check(f"prep_pixels ld {ld} masked", gm, ref_m, P.elem_bound(ref_m, torch.cat([mag * mk, pad], -1), BF), inputs)
    for g in (gp, gm):  # the padding channels are +0.0 bit for bit
        assert int(g.view[..., 3:].contiguous().view(torch.int16).abs().max()) == 0


@pytest.mark.parametrize("c_off", [5, 9])
def test_vae_sample(gpu, c_off):
    """Channels c_off..c_off+3 of a pitch-16 row; the logvar clamp; the other channels untouched."""
    Pn, ld_m, scaling, shift = F_ * H_ * H_, 8, 0.18215, 0.1
    mom = rnd(Pn, ld_m, seed=3)
    mom[:, 4:] *= 2.0
    mom[7, 4:] = torch.tensor([-40.0, 25.0, -30.0, 20.0])  # clamped to [-30, 20]
    mom[299, 4:] = torch.tensor([25.0, -40.0, 19.5, -29.5])
    eps = rnd(Pn, 4, seed=4)
    md, ed = dev(mom), dev(eps)
    g = P.guarded((Pn, 4), pitch=16, dtype=BF, device=DEV, offset=c_off)
    inputs = snaps(md, ed)
    ops.vae_sample(md, ed, scaling, shift, g.rows(Pn, 16, before=c_off), c_off)
    mean, lv = P.f64(mom[:, :4]), P.f64(mom[:, 4:]).clamp(-30.0, 20.0)
    noise = torch.exp(0.5 * lv) * P.f64(eps)
    s32, sh32 = float(torch.tensor(scaling, dtype=F32)), float(torch.tensor(shift, dtype=F32))
    ref = (mean + noise - sh32) * s32
    mag = (mean.abs() + 2 * noise.abs() + abs(sh32)) * abs(s32)  # (expf: 2 ulp, on the noise term)
    check(f"vae_sample c_off {c_off}", g, ref, P.elem_bound(ref, mag, BF), inputs)


@pytest.mark.parametrize("Bu,ld_in,R", [(1, 16, 20), (2, 24, 20), (2, 16, 80), (1, 24, 80)])
def test_pack_unet_input(gpu, Bu, ld_in, R):
    """R / h = 2 and 8 (the nearest mask), both batch counts and pitches: channels 0..3 the
    latents, 4 the mask, 5..12 cond, 13..15 zero, 16.. untouched."""
    h = H_
    Pn = F_ * h * h
    lat = rnd(Pn, 4, seed=5)
    cond = P.bf16_round(rnd(Pn, 16, seed=6))
    mask = torch.rand(R, R, generator=torch.Generator().manual_seed(7))
    ld_, cd, md = dev(lat), dev(cond.to(BF)), dev(mask)
    g = P.guarded((Bu * Pn, 16), pitch=ld_in, dtype=BF, device=DEV)
    inputs = snaps(ld_, cd, md)
    ops.pack_unet_input(ld_, cd, md, F_, R, h, Bu, g.rows(Bu * Pn, ld_in))
    idx = (torch.arange(h) * R) // h  # F.interpolate(mode="nearest"): floor(y R / h)
    m4 = P.f64(mask)[idx][:, idx].reshape(1, h * h).expand(F_, h * h).reshape(Pn, 1)
    ref = torch.cat([P.f64(lat), m4, P.f64(cond)[:, 5:13], torch.zeros(Pn, 3, dtype=torch.float64)], 1).repeat(Bu, 1)
    check(f"pack_unet_input Bu {Bu} ld {ld_in} R/h {R // h}", g, ref, P.elem_bound(ref, ref.abs(), BF), inputs)
    assert int(g.view[:, 13:].contiguous().view(torch.int16).abs().max()) == 0


@pytest.mark.parametrize("ld", [8, 16])
def test_scale_latents(gpu, ld):
    Pn, inv_s, shift = F_ * H_ * H_, 1 / 0.18215, 0.1
    lat = rnd(Pn, 4, seed=8)
    ld_ = dev(lat)
    g = P.guarded((Pn, ld), dtype=BF, device=DEV)
    inputs = snaps(ld_)
    ops.scale_latents(ld_, inv_s, shift, g.view)
    i32, s32 = float(torch.tensor(inv_s, dtype=F32)), float(torch.tensor(shift, dtype=F32))
    pad = torch.zeros(Pn, ld - 4, dtype=torch.float64)
    ref = torch.cat([P.f64(lat) * i32 + s32, pad], 1)
    mag = torch.cat([P.f64(lat).abs() * i32 + abs(s32), pad], 1)
    check(f"scale_latents ld {ld}", g, ref, P.elem_bound(ref, mag, BF), inputs)
    assert int(g.view[:, 4:].contiguous().view(torch.int16).abs().max()) == 0


@pytest.mark.parametrize("outs", ["f32", "u8", "both"])
def test_paste_back(gpu, outs):
    """fp32 only, uint8 only, both; values beyond +-1 (the clamp); uint8 = truncation of the
    formula, one count of freedom only where the fp64 value is within 2^-16 of an integer."""
    ld_dec, ld_pix = 8, 16
    dec = P.bf16_round(rnd(F_, R_, R_, ld_dec, seed=9, scale=0.8))  # |x| > 1 for about a fifth
    pix = P.bf16_round(rnd(F_, R_, R_, ld_pix, seed=10, scale=0.8))
    dec[0, 0, :4, :3] = torch.tensor([[-1.0, 1.0, 0.0], [-3.0, 2.5, 1.0 - 2 ** -8], [0.5, -0.5, 0.25], [1.5, -1.5, 0]])
    keep = torch.tensor([0.0, 1.0, 0.5, 0.25])[torch.randint(0, 4, (R_, R_), generator=torch.Generator().manual_seed(11))]
    dd, pd, kd = dev(dec.to(BF)), dev(pix.to(BF)), dev(keep)
    gf = P.guarded((F_, 3, R_, R_), dtype=F32, device=DEV) if outs != "u8" else None
    gu = P.guarded((F_, R_, R_, 3), dtype=U8, device=DEV) if outs != "f32" else None
    inputs = snaps(dd, pd, kd)
    ops.paste_back(dd, pd, kd, out_nchw=None if gf is None else gf.view, out_u8=None if gu is None else gu.view)
    k = P.f64(keep)[None, :, :, None]
    d3, p3 = P.f64(dec)[..., :3], P.f64(pix)[..., :3]
    v = d3 * (1 - k) + p3 * k  # (F, R, R, 3)
    if gf is not None:
        mag = d3.abs() * (1 + k) + (p3 * k).abs()
        check(f"paste_back {outs} fp32", gf, v.permute(0, 3, 1, 2), P.elem_bound(v, mag, F32).permute(0, 3, 1, 2), inputs)
    if gu is not None:
        torch.cuda.synchronize()
        t = (v / 2 + 0.5).clamp(0, 1) * 255
        got = gu.view.cpu().to(torch.int64)
        lo = torch.floor(t).to(torch.int64)
        near = (t - torch.round(t)).abs() < 2.0 ** -16
        ok = (got == lo) | (near & ((got == torch.round(t).to(torch.int64)) | (got == torch.round(t).to(torch.int64) - 1)))
        assert bool(ok.all()), (int((~ok).sum()), got[~ok][:8], t[~ok][:8])
        assert int(got.min()) == 0 and int(got.max()) == 255  # both clamps were reached
        P.assert_guard_intact(gu, "paste_back u8")
        for i, (x, s) in enumerate(inputs):
            P.assert_unchanged(x, s, f"paste_back input {i}")
        print(f"paste_back {outs} u8: {int(near.sum())} value(s) within 2^-16 of an integer, all others exact")


def test_add_rows(gpu):
    """ldx != ldy != C, rows % table_rows != 0."""
    rows, C, ldx, ldy, trows = 301, 20, 24, 36, 7
    x = P.bf16_round(rnd(rows, ldx, seed=12))
    table = rnd(trows, C, seed=13)
    xd, td = dev(x.to(BF)), dev(table)
    g = P.guarded((rows, C), pitch=ldy, dtype=BF, device=DEV)
    inputs = snaps(xd, td)
    ops.add_rows(xd[:, :C], td, out=g.view)
    t = P.f64(table)[torch.arange(rows) % trows]
    ref = P.f64(x)[:, :C] + t
    check("add_rows", g, ref, P.elem_bound(ref, P.f64(x)[:, :C].abs() + t.abs(), BF), inputs)


@pytest.mark.parametrize("Bu", [1, 2])
def test_ddim_cfg_step(gpu, Bu):
    """Bu = 1 (no guidance) and 2, ld_in = 8 with channels 4..7 of unet_in untouched; the
    latents in place (fp32), the step counter advanced by one."""
    Pn, ld_eps, ld_in, guidance, n_steps, step0 = F_ * H_ * H_, 8, 8, 1.5, 5, 2
    eps = P.bf16_round(rnd(Bu * Pn, ld_eps, seed=14))
    lat = rnd(Pn, 4, seed=15)
    a_t = torch.linspace(0.2, 0.9, n_steps)
    a_prev = torch.cat([a_t[1:], torch.ones(1)])
    coef = torch.stack([a_t.sqrt(), (1 - a_t).sqrt(), a_prev.sqrt(), (1 - a_prev).sqrt()], 1).float()
    ed, cd = dev(eps.to(BF)), dev(coef)
    step = torch.tensor([step0], dtype=torch.int32, device=DEV)
    gl = P.guarded((Pn, 4), dtype=F32, device=DEV)
    gl.view.copy_(lat)
    gu = P.guarded((Bu * Pn, 4), pitch=ld_in, dtype=BF, device=DEV)
    inputs = snaps(ed, cd)
    ops.ddim_cfg_step(ed, Bu, guidance, gl.view, cd, step, gu.rows(Bu * Pn, ld_in))
    c = P.f64(coef)[step0]
    e = P.f64(eps)[:Pn, :4]
    emag = e.abs()
    if Bu == 2:
        a = P.f64(eps)[Pn:, :4]
        emag = e.abs() + guidance * (a.abs() + e.abs())
        e = e + guidance * (a - e)
    x = P.f64(lat)
    ref = c[2] * (x - c[1] * e) / c[0] + c[3] * e
    mag = c[2] * (x.abs() + c[1] * emag) / c[0] + c[3] * emag
    check(f"ddim_cfg_step Bu {Bu} latents", gl, ref, P.elem_bound(ref, mag, F32), inputs)
    check(f"ddim_cfg_step Bu {Bu} unet_in", gu, ref.repeat(Bu, 1), P.elem_bound(ref, mag, BF).repeat(Bu, 1), inputs)
    assert int(step.item()) == step0 + 1


def test_elem_argument_checks(gpu):
    """Non-positive sizes, a negative c_off and c_off + 4 > ld_dst: LS_ERR_INVALID, nothing
    launched (every output keeps its sentinel)."""
    from latentsync_amd import _lib
    lib = _lib.load()
    INVALID = 1
    g = P.guarded((64, 16), dtype=BF, device=DEV)
    gf = P.guarded((64, 16), dtype=F32, device=DEV)
    gb = P.guarded((64, 16), dtype=U8, device=DEV)
    src = torch.zeros(4096, dtype=F32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    o, of, ob, s, st = (t.data_ptr() for t in (g.view, gf.view, gb.view, src, step))
    calls = []
    for F, R in ((0, 4), (-1, 4), (2, 0), (2, -3)):
        calls.append(("ls_prep_pixels", lib.ls_prep_pixels(s, F, R, s, o, o, 8, None)))
        calls.append(("ls_paste_back", lib.ls_paste_back(s, 8, s, 8, s, F, R, of, ob, None)))
    for Pn, c_off, ld_dst in ((0, 0, 16), (-5, 0, 16), (8, -1, 16), (8, 13, 16), (8, 4, 4), (8, 16, 16)):
        calls.append(("ls_vae_sample", lib.ls_vae_sample(s, 8, s, Pn, 1.0, 0.0, o, ld_dst, c_off, None)))
    for F, R, h, Bu in ((0, 4, 2, 1), (1, 0, 2, 1), (1, 4, 0, 1), (1, 4, 2, 0), (1, 4, -2, 1), (1, 4, 2, -1)):
        calls.append(("ls_pack_unet_input", lib.ls_pack_unet_input(s, s, s, F, R, h, Bu, o, 16, None)))
    for Pn in (0, -1):
        calls.append(("ls_scale_latents", lib.ls_scale_latents(s, Pn, 1.0, 0.0, o, 8, None)))
        calls.append(("ls_ddim_cfg_step", lib.ls_ddim_cfg_step(s, 8, 1, Pn, 1.0, of, s, st, o, 8, None)))
    for Bu in (0, 3, -1):
        calls.append(("ls_ddim_cfg_step", lib.ls_ddim_cfg_step(s, 8, Bu, 8, 1.0, of, s, st, o, 8, None)))
    for rows, C in ((0, 8), (-2, 8), (8, 0), (8, -8)):
        calls.append(("ls_add_rows", lib.ls_add_rows(s, rows, C, 16, s, 4, o, 16, None)))
    calls.append(("ls_add_rows", lib.ls_add_rows(s, 8, 8, 16, s, 0, o, 16, None)))
    calls.append(("ls_add_rows", lib.ls_add_rows(s, 8, 8, 4, s, 4, o, 16, None)))  # ldx < C
    bad = [(n, rc) for n, rc in calls if rc != INVALID]
    assert not bad, bad
    assert lib.ls_last_error()  # a message was left
    torch.cuda.synchronize()
    for gg in (g, gf, gb):
        P.assert_guard_intact(gg)
        assert bool((gg.view.contiguous().view(gg.bits_dtype) == (gg.sentinel if gg.bits_dtype != U8 else 0xA5)).all())
    assert int(step.item()) == 0


# ---------------------------------------------------------------- the time embedding
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("dim", P.TS_DIMS)
def test_timestep_embed(gpu, dim, flip, shift):
    """t = ts[*step] with step in 1 .. 4 (never the first entry), B = 1 and 2 identical rows,
    dim 320 (the model's) and 6 (half = 3: most threads idle), both orders, shift 0 and 1."""
    table = torch.tensor([7, *P.TS_T, 3], dtype=torch.int32)
    td = dev(table)
    worst = 0.0
    for k, t in enumerate(P.TS_T, start=1):
        assert int(table[k]) == t
        for B in (1, 2):
            step = torch.tensor([k], dtype=torch.int32, device=DEV)
            g = P.guarded((B, dim), dtype=F32, device=DEV)
            inputs = snaps(td, step)
            ops.timestep_embed(td, step, B, dim, flip, float(shift), out=g.view)
            ref, bound = P.timestep_bound(torch.full((B,), float(t)), dim, shift, flip)
            worst = max(worst, check(f"timestep_embed t {t} B {B} dim {dim} flip {flip} shift {shift}", g, ref, bound, inputs))
    print(f"timestep_embed dim {dim} flip {flip} shift {shift}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("dim", P.TS_DIMS)
def test_timestep_embed_f32(gpu, dim, flip, shift):
    """One block per sample: three distinct fractional timesteps, each row its own."""
    t = torch.tensor([0.25, 500.5, 998.75], dtype=F32)
    td = dev(t)
    g = P.guarded((3, dim), dtype=F32, device=DEV)
    inputs = snaps(td)
    ops.timestep_embed_f32(td, dim, flip, float(shift), out=g.view)
    ref, bound = P.timestep_bound(t, dim, shift, flip)
    check(f"timestep_embed_f32 dim {dim} flip {flip} shift {shift}", g, ref, bound, inputs)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("silu_in", [False, True])
@pytest.mark.parametrize("M,K,N", P.SMALL_LINEAR_CASES)
def test_small_linear(gpu, M, K, N, silu_in, with_bias):
    """fp32 x of deviation 2, bf16 W, fp32 out: the model's shapes (K 320 and 1280), N % 4 != 0
    (the waves past N leave after the barrier), a last row chunk of 1 and 3 rows, K = 8 (one
    working lane), and the limits K = 2048, M = 1024."""
    x = 2.0 * rnd(M, K, seed=M + K)
    w = P.bf16_round(rnd(N, K, seed=N + K + 1, scale=K ** -0.5))
    b = rnd(N, seed=N + 2, scale=0.1) if with_bias else None
    xd, wd, bd = dev(x), dev(w.to(BF)), None if b is None else dev(b)
    g = P.guarded((M, N), dtype=F32, device=DEV)
    inputs = snaps(xd, wd) + ([] if bd is None else snaps(bd))
    ops.small_linear(xd, wd, bd, silu_in=silu_in, out=g.view)
    ref, bound = P.dot_bound(x, w, b, silu_in)
    check(f"small_linear {M}x{K}x{N} silu {silu_in} bias {with_bias}", g, ref, bound, inputs)


def test_time_embedding_argument_checks(gpu):
    """K % 8 != 0, K > 2048, M > 1024, an odd dim and B = 0: LS_ERR_INVALID, nothing launched
    (the output keeps its sentinel)."""
    from latentsync_amd import _lib
    lib = _lib.load()
    INVALID = 1
    gf = P.guarded((64, 16), dtype=F32, device=DEV)
    src = torch.zeros(4096, dtype=F32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    of, s, st = gf.view.data_ptr(), src.data_ptr(), step.data_ptr()
    calls = []
    for M, K in ((1, 12), (1, 4), (1, 2056), (1025, 8), (0, 8)):
        calls.append((f"ls_small_linear M {M} K {K}", lib.ls_small_linear(s, M, K, s, s, 4, 0, of, None)))
    for B, dim in ((1, 7), (2, 321), (0, 8), (-1, 8)):
        calls.append((f"ls_timestep_embed B {B} dim {dim}", lib.ls_timestep_embed(s, st, B, dim, 1, 0.0, of, None)))
        calls.append((f"ls_timestep_embed_f32 B {B} dim {dim}", lib.ls_timestep_embed_f32(s, B, dim, 1, 0.0, of, None)))
    bad = [(n, rc) for n, rc in calls if rc != INVALID]
    assert not bad, bad
    assert lib.ls_last_error()
    torch.cuda.synchronize()
    P.assert_guard_intact(gf)
    assert bool((gf.view.contiguous().view(gf.bits_dtype) == gf.sentinel).all())
