"""The plan of ls_conv2d (ls_conv_plan / ops.conv_plan: host only, no launch, no GPU): which
kernel instance, launch geometry and trailing passes every descriptor of a named corpus gets.

CORPUS rows are (name, kind, call, tuning): kind "model" = a call unet.py / vae.py issue at the
bench configuration (256^2, 48 windows of 16 frames = 768 images, one timestep row), "edge" =
a shape chosen to reach one branch of the dispatch.  PINS holds each row's plan in the short
form of _fmt().  tests/golden/conv_path_parent.json holds what ops.conv_path answered for the
same corpus at commit 41d7641, whose ls_conv_path was a walk of its own: every row must still
get that answer except the rows of PATH_DIFFERS, where 41d7641's ls_conv_path named another
family than its ls_conv2d launched."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import REPO
from latentsync_amd import _lib, ops

BF = torch.bfloat16
NB = 768  # images per UNet call at the bench configuration
ROWS32, ROWS16, ROWS8, ROWS4 = NB * 1024, NB * 256, NB * 64, NB * 16
# tuning keys the corpus touches, with their defaults (restored after every row)
WS = 256 << 20  # the split-K workspace ops.conv hands ls_conv2d
DEFAULTS = {1: 0, 2: 0, 3: 0, 6: 1, 7: 1, 8: 1, 13: 0, 15: 1, 16: 1, 18: 1, 19: 1, 20: 0}


def _row(name, kind, x, w, tune=None, **call):
    return (name, kind, dict(x=x, w=w, **call), tune or {})


def _lin(name, kind, rows, k, n, tune=None, **call):
    return _row(name, kind, (1, 1, rows, k), (n, 1), tune, **call)


# call: x = (n, H, W, C1), w = (N, ksize), c2 = channels of the concat source, n_out = real output
# channels, aff = (imgs_per_sample, silu), rowvec = rows_per_vec, res / ln / stats / phase = True,
# everything else goes to ops.conv as it is
CORPUS = [
    # ---- UNet, 32x32 level (C = 320)
    _row("unet_conv_in", "model", (NB, 32, 32, 16), (320, 3), gn_out=True),
    _row("res32_conv1", "model", (NB, 32, 32, 320), (320, 3), aff=(16, True), rowvec=ROWS32, gn_out=True),
    _row("res32_conv2", "model", (NB, 32, 32, 320), (320, 3), aff=(16, True), res=True, gn_out=True),
    _row("down32", "model", (NB, 32, 32, 320), (320, 3), stride=2, pad=1, gn_out=True),
    _row("proj_in32", "model", (NB, 32, 32, 320), (320, 1), aff=(1, False), stats=True),
    _lin("qkv32", "model", ROWS32, 320, 960, ln=True),
    _lin("motion_qkv32", "model", ROWS32, 320, 960, ln=True, rowvec=(1024, 16)),
    _lin("attn_out32", "model", ROWS32, 320, 320, res=True, stats=True),
    _lin("q2_32", "model", ROWS32, 320, 320, ln=True),
    _lin("audio_kv", "model", NB * 50, 384, 640),
    _lin("ff1_32", "model", ROWS32, 320, 2560, ln=True, act=ops.ACT_GEGLU),
    _lin("ff2_32", "model", ROWS32, 1280, 320, res=True),
    _row("proj_out32", "model", (NB, 32, 32, 320), (320, 1), res=True, gn_out=True),
    _row("up32_conv1_cat", "model", (NB, 32, 32, 640), (320, 3), c2=320, aff=(16, True), rowvec=ROWS32, gn_out=True),
    _row("up32_shortcut_cat", "model", (NB, 32, 32, 640), (320, 1), c2=320),
    _row("unet_conv_out", "model", (NB, 32, 32, 320), (8, 3), n_out=8, aff=(16, True)),
    # ---- 16x16 level (C = 640)
    _row("res16_conv1_in320", "model", (NB, 16, 16, 320), (640, 3), aff=(16, True), rowvec=ROWS16, gn_out=True),
    _row("res16_shortcut", "model", (NB, 16, 16, 320), (640, 1)),
    _row("res16_conv2", "model", (NB, 16, 16, 640), (640, 3), aff=(16, True), res=True, gn_out=True),
    _row("down16", "model", (NB, 16, 16, 640), (640, 3), stride=2, pad=1, gn_out=True),
    _row("proj_in16", "model", (NB, 16, 16, 640), (640, 1), aff=(1, False), stats=True),
    _lin("qkv16", "model", ROWS16, 640, 1920, ln=True),
    _lin("attn_out16", "model", ROWS16, 640, 640, res=True, stats=True),
    _lin("ff1_16", "model", ROWS16, 640, 5120, ln=True, act=ops.ACT_GEGLU),
    _lin("ff2_16", "model", ROWS16, 2560, 640, res=True),
    _row("proj_out16", "model", (NB, 16, 16, 640), (640, 1), res=True, gn_out=True),
    _row("up16_conv1_cat", "model", (NB, 16, 16, 1280), (640, 3), c2=640, aff=(16, True), rowvec=ROWS16, gn_out=True),
    _row("upsample16_phase", "model", (NB, 16, 16, 640), (640, 3), upsample=True, phase=True, gn_out=True),
    # ---- 8x8 and 4x4 levels (C = 1280): the affine is materialised first (family 2 asks for it)
    _row("res8_conv1_in640_affine", "model", (NB, 8, 8, 640), (1280, 3), aff=(16, True), rowvec=ROWS8, gn_out=True),
    _row("res8_conv1_in640", "model", (NB, 8, 8, 640), (1280, 3), rowvec=ROWS8, gn_out=True),
    _row("res8_conv2", "model", (NB, 8, 8, 1280), (1280, 3), res=True, gn_out=True),
    _row("res8_shortcut", "model", (NB, 8, 8, 640), (1280, 1)),
    _row("down8", "model", (NB, 8, 8, 1280), (1280, 3), stride=2, pad=1, gn_out=True),
    _row("proj_in8_affine", "model", (NB, 8, 8, 1280), (1280, 1), aff=(1, False), stats=True),
    _row("proj_in8", "model", (NB, 8, 8, 1280), (1280, 1), stats=True),
    _lin("qkv8", "model", ROWS8, 1280, 3840, ln=True),
    _lin("attn_out8", "model", ROWS8, 1280, 1280, res=True, stats=True),
    _lin("ff1_8", "model", ROWS8, 1280, 10240, ln=True, act=ops.ACT_GEGLU),
    _lin("ff2_8", "model", ROWS8, 5120, 1280, res=True),
    _row("proj_out8", "model", (NB, 8, 8, 1280), (1280, 1), res=True, gn_out=True),
    _row("up8_conv1_cat", "model", (NB, 8, 8, 2560), (1280, 3), rowvec=ROWS8, gn_out=True),
    _row("up8_shortcut_cat", "model", (NB, 8, 8, 2560), (1280, 1), c2=1280),
    _row("upsample8_phase", "model", (NB, 8, 8, 1280), (1280, 3), upsample=True, phase=True, gn_out=True),
    _row("res4_conv1", "model", (NB, 4, 4, 1280), (1280, 3), rowvec=ROWS4, gn_out=True),
    _row("res4_conv2", "model", (NB, 4, 4, 1280), (1280, 3), res=True, gn_out=True),
    _row("upsample4_phase", "model", (NB, 4, 4, 1280), (1280, 3), upsample=True, phase=True, gn_out=True),
    # ---- SD-VAE (16 images per call)
    _row("vae_enc_in", "model", (16, 256, 256, 8), (128, 3), gn_out=True),
    _row("vae_res256", "model", (16, 256, 256, 128), (128, 3), aff=(1, True), res=True, gn_out=True),
    _row("vae_down256", "model", (16, 256, 256, 128), (128, 3), stride=2, pad=0, out_hw=(128, 128), gn_out=True),
    _row("vae_res128_in128", "model", (16, 128, 128, 128), (256, 3), aff=(1, True), gn_out=True),
    _row("vae_res64_in256", "model", (16, 64, 64, 256), (512, 3), aff=(1, True), gn_out=True),
    _row("vae_res32", "model", (16, 32, 32, 512), (512, 3), aff=(1, True), res=True, gn_out=True),
    _row("vae_attn_qkv", "model", (16, 32, 32, 512), (1536, 1)),
    _row("vae_attn_out", "model", (16, 32, 32, 512), (512, 1), res=True, gn_out=True),
    _row("vae_enc_out", "model", (16, 32, 32, 512), (8, 3), aff=(1, True)),
    _row("vae_quant", "model", (16, 32, 32, 8), (8, 1), out_f32=True),
    _row("vae_dec_in", "model", (16, 32, 32, 8), (512, 3), gn_out=True),
    _row("vae_upsample32_phase", "model", (16, 32, 32, 512), (512, 3), upsample=True, phase=True, gn_out=True),
    _row("vae_upsample128_phase", "model", (16, 128, 128, 256), (256, 3), upsample=True, phase=True, gn_out=True),
    _row("vae_dec_out", "model", (16, 256, 256, 128), (8, 3), aff=(1, True)),
    # ---- tiles of pick_tile, and tile 6 through key 2
    _lin("tile_128x128", "edge", 65536, 256, 384),
    _lin("tile_128x160", "edge", 65536, 1280, 320),
    _lin("tile_128x64", "edge", 65536, 256, 64),
    _lin("tile_64x64", "edge", 192, 256, 64),
    _lin("tile_128x32", "edge", 4096, 256, 32),
    _lin("tile_256x256", "edge", 65536, 512, 512),
    _lin("tile_256x128_forced", "edge", 4096, 256, 384, tune={2: 6}),
    _row("tile_256x256_forced_affine", "edge", (4, 16, 16, 256), (512, 1), tune={2: 5}, aff=(1, False)),
    _lin("forced_regstage", "edge", 4096, 256, 384, tune={1: 1}),
    # ---- gather forms and epilogues
    _row("conv3_tap_major_no_buf", "edge", (2, 24, 24, 32), (64, 3)),
    _row("conv3_stride2_buf", "edge", (2, 24, 24, 64), (128, 3), stride=2, pad=1),
    _lin("k_padded_no_buf", "edge", 4096, 96, 128),
    _lin("epi_geglu", "edge", 4096, 256, 512, act=ops.ACT_GEGLU),
    _lin("epi_any_gelu", "edge", 4096, 256, 384, act=ops.ACT_GELU),
    _lin("epi_any_f32", "edge", 4096, 256, 384, out_f32=True),
    _lin("epi_any_narrow_n", "edge", 4096, 256, 4, n_out=4),
    _row("epi_plainp", "edge", (2, 8, 8, 64), (128, 3), upsample=True, phase=True),
    # ---- row-block GEMM: the 12 flag sets at K = 320 and K = 640 (FM 2 and, key 15 off, FM 1)
    *[_lin(f"rb{k}_{nm}{'_fm1' if fm1 else ''}", "edge", 65536, k, 320 if "geglu" not in nm else 640,
           tune={**({15: 0} if fm1 else {}), **({20: 1} if "res" in nm and k == 640 else {})}, **kw)
      for k in (320, 640) for fm1 in ((False, True) if k == 640 else (False,))
      for nm, kw in (("plain", {}), ("ln", dict(ln=True)), ("ln_rv", dict(ln=True, rowvec=(1024, 16))),
                     ("res", dict(res=True)), ("ln_res", dict(ln=True, res=True)),
                     ("ln_geglu", dict(ln=True, act=ops.ACT_GEGLU)), ("geglu", dict(act=ops.ACT_GEGLU)),
                     ("stats", dict(stats=True)), ("res_stats", dict(res=True, stats=True)),
                     ("res_gncs", dict(res=True, gn_out=True)))],
    *[_row(f"rb{k}_{nm}", "edge", (256, 16, 16, k), (320, 1), aff=(1, False), **kw)
      for k in (320, 640) for nm, kw in (("aff", {}), ("aff_stats", dict(stats=True)))],
    # ---- the cs / stats chain
    _lin("chain_rb_stats_cs_pass", "edge", 65536, 320, 320, stats=True, gn_out=True),
    _lin("chain_rb_cs_pass", "edge", 65536, 320, 320, gn_out=True),
    _lin("chain_rb_stats_dropped_wide_n", "edge", 2048, 320, 640, stats=True),
    _lin("chain_rb_stats_dropped_cs_pass", "edge", 2048, 320, 640, stats=True, gn_out=True),
    _lin("chain_rb_res_stats_cs_pass", "edge", 65536, 320, 320, res=True, stats=True, gn_out=True),
    # (no LN | STATS instance: the statistics go; no round finds "statistics dropped, sums fused" -- the only
    # instance with the sums is RES | GNCS, and RES | STATS exists wherever it does)
    _lin("chain_rb_ln_stats_dropped_cs_pass", "edge", 65536, 320, 320, ln=True, res=True, stats=True, gn_out=True),
    _lin("chain_tiled_stats_cs_epi", "edge", 4096, 256, 384, stats=True, gn_out=True),
    _lin("chain_tiled_cs_pass_small_tile", "edge", 4096, 256, 64, gn_out=True),
    _lin("chain_tiled_cs_pass_256_rows", "edge", 65536, 512, 512, gn_out=True),
    _row("chain_tiled_phase_cs_pass_rows_mo", "edge", (2, 8, 8, 64), (128, 3), upsample=True, phase=True, gn_out=True),
    _lin("rowblock_off", "edge", 65536, 320, 320, tune={6: 0}),
    # ---- halo-tile conv
    _row("halo_bn160_th16", "edge", (2, 16, 16, 64), (160, 3)),
    _row("halo_bn128_th8", "edge", (2, 16, 16, 64), (128, 3)),
    _row("halo_bn128_th16_cin512", "edge", (2, 16, 16, 512), (128, 3)),
    _row("halo_bn128_th16_key16", "edge", (2, 16, 16, 64), (128, 3), tune={16: 0}),
    _row("halo_bn16", "edge", (2, 16, 16, 64), (8, 3)),
    _row("halo_gn_cs", "edge", (2, 16, 16, 64), (160, 3), aff=(1, True), gn_out=True),
    _row("halo_cs", "edge", (2, 16, 16, 64), (128, 3), gn_out=True),
    _row("halo_upsample_9tap", "edge", (2, 16, 16, 64), (160, 3), upsample=True),
    _row("halo_phase", "edge", (2, 16, 16, 64), (160, 3), upsample=True, phase=True, gn_out=True),
    _row("halo_phase_th8", "edge", (2, 16, 16, 64), (128, 3), upsample=True, phase=True),
    _row("halo_off", "edge", (2, 16, 16, 64), (160, 3), tune={8: 0}),
    _row("halo_narrow_off", "edge", (2, 16, 16, 64), (8, 3), tune={19: 0}),
    _row("halo_upsample_off", "edge", (2, 16, 16, 64), (160, 3), upsample=True, tune={18: 0}),
    # ---- split-K
    _row("split_cost_model", "edge", (16, 4, 4, 1280), (1280, 3), workspace_bytes=WS),
    _row("split_none_without_workspace", "edge", (16, 4, 4, 1280), (1280, 3)),
    _lin("split_forced", "edge", 4096, 1024, 384, split_k=4, workspace_bytes=WS),
    _lin("split_forced_no_workspace", "edge", 4096, 1024, 384, split_k=4),
    _row("split_fitted_to_2", "edge", (16, 4, 4, 1280), (1280, 3), split_k=8, workspace_bytes=2 * 256 * 1280 * 4 + 64),
    _row("split_fitted_to_1", "edge", (16, 4, 4, 1280), (1280, 3), split_k=8, workspace_bytes=256 * 1280 * 4),
    _lin("split_forced_rowblock_shape", "edge", 65536, 320, 320, split_k=2, workspace_bytes=WS),
    _lin("split_fitted_to_1_rowblock", "edge", 65536, 320, 320, split_k=2),
    _lin("split_key3", "edge", 4096, 1024, 384, tune={2: 1, 3: 2}, workspace_bytes=WS),
    # K = 640 on few rows: the cost model splits K where it has a workspace, and a split call is
    # not the row-block kernel's (ops.conv_path asks without one and hears 1)
    _lin("rb640_few_rows_workspace_splits", "edge", 256, 640, 192, workspace_bytes=WS),
    _lin("rb640_few_rows", "edge", 256, 640, 192),
    # ---- the keys read outside the planner's own file: 7 and 20 by the row-block GEMM's, 13 by the halo conv's
    _lin("rb640_key7_off", "edge", 256, 640, 640, tune={7: 0}),
    _lin("rb640_res_key20", "edge", 256, 640, 640, tune={20: 1}, res=True),
    _row("halo_bn128_key13", "edge", (2, 16, 16, 64), (640, 3), tune={13: 1}),
]

# rows where 41d7641's ls_conv_path named another family than its ls_conv2d launched
PATH_DIFFERS = {
    "chain_rb_stats_dropped_wide_n": "the walk kept row_stats_out and found no row-block instance; ls_conv2d retried without",
    "chain_rb_stats_dropped_cs_pass": "the same retry, the column sums by the read pass",
    "chain_rb_ln_stats_dropped_cs_pass": "the same retry: there is no LN | RES | STATS instance",
    "split_fitted_to_1_rowblock": "the walk knew nothing of the workspace fallback: split 2 kept it off the row-block kernel",
    "rb640_few_rows_workspace_splits": "41d7641's ops.conv_path could only ask without the workspace (1); its ls_conv2d, "
                                       "given one, split K and launched the tiled kernel",
}


def _fmt(p):
    """A plan as one line: family, instance, geometry, trailing passes, workspace."""
    if p is None:
        return "refused: " + _lib.load().ls_last_error().decode()
    f = p["family"]
    if f == 1:
        inst = f"rowblock kt{p['rb_kt']} fm{p['rb_fm']} flags{p['rb_flags']}"
    elif f in (3, 4):
        inst = f"halo bn{p['halo_bn']} th{p['halo_th']} gn{p['halo_gn']} cs{p['halo_cs']} ph{p['halo_ph']}"
    else:
        inst = f"tile {p['bm']}x{p['bn']} ks{p['ks']} tapu{p['tapu']} buf{p['buf']} epi{p['epi']}"
    tail = ("+reduce" if p["reduce"] else "") + (f"+colsum{p['colsum_rows']}" if p["colsum_rows"] else "") + \
        ("+rowstats" if p["row_stats"] else "")
    return f"{f}: {inst} split{p['split']} | {p['grid']}x{p['threads']} lds{p['lds_bytes']} | {tail or '-'} | ws{p['workspace_bytes']}"


def _args(call):
    """(x, Packed, kwargs) of ops.conv for a corpus call; untouched torch.empty storage."""
    call = dict(call)
    n, H, W, C1 = call.pop("x")
    N, ks = call.pop("w")
    c2 = call.pop("c2", 0)
    C1 -= c2
    cin = C1 + c2
    K = -(-ks * ks * cin // 64) * 64
    pw = ops.Packed(torch.empty((N, K), dtype=BF), torch.empty(N), cin, ks, call.pop("n_out", N))
    if call.pop("phase", False):
        pw.phase = torch.empty((4, N, 4 * cin), dtype=BF)
    kw = {}
    x = torch.empty((n, H, W, C1), dtype=BF)
    if c2:
        kw["x2"] = torch.empty((n, H, W, c2), dtype=BF)
    if "aff" in call:
        ipp, silu = call.pop("aff")
        kw["aff"] = (torch.empty(n // ipp, cin), torch.empty(n // ipp, cin), ipp, silu)
    if "out_hw" in call:
        Ho, Wo = call["out_hw"]
    elif ks == 1:
        Ho, Wo = H, W
    else:
        s, pad, up = call.get("stride", 1), call.get("pad", 1), 2 if call.get("upsample") else 1
        Ho, Wo = (up * H + 2 * pad - 3) // s + 1, (up * W + 2 * pad - 3) // s + 1
    M = n * Ho * Wo
    if "rowvec" in call:
        rv = call.pop("rowvec")
        rpv, mod = rv if isinstance(rv, tuple) else (rv, 0)
        kw["rowvec"] = (torch.empty(mod or -(-M // rpv), N), rpv, N, mod)
    if call.pop("res", False):
        kw["res"] = torch.empty((n, Ho, Wo, pw.n_out), dtype=BF)
    if call.pop("ln", False):
        pw.colsum = torch.empty(N)
        kw["ln_stats"] = torch.empty(M, 2)
    if call.pop("stats", False):
        kw["stats_out"] = torch.empty(M, 2)
    kw.update(call)
    return x, pw, kw


def _ask(row, what):
    _, kind, call, tune = row
    if kind == "model":  # as ops.conv launches them: with the workspace
        call = dict(call, workspace_bytes=WS)
    lib = _lib.load()
    try:
        for k, v in tune.items():
            assert lib.ls_set_tuning(k, v) == 0, lib.ls_last_error().decode()
        x, pw, kw = _args(call)
        return what(x, pw, **kw)
    finally:
        for k, v in DEFAULTS.items():
            assert lib.ls_set_tuning(k, v) == 0


@pytest.fixture(scope="module")
def parent_paths():
    return json.load(open(os.path.join(REPO, "tests", "golden", "conv_path_parent.json")))


def test_corpus_names_are_unique_and_pinned():
    names = [r[0] for r in CORPUS]
    assert len(set(names)) == len(names)
    assert set(names) == set(PINS)
    assert set(PATH_DIFFERS) <= {r[0] for r in CORPUS if r[1] == "edge"}


@pytest.mark.parametrize("row", CORPUS, ids=[r[0] for r in CORPUS])
def test_plan_is_pinned(row, parent_paths):
    name, kind = row[0], row[1]
    plan = _ask(row, ops.conv_plan)
    print(name, _fmt(plan))
    assert _fmt(plan) == PINS[name]
    path = _ask(row, ops.conv_path)
    assert path == (plan["family"] if plan else -1)
    if name not in PATH_DIFFERS:
        assert path == parent_paths[name], "ls_conv_path answers differently from commit 41d7641"


def test_corpus_reaches_every_branch():
    plans = {r[0]: _ask(r, ops.conv_plan) for r in CORPUS}
    ps = [p for p in plans.values() if p]
    tiled = [p for p in ps if p["family"] in (0, 2, 5)]
    assert {p["family"] for p in ps} == {0, 1, 2, 3, 4, 5}
    assert {(p["bm"], p["bn"]) for p in tiled} == {(128, 128), (128, 160), (128, 64), (64, 64), (128, 32), (256, 256),
                                                   (256, 128)}
    assert {p["buf"] for p in tiled if p["family"] != 2} == {0, 1}
    assert {p["epi"] for p in tiled if p["family"] != 2} == {0, 1, 2, 3}
    rb = {(p["rb_kt"], p["rb_fm"], p["rb_flags"]) for p in ps if p["family"] == 1}
    flags = (0, 1, 5, 2, 3, 9, 8, 16, 18, 34, 64, 80)
    assert {(10, 2, f) for f in flags} <= rb and {(20, 1, f) for f in flags} <= rb
    assert {(20, 2, f) for f in flags if not f & (2 | 16 | 32 | 64)} <= rb
    assert not {(kt, fm, f) for kt, fm, f in rb if kt == 20 and fm == 2 and f & (2 | 16 | 32 | 64)}  # (not compiled)
    assert all(p["lds_bytes"] <= 160 << 10 for p in ps)  # what a gfx950 workgroup can have
    halo = [p for p in ps if p["family"] in (3, 4)]
    assert {(p["halo_bn"], p["halo_th"]) for p in halo} == {(160, 16), (128, 8), (128, 16), (16, 8)}
    assert {(p["halo_gn"], p["halo_cs"]) for p in halo} >= {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {p["halo_ph"] for p in halo} == {0, 1}
    assert plans["split_cost_model"]["split"] > 1 and plans["split_cost_model"]["reduce"]
    assert plans["split_forced"]["split"] == 4
    assert plans["split_fitted_to_2"]["split"] == 2 and plans["split_fitted_to_1"]["split"] == 1
    assert plans["split_fitted_to_1"]["workspace_bytes"] == 8 * 256 * 1280 * 4  # what it asked for
    # the chain: statistics dropped to reach the row-block kernel (ntn != 1), ls_row_stats at the end
    p = plans["chain_rb_stats_dropped_wide_n"]
    assert p["family"] == 1 and not p["rb_flags"] & 16 and p["row_stats"] and p["grid"] > 2048 // 256
    assert plans["chain_tiled_cs_pass_256_rows"]["bm"] == 256 and plans["chain_tiled_cs_pass_256_rows"]["colsum_rows"] == 65536
    p = plans["chain_tiled_phase_cs_pass_rows_mo"]
    assert p["family"] == 5 and p["colsum_rows"] == 2 * 16 * 16  # the rows of y, four times the M of a parity
    p = plans["tile_256x256_forced_affine"]
    assert (p["family"], p["bm"], p["bn"]) == (2, 128, 128)


def _desc(**over):
    """A valid 3x3 descriptor (dummy pointers, never dereferenced) with fields replaced."""
    d = _lib.ConvDesc()
    d.x1 = d.w = d.y = 4096
    d.C1, d.ld1, d.n_img, d.H, d.W, d.Ho, d.Wo = 64, 64, 2, 16, 16, 16, 16
    d.ksize, d.stride, d.pad, d.K, d.N, d.ldy = 3, 1, 1, 576, 128, 128
    for k, v in over.items():
        setattr(d, k, v)
    return d


LINEAR = dict(ksize=1, pad=0, K=64)
# one descriptor per refusal of the plan
REFUSALS = [
    (dict(x1=None), "ls_conv2d: null pointer"),
    (dict(ksize=5), "ls_conv2d: ksize must be 1 or 3"),
    (dict(C1=60), "ls_conv2d: channels must be multiples of 8"),
    (dict(C2=64, K=1152), "ls_conv2d: C2 > 0 needs x2"),
    (dict(ld1=68), "ls_conv2d: pixel pitch must be a multiple of 8"),
    (dict(upsample=3), "ls_conv2d: upsample must be 0, 1 or 2"),
    (dict(upsample=2, K=256, Ho=32, Wo=32, stride=2),
     "ls_conv2d: upsample 2 (phase-packed weights) needs ksize 3, Cin % 64 == 0, K == 4 Cin, "
     "no affine prologue, stride 1, pad 1, Ho x Wo = 2H x 2W"),
    (dict(K=640), "ls_conv2d: K must be ksize^2*Cin rounded up to 64"),
    (dict(LINEAR, stride=2), "ls_conv2d: ksize 1 must be stride 1 with no resampling"),
    (dict(LINEAR, act=ops.ACT_GEGLU, N=48), "ls_conv2d: GEGLU needs N % 32 == 0"),
    (dict(LINEAR, act=ops.ACT_GEGLU, res=4096, ldr=64), "ls_conv2d: GEGLU takes no rowvec, residual or out_scale"),
    (dict(aff_scale=4096), "ls_conv2d: affine prologue needs shift and imgs_per_sample"),
    (dict(rowvec=4096), "ls_conv2d: rowvec needs rows_per_vec"),
    (dict(n_img=0), "ls_conv2d: bad M"),
    (dict(ln_rowstats=4096, ln_colsum=4096), "ls_conv2d: ln_rowstats needs ln_colsum, ksize 1"),
    (dict(row_stats_out=4096), "ls_conv2d: row_stats_out needs ksize 1, bf16 output, no GEGLU"),
    (dict(gn_colsum_out=4096, N=124), "ls_conv2d: gn_colsum_out needs M % 128 == 0, N % 8 == 0, bf16 output, no GEGLU"),
    (dict(upsample=2, K=256, Ho=32, Wo=32, N=1280, rowvec=4096, rows_per_vec=256),
     "ls_conv2d: no phase-form kernel for this shape (ls_conv_path -1): use upsample = 1"),
]


@pytest.mark.parametrize("over,msg", REFUSALS, ids=[m.split(": ", 1)[1][:28] for _, m in REFUSALS])
def test_refusals(over, msg):
    lib = _lib.load()
    d, info = _desc(**over), _lib.ConvPlanInfo()
    assert lib.ls_conv_plan(C.byref(d), C.byref(info)) == 1
    assert lib.ls_last_error().decode() == msg
    assert lib.ls_conv_path(C.byref(d)) == -1
    assert lib.ls_last_error().decode() == msg
    assert lib.ls_conv_workspace_bytes(C.byref(d)) == 0


PINS = {
    "unet_conv_in": "0: tile 128x160 ks3 tapu0 buf0 epi0 split1 | 12288x256 lds73728 | - | ws0",
    "res32_conv1": "3: halo bn160 th16 gn1 cs1 ph0 split1 | 6144x512 lds153600 | - | ws0",
    "res32_conv2": "3: halo bn160 th16 gn1 cs1 ph0 split1 | 6144x512 lds153600 | - | ws0",
    "down32": "0: tile 128x160 ks3 tapu1 buf1 epi0 split1 | 3072x256 lds73728 | - | ws0",
    "proj_in32": "1: rowblock kt10 fm2 flags80 split1 | 3072x512 lds63744 | - | ws0",
    "qkv32": "1: rowblock kt10 fm2 flags1 split1 | 3072x512 lds63744 | - | ws0",
    "motion_qkv32": "1: rowblock kt10 fm2 flags5 split1 | 3072x512 lds63744 | - | ws0",
    "attn_out32": "1: rowblock kt10 fm2 flags18 split1 | 3072x512 lds112896 | - | ws0",
    "q2_32": "1: rowblock kt10 fm2 flags1 split1 | 3072x512 lds63744 | - | ws0",
    "audio_kv": "0: tile 128x160 ks1 tapu0 buf1 epi0 split1 | 1200x256 lds73728 | - | ws0",
    "ff1_32": "1: rowblock kt10 fm2 flags9 split1 | 3072x512 lds63744 | - | ws0",
    "ff2_32": "0: tile 128x160 ks1 tapu0 buf1 epi0 split1 | 12288x256 lds73728 | - | ws0",
    "proj_out32": "1: rowblock kt10 fm2 flags34 split1 | 3072x512 lds116992 | - | ws0",
    "up32_conv1_cat": "3: halo bn160 th16 gn1 cs1 ph0 split1 | 6144x512 lds153600 | - | ws0",
    "up32_shortcut_cat": "0: tile 128x160 ks1 tapu0 buf1 epi0 split1 | 12288x256 lds73728 | - | ws0",
    "unet_conv_out": "3: halo bn16 th8 gn1 cs0 ph0 split1 | 6144x128 lds52224 | - | ws0",
    "res16_conv1_in320": "3: halo bn160 th16 gn1 cs1 ph0 split1 | 3072x512 lds153600 | - | ws0",
    "res16_shortcut": "1: rowblock kt10 fm2 flags0 split1 | 768x512 lds63744 | - | ws0",
    "res16_conv2": "3: halo bn160 th16 gn1 cs1 ph0 split1 | 3072x512 lds153600 | - | ws0",
    "down16": "0: tile 128x160 ks3 tapu1 buf1 epi0 split1 | 1536x256 lds73728 | - | ws0",
    "proj_in16": "1: rowblock kt20 fm1 flags80 split1 | 1536x512 lds125184 | - | ws0",
    "qkv16": "1: rowblock kt20 fm2 flags1 split1 | 768x512 lds125184 | - | ws0",
    "attn_out16": "0: tile 128x160 ks1 tapu0 buf1 epi0 split1 | 6144x256 lds73728 | +rowstats | ws0",
    "ff1_16": "1: rowblock kt20 fm2 flags9 split1 | 768x512 lds125184 | - | ws0",
    "ff2_16": "0: tile 128x160 ks1 tapu0 buf1 epi0 split1 | 6144x256 lds73728 | - | ws0",
    "proj_out16": "0: tile 128x160 ks1 tapu0 buf1 epi0 split1 | 6144x256 lds73728 | - | ws0",
    "up16_conv1_cat": "3: halo bn160 th16 gn1 cs1 ph0 split1 | 3072x512 lds153600 | - | ws0",
    "upsample16_phase": "4: halo bn160 th16 gn0 cs1 ph1 split1 | 12288x512 lds153600 | - | ws0",
    "res8_conv1_in640_affine": "2: tile 128x160 ks3 tapu1 buf0 epi-1 split1 | 3072x256 lds0 | - | ws0",
    "res8_conv1_in640": "0: tile 256x256 ks3 tapu1 buf1 epi0 split1 | 960x512 lds133120 | +colsum49152 | ws0",
    "res8_conv2": "0: tile 256x256 ks3 tapu1 buf1 epi0 split1 | 960x512 lds133120 | +colsum49152 | ws0",
    "res8_shortcut": "1: rowblock kt20 fm2 flags0 split1 | 384x512 lds125184 | - | ws0",
    "down8": "0: tile 256x256 ks3 tapu1 buf1 epi0 split1 | 240x512 lds133120 | +colsum12288 | ws0",
    "proj_in8_affine": "2: tile 128x160 ks1 tapu0 buf0 epi-1 split1 | 3072x256 lds0 | +rowstats | ws0",
    "proj_in8": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 960x512 lds133120 | +rowstats | ws0",
    "qkv8": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 2880x512 lds133120 | - | ws0",
    "attn_out8": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 960x512 lds133120 | +rowstats | ws0",
    "ff1_8": "0: tile 256x256 ks1 tapu0 buf1 epi1 split1 | 7680x512 lds133120 | - | ws0",
    "ff2_8": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 960x512 lds133120 | - | ws0",
    "proj_out8": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 960x512 lds133120 | +colsum49152 | ws0",
    "up8_conv1_cat": "0: tile 256x256 ks3 tapu1 buf1 epi0 split1 | 960x512 lds133120 | +colsum49152 | ws0",
    "up8_shortcut_cat": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 960x512 lds133120 | - | ws0",
    "upsample8_phase": "5: tile 256x256 ks3 tapu1 buf1 epi3 split1 | 3840x512 lds133120 | +colsum196608 | ws0",
    "res4_conv1": "0: tile 256x256 ks3 tapu1 buf1 epi0 split1 | 240x512 lds133120 | +colsum12288 | ws0",
    "res4_conv2": "0: tile 256x256 ks3 tapu1 buf1 epi0 split1 | 240x512 lds133120 | +colsum12288 | ws0",
    "upsample4_phase": "5: tile 256x256 ks3 tapu1 buf1 epi3 split1 | 960x512 lds133120 | +colsum49152 | ws0",
    "vae_enc_in": "0: tile 128x128 ks3 tapu0 buf0 epi0 split1 | 8192x256 lds65536 | - | ws0",
    "vae_res256": "3: halo bn128 th8 gn1 cs1 ph0 split1 | 8192x256 lds80896 | - | ws0",
    "vae_down256": "0: tile 128x128 ks3 tapu1 buf1 epi0 split1 | 2048x256 lds65536 | - | ws0",
    "vae_res128_in128": "3: halo bn128 th8 gn1 cs1 ph0 split1 | 4096x256 lds80896 | - | ws0",
    "vae_res64_in256": "3: halo bn128 th8 gn1 cs1 ph0 split1 | 2048x256 lds80896 | - | ws0",
    "vae_res32": "3: halo bn128 th16 gn1 cs1 ph0 split1 | 256x512 lds161792 | - | ws0",
    "vae_attn_qkv": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 384x512 lds133120 | - | ws0",
    "vae_attn_out": "0: tile 128x128 ks1 tapu0 buf1 epi0 split1 | 512x256 lds65536 | - | ws0",
    # (the cost model's split is asked for and then ignored by the halo kernel: kept as it was)
    "vae_enc_out": "3: halo bn16 th8 gn1 cs0 ph0 split4 | 128x128 lds52224 | - | ws2097152",
    "vae_quant": "0: tile 128x32 ks1 tapu0 buf0 epi2 split1 | 128x256 lds40960 | - | ws0",
    "vae_dec_in": "0: tile 128x128 ks3 tapu0 buf0 epi0 split1 | 512x256 lds65536 | - | ws0",
    "vae_upsample32_phase": "4: halo bn128 th16 gn0 cs1 ph1 split1 | 1024x512 lds161792 | - | ws0",
    "vae_upsample128_phase": "4: halo bn128 th8 gn0 cs1 ph1 split1 | 16384x256 lds80896 | - | ws0",
    "vae_dec_out": "3: halo bn16 th8 gn1 cs0 ph0 split1 | 8192x128 lds52224 | - | ws0",
    "tile_128x128": "0: tile 128x128 ks1 tapu0 buf1 epi0 split1 | 1536x256 lds65536 | - | ws0",
    "tile_128x160": "0: tile 128x160 ks1 tapu0 buf1 epi0 split1 | 1024x256 lds73728 | - | ws0",
    "tile_128x64": "0: tile 128x64 ks1 tapu0 buf1 epi0 split1 | 512x256 lds49152 | - | ws0",
    "tile_64x64": "0: tile 64x64 ks1 tapu0 buf1 epi0 split1 | 3x256 lds32768 | - | ws0",
    "tile_128x32": "0: tile 128x32 ks1 tapu0 buf1 epi0 split1 | 32x256 lds40960 | - | ws0",
    "tile_256x256": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 512x512 lds133120 | - | ws0",
    "tile_256x128_forced": "0: tile 256x128 ks1 tapu0 buf1 epi0 split1 | 48x512 lds98304 | - | ws0",
    "tile_256x256_forced_affine": "2: tile 128x128 ks1 tapu0 buf0 epi-1 split1 | 32x256 lds0 | - | ws0",
    "forced_regstage": "2: tile 128x64 ks1 tapu0 buf0 epi-1 split1 | 192x256 lds0 | - | ws0",
    "conv3_tap_major_no_buf": "0: tile 64x64 ks3 tapu0 buf0 epi0 split1 | 18x256 lds32768 | - | ws0",
    "conv3_stride2_buf": "0: tile 64x64 ks3 tapu1 buf1 epi0 split1 | 10x256 lds32768 | - | ws0",
    "k_padded_no_buf": "0: tile 64x64 ks1 tapu0 buf0 epi0 split1 | 128x256 lds32768 | - | ws0",
    "epi_geglu": "0: tile 128x64 ks1 tapu0 buf1 epi1 split1 | 256x256 lds49152 | - | ws0",
    "epi_any_gelu": "0: tile 128x64 ks1 tapu0 buf1 epi2 split1 | 192x256 lds49152 | - | ws0",
    "epi_any_f32": "0: tile 128x64 ks1 tapu0 buf1 epi2 split1 | 192x256 lds49152 | - | ws0",
    "epi_any_narrow_n": "0: tile 128x32 ks1 tapu0 buf1 epi2 split1 | 32x256 lds40960 | - | ws0",
    "epi_plainp": "5: tile 64x64 ks3 tapu1 buf1 epi3 split1 | 16x256 lds32768 | - | ws0",
    "rb320_plain": "1: rowblock kt10 fm2 flags0 split1 | 256x512 lds63744 | - | ws0",
    "rb320_ln": "1: rowblock kt10 fm2 flags1 split1 | 256x512 lds63744 | - | ws0",
    "rb320_ln_rv": "1: rowblock kt10 fm2 flags5 split1 | 256x512 lds63744 | - | ws0",
    "rb320_res": "1: rowblock kt10 fm2 flags2 split1 | 256x512 lds112896 | - | ws0",
    "rb320_ln_res": "1: rowblock kt10 fm2 flags3 split1 | 256x512 lds112896 | - | ws0",
    "rb320_ln_geglu": "1: rowblock kt10 fm2 flags9 split1 | 256x512 lds63744 | - | ws0",
    "rb320_geglu": "1: rowblock kt10 fm2 flags8 split1 | 256x512 lds63744 | - | ws0",
    "rb320_stats": "1: rowblock kt10 fm2 flags16 split1 | 256x512 lds63744 | - | ws0",
    "rb320_res_stats": "1: rowblock kt10 fm2 flags18 split1 | 256x512 lds112896 | - | ws0",
    "rb320_res_gncs": "1: rowblock kt10 fm2 flags34 split1 | 256x512 lds116992 | - | ws0",
    "rb640_plain": "1: rowblock kt20 fm2 flags0 split1 | 256x512 lds125184 | - | ws0",
    "rb640_ln": "1: rowblock kt20 fm2 flags1 split1 | 256x512 lds125184 | - | ws0",
    "rb640_ln_rv": "1: rowblock kt20 fm2 flags5 split1 | 256x512 lds125184 | - | ws0",
    # (key 20 with key 15: a residual keeps one fragment per wave -- at two, the 174336 bytes of LDS
    # planned before were more than a workgroup can have and ls_conv2d failed at the launch)
    "rb640_res": "1: rowblock kt20 fm1 flags2 split1 | 512x512 lds149760 | - | ws0",
    "rb640_ln_res": "1: rowblock kt20 fm1 flags3 split1 | 512x512 lds149760 | - | ws0",
    "rb640_ln_geglu": "1: rowblock kt20 fm2 flags9 split1 | 256x512 lds125184 | - | ws0",
    "rb640_geglu": "1: rowblock kt20 fm2 flags8 split1 | 256x512 lds125184 | - | ws0",
    "rb640_stats": "1: rowblock kt20 fm1 flags16 split1 | 512x512 lds125184 | - | ws0",
    "rb640_res_stats": "1: rowblock kt20 fm1 flags18 split1 | 512x512 lds149760 | - | ws0",
    "rb640_res_gncs": "1: rowblock kt20 fm1 flags34 split1 | 512x512 lds153856 | - | ws0",
    "rb640_plain_fm1": "1: rowblock kt20 fm1 flags0 split1 | 512x512 lds125184 | - | ws0",
    "rb640_ln_fm1": "1: rowblock kt20 fm1 flags1 split1 | 512x512 lds125184 | - | ws0",
    "rb640_ln_rv_fm1": "1: rowblock kt20 fm1 flags5 split1 | 512x512 lds125184 | - | ws0",
    "rb640_res_fm1": "1: rowblock kt20 fm1 flags2 split1 | 512x512 lds149760 | - | ws0",
    "rb640_ln_res_fm1": "1: rowblock kt20 fm1 flags3 split1 | 512x512 lds149760 | - | ws0",
    "rb640_ln_geglu_fm1": "1: rowblock kt20 fm1 flags9 split1 | 512x512 lds125184 | - | ws0",
    "rb640_geglu_fm1": "1: rowblock kt20 fm1 flags8 split1 | 512x512 lds125184 | - | ws0",
    "rb640_stats_fm1": "1: rowblock kt20 fm1 flags16 split1 | 512x512 lds125184 | - | ws0",
    "rb640_res_stats_fm1": "1: rowblock kt20 fm1 flags18 split1 | 512x512 lds149760 | - | ws0",
    "rb640_res_gncs_fm1": "1: rowblock kt20 fm1 flags34 split1 | 512x512 lds153856 | - | ws0",
    "rb320_aff": "1: rowblock kt10 fm2 flags64 split1 | 256x512 lds63744 | - | ws0",
    "rb320_aff_stats": "1: rowblock kt10 fm2 flags80 split1 | 256x512 lds63744 | - | ws0",
    "rb640_aff": "1: rowblock kt20 fm1 flags64 split1 | 512x512 lds125184 | - | ws0",
    "rb640_aff_stats": "1: rowblock kt20 fm1 flags80 split1 | 512x512 lds125184 | - | ws0",
    "chain_rb_stats_cs_pass": "1: rowblock kt10 fm2 flags16 split1 | 256x512 lds63744 | +colsum65536 | ws0",
    "chain_rb_cs_pass": "1: rowblock kt10 fm2 flags0 split1 | 256x512 lds63744 | +colsum65536 | ws0",
    "chain_rb_stats_dropped_wide_n": "1: rowblock kt10 fm2 flags0 split1 | 160x512 lds63744 | +rowstats | ws0",
    "chain_rb_stats_dropped_cs_pass": "1: rowblock kt10 fm2 flags0 split1 | 160x512 lds63744 | +colsum2048+rowstats | ws0",
    "chain_rb_res_stats_cs_pass": "1: rowblock kt10 fm2 flags18 split1 | 256x512 lds112896 | +colsum65536 | ws0",
    "chain_rb_ln_stats_dropped_cs_pass": "1: rowblock kt10 fm2 flags3 split1 | 256x512 lds112896 | +colsum65536+rowstats | ws0",
    "chain_tiled_stats_cs_epi": "0: tile 128x64 ks1 tapu0 buf1 epi0 split1 | 192x256 lds49152 | +rowstats | ws0",
    "chain_tiled_cs_pass_small_tile": "0: tile 64x64 ks1 tapu0 buf1 epi0 split1 | 64x256 lds32768 | +colsum4096 | ws0",
    "chain_tiled_cs_pass_256_rows": "0: tile 256x256 ks1 tapu0 buf1 epi0 split1 | 512x512 lds133120 | +colsum65536 | ws0",
    "chain_tiled_phase_cs_pass_rows_mo": "5: tile 64x64 ks3 tapu1 buf1 epi3 split1 | 16x256 lds32768 | +colsum512 | ws0",
    "rowblock_off": "0: tile 128x160 ks1 tapu0 buf1 epi0 split1 | 1024x256 lds73728 | - | ws0",
    "halo_bn160_th16": "3: halo bn160 th16 gn0 cs0 ph0 split1 | 2x512 lds153600 | - | ws0",
    "halo_bn128_th8": "3: halo bn128 th8 gn0 cs0 ph0 split1 | 4x256 lds80896 | - | ws0",
    "halo_bn128_th16_cin512": "3: halo bn128 th16 gn0 cs0 ph0 split1 | 2x512 lds161792 | - | ws0",
    "halo_bn128_th16_key16": "3: halo bn128 th16 gn0 cs0 ph0 split1 | 2x512 lds161792 | - | ws0",
    "halo_bn16": "3: halo bn16 th8 gn0 cs0 ph0 split1 | 4x128 lds52224 | - | ws0",
    "halo_gn_cs": "3: halo bn160 th16 gn1 cs1 ph0 split1 | 2x512 lds153600 | - | ws0",
    "halo_cs": "3: halo bn128 th8 gn0 cs1 ph0 split1 | 4x256 lds80896 | - | ws0",
    "halo_upsample_9tap": "3: halo bn160 th16 gn0 cs0 ph0 split1 | 8x512 lds153600 | - | ws0",
    "halo_phase": "4: halo bn160 th16 gn0 cs1 ph1 split1 | 8x512 lds153600 | - | ws0",
    "halo_phase_th8": "4: halo bn128 th8 gn0 cs0 ph1 split1 | 16x256 lds80896 | - | ws0",
    "halo_off": "0: tile 64x64 ks3 tapu1 buf1 epi0 split1 | 24x256 lds32768 | - | ws0",
    "halo_narrow_off": "0: tile 128x32 ks3 tapu1 buf1 epi0 split1 | 4x256 lds40960 | - | ws0",
    "halo_upsample_off": "0: tile 64x64 ks3 tapu1 buf1 epi0 split1 | 96x256 lds32768 | - | ws0",
    "split_cost_model": "0: tile 128x160 ks3 tapu1 buf1 epi2 split15 | 240x256 lds73728 | +reduce | ws19660800",
    "split_none_without_workspace": "0: tile 64x64 ks3 tapu1 buf1 epi0 split1 | 80x256 lds32768 | - | ws0",
    "split_forced": "0: tile 128x64 ks1 tapu0 buf1 epi2 split4 | 768x256 lds49152 | +reduce | ws25165824",
    "split_forced_no_workspace": "0: tile 128x64 ks1 tapu0 buf1 epi0 split1 | 192x256 lds49152 | - | ws25165824",
    "split_fitted_to_2": "0: tile 64x64 ks3 tapu1 buf1 epi2 split2 | 160x256 lds32768 | +reduce | ws10485760",
    "split_fitted_to_1": "0: tile 64x64 ks3 tapu1 buf1 epi0 split1 | 80x256 lds32768 | - | ws10485760",
    "split_forced_rowblock_shape": "0: tile 128x160 ks1 tapu0 buf1 epi2 split2 | 2048x256 lds73728 | +reduce | ws167772160",
    "split_fitted_to_1_rowblock": "1: rowblock kt10 fm2 flags0 split1 | 256x512 lds63744 | - | ws167772160",
    "split_key3": "0: tile 128x128 ks1 tapu0 buf1 epi2 split2 | 192x256 lds65536 | +reduce | ws12582912",
    "rb640_few_rows_workspace_splits": "0: tile 64x64 ks1 tapu0 buf1 epi2 split2 | 24x256 lds32768 | +reduce | ws393216",
    "rb640_few_rows": "1: rowblock kt20 fm2 flags0 split1 | 6x512 lds125184 | - | ws0",
    # (these three, and their conv_path_parent.json entries, as commit 82f8434 answered: with the key at its
    # default the plans are rowblock kt20 fm2 flags0, tile 64x64 and halo bn160 th16)
    "rb640_key7_off": "0: tile 64x64 ks1 tapu0 buf1 epi0 split1 | 40x256 lds32768 | - | ws0",
    "rb640_res_key20": "1: rowblock kt20 fm1 flags2 split1 | 40x512 lds149760 | - | ws0",
    "halo_bn128_key13": "3: halo bn128 th8 gn0 cs0 ph0 split1 | 20x256 lds80896 | - | ws0",
}
