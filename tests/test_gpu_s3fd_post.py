"""ls_s3fd_detect and ls_nms_boxes on identical fp32 inputs against what the reference's own
S3FDNet.forward tail, Detect and S3FD.detect_faces produced on them (tests/golden/s3fd_post.npz,
tests/make_s3fd_golden.py).  The discrete stages cannot be judged through a bf16 network, so
they get the seeded synthetic head maps of tests/s3fd_ref.py.  The generator searched seeds
until no score lies within 1e-4 of a threshold and no compared IoU within 1e-4 of its threshold
(tests/test_s3fd_host.py re-checks the margins on the CPU); under those margins the device must
return exactly the reference's kept boxes in the reference's order, scores to 1e-6 and
coordinates to 1e-5 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity as P
import s3fd_ref as R
from conftest import golden
from latentsync_amd import _lib, ops
from test_s3fd_host import post_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", ("work", "big", "none"))
def test_detect_and_nms_exact(gpu, name):
    """work: 697 priors; big: 5373 priors, all of them candidates, of which exactly the 5000
    highest may enter the NMS (three cells hold only lower ones and must yield no box); none: no
    candidate at all.  A second frame with the maps of another seed rides along: frames must
    not see each other."""
    g = golden("s3fd_post.npz")
    hw = tuple(int(v) for v in g[f"{name}_hw"])
    heads, priors = post_case(name)
    other = R.synthetic_heads(7, [tuple(m.shape[1:3]) for m in heads], n=1)
    maps = [torch.cat([o, m], 0).to(DEV).contiguous() for m, o in zip(heads, other)]
    snaps = [P.snapshot(m) for m in maps]
    out, counts, idx = ops.s3fd_detect(maps, torch.from_numpy(priors).to(DEV), want_idx=True)
    torch.cuda.synchronize()
    for m, s in zip(maps, snaps):
        P.assert_unchanged(m, s, "head map")
    rows, want_idx = g[f"{name}_rows"], g[f"{name}_idx"]
    k = int(g[f"{name}_count"])
    assert int(counts[1]) == k == rows.shape[0]
    got = out[1].cpu().numpy()
    assert np.array_equal(idx[1, :k].cpu().numpy(), want_idx), "kept priors or their order differ"
    assert bool((idx[1, k:] == -1).all()) and not got[k:].any(), "rows after the count must be zero"
    np.testing.assert_allclose(got[:k, 0], rows[:, 0], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:k, 1:], rows[:, 1:], rtol=1e-5, atol=1e-7)
    # the frame that rode along, against the float64 restatement
    d0 = R.detect_ref(other, priors)
    if d0["score_margin"] >= R.MARGIN_SCORE and d0["iou_margin"] >= R.MARGIN_IOU:  # seed 7 is not a searched one
        assert np.array_equal(idx[0, :int(counts[0])].cpu().numpy(), d0["idx"])

    # the rest of detect_faces
    final, final_idx = g[f"{name}_final"], g[f"{name}_final_idx"]
    res, cnt, keep = ops.nms_boxes(out, float(g["conf_th"]), hw[1], hw[0], 0.1, want_idx=True)
    torch.cuda.synchronize()
    kf = final.shape[0]
    assert int(cnt[1]) == kf
    assert np.array_equal(keep[1, :kf].cpu().numpy(), final_idx), "nms_ keep order differs"
    got = res[1].cpu().numpy()
    assert not got[kf:].any() and bool((keep[1, kf:] == -1).all())
    np.testing.assert_allclose(got[:kf, :4], final[:, :4], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[:kf, 4], final[:, 4], rtol=0, atol=1e-6)
    if name == "big":
        assert int(g["big_n_cand"]) == priors.shape[0] > 5000 and k < 750
    if name == "none":
        assert k == 0 and kf == 0


def test_detect_fills_750_rows_and_stops(gpu):
    """More than 750 survivors: small boxes that never overlap.  The first 750 by score come out."""
    h, w = 96, 128
    from latentsync_amd import s3fd
    sizes = s3fd.feature_map_sizes(h, w)
    priors = s3fd.prior_boxes(h, w, sizes)
    heads = R.synthetic_heads(11, sizes, n=1, lo=0.06, hi=0.999, loc_scale=0.0)
    for m in heads:
        m[..., 2:4] = -12.0  # exp(-2.4): boxes a tenth of their prior
    d = R.detect_ref(heads, priors)
    assert d["idx"].size == 750 and d["n_cand"] == priors.shape[0] == 1025 and d["iou_margin"] >= R.MARGIN_IOU
    out, counts, idx = ops.s3fd_detect([m.to(DEV) for m in heads], torch.from_numpy(priors).to(DEV), want_idx=True)
    torch.cuda.synchronize()
    assert int(counts[0]) == 750
    assert np.array_equal(idx[0].cpu().numpy(), d["idx"])
    np.testing.assert_allclose(out[0, :, 0].cpu().numpy(), d["scores"], rtol=0, atol=1e-6)


def test_concatenated_scales_share_one_nms(gpu):
    """Two per-scale lists of a frame one after the other, as the reference stacks bboxes."""
    rng = np.random.RandomState(3)

    def rows(k, x0):
        r = np.zeros((750, 5), dtype=np.float32)
        r[:k, 0] = np.sort(rng.uniform(0.91, 0.999, k))[::-1]
        r[:k, 1] = x0 + 0.11 * np.arange(k)
        r[:k, 2] = 0.2
        r[:k, 3] = r[:k, 1] + 0.1
        r[:k, 4] = 0.3
        return r

    det = np.concatenate([rows(4, 0.05), rows(3, 0.06)])[None]  # the second list overlaps the first heavily
    ref = R.nms_ref(det[0], 0.9, 640, 480)
    assert ref["iou_margin"] >= R.MARGIN_IOU and ref["score_margin"] >= R.MARGIN_SCORE and 0 < ref["idx"].size < 7
    res, cnt, keep = ops.nms_boxes(torch.from_numpy(det).to(DEV), 0.9, 640, 480, 0.1, want_idx=True)
    torch.cuda.synchronize()
    k = ref["idx"].size
    assert int(cnt[0]) == k and np.array_equal(keep[0, :k].cpu().numpy(), ref["idx"])
    np.testing.assert_allclose(res[0, :k].cpu().numpy(), ref["boxes"], rtol=1e-5, atol=1e-5)


def test_detect_and_nms_invalid_arguments_launch_nothing(gpu):
    lib = _lib.load()
    from latentsync_amd import s3fd
    sizes = s3fd.feature_map_sizes(76, 108)
    heads = [m.to(DEV) for m in R.synthetic_heads(1, sizes, n=1)]
    priors = torch.from_numpy(s3fd.prior_boxes(76, 108, sizes)).to(DEV)
    go = P.guarded((750, 5), dtype=torch.float32, device=DEV)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    nbytes = lib.ls_s3fd_detect_workspace_bytes(1, 697)
    assert nbytes > 0 and lib.ls_s3fd_detect_workspace_bytes(1, 65537) == 0 and lib.ls_s3fd_detect_workspace_bytes(0, 697) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    hw = [v for hw_ in sizes for v in hw_]

    def call(maps=heads, hw=hw, n=1, pr=priors.data_ptr(), P_=697, out=go.view.data_ptr(), c=cnt.data_ptr(),
             w=ws.data_ptr(), wb=nbytes):
        ptrs = (C.c_void_p * 6)(*[None if m is None else m.data_ptr() for m in maps])
        return lib.ls_s3fd_detect(ptrs, (C.c_int32 * 12)(*hw), n, pr, P_, out, c, None, w, wb, s)

    assert call(maps=[None] + heads[1:]) == 1
    assert call(n=0) == 1 and call(pr=None) == 1 and call(out=None) == 1 and call(c=None) == 1
    assert call(P_=696) == 1 and call(P_=65537) == 1 and call(P_=0) == 1
    assert call(hw=[0] + hw[1:]) == 1 and call(hw=[20] + hw[1:]) == 1
    assert call(pr=priors.data_ptr() + 4) == 1
    assert call(w=None) == 3 and call(wb=nbytes - 1) == 3  # LS_ERR_WORKSPACE
    torch.cuda.synchronize()
    P.assert_guard_intact(go, "refused ls_s3fd_detect")
    assert bool(torch.isnan(go.view).all()) and int(cnt[0]) == -7
    assert call() == 0
    torch.cuda.synchronize()
    P.assert_guard_intact(go, "accepted ls_s3fd_detect")
    with pytest.raises(ValueError, match="smaller scale"):
        big = [torch.zeros((1, 260, 260, 8), device=DEV)] + [torch.zeros((1, 1, 1, 6), device=DEV)] * 5
        ops.s3fd_detect(big, torch.zeros((260 * 260 + 5, 4), device=DEV))

    det = torch.zeros((1, 750, 5), device=DEV)
    g2 = P.guarded((750, 5), dtype=torch.float32, device=DEV)

    def nms(d=det.data_ptr(), n=1, R_=750, th=0.9, fw=640.0, fh=480.0, t=0.1, out=g2.view.data_ptr(), c=cnt.data_ptr()):
        return lib.ls_nms_boxes(d, n, R_, th, fw, fh, t, out, c, None, s)

    for kw in (dict(d=None), dict(out=None), dict(c=None), dict(n=0), dict(R_=0), dict(R_=4097), dict(th=-0.1),
               dict(th=float("nan")), dict(t=-1.0), dict(fw=0.0), dict(fh=-2.0)):
        assert nms(**kw) == 1, kw
    torch.cuda.synchronize()
    P.assert_guard_intact(g2, "refused ls_nms_boxes")
    assert bool(torch.isnan(g2.view).all())
    assert nms() == 0
    torch.cuda.synchronize()
    assert int(cnt[0]) == 0 and not g2.view.cpu().numpy().any()
    P.assert_guard_intact(g2, "accepted ls_nms_boxes")
