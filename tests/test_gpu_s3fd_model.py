"""S3FDNet and S3FD on the device.

Network golden: two 304 x 432 frames at scale 0.25 against the reference S3FDNet's fp32 stages
(tests/golden/s3fd_net.npz, tests/make_s3fd_golden.py): every ReLU output, the three L2Norm
outputs and the six raw head maps.  Tolerance, per tensor, as max |got - golden| / RMS(golden):
the error of the bf16-rounding restatement (s3fd_ref.forward(bf16=True), CPU) against the same
golden is REF_ERR (tests/test_s3fd_host.py measures and pins it on the CPU); the device rounds
at the same points and only its accumulation order differs, so it is allowed 2 x that figure --
the rule of tests/test_gpu_synceval_model.py.

End to end: S3FD.detect must equal the float64 post-processing restatement applied to the
device's OWN head maps, box for box; if one of the margins that make that comparison exact is
violated on those maps, the test says which and fails instead of comparing."""
import numpy as np
import pytest
import torch

import s3fd_ref as R
from conftest import golden
from latentsync_amd import ops, s3fd
from test_s3fd_host import ref_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEVICE_FACTOR = 2.0
E2E_CONF_TH = 0.6   # seeded weights give scores about 0.5: a threshold that lets some boxes through
E2E_SEED = 45   # chosen so that the four margins hold on the device's own head maps (smallest 2.6e-4)


@pytest.fixture(scope="module")
def net():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return s3fd.S3FDNet().load_state_dict(R.case_weights()).to(DEV).eval()


def test_network_matches_golden(gpu, net):
    g = golden("s3fd_net.npz")
    frames = R.case_frames().to(DEV)
    x = ops.s3fd_prep(frames, R.WORK_SCALE)
    assert tuple(x.shape) == (2, 76, 108, 8)
    assert tuple(net.priors(76, 108).shape) == (697, 4)
    assert np.array_equal(net.priors(76, 108).cpu().numpy().view(np.uint32), g["priors"].view(np.uint32))
    taps = {}
    heads = net.head_maps(x, taps)
    torch.cuda.synchronize()
    nchw = lambda ts: [t.permute(0, 3, 1, 2).float() for t in ts]
    errs = R.golden_errors(g, nchw(taps["relu"]), nchw(taps["l2norm"]), [h.float() for h in heads])
    fails = []
    for label, e in errs.items():
        allowed = DEVICE_FACTOR * ref_err(label)
        print(f"{label}: err / rms {e:.4g} (restatement {ref_err(label):.4g}, allowed {allowed:.4g})")
        if not (np.isfinite(e) and e <= allowed):
            fails.append((label, e, allowed))
    assert not fails, fails
    # each frame alone equals the frame in the batch, bit for bit
    for f in range(2):
        t1 = {}
        h1 = net.head_maps(ops.s3fd_prep(frames[f:f + 1], R.WORK_SCALE), t1)
        torch.cuda.synchronize()
        for kind in ("relu", "l2norm"):
            for a, b in zip(t1[kind], taps[kind]):
                assert torch.equal(a[0], b[f]), (kind, f)
        for a, b in zip(h1, heads):
            assert torch.equal(a[0], b[f]), ("head", f)


def test_forward_keeps_the_reference_interface(gpu, net):
    x = R.prep(R.case_frames(), R.WORK_SCALE)
    out = net(x.to(DEV))
    assert tuple(out.shape) == (2, 2, 750, 5) and out.dtype == torch.float32
    assert not bool(out[:, 0].any())
    det, counts = net.detections(ops.s3fd_prep(R.case_frames().to(DEV), R.WORK_SCALE))
    assert torch.equal(out[:, 1], det)
    k = int(counts[0])
    assert 0 < k <= 750 and bool((det[0, :k, 0] > 0.05).all()) and not bool(det[0, k:].any())
    assert bool((det[0, :k - 1, 0] >= det[0, 1:k, 0]).all())
    with pytest.raises(ValueError, match="too small"):
        net.head_maps(torch.zeros((1, 16, 16, 8), dtype=torch.bfloat16, device=DEV))


def test_detect_equals_postprocessing_of_its_own_head_maps(gpu, net):
    frames = R.case_frames(2, R.WORK_HW, seed=E2E_SEED)
    H, W = R.WORK_HW
    det = s3fd.S3FD.__new__(s3fd.S3FD)
    det.device, det.net = net.device, net
    boxes = det.detect(frames.to(DEV), conf_th=E2E_CONF_TH, scale=R.WORK_SCALE)
    heads = [h.cpu() for h in net.head_maps(ops.s3fd_prep(frames.to(DEV), R.WORK_SCALE))]
    priors = net.priors(76, 108).cpu().numpy()
    assert len(boxes) == 2
    total = 0
    for f in range(2):
        d = R.detect_ref(heads, priors, frame=f)
        rows = np.zeros((750, 5), dtype=np.float32)
        k = d["idx"].size
        rows[:k, 0], rows[:k, 1:] = d["scores"], d["boxes"]
        n = R.nms_ref(rows, E2E_CONF_TH, W, H)
        for what, margin, need in (("a score within 1e-4 of 0.05", d["score_margin"], R.MARGIN_SCORE),
                                   ("an IoU of Detect's NMS within 1e-4 of 0.3", d["iou_margin"], R.MARGIN_IOU),
                                   ("a score within 1e-4 of conf_th", n["score_margin"], R.MARGIN_SCORE),
                                   ("an IoU of nms_ within 1e-4 of 0.1", n["iou_margin"], R.MARGIN_IOU)):
            assert margin >= need, f"frame {f}: the device's own head maps put {what} (margin {margin:.3g}): " \
                                   "the comparison would not be exact; pick another E2E_SEED"
        assert boxes[f].shape == n["boxes"].shape, (f, boxes[f].shape, n["boxes"].shape)
        np.testing.assert_allclose(boxes[f][:, :4], n["boxes"][:, :4], rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(boxes[f][:, 4], n["boxes"][:, 4], rtol=0, atol=1e-6)
        total += boxes[f].shape[0]
        one = det.detect_faces(frames[f].numpy(), conf_th=E2E_CONF_TH, scales=[R.WORK_SCALE])
        assert one.dtype == np.float64 and np.array_equal(one, boxes[f]), f"detect_faces differs from detect on frame {f}"
    assert total > 0, "no box above the threshold: the test compares nothing"
