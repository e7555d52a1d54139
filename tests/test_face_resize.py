"""Host side of the ingest face resize (ls_resize_faces_u8, ABI 14) and of the
ImageProcessor drop-in: exports, argument refusals that need no device, and the
options this build refuses.  The kernel itself is checked on the GPU in
tests/test_gpu_face_resize.py."""
import inspect

import pytest
import torch

from latentsync_amd import _lib

LS_OK, LS_ERR_INVALID = 0, 1
PTR = 16  # never dereferenced: validation fails first (tests/test_capi.py)


def test_library_exports_resize_and_abi_14():
    lib = _lib.load()
    assert "ls_resize_faces_u8" in _lib.EXPORTED and hasattr(lib, "ls_resize_faces_u8")
    assert lib.ls_abi_version() == 14 == _lib.ABI_VERSION


@pytest.mark.parametrize("args,what", [
    ((None, 1, 64, 64, 32, 32, PTR), "bad args"),          # null src
    ((PTR, 1, 64, 64, 32, 32, None), "bad args"),          # null dst
    ((PTR, -1, 64, 64, 32, 32, PTR), "bad args"),
    ((PTR, 1, 0, 64, 32, 32, PTR), "bad args"),
    ((PTR, 1, 64, -3, 32, 32, PTR), "bad args"),
    ((PTR, 1, 64, 64, 0, 32, PTR), "bad args"),
    ((PTR, 1, 64, 64, 32, -1, PTR), "bad args"),
    ((PTR, 1, 64, 225, 32, 32, PTR), "downscale factor above 7"),  # 7.03:1 in w: 17 taps
    ((PTR, 1, 257, 64, 32, 32, PTR), "downscale factor above 7"),  # 8.03:1 in h
])
def test_host_refusals(args, what):
    lib = _lib.load()
    src, N, ih, iw, oh, ow, dst = args
    assert lib.ls_resize_faces_u8(src, N, ih, iw, oh, ow, dst, None) == LS_ERR_INVALID
    msg = lib.ls_last_error().decode()
    assert "ls_resize_faces_u8" in msg and what in msg


def test_empty_batch_launches_nothing():
    # 7:1 is the largest accepted factor (16 taps); N = 0 returns before any launch
    assert _lib.load().ls_resize_faces_u8(PTR, 0, 224, 224, 32, 32, PTR, None) == LS_OK


def test_op_refuses_host_and_non_uint8_tensors():
    from latentsync_amd import ops
    with pytest.raises(ValueError):
        ops.resize_faces_u8(torch.zeros((1, 3, 8, 8), dtype=torch.uint8), 4, 4)  # not on the device
    with pytest.raises(ValueError):
        ops.resize_faces_u8(torch.zeros((1, 3, 8, 8)), 4, 4)
    with pytest.raises(ValueError):
        ops.resize_faces_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4, 4)


def test_image_processor_constructs_on_cpu():
    import latentsync_amd
    from latentsync_amd import ImageProcessor, image_processor, pipeline
    assert ImageProcessor is image_processor.ImageProcessor is latentsync_amd.ImageProcessor
    assert image_processor.load_fixed_mask is pipeline.load_fixed_mask
    ip = ImageProcessor()
    assert ip.resolution == 512 and ip.mask == "fix_mask" and ip.device == torch.device("cpu")
    ip = ImageProcessor(256, "fix_mask", "cpu", mask_image=pipeline.load_fixed_mask(256))
    assert ip.resolution == 256
    ip.close()
    with pytest.raises(AttributeError):
        latentsync_amd.NoSuchName


@pytest.mark.parametrize("mask", ["mouth", "face", "eye"])
def test_image_processor_refuses_landmark_masks(mask):
    from latentsync_amd import ImageProcessor
    with pytest.raises(NotImplementedError, match="landmark"):
        ImageProcessor(256, mask=mask)


def test_image_processor_refuses_affine_transform():
    from latentsync_amd import ImageProcessor
    ip = ImageProcessor(64)
    img = torch.zeros((2, 3, 128, 128), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="landmark"):
        ip.prepare_masks_and_masked_images(img, affine_transform=True)
    with pytest.raises(NotImplementedError, match="landmark"):
        ip.preprocess_fixed_mask_image(img[0], affine_transform=True)
    with pytest.raises(NotImplementedError, match="landmark"):
        ip.affine_transform(img[0])


def test_engine_load_rejects_wrong_face_size():
    """WindowEngine.load checks the faces against the buffer it stages them in -- the
    R-sized one, or the S-sized source of an engine built with face_resolution=S --
    before it touches anything else, so the check is reachable without a device."""
    from latentsync_amd.pipeline import WindowEngine
    eng = WindowEngine.__new__(WindowEngine)
    eng.FT, eng.h = 8, 8
    eng.faces = torch.zeros((8, 3, 64, 64), dtype=torch.uint8)
    eng.faces_src = None
    for bad in [(8, 3, 128, 128), (4, 3, 64, 64), (8, 1, 64, 64), (1, 3, 64, 64)]:
        with pytest.raises(ValueError):
            eng.load(torch.zeros(bad, dtype=torch.uint8), None, None, None, None, None)
    eng.faces_src = torch.zeros((8, 3, 128, 128), dtype=torch.uint8)
    for bad in [(8, 3, 64, 64), (8, 3, 128, 64), (16, 3, 128, 128)]:
        with pytest.raises(ValueError):
            eng.load(torch.zeros(bad, dtype=torch.uint8), None, None, None, None, None)


def test_pipeline_signatures_take_the_face_resolution():
    from latentsync_amd.pipeline import LipsyncPipeline, WindowEngine
    assert inspect.signature(WindowEngine.__init__).parameters["face_resolution"].default is None
    assert inspect.signature(LipsyncPipeline.engine).parameters["face_resolution"].default is None
    assert inspect.signature(LipsyncPipeline.run_windows).parameters["height"].default is None
