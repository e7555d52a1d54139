"""ImageProcessor -- drop-in for the part of latentsync/utils/image_processor.py that
the inference path uses (``fix_mask``: resize, normalise, apply the fixed mask).

The resize is the HIP kernel behind ``ops.resize_faces_u8`` (torchvision's
``transforms.Resize((R, R), BILINEAR, antialias=True)`` on uint8, image_processor.py:42-44);
normalising and masking are plain torch on the device.  ``LipsyncPipeline`` does not
go through this class -- its window engine fuses the same steps into the captured
encode graph (``ls_resize_faces_u8`` + ``ls_prep_pixels``); the class is for callers
that used the reference's ``ImageProcessor`` directly.

Not carried: landmark detection (mediapipe / face_alignment), so ``affine_transform=True``
and the "mouth" / "face" / "eye" masks raise NotImplementedError; the "half" mask is
not implemented either.
"""
import numpy as np
import torch

from . import ops
from .pipeline import load_fixed_mask  # noqa: F401  (re-exported, as the reference module does)

__all__ = ["ImageProcessor", "load_fixed_mask"]

_LANDMARK_MASKS = ("mouth", "face", "eye")


class ImageProcessor:
    """ImageProcessor(resolution, mask, device, mask_image) (image_processor.py:39-68).

    ``device``: the reference uses it to pick the landmark detector only; here it is
    where the results live.  The resize is a HIP kernel, so "cpu" (the reference's
    default) means the current HIP device.  ``mask_image``: a keep-mask (R,R) or
    (C,R,R), e.g. ``load_fixed_mask(R)``; loaded on first use when None."""

    def __init__(self, resolution=512, mask="fix_mask", device="cpu", mask_image=None):
        if mask in _LANDMARK_MASKS:
            raise NotImplementedError(f"mask={mask!r} needs the mediapipe FaceMesh landmark model, which this build "
                                      "does not carry (image_processor.py:48-49, 84-107)")
        if mask != "fix_mask":
            raise NotImplementedError(f"mask={mask!r}: only 'fix_mask' is on the inference path")
        self.resolution = int(resolution)
        self.mask = mask
        self.device = torch.device(device)
        self.face_mesh = None
        self.fa = None
        self._mask_image = mask_image
        self._lut = None

    # -- helpers -----------------------------------------------------------------
    def _dev(self):
        if self.device.type == "cuda":
            return self.device
        return torch.device("cuda", torch.cuda.current_device())

    @property
    def mask_image(self):
        """The keep-mask (1,R,R) fp32 on the device (the reference holds three equal
        channels and hands out channel 0, :152)."""
        m = self._mask_image
        dev = self._dev()
        if m is None:
            m = load_fixed_mask(self.resolution, device=dev)
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(m)
        if m.dim() == 3:
            m = m[0]
        R = self.resolution
        if tuple(m.shape) != (R, R):
            raise ValueError(f"mask_image {tuple(m.shape)}: ({R},{R}) or (C,{R},{R}) expected")
        m = m.to(dev, torch.float32).unsqueeze(0)
        self._mask_image = m
        return m

    def _normalize(self, u8):
        """transforms.Normalize([0.5], [0.5])(x / 255.0) of uint8 values, fp32.  Through a
        256-entry table computed on the host: a device division by the scalar 255 may be
        a multiplication by its reciprocal, an ulp away from the reference's x / 255.0."""
        if self._lut is None or self._lut.device != u8.device:
            self._lut = ((torch.arange(256, dtype=torch.float32) / 255.0 - 0.5) / 0.5).to(u8.device)
        return self._lut[u8.long()]

    @staticmethod
    def _chw(images):
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(images)
        if images.dim() == 4 and images.shape[3] == 3:  # "f h w c -> f c h w" (:157-158, :170-171)
            images = images.permute(0, 3, 1, 2)
        if images.dtype != torch.uint8 or images.dim() < 3 or images.shape[-3] != 3:
            raise ValueError(f"uint8 (...,3,H,W) or (F,H,W,3) images expected, got {images.dtype} "
                             f"{tuple(images.shape)}")
        return images

    # -- the reference's methods ---------------------------------------------------
    def resize(self, images):
        """self.resize (:42-44): uint8 (...,3,H,W) or (F,H,W,3) -> uint8 (...,3,R,R) on the
        device.  Images already at the resolution are returned as they are."""
        images = self._chw(images).to(self._dev())
        R = self.resolution
        if tuple(images.shape[-2:]) == (R, R):
            return images
        lead = tuple(images.shape[:-3])
        flat = images.reshape((-1,) + tuple(images.shape[-3:])).contiguous()
        return ops.resize_faces_u8(flat, R, R).reshape(lead + (3, R, R))

    def process_images(self, images):
        """:167-174 -> (F,3,R,R) fp32 in [-1,1]."""
        return self._normalize(self.resize(images))

    def affine_transform(self, image, allow_multi_faces=True):
        raise NotImplementedError("affine_transform needs the face_alignment / mediapipe landmark detector, which "
                                  "this build does not carry (image_processor.py:118-143); align the faces "
                                  "beforehand (latentsync_amd.align, data.pth) and pass them with "
                                  "affine_transform=False")

    def preprocess_fixed_mask_image(self, image, affine_transform=False):
        """:145-152 for one (3,H,W) image (or a batch): pixel_values, masked_pixel_values,
        mask (1,R,R)."""
        if affine_transform:
            self.affine_transform(image)
        pixel_values = self._normalize(self.resize(image))
        mask = self.mask_image
        return pixel_values, pixel_values * mask, mask

    def prepare_masks_and_masked_images(self, images, affine_transform=False):
        """:154-165 -> (pixel_values (F,3,R,R), masked_pixel_values (F,3,R,R), masks (F,1,R,R)),
        fp32 on the device; the whole batch is one resize launch."""
        if affine_transform:
            self.affine_transform(images)
        images = self._chw(images)
        if images.dim() != 4:
            raise ValueError(f"(F,3,H,W) or (F,H,W,3) images expected, got {tuple(images.shape)}")
        pixel_values, masked, mask = self.preprocess_fixed_mask_image(images)
        return pixel_values, masked, mask.unsqueeze(0).expand(images.shape[0], -1, -1, -1).contiguous()

    def close(self):
        pass
