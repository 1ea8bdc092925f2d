"""Mirror of the one function of the reference's ``model/dataset/util.py`` that has arithmetic in it: compute_distance_transform
(util.py:12-18), there two cv2.distanceTransform(..., DIST_L2, DIST_MASK_PRECISE) calls per sample on the host, here one call of
the exact Euclidean distance transform on the GPU (csrc/edt.hip, include/a3d_edt.h).  The loaders of that file stay the reference's own;
this module is not part of the overlay (overlay.MODULES): a maintainer calls it where the batch has reached the device
(INTEGRATION.md)."""
import torch

from ... import ops


def compute_distance_transform(mask):
    """mask [B,C,H,W] on the GPU, channel 0 is used -> float32 [B,2,H,W] on the mask's device, the reference's order: channel 0 is the
    distance INSIDE the mask to the background (the transform of np.uint8(m)), channel 1 the distance OUTSIDE to the mask (the
    transform of np.uint8(1 - m)), in pixels.  np.uint8 truncates, so on a mask with values in [0,1] a pixel is inside where m >= 1
    and outside where m <= 0; a NaN is neither (a zero pixel of both channels).  A channel whose image has no zero pixel at all (an
    empty or a full mask) is H * H + W * W under the root everywhere: finite, where cv2 and scipy give arbitrary or huge values.
    No gradient: the reference never differentiates mask_dt."""
    if not torch.is_tensor(mask) or mask.dim() != 4:
        raise ValueError(f"compute_distance_transform: expected a mask [B,C,H,W], got {list(getattr(mask, 'shape', [])) or type(mask)}")
    return ops.distance_transform(mask[:, 0].float(), thresholds=(1.0, 0.0))
