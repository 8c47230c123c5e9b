"""Colour-space and chroma-sampling transforms on tensors (reference: compressai/transforms/functional.py).

The general tensor API: plain torch, differentiable, any device and floating dtype.  The raw-video evaluation does
not go through these; its per-frame path is fused in csrc/video.hip (``compressai.utils.video.frames``).
"""
from typing import Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor

__all__ = ["YCBCR_WEIGHTS", "rgb2ycbcr", "ycbcr2rgb", "yuv_444_to_420", "yuv_420_to_444"]

# (K_r, K_g, K_b), K_g = 1 - K_r - K_b
YCBCR_WEIGHTS = {"ITU-R_BT.709": (0.2126, 0.7152, 0.0722)}


def _check_input_tensor(tensor: Tensor) -> None:
    ok = (isinstance(tensor, Tensor) and tensor.is_floating_point() and tensor.dim() in (3, 4)
          and tensor.size(-3) == 3)
    if not ok:
        raise ValueError("Expected a 3D or 4D tensor with shape (Nx3xHxW) or (3xHxW) as input")


def rgb2ycbcr(rgb: Tensor) -> Tensor:
    """RGB -> YCbCr (ITU-R BT.709) of a floating (3xHxW) or (Nx3xHxW) tensor."""
    _check_input_tensor(rgb)
    Kr, Kg, Kb = YCBCR_WEIGHTS["ITU-R_BT.709"]
    r, g, b = rgb.unbind(-3)
    y = Kr * r + Kg * g + Kb * b
    cb = 0.5 * (b - y) / (1 - Kb) + 0.5
    cr = 0.5 * (r - y) / (1 - Kr) + 0.5
    return torch.stack((y, cb, cr), dim=-3)


def ycbcr2rgb(ycbcr: Tensor) -> Tensor:
    """YCbCr -> RGB (ITU-R BT.709) of a floating (3xHxW) or (Nx3xHxW) tensor."""
    _check_input_tensor(ycbcr)
    Kr, Kg, Kb = YCBCR_WEIGHTS["ITU-R_BT.709"]
    y, cb, cr = ycbcr.unbind(-3)
    r = y + (2 - 2 * Kr) * (cr - 0.5)
    b = y + (2 - 2 * Kb) * (cb - 0.5)
    g = (y - Kr * r - Kb * b) / Kg
    return torch.stack((r, g, b), dim=-3)


def yuv_444_to_420(yuv: Union[Tensor, Tuple[Tensor, Tensor, Tensor]],
                   mode: str = "avg_pool") -> Tuple[Tensor, Tensor, Tensor]:
    """4:4:4 -> 4:2:0.  ``yuv`` is a (Nx3xHxW) tensor or three (Nx1xHxW) tensors; the chroma is averaged 2 x 2."""
    if mode not in ("avg_pool",):
        raise ValueError(f'Invalid downsampling mode "{mode}".')
    y, u, v = yuv.chunk(3, 1) if isinstance(yuv, Tensor) else yuv
    return y, F.avg_pool2d(u, kernel_size=2, stride=2), F.avg_pool2d(v, kernel_size=2, stride=2)


def yuv_420_to_444(yuv: Tuple[Tensor, Tensor, Tensor], mode: str = "bilinear",
                   return_tuple: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor, Tensor]]:
    """4:2:0 -> 4:4:4: the chroma of three (Nx1xHxW) tensors upsampled x2 (``'bilinear'`` | ``'bicubic'`` |
    ``'nearest'``, align_corners=False); one (Nx3xHxW) tensor, or the three planes with ``return_tuple``."""
    if len(yuv) != 3 or any(not isinstance(c, Tensor) for c in yuv):
        raise ValueError("Expected a tuple of 3 torch tensors")
    if mode not in ("bilinear", "bicubic", "nearest"):
        raise ValueError(f'Invalid upsampling mode "{mode}".')
    kwargs = {} if mode == "nearest" else {"align_corners": False}
    y, u, v = yuv
    u = F.interpolate(u, scale_factor=2, mode=mode, **kwargs)
    v = F.interpolate(v, scale_factor=2, mode=mode, **kwargs)
    return (y, u, v) if return_tuple else torch.cat((y, u, v), dim=1)
