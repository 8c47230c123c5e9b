"""Tensor transforms (reference: compressai/transforms): BT.709 colour conversion and 4:2:0 <-> 4:4:4 resampling,
as functions in ``functional`` and as callable classes here."""
from . import functional
from .functional import rgb2ycbcr, ycbcr2rgb, yuv_420_to_444, yuv_444_to_420

__all__ = ["RGB2YCbCr", "YCbCr2RGB", "YUV444To420", "YUV420To444", "functional"]


class RGB2YCbCr:
    """RGB -> YCbCr of a floating (3xHxW) or (Nx3xHxW) tensor in [0, 1]."""

    def __call__(self, rgb):
        return rgb2ycbcr(rgb)

    def __repr__(self):
        return f"{self.__class__.__name__}()"


class YCbCr2RGB:
    """YCbCr -> RGB of a floating (3xHxW) or (Nx3xHxW) tensor in [0, 1]."""

    def __call__(self, ycbcr):
        return ycbcr2rgb(ycbcr)

    def __repr__(self):
        return f"{self.__class__.__name__}()"


class YUV444To420:
    """4:4:4 (one (Nx3xHxW) tensor or three (Nx1xHxW)) -> the three planes of 4:2:0; ``mode``: ``'avg_pool'``."""

    def __init__(self, mode: str = "avg_pool"):
        self.mode = str(mode)

    def __call__(self, yuv):
        return yuv_444_to_420(yuv, mode=self.mode)

    def __repr__(self):
        return f"{self.__class__.__name__}()"


class YUV420To444:
    """Three 4:2:0 planes (Nx1xHxW) -> 4:4:4; ``mode``: ``'bilinear'`` | ``'bicubic'`` | ``'nearest'``; one
    (Nx3xHxW) tensor, or the three planes with ``return_tuple``."""

    def __init__(self, mode: str = "bilinear", return_tuple: bool = False):
        self.mode = str(mode)
        self.return_tuple = bool(return_tuple)

    def __call__(self, yuv):
        return yuv_420_to_444(yuv, mode=self.mode, return_tuple=self.return_tuple)

    def __repr__(self):
        return f"{self.__class__.__name__}(return_tuple={self.return_tuple})"
