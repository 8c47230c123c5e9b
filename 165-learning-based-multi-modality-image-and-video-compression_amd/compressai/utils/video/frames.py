"""The per-frame path around the video codec when it is evaluated on raw YUV 4:2:0.

Into the model: ``yuv420_to_rgb`` turns the integer planes of one frame into the zero-padded fp32 RGB model input
and the RGB levels ``org_q`` the metrics compare against.  Out of the model: ``frame_metrics`` turns the
reconstruction into PSNR-Y/U/V/YUV, MSE / PSNR-RGB and MS-SSIM-RGB, all as 0-dim device tensors -- nothing here
reads back to the host, the driver does that once per sequence.  Out of the decoder: ``rgb_to_yuv420`` turns the
reconstruction into the integer 4:2:0 frame, with the levels the metrics measure, as one buffer in file order, and
``write_frame`` appends it to a raw file (utils/codec_rgbt.py).

On GPU tensors each direction is one launch of csrc/video.hip (``_ops.yuv420_to_rgb`` / ``_ops.video_frame_sse`` /
``_ops.rgb_to_yuv420``) plus the MS-SSIM op; the squared level differences are integers and are summed as integers, so the sums do not
depend on any order.  On CPU tensors the ``*_torch`` bodies below spell out the same formulas in fp32 with torch
ops: the composition the reference's driver runs (true division, ``interpolate``, ``cat``, ``ycbcr2rgb``, ``pad``
/ crop, ``rgb2ycbcr``, two ``avg_pool2d``, clamp-round per plane).  They also run on GPU tensors, which is what
tools/video_eval_bench.py times the kernels against.
"""
import math
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ...transforms.functional import rgb2ycbcr, ycbcr2rgb, yuv_420_to_444, yuv_444_to_420
from ..metrics import ms_ssim

__all__ = ["to_planes", "pad_geometry", "yuv420_to_rgb", "frame_sse", "frame_metrics", "yuv420_to_rgb_torch",
           "frame_sse_torch", "rgb_to_yuv420", "rgb_to_yuv420_torch", "write_frame"]

BITDEPTHS = (8, 10, 12, 14, 16)
MODES = ("nearest", "bilinear", "bicubic")
MSSSIM_MIN_SIDE = 160       # the 5-scale MS-SSIM needs sides above (11 - 1) * 2^4


def to_planes(planes, device=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(y, u, v) integer tensors on ``device``.  A structured numpy record with fields y, u, v (what a
    ``RawVideoSequence`` yields) is uploaded as the integers it holds, in one copy of the whole frame; a tuple of
    tensors is moved if a device is given."""
    if isinstance(planes, (tuple, list)):
        if len(planes) != 3 or any(not isinstance(p, torch.Tensor) for p in planes):
            raise ValueError("expected the three planes (y, u, v) as tensors")
        if any(p.is_floating_point() or p.is_complex() or p.dtype == torch.bool for p in planes):
            raise ValueError("the planes must be integer tensors")
        return tuple(p if device is None else p.to(device) for p in planes)
    rec = np.asarray(planes)
    if rec.dtype.names != ("y", "u", "v"):
        raise ValueError("expected a tuple of three tensors or a numpy record with fields y, u, v")
    kind = rec.dtype["y"].base
    if kind not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise ValueError(f"unsupported sample type {kind}")
    if rec.ndim != 0:
        raise ValueError(f"expected one frame, got an array of shape {rec.shape}")
    buf = torch.from_numpy(np.array(rec).reshape(1).view(np.uint8))      # one host copy out of the file mapping
    if device is not None:
        buf = buf.to(device)
    out, at = [], 0
    for name in ("y", "u", "v"):
        shape = rec.dtype[name].shape
        n = int(np.prod(shape)) * kind.itemsize
        part = buf[at:at + n]
        out.append((part if kind.itemsize == 1 else part.view(torch.int16)).view(shape))
        at += n
    return tuple(out)


def _levels(t: torch.Tensor) -> torch.Tensor:
    """The samples as fp32 (16-bit containers hold unsigned words whatever the tensor's dtype says)."""
    if t.dtype == torch.uint16:
        t = t.view(torch.int16)
    if t.dtype == torch.int16:
        return (t.to(torch.int32) & 0xFFFF).float()
    return t.float()


def _container(t: torch.Tensor, bitdepth: int) -> torch.Tensor:
    """The plane in the container the kernels read: uint8 at 8 bits, 16-bit words above."""
    if bitdepth == 8:
        return (t if t.dtype == torch.uint8 else t.to(torch.uint8)).contiguous()
    if t.dtype in (torch.int16, torch.uint16):
        return t.contiguous()
    return t.to(torch.int16).contiguous()       # keeps the low 16 bits


def _check(planes, bitdepth: int):
    if bitdepth not in BITDEPTHS:
        raise ValueError(f"bit depth {bitdepth} not in {BITDEPTHS}")
    y, u, v = planes
    if y.dim() != 2:
        raise ValueError(f"the luma plane must be [H, W], got {tuple(y.shape)}")
    H, W = y.shape
    if H % 2 or W % 2 or H < 2 or W < 2:
        raise ValueError(f"4:2:0 needs even H and W, got {H} x {W}")
    for name, c in (("u", u), ("v", v)):
        if tuple(c.shape) != (H // 2, W // 2):
            raise ValueError(f"plane {name} must be [{H // 2}, {W // 2}], got {tuple(c.shape)}")
    return H, W


def pad_geometry(H: int, W: int, pad_to: int = 128):
    """(Hp, Wp, (left, right, top, bottom)): centred padding to multiples of ``pad_to``, the extra pixel of an odd
    difference on the right / bottom."""
    if pad_to < 1:
        raise ValueError(f"pad_to must be positive, got {pad_to}")
    Hp, Wp = (H + pad_to - 1) // pad_to * pad_to, (W + pad_to - 1) // pad_to * pad_to
    left, top = (Wp - W) // 2, (Hp - H) // 2
    return Hp, Wp, (left, Wp - W - left, top, Hp - H - top)


# ---------------------------------------------------------------------------------------------------------
# torch bodies (fp32; CPU tensors, and the baseline the kernels are timed against)
# ---------------------------------------------------------------------------------------------------------
def yuv420_to_rgb_torch(planes, bitdepth: int, mode: str, padding):
    max_val = 2 ** bitdepth - 1
    yuv = tuple((_levels(p) / float(max_val))[None, None] for p in planes)
    rgb = ycbcr2rgb(yuv_420_to_444(yuv, mode=mode))
    org_q = (rgb[0] * max_val).clamp(0, max_val).round()
    return F.pad(rgb, padding, mode="constant", value=0), org_q


def frame_sse_torch(planes, org_q, x_rec, padding, bitdepth: int):
    max_val = 2 ** bitdepth - 1
    rec = F.pad(x_rec.float(), tuple(-p for p in padding)).clamp(0, 1)
    rec_yuv = yuv_444_to_420(rgb2ycbcr(rec), mode="avg_pool")
    sums = []
    for org, r in zip(planes, rec_yuv):
        d = ((r[0, 0] * max_val).clamp(0, max_val).round() - _levels(org)).to(torch.int64)
        sums.append((d * d).sum())
    rec_q = (rec[0] * max_val).clamp(0, max_val).round()
    d = (rec_q - org_q).to(torch.int64)
    sums.append((d * d).sum())
    return torch.stack(sums), rec_q


# ---------------------------------------------------------------------------------------------------------
# public ops
# ---------------------------------------------------------------------------------------------------------
def yuv420_to_rgb(planes, bitdepth: int, mode: str = "bicubic", pad_to: int = 128):
    """One 4:2:0 frame -> (x fp32 [1, 3, Hp, Wp], padding (left, right, top, bottom), org_q fp32 [3, H, W]).

    x is the frame as BT.709 RGB, the chroma upsampled x2 with ``mode``, centred in a zero image whose sides are
    multiples of ``pad_to``; org_q holds its levels ``round(clamp(x * max_val, 0, max_val))``.  ``planes``: three
    integer tensors, or a numpy record with fields y, u, v.  Odd H or W raises ValueError before any launch."""
    planes = to_planes(planes)
    H, W = _check(planes, bitdepth)
    if mode not in MODES:
        raise ValueError(f'Invalid upsampling mode "{mode}".')
    Hp, Wp, padding = pad_geometry(H, W, pad_to)
    if planes[0].is_cuda:
        from ... import _ops

        x, org_q = _ops.yuv420_to_rgb(tuple(_container(p, bitdepth) for p in planes), bitdepth, mode, Hp, Wp,
                                      padding[2], padding[0])
    else:
        x, org_q = yuv420_to_rgb_torch(planes, bitdepth, mode, padding)
    return x, padding, org_q


def _sse(planes, org_q, x_rec, padding, bitdepth):
    planes = to_planes(planes)
    H, W = _check(planes, bitdepth)
    left, right, top, bottom = padding
    if x_rec.dim() != 4 or tuple(x_rec.shape[:2]) != (1, 3) or tuple(x_rec.shape[2:]) != (H + top + bottom,
                                                                                         W + left + right):
        raise ValueError(f"the reconstruction must be [1, 3, {H + top + bottom}, {W + left + right}], got "
                         f"{tuple(x_rec.shape)}")
    if tuple(org_q.shape) != (3, H, W):
        raise ValueError(f"org_q must be [3, {H}, {W}], got {tuple(org_q.shape)}")
    if planes[0].is_cuda:
        from ... import _ops

        return _ops.video_frame_sse(tuple(_container(p, bitdepth) for p in planes), bitdepth, org_q, x_rec, top, left)
    return frame_sse_torch(planes, org_q, x_rec, padding, bitdepth)


class FramePlanes(tuple):
    """(y, u, v) of one written frame.  ``buffer`` is the flat tensor of H W 3 / 2 samples in file order that the
    three planes are views of: a frame goes to the host, and to a file, in one copy."""

    def __new__(cls, buffer: torch.Tensor, H: int, W: int):
        n = H * W
        if buffer.dim() != 1 or buffer.numel() != n * 3 // 2:
            raise ValueError(f"a {H} x {W} 4:2:0 frame holds {n * 3 // 2} samples, got {tuple(buffer.shape)}")
        self = super().__new__(cls, (buffer[:n].view(H, W), buffer[n:n + n // 4].view(H // 2, W // 2),
                                     buffer[n + n // 4:].view(H // 2, W // 2)))
        self.buffer = buffer
        return self


def _check_rec(x_rec, padding, bitdepth: int):
    if bitdepth not in BITDEPTHS:
        raise ValueError(f"bit depth {bitdepth} not in {BITDEPTHS}")
    if len(padding) != 4 or any(int(p) != p or p < 0 for p in padding):
        raise ValueError(f"padding must be four non-negative integers (left, right, top, bottom), got {padding}")
    if not isinstance(x_rec, torch.Tensor) or x_rec.dim() != 4 or tuple(x_rec.shape[:2]) != (1, 3):
        got = tuple(x_rec.shape) if isinstance(x_rec, torch.Tensor) else type(x_rec).__name__
        raise ValueError(f"the reconstruction must be [1, 3, Hp, Wp], got {got}")
    left, right, top, bottom = (int(p) for p in padding)
    H, W = x_rec.shape[2] - top - bottom, x_rec.shape[3] - left - right
    if H % 2 or W % 2 or H < 2 or W < 2:
        raise ValueError(f"4:2:0 needs even H and W, got {H} x {W}")
    return H, W, top, left


def rgb_to_yuv420_torch(x_rec, padding, bitdepth: int) -> FramePlanes:
    H, W, _, _ = _check_rec(x_rec, padding, bitdepth)
    max_val = 2 ** bitdepth - 1
    rec = F.pad(x_rec.float(), tuple(-int(p) for p in padding)).clamp(0, 1)
    levels = [(r[0, 0] * max_val).clamp(0, max_val).round().reshape(-1)
              for r in yuv_444_to_420(rgb2ycbcr(rec), mode="avg_pool")]
    return FramePlanes(_container(torch.cat(levels).to(torch.int32), bitdepth), H, W)


def rgb_to_yuv420(x_rec, padding, bitdepth: int) -> FramePlanes:
    """The reconstruction ``x_rec`` [1, 3, Hp, Wp] (any float dtype; clamped to [0, 1] here) -> the integer 4:2:0
    frame inside ``padding`` (left, right, top, bottom): (y [H, W], u, v [H/2, W/2]), uint8 at 8 bits and unsigned
    words in int16 tensors above, views of one buffer in file order (``.buffer``).  The levels are the ones
    ``frame_sse`` measures: BT.709 RGB -> YCbCr, 2 x 2 chroma mean, rounded to nearest.  On the GPU one launch.  A
    wrong shape, odd H or W or another bit depth raises ValueError before any launch."""
    H, W, top, left = _check_rec(x_rec, padding, bitdepth)
    if x_rec.is_cuda:
        from ... import _ops

        return FramePlanes(_ops.rgb_to_yuv420(x_rec, bitdepth, H, W, top, left), H, W)
    return rgb_to_yuv420_torch(x_rec, padding, bitdepth)


def write_frame(fout, planes_or_buffer, bitdepth: int) -> int:
    """Append one frame to the open binary file ``fout`` as raw planar samples: Y, U, V, one byte each at 8 bits,
    little-endian 16-bit words above.  Takes what ``rgb_to_yuv420`` returns (one copy to the host), its flat buffer,
    or any three integer planes.  Returns the bytes written."""
    if bitdepth not in BITDEPTHS:
        raise ValueError(f"bit depth {bitdepth} not in {BITDEPTHS}")
    if isinstance(planes_or_buffer, FramePlanes):
        parts = [planes_or_buffer.buffer]
    elif isinstance(planes_or_buffer, torch.Tensor):
        parts = [planes_or_buffer]
    else:
        parts = list(to_planes(planes_or_buffer))
    n = 0
    for t in parts:
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("the samples must be integers")
        a = _container(t, bitdepth).cpu().numpy()
        data = a.tobytes() if bitdepth == 8 else a.view(np.uint16).astype("<u2", copy=False).tobytes()
        fout.write(data)
        n += len(data)
    return n


def frame_sse(planes, org_q, x_rec, padding, bitdepth: int) -> torch.Tensor:
    """int64 [4]: the sums of squared level differences between the frame and the reconstruction ``x_rec``
    [1, 3, Hp, Wp] (clamped to [0, 1] here): Y, U, V against the integer planes (RGB -> YCbCr, 2 x 2 chroma mean,
    rounded to levels) and RGB against ``org_q``."""
    return _sse(planes, org_q, x_rec, padding, bitdepth)[0]


def frame_metrics(planes, org_q, x_rec, padding, bitdepth: int) -> Dict[str, torch.Tensor]:
    """The reference driver's per-frame metrics as 0-dim tensors on the inputs' device: psnr-y, psnr-u, psnr-v,
    psnr-yuv = (4 y + u + v) / 6, mse-rgb, psnr-rgb and, when both sides exceed 160, ms-ssim-rgb (on the RGB
    levels, data_range = max_val)."""
    sums, rec_q = _sse(planes, org_q, x_rec, padding, bitdepth)
    max_val = 2 ** bitdepth - 1
    _, H, W = org_q.shape
    counts = torch.tensor([H * W, H * W // 4, H * W // 4, 3 * H * W], dtype=torch.float64, device=sums.device)
    mse = sums.double() / counts
    psnr = 20 * math.log10(max_val) - 10 * torch.log10(mse)
    out = {"psnr-y": psnr[0], "psnr-u": psnr[1], "psnr-v": psnr[2], "psnr-yuv": (4 * psnr[0] + psnr[1] + psnr[2]) / 6,
           "mse-rgb": mse[3], "psnr-rgb": psnr[3]}
    if min(H, W) > MSSSIM_MIN_SIDE:
        out["ms-ssim-rgb"] = ms_ssim(org_q[None], rec_q[None], data_range=float(max_val)).reshape(())
    return out
