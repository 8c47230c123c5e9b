"""Model helpers (reference: compressai/models/utils.py:20-146)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .._native import Q_DEQUANTIZE
from ..layers.conv import Conv2d, ConvTranspose2d


def find_named_module(module, query):
    return next((m for n, m in module.named_modules() if n == query), None)


def find_named_buffer(module, query):
    return next((b for n, b in module.named_buffers() if n == query), None)


def _update_registered_buffer(module, buffer_name, state_dict_key, state_dict, policy="resize_if_empty",
                              dtype=torch.int):
    new_size = state_dict[state_dict_key].size()
    registered_buf = find_named_buffer(module, buffer_name)
    if policy in ("resize_if_empty", "resize"):
        if registered_buf is None:
            raise RuntimeError(f'buffer "{buffer_name}" was not registered')
        if policy == "resize" or registered_buf.numel() == 0:
            registered_buf.resize_(new_size)
    elif policy == "register":
        if registered_buf is not None:
            raise RuntimeError(f'buffer "{buffer_name}" was already registered')
        module.register_buffer(buffer_name, torch.empty(new_size, dtype=dtype).fill_(0))
    else:
        raise ValueError(f'Invalid policy "{policy}"')


def update_registered_buffers(module, module_name, buffer_names, state_dict, policy="resize_if_empty",
                              dtype=torch.int):
    valid = [n for n, _ in module.named_buffers()]
    for b in buffer_names:
        if b not in valid:
            raise ValueError(f'Invalid buffer name "{b}"')
    for b in buffer_names:
        _update_registered_buffer(module, b, f"{module_name}.{b}", state_dict, policy, dtype)


def conv(in_channels, out_channels, kernel_size=5, stride=2):
    """Conv2d(k, s, p=k//2) -- models/utils.py:128-135."""
    return Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2)


def deconv(in_channels, out_channels, kernel_size=5, stride=2):
    """ConvTranspose2d(k, s, p=k//2, output_padding=s-1) -- models/utils.py:138-146."""
    return ConvTranspose2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                           output_padding=stride - 1, padding=kernel_size // 2)


class _QuantizeSteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        from ..entropy_models.entropy_models import _QuantizeFn

        return _QuantizeFn.forward(ctx, x, None, None, Q_DEQUANTIZE)

    @staticmethod
    def backward(ctx, g):
        return g


def quantize_ste(x):
    """round(x) on the quantize kernel with the straight-through (identity) gradient."""
    return _QuantizeSteFn.apply(x)


def gaussian_kernel1d(kernel_size: int, sigma: float, device: torch.device, dtype: torch.dtype):
    """Normalised Gaussian taps exp(-d^2 / (2 sigma^2)) at the integer (odd size) or half-integer (even size)
    distances d from the window's centre."""
    d = torch.arange(kernel_size, device=device, dtype=dtype) - 0.5 * (kernel_size - 1)
    taps = torch.exp(d * d / (-2.0 * sigma * sigma))
    return taps / taps.sum()


def gaussian_kernel2d(kernel_size: int, sigma: float, device: torch.device, dtype: torch.dtype):
    """The separable 2D Gaussian window: the outer product of the 1D taps with themselves."""
    taps = gaussian_kernel1d(kernel_size, sigma, device, dtype)
    return torch.outer(taps, taps)


def gaussian_blur(x, kernel=None, kernel_size=None, sigma=None):
    """2D Gaussian blur with replicate padding on the scale-space blur kernel
    (csrc/ssf.hip).  That kernel builds its own taps from sigma, for the size the model uses
    (2 ceil(3 sigma) + 1): a `kernel` argument is accepted when it is such a Gaussian (its sigma is read back
    from its centre taps), anything else is refused.  A convenience, not a hot path: it is slice 1 of a one-level
    volume, which also writes the slice-0 copy."""
    from .._ops import ScaleSpaceVolumeFn

    if kernel is None:
        if kernel_size is None or sigma is None:
            raise RuntimeError("Missing kernel_size or sigma parameters")
    else:
        if kernel.dim() != 2 or kernel.shape[0] != kernel.shape[1] or kernel.shape[0] % 2 == 0 or kernel.shape[0] < 3:
            raise ValueError("gaussian_blur: kernel must be a square 2D Gaussian of odd size >= 3")
        k1 = kernel.detach().double().cpu()      # a host read: the blur kernel takes sigma, not taps
        kernel_size = k1.shape[0]
        c = kernel_size // 2
        ratio = float(k1[c, c] / k1[c, c + 1]) if float(k1[c, c + 1]) > 0 else 0.0
        if not ratio > 1.0:
            raise ValueError("gaussian_blur: only normalised Gaussian kernels are supported")
        sigma = math.sqrt(0.5 / math.log(ratio))
        want = gaussian_kernel2d(kernel_size, sigma, torch.device("cpu"), torch.float64)
        if not torch.allclose(k1, want, rtol=1e-4, atol=1e-7):
            raise ValueError("gaussian_blur: only normalised Gaussian kernels are supported")
    if kernel_size != 2 * int(math.ceil(3 * sigma)) + 1:
        raise ValueError(f"gaussian_blur: kernel_size {kernel_size} is not 2 ceil(3 sigma) + 1 for sigma {sigma:g}")
    return ScaleSpaceVolumeFn.apply(x, float(sigma), 1)[:, :, 1]


def meshgrid2d(N: int, C: int, H: int, W: int, device: torch.device):
    """The identity sampling grid [N, H, W, 2] of grid_sample (pixel centres, align_corners=False)."""
    identity = torch.zeros(N, 2, 3, device=device)
    identity[:, 0, 0] = 1.0
    identity[:, 1, 1] = 1.0
    return F.affine_grid(identity, [N, C, H, W], align_corners=False)
