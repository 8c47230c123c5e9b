"""Shared by test_codec_video_cpu.py and test_codec_video_gpu.py (helper, not a test): the seeded reconstructions,
the fp64 levels of a written 4:2:0 frame, and the level rule.

The levels restate the formulas only, on top of tests/video_reference.py: the reconstruction cropped to the frame
and clamped to [0, 1], BT.709 RGB -> YCbCr, Y per pixel and the 2 x 2 mean of Cb and Cr, times max_val, clamped to
[0, max_val] -- *before* rounding.

The level rule (test_video_frames_gpu.py's): a written level equals the rounded fp64 level, except where the fp64
level lies within max_val * EPS_REC (1e-6: the values derive from a reconstruction in [0, 1]) of a half-integer;
there it may differ by exactly 1.  Such elements are at most TIE_SHARE = 2 % of any plane of any case; that is a
property of the seeded inputs and the restatement alone, and `check_levels` asserts it on them before it looks at the
levels under test.  For the sixteen cases below the share is at most 0.5 % per plane, and 0 for the two small shapes.
"""
import functools

import numpy as np
import torch

import video_reference as R

SHAPES = [(2, 2), (6, 10), (34, 70), (130, 258)]    # one quad; small; odd W/2 and odd centred offsets; several blocks
BITDEPTHS = (8, 10)
PADS = (128, 1)


@functools.lru_cache(maxsize=None)
def rec_of(H, W, bitdepth, pad_to):
    """(reconstruction fp32 [1, 3, Hp, Wp] uniform in [-0.1, 1.1], padding (left, right, top, bottom))"""
    Hp, Wp, padding = R.pad_geometry(H, W, pad_to)
    return R.noise_rec(Hp, Wp, seed=H + W + bitdepth + 1), padding


def yuv_levels(x_rec, padding, bitdepth):
    """fp64 (Y [H, W], U [H/2, W/2], V [H/2, W/2]) before rounding."""
    max_val = 2 ** bitdepth - 1
    left, right, top, bottom = padding
    x = R.f64(x_rec).reshape((3,) + tuple(x_rec.shape[-2:]))
    H, W = x.shape[1] - top - bottom, x.shape[2] - left - right
    ycc = R.rgb2ycbcr(x[:, top:top + H, left:left + W].clamp(0, 1))
    return tuple((p * max_val).clamp(0, max_val) for p in (ycc[0], R.pool2(ycc[1]), R.pool2(ycc[2])))


@functools.lru_cache(maxsize=None)
def levels_of(H, W, bitdepth, pad_to):
    rec, padding = rec_of(H, W, bitdepth, pad_to)
    return yuv_levels(rec, padding, bitdepth)


def check_levels(planes, levels, bitdepth, what=""):
    """Assert the level rule plane by plane; returns (near-tie shares, levels off by one) for printing."""
    max_val = 2 ** bitdepth - 1
    ties = [R.near_tie(lv, max_val, R.EPS_REC) for lv in levels]
    shares = [t.double().mean().item() for t in ties]
    assert max(shares) <= R.TIE_SHARE, (what, shares)
    off = []
    for name, p, lv, tie in zip("yuv", planes, levels, ties):
        assert tuple(p.shape) == tuple(lv.shape), (what, name, tuple(p.shape))
        got = R.f64(p)
        assert got.min() >= 0 and got.max() <= max_val, (what, name)
        diff = (got - lv.round()).abs()
        assert (diff[~tie] == 0).all() and (diff[tie] <= 1).all(), (what, name, diff.max().item())
        off.append(int((diff == 1).sum()))
    return shares, off


def block_rec(Hp, Wp, seed):
    """A reconstruction of 2 x 2 blocks whose three channels are all 0 or all 1 (Hp and Wp even): every Y level is
    0 or max_val, far from any tie."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 2, (Hp // 2, Wp // 2), generator=g).float()
    return bits.repeat_interleave(2, 0).repeat_interleave(2, 1).expand(1, 3, Hp, Wp).contiguous()


def parse_frames(data: bytes, H, W, bitdepth):
    """The raw planar file's bytes -> [(y, u, v) int64 numpy arrays per frame]; 16-bit samples little-endian."""
    a = np.frombuffer(data, dtype=np.uint8 if bitdepth == 8 else np.dtype("<u2")).astype(np.int64)
    n = H * W
    assert a.size % (n * 3 // 2) == 0
    out = []
    for f in a.reshape(-1, n * 3 // 2):
        out.append((f[:n].reshape(H, W), f[n:n + n // 4].reshape(H // 2, W // 2), f[n + n // 4:].reshape(H // 2, W // 2)))
    return out


def sse(planes_a, planes_b):
    """Python ints: the sums of squared differences of Y, U, V between two frames of integer planes."""
    out = []
    for a, b in zip(planes_a, planes_b):
        d = R.f64(a).to(torch.int64) - R.f64(b).to(torch.int64)
        out.append(int((d * d).sum().item()))
    return out
