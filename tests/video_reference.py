"""fp64 restatement of the raw-video frame path, from formulas only (helper, not a test).

The four transforms of compressai.transforms.functional, the padded YUV 4:2:0 -> RGB conversion and the per-frame
metrics of compressai.utils.video.frames.  Nothing here calls an interpolation or pooling routine: the x2
upsampling is written out with its taps (align_corners = false semantics: output 2k sits at source k - 1/4, output
2k + 1 at k + 1/4; tap indices clamp to the plane).

Besides the values, the conversions return the fp64 levels *before* rounding.  An fp32 implementation may round an
element the other way only where that level lies within ``max_val * eps`` of a half-integer (``near_tie``); the
tests allow a difference of exactly 1 there and nowhere else, and bound the sums of squares accordingly
(``sse_slack``).
"""
import math

import numpy as np
import torch

KR, KG, KB = 0.2126, 0.7152, 0.0722
BICUBIC = (-0.03515625, 0.26171875, 0.87890625, -0.10546875)      # A = -0.75 at t = 3/4: taps k-2 .. k+1 of output 2k
EPS_ORG = 4e-6      # the model-input bound: at most 16 fp32 roundings of intermediates below 4
EPS_REC = 1e-6      # everything derived from the reconstruction, whose values are in [0, 1]
TIE_SHARE = 0.02


def f64(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t).astype(np.int64))
    if t.dtype == torch.int16:
        t = t.to(torch.int32) & 0xFFFF
    return t.detach().cpu().double()


def _up2_axis(x, mode, axis):
    n = x.shape[axis]
    k = torch.arange(n)

    def tap(off):
        return x.index_select(axis, (k + off).clamp(0, n - 1))

    if mode == "nearest":
        even = odd = tap(0)
    elif mode == "bilinear":
        even = 0.25 * tap(-1) + 0.75 * tap(0)     # k = 0: the coordinate is clamped to 0, which is sample 0 again
        odd = 0.75 * tap(0) + 0.25 * tap(1)
    elif mode == "bicubic":
        w = BICUBIC
        even = w[0] * tap(-2) + w[1] * tap(-1) + w[2] * tap(0) + w[3] * tap(1)
        odd = w[3] * tap(-1) + w[2] * tap(0) + w[1] * tap(1) + w[0] * tap(2)
    else:
        raise ValueError(mode)
    axis = axis % x.dim()
    out = torch.stack((even, odd), dim=axis + 1)
    shape = list(x.shape)
    shape[axis] = 2 * n
    return out.reshape(shape)


def up2(x, mode):
    """[..., h, w] -> [..., 2h, 2w]"""
    return _up2_axis(_up2_axis(x, mode, -1), mode, -2)


def pool2(x):
    """[..., 2h, 2w] -> [..., h, w]: the 2 x 2 mean"""
    return (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) / 4


def rgb2ycbcr(rgb):
    r, g, b = rgb.unbind(-3)
    y = KR * r + KG * g + KB * b
    return torch.stack((y, 0.5 * (b - y) / (1 - KB) + 0.5, 0.5 * (r - y) / (1 - KR) + 0.5), dim=-3)


def ycbcr2rgb(ycbcr):
    y, cb, cr = ycbcr.unbind(-3)
    r = y + (2 - 2 * KR) * (cr - 0.5)
    b = y + (2 - 2 * KB) * (cb - 0.5)
    return torch.stack((r, (y - KR * r - KB * b) / KG, b), dim=-3)


def yuv_444_to_420(yuv):
    y, u, v = yuv.chunk(3, 1) if isinstance(yuv, torch.Tensor) else yuv
    return y, pool2(u), pool2(v)


def yuv_420_to_444(yuv, mode="bilinear"):
    y, u, v = yuv
    return torch.cat((y, up2(u, mode), up2(v, mode)), dim=1)


def pad_geometry(H, W, pad_to):
    Hp, Wp = (H + pad_to - 1) // pad_to * pad_to, (W + pad_to - 1) // pad_to * pad_to
    left, top = (Wp - W) // 2, (Hp - H) // 2
    return Hp, Wp, (left, Wp - W - left, top, Hp - H - top)


def to_rgb(planes, bitdepth, mode="bicubic", pad_to=128):
    """{x [3, Hp, Wp], padding, level [3, H, W] (before rounding), org_q [3, H, W]}"""
    max_val = 2 ** bitdepth - 1
    y, u, v = (f64(p) / max_val for p in planes)
    rgb = ycbcr2rgb(torch.stack((y, up2(u, mode), up2(v, mode))))
    H, W = y.shape
    Hp, Wp, padding = pad_geometry(H, W, pad_to)
    x = torch.zeros(3, Hp, Wp, dtype=torch.float64)
    x[:, padding[2]:padding[2] + H, padding[0]:padding[0] + W] = rgb
    level = (rgb * max_val).clamp(0, max_val)
    return {"x": x, "padding": padding, "level": level, "org_q": level.round()}


def near_tie(level, max_val, eps):
    return ((level - level.floor()) - 0.5).abs() < max_val * eps


def sse_slack(d, tie):
    """What a sum of d^2 may move by when every near-tie element's difference moves by 1: sum of 2 |d| + 1."""
    return int((2 * d[tie].abs() + 1).sum().item())


def frame_metrics(planes, org_q, x_rec, padding, bitdepth, org_tie=None):
    """The per-frame metrics of the reconstruction x_rec [3, Hp, Wp] (or [1, 3, Hp, Wp]) against the integer
    planes and the RGB levels org_q.  Returns the four sums ("sse": Y, U, V, RGB, python ints), their slacks under
    the near-tie rule (org_tie: the near-tie mask of org_q, when it is the restatement's own), the PSNRs, mse-rgb,
    rec_q, its pre-rounding level and its near-tie mask."""
    max_val = 2 ** bitdepth - 1
    left, right, top, bottom = padding
    x_rec = f64(x_rec).reshape((3,) + tuple(x_rec.shape[-2:]))
    H, W = x_rec.shape[1] - top - bottom, x_rec.shape[2] - left - right
    rec = x_rec[:, top:top + H, left:left + W].clamp(0, 1)
    ycc = rgb2ycbcr(rec)
    levels = [(ycc[0] * max_val).clamp(0, max_val), (pool2(ycc[1]) * max_val).clamp(0, max_val),
              (pool2(ycc[2]) * max_val).clamp(0, max_val)]
    sse, slack = [], []
    for lv, org in zip(levels, planes):
        d = lv.round() - f64(org)
        sse.append(int((d * d).sum().item()))
        slack.append(sse_slack(d, near_tie(lv, max_val, EPS_REC)))
    rec_level = (rec * max_val).clamp(0, max_val)
    rec_tie = near_tie(rec_level, max_val, EPS_REC)
    d = rec_level.round() - f64(org_q)
    sse.append(int((d * d).sum().item()))
    slack.append(sse_slack(d, rec_tie if org_tie is None else rec_tie | org_tie))
    counts = [H * W, H * W // 4, H * W // 4, 3 * H * W]
    ties = [int(near_tie(lv, max_val, EPS_REC).sum()) for lv in levels] + [int(rec_tie.sum())]
    psnr = [20 * math.log10(max_val) - 10 * math.log10(s / n) if s else math.inf for s, n in zip(sse, counts)]
    return {"sse": sse, "slack": slack, "counts": counts, "tie_share": [t / n for t, n in zip(ties, counts)],
            "psnr-y": psnr[0], "psnr-u": psnr[1], "psnr-v": psnr[2], "psnr-yuv": (4 * psnr[0] + psnr[1] + psnr[2]) / 6,
            "mse-rgb": sse[3] / counts[3], "psnr-rgb": psnr[3], "rec_q": rec_level.round(), "rec_level": rec_level,
            "rec_tie": rec_tie}


def psnr_slack(sse, slack):
    """|delta PSNR| allowed when the sum may move by `slack`: 10 log10((sse + slack) / (sse - slack))."""
    if slack == 0:
        return 1e-9        # the PSNR itself is an fp64 log of the same integers
    if sse - slack <= 0:
        return math.inf
    return 10 * math.log10((sse + slack) / (sse - slack)) + 1e-9


# ---------------------------------------------------------------------------------------------------------
# seeded inputs shared by the CPU and GPU tests
# ---------------------------------------------------------------------------------------------------------
def noise_planes(H, W, bitdepth, seed):
    """Uniform noise over the whole range, as torch tensors in the file's container (uint8 / int16 words)."""
    rng = np.random.default_rng(seed)
    max_val = 2 ** bitdepth - 1
    shapes = ((H, W), (H // 2, W // 2), (H // 2, W // 2))
    return tuple(as_container(rng.integers(0, max_val + 1, size=s), bitdepth) for s in shapes)


def extreme_planes(H, W, bitdepth, seed):
    """Every sample 0 or max_val, in blocks: the bicubic overshoots and the clamp to [0, max_val] acts."""
    rng = np.random.default_rng(seed)
    max_val = 2 ** bitdepth - 1
    shapes = ((H, W), (H // 2, W // 2), (H // 2, W // 2))
    return tuple(as_container(rng.integers(0, 2, size=s) * max_val, bitdepth) for s in shapes)


def as_container(a, bitdepth):
    a = np.asarray(a)
    if bitdepth == 8:
        return torch.from_numpy(a.astype(np.uint8))
    return torch.from_numpy(a.astype(np.uint16).view(np.int16))


def noise_rec(Hp, Wp, seed):
    """A reconstruction uniform in [-0.1, 1.1] (fp32 values): its clamp to [0, 1] acts."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(1, 3, Hp, Wp, generator=g, dtype=torch.float64) * 1.2 - 0.1).float()


def write_clip(path, frames, bitdepth):
    """frames: a list of (y, u, v) integer numpy arrays -> a raw planar file (uint8, or little-endian uint16)."""
    dt = np.uint8 if bitdepth == 8 else np.dtype("<u2")
    with open(path, "wb") as f:
        for planes in frames:
            for p in planes:
                f.write(np.ascontiguousarray(p).astype(dt).tobytes())


def moving_clip(H, W, n, bitdepth, seed):
    """A smooth seeded pattern drifting a few pixels per frame plus a little noise, as n frames of integer planes."""
    rng = np.random.default_rng(seed)
    max_val = 2 ** bitdepth - 1
    yy, xx = np.mgrid[0:H + 4 * n, 0:W + 4 * n].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, size=6)
    base = [0.5 + 0.25 * np.sin(xx / 17 + ph[2 * c]) * np.cos(yy / 23 + ph[2 * c + 1])
            + 0.15 * np.sin((xx + yy) / 9 + ph[c]) for c in range(3)]
    frames = []
    for i in range(n):
        planes = []
        for c in range(3):
            win = base[c][3 * i:3 * i + H, 2 * i:2 * i + W]
            if c:
                win = 0.5 + 0.5 * (win[0::2, 0::2] - 0.5)
            win = win + 0.02 * rng.standard_normal(win.shape)
            planes.append(np.clip(np.rint(win * max_val), 0, max_val).astype(np.int64))
        frames.append(tuple(planes))
    return frames
