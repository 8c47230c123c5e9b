"""Plain-torch restatement of the ScaleSpaceFlow video model, written from its description: the comparison
target of test_ssf_*.py.  CPU (or any device torch runs on), fp32 or fp64; built on the oracle's entropy models.

  QReLU              clamp(0, 2^bits - 1); backward g inside, g exp(-alpha^beta |2x/max - 1|^beta) outside
  quantize_ste       round with identity gradient
  gaussian_volume    level 0 = x, level 1 = blur(x) (replicate padding, k = 2 ceil(3 sigma) + 1), level i + 1 =
                     avg_pool 2x2 -> blur -> bilinear x2 (align_corners=False) applied i times
  warp_volume        5-D grid_sample (trilinear, border, align_corners=False) at (base_xy + flow, scale)
  Hyperprior         mean-scale hyperprior; y_hat = quantize_ste(y - means) + means (optionally overridden:
                     teacher forcing for the staged model comparison)
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import cai_oracle as O

ALPHA = 0.9943258522851727


class QReLU(torch.autograd.Function):
    """Clamp to [0, top], top = 2^bits - 1.  The gradient passes unchanged inside the range; outside it is damped by
    exp(-(ALPHA |u|)^beta) with u = 2 x / top - 1, written here as exp(-ALPHA^beta |u|^beta)."""

    @staticmethod
    def forward(ctx, x, bit_depth, beta):
        top = float(2 ** bit_depth - 1)
        ctx.save_for_backward(x)
        ctx.top, ctx.beta = top, beta
        return torch.clamp(x, 0.0, top)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        u = (2.0 * x / ctx.top - 1).abs()
        damp = torch.exp(-(ALPHA ** ctx.beta) * u.pow(ctx.beta))
        outside = (x < 0) | (x > ctx.top)
        return torch.where(outside, g * damp, g), None, None


def quantize_ste(x):
    """round(x) in value, x in gradient."""
    return x + (torch.round(x) - x).detach()


def gaussian_kernel1d(kernel_size, sigma, device, dtype):
    """Normalised samples of exp(-d^2 / (2 sigma^2)) at the tap distances d from the window centre."""
    centre = (kernel_size - 1) / 2
    d = torch.tensor([k - centre for k in range(kernel_size)], device=device, dtype=dtype)
    w = torch.exp(-(d / sigma) ** 2 / 2)
    return w / w.sum()


def gaussian_kernel2d(kernel_size, sigma, device, dtype):
    w = gaussian_kernel1d(kernel_size, sigma, device, dtype)
    return w.unsqueeze(1) * w.unsqueeze(0)


def gaussian_blur(x, kernel):
    """Depthwise 2-D filter with the border pixels repeated outwards."""
    k = kernel.shape[-1]
    C = x.shape[1]
    padded = F.pad(x, [k // 2] * 4, mode="replicate")
    return F.conv2d(padded, kernel[None, None].repeat(C, 1, 1, 1), groups=C)


def _times_two(t, steps):
    """`steps` successive bilinear x2 resamplings (not one x2^steps resampling: a different operator)."""
    for _ in range(steps):
        t = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
    return t


def gaussian_volume(x, sigma, num_levels):
    """Slices: x; blur(x); then, level by level, the previous blurred image pooled 2x2 and blurred again, brought
    back to full size by as many x2 steps as it was pooled."""
    kernel = gaussian_kernel2d(2 * int(math.ceil(3 * sigma)) + 1, sigma, x.device, x.dtype)
    coarse = gaussian_blur(x, kernel)
    slices = [x, coarse]
    for pooled in range(1, num_levels):
        coarse = gaussian_blur(F.avg_pool2d(coarse, 2), kernel)
        slices.append(_times_two(coarse, pooled))
    return torch.stack(slices, dim=2)


def base_grid(N, H, W, device, dtype, exact=False):
    """The warp's identity grid [N, H, W, 2].  exact=False: affine_grid's (linspace(-1, 1) scaled by (n - 1) / n,
    the upstream weighting); exact=True: (2 i + 1) / n - 1 evaluated directly."""
    if exact:
        xs = (2 * torch.arange(W, device=device, dtype=dtype) + 1) / W - 1
        ys = (2 * torch.arange(H, device=device, dtype=dtype) + 1) / H - 1
        return torch.stack((xs[None, :].expand(H, W), ys[:, None].expand(H, W)), dim=-1)[None].expand(N, H, W, 2)
    identity = torch.zeros(N, 2, 3, device=device, dtype=dtype)
    identity[:, 0, 0] = 1
    identity[:, 1, 1] = 1
    return F.affine_grid(identity, [N, 1, H, W], align_corners=False)


def warp_volume(volume, flow, scale_field, exact_grid=False):
    """Trilinear border-clamped sample of [N, C, D, H, W] at (identity_xy + flow, scale) per output pixel."""
    N, C, D, H, W = volume.shape
    xy = base_grid(N, H, W, volume.device, volume.dtype, exact_grid) + flow.movedim(1, -1)
    coords = torch.cat((xy, scale_field.movedim(1, -1)), dim=-1)             # [N, H, W, 3]
    sampled = F.grid_sample(volume, coords[:, None], mode="bilinear", padding_mode="border", align_corners=False)
    return sampled[:, :, 0]


def forward_prediction(x_ref, motion_info, sigma0=1.5, num_levels=5):
    flow, scale_field = motion_info[:, :2], motion_info[:, 2:]
    return warp_volume(gaussian_volume(x_ref, sigma0, num_levels), flow, scale_field)


def _encoder(cin, mid=128, cout=192):
    return nn.Sequential(O.conv(cin, mid), nn.ReLU(inplace=True), O.conv(mid, mid), nn.ReLU(inplace=True),
                         O.conv(mid, mid), nn.ReLU(inplace=True), O.conv(mid, cout))


def _decoder(cout, cin=192, mid=128):
    return nn.Sequential(O.deconv(cin, mid), nn.ReLU(inplace=True), O.deconv(mid, mid), nn.ReLU(inplace=True),
                         O.deconv(mid, mid), nn.ReLU(inplace=True), O.deconv(mid, cout))


def _hyper_encoder(p=192):
    return nn.Sequential(O.conv(p, p), nn.ReLU(inplace=True), O.conv(p, p), nn.ReLU(inplace=True), O.conv(p, p))


def _hyper_decoder(p=192):
    return nn.Sequential(O.deconv(p, p), nn.ReLU(inplace=True), O.deconv(p, p), nn.ReLU(inplace=True),
                         O.deconv(p, p))


class ScaleDecoder(nn.Module):
    """deconv1..3, each followed by QReLU(8 bits, beta 100)."""

    def __init__(self, p=192):
        super().__init__()
        for i in (1, 2, 3):
            setattr(self, f"deconv{i}", O.deconv(p, p))

    def forward(self, t):
        for i in (1, 2, 3):
            t = QReLU.apply(getattr(self, f"deconv{i}")(t), 8, 100)
        return t


class Hyperprior(O.CompressionModel):
    def __init__(self, planes=192):
        super().__init__(entropy_bottleneck_channels=planes)
        self.hyper_encoder = _hyper_encoder(planes)
        self.hyper_decoder_mean = _hyper_decoder(planes)
        self.hyper_decoder_scale = ScaleDecoder(planes)
        self.gaussian_conditional = O.GaussianConditional(None)

    def forward(self, y, y_hat=None, trace=None):
        """y_hat: the quantised latent to use instead of this model's own rounding (its value; the gradient
        still passes straight through to y).  trace: a dict that receives y, means, scales."""
        z = self.hyper_encoder(y)
        z_hat, z_lik = self.entropy_bottleneck(z)
        scales = self.hyper_decoder_scale(z_hat)
        means = self.hyper_decoder_mean(z_hat)
        _, y_lik = self.gaussian_conditional(y, scales, means)
        own = quantize_ste(y - means) + means
        if trace is not None:
            trace.update(y=y, means=means, scales=scales, y_hat=own)
        if y_hat is not None:
            own = (y_hat.to(y.dtype) - y).detach() + y
        return own, {"y": y_lik, "z": z_lik}


class ScaleSpaceFlow(nn.Module):
    def __init__(self, num_levels=5, sigma0=1.5, scale_field_shift=1.0):
        super().__init__()
        self.img_encoder = _encoder(3)
        self.img_decoder = _decoder(3)
        self.img_hyperprior = Hyperprior()
        self.res_encoder = _encoder(3)
        self.res_decoder = _decoder(3, cin=384)
        self.res_hyperprior = Hyperprior()
        self.motion_encoder = _encoder(6)
        self.motion_decoder = _decoder(3)
        self.motion_hyperprior = Hyperprior()
        self.sigma0, self.num_levels, self.scale_field_shift = sigma0, num_levels, scale_field_shift

    def forward(self, frames, y_hats=None, traces=None):
        """y_hats: per frame {"keyframe": t} / {"motion": t, "residual": t} overrides (teacher forcing);
        traces: a list that receives one dict of stage tensors per frame."""
        if not isinstance(frames, list):
            raise RuntimeError("Invalid number of frames")

        def hp(mod, y, i, key):
            tr = {} if traces is not None else None
            out = mod(y, None if y_hats is None else y_hats[i][key], tr)
            if traces is not None:
                traces[i][key] = tr
            return out

        if traces is not None:
            traces.extend({} for _ in frames)
        recs, liks = [], []
        y = self.img_encoder(frames[0])
        y_hat, lk = hp(self.img_hyperprior, y, 0, "keyframe")
        x_hat = self.img_decoder(y_hat)
        recs.append(x_hat)
        liks.append({"keyframe": lk})
        x_ref = x_hat.detach()
        for i in range(1, len(frames)):
            x_cur = frames[i]
            y_m = self.motion_encoder(torch.cat((x_cur, x_ref), dim=1))
            y_m_hat, lk_m = hp(self.motion_hyperprior, y_m, i, "motion")
            motion_info = self.motion_decoder(y_m_hat)
            x_pred = forward_prediction(x_ref, motion_info, self.sigma0, self.num_levels)
            y_r = self.res_encoder(x_cur - x_pred)
            y_r_hat, lk_r = hp(self.res_hyperprior, y_r, i, "residual")
            x_res_hat = self.res_decoder(torch.cat((y_r_hat, y_m_hat), dim=1))
            x_ref = x_pred + x_res_hat
            recs.append(x_ref)
            liks.append({"motion": lk_m, "residual": lk_r})
        return {"x_hat": recs, "likelihoods": liks}

    def aux_loss(self):
        return [m.aux_loss() for m in self.modules() if isinstance(m, O.CompressionModel)]


def video_rd_loss(output, frames, lmbda):
    """Per frame lmbda * 255^2 * mse + bpp, averaged over the frames."""
    tot = {"loss": 0.0, "mse_loss": 0.0, "bpp_loss": 0.0}
    for x_hat, x, fl in zip(output["x_hat"], frames, output["likelihoods"]):
        N, _, H, W = x.shape
        bpp = sum(torch.log(lk).sum() for s in fl.values() for lk in s.values()) / (-math.log(2) * N * H * W)
        mse = torch.mean((x_hat - x) ** 2)
        tot["bpp_loss"] = tot["bpp_loss"] + bpp
        tot["mse_loss"] = tot["mse_loss"] + mse
        tot["loss"] = tot["loss"] + lmbda * 255.0 ** 2 * mse + bpp
    return {k: v / len(frames) for k, v in tot.items()}
