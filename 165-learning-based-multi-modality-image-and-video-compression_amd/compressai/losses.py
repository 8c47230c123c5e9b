"""RD loss of the reference training script (examples/train.py:59-82).

bpp = sum_k sum(log lik_k) / (-ln2 * N*H*W); mse = mean((x_hat - x)^2);
loss = lmbda[q] * mse + bpp.  The forward is two HIP launches
(cai_rd_loss_fwd: every sum in one grid, then a fixed-order fold that forms
the three scalars), the backward one (cai_rd_loss_bwd).

metric="ms-ssim" (upstream CompressAI's second distortion): loss =
lmbda * (1 - ms_ssim(x_hat, x, data_range=1)) + bpp, the MS-SSIM and its
gradient from csrc/msssim.hip (_ops.MsSsimFn), the bpp from the same RD
kernels.  The lmbda table is the reference's, tuned for MSE on [0, 1]
images: pass `lmbda` explicitly for MS-SSIM.
"""
import torch.nn as nn

from . import _ops
from ._ops import MsSsimFn, RdLossFn, RdLossFnUnfused

LMBDA = [256, 512, 1024, 2048, 4096, 8192, 10240]   # train.py:65
METRICS = ("mse", "ms-ssim")


class RateDistortionLoss(nn.Module):
    def __init__(self, q, metric="mse", lmbda=None):
        super().__init__()
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
        self.lmbda = list(LMBDA)
        self.q = q
        self.metric = metric
        self.lmbda_override = None if lmbda is None else float(lmbda)

    def forward(self, output, target):
        N, _, H, W = target.size()
        liks = list(output["likelihoods"].values())
        fn = RdLossFnUnfused if _ops._RD_UNFUSED else RdLossFn
        lmbda = float(self.lmbda[self.q]) if self.lmbda_override is None else self.lmbda_override
        if self.metric == "mse":
            loss, mse, bpp = fn.apply(output["x_hat"], target, lmbda, N * H * W, *liks)
            return {"bpp_loss": bpp, "mse_loss": mse, "loss": loss}
        # the bpp term from the RD kernels with their squared-error segment cut down to one pixel
        # (lmbda 0: it contributes nothing, forward or backward)
        one = target.detach().reshape(-1)[:1]
        _, _, bpp = fn.apply(one, one, 0.0, N * H * W, *liks)
        ms, _ = MsSsimFn.apply(output["x_hat"], target, 1.0)
        loss = lmbda * (1.0 - ms) + bpp
        return {"bpp_loss": bpp, "ms_ssim_loss": ms, "loss": loss}


class VideoRateDistortionLoss(nn.Module):
    """Rate-distortion loss of a ScaleSpaceFlow forward: per frame lmbda * 255^2 * mse + bpp through the RD
    kernels (2 likelihood tensors for the keyframe, 4 for an inter frame), averaged over the frames."""

    def __init__(self, lmbda=1e-2):
        super().__init__()
        self.lmbda = float(lmbda)

    def forward(self, output, target):
        if not isinstance(target, (list, tuple)) or len(target) != len(output["x_hat"]):
            raise ValueError("VideoRateDistortionLoss: target must be the list of frames the model was given")
        fn = RdLossFnUnfused if _ops._RD_UNFUSED else RdLossFn
        n = len(target)
        tot = {"loss": None, "mse_loss": None, "bpp_loss": None}
        for x_hat, x, frame_liks in zip(output["x_hat"], target, output["likelihoods"]):
            N, _, H, W = x.size()
            liks = [lk for stream in frame_liks.values() for lk in stream.values()]
            loss, mse, bpp = fn.apply(x_hat, x, self.lmbda * 255.0 ** 2, N * H * W, *liks)
            for k, v in (("loss", loss), ("mse_loss", mse), ("bpp_loss", bpp)):
                tot[k] = v if tot[k] is None else tot[k] + v
        return {k: v / n for k, v in tot.items()}
