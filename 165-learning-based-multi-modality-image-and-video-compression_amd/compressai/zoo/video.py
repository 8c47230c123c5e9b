"""Video model registry (reference: compressai/zoo/video.py).

``ssf2020`` takes a quality 1..9 only to pick pretrained weights, which are remote downloads in the reference;
this build has no network, so ``pretrained=True`` raises.
"""
from ..models.video import ScaleSpaceFlow

__all__ = ["ssf2020"]

model_architectures = {
    "ssf2020": ScaleSpaceFlow,
}


def _load_model(architecture, metric, quality, pretrained=False, progress=True, **kwargs):
    if architecture not in model_architectures:
        raise ValueError(f'Invalid architecture name "{architecture}"')
    if quality not in range(1, 10):
        raise ValueError(f'Invalid quality value "{quality}"')
    if pretrained:
        raise RuntimeError("Pre-trained weights are remote downloads in the reference; not available offline")
    return model_architectures[architecture](**kwargs)


def ssf2020(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    """Scale-space flow video codec (Agustsson et al., CVPR 2020): quality 1 (lowest) .. 9."""
    if metric not in ("mse", "ms-ssim"):
        raise ValueError(f'Invalid metric "{metric}"')
    if quality < 1 or quality > 9:
        raise ValueError(f'Invalid quality "{quality}", should be between (1, 9)')
    return _load_model("ssf2020", metric, quality, pretrained, progress, **kwargs)
