"""MS-SSIM op: the C-ABI argument validation (no kernel is launched), the loss's metric argument, and a pin of
the torch body's single-scale SSIM against an independent scipy.ndimage computation."""
import ctypes
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def native():
    from compressai import _native

    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libcai.so not built")
    _native.lib.load()
    return _native


def test_abi_rejects_bad_arguments(native):
    lib = native.lib.load()
    buf = ctypes.create_string_buffer(64)           # never dereferenced: validation returns before any device work
    p = ctypes.c_void_p(ctypes.addressof(buf))
    P, H, W = 3, 161, 200
    need = lib.cai_msssim_workspace_bytes(P, H, W, 1)
    assert need > lib.cai_msssim_workspace_bytes(P, H, W, 0) > 0

    def fwd(x=p, y=p, planes=P, h=H, w=W, per_plane=p, mean=p, ws=p, nb=need):
        return lib.cai_msssim_fwd(x, y, planes, h, w, 1.0, 1, per_plane, mean, ws, nb, None)

    def bwd(x=p, y=p, planes=P, h=H, w=W, per_plane=p, g=p, dx=p, ws=p, nb=need):
        return lib.cai_msssim_bwd(x, y, planes, h, w, per_plane, g, None, dx, ws, nb, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(x=None), b"null pointer"), (dict(y=None), b"null pointer"),
                        (dict(per_plane=None), b"null pointer"),
                        (dict(planes=0), b"positive"), (dict(h=0), b"positive"), (dict(w=-4), b"positive"),
                        (dict(h=160), b"must exceed 160"), (dict(w=160), b"must exceed 160"),
                        (dict(ws=None), b"workspace"), (dict(nb=need - 4), b"workspace")):
            assert call(**kw) == native.CAI_EINVAL, kw
            assert msg in lib.cai_last_error(), (kw, lib.cai_last_error())
    assert fwd(mean=None) == native.CAI_EINVAL and b"null pointer" in lib.cai_last_error()
    assert bwd(dx=None) == native.CAI_EINVAL and b"null pointer" in lib.cai_last_error()
    assert bwd(g=None) == native.CAI_EINVAL and b"upstream" in lib.cai_last_error()
    for shape in ((0, H, W), (P, 160, W), (P, H, 100), (P, -1, W)):
        assert lib.cai_msssim_workspace_bytes(*shape, 1) == 0
    with pytest.raises(ValueError, match="must exceed 160"):
        native.lib.cai_msssim_fwd(p, p, P, 160, 160, 1.0, 0, p, p, p, need, None)


def test_loss_metric_argument():
    from compressai.losses import RateDistortionLoss

    with pytest.raises(ValueError):
        RateDistortionLoss(1, metric="psnr")
    assert RateDistortionLoss(1, metric="ms-ssim", lmbda=8.0).metric == "ms-ssim"
    assert RateDistortionLoss(1).metric == "mse"


def test_single_scale_ssim_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    from compressai.utils import metrics

    rng = np.random.default_rng(0)
    x = rng.uniform(0, 1, (40, 50))
    y = np.clip(x + rng.normal(0, 0.1, x.shape), 0, 1)
    k = np.arange(11) - 5
    g = np.exp(-(k ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()

    def filt(a):
        a = ndimage.correlate1d(a, g, axis=0, mode="constant")
        return ndimage.correlate1d(a, g, axis=1, mode="constant")[5:-5, 5:-5]

    m1, m2 = filt(x), filt(y)
    s1, s2, s12 = filt(x * x) - m1 * m1, filt(y * y) - m2 * m2, filt(x * y) - m1 * m2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim = (2 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1) * cs
    X = torch.tensor(x)[None, None]
    Y = torch.tensor(y)[None, None]
    win = metrics._gauss_1d(11, 1.5, X.device, torch.float64)
    got_ssim, got_cs = metrics._ssim(X, Y, win, 1.0)
    assert got_ssim.dtype == torch.float64
    assert abs(got_ssim.item() - ssim.mean()) <= 1e-10
    assert abs(got_cs.item() - cs.mean()) <= 1e-10
