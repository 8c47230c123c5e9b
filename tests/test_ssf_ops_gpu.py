"""The scale-space ops of ScaleSpaceFlow on the GPU (csrc/ssf.hip, QReLU in csrc/elementwise.hip) against the
plain-torch restatement (tests/ssf_reference.py) run on the CPU in fp64.

Bars: 4 x e_ref per tensor, e_ref = the fp32 CPU restatement's own max error against fp64 on the same inputs,
computed inside each test (margin 4: the kernels order the eight-term blend, the separable blur and the
coordinate arithmetic differently under the same error model).  Exact cases are bit-equal.
"""
import pytest
import torch

import ssf_reference as R

pytestmark = pytest.mark.gpu

MARGIN = 4.0


def maxerr(a, b64):
    return (a.detach().double().cpu() - b64.detach().double().cpu()).abs().max().item()


def check(name, got, ref32, ref64):
    e, e_ref = maxerr(got, ref64), maxerr(ref32, ref64)
    print(f"\n{name}: kernel {e:.3e}  fp32 restatement {e_ref:.3e}  (|ref| max {ref64.abs().max().item():.3g})")
    assert e <= MARGIN * e_ref, (name, e, e_ref)


# ------------------------------------------------------------------------------------------------ warp

def test_warp_exact_integer_shifts(cuda):
    """Integer volume, integer pixel shifts (flow = 2 d / W, power-of-two sizes), scale +-0.5 at D = 2 (iz exactly
    0 or 1): bit-equal to the analytic gather vol[n, c, lev, clamp(h + dy), clamp(w + dx)]."""
    from compressai._ops import ScaleSpaceWarpFn

    g = torch.Generator().manual_seed(0)
    N, C, D, H, W = 2, 3, 2, 16, 32
    vol = torch.randint(-3, 4, (N, C, D, H, W), generator=g).float()
    dx = torch.randint(-5, 6, (N, H, W), generator=g)
    dy = torch.randint(-5, 6, (N, H, W), generator=g)
    lev = torch.randint(0, 2, (N, H, W), generator=g)
    motion = torch.stack((2.0 * dx / W, 2.0 * dy / H, lev.float() - 0.5), dim=1)
    hh = (torch.arange(H)[None, :, None] + dy).clamp(0, H - 1)
    ww = (torch.arange(W)[None, None, :] + dx).clamp(0, W - 1)
    assert (ww != torch.arange(W)[None, None, :] + dx).any() and (hh != torch.arange(H)[None, :, None] + dy).any()
    n = torch.arange(N)[:, None, None].expand(N, H, W)
    want = torch.stack([vol[n, c, lev, hh, ww] for c in range(C)], dim=1)
    out = ScaleSpaceWarpFn.apply(vol.to(cuda), motion.to(cuda))
    assert torch.equal(out.cpu(), want)
    # the same through a pixel-major (channels-last, padded) motion tensor: read in place through its strides
    buf = torch.zeros(N, H, W, 8, device=cuda)
    buf[..., :3] = motion.to(cuda).permute(0, 2, 3, 1)
    out2 = ScaleSpaceWarpFn.apply(vol.to(cuda), buf.permute(0, 3, 1, 2)[:, :3])
    assert torch.equal(out2.cpu(), want)


def _fractional_case(N, C, D, H, W, seed):
    """Targets integer + frac, frac in [0.15, 0.85]; integers from [-4, size + 3) (depth [-1, D)): every axis is
    clamped somewhere, and every sample stays >= 0.15 of a cell from a gradient discontinuity."""
    g = torch.Generator().manual_seed(seed)

    def target(size, lo, hi, shape):
        i = torch.randint(lo, hi, shape, generator=g).double()
        return i + 0.15 + 0.7 * torch.rand(shape, generator=g, dtype=torch.float64)

    tx = target(W, -4, W + 3, (N, H, W))
    ty = target(H, -4, H + 3, (N, H, W))
    tz = target(D, -1, D, (N, H, W))
    fx = (tx - torch.arange(W, dtype=torch.float64)[None, None, :]) * 2 / W
    fy = (ty - torch.arange(H, dtype=torch.float64)[None, :, None]) * 2 / H
    sc = (2 * tz + 1) / D - 1
    motion = torch.stack((fx, fy, sc), dim=1).float()
    vol = torch.randn(N, C, D, H, W, generator=g)
    gout = torch.randn(N, C, H, W, generator=g)
    x_cur = torch.rand(N, C, H, W, generator=g)
    return vol, motion, gout, x_cur


def _warp_ref(vol, motion, gout, dtype):
    v = vol.clone().to(dtype).requires_grad_(True)
    m = motion.clone().to(dtype).requires_grad_(True)
    out = R.warp_volume(v, m[:, :2], m[:, 2:])
    out.backward(gout.to(dtype))
    return out.detach(), m.grad, v.grad


@pytest.mark.parametrize("H,W", [(32, 48), (16, 16)])
def test_warp_fractional_against_fp64(cuda, H, W):
    from compressai._ops import ScaleSpaceWarpFn

    N, C, D = 2, 3, 6
    vol, motion, gout, x_cur = _fractional_case(N, C, D, H, W, seed=H + W)
    o64, dm64, dv64 = _warp_ref(vol, motion, gout, torch.float64)
    o32, dm32, dv32 = _warp_ref(vol, motion, gout, torch.float32)
    v = vol.to(cuda).requires_grad_(True)
    m = motion.to(cuda).requires_grad_(True)
    x_pred, x_res = ScaleSpaceWarpFn.apply(v, m, x_cur.to(cuda))
    assert torch.equal(x_res, x_cur.to(cuda) - x_pred)
    x_pred.backward(gout.to(cuda))
    check("warp out", x_pred, o32, o64)
    check("warp d_flow", m.grad[:, :2], dm32[:, :2], dm64[:, :2])
    check("warp d_scale", m.grad[:, 2:], dm32[:, 2:], dm64[:, 2:])
    check("warp d_volume", v.grad, dv32, dv64)
    # the residual output's gradient is the prediction's, negated; without a volume gradient only d_motion runs
    m2 = motion.to(cuda).requires_grad_(True)
    _, r2 = ScaleSpaceWarpFn.apply(vol.to(cuda), m2, x_cur.to(cuda))
    r2.backward(-gout.to(cuda))
    assert torch.equal(m2.grad, m.grad)
    single = ScaleSpaceWarpFn.apply(vol.to(cuda), motion.to(cuda))
    assert torch.equal(single, x_pred)


# ---------------------------------------------------------------------------------------------- volume

VOLUME_CASES = [(16, 16, 1.5), (16, 48, 1.5), (32, 16, 1.5), (128, 256, 1.5), (32, 48, 0.5)]


def _volume_ref(x, gvol, sigma, levels, dtype):
    xx = x.clone().to(dtype).requires_grad_(True)
    vol = R.gaussian_volume(xx, sigma, levels)
    vol.backward(gvol.to(dtype))
    return vol.detach(), xx.grad


@pytest.mark.parametrize("H,W,sigma", VOLUME_CASES)
def test_volume_forward_and_backward_against_fp64(cuda, H, W, sigma):
    from compressai._ops import ScaleSpaceVolumeFn

    g = torch.Generator().manual_seed(H * W)
    N, C, L = 2, 3, 5
    x = torch.rand(N, C, H, W, generator=g)
    gvol = torch.randn(N, C, L + 1, H, W, generator=g)
    v64, dx64 = _volume_ref(x, gvol, sigma, L, torch.float64)
    v32, dx32 = _volume_ref(x, gvol, sigma, L, torch.float32)
    assert torch.equal(v32[:, :, 0], x)
    xc = x.to(cuda).requires_grad_(True)
    vol = ScaleSpaceVolumeFn.apply(xc, sigma, L)
    assert vol.shape == (N, C, L + 1, H, W) and vol.dtype == torch.float32
    assert torch.equal(vol[:, :, 0].cpu(), x)
    vol.backward(gvol.to(cuda))
    check("volume fwd", vol[:, :, 1:], v32[:, :, 1:], v64[:, :, 1:])
    check("volume bwd", xc.grad, dx32, dx64)


def test_volume_adjoint_identity_on_integers(cuda):
    """<volume(x), g> = <x, volume_bwd(g)>.  Each side is a sum of n products whose factors carry elementwise errors
    of at most the bars of the test above (4 x e_ref); such errors do not line up with the other factor's signs, so
    the sum is off by about (elementwise bar) x (the other factor's L2 norm), not its L1 norm."""
    from compressai._ops import ScaleSpaceVolumeFn

    gen = torch.Generator().manual_seed(7)
    N, C, L, H, W = 1, 2, 5, 32, 48
    x = torch.randint(-3, 4, (N, C, H, W), generator=gen).float()
    gvol = torch.randint(-3, 4, (N, C, L + 1, H, W), generator=gen).float()
    v64, dx64 = _volume_ref(x, gvol, 1.5, L, torch.float64)
    v32, dx32 = _volume_ref(x, gvol, 1.5, L, torch.float32)
    xc = x.to(cuda).requires_grad_(True)
    vol = ScaleSpaceVolumeFn.apply(xc, 1.5, L)
    vol.backward(gvol.to(cuda))
    lhs = (vol.detach().double().cpu() * gvol.double()).sum().item()
    rhs = (x.double() * xc.grad.double().cpu()).sum().item()
    bar = MARGIN * (maxerr(v32, v64) * gvol.norm().item() + maxerr(dx32, dx64) * x.norm().item())
    print(f"\nadjoint: lhs {lhs:.9g} rhs {rhs:.9g} diff {abs(lhs - rhs):.3e} bar {bar:.3e}")
    assert abs(lhs - rhs) <= bar


def test_gaussian_blur_helper_is_level_one(cuda):
    from compressai.models.utils import gaussian_blur, gaussian_kernel2d

    x = torch.rand(1, 3, 16, 24, generator=torch.Generator().manual_seed(3))
    k64 = R.gaussian_kernel2d(11, 1.5, torch.device("cpu"), torch.float64)
    ref64, ref32 = R.gaussian_blur(x.double(), k64), R.gaussian_blur(x, k64.float())
    check("blur(sigma)", gaussian_blur(x.to(cuda), kernel_size=11, sigma=1.5), ref32, ref64)
    check("blur(kernel)", gaussian_blur(x.to(cuda), kernel=gaussian_kernel2d(11, 1.5, cuda, torch.float32)), ref32,
          ref64)
    with pytest.raises(ValueError):
        gaussian_blur(x.to(cuda), kernel=torch.ones(3, 3, device=cuda) / 9)


# ----------------------------------------------------------------------------------------------- QReLU

LADDER = [-300.0, -1.0, -1e-3, 0.0, 0.5, 255.0, 255.0 + 1e-3, 256.0, 600.0]


@pytest.mark.parametrize("C", [12, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_qrelu_ladder(cuda, dtype, C):
    from compressai.layers import QReLU

    gen = torch.Generator().manual_seed(C)
    n = 2 * C * 3 * 3
    x = torch.tensor(LADDER).repeat(n // len(LADDER) + 1)[:n].reshape(2, C, 3, 3).to(dtype)
    gout = torch.randn(2, C, 3, 3, generator=gen).to(dtype)

    def ref(dt):
        xx = x.clone().to(dt).requires_grad_(True)
        y = R.QReLU.apply(xx, 8, 100)
        y.backward(gout.to(dt))
        return y.detach(), xx.grad

    y64, g64 = ref(torch.float64)
    _, gref = ref(dtype)
    xc = x.to(cuda).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        y = QReLU.apply(xc, 8, 100)
    assert y.dtype == dtype
    assert torch.equal(y.cpu(), x.clamp(0, 255))
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        y.backward(gout.to(cuda))
    assert torch.isfinite(xc.grad).all()
    check(f"qrelu bwd {dtype}", xc.grad, gref, g64)
    if dtype == torch.bfloat16:
        # the bf16 CPU restatement rounds u = 2 x / max - 1 itself (256 -> u = 1), so its error is no measure of a
        # kernel that computes in fp32: one rounding of an fp32-accurate value is 2^-9 relative, margin 2
        assert maxerr(xc.grad, g64) <= 2.0 ** -8 * g64.abs().max().item()


def test_quantize_ste(cuda):
    from compressai.models.utils import quantize_ste

    x = (torch.randn(2, 8, 4, 4, generator=torch.Generator().manual_seed(1)) * 3).to(cuda).requires_grad_(True)
    y = quantize_ste(x)
    assert torch.equal(y, torch.round(x.detach()))
    g = torch.randn_like(y)
    y.backward(g)
    assert torch.equal(x.grad, g)


# ------------------------------------------------------------------------------------------- arguments

def test_bad_arguments(cuda):
    from compressai._ops import ScaleSpaceVolumeFn, ScaleSpaceWarpFn

    with pytest.raises(ValueError, match="multiples of"):
        ScaleSpaceVolumeFn.apply(torch.zeros(1, 3, 24, 32, device=cuda), 1.5, 5)
    with pytest.raises(ValueError, match="taps"):
        ScaleSpaceVolumeFn.apply(torch.zeros(1, 3, 32, 32, device=cuda), 6.0, 5)
    with pytest.raises(ValueError, match="GPU tensors only"):
        ScaleSpaceVolumeFn.apply(torch.zeros(1, 3, 32, 32), 1.5, 5)
    with pytest.raises(ValueError, match="GPU tensors only"):
        ScaleSpaceWarpFn.apply(torch.zeros(1, 3, 6, 16, 16, device=cuda), torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="motion_info"):
        ScaleSpaceWarpFn.apply(torch.zeros(1, 3, 6, 16, 16, device=cuda), torch.zeros(1, 2, 16, 16, device=cuda))
    with pytest.raises(ValueError, match="dimensions"):
        ScaleSpaceWarpFn.apply(torch.zeros(1, 3, 16, 16, device=cuda), torch.zeros(1, 3, 16, 16, device=cuda))
