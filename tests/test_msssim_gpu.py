"""MS-SSIM as a HIP op (csrc/msssim.hip, _ops.MsSsimFn) against the torch body of metrics.ms_ssim in fp64.

Oracle: compressai.utils.metrics._ms_ssim_torch run in fp64 on the CPU, with autograd.  Yardstick e32: the error
of the same body run in fp32 on the CPU against the fp64 result, computed here (value: largest relative error of a
plane; gradient: relative L2 error).  Bars: value (per plane and mean) within 4 * e32 + 1e-6 relative (the factor 4
for the different summation order, tiled tree against torch's; the floor is ~16 fp32 ulps of a value near 1),
gradient within 4 * e32_grad relative L2.

Shapes: 161 is odd at every scale (every pooling step pads; scale 4 is an 11 x 11 plane with one output), 200
pads only at the fourth pooling, 176 x 163 mixes the two, 256^2 is the training patch.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [((2, 3, 161, 200), 0.05), ((1, 1, 176, 163), 0.2), ((2, 3, 256, 256), 0.02)]


def _images(b, c, h, w, noise, seed=0):
    """The generator of test_eval_gpu.py::_write_images per plane (k: channel, n: image), and a noisy copy."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([[np.sin(xx / (7 + k + 3 * n) + yy / (11 + 2 * k)) * 0.35 + 0.5 for k in range(c)]
                     for n in range(b)])
    x = np.clip(base + rng.normal(0, 0.05, base.shape), 0, 1)
    y = np.clip(x + rng.normal(0, noise, base.shape), 0, 1)
    return torch.tensor(x, dtype=torch.float32), torch.tensor(y, dtype=torch.float32)


def _torch_ref(x, y, dtype):
    from compressai.utils.metrics import _ms_ssim_torch

    xx = x.clone().to(dtype).requires_grad_(True)
    v = _ms_ssim_torch(xx, y, 1.0, dtype=dtype)
    v.mean().backward()
    return v.detach().double(), xx.grad.double()


_REF = {}


def _case(i):
    """x, y, the fp64 oracle (per-plane values, gradient of their mean) and e32 of case i; computed once."""
    if i not in _REF:
        shape, noise = CASES[i]
        x, y = _images(*shape, noise)
        v64, g64 = _torch_ref(x, y, torch.float64)
        v32, g32 = _torch_ref(x, y, torch.float32)
        e32 = ((v32 - v64).abs() / v64).max().item()
        e32g = ((g32 - g64).norm() / g64.norm()).item()
        _REF[i] = (x, y, v64, g64, e32, e32g)
    return _REF[i]


def _run(x, y, cuda, upstream=None, which="mean"):
    from compressai._ops import MsSsimFn

    xd = x.to(cuda).requires_grad_(True)
    mean, planes = MsSsimFn.apply(xd, y.to(cuda), 1.0)
    out = mean if which == "mean" else planes.mean()
    if upstream is not None:
        out = out * upstream
    out.backward()
    return mean.detach(), planes.detach(), xd.grad


@pytest.mark.parametrize("i", range(len(CASES)))
def test_value(cuda, i):
    x, y, v64, _, e32, _ = _case(i)
    mean, planes, _ = _run(x, y, cuda)
    bar = 4 * e32 + 1e-6
    err = ((planes.double().cpu() - v64).abs() / v64).max().item()
    m64 = v64.mean().item()
    err_mean = abs(mean.double().item() - m64) / m64
    print(f"case {CASES[i]}: e32 {e32:.3e} bar {bar:.3e} per-plane err {err:.3e} mean err {err_mean:.3e}")
    assert err <= bar, (err, bar)
    assert err_mean <= bar, (err_mean, bar)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_gradient(cuda, i):
    """Measured on an MI355X (relative L2 against fp64 autograd; bar 4 * e32_grad): see DESIGN.md section 6."""
    x, y, _, g64, _, e32g = _case(i)
    bar = 4 * e32g
    n64 = g64.norm()
    for which in ("mean", "planes"):
        _, _, g = _run(x, y, cuda, which=which)
        assert g.dtype == torch.float32 and g.shape == x.shape
        err = ((g.double().cpu() - g64).norm() / n64).item()
        print(f"case {CASES[i]} via {which}: e32_grad {e32g:.3e} bar {bar:.3e} err {err:.3e}")
        assert err <= bar, (which, err, bar)
    r = float(torch.empty(1).uniform_(0.5, 2.0, generator=torch.Generator().manual_seed(i)).item())
    up = torch.tensor(-r, device=cuda)
    _, _, g = _run(x, y, cuda, upstream=up)
    err = ((g.double().cpu() - (-r) * g64).norm() / (r * n64)).item()
    print(f"case {CASES[i]} upstream {-r:.4f}: err {err:.3e}")
    assert err <= bar, (err, bar)


def test_relu_plane(cuda):
    """y = 1 - x on plane 1: its contrast terms are negative, the ReLU clamps, the per-plane values are [1, 0]
    (fp64 torch agrees) and autograd's gradient there is exactly 0, not NaN."""
    x, _ = _images(1, 2, 161, 161, 0.0)
    y = x.clone()
    y[:, 1] = 1 - x[:, 1]
    mean, planes, g = _run(x, y, cuda)
    assert abs(planes[0, 0].item() - 1.0) <= 1e-6
    assert planes[0, 1].item() == 0.0
    assert abs(mean.item() - 0.5) <= 1e-6
    assert torch.isfinite(g).all()
    assert (g[:, 1] == 0).all()


def test_reproducible_and_graph(cuda):
    from compressai._ops import MsSsimFn

    x, y, _, _, _, _ = _case(0)
    m1, p1, g1 = _run(x, y, cuda)
    m2, p2, g2 = _run(x, y, cuda)
    assert torch.equal(m1, m2) and torch.equal(p1, p2) and torch.equal(g1, g2)

    xs = x.to(cuda).requires_grad_(True)
    ys = y.to(cuda)

    def fwd_bwd():
        mean, planes = MsSsimFn.apply(xs, ys, 1.0)
        (g,) = torch.autograd.grad(mean, xs)
        return mean, planes, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mean, planes, g = fwd_bwd()
    for _ in range(2):
        mean.detach().zero_()
        planes.detach().zero_()
        g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mean.detach(), m1) and torch.equal(planes.detach(), p1) and torch.equal(g, g1)


def test_bf16_input(cuda):
    x, y, _, _, _, _ = _case(1)
    xb = x.to(torch.bfloat16)
    mean_b, planes_b, g_b = _run(xb, y, cuda)
    assert g_b.dtype == torch.bfloat16 and g_b.shape == x.shape
    mean_f, planes_f, g_f = _run(xb.float(), y, cuda)
    assert torch.equal(mean_b, mean_f) and torch.equal(planes_b, planes_f)
    assert torch.equal(g_b, g_f.to(torch.bfloat16))


def _kinds(fn):
    from compressai import _ledger

    with _ledger.recording(keep_replay=False) as led:
        out = fn()
    torch.cuda.synchronize()
    return out, [e.kind for e in led.entries]


def test_dispatch(cuda, monkeypatch):
    from compressai._ops import MsSsimFn
    from compressai.utils import metrics

    x, y, v64, _, e32, _ = _case(1)
    xd, yd = x.to(cuda), y.to(cuda)
    monkeypatch.delenv("CAI_MSSSIM_TORCH", raising=False)
    v, kinds = _kinds(lambda: metrics.ms_ssim(xd, yd, data_range=1.0))
    assert "msssim_fwd" in kinds
    assert v.dim() == 0 and abs(v.item() - v64.mean().item()) <= (4 * e32 + 1e-6) * v64.mean().item()
    # another window is the torch body's
    _, kinds = _kinds(lambda: metrics.ms_ssim(xd, yd, win_sigma=1.0))
    assert "msssim_fwd" not in kinds
    # the gradient of a second argument comes through the swap
    yg = yd.clone().requires_grad_(True)
    v2, kinds = _kinds(lambda: metrics.ms_ssim(xd, yg))
    assert "msssim_fwd" in kinds
    v2.backward()
    yr = yd.clone().requires_grad_(True)
    MsSsimFn.apply(yr, xd, 1.0)[0].backward()
    assert yg.grad is not None and torch.equal(yg.grad, yr.grad) and yg.grad.abs().max().item() > 0
    # both arguments: torch autograd
    _, kinds = _kinds(lambda: metrics.ms_ssim(xd.clone().requires_grad_(True), yg))
    assert "msssim_fwd" not in kinds
    monkeypatch.setenv("CAI_MSSSIM_TORCH", "1")
    vt, kinds = _kinds(lambda: metrics.ms_ssim(xd, yd, data_range=1.0))
    assert "msssim_fwd" not in kinds
    assert abs(vt.item() - v.item()) <= 1e-5


def test_loss(cuda):
    """RateDistortionLoss(metric="ms-ssim") on ScaleHyperprior(32, 48) with the oracle's weights and noise, as
    smoke() does for MSE: against the oracle model's output put through the fp32 torch MS-SSIM and its bpp."""
    import cai_oracle as O
    from compressai.entropy_models import set_noise_source
    from compressai.losses import RateDistortionLoss
    from compressai.models import ScaleHyperprior
    from compressai.utils.metrics import _ms_ssim_torch

    lmbda = 64.0
    torch.manual_seed(0)
    ref = O.ScaleHyperprior(32, 48)
    net = ScaleHyperprior(32, 48)
    net.load_state_dict(ref.state_dict())
    net = net.to(cuda)
    x = torch.rand(2, 3, 192, 192, generator=torch.Generator().manual_seed(0))
    noises = [torch.empty(2, 32, 3, 3).uniform_(-0.5, 0.5), torch.empty(2, 48, 12, 12).uniform_(-0.5, 0.5)]
    with O.NoiseFeed(list(noises)):
        out_r = ref(x)
    want = {"bpp_loss": O.RateDistortionLoss(3)(out_r, x)["bpp_loss"],
            "ms_ssim_loss": _ms_ssim_torch(out_r["x_hat"], x, 1.0).mean()}
    want["loss"] = lmbda * (1 - want["ms_ssim_loss"]) + want["bpp_loss"]
    want["loss"].backward()
    q = [n.to(cuda) for n in noises]
    set_noise_source(lambda t: q.pop(0))
    try:
        out = net(x.to(cuda))
    finally:
        set_noise_source(None)
    crit = RateDistortionLoss(3, metric="ms-ssim", lmbda=lmbda)(out, x.to(cuda))
    assert set(crit) == {"loss", "bpp_loss", "ms_ssim_loss"}
    crit["loss"].backward()
    torch.cuda.synchronize()
    for k, b in want.items():
        a, b = crit[k].item(), b.item()
        print(f"{k}: {a} vs oracle {b}")
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (k, a, b)
    ga = net.g_a[0].weight.grad.cpu()
    gr = ref.g_a[0].weight.grad
    err = (ga - gr).abs().max().item() / gr.abs().max().item()
    print(f"g_a.0.weight grad max-relative error {err:.3e}")
    assert err <= 1e-3, err
    with torch.no_grad():
        assert set(RateDistortionLoss(3)(out, x.to(cuda))) == {"loss", "bpp_loss", "mse_loss"}
