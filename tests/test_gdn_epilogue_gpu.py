"""The forward GDN / IGDN run inside the kernels of the conv that produces its input (cai_conv_gdn_fwd,
_ops.GdnEpilogue) against the two-launch path, on the same inputs and weights in one process.

The fused forms follow the recipe that makes gdn_fwd_lane_kernel bit-identical to gdn_fwd_kernel (csrc/gdn_tile.hpp),
and the conv part keeps the arithmetic of the kernels it replaces, so every comparison here is torch.equal: the
conv's output x, y = GDN(x), and after a backward from a fixed upstream gradient the input gradient, the conv's
weight and bias gradients, dgamma and dbeta (the backward kernels are the same in both paths and read x).

Hosts and the shapes that reach them with their edge cases:
* edge_s2d_kernel's GDN variant (Conv 3->128 k5 s2 straight from the NCHW fp32 image, which takes no input
  gradient): B=2 and B=1 on 3 x 136 x 200 -> 68 x 100, one full and one ragged 64-pixel column block, fewer tiles
  than persistent blocks (one tile per block), and B=2 on 3 x 800 x 200 -> 1600 tiles on 768 blocks, so blocks
  run several tiles through the same LDS images;
* conv_halo_kernel<5>, no split (>= 256 tiles of 8 x 32): Conv 128->128 k5 s2, output 1 x 60 x 1100 = 8 x 35 tiles,
  the last tile row and the last tile column ragged;
* conv_halo_phase_kernel<128>, no split: ConvTranspose 128->128 k5 s2 + IGDN, 60 x 500 per phase = 4 x 128 blocks,
  ragged rows and columns;
* the split-K reduce: Conv 128->128 k5 s2 at B=2 to 32 x 32 (conv_halo_kernel<5>, 4 splits) and to 31 x 33 (rows
  that are no multiple of the 16-row tile), ConvTranspose 256->128 k5 s2 + IGDN 32^2 -> 64^2 (phase kernel, 4
  splits) and ConvTranspose 128->128 k5 s2 p2 without output padding 23^2 -> 45^2 (four phases of different sizes,
  conv_glds_kernel split).
The 192->128 ConvTranspose at 16^2 -> 32^2 (g_s.0 of the hyperprior) never splits K -- conv_small_kernel at small
batches, conv_glds_kernel<64x128> with one split at B=16 -- so it has no host: it is a fallback case here.
Fallbacks (C = 192, fp32, an activation between conv and GDN, the switch off, evaluation under no_grad) must run
the standalone GDN kernels with unchanged results.

gamma / beta are perturbed from their initial values (gamma starts as 0.1 I, which would hide a permuted row).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _perturb(mods, seed):
    """A few random steps on every parameter (the GDN's raw gamma becomes a dense matrix)."""
    from compressai.layers import GDN

    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                scale = 0.03 if isinstance(m, GDN) else 0.1 * p.abs().max().item()
                for _ in range(3):
                    p.add_(scale * torch.randn(p.shape, generator=gen))


def _layers(kind, cin, cout, inverse, seed, dev):
    from compressai.layers import GDN, Conv2d, ConvTranspose2d

    torch.manual_seed(seed)
    if kind == "conv":
        conv = Conv2d(cin, cout, kernel_size=5, stride=2, padding=2)
    else:
        conv = ConvTranspose2d(cin, cout, kernel_size=5, stride=2, padding=2, output_padding=1 if kind == "deconv" else 0)
    gdn = GDN(cout, inverse=inverse)
    _perturb([conv, gdn], seed + 1)
    return conv.to(dev), gdn.to(dev)


def _step(conv, gdn, x, gy_seed, fused, bf16=True, mid=None, input_grad=True):
    """conv -> [mid] -> gdn through layers.Sequential, forward and backward, under the ledger.  Returns the tensors
    compared between the two paths and the ledger entries."""
    from compressai import _ledger, _ops
    from compressai.layers import Sequential

    seq = Sequential(*([conv] + ([mid] if mid is not None else []) + [gdn]))
    for p in seq.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(input_grad)   # the image-side edge kernels run only without an input gradient
    old = _ops.GDN_EPI
    _ops.GDN_EPI = fused
    try:
        with _ledger.recording(keep_replay=False) as led:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                y = seq(xin)
            # the conv's output is what the GDN node saved for its backward
            xo = y.grad_fn.saved_tensors[0].detach().clone() if mid is None else None
            gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gy_seed)).to(y.device)
            y.backward(gy)
            torch.cuda.synchronize()
    finally:
        _ops.GDN_EPI = old
    out = {"y": y.detach(), "dw": conv.weight.grad, "db": conv.bias.grad, "dgamma": gdn.gamma.grad,
           "dbeta": gdn.beta.grad}
    if xo is not None:
        out["x"] = xo
    if input_grad:
        out["dx"] = xin.grad
    return {k: v.clone() for k, v in out.items()}, led.entries


def _fwd_entries(entries):
    conv = [e for e in entries if e.kind == "conv_fwd"]
    gdn = [e for e in entries if e.kind == "gdn_fwd"]
    return conv, gdn


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), (k, (a[k].float() - b[k].float()).abs().max().item())


def _query(conv, x, inverse):
    from compressai import _native, _ops

    cout = conv.out_channels
    g = _ops.conv_geom(conv._spec(), x.shape[0], x.shape[1], x.shape[2], x.shape[3], cout)
    host = _native.lib.cai_conv_gdn_fused(ctypes.byref(g), _native.BF16, 0)
    name = _native.lib.cai_conv_gdn_kernel_name(ctypes.byref(g), _native.BF16, 0, int(inverse)).decode()
    ks = _native.lib.cai_conv_split_factor(ctypes.byref(g), _native.BF16, 0, 0)
    return host, name, ks


HALO, PHASE, REDUCE = 1, 2, 3

FUSED_CASES = [
    # id, kind, B, cin, H, W, inverse, host, kernel that runs the GDN, splits
    ("halo-ragged", "conv", 1, 128, 120, 2200, False, HALO, "conv_halo_kernel<5,gdn>", 1),
    ("phase-ragged", "deconv", 1, 128, 60, 500, True, PHASE, "conv_halo_phase_gdn_kernel<igdn>", 1),
    ("splitk-halo-32", "conv", 2, 128, 64, 64, False, REDUCE, "conv_splitk_reduce_gdn_kernel<gdn>", 4),
    ("splitk-halo-31x33", "conv", 2, 128, 62, 66, False, REDUCE, "conv_splitk_reduce_gdn_kernel<gdn>", 4),
    ("splitk-phase-256", "deconv", 2, 256, 32, 32, True, REDUCE, "conv_splitk_reduce_gdn_kernel<igdn>", 4),
    ("splitk-glds-odd-phases", "deconv-op0", 2, 128, 23, 23, True, REDUCE, "conv_splitk_reduce_gdn_kernel<igdn>", None),
]


@pytest.mark.parametrize("case", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_fused_equals_unfused(cuda, case):
    _, kind, B, cin, H, W, inverse, host, kernel, splits = case
    conv, gdn = _layers(kind, cin, 128, inverse, 7, cuda)
    x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(11)).to(cuda)
    q_host, q_name, q_ks = _query(conv, x, inverse)
    assert (q_host, q_name) == (host, kernel)
    assert q_ks == splits if splits is not None else q_ks > 1
    fused, ent_f = _step(conv, gdn, x, 13, True)
    plain, ent_p = _step(conv, gdn, x, 13, False)
    conv_f, gdn_f = _fwd_entries(ent_f)
    conv_p, gdn_p = _fwd_entries(ent_p)
    tag = " +IGDN" if inverse else " +GDN"
    # the fused step: one conv launch marked with the fusion, no standalone GDN; the plain step: both
    assert len(conv_f) == 1 and conv_f[0].shape.endswith(tag) and not gdn_f, [(e.kernel, e.shape) for e in ent_f]
    assert len(conv_p) == 1 and not conv_p[0].shape.endswith(tag) and len(gdn_p) == 1
    assert conv_f[0].kernel == conv_p[0].kernel                      # the host keeps its ledger label
    npix, C = fused["y"].shape[0] * fused["y"].shape[2] * fused["y"].shape[3], 128
    assert conv_f[0].flops == conv_p[0].flops + gdn_p[0].flops
    assert conv_f[0].nbytes == conv_p[0].nbytes + gdn_p[0].nbytes - 2 * npix * C   # minus the read of x
    assert float(fused["y"].float().abs().max()) > 0
    _assert_same(fused, plain)


@pytest.mark.parametrize("B,H,W", [(2, 136, 200), (1, 136, 200), (2, 800, 200)],
                         ids=["B2-ragged-column-block", "B1-one-tile-per-block", "B2-several-tiles-per-block"])
def test_edge_host_fused_equals_unfused(cuda, B, H, W):
    from compressai import _native, _ops

    conv, gdn = _layers("conv", 3, 128, False, 17, cuda)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(21)).to(cuda)
    g = _ops.conv_geom(conv._spec(), B, 3, H, W, 128)
    assert _native.lib.cai_edge_conv_gdn_fused(ctypes.byref(g)) == 1
    fused, ent_f = _step(conv, gdn, x, 23, True, input_grad=False)
    plain, ent_p = _step(conv, gdn, x, 23, False, input_grad=False)
    conv_f, gdn_f = _fwd_entries(ent_f)
    conv_p, gdn_p = _fwd_entries(ent_p)
    assert len(conv_f) == 1 and conv_f[0].shape.endswith(" +GDN") and not gdn_f, [(e.kernel, e.shape) for e in ent_f]
    assert len(conv_p) == 1 and "GDN" not in conv_p[0].shape and len(gdn_p) == 1
    assert conv_f[0].kernel == conv_p[0].kernel == "edge_s2d_kernel (conv fwd)"
    npix = B * (H // 2) * (W // 2)
    assert conv_f[0].flops == conv_p[0].flops + gdn_p[0].flops
    assert conv_f[0].nbytes == conv_p[0].nbytes + gdn_p[0].nbytes - 2 * npix * 128
    assert "x" in fused and float(fused["y"].float().abs().max()) > 0
    _assert_same(fused, plain)


FALLBACK_CASES = [
    # id, kind, B, cin, cout, H, W, inverse, bf16, LeakyReLU between
    ("c192", "conv", 2, 192, 192, 64, 64, False, True, False),
    ("fp32", "conv", 2, 128, 128, 64, 64, False, False, False),
    ("leaky-relu", "conv", 2, 128, 128, 64, 64, False, True, True),
    ("gs0-deconv-no-split", "deconv", 2, 192, 128, 16, 16, True, True, False),
]


@pytest.mark.parametrize("case", FALLBACK_CASES, ids=[c[0] for c in FALLBACK_CASES])
def test_fallbacks_run_the_unfused_kernels(cuda, case):
    _, kind, B, cin, cout, H, W, inverse, bf16, leaky = case
    from compressai.layers import GDN, Conv2d, ConvTranspose2d

    torch.manual_seed(5)
    cls = Conv2d if kind == "conv" else ConvTranspose2d
    kw = dict(kernel_size=5, stride=2, padding=2)
    if kind != "conv":
        kw["output_padding"] = 1
    conv, gdn = cls(cin, cout, **kw), GDN(cout, inverse=inverse)
    _perturb([conv, gdn], 6)
    conv, gdn = conv.to(cuda), gdn.to(cuda)
    mid = torch.nn.LeakyReLU(0.01) if leaky else None
    x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(12)).to(cuda)
    on, ent_on = _step(conv, gdn, x, 14, True, bf16=bf16, mid=mid)
    off, ent_off = _step(conv, gdn, x, 14, False, bf16=bf16, mid=mid)
    for ent in (ent_on, ent_off):
        conv_e, gdn_e = _fwd_entries(ent)
        assert len(conv_e) == 1 and "GDN" not in conv_e[0].shape
        assert len(gdn_e) == 1 and gdn_e[0].kernel.startswith("gdn_fwd")
    assert [(e.kind, e.kernel, e.shape) for e in ent_on] == [(e.kind, e.kernel, e.shape) for e in ent_off]
    _assert_same(on, off)


def test_switch_off_and_no_grad_take_the_unfused_path(cuda):
    """With the switch off, and in evaluation under no_grad with it on, a fusable pair launches conv + GDN; the
    outputs equal the fused training forward's."""
    from compressai import _ledger, _ops
    from compressai.layers import Sequential

    conv, gdn = _layers("conv", 128, 128, False, 7, cuda)
    x = torch.randn(2, 128, 64, 64, generator=torch.Generator().manual_seed(11)).to(cuda)
    fused, ent = _step(conv, gdn, x, 13, True)
    assert not _fwd_entries(ent)[1]
    seq = Sequential(conv, gdn)
    assert _ops.GDN_EPI, "the switch defaults to on"
    with _ledger.recording(keep_replay=False) as led, torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = seq(x)
        torch.cuda.synchronize()
    conv_e, gdn_e = _fwd_entries(led.entries)
    assert len(conv_e) == 1 and "GDN" not in conv_e[0].shape and len(gdn_e) == 1
    assert torch.equal(y, fused["y"])


def test_unfusable_call_is_an_error(cuda):
    """cai_conv_gdn_fwd on a geometry without a host fails with a message (no silent fallback)."""
    from compressai import _native, _ops

    spec = _ops.ConvSpec(5, 2, 2, 1, True)
    g = _ops.conv_geom(spec, 2, 192, 16, 16, 128)
    assert _native.lib.cai_conv_gdn_fused(ctypes.byref(g), _native.BF16, 0) == 0
    assert _native.lib.cai_conv_gdn_kernel_name(ctypes.byref(g), _native.BF16, 0, 1) == b""
    t = torch.zeros(1 << 20, dtype=torch.bfloat16, device=cuda)
    p = ctypes.c_void_p(t.data_ptr())
    with pytest.raises(ValueError, match="no kernel runs the GDN"):
        _native.lib.cai_conv_gdn_fwd(ctypes.byref(g), _native.BF16, p, 192, 0, p, None, p, 32 * 32 * 128, 1, 32 * 128,
                                     128, p, p, 1, p, 128, p, t.numel() * 2, None)


def _model_step(net, x, noise, fused):
    from compressai import _ledger, _ops
    from compressai.entropy_models import set_noise_source
    from compressai.losses import RateDistortionLoss

    for p in net.parameters():
        p.grad = None
    old = _ops.GDN_EPI
    _ops.GDN_EPI = fused
    set_noise_source(lambda t: noise[tuple(t.shape)])
    try:
        with _ledger.recording(keep_replay=False) as led:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = net(x)
                c = RateDistortionLoss(1)(out, x)
            c["loss"].backward()
            torch.cuda.synchronize()
    finally:
        set_noise_source(None)
        _ops.GDN_EPI = old
    res = {"x_hat": out["x_hat"].detach().clone(), "loss": c["loss"].detach().clone()}
    for k, v in out["likelihoods"].items():
        res["lik_" + k] = v.detach().clone()
    for n, p in net.named_parameters():
        if p.grad is not None:
            res["grad_" + n] = p.grad.detach().clone()
    return res, led.entries


def test_hyperprior_step_fused_equals_unfused(cuda):
    """bmshj2018-hyperprior (128, 192) at B=16 256^2, the bench's model: x_hat, likelihoods and every parameter
    gradient equal with and without the fusion.  The fused step's standalone forward GDN launches are exactly the
    layers no host covers: g_s.5 after the four-phase kernel (gdn_fwd_lane_kernel<128>, which the production-mix
    test asserts) and g_s.1, whose 192->128 deconv does not split K at B=16 (conv_glds_kernel<64x128>, one split),
    so the split-K host does not see it."""
    from compressai.zoo import model_architectures

    torch.manual_seed(0)
    net = model_architectures["bmshj2018-hyperprior"](128, 192)
    _perturb([m for m in net.modules() if type(m).__name__ == "GDN"], 3)
    net = net.to(cuda)
    gen = torch.Generator().manual_seed(41)
    x = torch.rand(16, 3, 256, 256, generator=gen).to(cuda)
    noise = {s: (torch.rand(s, generator=gen) - 0.5).to(cuda) for s in ((16, 128, 4, 4), (16, 192, 16, 16))}
    fused, ent_f = _model_step(net, x, noise, True)
    plain, ent_p = _model_step(net, x, noise, False)
    assert any(k.startswith("grad_g_a.1.gamma") for k in fused) and len(fused) > 30
    _assert_same(fused, plain)
    npx = {32: 16 * 32 * 32, 64: 16 * 64 * 64, 128: 16 * 128 * 128}
    standalone = sorted((e.kernel, e.shape) for e in ent_f if e.kind == "gdn_fwd")
    assert standalone == sorted([
        ("gdn_fwd_kernel<128>", f"IGDN C=128 npix={npx[32]}"),          # g_s.1
        ("gdn_fwd_lane_kernel<128>", f"IGDN C=128 npix={npx[128]}"),    # g_s.5, after conv_halo_quad_kernel
    ]), standalone
    assert len([e for e in ent_p if e.kind == "gdn_fwd"]) == 6
    marked = sorted(e.shape for e in ent_f if e.kind == "conv_fwd" and "GDN" in e.shape)
    assert len(marked) == 4 and len(ent_f) == len(ent_p) - 4, marked
