"""Checkerboard context models on the GPU: the parity kernels (exact), the two-pass coding at the latent level
(bit-identical decoder, byte-identical streams, teacher-forced parity with the plain-torch restatement), and the
models (round trips, the multi-modal pair through the container, training forward + backward)."""
import copy
import math
import warnings

import pytest
import torch

import cai_oracle as O
import ckbd_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 1, 1), (2, 40, 3, 5), (1, 192, 4, 6)]
CODING_SHAPES = SHAPES + [(2, 32, 2, 1), (1, 32, 1, 2)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _parity_mask(H, W, parity, dev):
    return (R.anchor_map(H, W) == bool(parity)).to(dev)


# ---- kernels, exact --------------------------------------------------------------------------------------------

def _check_parity_zero(x, parity, bf16):
    from compressai._ops import ParityZeroFn

    B, C, H, W = x.shape
    x = x.requires_grad_()
    g = torch.randn(B, C, H, W, generator=_gen(B + C), dtype=torch.float32).to(x.device, x.dtype)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        out = ParityZeroFn.apply(x, parity)
    out.backward(g)
    sel = _parity_mask(H, W, parity, x.device)
    want, gwant = x.detach().clone(), g.clone()
    want[..., sel] = 0
    gwant[..., sel] = 0
    assert out.dtype == x.dtype and out.shape == x.shape
    assert torch.equal(out.detach(), want) and torch.equal(x.grad, gwant)
    assert (out.detach()[..., sel] == 0).all() and not torch.signbit(out.detach()[..., sel]).any()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("parity", [0, 1])
def test_parity_zero_forward_and_backward(cuda, shape, bf16, parity):
    dt = torch.bfloat16 if bf16 else torch.float32
    x = torch.randn(*shape, generator=_gen(sum(shape))).to(cuda, dt)
    _check_parity_zero(x, parity, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_parity_zero_on_a_channel_half_view(cuda, bf16):
    from compressai._ops import empty_pm, pixel_major_ld

    dt = torch.bfloat16 if bf16 else torch.float32
    B, C, H, W = 2, 40, 3, 5
    buf = empty_pm(B, 2 * C, H, W, dt, cuda)
    buf.copy_(torch.randn(B, 2 * C, H, W, generator=_gen(9)))
    x = buf[:, C:].detach()
    assert pixel_major_ld(x) == 2 * C
    _check_parity_zero(x, 1, bf16)


def _coding_inputs(shape, cuda, seed):
    from compressai._ops import empty_pm
    from compressai.models.google import get_scale_table

    B, C, H, W = shape
    g = _gen(seed)
    y = 3 * torch.randn(B, C, H, W, generator=g)
    y.view(-1)[::7] *= 15                       # |y - mean| past the CDF tables' range: escapes of both signs
    y.view(-1)[3::11] = 5000.0
    y.view(-1)[5::11] = -5000.0
    sm = empty_pm(B, 2 * C, H, W, torch.float32, cuda)      # scales and means: the channel halves of one buffer
    sm.copy_(torch.cat((torch.exp(2 * torch.randn(B, C, H, W, generator=g)) - 0.3, torch.randn(B, C, H, W, generator=g)), 1))
    return y.to(cuda), sm[:, :C], sm[:, C:], get_scale_table().to(cuda), 0.11


@pytest.mark.parametrize("shape", CODING_SHAPES, ids=str)
@pytest.mark.parametrize("parity", [0, 1])
def test_ckbd_quantize_indexes_dequantize_exact(cuda, shape, parity):
    from compressai import _ops

    B, C, H, W = shape
    y, scales, means, table, bound = _coding_inputs(shape, cuda, 40 + H * W + C)
    if B * H * W > 1:       # a single pixel has no pitch
        assert _ops.pixel_major_ld(scales) == 2 * C and _ops.pixel_major_ld(means) == 2 * C
    n = H * W * C
    SENT, FSENT = -777, 123.25
    lo, hi = _ops.ckbd_slot_range(H, W, parity)
    own = torch.zeros(H * W, dtype=torch.bool)
    own[lo:hi] = True
    own = own.repeat_interleave(C).to(cuda)
    sel = _parity_mask(H, W, parity, cuda)
    assert int(sel.sum()) == hi - lo
    # what torch makes of the same scales / means tensors
    sym_map = torch.round(y - means).int()
    sym_want = R.to_coder_order(sym_map.cpu())
    idx_want = R.to_coder_order(R.build_indexes(scales.cpu(), table.cpu(), bound))
    yhat_want = sym_map.float() + means
    assert (sym_map.abs() > 200).any()

    def fresh():
        y_hat = torch.full((B, H, W, C), FSENT, device=cuda).permute(0, 3, 1, 2)
        return y_hat, torch.full((B, n), SENT, dtype=torch.int32, device=cuda), torch.full((B, n), SENT, dtype=torch.int32, device=cuda)

    y_hat, symbols, indexes = fresh()
    _ops.ckbd_quantize(y, scales, means, table, bound, parity, y_hat, symbols, indexes)
    for got, want in ((symbols, sym_want), (indexes, idx_want)):
        assert torch.equal(got[:, own].cpu(), want[:, own.cpu()])
        assert (got[:, ~own] == SENT).all()
    assert torch.equal(y_hat[..., sel], yhat_want[..., sel]) and (y_hat[..., ~sel] == FSENT).all()
    # the decoder's two kernels
    y_hat2, _, indexes2 = fresh()
    _ops.ckbd_indexes(scales, table, bound, parity, indexes2)
    assert torch.equal(indexes2, indexes)
    _ops.ckbd_dequantize(symbols, means, parity, y_hat2)
    assert torch.equal(y_hat2, y_hat)


# ---- coding at the latent level --------------------------------------------------------------------------------

def _jahp(cuda, N, M, seed, context="checkerboard"):
    from compressai.models import JointAutoregressiveHierarchicalPriors

    torch.manual_seed(seed)
    net = JointAutoregressiveHierarchicalPriors(N, M, context=context).to(cuda).eval()
    net.update()
    return net


@pytest.fixture(scope="module")
def net32(cuda):
    return _jahp(cuda, 32, 32, 21)


@pytest.fixture(scope="module")
def net192(cuda):
    return _jahp(cuda, 8, 192, 22)


def _synthetic(net, B, H, W, seed, cuda, amp=3.0):
    M = net.context_prediction.in_channels
    y = (amp * torch.randn(B, M, H, W, generator=_gen(seed))).to(cuda)
    params = torch.randn(B, 2 * M, H, W, generator=_gen(seed + 1)).to(cuda)
    return y, params


LATENTS = [(1, 1, 1), (2, 1, 2), (1, 2, 1), (2, 3, 5), (1, 4, 6)]


@pytest.mark.parametrize("B, H, W", LATENTS)
def test_latent_coding_round_trip_and_streams(cuda, net32, B, H, W):
    from compressai.ans import RansDecoder, RansEncoder

    gc = net32.gaussian_conditional
    y, params = _synthetic(net32, B, H, W, 100 + 10 * H + W, cuda)
    if H * W > 1:
        y[0, 3, 0, 0], y[-1, 7, H - 1, W - 1] = 5000.0, -40.0       # escapes in both groups' neighbourhood
    with torch.no_grad():
        e = net32._ckbd_encode(y, params, with_params=True)
        strings = net32._ar_encode_all(y, params)
        y_dec = net32._ar_decode_all(strings, params)
    assert strings == e["strings"] and all(isinstance(s, bytes) for s in strings)
    assert y_dec.shape == y.shape and torch.equal(y_dec, e["y_hat"])
    assert (e["y_hat"] - y).abs().max().item() <= 0.5 + 1e-3
    # the stream is the reference coder's on the anchors-then-non-anchors lists
    M = y.size(1)
    sym = R.to_coder_order(torch.round(y - e["means"]).int().cpu())
    idx = R.to_coder_order(gc.build_indexes(e["scales"]).cpu())
    assert torch.equal(e["symbols"].cpu(), sym) and torch.equal(e["indexes"].cpu(), idx)
    cdf, lens, offs = net32._gc_tables()
    n1 = (H * W // 2) * M
    for b in range(B):
        s, i = sym[b].tolist(), idx[b].tolist()
        assert RansEncoder().encode_with_indexes(s, i, cdf, lens, offs) == strings[b]
        dec = RansDecoder()
        dec.set_stream(strings[b])
        assert dec.decode_stream(i[:n1], cdf, lens, offs) + dec.decode_stream(i[n1:], cdf, lens, offs) == s


@pytest.mark.parametrize("which, B, H, W", [("net32", 2, 3, 5), ("net32", 1, 4, 6), ("net192", 1, 4, 4)])
def test_teacher_forced_parity(cuda, request, which, B, H, W):
    """The path's scales / means against the fp64 restatement given the path's own y_hat, within the fused
    coder's bar (1e-4 max(1, max|ref|), tests/test_ar_fused_gpu.py); the discrete steps exactly."""
    net = request.getfixturevalue(which)
    gc = net.gaussian_conditional
    y, params = _synthetic(net, B, H, W, 300 + H, cuda)
    with torch.no_grad():
        e = net._ckbd_encode(y, params, with_params=True)
    cw, cb, layers, slope = R.model_weights(net)
    scales_r, means_r = R.entropy_params(e["y_hat"].double().cpu(), params.double().cpu(), cw, cb, layers, slope)
    for name, got, ref in (("scales", e["scales"], scales_r), ("means", e["means"], means_r)):
        err = (got.double().cpu() - ref).abs().max().item()
        tol = 1e-4 * max(1.0, ref.abs().max().item())
        print(f"{which} {name}: max err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (name, err, tol)
    sym = torch.round(y - e["means"]).int()
    assert torch.equal(e["symbols"].cpu(), R.to_coder_order(sym.cpu()))
    assert torch.equal(e["y_hat"], sym.float() + e["means"])
    assert torch.equal(e["indexes"].cpu(), R.to_coder_order(gc.build_indexes(e["scales"]).cpu()))


def test_truncated_stream_is_a_value_error(cuda, net32):
    y, params = _synthetic(net32, 2, 3, 5, 500, cuda)
    with torch.no_grad():
        strings = net32._ar_encode_all(y, params)
        assert len(strings[1]) >= 16
        with pytest.raises(ValueError, match="truncated or corrupt stream|shorter than"):
            net32._ar_decode_all([strings[0], strings[1][:-8]], params)
        with pytest.raises(ValueError, match="multiple of 4"):
            net32._ar_decode_all([strings[0][:-2], strings[1]], params)


# ---- models ----------------------------------------------------------------------------------------------------

def _round_trip(net, x):
    from compressai._prepack import prepacked_forward

    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)          # no "not recommended on GPU" warning
        enc = net.compress(x)
        dec = net.decompress(enc["strings"], enc["shape"])
    assert net.compress(x)["strings"] == enc["strings"]
    with torch.no_grad(), prepacked_forward(net):
        y = net.g_a(x)
        params = net.h_s(net.entropy_bottleneck.decompress(enc["strings"][1], enc["shape"]))
        e = net._ckbd_encode(y, params)
        assert e["strings"] == enc["strings"][0]
        x_rec = net.g_s(e["y_hat"]).clamp_(0, 1)
    assert torch.equal(dec["x_hat"], x_rec)
    return enc


@pytest.mark.parametrize("size", [(64, 64), (64, 128)], ids=str)
def test_round_trip_small_jahp(cuda, size):
    net = _jahp(cuda, 32, 48, 5)
    net.ar_backend = "fused"                                 # not consulted
    x = torch.rand(2, 3, *size, generator=_gen(6)).to(cuda)
    enc = _round_trip(net, x)
    one = net.compress(x[1:2])
    assert one["strings"][0][0] == enc["strings"][0][1] and one["strings"][1][0] == enc["strings"][1][1]


def test_round_trip_cheng2020_anchor(cuda):
    from compressai.zoo import image_models

    torch.manual_seed(15)
    net = image_models["cheng2020-anchor"](1, context="checkerboard").to(cuda).eval()
    net.update()
    _round_trip(net, torch.rand(1, 3, 64, 128, generator=_gen(16)).to(cuda))


@pytest.mark.parametrize("guide_context", ["checkerboard", "raster"])
def test_codec_rgbt_file_round_trip_pair(cuda, tmp_path, guide_context):
    from compressai.models import Guided_compresser, Master_compresser
    from compressai.utils.codec_rgbt import decode_image, encode_image

    torch.manual_seed(7)
    g = Guided_compresser(channel=3, context=guide_context).to(cuda).eval()
    m = Master_compresser(width=64, height=64, channel=1, context="checkerboard").to(cuda).eval()
    for n in (g, m):
        n.update()
    g.ar_backend = m.ar_backend = "fused"       # the raster guide's backend; the checkerboard models ignore it
    x = torch.rand(1, 1, 64, 64, generator=_gen(8)).to(cuda)
    rgb = torch.rand(1, 3, 128, 128, generator=_gen(9)).to(cuda)
    path = tmp_path / "m.bin"
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        r = encode_image(x, [g, m], str(path), "Master_compresser", "mse", 3, guided=rgb)
        hdr, x_hat = decode_image(str(path), [g, m], guided=rgb)
        enc_g = g.compress(rgb)
        dec_g = g.decompress(enc_g["strings"], enc_g["shape"])
        ref = m.decompress(m.compress(x, dec_g["x_hat"]), dec_g)["x_hat"]
    assert not [w for w in caught if "not recommended" in str(w.message)]
    assert r["bpp"] == path.stat().st_size * 8.0 / (64 * 64)
    assert hdr == ("Master_compresser", "mse", 3, (64, 64), 8)
    assert torch.equal(x_hat, ref)


def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    d = b.abs().max().item()
    return (a - b).abs().max().item() / (d if d > 0 else 1.0)


def _train_both(cuda, bf16, side, monkeypatch):
    """tests/test_models_wide_gpu.py::_run_both for the small checkerboard JAHP against the oracle made
    checkerboard by the restatement (mask + anchor zeroing)."""
    from compressai.entropy_models import set_noise_source
    from compressai.losses import RateDistortionLoss
    from compressai.models import JointAutoregressiveHierarchicalPriors
    from compressai.models import google

    monkeypatch.setattr(google, "_HYPER_STREAM", "1" if side else "0")
    torch.manual_seed(0)
    ref = R.make_oracle_checkerboard(O.ARCHS["mbt2018"](32, 32))
    net = JointAutoregressiveHierarchicalPriors(32, 32, context="checkerboard")
    net.load_state_dict(ref.state_dict())
    net = net.to(cuda)
    x = torch.rand(2, 3, 64, 64, generator=_gen(4 if bf16 else 0))
    feed = O.NoiseFeed(record=_gen(1))
    with feed:
        out_r = ref(x)
    cr = O.RateDistortionLoss(1)(out_r, x)
    cr["loss"].backward()
    q = [n.to(cuda) for n in feed.drawn]
    set_noise_source(lambda t: q.pop(0))
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            out = net(x.to(cuda))
            c = RateDistortionLoss(1)(out, x.to(cuda))
    finally:
        set_noise_source(None)
    assert not q
    c["loss"].backward()
    torch.cuda.synchronize()
    wg, mask = net.context_prediction.weight.grad, net.context_prediction.mask
    assert wg is not None and (wg[mask == 0] == 0).all() and (wg[mask != 0] != 0).any()
    return ref, net, out_r, out, cr, c, feed.drawn, x


@pytest.mark.parametrize("side", [True, False], ids=["side-stream", "single-stream"])
def test_training_fp32_against_the_restatement(cuda, side, monkeypatch):
    """The fp32 bars of test_models_wide_gpu.py::test_fp32_parity_at_configured_width."""
    ref, net, out_r, out, cr, c, drawn, x = _train_both(cuda, False, side, monkeypatch)
    r64 = R.mask_weight_grad(copy.deepcopy(ref).double())
    for p in r64.parameters():
        p.grad = None
    with O.NoiseFeed([n.double() for n in drawn]):
        out64 = r64(x.double())
    O.RateDistortionLoss(1)(out64, x.double())["loss"].backward()

    def check(a, a32, a64, bar, what):
        e, e32 = relerr(a, a64), relerr(a32, a64)
        print(f"{what}: hip {e:.3e} cpu fp32 {e32:.3e}")
        assert e < max(bar, 2 * e32), (what, e, e32)

    check(out["x_hat"], out_r["x_hat"], out64["x_hat"], 1e-4, "x_hat")
    for k in out_r["likelihoods"]:
        check(out["likelihoods"][k], out_r["likelihoods"][k], out64["likelihoods"][k], 1e-4, k)
    for k in ("loss", "bpp_loss", "mse_loss"):
        assert abs(c[k].item() - cr[k].item()) <= 1e-4 * max(1.0, abs(cr[k].item())), k
    pr, p64 = dict(ref.named_parameters()), dict(r64.named_parameters())
    for n, p in net.named_parameters():
        if pr[n].grad is None:
            assert p.grad is None or p.grad.abs().max().item() == 0, n
            continue
        check(p.grad, pr[n].grad, p64[n].grad, 2e-3, n)


@pytest.mark.parametrize("side", [True, False], ids=["side-stream", "single-stream"])
def test_training_bf16_against_the_restatement(cuda, side, monkeypatch):
    """The bf16 bars of test_models_wide_gpu.py::test_bf16_bounds_at_configured_width."""
    from test_models_wide_gpu import BF16_LIK, BF16_LOSS, BF16_XHAT, GRAD_COS, TENSOR_COS

    ref, net, out_r, out, cr, c, _, _ = _train_both(cuda, True, side, monkeypatch)
    ex = relerr(out["x_hat"], out_r["x_hat"])
    el = {k: relerr(out["likelihoods"][k], out_r["likelihoods"][k]) for k in out_r["likelihoods"]}
    eloss = abs(c["loss"].item() - cr["loss"].item()) / abs(cr["loss"].item())
    pr = dict(ref.named_parameters())
    tcos, dots, na, nb = {}, 0.0, 0.0, 0.0
    for n, p in net.named_parameters():
        gr = pr[n].grad
        if gr is None or p.grad is None:
            continue
        g = p.grad.detach().float().cpu()
        assert torch.isfinite(g).all(), n
        tcos[n] = float(torch.nn.functional.cosine_similarity(g.double().flatten(), gr.double().flatten(), dim=0))
        dots += float((g.double() * gr.double()).sum())
        na += float((g.double() ** 2).sum())
        nb += float((gr.double() ** 2).sum())
    cos = dots / math.sqrt(na * nb)
    low = sorted(tcos.items(), key=lambda kv: kv[1])[:3]
    print(f"bf16 checkerboard JAHP: x_hat {ex:.3e} lik {el} loss {eloss:.3e} grad cos {cos:.6f} lowest {low}")
    assert ex < BF16_XHAT
    for k, v in el.items():
        assert v < BF16_LIK, k
    assert eloss < BF16_LOSS
    assert cos > GRAD_COS
    assert low[0][1] > TENSOR_COS, low
