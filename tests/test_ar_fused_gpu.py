"""ar_backend = "fused": the autoregressive scan of the context models in one kernel launch (csrc/ar_coder.hip).

  * decompress(compress(x)) rebuilds exactly the encoder-side reconstruction, strings are deterministic and do
    not depend on the batch, and no "not recommended on GPU" warning is left;
  * the decoder's y_hat equals the encoder's bit for bit at odd layer widths (128 -> 106 -> 85 -> 64) and edge
    geometries (1x1, 1x9, 6x1, 5x7 latents);
  * teacher-forced parity: the scales / means the kernel used agree with an fp64 CPU recomputation from its own
    y_hat (F.conv2d with the masked weight, the 1x1 stack) within the project's fp32 bar 1e-4 * max(1, max|ref|),
    and the discrete steps (symbols, y_hat, indexes) hold exactly given the kernel's values;
  * the in-kernel rANS decoder reads what the host coder reads, escapes (both signs, >= 3 bypass nibbles) included;
  * a truncated stream ends in the host decoder's ValueError, the other stream of the batch is unharmed;
  * the multi-modal pair and the container file work unchanged on the fused backend.
"""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _jahp(cuda, N, M, seed):
    from compressai.models import JointAutoregressiveHierarchicalPriors

    torch.manual_seed(seed)
    net = JointAutoregressiveHierarchicalPriors(N, M).to(cuda).eval()
    net.update()
    net.ar_backend = "fused"
    return net


@pytest.fixture(scope="module")
def net32(cuda):
    """Layer widths 128 -> 106 -> 85 -> 64: no divisibility to lean on."""
    return _jahp(cuda, 32, 32, 21)


@pytest.fixture(scope="module")
def net192(cuda):
    """The flagship entropy model (768 -> 640 -> 512 -> 384) on a small transform."""
    return _jahp(cuda, 8, 192, 22)


def _synthetic(net, B, H, W, seed, cuda, amp=3.0):
    M = net.context_prediction.in_channels
    y = (amp * torch.randn(B, M, H, W, generator=_gen(seed))).to(cuda)
    params = torch.randn(B, 2 * M, H, W, generator=_gen(seed + 1)).to(cuda)
    return y, params


def test_round_trip_small_jahp(cuda):
    from compressai._prepack import prepacked_forward

    net = _jahp(cuda, 32, 48, 5)
    x = torch.rand(2, 3, 64, 128, generator=_gen(6)).to(cuda)
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)
        enc = net.compress(x)
        dec = net.decompress(enc["strings"], enc["shape"])
        enc2 = net.compress(x)
    assert enc2["strings"] == enc["strings"]                      # deterministic
    assert all(isinstance(s, bytes) and len(s) >= 8 for s in enc["strings"][0])
    # the encoder-side y_hat, and what g_s makes of it
    with torch.no_grad(), prepacked_forward(net):
        y = net.g_a(x)
        assert tuple(y.shape[2:]) == (4, 8)
        z_hat = net.entropy_bottleneck.decompress(enc["strings"][1], enc["shape"])
        params = net.h_s(z_hat)
        e = net._ar_encode_fused(y, params)
        assert e["strings"] == enc["strings"][0]
        x_rec = net.g_s(e["y_hat"]).clamp_(0, 1)
    assert torch.equal(dec["x_hat"], x_rec)
    # every image's strings are those of a batch of one
    for i in range(2):
        one = net.compress(x[i:i + 1])
        assert one["strings"][0][0] == enc["strings"][0][i]
        assert one["strings"][1][0] == enc["strings"][1][i]


def test_round_trip_cheng2020_anchor(cuda):
    """The cheng2020 models inherit the coding from JointAutoregressiveHierarchicalPriors (M = N)."""
    from compressai._prepack import prepacked_forward
    from compressai.models import Cheng2020Anchor

    torch.manual_seed(15)
    net = Cheng2020Anchor(N=32).to(cuda).eval()
    net.update()
    net.ar_backend = "fused"
    x = torch.rand(1, 3, 64, 128, generator=_gen(16)).to(cuda)
    enc = net.compress(x)
    dec = net.decompress(enc["strings"], enc["shape"])
    with torch.no_grad(), prepacked_forward(net):
        y = net.g_a(x)
        params = net.h_s(net.entropy_bottleneck.decompress(enc["strings"][1], enc["shape"]))
        e = net._ar_encode_fused(y, params)
        assert e["strings"] == enc["strings"][0]
        x_rec = net.g_s(e["y_hat"]).clamp_(0, 1)
    assert torch.equal(dec["x_hat"], x_rec)


@pytest.mark.parametrize("B, H, W", [(1, 1, 1), (2, 1, 9), (1, 6, 1), (2, 5, 7)])
def test_odd_widths_and_edge_geometry(cuda, net32, B, H, W):
    ep = net32.entropy_parameters
    assert [ep[i].out_channels for i in (0, 2, 4)] == [106, 85, 64] and ep[0].in_channels == 128
    y, params = _synthetic(net32, B, H, W, 100 + 10 * H + W, cuda)
    e = net32._ar_encode_fused(y, params)
    y_dec = net32._ar_decode_all(e["strings"], params)
    assert y_dec.shape == y.shape
    assert torch.equal(y_dec, e["y_hat"])
    assert (e["y_hat"] - y).abs().max().item() <= 0.5 + 1e-3     # rounding around the mean


def _reference_params(net, y_hat, params):
    """The entropy parameters as the reference computes them (google.py:498-507), fp64 on the CPU."""
    cp, ep = net.context_prediction, net.entropy_parameters
    w = (cp.weight.data * cp.mask).double().cpu()
    ctx = F.conv2d(y_hat.double().cpu(), w, cp.bias.double().cpu(), padding=2)
    h = torch.cat((params.double().cpu(), ctx), 1)
    for i in (0, 2, 4):
        h = F.conv2d(h, ep[i].weight.double().cpu(), ep[i].bias.double().cpu())
        if i < 4:
            h = F.leaky_relu(h, ep[i + 1].negative_slope)
    return h.chunk(2, 1)


@pytest.mark.parametrize("which, B, H, W", [("net32", 2, 5, 7), ("net192", 1, 4, 4)])
def test_teacher_forced_parity(cuda, request, which, B, H, W):
    net = request.getfixturevalue(which)
    gc = net.gaussian_conditional
    y, params = _synthetic(net, B, H, W, 300 + H, cuda)
    e = net._ar_encode_fused(y, params, with_params=True)
    M = y.size(1)
    scales_k = e["scales"].permute(0, 3, 1, 2)        # [B, H, W, M] -> [B, M, H, W]
    means_k = e["means"].permute(0, 3, 1, 2)
    symbols = e["symbols"].reshape(B, H, W, M).permute(0, 3, 1, 2)
    indexes = e["indexes"].reshape(B, H, W, M).permute(0, 3, 1, 2)
    scales_r, means_r = _reference_params(net, e["y_hat"], params)
    for name, got, ref in (("scales", scales_k, scales_r), ("means", means_k, means_r)):
        err = (got.double().cpu() - ref).abs().max().item()
        tol = 1e-4 * max(1.0, ref.abs().max().item())
        print(f"{which} {name}: max err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (name, err, tol)
    # the discrete steps, exact on the kernel's own values
    assert torch.equal(symbols, torch.round(y - means_k).int())
    assert torch.equal(e["y_hat"], symbols.float() + means_k)
    assert torch.equal(indexes, gc.build_indexes(scales_k))


def test_device_decoder_equals_host_decoder_with_escapes(cuda, net32):
    from compressai import _coder, _ops

    gc = net32.gaussian_conditional
    B, H, W = 2, 5, 7
    y, params = _synthetic(net32, B, H, W, 400, cuda)
    y[0, 3, 1, 2], y[0, 7, 2, 5], y[1, 0, 0, 0], y[1, 31, 4, 6] = 40.0, -40.0, 5000.0, -5000.0
    e = net32._ar_encode_fused(y, params, with_params=True)
    sym, idx = e["symbols"].cpu().numpy().astype(np.int64), e["indexes"].cpu().numpy()
    offset, length = gc._offset.cpu().numpy()[idx], gc._cdf_length.cpu().numpy()[idx]
    value, max_value = sym - offset, length - 2
    neg, pos = value < 0, value >= max_value
    raw = np.where(neg, -2 * value - 1, 2 * (value - max_value))
    assert pos.any() and neg.any()                         # escapes of both signs
    assert ((neg | pos) & (raw >= 1 << 8)).any()           # one needs >= 3 bypass nibbles
    assert (~neg & ~pos).any()                             # and in-range symbols
    # the host decoder reads the kernel's symbols back from the strings ...
    assert np.array_equal(_coder.decode_streams(e["strings"], idx, gc._tables()), sym)
    # ... and so does the kernel's: symbols, indexes and y_hat bit for bit
    d = _ops.ar_decode(net32._ar_fused_pack(params), e["strings"], params, with_params=True)
    assert d["status"].tolist() == [0, 0]
    assert torch.equal(d["symbols"], e["symbols"]) and torch.equal(d["indexes"], e["indexes"])
    assert torch.equal(d["y_hat"], e["y_hat"])
    assert torch.equal(d["scales"], e["scales"]) and torch.equal(d["means"], e["means"])


def test_bad_stream_is_a_value_error(cuda, net32):
    from compressai import _ops

    y, params = _synthetic(net32, 2, 5, 7, 500, cuda)
    e = net32._ar_encode_fused(y, params)
    strings = [e["strings"][0], e["strings"][1][:-8]]
    assert len(strings[1]) >= 8
    with pytest.raises(ValueError, match="item 1: truncated or corrupt stream"):
        net32._ar_decode_all(strings, params)
    d = _ops.ar_decode(net32._ar_fused_pack(params), strings, params, check=False)
    assert d["status"].tolist() == [0, 1]
    assert torch.equal(d["y_hat"][0], e["y_hat"][0])       # the intact stream is decoded in full
    with pytest.raises(ValueError, match="item 0: stream length"):
        net32._ar_decode_all([e["strings"][0][:-2], e["strings"][1]], params)


@pytest.fixture(scope="module")
def pair(cuda):
    from compressai.models import Guided_compresser, Master_compresser

    torch.manual_seed(7)
    g = Guided_compresser(channel=3).to(cuda).eval()
    m = Master_compresser(width=64, height=64, channel=1).to(cuda).eval()
    for n in (g, m):
        n.update()
        n.ar_backend = "fused"
    x = torch.rand(1, 1, 64, 64, generator=_gen(8)).to(cuda)
    rgb = torch.rand(1, 3, 128, 128, generator=_gen(9)).to(cuda)
    return g, m, x, rgb


def test_multimodal_round_trip_fused(cuda, pair):
    """test_coding_gpu.py::test_multimodal_round_trip's scenario on the fused backend."""
    from compressai._ops import CatFn, ChannelAffineFn
    from compressai._prepack import prepacked_forward

    g, m, x, rgb = pair
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        enc_g = g.compress(rgb)
        dec_g = g.decompress(enc_g["strings"], enc_g["shape"])
        enc_m = m.compress(x, dec_g["x_hat"])
        dec_m = m.decompress(enc_m, dec_g)
    assert not [w for w in caught if "not recommended" in str(w.message)]
    assert dec_g["x_hat"].shape == rgb.shape and set(dec_g["hidden"]) == {"gs1", "gs2", "gs3"}
    with torch.no_grad(), prepacked_forward(m):
        xf = m.fencoder1(x)
        ga, beta, gamma = m.ch_aligner(xf, m.fencoder2(dec_g["x_hat"]))
        y = m.g_a(CatFn.apply(xf, ga))
        z_hat = m.entropy_bottleneck.decompress(enc_m["strings"][1], enc_m["shape"])
        params = m.h_s(z_hat)
        e = m._ar_encode_fused(y, params)
        assert e["strings"] == enc_m["strings"][0]
        res = m.decoder(e["y_hat"], dec_g["hidden"])
        ga2 = ChannelAffineFn.apply(m.fencoder2(dec_g["x_hat"]), gamma, beta)
        x_rec = m.fdecoder(CatFn.apply(res["x_feature_hat"], ga2)).clamp_(0, 1)
    assert torch.equal(dec_m["x_hat"], x_rec)


def test_codec_rgbt_file_round_trip_fused(cuda, pair, tmp_path):
    """test_coding_gpu.py::test_codec_rgbt_file_round_trip's Master case through the container, fused."""
    from compressai.utils.codec_rgbt import decode_image, encode_image

    g, m, x, rgb = pair
    path = tmp_path / "m.bin"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = encode_image(x, [g, m], str(path), "Master_compresser", "mse", 3, guided=rgb)
        hdr, x_hat = decode_image(str(path), [g, m], guided=rgb)
        enc_g = g.compress(rgb)
        dec_g = g.decompress(enc_g["strings"], enc_g["shape"])
        ref = m.decompress(m.compress(x, dec_g["x_hat"]), dec_g)["x_hat"]
    assert r["bpp"] == path.stat().st_size * 8.0 / (64 * 64)
    assert hdr == ("Master_compresser", "mse", 3, (64, 64), 8)
    assert torch.equal(x_hat, ref)
