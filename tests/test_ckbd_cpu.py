"""Checkerboard context models, the parts that need no kernel: the mask, the constructor option, state_dict
compatibility and the checkpoint rule, the coder's slot order, and the causality of the plain-torch restatement
(tests/ckbd_reference.py) the GPU tests compare against."""
import pytest
import torch

import ckbd_reference as R


def _models(context):
    from compressai.models import (Cheng2020Anchor, Cheng2020Attention, Guided_compresser,
                                   JointAutoregressiveHierarchicalPriors, Master_compresser)

    return {"mbt2018": JointAutoregressiveHierarchicalPriors(8, 16, context=context),
            "cheng2020-anchor": Cheng2020Anchor(8, context=context),
            "cheng2020-attn": Cheng2020Attention(8, context=context),
            "Guided_compresser": Guided_compresser(N=8, M=16, channel=3, context=context),
            "Master_compresser": Master_compresser(width=64, height=64, channel=1, context=context)}


@pytest.fixture(scope="module")
def nets():
    return {c: _models(c) for c in ("raster", "checkerboard")}


def test_mask_has_the_12_odd_taps_in_every_channel_pair():
    from compressai.layers import CheckerboardMaskedConv2d, MaskedConv2d

    for conv in (MaskedConv2d(6, 12, 5, padding=2, mask_type="checkerboard"), CheckerboardMaskedConv2d(6, 12, 5, padding=2)):
        assert conv.mask.shape == (12, 6, 5, 5)
        want = torch.tensor([[(i + j) % 2 for j in range(5)] for i in range(5)], dtype=conv.mask.dtype)
        assert torch.equal(conv.mask, want.expand(12, 6, 5, 5))
        assert int(conv.mask[3, 2].sum()) == 12 and conv.mask[0, 0, 2, 2] == 0
    assert torch.equal(want != 0, R.checkerboard_mask())
    assert isinstance(CheckerboardMaskedConv2d(2, 4, 5, padding=2), MaskedConv2d)
    # the raster masks are what they were
    a = MaskedConv2d(1, 1, 5, padding=2).mask[0, 0]
    assert a.flatten()[:12].all() and not a.flatten()[12:].any()
    assert int(MaskedConv2d(1, 1, 5, padding=2, mask_type="B").mask.sum()) == 13


def test_bad_context_or_mask_type_is_a_value_error():
    from compressai.layers import MaskedConv2d
    from compressai.models import (Cheng2020Anchor, Guided_compresser, JointAutoregressiveHierarchicalPriors,
                                   Master_compresser)

    with pytest.raises(ValueError, match="mask_type"):
        MaskedConv2d(2, 4, 5, mask_type="C")
    for build in (lambda: JointAutoregressiveHierarchicalPriors(8, 16, context="diagonal"),
                  lambda: Cheng2020Anchor(8, context="Checkerboard"),
                  lambda: Guided_compresser(N=8, M=16, context=None),
                  lambda: Master_compresser(width=64, height=64, channel=1, context="zigzag")):
        with pytest.raises(ValueError, match="context must be one of"):
            build()


def test_context_property_and_default(nets):
    from compressai.models import JointAutoregressiveHierarchicalPriors

    assert JointAutoregressiveHierarchicalPriors(8, 16).context == "raster"
    for c, group in nets.items():
        for name, net in group.items():
            assert net.context == c, name
            with pytest.raises(AttributeError):
                net.context = "raster"
            assert int(net.context_prediction.mask[0, 0].sum()) == 12


def test_state_dict_keys_and_shapes_equal_the_raster_models(nets):
    for name, ras in nets["raster"].items():
        a, b = ras.state_dict(), nets["checkerboard"][name].state_dict()
        assert list(a) == list(b), name
        assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a), name
        assert [n for n, _ in ras.named_modules()] == [n for n, _ in nets["checkerboard"][name].named_modules()]


def test_dp_phases_equal_the_raster_models(nets):
    for name, ras in nets["raster"].items():
        assert nets["checkerboard"][name].dp_phases() == ras.dp_phases(), name


def test_from_state_dict_picks_the_context_from_the_mask(nets):
    from compressai.models import Cheng2020Anchor, Cheng2020Attention, JointAutoregressiveHierarchicalPriors
    from compressai.models.google import context_of

    classes = {"mbt2018": JointAutoregressiveHierarchicalPriors, "cheng2020-anchor": Cheng2020Anchor,
               "cheng2020-attn": Cheng2020Attention}
    for c, group in nets.items():
        for name, cls in classes.items():
            sd = group[name].state_dict()
            assert context_of(sd) == c
            net = cls.from_state_dict(sd)
            assert net.context == c and type(net) is cls
            assert torch.equal(net.context_prediction.mask, group[name].context_prediction.mask)
    assert context_of({}) == "raster" and context_of({}, default=None) is None
    bad = {"context_prediction.mask": torch.ones(4, 2, 5, 5)}
    with pytest.raises(ValueError, match="neither"):
        context_of(bad)


def test_loaders_read_the_context_from_the_checkpoint(nets, tmp_path):
    from compressai.utils.eval_model.__main__ import load_checkpoint
    from compressai.utils.update_model.__main__ import build

    for c, group in nets.items():
        sd = group["mbt2018"].state_dict()
        assert build("jarhp", sd, 3).context == c
        path = tmp_path / f"{c}.pth"
        torch.save(sd, path)
        assert load_checkpoint("mbt2018", str(path)).context == c


def test_loading_the_other_contexts_checkpoint_raises(nets):
    for name in nets["raster"]:
        ras, ck = nets["raster"][name], nets["checkerboard"][name]
        for model, sd in ((ck, ras.state_dict()), (ras, ck.state_dict())):
            before = model.context_prediction.mask.clone()
            with pytest.raises(ValueError, match="raster.*checkerboard|checkerboard.*raster"):
                model.load_state_dict(sd)
            assert torch.equal(model.context_prediction.mask, before), name
        ck.load_state_dict(ck.state_dict())
        ras.load_state_dict(ras.state_dict())


def test_zoo_keyword():
    from compressai.zoo import image_models

    net = image_models["cheng2020-anchor"](1, context="checkerboard")
    assert net.context == "checkerboard" and int(net.context_prediction.mask[0, 0].sum()) == 12
    assert image_models["mbt2018"](1, context="checkerboard").context == "checkerboard"
    assert image_models["mbt2018"](1).context == "raster"
    assert not [k for k in image_models if "checkerboard" in k]


@pytest.mark.parametrize("H", [1, 2, 3, 5, 6])
@pytest.mark.parametrize("W", [1, 2, 5, 6])
def test_closed_form_slot_equals_the_enumeration(H, W):
    from compressai._ops import ANCHOR, NON_ANCHOR, ckbd_slot_range

    order = R.slot_order(H, W)
    n1 = H * W // 2
    assert int(R.anchor_map(H, W).sum()) == n1
    assert ckbd_slot_range(H, W, ANCHOR) == (0, n1) and ckbd_slot_range(H, W, NON_ANCHOR) == (n1, H * W)
    assert sorted(order) == [(h, w) for h in range(H) for w in range(W)]
    for slot, (h, w) in enumerate(order):
        anchor = (h + w) % 2 == 1
        assert bool(R.anchor_map(H, W)[h, w]) == anchor
        assert slot == R.slot_closed_form(h, w, H, W) + (0 if anchor else n1), (h, w)
    t = torch.arange(2 * 3 * H * W).reshape(2, 3, H, W)
    flat = R.to_coder_order(t).reshape(2, H * W, 3)
    for slot, (h, w) in enumerate(order):
        assert torch.equal(flat[:, slot], t[:, :, h, w])


def test_invalid_arguments_are_einval_before_any_launch():
    """No GPU here and the pointers are not device memory: a call that got past validation could not return
    CAI_EINVAL."""
    import ctypes
    import os

    from compressai import _native

    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libcai.so not built")
    lib = _native.lib.load()
    P = ctypes.c_void_p(4096)
    F = _native.F32
    calls = [
        lib.cai_parity_zero(7, P, 8, P, 8, 1, 2, 2, 8, 0, None),             # dtype
        lib.cai_parity_zero(F, None, 8, P, 8, 1, 2, 2, 8, 0, None),          # null
        lib.cai_parity_zero(F, P, 8, P, 8, 1, 2, 2, 8, 0, None),             # aliased
        lib.cai_parity_zero(F, P, 4, ctypes.c_void_p(8192), 8, 1, 2, 2, 8, 0, None),   # pitch
        lib.cai_parity_zero(F, P, 8, ctypes.c_void_p(8192), 8, 1, 2, 2, 8, 2, None),   # parity
        lib.cai_parity_zero(F, P, 8, ctypes.c_void_p(8192), 8, 1, 0, 2, 8, 1, None),   # shape
        lib.cai_parity_zero(F, P, 8, ctypes.c_void_p(8192), 8, 1 << 12, 1 << 10, 1 << 9, 8, 1, None),   # 2^31
        lib.cai_ckbd_quantize(P, 8, None, 8, P, 8, P, 64, 0.11, 1, 2, 2, 8, 1, P, 8, P, P, None),
        lib.cai_ckbd_quantize(P, 8, P, 8, P, 8, P, 64, 0.11, 1, 2, 2, 8, 1, None, 8, P, P, None),
        lib.cai_ckbd_quantize(P, 8, P, 8, P, 4, P, 64, 0.11, 1, 2, 2, 8, 1, P, 8, P, P, None),
        lib.cai_ckbd_quantize(P, 8, P, 8, P, 8, P, 0, 0.11, 1, 2, 2, 8, 1, P, 8, P, P, None),
        lib.cai_ckbd_indexes(P, 8, P, 64, 0.11, 1, 2, 2, 8, -1, P, None),
        lib.cai_ckbd_indexes(P, 7, P, 64, 0.11, 1, 2, 2, 8, 0, P, None),
        lib.cai_ckbd_indexes(P, 8, P, 64, 0.11, 1, 2, 2, 8, 0, None, None),
        lib.cai_ckbd_dequantize(None, P, 8, 1, 2, 2, 8, 0, P, 8, None),
        lib.cai_ckbd_dequantize(P, P, 8, 1, 2, 2, 8, 0, P, 6, None),
        lib.cai_ckbd_dequantize(P, P, 8, 0, 2, 2, 8, 0, P, 8, None),
    ]
    assert calls == [_native.CAI_EINVAL] * len(calls)
    assert lib.cai_last_error()
    # a 1 x 1 map has no anchors: nothing to launch, and that is not an error
    assert lib.cai_ckbd_indexes(P, 8, P, 64, 0.11, 1, 1, 1, 8, 1, P, None) == _native.CAI_OK
    with pytest.raises(ValueError, match="parity"):
        _native.lib.cai_ckbd_dequantize(P, P, 8, 1, 2, 2, 8, 5, P, 8, None)


def _restatement_inputs(seed, B=2, M=8, H=5, W=6):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    widths = [4 * M, 3 * M + 1, 2 * M + 3, 2 * M]
    layers = [(r(widths[i + 1], widths[i], 1, 1) * 0.2, r(widths[i + 1])) for i in range(3)]
    return r(B, M, H, W) * 3, r(B, 2 * M, H, W), r(2 * M, M, 5, 5) * 0.2, r(2 * M), layers


def test_restatement_is_causal():
    """Anchors' parameters do not depend on y_hat at all; non-anchors' do not depend on non-anchor y_hat (they do
    depend on the anchors')."""
    y_hat, params, cw, cb, layers = _restatement_inputs(3)
    anchor = R.anchor_map(5, 6)
    s0, m0 = R.entropy_params(y_hat, params, cw, cb, layers)
    noise = torch.randn(y_hat.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    s1, m1 = R.entropy_params(y_hat + noise, params, cw, cb, layers)
    assert torch.equal(s1[..., anchor], s0[..., anchor]) and torch.equal(m1[..., anchor], m0[..., anchor])
    assert not torch.equal(m1[..., ~anchor], m0[..., ~anchor])
    s2, m2 = R.entropy_params(y_hat + noise * (~anchor), params, cw, cb, layers)
    assert torch.equal(s2, s0) and torch.equal(m2, m0)
    # the two-pass encode is what a decoder can follow: y_hat's parameters are those of its own y_hat
    table = torch.exp(torch.linspace(-2.0, 5.0, 16, dtype=torch.float64))
    e = R.two_pass_encode(y_hat, params, cw, cb, layers, 0.01, table, 0.11)
    s3, m3 = R.entropy_params(e["y_hat"], params, cw, cb, layers)
    assert torch.equal(s3, e["scales"]) and torch.equal(m3, e["means"])
    assert torch.equal(e["y_hat"], torch.round(y_hat - m3) + m3)
    assert (e["y_hat"] - y_hat).abs().max() <= 0.5
