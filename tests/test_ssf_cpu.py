"""ScaleSpaceFlow (ssf2020) API surface on the CPU: no kernel is launched.

Class / zoo names and exports, the reference's argument errors, state_dict keys and shapes against the plain-torch
restatement (tests/ssf_reference.py), argument validation of the cai_ssf_* / cai_qrelu_* entry points, the
conv geometries of the three streams on the kernel dispatch, and the optimizer's parameter groups.
"""
import ctypes
import os

import pytest
import torch

import ssf_reference as R


@pytest.fixture(scope="module")
def native():
    from compressai import _native

    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libcai.so not built")
    _native.lib.load()
    return _native


def test_names_and_exports():
    import compressai
    from compressai import layers, zoo
    from compressai.losses import VideoRateDistortionLoss
    from compressai.models import utils
    from compressai.models.video import ScaleSpaceFlow
    from compressai.zoo.video import ssf2020

    assert zoo.video_models == {"ssf2020": ssf2020}
    assert zoo.models["ssf2020"] is ssf2020
    assert set(zoo.models) == set(zoo.image_models) | {"ssf2020"}
    assert "ssf2020" not in zoo.image_models
    assert compressai.models.video.ScaleSpaceFlow is ScaleSpaceFlow
    assert "QReLU" in layers.__all__ and issubclass(layers.QReLU, torch.autograd.Function)
    for fn in ("quantize_ste", "gaussian_kernel1d", "gaussian_kernel2d", "gaussian_blur", "meshgrid2d", "conv",
               "deconv", "update_registered_buffers"):
        assert callable(getattr(utils, fn)), fn
    net = ssf2020(3, num_levels=4, sigma0=1.0, scale_field_shift=0.5)
    assert isinstance(net, ScaleSpaceFlow)
    assert (net.num_levels, net.sigma0, net.scale_field_shift) == (4, 1.0, 0.5)
    for m in ("forward_keyframe", "forward_inter", "forward_prediction", "gaussian_volume", "warp_volume",
              "encode_keyframe", "decode_keyframe", "encode_inter", "decode_inter", "compress", "decompress",
              "aux_loss", "update", "load_state_dict", "from_state_dict"):
        assert callable(getattr(net, m)), m
    assert VideoRateDistortionLoss(0.01).lmbda == 0.01


def test_reference_argument_errors():
    from compressai.zoo import ssf2020

    for q in (0, 10):
        with pytest.raises(ValueError, match="quality"):
            ssf2020(q)
    with pytest.raises(ValueError, match="metric"):
        ssf2020(1, metric="psnr")
    with pytest.raises(RuntimeError):
        ssf2020(1, pretrained=True)
    net = ssf2020(1)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 128, 128))              # not a list
    with pytest.raises(RuntimeError):
        net.compress(torch.zeros(1, 3, 128, 128))
    with pytest.raises(RuntimeError):
        net.decompress("x", [])
    with pytest.raises(ValueError, match="multiples of 128"):
        net([torch.zeros(1, 3, 128, 192), torch.zeros(1, 3, 128, 192)])
    with pytest.raises(ValueError, match="multiples of 128"):
        net.compress([torch.zeros(1, 3, 64, 128)])


def test_kernel_helpers_match_restatement():
    from compressai.models.utils import gaussian_kernel1d, gaussian_kernel2d, meshgrid2d

    cpu = torch.device("cpu")
    for k, sg in ((11, 1.5), (5, 0.5)):
        # two independent formulations: equal to a few fp32 roundings, and to fp64 resolution in fp64
        a, b = gaussian_kernel1d(k, sg, cpu, torch.float32), R.gaussian_kernel1d(k, sg, cpu, torch.float32)
        assert a.shape == (k,) and torch.allclose(a, b, rtol=1e-6, atol=0) and abs(a.sum().item() - 1) < 1e-6
        a, b = gaussian_kernel2d(k, sg, cpu, torch.float64), R.gaussian_kernel2d(k, sg, cpu, torch.float64)
        assert a.shape == (k, k) and torch.allclose(a, b, rtol=1e-14, atol=0)
        assert torch.equal(a, a.t())
    assert torch.equal(meshgrid2d(2, 3, 4, 8, cpu), R.base_grid(2, 4, 8, cpu, torch.float32))


def test_state_dict_matches_restatement():
    from compressai.models.video import ScaleSpaceFlow

    torch.manual_seed(0)
    ref = R.ScaleSpaceFlow()
    net = ScaleSpaceFlow()
    a = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    b = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert a == b
    for k in ("motion_hyperprior.hyper_decoder_scale.deconv2.weight", "res_hyperprior.entropy_bottleneck._matrix0",
              "img_encoder.6.bias", "res_decoder.0.weight", "motion_decoder.6.weight",
              "img_hyperprior.gaussian_conditional.scale_table"):
        assert k in b, k
    assert b["res_decoder.0.weight"] == (384, 128, 5, 5)
    assert b["motion_encoder.0.weight"] == (128, 6, 5, 5)
    assert b["motion_decoder.6.weight"] == (128, 3, 5, 5)
    net.load_state_dict(ref.state_dict())   # strict
    for (ka, va), (kb, vb) in zip(ref.state_dict().items(), net.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_load_state_dict_resizes_the_six_cdf_buffer_sets():
    from compressai.models.video import ScaleSpaceFlow

    torch.manual_seed(0)
    sd = ScaleSpaceFlow().state_dict()
    for s in ("img", "res", "motion"):
        sd[f"{s}_hyperprior.entropy_bottleneck._quantized_cdf"] = torch.zeros(192, 7, dtype=torch.int32)
        sd[f"{s}_hyperprior.entropy_bottleneck._offset"] = torch.zeros(192, dtype=torch.int32)
        sd[f"{s}_hyperprior.entropy_bottleneck._cdf_length"] = torch.full((192,), 7, dtype=torch.int32)
        sd[f"{s}_hyperprior.gaussian_conditional._quantized_cdf"] = torch.zeros(64, 9, dtype=torch.int32)
        sd[f"{s}_hyperprior.gaussian_conditional._offset"] = torch.zeros(64, dtype=torch.int32)
        sd[f"{s}_hyperprior.gaussian_conditional._cdf_length"] = torch.full((64,), 9, dtype=torch.int32)
        sd[f"{s}_hyperprior.gaussian_conditional.scale_table"] = torch.linspace(0.11, 256, 64)
    net = ScaleSpaceFlow.from_state_dict(sd)
    assert net.res_hyperprior.entropy_bottleneck._quantized_cdf.shape == (192, 7)
    assert net.motion_hyperprior.gaussian_conditional._quantized_cdf.shape == (64, 9)
    assert net.img_hyperprior.gaussian_conditional.scale_table.shape == (64,)


def test_parameter_groups_put_the_three_quantiles_into_aux():
    from compressai.models.video import ScaleSpaceFlow
    from compressai.optim import parameter_groups

    main, aux = parameter_groups(ScaleSpaceFlow())
    assert aux == sorted(f"{s}_hyperprior.entropy_bottleneck.quantiles" for s in ("img", "res", "motion"))
    assert "motion_hyperprior.hyper_decoder_scale.deconv1.weight" in main


def test_cpu_tensors_are_refused():
    from compressai._ops import QReluFn, ScaleSpaceVolumeFn, ScaleSpaceWarpFn
    from compressai.models.utils import quantize_ste

    with pytest.raises(ValueError, match="GPU tensors only"):
        ScaleSpaceVolumeFn.apply(torch.zeros(1, 3, 16, 16), 1.5, 5)
    with pytest.raises(ValueError, match="GPU tensors only"):
        ScaleSpaceWarpFn.apply(torch.zeros(1, 3, 6, 16, 16), torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="GPU tensors only"):
        QReluFn.apply(torch.zeros(1, 8, 4, 4), 8, 100)
    with pytest.raises(ValueError, match="GPU tensors only"):
        quantize_ste(torch.zeros(1, 8, 4, 4))


def _einval(native, rc, text):
    assert rc == native.CAI_EINVAL
    msg = native.lib.load().cai_last_error()
    assert text in msg, msg


def test_ssf_entry_points_validate_before_launching(native):
    lib = native.lib.load()
    one = ctypes.c_void_p(16)       # a non-null pointer: validation must fail before anything reads it
    st = (ctypes.c_int64 * 4)(3 * 256, 256, 16, 1)
    assert lib.cai_ssf_workspace_bytes(6, 16, 16, 5) > 0
    assert lib.cai_ssf_workspace_bytes(6, 24, 16, 5) == 0
    assert b"multiples of 2^(levels-1)" in lib.cai_last_error()
    assert lib.cai_ssf_workspace_bytes(6, 16, 16, 0) == 0
    for fn in (lib.cai_ssf_volume_fwd, lib.cai_ssf_volume_bwd):
        _einval(native, fn(None, 6, 16, 16, 1.5, 5, one, one, 1 << 20, None), b"null pointer")
        _einval(native, fn(one, 6, 16, 16, 1.5, 0, one, one, 1 << 20, None), b"levels")
        _einval(native, fn(one, 6, 16, 40, 1.5, 5, one, one, 1 << 20, None), b"multiples of 2^(levels-1)")
        _einval(native, fn(one, 6, 16, 16, 5.5, 5, one, one, 1 << 20, None), b"taps")     # k = 35 > 31
        _einval(native, fn(one, 6, 16, 16, 0.0, 5, one, one, 1 << 20, None), b"taps")
        assert fn(one, 6, 16, 16, 1.5, 5, one, one, 16, None) == native.CAI_EWORKSPACE
    _einval(native, lib.cai_ssf_warp_fwd(None, one, st, 1, 3, 6, 16, 16, one, None, None, None), b"null pointer")
    _einval(native, lib.cai_ssf_warp_fwd(one, one, st, 1, 3, 0, 16, 16, one, None, None, None), b"bad shape")
    _einval(native, lib.cai_ssf_warp_fwd(one, one, st, 1, 3, 6, 16, 16, None, None, None, None), b"null output")
    _einval(native, lib.cai_ssf_warp_fwd(one, one, st, 1, 3, 6, 16, 16, one, one, None, None), b"go together")
    _einval(native, lib.cai_ssf_warp_bwd(one, None, st, 1, 3, 6, 16, 16, one, None, one, None, None), b"null pointer")
    _einval(native, lib.cai_ssf_warp_bwd(one, one, st, 1, 3, 6, 16, 16, None, None, one, None, None), b"upstream")
    _einval(native, lib.cai_ssf_warp_bwd(one, one, st, 1, 3, 6, 16, 16, one, None, None, None, None), b"null outputs")
    with pytest.raises(ValueError, match="levels"):
        native.lib.cai_ssf_volume_fwd(one, 6, 16, 16, 1.5, -1, one, one, 1 << 20, None)


def test_qrelu_entry_points_validate_before_launching(native):
    lib = native.lib.load()
    one = ctypes.c_void_p(16)
    _einval(native, lib.cai_qrelu_fwd(native.F32, None, 8, one, 8, 4, 8, 8, None), b"null pointer")
    _einval(native, lib.cai_qrelu_fwd(7, one, 8, one, 8, 4, 8, 8, None), b"bad dtype")
    _einval(native, lib.cai_qrelu_fwd(native.BF16, one, 4, one, 8, 4, 4, 8, None), b"multiple of 8")
    _einval(native, lib.cai_qrelu_fwd(native.F32, one, 8, one, 8, 4, 8, 0, None), b"bit_depth")
    _einval(native, lib.cai_qrelu_bwd(native.F32, one, 8, None, 8, one, 8, 4, 8, 8, 100.0, None), b"upstream")
    _einval(native, lib.cai_qrelu_bwd(native.F32, one, 8, one, 8, one, 8, 4, 8, 8, 0.0, None), b"beta")
    _einval(native, lib.cai_qrelu_bwd(native.F32, one, 8, one, 8, None, 8, 4, 8, 8, 100.0, None), b"null pointer")


def test_stream_geometries_dispatch(native):
    """Every conv geometry of the three streams has a kernel in each direction, fp32 and bf16 (host-side choice,
    no launch): 6 -> 128 conv, 384 -> 128 deconv, 192 -> 192 k5 s2 conv / deconv down to 1x1, 128 -> 3 deconv."""
    lib = native.lib.load()
    G = native.ConvGeom
    geoms = [G(1, 6, 128, 128, 128, 64, 64, 5, 2, 2, 0, 0), G(1, 3, 128, 128, 128, 64, 64, 5, 2, 2, 0, 0),
             G(1, 128, 16, 16, 192, 8, 8, 5, 2, 2, 0, 0), G(1, 384, 8, 8, 128, 16, 16, 5, 2, 2, 1, 1),
             G(1, 192, 8, 8, 192, 4, 4, 5, 2, 2, 0, 0), G(1, 192, 2, 2, 192, 1, 1, 5, 2, 2, 0, 0),
             G(1, 192, 1, 1, 192, 2, 2, 5, 2, 2, 1, 1), G(1, 192, 4, 4, 192, 8, 8, 5, 2, 2, 1, 1),
             G(1, 128, 64, 64, 3, 128, 128, 5, 2, 2, 1, 1)]
    for dt in (native.F32, native.BF16):
        for g in geoms:
            for direction in (0, 1, 2):
                name = lib.cai_conv_kernel_name(ctypes.byref(g), dt, direction, 0).decode()
                assert name and "none" not in name.lower(), (dt, g.in_c, g.out_c, g.in_h, direction, name)
