"""The fused autoregressive coding backend, the parts that need no GPU: the backend switch of the context
models, its refusal of CPU tensors (no silent fallback: the two backends sum in different orders), the
structure check, the command-line flags, and the C entry points' argument validation (no launch)."""
import ctypes

import pytest
import torch
import torch.nn as nn


def _jahp(N=8, M=8):
    from compressai.models import JointAutoregressiveHierarchicalPriors

    return JointAutoregressiveHierarchicalPriors(N, M)


def test_default_backend_is_serial():
    from compressai.models import Cheng2020Anchor, Guided_compresser, Master_compresser

    assert _jahp().ar_backend == "serial"
    for cls in (Cheng2020Anchor, Guided_compresser, Master_compresser):
        assert cls.ar_backend.fget(cls.__new__(cls)) == "serial"


def test_backend_is_per_instance_and_validated():
    a, b = _jahp(), _jahp()
    a.ar_backend = "fused"
    assert a.ar_backend == "fused" and b.ar_backend == "serial"
    a.ar_backend = "serial"
    assert a.ar_backend == "serial"
    with pytest.raises(ValueError, match="ar_backend"):
        a.ar_backend = "parallel"
    assert a.ar_backend == "serial"


def test_fused_on_cpu_raises_at_compress():
    net = _jahp().eval()
    net.update()
    net.ar_backend = "fused"
    with pytest.raises(ValueError, match="GPU only"):
        net.compress(torch.rand(1, 3, 64, 64))
    with pytest.raises(ValueError, match="GPU only"):
        net._ar_encode_all(torch.zeros(1, 8, 2, 2), torch.zeros(1, 16, 2, 2))
    with pytest.raises(ValueError, match="GPU only"):
        net._ar_decode_all([b"\0" * 8], torch.zeros(1, 16, 2, 2))


def test_cli_flags():
    from compressai.utils.codec_rgbt import decode_parser, encode_parser
    from compressai.utils.eval_model.__main__ import setup_args

    base = ["in.png", "--path", "g.pth", "-o", "out.bin"]
    for parser in (encode_parser(), decode_parser()):
        assert parser.parse_args(base).ar_backend == "serial"
        assert parser.parse_args(base + ["--ar-backend", "fused"]).ar_backend == "fused"
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--ar-backend", "other"])
    ev = ["checkpoint", "/data", "-a", "mbt2018", "-p", "x.pth"]
    assert setup_args().parse_args(ev).ar_backend == "serial"
    assert setup_args().parse_args(ev + ["--ar-backend", "fused"]).ar_backend == "fused"


def test_structure_validation_rejects_other_entropy_parameters():
    from compressai.layers import MaskedConv2d
    from compressai.layers.conv import Conv2d

    net = _jahp()
    net.ar_backend = "fused"
    p = torch.zeros(1, 16, 2, 2)
    # four layers instead of three
    net.entropy_parameters = nn.Sequential(Conv2d(32, 26, 1), nn.LeakyReLU(), Conv2d(26, 21, 1), nn.LeakyReLU(),
                                           Conv2d(21, 16, 1), nn.LeakyReLU(), Conv2d(16, 16, 1))
    with pytest.raises(ValueError, match="three 1x1 convs"):
        net._ar_fused_pack(p)
    # ReLU between them
    net.entropy_parameters = nn.Sequential(Conv2d(32, 26, 1), nn.ReLU(), Conv2d(26, 21, 1), nn.ReLU(), Conv2d(21, 16, 1))
    with pytest.raises(ValueError, match="three 1x1 convs"):
        net._ar_fused_pack(p)
    # a 3x3 layer
    net.entropy_parameters = nn.Sequential(Conv2d(32, 26, 3, padding=1), nn.LeakyReLU(), Conv2d(26, 21, 1),
                                           nn.LeakyReLU(), Conv2d(21, 16, 1))
    with pytest.raises(ValueError, match="three 1x1 convs"):
        net._ar_fused_pack(p)
    # widths that do not chain from cat(params, ctx) to 2M
    net.entropy_parameters = nn.Sequential(Conv2d(32, 26, 1), nn.LeakyReLU(), Conv2d(26, 21, 1), nn.LeakyReLU(),
                                           Conv2d(21, 12, 1))
    with pytest.raises(ValueError, match="three 1x1 convs"):
        net._ar_fused_pack(p)
    # a 3x3 context model
    good = _jahp()
    good.ar_backend = "fused"
    good.context_prediction = MaskedConv2d(8, 16, kernel_size=3, padding=1, stride=1)
    with pytest.raises(ValueError, match="5x5"):
        good._ar_fused_pack(p)


@pytest.fixture(scope="module")
def native():
    import os

    from compressai import _native

    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libcai.so not built")
    _native.lib.load()
    return _native


def _args(native, **over):
    """A well-formed call with fake, aligned, never dereferenced pointers: validation runs before any launch."""
    a = native.ArArgs()
    a.B, a.H, a.W, a.M, a.Cp, a.Cx, a.C1, a.C2 = 1, 2, 3, 8, 16, 16, 26, 21
    for n in ("y", "params", "w_ctx", "b_ctx", "w1p", "w1c", "b1", "w2", "b2", "w3", "b3", "scale_table", "y_hat",
              "symbols", "indexes", "data", "offsets", "lengths", "cdfs", "cdf_sizes", "cdf_offsets", "status"):
        setattr(a, n, 0x1000)
    a.slope, a.scale_bound, a.n_scales, a.cdf_stride, a.n_cdfs, a.data_bytes = 0.01, 0.11, 64, 100, 64, 16
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over, msg", [
    (dict(H=0), "bad latent shape"),
    (dict(C1=0), "bad layer widths"),
    (dict(C1=5000), "exceeds"),
    (dict(M=1024, Cx=2048), "LDS"),
    (dict(n_scales=257), "scale table"),
    (dict(n_scales=0), "scale table"),
    (dict(w2=None), "null pointer"),
    (dict(w3=0x1004), "16-byte aligned"),
    (dict(scale_bound=0.0), "scale bound"),
])
def test_entry_points_validate_before_launch(native, over, msg):
    a = _args(native, **over)
    for fn in (native.lib.cai_ar_encode, native.lib.cai_ar_decode):
        with pytest.raises(ValueError, match=msg):
            fn(ctypes.byref(a), ctypes.c_void_p(0x1000), 1 << 30, None)


def test_entry_points_mode_specific_validation(native):
    with pytest.raises(ValueError, match="null pointer"):
        native.lib.cai_ar_encode(ctypes.byref(_args(native, symbols=None)), ctypes.c_void_p(0x1000), 1 << 30, None)
    for over, msg in ((dict(status=None), "null stream pointer"), (dict(data=0x1002), "4-byte aligned"),
                      (dict(cdf_stride=1), "CDF tables"), (dict(n_cdfs=32), "64 scales but 32 CDFs")):
        with pytest.raises(ValueError, match=msg):
            native.lib.cai_ar_decode(ctypes.byref(_args(native, **over)), ctypes.c_void_p(0x1000), 1 << 30, None)


def test_workspace_query_and_short_workspace(native):
    a = _args(native)
    assert native.lib.cai_ar_workspace_bytes(ctypes.byref(a)) == 1 * 2 * 3 * 26 * 4
    assert native.lib.cai_ar_workspace_bytes(ctypes.byref(_args(native, W=0))) == 0
    with pytest.raises(ValueError, match="workspace of 8 bytes, need 624"):
        native.lib.cai_ar_encode(ctypes.byref(a), ctypes.c_void_p(0x1000), 8, None)
