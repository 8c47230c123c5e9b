"""The raw-video front door on the CPU: the fp64 restatement (tests/video_reference.py) against torch, the public
transforms against the restatement, the raw reader, the frame-folder dataset, the bitstream container, and the torch
body of compressai.utils.video.frames against the restatement under the GPU test's tolerances."""
import io
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import video_reference as R

MODES = ("nearest", "bilinear", "bicubic")


def rand64(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------
# the restatement against torch in fp64
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (17, 9)])
def test_upsampling_matches_interpolate(mode, shape):
    x = rand64(2, 1, *shape, seed=shape[0])
    kw = {} if mode == "nearest" else {"align_corners": False}
    want = F.interpolate(x, scale_factor=2, mode=mode, **kw)
    got = R.up2(x, mode)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("shape", [(2, 2), (4, 6), (34, 18)])
def test_pooling_matches_avg_pool(shape):
    x = rand64(2, 1, *shape, seed=3)
    assert (R.pool2(x) - F.avg_pool2d(x, kernel_size=2, stride=2)).abs().max().item() <= 1e-12


def test_bicubic_impulse_response_is_dyadic():
    x = torch.zeros(1, 1, 1, 9, dtype=torch.float64)
    x[..., 4] = 1.0
    row = R.up2(x, "bicubic")[0, 0, 0]
    w = R.BICUBIC
    # sample 4 is tap k+1, k, k-1, k-2 of the even outputs 6, 8, 10, 12 (weights w3, w2, w1, w0) and tap k+2, k+1, k,
    # k-1 of the odd outputs 5, 7, 9, 11 (the mirrored set: w0, w1, w2, w3)
    want = {5: w[0], 6: w[3], 7: w[1], 8: w[2], 9: w[2], 10: w[1], 11: w[3], 12: w[0]}
    for i in range(18):
        assert row[i].item() == want.get(i, 0.0), i
    for mode in MODES:      # every filter has unit gain
        assert torch.equal(R.up2(torch.ones(1, 1, 5, 7, dtype=torch.float64), mode), torch.ones(1, 1, 10, 14,
                                                                                               dtype=torch.float64))


def test_colour_round_trip_and_known_values():
    x = rand64(2, 3, 5, 7, seed=1)
    assert (R.ycbcr2rgb(R.rgb2ycbcr(x)) - x).abs().max().item() <= 1e-12

    def px(r, g, b):
        return R.rgb2ycbcr(torch.tensor([r, g, b], dtype=torch.float64).reshape(3, 1, 1)).flatten().tolist()

    assert px(1, 1, 1) == pytest.approx([1.0, 0.5, 0.5], abs=1e-12)
    assert px(0, 0, 0) == pytest.approx([0.0, 0.5, 0.5], abs=1e-12)
    # red: y = Kr, cb = 0.5 - 0.5 Kr / (1 - Kb), cr = 1
    assert px(1, 0, 0) == pytest.approx([0.2126, 0.5 - 0.5 * 0.2126 / (1 - 0.0722), 1.0], abs=1e-12)


# ---------------------------------------------------------------------------------------------------------
# compressai.transforms against the restatement
# ---------------------------------------------------------------------------------------------------------
def test_transforms_functional_fp64():
    from compressai.transforms import functional as T

    x = rand64(2, 3, 6, 10, seed=2)
    assert (T.rgb2ycbcr(x) - R.rgb2ycbcr(x)).abs().max().item() <= 1e-12
    assert (T.ycbcr2rgb(x) - R.ycbcr2rgb(x)).abs().max().item() <= 1e-12
    assert (T.rgb2ycbcr(x[0]) - R.rgb2ycbcr(x[0])).abs().max().item() <= 1e-12        # 3-D input
    for got, want in zip(T.yuv_444_to_420(x), R.yuv_444_to_420(x)):
        assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12
    for got, want in zip(T.yuv_444_to_420(tuple(x.chunk(3, 1))), R.yuv_444_to_420(x)):
        assert (got - want).abs().max().item() <= 1e-12
    yuv = (rand64(2, 1, 6, 10, seed=4), rand64(2, 1, 3, 5, seed=5), rand64(2, 1, 3, 5, seed=6))
    for mode in MODES:
        want = R.yuv_420_to_444(yuv, mode)
        got = T.yuv_420_to_444(yuv, mode=mode)
        assert got.shape == (2, 3, 6, 10) and (got - want).abs().max().item() <= 1e-12
        parts = T.yuv_420_to_444(yuv, mode=mode, return_tuple=True)
        assert isinstance(parts, tuple) and len(parts) == 3
        assert (torch.cat(parts, dim=1) - want).abs().max().item() <= 1e-12
    assert T.yuv_420_to_444(yuv).equal(T.yuv_420_to_444(yuv, mode="bilinear"))


def test_transforms_are_differentiable_and_classes_call_them():
    from compressai import transforms as TT
    from compressai.transforms import functional as T

    x = rand64(1, 3, 4, 4, seed=7).requires_grad_()
    T.ycbcr2rgb(T.rgb2ycbcr(x)).sum().backward()
    assert (x.grad - 1).abs().max().item() <= 1e-12
    y = x.detach()
    assert TT.RGB2YCbCr()(y).equal(T.rgb2ycbcr(y)) and TT.YCbCr2RGB()(y).equal(T.ycbcr2rgb(y))
    planes = TT.YUV444To420()(y)
    assert [tuple(p.shape) for p in planes] == [(1, 1, 4, 4), (1, 1, 2, 2), (1, 1, 2, 2)]
    assert TT.YUV420To444(mode="bicubic")(planes).equal(T.yuv_420_to_444(planes, mode="bicubic"))
    assert isinstance(TT.YUV420To444(return_tuple=True)(planes), tuple)
    assert repr(TT.RGB2YCbCr()) == "RGB2YCbCr()"


def test_transforms_value_errors():
    from compressai.transforms import functional as T

    for fn in (T.rgb2ycbcr, T.ycbcr2rgb):
        with pytest.raises(ValueError, match="Expected a 3D or 4D tensor"):
            fn(torch.rand(3, 4))                             # wrong rank
        with pytest.raises(ValueError, match="Expected a 3D or 4D tensor"):
            fn(torch.zeros(1, 3, 4, 4, dtype=torch.int32))   # integer dtype
        with pytest.raises(ValueError, match="Expected a 3D or 4D tensor"):
            fn(torch.rand(1, 4, 4, 4))                       # not three channels
    with pytest.raises(ValueError, match="Invalid downsampling mode"):
        T.yuv_444_to_420(torch.rand(1, 3, 4, 4), mode="lanczos")
    planes = (torch.rand(1, 1, 4, 4), torch.rand(1, 1, 2, 2), torch.rand(1, 1, 2, 2))
    with pytest.raises(ValueError, match="Invalid upsampling mode"):
        T.yuv_420_to_444(planes, mode="area")
    with pytest.raises(ValueError, match="tuple of 3 torch tensors"):
        T.yuv_420_to_444(planes[:2])
    with pytest.raises(ValueError, match="tuple of 3 torch tensors"):
        T.yuv_420_to_444((planes[0], planes[1], np.zeros((1, 1, 2, 2))))


# ---------------------------------------------------------------------------------------------------------
# RawVideoSequence
# ---------------------------------------------------------------------------------------------------------
def test_file_name_parsing():
    from compressai.datasets import VideoFormat, get_raw_video_file_info

    a = get_raw_video_file_info("a_208x176_30Hz_8bit_P420.yuv")
    assert (a["width"], a["height"], a["bitdepth"], a["format"]) == (208, 176, 8, VideoFormat.YUV420)
    assert a["framerate"] == Fraction(30) and a["extension"] == "yuv"
    b = get_raw_video_file_info("b_64x48_29.97fps_yuv420p10le.yuv")
    assert (b["width"], b["height"], b["bitdepth"], b["format"]) == (64, 48, 10, VideoFormat.YUV420)
    assert b["framerate"] == Fraction(30000, 1001) and b["endianness"] == "le"
    c = get_raw_video_file_info("c_1920x1080_50fps_I420_10LE.yuv")
    assert (c["bitdepth"], c["format"], c["framerate"]) == (10, VideoFormat.YUV420, Fraction(50))
    assert get_raw_video_file_info("d_16x8_24Hz_8bit_P444.yuv")["format"] == VideoFormat.YUV444
    with pytest.raises(ValueError, match="bit-depth twice"):
        get_raw_video_file_info("e_64x48_30Hz_8bit_yuv420p10le.yuv")


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_raw_sequence_reads_what_was_written(tmp_path, bitdepth):
    from compressai.datasets import RawVideoSequence, VideoFormat

    H, W, n = 6, 10, 3
    rng = np.random.default_rng(bitdepth)
    clip = [tuple(rng.integers(0, 2 ** bitdepth, size=s) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))
            for _ in range(n)]
    name = f"clip_{W}x{H}_30Hz_8bit_P420.yuv" if bitdepth == 8 else f"clip_{W}x{H}_29.97fps_yuv420p10le.yuv"
    path = tmp_path / name
    R.write_clip(path, clip, bitdepth)
    with open(path, "ab") as f:
        f.write(b"\x00" * 7)                 # a trailing partial frame is not a frame
    seq = RawVideoSequence.from_file(str(path))
    assert (seq.width, seq.height, seq.bitdepth, seq.format) == (W, H, bitdepth, VideoFormat.YUV420)
    assert len(seq) == n == seq.total_frms       # file bytes // frame bytes, the sample size on every plane
    for i in range(n):
        rec = seq[i]
        assert rec.dtype.names == ("y", "u", "v")
        for k, name in enumerate("yuv"):
            assert rec[name].dtype == (np.uint8 if bitdepth == 8 else np.uint16)
            assert np.array_equal(rec[name], clip[i][k])
    like = RawVideoSequence.new_like(seq, str(path))
    assert len(like) == n and np.array_equal(like[1]["v"], clip[1][2])
    with pytest.raises(RuntimeError, match="Could not get sequence information"):
        RawVideoSequence.from_file(str(tmp_path / "nosize_30Hz_8bit_P420.yuv"))
    # what the name lacks can be given
    bare = tmp_path / "bare.yuv"
    R.write_clip(bare, clip, bitdepth)
    seq2 = RawVideoSequence.from_file(str(bare), width=W, height=H, bitdepth=bitdepth, format=VideoFormat.YUV420)
    assert len(seq2) == n and np.array_equal(seq2[2]["y"], clip[2][0])


# ---------------------------------------------------------------------------------------------------------
# VideoFolder
# ---------------------------------------------------------------------------------------------------------
def test_video_folder(tmp_path):
    from PIL import Image

    from compressai.datasets import VideoFolder

    seq = tmp_path / "sequences" / "00001" / "0001"
    seq.mkdir(parents=True)
    for i in range(5):       # frame i is filled with the value 10 (i + 1)
        Image.fromarray(np.full((8, 12, 3), 10 * (i + 1), dtype=np.uint8)).save(seq / f"im{i + 1}.png")
    (tmp_path / "train.list").write_text("00001/0001\n")

    def transform(a):
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float()

    ds = VideoFolder(str(tmp_path), transform=transform, split="train")
    assert len(ds) == 1
    frames = ds[0]
    assert len(frames) == 3 and all(tuple(f.shape) == (3, 8, 12) for f in frames)
    assert [int(f[0, 0, 0]) for f in frames] == [10, 20, 30]
    five = VideoFolder(str(tmp_path), transform=transform, split="train", max_frames=5)[0]
    assert [int(f[0, 0, 0]) for f in five] == [10, 20, 30, 40, 50]
    two = VideoFolder(str(tmp_path), transform=transform, max_frames=2, rnd_interval=True)
    for _ in range(8):       # interval 1 .. (5 + 2) // 2 = 3: the second frame is 1, 2 or 3 steps on
        a, b = (int(f[0, 0, 0]) for f in two[0])
        assert a == 10 and b in (20, 30, 40)
    rev = VideoFolder(str(tmp_path), transform=transform, rnd_temp_order=True)
    seen = {tuple(int(f[0, 0, 0]) for f in rev[0]) for _ in range(40)}
    assert seen <= {(10, 20, 30), (30, 20, 10)} and len(seen) == 2
    with pytest.raises(RuntimeError, match="Transform must be applied"):
        VideoFolder(str(tmp_path))
    with pytest.raises(RuntimeError, match="Invalid file"):
        VideoFolder(str(tmp_path), transform=transform, split="test")


# ---------------------------------------------------------------------------------------------------------
# the container
# ---------------------------------------------------------------------------------------------------------
def test_container_round_trip_and_header_bytes():
    from compressai.utils.video.eval_model.__main__ import (read_body, read_bytes, read_header, read_uchars, read_uints,
                                                            write_body, write_bytes, write_header, write_uchars,
                                                            write_uints)

    fd = io.BytesIO()
    assert write_header(fd, 176, 208, 10, 3) == 13
    assert fd.getvalue() == bytes([0, 0, 0, 176, 0, 0, 0, 208, 10, 0, 0, 0, 3])
    strings = [[b"\x01\x02\x03"], [b""], [bytes(range(256)) * 3]]
    n = write_body(fd, (2, 1), strings)
    assert n == 12 + sum(4 + len(s[0]) for s in strings) == len(fd.getvalue()) - 13
    assert fd.getvalue()[13:25] == bytes([0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0, 3])
    write_body(fd, (7, 9), [[b"xyz"]])
    fd.seek(0)
    assert read_header(fd) == (176, 208, 10, 3)
    got, shape = read_body(fd)
    assert got == strings and tuple(shape) == (2, 1)
    got, shape = read_body(fd)
    assert got == [[b"xyz"]] and tuple(shape) == (7, 9)
    assert fd.read() == b""
    fd = io.BytesIO()
    assert write_uints(fd, (1, 2 ** 32 - 1)) == 8 and write_uchars(fd, (255,)) == 1 and write_bytes(fd, b"ab") == 2
    fd.seek(0)
    assert read_uints(fd, 2) == (1, 2 ** 32 - 1) and read_uchars(fd, 1) == (255,) and read_bytes(fd, 2) == b"ab"
    with pytest.raises(ValueError, match="truncated"):
        read_body(io.BytesIO(bytes([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 9, 65])))


# ---------------------------------------------------------------------------------------------------------
# the torch body of utils.video.frames against the restatement (the GPU test's tolerances)
# ---------------------------------------------------------------------------------------------------------
CASES = [(2, 2, 8, 128), (6, 10, 10, 128), (34, 70, 8, 128), (34, 70, 10, 1), (130, 258, 10, 128)]


@pytest.mark.parametrize("H,W,bitdepth,pad_to", CASES)
@pytest.mark.parametrize("mode", MODES)
def test_cpu_body_to_rgb(H, W, bitdepth, pad_to, mode):
    from compressai.utils.video import frames

    max_val = 2 ** bitdepth - 1
    planes = R.noise_planes(H, W, bitdepth, seed=H + bitdepth)
    ref = R.to_rgb(planes, bitdepth, mode, pad_to)
    x, padding, org_q = frames.yuv420_to_rgb(planes, bitdepth, mode, pad_to)
    assert padding == ref["padding"] and x.dtype == torch.float32 and tuple(x.shape) == (1, 3) + ref["x"].shape[1:]
    assert (x[0].double() - ref["x"]).abs().max().item() <= 4e-6
    left, right, top, bottom = padding
    frame = torch.zeros(x.shape[-2:], dtype=torch.bool)
    frame[top:top + H, left:left + W] = True
    assert (x[0][:, ~frame] == 0).all()
    check_levels(org_q, ref["org_q"], ref["level"], max_val, R.EPS_ORG)


def check_levels(q, q64, level, max_val, eps):
    """Integer-valued, equal to the fp64 rounding except by exactly 1 at near-tie elements; near ties <= 2 %."""
    q = q.detach().cpu().double()
    assert q.shape == q64.shape and (q == q.round()).all()
    tie = R.near_tie(level, max_val, eps)
    share = tie.double().mean().item()
    assert share <= R.TIE_SHARE, share
    diff = (q - q64).abs()
    assert (diff[~tie] == 0).all()
    assert (diff[tie] <= 1).all()
    return tie


@pytest.mark.parametrize("H,W,bitdepth,pad_to", CASES)
def test_cpu_body_metrics(H, W, bitdepth, pad_to):
    from compressai.utils.video import frames

    max_val = 2 ** bitdepth - 1
    planes = R.noise_planes(H, W, bitdepth, seed=H + bitdepth)
    x, padding, org_q = frames.yuv420_to_rgb(planes, bitdepth, "bicubic", pad_to)
    rec = R.noise_rec(x.shape[2], x.shape[3], seed=W)
    ref = R.frame_metrics(planes, org_q, rec, padding, bitdepth)
    assert max(ref["tie_share"]) <= R.TIE_SHARE
    sums = frames.frame_sse(planes, org_q, rec, padding, bitdepth)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (4,)
    for got, want, slack in zip(sums.tolist(), ref["sse"], ref["slack"]):
        assert abs(got - want) <= slack, (got, want, slack)
    out = frames.frame_metrics(planes, org_q, rec, padding, bitdepth)
    keys = {"psnr-y", "psnr-u", "psnr-v", "psnr-yuv", "mse-rgb", "psnr-rgb"}
    assert set(out) == (keys | {"ms-ssim-rgb"} if min(H, W) > 160 else keys)
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in out.values())
    for k, i in (("psnr-y", 0), ("psnr-u", 1), ("psnr-v", 2), ("psnr-rgb", 3)):
        assert abs(out[k].item() - ref[k]) <= R.psnr_slack(ref["sse"][i], ref["slack"][i]), k
    assert out["psnr-yuv"].item() == pytest.approx((4 * out["psnr-y"].item() + out["psnr-u"].item()
                                                    + out["psnr-v"].item()) / 6, abs=1e-9)
    assert out["mse-rgb"].item() == pytest.approx(sums[3].item() / (3 * H * W), rel=1e-12)


def test_cpu_body_numpy_record_and_ms_ssim():
    """A structured record goes in as it is; a frame with sides above 160 also gets ms-ssim-rgb."""
    from compressai.utils.metrics import _ms_ssim_torch
    from compressai.utils.video import frames

    H, W, bitdepth = 162, 164, 10
    planes = R.noise_planes(H, W, bitdepth, seed=9)
    dt = np.dtype([("y", np.uint16, (H, W)), ("u", np.uint16, (H // 2, W // 2)), ("v", np.uint16, (H // 2, W // 2))])
    rec = np.zeros((), dtype=dt)
    for name, p in zip("yuv", planes):
        rec[name] = p.numpy().view(np.uint16)
    got = frames.to_planes(rec)
    assert all(torch.equal(a, b) for a, b in zip(got, planes))
    x, padding, org_q = frames.yuv420_to_rgb(rec, bitdepth, "bicubic", 128)
    x2, _, org_q2 = frames.yuv420_to_rgb(planes, bitdepth, "bicubic", 128)
    assert torch.equal(x, x2) and torch.equal(org_q, org_q2)
    x_rec = (x + 0.02 * torch.randn(x.shape, generator=torch.Generator().manual_seed(1))).clamp(0, 1)
    out = frames.frame_metrics(rec, org_q, x_rec, padding, bitdepth)
    ref = R.frame_metrics(planes, org_q, x_rec, padding, bitdepth)
    want = _ms_ssim_torch(org_q[None], ref["rec_q"][None], data_range=1023.0, dtype=torch.float64).mean().item()
    assert out["ms-ssim-rgb"].dim() == 0 and abs(out["ms-ssim-rgb"].item() - want) <= 1e-4
    # three integer tensors of another dtype are the same frame
    wide = tuple((p.to(torch.int32) & 0xFFFF).to(torch.int64) for p in planes)
    assert torch.equal(frames.yuv420_to_rgb(wide, bitdepth, "bicubic", 128)[0], x)


def test_bad_frames_raise_before_any_work():
    from compressai.utils.video import frames

    odd = (torch.zeros(5, 6, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="even H and W"):
        frames.yuv420_to_rgb(odd, 8)
    ok = R.noise_planes(4, 6, 8, seed=0)
    with pytest.raises(ValueError, match="bit depth"):
        frames.yuv420_to_rgb(ok, 9)
    with pytest.raises(ValueError, match="Invalid upsampling mode"):
        frames.yuv420_to_rgb(ok, 8, mode="area")
    with pytest.raises(ValueError, match="plane u"):
        frames.yuv420_to_rgb((ok[0], ok[1][:1], ok[2]), 8)
    with pytest.raises(ValueError, match="integer tensors"):
        frames.yuv420_to_rgb(tuple(p.float() for p in ok), 8)
    x, padding, org_q = frames.yuv420_to_rgb(ok, 8)
    with pytest.raises(ValueError, match="reconstruction must be"):
        frames.frame_sse(ok, org_q, x[:, :, :-1], padding, 8)


def test_pretrained_is_refused():
    from compressai.utils.video.eval_model.__main__ import create_parser, load_pretrained

    with pytest.raises(RuntimeError, match="not available offline"):
        load_pretrained("ssf2020", "mse", 1)
    args = create_parser().parse_args(["checkpoint", "in", "out", "-a", "ssf2020", "-p", "a.pth.tar", "--half",
                                       "--entropy-estimation", "--keep_binaries", "-f", "-v", "-m", "mse", "--cuda"])
    assert args.paths == ["a.pth.tar"] and args.half and args.entropy_estimation and args.keep_binaries and args.force
    assert create_parser().parse_args(["pretrained", "in", "out", "-a", "ssf2020", "-q", "3", "1"]).qualities == [3, 1]
