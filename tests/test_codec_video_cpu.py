"""The video branch of compressai.utils.codec_rgbt on the CPU: the stream's header bytes, the torch body of
frames.rgb_to_yuv420 against the fp64 levels under the level rule (tests/codec_video_cases.py), write_frame's bytes,
the argument errors and the parser."""
import io
import struct

import numpy as np
import pytest
import torch

import codec_video_cases as C
import video_reference as R


def _bodies():
    return [((4, 5), [[bytes(range(9))], [b"\x00\xffz"]]), ((2, 3), [[b"m" * 5], [b""]]), ((2, 3), [[b"r"], [b"zz"]])]


def test_video_header_bytes_and_truncation():
    from compressai.utils import codec_rgbt as K
    from compressai.utils.video.eval_model.__main__ import read_body, write_body

    buf = io.BytesIO()
    n = K.write_video_header(buf, "ms-ssim", 4, 176, 208, 10, 3)
    head = buf.getvalue()
    assert n == len(head) == 15
    assert head == struct.pack(">BBIIBI", 6, (1 << 4) | 3, 176, 208, 10, 3)
    for shape, strings in _bodies():
        write_body(buf, shape, strings)
    data = buf.getvalue()

    f = io.BytesIO(data)
    hdr = K.read_video_header(f)
    assert hdr == ("ssf2020", "ms-ssim", 4, (176, 208), 10, 3)
    assert hdr.frames == 3 and hdr.bitdepth == 10 and hdr.original_size == (176, 208)
    for shape, strings in _bodies():
        got, got_shape = read_body(f)
        assert got == strings and tuple(got_shape) == shape
    assert f.read() == b""

    for cut in range(len(head)):
        with pytest.raises(ValueError):
            K.read_video_header(io.BytesIO(head[:cut]))
    for cut in range(len(head), len(data)):       # every cut inside a body: some read of it comes up short
        f = io.BytesIO(data[:cut])
        K.read_video_header(f)
        with pytest.raises(ValueError, match="truncated"):
            for _ in _bodies():
                read_body(f)


def test_video_reader_refuses_other_models():
    from compressai.utils import codec_rgbt as K

    buf = io.BytesIO()
    K.write_stream(buf, "bmshj2018-hyperprior", "mse", 3, (64, 64), {"shape": (4, 4), "strings": [[b"ab"], [b"c"]]})
    with pytest.raises(ValueError, match="not a video model"):
        K.read_video_header(io.BytesIO(buf.getvalue()))
    with pytest.raises(ValueError, match="not a video model"):
        K.write_video_header(io.BytesIO(), "mse", 3, 64, 64, 8, 1, model="mbt2018")
    with pytest.raises(ValueError):
        K.read_video_header(io.BytesIO(bytes([42, 0]) + bytes(13)))


@pytest.mark.parametrize("pad_to", C.PADS)
@pytest.mark.parametrize("bitdepth", C.BITDEPTHS)
@pytest.mark.parametrize("H,W", C.SHAPES)
def test_torch_body_levels(H, W, bitdepth, pad_to):
    from compressai.utils.video import frames

    rec, padding = C.rec_of(H, W, bitdepth, pad_to)
    planes = frames.rgb_to_yuv420(rec, padding, bitdepth)
    direct = frames.rgb_to_yuv420_torch(rec, padding, bitdepth)
    y, u, v = planes
    assert tuple(y.shape) == (H, W) and tuple(u.shape) == tuple(v.shape) == (H // 2, W // 2)
    assert all(p.dtype == (torch.uint8 if bitdepth == 8 else torch.int16) for p in planes)
    assert all(torch.equal(a, b) for a, b in zip(planes, direct))
    assert planes.buffer.dim() == 1 and planes.buffer.numel() == H * W * 3 // 2
    assert torch.equal(planes.buffer, torch.cat([p.reshape(-1) for p in planes]))
    shares, off = C.check_levels(planes, C.levels_of(H, W, bitdepth, pad_to), bitdepth, "torch body")
    print(f"{H}x{W} {bitdepth} bit pad {pad_to}: near ties {[round(s, 4) for s in shares]}, levels off by one {off}")


def test_torch_body_casts_other_float_types():
    from compressai.utils.video import frames

    rec, padding = C.rec_of(6, 10, 8, 128)
    want = frames.rgb_to_yuv420(rec.double().float(), padding, 8)
    got = frames.rgb_to_yuv420(rec.double(), padding, 8)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("bitdepth", [8, 10, 16])
def test_write_frame_bytes(bitdepth):
    from compressai.utils.video import frames

    H, W = 4, 6
    max_val = 2 ** bitdepth - 1
    rng = np.random.default_rng(bitdepth)
    arrays = [rng.integers(0, max_val + 1, size=s) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
    arrays[0][0, 0], arrays[0][0, 1] = max_val, 0x0102 & max_val
    planes = tuple(R.as_container(a, bitdepth) for a in arrays)
    dt = np.uint8 if bitdepth == 8 else np.dtype("<u2")
    want = b"".join(a.astype(dt).tobytes() for a in arrays)
    assert len(want) == H * W * 3 // 2 * (1 if bitdepth == 8 else 2)

    out = io.BytesIO()
    assert frames.write_frame(out, planes, bitdepth) == len(want)        # three planes
    assert out.getvalue() == want
    whole = frames.FramePlanes(torch.cat([p.reshape(-1) for p in planes]), H, W)
    assert all(torch.equal(a, b) for a, b in zip(whole, planes))
    for arg in (whole, whole.buffer):                                    # what rgb_to_yuv420 returns; its buffer
        out = io.BytesIO()
        assert frames.write_frame(out, arg, bitdepth) == len(want)
        assert out.getvalue() == want
    if bitdepth > 8:
        assert want[:2] == struct.pack("<H", max_val) and want[2:4] == struct.pack("<H", 0x0102 & max_val)
    got = C.parse_frames(want + want, H, W, bitdepth)
    assert len(got) == 2 and all((g == a).all() for g, a in zip(got[1], arrays))

    with pytest.raises(ValueError, match="bit depth 9"):
        frames.write_frame(io.BytesIO(), planes, 9)
    with pytest.raises(ValueError, match="integers"):
        frames.write_frame(io.BytesIO(), torch.zeros(36), 8)


def test_argument_errors():
    from compressai.utils.video import frames

    rec = torch.zeros(1, 3, 8, 8)
    for fn in (frames.rgb_to_yuv420, frames.rgb_to_yuv420_torch):
        with pytest.raises(ValueError, match="even H and W"):
            fn(rec, (0, 0, 1, 0), 8)            # H = 7
        with pytest.raises(ValueError, match="even H and W"):
            fn(rec, (2, 1, 0, 0), 8)            # W = 5
        with pytest.raises(ValueError, match="even H and W"):
            fn(rec, (4, 4, 0, 0), 8)            # W = 0
        with pytest.raises(ValueError, match="bit depth 9"):
            fn(rec, (0, 0, 0, 0), 9)
        for bad in (torch.zeros(3, 8, 8), torch.zeros(1, 1, 8, 8), torch.zeros(2, 3, 8, 8)):
            with pytest.raises(ValueError, match=r"\[1, 3, Hp, Wp\]"):
                fn(bad, (0, 0, 0, 0), 8)
        with pytest.raises(ValueError, match="padding"):
            fn(rec, (0, 0, -2, 0), 8)
    with pytest.raises(ValueError, match="samples"):
        frames.FramePlanes(torch.zeros(35, dtype=torch.uint8), 4, 6)
    assert {"rgb_to_yuv420", "rgb_to_yuv420_torch", "write_frame"} <= set(frames.__all__)


def test_encode_video_refuses_other_inputs(tmp_path):
    from compressai.utils import codec_rgbt as K

    with pytest.raises(NotImplementedError, match="extension"):
        K.encode_video(str(tmp_path / "clip.mp4"), None, str(tmp_path / "o.bin"))
    path = tmp_path / "clip_4x4_30fps_yuv444_8bit.yuv"
    path.write_bytes(bytes(48))
    with pytest.raises(NotImplementedError, match="format"):
        K.encode_video(str(path), None, str(tmp_path / "o.bin"))
    path = tmp_path / "clip_4x4_30fps_420_8bit.yuv"
    path.write_bytes(bytes(24 * 2))
    with pytest.raises(ValueError, match="3 frames asked for"):
        K.encode_video(str(path), None, str(tmp_path / "o.bin"), num_frames=3)
    assert not (tmp_path / "o.bin").exists()


def test_parser_takes_a_frame_count():
    from compressai.utils.codec_rgbt import decode_parser, encode_parser

    base = ["clip.yuv", "--model", "ssf2020", "--path", "c.pth", "-o", "o.bin"]
    assert encode_parser().parse_args(base).num_of_frames == -1
    assert encode_parser().parse_args(base + ["-f", "2"]).num_of_frames == 2
    assert encode_parser().parse_args(base + ["--num_of_frames", "7"]).num_of_frames == 7
    assert decode_parser().parse_args(["o.bin", "--model", "ssf2020", "--path", "c.pth", "-o", "r.yuv"]).model == "ssf2020"
