"""The video branch of compressai.utils.codec_rgbt on the GPU: rgb_to_yuv420_kernel (csrc/video.hip) against the
fp64 levels, against the levels the frame-sse kernel measures, at the C ABI, and the codec end to end.

Kernel: the sixteen cases of tests/codec_video_cases.py under its level rule (equal to the rounded fp64 level, off by
exactly 1 only within max_val * 1e-6 of a tie, such elements at most 2 % of a plane).  34x70 has odd centred offsets
(the scalar loads), pad_to = 1 the aligned float2 loads; 130x258 spans several blocks.

Same levels as the metrics: the integer sums of squared differences between the written planes and the source
planes, formed on the host, equal video_frame_sse's Y, U, V sums exactly -- both kernels take their levels from one
device function, whose one contractible expression is written with explicit fused steps (a form of it that left the
contraction to the compiler passed the noise cases here and missed the end-to-end equality below by two Y levels at
10 bit: the two call sites had been contracted differently).

End to end: the clip of test_video_eval_gpu.py (3 frames, 208x176, 8 and 10 bit) and its livened ssf2020(1).
encode_video's stream is eval_model's behind two bytes; decode_video's file holds, frame by frame, the levels of the
frames decode_sequence returns, and its PSNR-Y/U/V against the source are eval_model's (1e-9: the same integers
through the same fp64 formula).
"""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import codec_video_cases as C
import video_reference as R
from test_video_eval_gpu import NAMES, H, N, W, liven

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_to", C.PADS)
@pytest.mark.parametrize("bitdepth", C.BITDEPTHS)
@pytest.mark.parametrize("h,w", C.SHAPES)
def test_kernel_levels(cuda, h, w, bitdepth, pad_to):
    from compressai.utils.video import frames

    rec, padding = C.rec_of(h, w, bitdepth, pad_to)
    planes = frames.rgb_to_yuv420(rec.to(cuda), padding, bitdepth)
    again = frames.rgb_to_yuv420(rec.to(cuda), padding, bitdepth)
    y, u, v = planes
    assert planes.buffer.is_cuda and planes.buffer.dim() == 1 and planes.buffer.numel() == h * w * 3 // 2
    assert planes.buffer.dtype == (torch.uint8 if bitdepth == 8 else torch.int16)
    assert tuple(y.shape) == (h, w) and tuple(u.shape) == tuple(v.shape) == (h // 2, w // 2)
    assert all(p.untyped_storage().data_ptr() == planes.buffer.untyped_storage().data_ptr() for p in planes)
    assert torch.equal(planes.buffer, again.buffer), "two calls on the same input differ"
    shares, off = C.check_levels(planes, C.levels_of(h, w, bitdepth, pad_to), bitdepth, "kernel")
    print(f"{h}x{w} {bitdepth} bit pad {pad_to}: near ties {[round(s, 4) for s in shares]}, levels off by one {off}")


def test_kernel_takes_other_float_types_and_refuses_before_any_launch(cuda):
    from compressai import _ledger
    from compressai.utils.video import frames

    rec, padding = C.rec_of(6, 10, 8, 128)
    want = frames.rgb_to_yuv420(rec.to(cuda), padding, 8)
    half = rec.to(cuda).bfloat16()
    assert torch.equal(frames.rgb_to_yuv420(half, padding, 8).buffer, frames.rgb_to_yuv420(half.float(), padding, 8).buffer)
    assert torch.equal(frames.rgb_to_yuv420(rec.to(cuda).double(), padding, 8).buffer, want.buffer)
    with _ledger.recording(keep_replay=False) as led:
        with pytest.raises(ValueError, match="even H and W"):
            frames.rgb_to_yuv420(torch.zeros(1, 3, 8, 8, device=cuda), (0, 1, 0, 0), 8)
        with pytest.raises(ValueError, match="bit depth 9"):
            frames.rgb_to_yuv420(torch.zeros(1, 3, 8, 8, device=cuda), (0, 0, 0, 0), 9)
        with pytest.raises(ValueError, match=r"\[1, 3, Hp, Wp\]"):
            frames.rgb_to_yuv420(torch.zeros(3, 8, 8, device=cuda), (0, 0, 0, 0), 8)
    assert not led.entries


def test_16_bit_words_are_unsigned(cuda):
    """34x70 of 2 x 2 blocks whose channels are all 0 or all 1, with values pushed past [0, 1] so that the clamp
    acts: every Y level is 0 or 65535, far from any tie, and must equal the restatement exactly when the words are
    read as unsigned.  (U and V are 0.5 max_val there: a tie at every bit depth, not compared.)"""
    from compressai.utils.video import frames

    h, w = 34, 70
    Hp, Wp, padding = R.pad_geometry(h, w, 128)
    rec = C.block_rec(Hp, Wp, seed=16) * 1.5 - 0.25
    assert rec.min() < 0 and rec.max() > 1
    want = C.yuv_levels(rec, padding, 16)[0]
    assert set(want.unique().tolist()) == {0.0, 65535.0}
    assert not R.near_tie(want, 65535, R.EPS_REC).any()
    planes = frames.rgb_to_yuv420(rec.to(cuda), padding, 16)
    assert planes[0].dtype == torch.int16
    y = planes[0].cpu().numpy().view(np.uint16).astype(np.int64)
    assert (y == want.numpy().astype(np.int64)).all()
    assert (planes[0].cpu() < 0).any()      # 65535 is -1 in the container: signed reading would have failed above


@pytest.mark.parametrize("bitdepth", C.BITDEPTHS)
def test_written_levels_are_the_measured_levels(cuda, bitdepth):
    from compressai import _ops
    from compressai.utils.video import frames

    h, w = 130, 258
    src = R.noise_planes(h, w, bitdepth, seed=1000 * bitdepth + h + 1)
    planes = tuple(p.to(cuda) for p in src)
    for pad_to in C.PADS:
        rec, padding = C.rec_of(h, w, bitdepth, pad_to)
        _, _, org_q = frames.yuv420_to_rgb(planes, bitdepth, "bicubic", pad_to)
        sums, _ = _ops.video_frame_sse(planes, bitdepth, org_q, rec.to(cuda), padding[2], padding[0])
        written = frames.rgb_to_yuv420(rec.to(cuda), padding, bitdepth)
        got = C.sse(tuple(p.cpu() for p in written), src)
        print(f"{bitdepth} bit pad {pad_to}: sse of the written planes {got}, video_frame_sse {sums.tolist()[:3]}")
        assert got == sums.tolist()[:3]


def test_einval_through_the_c_abi():
    """Validation precedes any device work: the pointers are not device memory, so a call that got past it to a
    launch could not return CAI_EINVAL."""
    from compressai import _native

    lib = _native.lib.load()
    P = ctypes.c_void_p(4096)

    def call(rec=P, Hp=8, Wp=8, top=2, left=1, H=4, W=6, bits=8, out=P):
        return lib.cai_rgb_to_yuv420(rec, Hp, Wp, top, left, H, W, bits, out, None)

    for kw, fragment in (({"W": 5}, b"even"), ({"H": 0}, b"even"), ({"bits": 9}, b"bit depth"),
                         ({"left": 3}, b"does not fit"), ({"Hp": 3}, b"does not fit"),
                         ({"top": -1}, b"negative padding"), ({"rec": None}, b"null pointer"),
                         ({"out": None}, b"null pointer"),
                         ({"bits": 10, "out": ctypes.c_void_p(4097)}, b"2-byte aligned")):
        rc = call(**kw)
        msg = lib.cai_last_error()
        assert rc == _native.CAI_EINVAL, (kw, rc, msg)
        assert fragment in msg and b"rgb_to_yuv420" in msg, (kw, msg)
    with pytest.raises(ValueError, match="bit depth 9"):
        _native.lib.cai_rgb_to_yuv420(P, 8, 8, 2, 1, 4, 6, 9, P, None)


# ---------------------------------------------------------------------------------------------------------
# the codec end to end
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(cuda):
    from compressai.zoo import ssf2020

    torch.manual_seed(0)
    model = liven(ssf2020(1)).to(cuda).eval()
    model.update(force=True)
    return model


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """{bitdepth: (path, [frames of integer planes])}"""
    root = tmp_path_factory.mktemp("codec_clips")
    out = {}
    for bitdepth in (8, 10):
        clip = R.moving_clip(H, W, N, bitdepth, seed=bitdepth)
        path = root / NAMES[bitdepth]
        R.write_clip(path, clip, bitdepth)
        out[bitdepth] = (path, clip)
    return out


@pytest.fixture(scope="module")
def coded(net, clips, tmp_path_factory):
    """{bitdepth: everything one run of the codec and of eval_model on the clip leaves behind}"""
    from compressai.utils.codec_rgbt import decode_video, encode_video
    from compressai.utils.video.eval_model.__main__ import decode_sequence, eval_model

    root = tmp_path_factory.mktemp("codec_bins")
    out = {}
    for bitdepth, (path, _) in clips.items():
        a, b, rec = root / f"a{bitdepth}.bin", root / f"b{bitdepth}.bin", root / f"rec{bitdepth}_{W}x{H}.yuv"
        enc = encode_video(str(path), net, str(a), "mse", 3)
        results = eval_model(net, path, b, keep_binaries=True)
        hdr, last = decode_video(str(a), net, str(rec))
        out[bitdepth] = {"a": a, "b": b, "rec": rec, "enc": enc, "results": results, "hdr": hdr, "last": last,
                         "decoded": decode_sequence(net, b)}
    return out


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_stream_is_the_evaluations_behind_two_bytes(coded, bitdepth):
    c = coded[bitdepth]
    a, b = c["a"].read_bytes(), c["b"].read_bytes()
    assert a[:2] == bytes([6, 2])                       # ssf2020; mse << 4 | quality 3 - 1
    assert a[2:] == b
    assert struct.unpack(">IIBI", a[2:15]) == (H, W, bitdepth, N)
    enc = c["enc"]
    assert set(enc) == {"bpp", "frames", "avg_frm_enc_time"} and enc["frames"] == N and enc["avg_frm_enc_time"] > 0
    assert enc["bpp"] == len(a) * 8 / (H * W * N)


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_decoded_file_holds_the_measured_levels(cuda, coded, clips, bitdepth):
    from compressai.utils.video import frames

    c = coded[bitdepth]
    max_val = 2 ** bitdepth - 1
    assert c["hdr"] == ("ssf2020", "mse", 3, (H, W), bitdepth, N)
    data = c["rec"].read_bytes()
    assert len(data) == N * H * W * 3 // 2 * (1 if bitdepth == 8 else 2)
    written = C.parse_frames(data, H, W, bitdepth)
    assert len(written) == len(c["decoded"]) == N
    assert tuple(c["last"].shape) == (1, 3, H, W) and torch.equal(c["last"], c["decoded"][-1])
    psnr = {k: [] for k in "yuv"}
    for planes, x, src in zip(written, c["decoded"], clips[bitdepth][1]):
        direct = frames.rgb_to_yuv420(x, (0, 0, 0, 0), bitdepth)
        for got, want in zip(planes, direct):
            assert (got == R.f64(want).numpy().astype(np.int64)).all()
        src_dev = tuple(R.as_container(p, bitdepth).to(cuda) for p in src)
        _, _, org_q = frames.yuv420_to_rgb(src_dev, bitdepth, "bicubic", 1)
        sums = frames.frame_sse(src_dev, org_q, x, (0, 0, 0, 0), bitdepth).tolist()
        got = C.sse(planes, src)
        assert got == sums[:3]
        for k, s, n in zip("yuv", got, (H * W, H * W // 4, H * W // 4)):
            assert s > 0
            psnr[k].append(20 * math.log10(max_val) - 10 * math.log10(s / n))
    for k in "yuv":
        mean = sum(psnr[k]) / N
        print(f"{bitdepth} bit psnr-{k}: decoded file {mean:.9f}, eval_model {c['results'][f'psnr-{k}']:.9f}")
        assert abs(mean - c["results"][f"psnr-{k}"]) <= 1e-9


def test_decoding_to_an_image_and_a_short_stream(coded, net, tmp_path):
    from PIL import Image

    from compressai.utils.codec_rgbt import decode_video, torch2img

    c = coded[8]
    hdr, last = decode_video(str(c["a"]), net, str(tmp_path / "last.png"))
    assert hdr.frames == N and torch.equal(last, c["last"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "last.png")), np.asarray(torch2img(last)))
    hdr, last = decode_video(str(c["a"]), net)                   # no output: nothing is written
    assert torch.equal(last, c["last"])
    a = c["a"].read_bytes()
    (tmp_path / "short.bin").write_bytes(a[:-3])
    with pytest.raises(ValueError, match="truncated"):
        decode_video(str(tmp_path / "short.bin"), net, str(tmp_path / "short.yuv"))
    (tmp_path / "image.bin").write_bytes(bytes([1]) + a[1:])     # the id of an image model
    with pytest.raises(ValueError, match="not a video model"):
        decode_video(str(tmp_path / "image.bin"), net)


def test_cli(cuda, coded, clips, net, tmp_path):
    from compressai.utils.codec_rgbt import main, write_stream

    c = coded[8]
    clip = str(clips[8][0])
    ckpt = tmp_path / "ssf-test.pth.tar"
    torch.save(net.state_dict(), ckpt)
    common = ["--model", "ssf2020", "--path", str(ckpt)]
    main(["encode", clip] + common + ["-o", str(tmp_path / "c.bin")])
    assert (tmp_path / "c.bin").read_bytes() == c["a"].read_bytes()
    main(["encode", clip] + common + ["-f", "2", "-o", str(tmp_path / "c2.bin")])
    two = (tmp_path / "c2.bin").read_bytes()
    assert struct.unpack(">BBIIBI", two[:15]) == (6, 2, H, W, 8, 2)
    assert c["a"].read_bytes()[15:len(two)] == two[15:]                # the first two frames' bodies
    rec2 = tmp_path / f"rec2_{W}x{H}.yuv"
    main(["decode", str(tmp_path / "c2.bin")] + common + ["-o", str(rec2)])
    frame_bytes = H * W * 3 // 2
    assert rec2.read_bytes() == c["rec"].read_bytes()[:2 * frame_bytes]
    with pytest.raises(ValueError, match="4 frames asked for"):
        main(["encode", clip] + common + ["-f", "4", "-o", str(tmp_path / "c4.bin")])
    with (tmp_path / "image.bin").open("wb") as f:
        write_stream(f, "bmshj2018-hyperprior", "mse", 3, (64, 64), {"shape": (4, 4), "strings": [[b"ab"], [b"c"]]})
    with pytest.raises(ValueError, match="bmshj2018-hyperprior"):
        main(["decode", str(tmp_path / "image.bin")] + common + ["-o", str(tmp_path / "x.yuv")])
    with pytest.raises(ValueError, match="ssf2020"):
        main(["decode", str(tmp_path / "c.bin"), "--model", "bmshj2018-hyperprior", "--path", str(ckpt), "-o",
              str(tmp_path / "x.png")])
