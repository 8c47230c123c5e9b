"""The two frame kernels of csrc/video.hip against the fp64 restatement (tests/video_reference.py).

Shapes: 2x2 (every tap clamped), 6x10 (small interior), 34x70 (W/2 odd, no vector-width multiple), 130x258 (several
blocks: the cross-block sums).  pad_to = 128 and 1 (no padding); the centred offsets are odd for 34x70 and 130x258,
which takes the kernels' scalar path.

Model input: |err| <= 4e-6 per element (at most 16 fp32 roundings of intermediates below 4 in magnitude:
16 * 4 * 2^-24 = 3.8e-6), the padding exactly 0.  Levels (org_q, rec_q): integer-valued and equal to the fp64
rounding except, by exactly 1, where the fp64 level before rounding lies within max_val * eps of a half-integer
(eps 4e-6 for org_q, 1e-6 for what derives from the reconstruction, whose values are in [0, 1]); such elements are
at most 2 % of any case.  Sums: |sse - sse_fp64| <= sum over near-tie elements of 2 |d| + 1.

The near-tie share is a property of the seeded inputs and of the fp64 restatement alone (a 6x10 frame has 180 RGB
elements: four near ties are already 2.2 %); the seeds below are ones for which it holds in every case, and every
test asserts it again.
"""
import ctypes
import functools

import pytest
import torch

import video_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (6, 10), (34, 70), (130, 258)]
MODES = ("nearest", "bilinear", "bicubic")


@functools.lru_cache(maxsize=None)
def planes_of(H, W, bitdepth, kind="noise"):
    make = R.noise_planes if kind == "noise" else R.extreme_planes
    return make(H, W, bitdepth, seed=1000 * bitdepth + H + 1)


@functools.lru_cache(maxsize=None)
def rgb_ref(H, W, bitdepth, mode, pad_to, kind="noise"):
    return R.to_rgb(planes_of(H, W, bitdepth, kind), bitdepth, mode, pad_to)


def check_rgb(cuda, H, W, bitdepth, mode, pad_to, kind="noise"):
    from compressai.utils.video import frames

    max_val = 2 ** bitdepth - 1
    ref = rgb_ref(H, W, bitdepth, mode, pad_to, kind)
    planes = tuple(p.to(cuda) for p in planes_of(H, W, bitdepth, kind))
    x, padding, org_q = frames.yuv420_to_rgb(planes, bitdepth, mode, pad_to)
    assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (1, 3) + tuple(ref["x"].shape[1:])
    assert padding == ref["padding"]
    x, org_q = x.cpu(), org_q.cpu()
    err = (x[0].double() - ref["x"]).abs().max().item()
    left, right, top, bottom = padding
    frame = torch.zeros(x.shape[-2:], dtype=torch.bool)
    frame[top:top + H, left:left + W] = True
    tie = R.near_tie(ref["level"], max_val, R.EPS_ORG)
    share = tie.double().mean().item()
    diff = (org_q.double() - ref["org_q"]).abs()
    print(f"{H}x{W} {bitdepth} bit {mode} pad {pad_to} {kind}: x err {err:.2e}, near ties {share:.4f}, "
          f"levels off by one {int((diff == 1).sum())}")
    assert err <= 4e-6
    assert (x[0][:, ~frame] == 0).all()
    assert (org_q == org_q.round()).all() and org_q.min() >= 0 and org_q.max() <= max_val
    assert share <= R.TIE_SHARE
    assert (diff[~tie] == 0).all() and (diff[tie] <= 1).all()
    return ref


@pytest.mark.parametrize("pad_to", [128, 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bitdepth", [8, 10])
@pytest.mark.parametrize("H,W", SHAPES)
def test_model_input_and_levels(cuda, H, W, bitdepth, mode, pad_to):
    check_rgb(cuda, H, W, bitdepth, mode, pad_to)


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_extreme_planes_overshoot_and_clamp(cuda, bitdepth):
    """Planes of 0 and max_val only: the bicubic overshoots [0, 1] and the levels' clamp acts on both sides."""
    ref = check_rgb(cuda, 34, 70, bitdepth, "bicubic", 128, kind="extreme")
    max_val = 2 ** bitdepth - 1
    frame = ref["x"][:, ref["padding"][2]:ref["padding"][2] + 34, ref["padding"][0]:ref["padding"][0] + 70]
    assert frame.min() < -0.05 and frame.max() > 1.05
    assert (ref["org_q"] == 0).any() and (ref["org_q"] == max_val).any()


def run_sse(cuda, H, W, bitdepth, pad_to, kind="noise"):
    from compressai import _ops
    from compressai.utils.video import frames

    planes = tuple(p.to(cuda) for p in planes_of(H, W, bitdepth, kind))
    x, padding, org_q = frames.yuv420_to_rgb(planes, bitdepth, "bicubic", pad_to)
    rec = R.noise_rec(x.shape[2], x.shape[3], seed=H + W + bitdepth + 1)
    ref = R.frame_metrics(planes_of(H, W, bitdepth, kind), org_q, rec, padding, bitdepth)
    sums, rec_q = _ops.video_frame_sse(planes, bitdepth, org_q, rec.to(cuda), padding[2], padding[0])
    again = frames.frame_sse(planes, org_q, rec.to(cuda), padding, bitdepth)
    return planes, org_q, rec, padding, ref, sums, rec_q, again


@pytest.mark.parametrize("pad_to", [128, 1])
@pytest.mark.parametrize("bitdepth", [8, 10])
@pytest.mark.parametrize("H,W", SHAPES)
def test_sums_and_rec_levels(cuda, H, W, bitdepth, pad_to):
    max_val = 2 ** bitdepth - 1
    planes, org_q, rec, padding, ref, sums, rec_q, again = run_sse(cuda, H, W, bitdepth, pad_to)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (4,)
    assert torch.equal(sums, again), "two calls on the same inputs differ"
    rec_q = rec_q.cpu().double()
    diff = (rec_q - ref["rec_q"]).abs()
    print(f"{H}x{W} {bitdepth} bit pad {pad_to}: sse {sums.tolist()} fp64 {ref['sse']} slack {ref['slack']} "
          f"near ties {[round(s, 4) for s in ref['tie_share']]}, rec levels off by one {int((diff == 1).sum())}")
    assert (rec_q == rec_q.round()).all() and rec_q.min() >= 0 and rec_q.max() <= max_val
    assert max(ref["tie_share"]) <= R.TIE_SHARE
    assert (diff[~ref["rec_tie"]] == 0).all() and (diff[ref["rec_tie"]] <= 1).all()
    for got, want, slack in zip(sums.tolist(), ref["sse"], ref["slack"]):
        assert abs(got - want) <= slack, (got, want, slack)


def test_extreme_planes_sums(cuda):
    planes, org_q, rec, padding, ref, sums, rec_q, again = run_sse(cuda, 34, 70, 10, 128, kind="extreme")
    assert torch.equal(sums, again)
    for got, want, slack in zip(sums.tolist(), ref["sse"], ref["slack"]):
        assert abs(got - want) <= slack, (got, want, slack)


def test_sums_match_the_cpu_body(cuda):
    """The 130x258 case: the kernel's sums against the torch body on the CPU, within the near-tie rule; the metrics
    dict holds 0-dim device tensors, without ms-ssim-rgb below 161 pixels."""
    from compressai.utils.video import frames

    planes, org_q, rec, padding, ref, sums, rec_q, _ = run_sse(cuda, 130, 258, 10, 128)
    cpu = frames.frame_sse(tuple(p.cpu() for p in planes), org_q.cpu(), rec, padding, 10)
    print(f"gpu {sums.tolist()} cpu body {cpu.tolist()} fp64 {ref['sse']} slack {ref['slack']}")
    for got, want, slack in zip(sums.tolist(), cpu.tolist(), ref["slack"]):
        assert abs(got - want) <= slack, (got, want, slack)
    out = frames.frame_metrics(planes, org_q, rec.to(cuda), padding, 10)
    assert set(out) == {"psnr-y", "psnr-u", "psnr-v", "psnr-yuv", "mse-rgb", "psnr-rgb"}
    assert all(v.is_cuda and v.dim() == 0 for v in out.values())
    for k, i in (("psnr-y", 0), ("psnr-u", 1), ("psnr-v", 2), ("psnr-rgb", 3)):
        assert abs(out[k].item() - ref[k]) <= R.psnr_slack(ref["sse"][i], ref["slack"][i]), k


def test_odd_frames_raise_before_any_launch(cuda):
    from compressai import _ledger
    from compressai.utils.video import frames

    odd = tuple(torch.zeros(s, dtype=torch.uint8, device=cuda) for s in ((6, 5), (3, 2), (3, 2)))
    with _ledger.recording(keep_replay=False) as led:
        with pytest.raises(ValueError, match="even H and W"):
            frames.yuv420_to_rgb(odd, 8)
    assert not led.entries


def test_einval_through_the_c_abi():
    """Validation precedes any device work: the pointers are not device memory, so a call that got past it to a
    launch could not return CAI_EINVAL."""
    from compressai import _native

    lib = _native.lib.load()
    P = ctypes.c_void_p(4096)

    def rgb(y=P, u=P, v=P, H=4, W=6, bits=8, mode=2, out=P, Hp=8, Wp=8, top=2, left=1):
        return lib.cai_yuv420_to_rgb(y, u, v, H, W, bits, mode, out, Hp, Wp, top, left, None, None)

    def sse(y=P, u=P, v=P, H=4, W=6, bits=8, org=P, rec=P, Hp=8, Wp=8, top=2, left=1, sums=P):
        return lib.cai_video_frame_sse(y, u, v, H, W, bits, org, rec, Hp, Wp, top, left, sums, None, None)

    for call in (rgb, sse):
        for kw, fragment in (({"W": 5}, b"even"), ({"H": 0}, b"even"), ({"bits": 9}, b"bit depth"),
                             ({"left": 3}, b"does not fit"), ({"top": -1}, b"negative padding"),
                             ({"Hp": 3}, b"does not fit"), ({"u": None}, b"null plane"), ({"y": None}, b"null plane")):
            rc = call(**kw)
            msg = lib.cai_last_error()
            assert rc == _native.CAI_EINVAL, (call.__name__, kw, rc, msg)
            assert fragment in msg, (call.__name__, kw, msg)
    assert rgb(mode=3) == _native.CAI_EINVAL and b"unknown upsampling mode" in lib.cai_last_error()
    assert rgb(out=None) == _native.CAI_EINVAL and b"null output" in lib.cai_last_error()
    assert sse(sums=None) == _native.CAI_EINVAL and b"null pointer" in lib.cai_last_error()
    with pytest.raises(ValueError, match="bit depth 9"):
        _native.lib.cai_yuv420_to_rgb(P, P, P, 4, 6, 9, 2, P, 8, 8, 2, 1, None, None)
