"""python -m compressai.utils.video.eval_model end to end on the GPU: file -> container -> reconstruction -> numbers.

One clip of 3 frames, 208x176 (padded to 256x256, the smallest the 5-scale MS-SSIM accepts), a smooth seeded
pattern drifting a few pixels per frame plus noise, written once as 8-bit and once as 10-bit.  The net is ssf2020(1)
with seeded weights, livened so that the latents span several symbols and the flow moves.

The PSNRs are recomputed from the frames ``decode_sequence`` returns by the fp64 restatement
(tests/video_reference.py) and must agree within what the near-tie rule of test_video_frames_gpu.py permits:
|dPSNR| <= 10 log10((sse + slack) / (sse - slack)).  That the decoder reproduces the encoder bit for bit is
tests/test_ssf_model_gpu.py's.

ms-ssim-rgb against metrics._ms_ssim_torch in fp64 on the same levels, data_range = max_val: the bound is
tests/test_msssim_gpu.py's for the op against fp64 (1e-5).  Measured on MI355X on these frames: see
profiles/video_eval.log.
"""
import json
import math
import struct

import pytest
import torch

import video_reference as R

pytestmark = pytest.mark.gpu

H, W, N, FPS = 176, 208, 3, 30
NAMES = {8: f"clip_{W}x{H}_{FPS}Hz_8bit_P420.yuv", 10: f"clip_{W}x{H}_{FPS}fps_yuv420p10le.yuv"}
PSNR_KEYS = (("psnr-y", 0), ("psnr-u", 1), ("psnr-v", 2), ("psnr-rgb", 3))
MSSSIM_BOUND = 1e-5


def liven(net):
    """The default initialisation leaves every latent inside (-0.1, 0.1) and the flow at zero: nothing would round
    or move.  Scale the last encoder layers, lift the scale decoders into QReLU's range and give the motion decoder
    a real displacement (the same edits as tests/test_ssf_model_gpu.py makes)."""
    with torch.no_grad():
        for s in ("img", "res", "motion"):
            getattr(net, f"{s}_encoder")[6].weight.mul_(40.0)
            hs = getattr(net, f"{s}_hyperprior").hyper_decoder_scale
            hs.deconv1.bias.add_(0.3)
            hs.deconv2.bias.add_(0.3)
            hs.deconv3.weight.mul_(8.0)
            hs.deconv3.bias.add_(0.6)
            getattr(net, f"{s}_hyperprior").hyper_decoder_mean[4].weight.mul_(8.0)
        net.img_decoder[6].bias.add_(0.45)
        net.motion_decoder[6].weight.mul_(6.0)
        net.motion_decoder[6].bias.copy_(torch.tensor([0.04, -0.03, 0.15]))
    return net


@pytest.fixture(scope="module")
def net(cuda):
    from compressai.zoo import ssf2020

    torch.manual_seed(0)
    model = liven(ssf2020(1)).to(cuda).eval()
    model.update(force=True)
    return model


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """{bitdepth: (path, [frames of integer planes])}; both files in one directory."""
    root = tmp_path_factory.mktemp("clips")
    out = {}
    for bitdepth in (8, 10):
        frames = R.moving_clip(H, W, N, bitdepth, seed=bitdepth)
        path = root / NAMES[bitdepth]
        R.write_clip(path, frames, bitdepth)
        out[bitdepth] = (path, frames)
    return out


@pytest.fixture(scope="module")
def coded(net, clips, tmp_path_factory):
    """{bitdepth: (results of eval_model(keep_binaries=True), the .bin path, the decoded frames)}"""
    from compressai.utils.video.eval_model.__main__ import decode_sequence, eval_model

    outdir = tmp_path_factory.mktemp("bins")
    out = {}
    for bitdepth, (path, _) in clips.items():
        binpath = outdir / f"clip{bitdepth}.bin"
        results = eval_model(net, path, binpath, keep_binaries=True)
        out[bitdepth] = (results, binpath, decode_sequence(net, binpath))
    return out


def restated(frames, bitdepth, decoded):
    """Per frame: the fp64 metrics of the decoded frame against the clip, org_q and its near ties the restatement's."""
    per_frame = []
    for planes, x in zip(frames, decoded):
        rgb = R.to_rgb(planes, bitdepth, "bicubic", 128)
        tie = R.near_tie(rgb["level"], 2 ** bitdepth - 1, R.EPS_ORG)
        per_frame.append(R.frame_metrics(planes, rgb["org_q"], x, (0, 0, 0, 0), bitdepth, org_tie=tie))
    return per_frame


def check_psnrs(results, per_frame):
    for key, i in PSNR_KEYS:
        want = sum(m[key] for m in per_frame) / len(per_frame)
        allowed = sum(R.psnr_slack(m["sse"][i], m["slack"][i]) for m in per_frame) / len(per_frame)
        print(f"{key}: {results[key]:.6f} restated {want:.6f} allowed {allowed:.2e}")
        assert math.isfinite(results[key]) and abs(results[key] - want) <= allowed, key
    assert results["psnr-yuv"] == pytest.approx((4 * results["psnr-y"] + results["psnr-u"] + results["psnr-v"]) / 6,
                                                abs=1e-9)
    want = sum(m["mse-rgb"] for m in per_frame) / len(per_frame)
    allowed = sum(m["slack"][3] / m["counts"][3] for m in per_frame) / len(per_frame)
    assert abs(results["mse-rgb"] - want) <= allowed + 1e-12 * want


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_container_decodes_to_the_measured_frames(coded, clips, bitdepth):
    results, binpath, decoded = coded[bitdepth]
    raw = binpath.read_bytes()
    assert struct.unpack(">IIBI", raw[:13]) == (H, W, bitdepth, N)
    assert len(decoded) == N
    for x in decoded:
        assert tuple(x.shape) == (1, 3, H, W) and x.dtype == torch.float32
        assert x.min() >= 0 and x.max() <= 1
    assert not torch.equal(decoded[0], decoded[1])      # untrained, but the net does something: the frames differ
    assert set(results) == {"psnr-y", "psnr-u", "psnr-v", "psnr-yuv", "mse-rgb", "psnr-rgb", "ms-ssim-rgb", "bitrate"}
    assert all(isinstance(v, float) for v in results.values())
    per_frame = restated(clips[bitdepth][1], bitdepth, decoded)
    assert max(max(m["tie_share"]) for m in per_frame) <= R.TIE_SHARE
    check_psnrs(results, per_frame)
    assert results["bitrate"] == len(raw) * 8 * FPS / (N * 1000)


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_ms_ssim_rgb_on_levels(cuda, coded, clips, bitdepth):
    """The MS-SSIM op at data_range = max_val on the decoded frames' levels, against the fp64 torch body."""
    from compressai import _ops
    from compressai.utils.metrics import _ms_ssim_torch, ms_ssim
    from compressai.utils.video import frames

    max_val = 2 ** bitdepth - 1
    results, _, decoded = coded[bitdepth]
    got, want, scaled = [], [], []
    for planes, x in zip(clips[bitdepth][1], decoded):
        planes = tuple(R.as_container(p, bitdepth).to(cuda) for p in planes)
        _, _, org_q = frames.yuv420_to_rgb(planes, bitdepth, "bicubic", 1)
        m = frames.frame_metrics(planes, org_q, x, (0, 0, 0, 0), bitdepth)
        _, rec_q = _ops.video_frame_sse(planes, bitdepth, org_q, x, 0, 0)
        got.append(m["ms-ssim-rgb"].item())
        want.append(_ms_ssim_torch(org_q[None].cpu(), rec_q[None].cpu(), data_range=float(max_val),
                                   dtype=torch.float64).mean().item())
        scaled.append(ms_ssim(org_q[None] / max_val, rec_q[None] / max_val, data_range=1.0).item())
    d_levels = max(abs(a - b) for a, b in zip(got, want))
    d_scaled = max(abs(a - b) for a, b in zip(scaled, want))
    print(f"ms-ssim-rgb {bitdepth} bit: fp64 {want}; |op at data_range {max_val} - fp64| {d_levels:.3e}; "
          f"|op on levels / max_val at data_range 1 - fp64| {d_scaled:.3e}")
    assert d_levels <= MSSSIM_BOUND
    assert abs(results["ms-ssim-rgb"] - sum(want) / N) <= MSSSIM_BOUND


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_entropy_estimation(cuda, net, clips, bitdepth):
    from compressai._prepack import prepacked_forward
    from compressai.utils.video import frames
    from compressai.utils.video.eval_model.__main__ import eval_model_entropy_estimation

    path, clip = clips[bitdepth]
    results = eval_model_entropy_estimation(net, path)
    bits, recs = [], []
    with torch.no_grad(), prepacked_forward(net):
        x_rec = None
        for planes in clip:
            planes = tuple(R.as_container(p, bitdepth).to(cuda) for p in planes)
            x, padding, _ = frames.yuv420_to_rgb(planes, bitdepth, "bicubic", 128)
            x_rec, liks = net.forward_keyframe(x) if x_rec is None else net.forward_inter(x, x_rec)
            x_rec = x_rec.clamp(0, 1)
            bits.append(sum(-torch.log2(l[k].double()).sum().item() for l in liks.values() for k in ("y", "z")))
            left, _, top, _ = padding
            recs.append(x_rec[:, :, top:top + H, left:left + W].cpu())
    want = sum(bits) / N * FPS / 1000
    print(f"{bitdepth} bit: bitrate {results['bitrate']:.6f} kbit/s, own sum {want:.6f}")
    assert want > 0 and abs(results["bitrate"] - want) <= 1e-6 * want
    check_psnrs(results, restated(clip, bitdepth, recs))


def test_cli(cuda, net, clips, tmp_path, monkeypatch):
    import compressai.utils.video.eval_model.__main__ as M

    dataset = clips[8][0].parent
    ckpt = tmp_path / "ssf-test.pth.tar"
    torch.save(net.state_dict(), ckpt)
    out = tmp_path / "out"
    argv = ["checkpoint", str(dataset), str(out), "-a", "ssf2020", "-p", str(ckpt), "--entropy-estimation"]
    res = M.main(argv)
    agg = out / "ssf2020-entropy-estimation.json"
    assert json.loads(agg.read_text()) == json.loads(json.dumps(res))
    assert set(res) == {"name", "description", "results"}
    assert res["name"] == "ssf2020-mse" and res["description"] == "Inference (entropy-estimation)"
    metrics = {"psnr-y", "psnr-u", "psnr-v", "psnr-yuv", "mse-rgb", "psnr-rgb", "ms-ssim-rgb", "bitrate"}
    assert set(res["results"]) == metrics | {"q"} and res["results"]["q"] == ["ssf-test-entropy-estimation"]
    per_seq = []
    for bitdepth in (8, 10):
        f = out / f"{clips[bitdepth][0].stem}-ssf-test-entropy-estimation.json"
        data = json.loads(f.read_text())
        assert set(data) == {"source", "name", "description", "results"}
        assert data["source"] == clips[bitdepth][0].stem and data["name"] == "ssf2020"
        assert set(data["results"]) == metrics and all(math.isfinite(v) for v in data["results"].values())
        per_seq.append((f, f.stat().st_mtime_ns, data))
    for k in metrics:       # the aggregate is the mean over the sequences
        assert res["results"][k] == [pytest.approx(sum(d["results"][k] for _, _, d in per_seq) / 2, rel=1e-12)]
    # the checkpoint round trip: the same numbers as the net it was saved from
    direct = M.eval_model_entropy_estimation(net, clips[8][0])
    assert per_seq[0][2]["results"] == pytest.approx(direct, rel=1e-9)

    def refuse(*a, **k):
        raise AssertionError("a sequence with a result file was evaluated again")

    monkeypatch.setattr(M, "eval_model_entropy_estimation", refuse)
    again = M.main(argv)
    assert again["results"] == res["results"]
    assert [f.stat().st_mtime_ns for f, _, _ in per_seq] == [t for _, t, _ in per_seq]
    with pytest.raises(AssertionError, match="evaluated again"):
        M.main(argv + ["-f"])
