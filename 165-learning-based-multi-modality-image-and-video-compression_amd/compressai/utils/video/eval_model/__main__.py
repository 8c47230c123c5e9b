"""Evaluate a video codec on a directory of raw YUV 4:2:0 sequences.

Reference: compressai/utils/video/eval_model/__main__.py -- same command line, same JSON files (one
``<sequence>-<net>.json`` per sequence and the aggregate ``<arch>-<description>.json``), same bitstream container.

  python -m compressai.utils.video.eval_model checkpoint DIR OUT -a ssf2020 -p CKPT [--entropy-estimation] [--cuda]

Per frame: ``frames.yuv420_to_rgb`` (integer planes -> padded model input, one launch), ``encode_keyframe`` /
``encode_inter`` (or the ``forward_*`` pair when only estimating the rate), an in-place clamp of the reconstruction
to [0, 1] -- the clamped frame is the next reference -- and ``frames.frame_metrics`` (one launch + MS-SSIM).  The
planes go to the device as the integers they are, the whole sequence runs inside one ``prepacked_forward``, and the
metrics stay on the device until the sequence ends.

The container, big-endian: ``uint32 H, uint32 W, uint8 bitdepth, uint32 frames``, then per frame one body (a
keyframe) or two (motion, residual); a body is ``uint32 shape[0], uint32 shape[1], uint32 n_strings`` and per string
``uint32 length`` + the bytes.  The reference only writes it; ``decode_sequence`` here reads it back into frames.

Differences from the reference: ``--half`` runs bf16 autocast (as the image eval_model of this package does; the
reference casts the model to fp16); ``pretrained`` sources are remote downloads and raise the zoo's error; the
sequences are visited in sorted order.
"""
import argparse
import json
import math
import struct
import sys
from collections import defaultdict
from pathlib import Path
from typing import Any, Dict, List

import numpy as np
import torch
import torch.nn as nn

import compressai
from compressai._prepack import prepacked_forward
from compressai.datasets import RawVideoSequence, VideoFormat
from compressai.models.video import ScaleSpaceFlow
from compressai.utils.video import frames
from compressai.utils.video.pipeline import StagingRing, check_frames_in_flight, run_ordered
from compressai.zoo import load_state_dict
from compressai.zoo import video_models as pretrained_models

models = {"ssf2020": ScaleSpaceFlow}

RAWVIDEO_EXTENSIONS = (".yuv",)
UPSAMPLING = "bicubic"      # the chroma filter of the reference's driver


def collect_videos(rootpath: str) -> List[Path]:
    return sorted(p for ext in RAWVIDEO_EXTENSIONS for p in Path(rootpath).glob(f"*{ext}"))


def aggregate_results(filepaths: List[Path]) -> Dict[str, Any]:
    """The mean of every metric over the per-sequence JSON files."""
    metrics = defaultdict(list)
    for f in filepaths:
        with f.open("r") as fd:
            data = json.load(fd)
        for k, v in data["results"].items():
            metrics[k].append(v)
    return {k: float(np.mean(v)) for k, v in metrics.items()}


def estimate_bits_frame(likelihoods) -> torch.Tensor:
    """-sum log2 likelihood over every stream's y and z (a 0-dim tensor)."""
    return sum(torch.log(lkl[k].float()).sum() / (-math.log(2)) for lkl in likelihoods.values() for k in ("y", "z"))


def filesize(filepath) -> int:
    if not Path(filepath).is_file():
        raise ValueError(f'Invalid file "{filepath}".')
    return Path(filepath).stat().st_size


# ---------------------------------------------------------------------------------------------------------
# the container
# ---------------------------------------------------------------------------------------------------------
def write_uints(fd, values, fmt=">{:d}I"):
    fd.write(struct.pack(fmt.format(len(values)), *values))
    return len(values) * 4


def write_uchars(fd, values, fmt=">{:d}B"):
    fd.write(struct.pack(fmt.format(len(values)), *values))
    return len(values)


def read_uints(fd, n, fmt=">{:d}I"):
    return struct.unpack(fmt.format(n), _read(fd, 4 * n))


def read_uchars(fd, n, fmt=">{:d}B"):
    return struct.unpack(fmt.format(n), _read(fd, n))


def write_bytes(fd, values, fmt=">{:d}s"):
    if len(values) == 0:
        return 0
    fd.write(struct.pack(fmt.format(len(values)), values))
    return len(values)


def read_bytes(fd, n, fmt=">{:d}s"):
    return struct.unpack(fmt.format(n), _read(fd, n))[0]


def _read(fd, n):
    data = fd.read(n)
    if len(data) != n:
        raise ValueError(f"truncated bitstream: wanted {n} bytes, got {len(data)}")
    return data


def write_body(fd, shape, out_strings):
    """One coded stream: its latent grid and its strings (the first sample of each: the driver codes one clip)."""
    cnt = write_uints(fd, (shape[0], shape[1], len(out_strings)))
    for s in out_strings:
        cnt += write_uints(fd, (len(s[0]),))
        cnt += write_bytes(fd, s[0])
    return cnt


def read_body(fd):
    shape = read_uints(fd, 2)
    n_strings = read_uints(fd, 1)[0]
    lstrings = [[read_bytes(fd, read_uints(fd, 1)[0])] for _ in range(n_strings)]
    return lstrings, shape


def write_header(fd, height, width, bitdepth, num_frames):
    return write_uints(fd, (height, width)) + write_uchars(fd, (bitdepth,)) + write_uints(fd, (num_frames,))


def read_header(fd):
    """(height, width, bitdepth, num_frames)"""
    height, width = read_uints(fd, 2)
    return height, width, read_uchars(fd, 1)[0], read_uints(fd, 1)[0]


# ---------------------------------------------------------------------------------------------------------
# one sequence
# ---------------------------------------------------------------------------------------------------------
def _open(sequence) -> RawVideoSequence:
    org_seq = RawVideoSequence.from_file(str(sequence))
    if org_seq.format != VideoFormat.YUV420:
        raise NotImplementedError(f"Unsupported video format: {org_seq.format}")
    return org_seq


def _autocast(half: bool, device):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(half and device.type == "cuda"))


def _finish(results: Dict[str, list]) -> Dict[str, float]:
    """Per-metric means over the frames; the one read-back of the sequence."""
    keys = list(results)
    means = torch.stack([torch.stack([v.double() for v in results[k]]).mean() for k in keys]).cpu()
    return {k: means[i].item() for i, k in enumerate(keys)}


@torch.no_grad()
def encode_frames(net: nn.Module, org_seq: RawVideoSequence, f, num_frames: int, half: bool = False,
                  per_frame=None, frames_in_flight: int = 1) -> None:
    """Write the container of the first ``num_frames`` frames of ``org_seq`` to the open file ``f``: the header, then
    each frame's bodies.  ``per_frame(i, planes, org_q, x_rec, padding)`` is called after frame i is written, with
    its integer planes on the device, its RGB levels and the clamped reconstruction (the next reference: it must
    not be changed).  The one encoder loop of this package: the evaluation and the codec CLI both run it.

    ``frames_in_flight = W > 1``: the device work of frame i + 1 is issued while the strings of the frames <= i are
    still being coded on host threads, up to W frames deep (utils/video/pipeline.py).  The file's bytes are those of
    W = 1.  Bodies are written and ``per_frame`` is called in frame order, but ``per_frame(i, ...)`` may then run
    before body i reaches the file: it runs when frame i's device work has been issued."""
    device = next(net.parameters()).device
    bitdepth = org_seq.bitdepth
    if check_frames_in_flight(frames_in_flight) > 1:
        with prepacked_forward(net):
            write_header(f, org_seq.height, org_seq.width, bitdepth, num_frames)
            _encode_frames_in_flight(net, org_seq, f, num_frames, half, per_frame, frames_in_flight, device)
        return
    with prepacked_forward(net):
        write_header(f, org_seq.height, org_seq.width, bitdepth, num_frames)
        x_rec = None
        for i in range(num_frames):
            planes = frames.to_planes(org_seq[i], device)
            x_cur, padding, org_q = frames.yuv420_to_rgb(planes, bitdepth, UPSAMPLING, net.downsampling_factor)
            with _autocast(half, device):
                if i == 0:
                    x_rec, enc_info = net.encode_keyframe(x_cur)
                    write_body(f, enc_info["shape"], enc_info["strings"])
                else:
                    x_rec, enc_info = net.encode_inter(x_cur, x_rec)
                    for key in ("motion", "residual"):
                        write_body(f, enc_info["shape"][key], enc_info["strings"][key])
            x_rec = x_rec.float().clamp_(0, 1)
            if per_frame is not None:
                per_frame(i, planes, org_q, x_rec, padding)


def _encode_frames_in_flight(net, org_seq, f, num_frames, half, per_frame, frames_in_flight, device):
    bitdepth = org_seq.bitdepth
    ring = StagingRing(frames_in_flight)
    ref = [None]

    def issue(i):
        planes = frames.to_planes(org_seq[i], device)
        x_cur, padding, org_q = frames.yuv420_to_rgb(planes, bitdepth, UPSAMPLING, net.downsampling_factor)
        with _autocast(half, device):
            if i == 0:
                x_rec, pending = net.encode_keyframe_deferred(x_cur, ring.slot(i))
            else:
                x_rec, pending = net.encode_inter_deferred(x_cur, ref[0], ring.slot(i))
        ref[0] = x_rec = x_rec.float().clamp_(0, 1)
        if per_frame is not None:
            per_frame(i, planes, org_q, x_rec, padding)
        return pending, pending.jobs()

    def deliver(i, pending, _):
        enc_info = pending.result()
        if i == 0:
            write_body(f, enc_info["shape"], enc_info["strings"])
        else:
            for key in ("motion", "residual"):
                write_body(f, enc_info["shape"][key], enc_info["strings"][key])

    run_ordered(num_frames, frames_in_flight, issue, deliver)


@torch.no_grad()
def eval_model(net: nn.Module, sequence: Path, binpath: Path, keep_binaries: bool = False,
               half: bool = False, frames_in_flight: int = 1) -> Dict[str, Any]:
    """Code ``sequence`` into ``binpath``; the metrics of the encoder's reconstructions and the file's bit rate."""
    sequence, binpath = Path(sequence), Path(binpath)
    org_seq = _open(sequence)
    num_frames, bitdepth = len(org_seq), org_seq.bitdepth
    results = defaultdict(list)

    def measure(i, planes, org_q, x_rec, padding):
        for k, v in frames.frame_metrics(planes, org_q, x_rec, padding, bitdepth).items():
            results[k].append(v)

    print(f" encoding {sequence.stem}", file=sys.stderr)
    with binpath.open("wb") as f:
        encode_frames(net, org_seq, f, num_frames, half, measure, frames_in_flight)
    seq_results: Dict[str, Any] = _finish(results)
    seq_results["bitrate"] = float(filesize(binpath)) * 8 * float(org_seq.framerate) / (num_frames * 1000)
    if not keep_binaries:
        binpath.unlink()
    return seq_results


@torch.no_grad()
def eval_model_entropy_estimation(net: nn.Module, sequence: Path, half: bool = False) -> Dict[str, Any]:
    """The eval-mode forward of every frame; the bit rate from the likelihoods."""
    sequence = Path(sequence)
    org_seq = _open(sequence)
    device = next(net.parameters()).device
    num_frames, bitdepth = len(org_seq), org_seq.bitdepth
    results = defaultdict(list)
    print(f" encoding {sequence.stem}", file=sys.stderr)
    with prepacked_forward(net):
        x_rec = None
        for i in range(num_frames):
            planes = frames.to_planes(org_seq[i], device)
            x_cur, padding, org_q = frames.yuv420_to_rgb(planes, bitdepth, UPSAMPLING, net.downsampling_factor)
            with _autocast(half, device):
                if i == 0:
                    x_rec, likelihoods = net.forward_keyframe(x_cur)
                else:
                    x_rec, likelihoods = net.forward_inter(x_cur, x_rec)
            x_rec = x_rec.float().clamp_(0, 1)
            metrics = frames.frame_metrics(planes, org_q, x_rec, padding, bitdepth)
            metrics["bitrate"] = estimate_bits_frame(likelihoods)
            for k, v in metrics.items():
                results[k].append(v)
    seq_results: Dict[str, Any] = _finish(results)
    seq_results["bitrate"] = seq_results["bitrate"] * float(org_seq.framerate) / 1000
    return seq_results


@torch.no_grad()
def decode_frames(net: nn.Module, f, height: int, width: int, num_frames: int, per_frame, half: bool = False,
                  frames_in_flight: int = 1) -> None:
    """Decode the ``num_frames`` frames that follow the header in the open file ``f``.  ``per_frame(i, x_rec,
    padding)`` is called with each clamped, still padded reconstruction (the next reference: it must not be
    changed) and the (left, right, top, bottom) of the frame inside it.

    ``frames_in_flight = W > 1``: the first half of the decode (read the bodies, decode z, hyper decoders, queue the
    y strings on host threads) runs for the frames up to i + W - 1 before the second half of frame i (synthesis,
    warp, add), which needs frame i - 1.  The frames are those of W = 1, bit for bit, and arrive in order."""
    device = next(net.parameters()).device
    Hp, Wp, padding = frames.pad_geometry(height, width, net.downsampling_factor)
    if check_frames_in_flight(frames_in_flight) > 1:
        with prepacked_forward(net):
            _decode_frames_in_flight(net, f, num_frames, per_frame, half, frames_in_flight, device, (Hp, Wp), padding)
        return
    with prepacked_forward(net):
        x_rec = None
        for i in range(num_frames):
            with _autocast(half, device):
                if i == 0:
                    strings, shape = read_body(f)
                    x_rec = net.decode_keyframe(strings, shape)
                else:
                    bodies = {key: read_body(f) for key in ("motion", "residual")}
                    x_rec = net.decode_inter(x_rec, {k: b[0] for k, b in bodies.items()},
                                             {k: b[1] for k, b in bodies.items()})
            x_rec = x_rec.float().clamp_(0, 1)
            if tuple(x_rec.shape[-2:]) != (Hp, Wp):
                raise ValueError(f"frame {i} decodes to {tuple(x_rec.shape[-2:])}, the header says {Hp} x {Wp} padded")
            per_frame(i, x_rec, padding)


def _decode_frames_in_flight(net, f, num_frames, per_frame, half, frames_in_flight, device, padded, padding):
    ring = StagingRing(frames_in_flight)
    ref = [None]

    def issue(i):
        with _autocast(half, device):
            if i == 0:
                strings, shape = read_body(f)
                pending = net.decode_keyframe_begin(strings, shape, ring.slot(i))
            else:
                bodies = {key: read_body(f) for key in ("motion", "residual")}
                pending = net.decode_inter_begin({k: b[0] for k, b in bodies.items()},
                                                 {k: b[1] for k, b in bodies.items()}, ring.slot(i))
        return pending, pending.jobs()

    def deliver(i, pending, _):
        with _autocast(half, device):
            x_rec = pending.finish(ref[0])
        ref[0] = x_rec = x_rec.float().clamp_(0, 1)
        if tuple(x_rec.shape[-2:]) != padded:
            raise ValueError(f"frame {i} decodes to {tuple(x_rec.shape[-2:])}, the header says "
                             f"{padded[0]} x {padded[1]} padded")
        per_frame(i, x_rec, padding)

    run_ordered(num_frames, frames_in_flight, issue, deliver)


def crop(x_rec: torch.Tensor, padding, height: int, width: int) -> torch.Tensor:
    left, _, top, _ = padding
    return x_rec[:, :, top:top + height, left:left + width].clone()


@torch.no_grad()
def decode_sequence(net: nn.Module, binpath: Path, half: bool = False, frames_in_flight: int = 1) -> List[torch.Tensor]:
    """The frames a bitstream written by ``eval_model`` decodes to: [1, 3, H, W] each, cropped and clamped to
    [0, 1] (the clamped, uncropped frame is the next reference, as on the encoder side)."""
    out = []
    with Path(binpath).open("rb") as f:
        height, width, _, num_frames = read_header(f)
        decode_frames(net, f, height, width, num_frames,
                      lambda i, x_rec, padding: out.append(crop(x_rec, padding, height, width)), half,
                      frames_in_flight)
    return out


def run_inference(filepaths, net: nn.Module, outputdir: Path, force: bool = False, entropy_estimation: bool = False,
                  trained_net: str = "", description: str = "", **args: Any) -> Dict[str, Any]:
    results_paths = []
    for filepath in filepaths:
        filepath = Path(filepath)
        sequence_metrics_path = Path(outputdir) / f"{filepath.stem}-{trained_net}.json"
        results_paths.append(sequence_metrics_path)
        if force:
            sequence_metrics_path.unlink(missing_ok=True)
        if sequence_metrics_path.is_file():
            continue
        half = bool(args.get("half", False))
        if entropy_estimation:
            metrics = eval_model_entropy_estimation(net, filepath, half)
        else:
            sequence_bin = sequence_metrics_path.with_suffix(".bin")
            metrics = eval_model(net, filepath, sequence_bin, bool(args.get("keep_binaries", False)), half,
                                 int(args.get("frames_in_flight", 1)))
        with sequence_metrics_path.open("wb") as f:
            output = {
                "source": filepath.stem,
                "name": args.get("architecture", ""),
                "description": f"Inference ({description})",
                "results": metrics,
            }
            f.write(json.dumps(output, indent=2).encode())
    return aggregate_results(results_paths)


def load_checkpoint(arch: str, checkpoint_path: str) -> nn.Module:
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    for key in ("network", "state_dict"):
        if isinstance(ckpt, dict) and key in ckpt:
            ckpt = ckpt[key]
    net = models[arch]()
    net.load_state_dict(load_state_dict(ckpt))
    return net.eval()


def load_pretrained(model: str, metric: str, quality: int) -> nn.Module:
    return pretrained_models[model](quality=quality, metric=metric, pretrained=True).eval()


def create_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Video compression network evaluation.",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parent = argparse.ArgumentParser(add_help=False)
    parent.add_argument("dataset", type=str, help="sequences directory")
    parent.add_argument("output", type=str, help="output directory")
    parent.add_argument("-a", "--architecture", type=str, choices=models.keys(), help="model architecture",
                        required=True)
    parent.add_argument("-f", "--force", action="store_true", help="overwrite previous runs")
    parent.add_argument("--cuda", action="store_true", help="use the GPU (the model's kernels have no CPU form)")
    parent.add_argument("--half", action="store_true", help="bf16 autocast")
    parent.add_argument("--entropy-estimation", action="store_true",
                        help="use evaluated entropy estimation (no entropy coding)")
    parent.add_argument("-c", "--entropy-coder", choices=compressai.available_entropy_coders(),
                        default=compressai.available_entropy_coders()[0], help="entropy coder (default: %(default)s)")
    parent.add_argument("--keep_binaries", action="store_true", help="keep bitstream files in output directory")
    parent.add_argument("--frames-in-flight", type=int, default=1, metavar="N",
                        help="code up to N frames' strings on host threads behind the device (same bytes; N frames "
                             "of delay and staging memory)")
    parent.add_argument("-v", "--verbose", action="store_true", help="verbose mode")
    parent.add_argument("-m", "--metric", type=str, choices=["mse", "ms-ssim"], default="mse",
                        help="metric trained against (default: %(default)s)")
    subparsers = parser.add_subparsers(help="model source", dest="source")
    subparsers.required = True
    pretrained_parser = subparsers.add_parser("pretrained", parents=[parent])
    pretrained_parser.add_argument("-q", "--quality", dest="qualities", nargs="+", type=int, default=(1,))
    checkpoint_parser = subparsers.add_parser("checkpoint", parents=[parent])
    checkpoint_parser.add_argument("-p", "--path", dest="paths", type=str, nargs="*", required=True,
                                   help="checkpoint path")
    return parser


def _checkpoint_name(path: str) -> str:
    name = Path(path).name
    for suffix in (".pth.tar", ".tar.pth", ".pth", ".pt", ".tar"):
        if name.endswith(suffix):
            return name[: -len(suffix)]
    return name


def main(args: Any = None) -> Dict[str, Any]:
    if args is None:
        args = sys.argv[1:]
    parser = create_parser()
    args = parser.parse_args(args)
    description = "entropy-estimation" if args.entropy_estimation else args.entropy_coder
    filepaths = collect_videos(args.dataset)
    if len(filepaths) == 0:
        print("Error: no video found in directory.", file=sys.stderr)
        raise SystemExit(1)
    outputdir = args.output
    Path(outputdir).mkdir(parents=True, exist_ok=True)
    compressai.set_entropy_coder(args.entropy_coder)

    if args.source == "pretrained":
        runs, opts, load_func = sorted(args.qualities), (args.architecture, args.metric), load_pretrained
        log_fmt = "\rEvaluating {0} | {run:d}"
    else:
        runs, opts, load_func = args.paths, (args.architecture,), load_checkpoint
        log_fmt = "\rEvaluating {run:s}"

    results = defaultdict(list)
    for run in runs:
        if args.verbose:
            sys.stderr.write(log_fmt.format(*opts, run=run))
            sys.stderr.flush()
        model = load_func(*opts, run)
        if args.source == "pretrained":
            trained_net = f"{args.architecture}-{args.metric}-{run}-{description}"
        else:
            trained_net = f"{_checkpoint_name(run)}-{description}"
        print(f"Using trained model {trained_net}", file=sys.stderr)
        if not torch.cuda.is_available():
            raise SystemExit("eval_model: this build runs on the GPU only (MI355X HIP kernels) and no GPU is visible")
        model = model.to("cuda")
        if not args.entropy_estimation:
            model.update(force=True)
        metrics = run_inference(filepaths, model, outputdir, trained_net=trained_net, description=description,
                                **vars(args))
        results["q"].append(trained_net)
        for k, v in metrics.items():
            results[k].append(v)

    output = {
        "name": f"{args.architecture}-{args.metric}",
        "description": f"Inference ({description})",
        "results": results,
    }
    with (Path(outputdir) / f"{args.architecture}-{description}.json").open("wb") as f:
        f.write(json.dumps(output, indent=2).encode())
    print(json.dumps(output, indent=2))
    return output


if __name__ == "__main__":
    main(sys.argv[1:])
