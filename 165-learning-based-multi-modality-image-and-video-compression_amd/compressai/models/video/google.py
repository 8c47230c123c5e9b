"""ScaleSpaceFlow, the scale-space flow video codec of Agustsson et al. (CVPR 2020); zoo name ``ssf2020``.

Drop-in for the reference's ``compressai.models.video.ScaleSpaceFlow``: same constructor arguments, public methods,
return values and state_dict keys; the code below is this project's own.

Three streams -- ``img`` (the keyframe), ``motion`` and ``res`` (the residual) -- each own an analysis stack, a
synthesis stack and a mean-scale hyperprior (``_StreamPrior``).  All of them are k5 s2 conv / deconv chains built
by ``_chain`` from a width list, so the ReLUs run in the conv epilogues (``layers.Sequential``).  ``_TABLE`` holds the
widths; the three hyperpriors are identical.

An inter frame is coded by ``_inter_frame`` in one of three modes (training / estimation, encoding, decoding);
``forward_inter``, ``encode_inter`` and ``decode_inter`` are thin views of it, and the keyframe has the same shape
in ``_key_frame``.  Scale-space motion compensation -- the Gaussian pyramid volume of the previous reconstruction
and its trilinear warp by the decoded (flow_x, flow_y, scale) field -- runs on csrc/ssf.hip
(``_ops.ScaleSpaceVolumeFn`` / ``ScaleSpaceWarpFn``), in fp32 whatever the autocast state.  The warp reads the
motion decoder's output in place (no chunk copies) and, on the encoder side, writes the residual
``x_cur - x_pred`` from the same launch.

``y_hat = round(y - means) + means`` rounds in training too: one launch of the quantize kernel whose gradient goes
to ``y`` alone (the two ``means`` terms of the straight-through form cancel).

Coding can run with several frames in flight (``compress(frames, frames_in_flight=W)``, the ``*_deferred`` encoders
and the ``decode_*_begin`` / ``PendingDecode.finish`` halves): the device side of a frame returns at once and the host
coder of up to W frames runs on worker threads (``utils/video/pipeline.py``).  The strings stay one serial rANS state
each, byte for byte those of W = 1; W = 1 is the code path above, unchanged.

Frames must have H and W that are multiples of 128 (four stride-2 stages, three more in the hyperprior); other
sizes raise ``ValueError`` before anything is launched.
"""
from typing import List

import torch
import torch.nn as nn

from ... import _prepack
from ..._native import Q_DEQUANTIZE
from ..._ops import CatFn, ScaleSpaceVolumeFn, ScaleSpaceWarpFn
from ..._prepack import prepacked_forward
from ...entropy_models import GaussianConditional
from ...entropy_models.entropy_models import _QuantizeFn
from ...layers import QReLU, Sequential
from ...utils.video.pipeline import StagingRing, check_frames_in_flight, run_ordered
from ..google import CompressionModel, get_scale_table
from ..utils import conv, deconv, update_registered_buffers

__all__ = ["ScaleSpaceFlow"]

LATENT = 192          # channels of every y and z
WIDTH = 128           # channels between the image-side layers
QRELU_BITS, QRELU_BETA = 8, 100

# stream prefix -> (analysis input channels, synthesis input channels, synthesis output channels, output key)
_TABLE = {
    "img": (3, LATENT, 3, "keyframe"),
    "res": (3, 2 * LATENT, 3, "residual"),       # decoded from cat(y_res_hat, y_motion_hat)
    "motion": (6, LATENT, 3, "motion"),           # cat(x_cur, x_ref) in; flow x, flow y and scale out
}

TRAIN, ENCODE, DECODE, ENCODE_DEFERRED = "train", "encode", "decode", "encode-deferred"


def _chain(layer, widths):
    """layer(widths[0], widths[1]) -> ReLU -> layer(widths[1], widths[2]) -> ... (no ReLU after the last)."""
    mods = []
    for cin, cout in zip(widths[:-1], widths[1:]):
        if mods:
            mods.append(nn.ReLU(inplace=True))
        mods.append(layer(cin, cout, kernel_size=5, stride=2))
    return Sequential(*mods)


class _RoundSte(torch.autograd.Function):
    """round(y - means) + means; backward: dy = g, dmeans = 0."""

    @staticmethod
    def forward(ctx, y, means):
        return _QuantizeFn.forward(ctx, y, means, None, Q_DEQUANTIZE)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _ScaleSynthesis(nn.Module):
    """Three deconvs, each clamped by a QReLU: the scales stay in [0, 2^bits - 1] as in an integer network."""

    def __init__(self, planes):
        super().__init__()
        for i in (1, 2, 3):
            setattr(self, f"deconv{i}", deconv(planes, planes, kernel_size=5, stride=2))

    def forward(self, t):
        for i in (1, 2, 3):
            t = QReLU.apply(getattr(self, f"deconv{i}")(t), QRELU_BITS, QRELU_BETA)
        return t


class _StreamPrior(CompressionModel):
    """Mean-scale hyperprior of one stream's latent."""

    def __init__(self, planes: int = LATENT):
        super().__init__(entropy_bottleneck_channels=planes)
        self.hyper_encoder = _chain(conv, [planes] * 4)
        self.hyper_decoder_mean = _chain(deconv, [planes] * 4)
        self.hyper_decoder_scale = _ScaleSynthesis(planes)
        self.gaussian_conditional = GaussianConditional(None)

    def __call__(self, *args, **kwargs):
        # inside ScaleSpaceFlow the enclosing model's weight packs are active: one pack launch per model
        # forward, not one per hyperprior call
        if _prepack.active() is not None:
            return nn.Module.__call__(self, *args, **kwargs)
        return super().__call__(*args, **kwargs)

    def _entropy_params(self, z_hat):
        return self.hyper_decoder_scale(z_hat), self.hyper_decoder_mean(z_hat)

    def forward(self, y):
        z_hat, lik_z = self.entropy_bottleneck(self.hyper_encoder(y))
        scales, means = self._entropy_params(z_hat)
        lik_y = self.gaussian_conditional(y, scales, means)[1]
        return _RoundSte.apply(y, means), {"y": lik_y, "z": lik_z}

    def compress(self, y):
        z = self.hyper_encoder(y)
        grid = z.size()[-2:]
        coded_z = self.entropy_bottleneck.compress(z)
        scales, means = self._entropy_params(self.entropy_bottleneck.decompress(coded_z, grid))
        gc = self.gaussian_conditional
        coded_y = gc.compress(y, gc.build_indexes(scales), means)
        return gc.quantize(y, "dequantize", means), {"strings": [coded_y, coded_z], "shape": grid}

    def decompress(self, strings, shape):
        if not isinstance(strings, list) or len(strings) != 2:
            raise ValueError("a stream is coded as [y strings, z strings]")
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
        scales, means = self._entropy_params(z_hat)
        gc = self.gaussian_conditional
        return gc.decompress(strings[0], gc.build_indexes(scales), z_hat.dtype, means)

    # ---- deferred forms: the device side returns at once, the host coder runs behind it (frames in flight) ----
    def compress_deferred(self, y, slot=None, key=""):
        """(y_hat, _PendingStream): compress(y) without waiting for the host.  z_hat comes from the coding front
        end (the integers the z strings will hold, plus the medians), so there is no host round trip for z; the
        hyper decoders run on it as in compress()."""
        z = self.hyper_encoder(y)
        grid = z.size()[-2:]
        z_hat, coded_z = self.entropy_bottleneck.compress_deferred(z, slot, (key, "z"))
        scales, means = self._entropy_params(z_hat)
        y_hat, coded_y = self.gaussian_conditional.compress_deferred(y, scales, means, slot, (key, "y"))
        return y_hat, _PendingStream([coded_y, coded_z], grid)

    def decompress_begin(self, strings, shape, slot=None, key=""):
        """First half of decompress(): the z strings are decoded here (they are small and everything else waits for
        them), the hyper decoders and the index launch follow, and the y strings are left pending.  ``jobs()`` of
        the result go to the pool; its ``finish()`` returns y_hat."""
        if not isinstance(strings, list) or len(strings) != 2:
            raise ValueError("a stream is coded as [y strings, z strings]")
        z_hat = self.entropy_bottleneck.decompress_host(strings[1], shape, slot, (key, "z"))
        scales, means = self._entropy_params(z_hat)
        return self.gaussian_conditional.decompress_deferred(strings[0], scales, means, z_hat.dtype, slot, (key, "y"))


class _PendingStream:
    """The [y strings, z strings] of one stream, pending."""

    def __init__(self, pending, grid):
        self.pending, self.grid = pending, grid

    def jobs(self):
        return [p.run for p in self.pending]

    def result(self):
        return {"strings": [p.result() for p in self.pending], "shape": self.grid}


class PendingFrame:
    """The side information of one deferred encode: ``jobs()`` are the host-coder calls (any thread), ``result()``
    the ``{"strings", "shape"}`` dictionary encode_keyframe / encode_inter return."""

    def __init__(self, streams, inter: bool):
        self._streams, self._inter = streams, inter

    def jobs(self):
        return [j for s in self._streams.values() for j in s.jobs()]

    def result(self):
        side = {k: s.result() for k, s in self._streams.items()}
        if not self._inter:
            return side["keyframe"]
        return {field: {k: v[field] for k, v in side.items()} for field in ("strings", "shape")}


class PendingDecode:
    """One frame between the two halves of its decode: ``jobs()`` decode the y strings (any thread);
    ``finish(x_ref)`` -- main thread, in frame order -- runs the back ends, the synthesis nets, the warp and the add."""

    def __init__(self, net, latents):
        self._net, self._latents = net, latents

    def jobs(self):
        return [p.run for p in self._latents.values()]

    def finish(self, x_ref=None):
        net, lat = self._net, self._latents
        if "keyframe" in lat:
            return net.img_decoder(lat["keyframe"].finish())
        if x_ref is None:
            raise ValueError("an inter frame needs its reference")
        y_m_hat = lat["motion"].finish()
        x_pred = net._predict(x_ref, net.motion_decoder(y_m_hat))
        y_r_hat = lat["residual"].finish()
        return x_pred + net.res_decoder(CatFn.apply(y_r_hat, y_m_hat))


def _want_list(*values):
    for v in values:
        if not isinstance(v, List):
            raise RuntimeError(f"Invalid number of frames: {len(v)}.")


class ScaleSpaceFlow(nn.Module):
    r"""Scale-space flow video codec.

    Args:
        num_levels (int): levels of the Gaussian scale space (the volume has ``num_levels + 1`` slices)
        sigma0 (float): standard deviation of the scale space's Gaussian kernel
        scale_field_shift (float): kept for interface compatibility; unused, as in the reference
    """

    downsampling_factor = 2 ** (4 + 3)

    def __init__(self, num_levels: int = 5, sigma0: float = 1.5, scale_field_shift: float = 1.0):
        super().__init__()
        for prefix, (a_in, s_in, s_out, _) in _TABLE.items():
            setattr(self, f"{prefix}_encoder", _chain(conv, [a_in, WIDTH, WIDTH, WIDTH, LATENT]))
            setattr(self, f"{prefix}_decoder", _chain(deconv, [s_in, WIDTH, WIDTH, WIDTH, s_out]))
            setattr(self, f"{prefix}_hyperprior", _StreamPrior())
        self.sigma0 = sigma0
        self.num_levels = num_levels
        self.scale_field_shift = scale_field_shift

    # ------------------------------------------------------------------ plumbing
    def _priors(self):
        return [(prefix, getattr(self, f"{prefix}_hyperprior")) for prefix in _TABLE]

    def _check_frames(self, frames):
        _want_list(frames)
        f = self.downsampling_factor
        for i, x in enumerate(frames):
            if x.dim() != 4 or x.shape[1] != 3:
                raise ValueError(f"frame {i}: expected a [B, 3, H, W] tensor, got {tuple(x.shape)}")
            if x.shape[2] % f or x.shape[3] % f:
                raise ValueError(f"frame {i}: H = {x.shape[2]} and W = {x.shape[3]} must be multiples of {f}")

    def __call__(self, frames, *args, **kwargs):
        self._check_frames(frames)      # before the pack launch
        with prepacked_forward(self):
            return super().__call__(frames, *args, **kwargs)

    def _latent(self, prefix, mode, y=None, coded=None, slot=None):
        """(y_hat, side information) of one stream: likelihoods (TRAIN), strings + shape (ENCODE), the same pending
        (ENCODE_DEFERRED), None (DECODE)."""
        prior = getattr(self, f"{prefix}_hyperprior")
        if mode == TRAIN:
            return prior(y)
        if mode == ENCODE_DEFERRED:
            return prior.compress_deferred(y, slot, prefix)
        if mode == ENCODE:
            return prior.compress(y)
        return prior.decompress(*coded), None

    def _key_frame(self, mode, x=None, coded=None, slot=None):
        y = None if mode == DECODE else self.img_encoder(x)
        y_hat, side = self._latent("img", mode, y, coded, slot)
        return self.img_decoder(y_hat), side

    def _inter_frame(self, mode, x_ref, x_cur=None, coded=None, slot=None):
        """One predicted frame.  coded (DECODE): ({"motion": strings, "residual": strings}, the same for shapes)."""
        def pick(key):
            return None if coded is None else (coded[0][key], coded[1][key])

        side = {}
        y_m = None if mode == DECODE else self.motion_encoder(torch.cat((x_cur, x_ref), dim=1))
        y_m_hat, side["motion"] = self._latent("motion", mode, y_m, pick("motion"), slot)
        motion_info = self.motion_decoder(y_m_hat)
        if mode == DECODE:
            x_pred, y_r = self._predict(x_ref, motion_info), None
        else:       # the prediction and x_cur - x_pred from one warp launch
            x_pred, x_res = self._predict(x_ref, motion_info, x_cur)
            y_r = self.res_encoder(x_res)
        y_r_hat, side["residual"] = self._latent("res", mode, y_r, pick("residual"), slot)
        x_rec = x_pred + self.res_decoder(CatFn.apply(y_r_hat, y_m_hat))
        return x_rec, side

    def _predict(self, x_ref, motion_info, x_cur=None):
        volume = self.gaussian_volume(x_ref, self.sigma0, self.num_levels)
        if x_cur is None:
            return ScaleSpaceWarpFn.apply(volume, motion_info)
        return ScaleSpaceWarpFn.apply(volume, motion_info, x_cur)

    # ------------------------------------------------------- training / estimation
    def forward(self, frames):
        x_hat, liks = self.forward_keyframe(frames[0])
        out = {"x_hat": [x_hat], "likelihoods": [liks]}
        x_ref = x_hat.detach()          # the keyframe is a constant for the frames predicted from it
        for x in frames[1:]:
            x_ref, liks = self.forward_inter(x, x_ref)      # later references keep their graph
            out["x_hat"].append(x_ref)
            out["likelihoods"].append(liks)
        return out

    def forward_keyframe(self, x):
        x_hat, liks = self._key_frame(TRAIN, x)
        return x_hat, {"keyframe": liks}

    def forward_inter(self, x_cur, x_ref):
        return self._inter_frame(TRAIN, x_ref, x_cur)

    def forward_prediction(self, x_ref, motion_info):
        return self._predict(x_ref, motion_info)

    @staticmethod
    def gaussian_volume(x, sigma: float, num_levels: int):
        """[N, C, H, W] -> [N, C, num_levels + 1, H, W]: x, its blur, then for every further level the previous
        blurred image pooled 2x2, blurred and brought back by repeated bilinear x2 steps (csrc/ssf.hip)."""
        return ScaleSpaceVolumeFn.apply(x, sigma, num_levels)

    def warp_volume(self, volume, flow, scale_field, padding_mode: str = "border"):
        """Trilinear warp of a [N, C, D, H, W] volume (align_corners=False), fp32 whatever the autocast state."""
        if volume.ndimension() != 5:
            raise ValueError(f"Invalid number of dimensions for volume {volume.ndimension()}")
        if padding_mode != "border":
            raise ValueError(f'padding_mode "{padding_mode}" is not supported (the model uses "border")')
        return ScaleSpaceWarpFn.apply(volume, torch.cat((flow.float(), scale_field.float()), dim=1))

    def aux_loss(self):
        """The auxiliary losses of the three hyperpriors, as a list."""
        return [m.aux_loss() for m in self.modules() if isinstance(m, CompressionModel)]

    # --------------------------------------------------------------------- coding
    def encode_keyframe(self, x):
        return self._key_frame(ENCODE, x)

    def decode_keyframe(self, strings, shape):
        return self._key_frame(DECODE, coded=(strings, shape))[0]

    def encode_inter(self, x_cur, x_ref):
        x_rec, side = self._inter_frame(ENCODE, x_ref, x_cur)
        return x_rec, {field: {k: v[field] for k, v in side.items()} for field in ("strings", "shape")}

    def decode_inter(self, x_ref, strings, shapes):
        return self._inter_frame(DECODE, x_ref, coded=(strings, shapes))[0]

    # ---- deferred coding (frames in flight): see utils/video/pipeline.py ----
    def encode_keyframe_deferred(self, x, slot=None):
        """(x_rec, PendingFrame): encode_keyframe without waiting for the host coder; ``pending.result()`` is
        encode_keyframe's dictionary.  slot: a pipeline.StagingSlot for the pinned buffers (None: new ones)."""
        x_rec, side = self._key_frame(ENCODE_DEFERRED, x, slot=slot)
        return x_rec, PendingFrame({"keyframe": side}, inter=False)

    def encode_inter_deferred(self, x_cur, x_ref, slot=None):
        """(x_rec, PendingFrame): encode_inter without waiting for the host coder."""
        x_rec, side = self._inter_frame(ENCODE_DEFERRED, x_ref, x_cur, slot=slot)
        return x_rec, PendingFrame(side, inter=True)

    def decode_keyframe_begin(self, strings, shape, slot=None):
        """First half of decode_keyframe: everything up to "the y strings are queued"; PendingDecode.finish() is
        the second.  The hyper-decoder launches are decode_keyframe's, at its shapes."""
        return PendingDecode(self, {"keyframe": self.img_hyperprior.decompress_begin(strings, shape, slot, "img")})

    def decode_inter_begin(self, strings, shapes, slot=None):
        """First half of decode_inter: it needs no reconstruction, so it can run ahead of the frames before it;
        PendingDecode.finish(x_ref) is the second half."""
        return PendingDecode(self, {
            "motion": self.motion_hyperprior.decompress_begin(strings["motion"], shapes["motion"], slot, "motion"),
            "residual": self.res_hyperprior.decompress_begin(strings["residual"], shapes["residual"], slot, "res")})

    def _compress_in_flight(self, frames, frames_in_flight):
        ring = StagingRing(frames_in_flight)
        strings, shapes, ref = [], [], [None]

        def issue(i):
            slot = ring.slot(i)
            if i == 0:
                ref[0], pending = self.encode_keyframe_deferred(frames[i], slot)
            else:
                ref[0], pending = self.encode_inter_deferred(frames[i], ref[0], slot)
            return pending, pending.jobs()

        def deliver(i, pending, _):
            info = pending.result()
            strings.append(info["strings"])
            shapes.append(info["shape"])

        run_ordered(len(frames), frames_in_flight, issue, deliver)
        return strings, shapes

    def _decompress_in_flight(self, strings, shapes, frames_in_flight):
        ring = StagingRing(frames_in_flight)
        frames = []

        def issue(i):
            slot = ring.slot(i)
            begin = self.decode_keyframe_begin if i == 0 else self.decode_inter_begin
            pending = begin(strings[i], shapes[i], slot)
            return pending, pending.jobs()

        def deliver(i, pending, _):
            frames.append(pending.finish(frames[-1] if frames else None))

        run_ordered(len(strings), frames_in_flight, issue, deliver)
        return frames

    @torch.no_grad()
    def compress(self, frames, frames_in_flight: int = 1):
        """frames_in_flight = W > 1: the host coder of up to W frames runs on worker threads behind the device
        work of the frames after them; the strings are those of W = 1, byte for byte."""
        self._check_frames(frames)
        if check_frames_in_flight(frames_in_flight) > 1:
            with prepacked_forward(self):
                return self._compress_in_flight(frames, frames_in_flight)
        strings, shapes = [], []
        with prepacked_forward(self):
            x_ref = None
            for x in frames:
                x_ref, info = self.encode_keyframe(x) if x_ref is None else self.encode_inter(x, x_ref)
                strings.append(info["strings"])
                shapes.append(info["shape"])
        return strings, shapes

    @torch.no_grad()
    def decompress(self, strings, shapes, frames_in_flight: int = 1):
        _want_list(strings, shapes)
        if len(strings) != len(shapes):
            raise ValueError(f"{len(strings)} coded frames but {len(shapes)} shapes")
        if check_frames_in_flight(frames_in_flight) > 1:
            with prepacked_forward(self):
                return self._decompress_in_flight(strings, shapes, frames_in_flight)
        frames = []
        with prepacked_forward(self):
            for s, sh in zip(strings, shapes):
                frames.append(self.decode_inter(frames[-1], s, sh) if frames else self.decode_keyframe(s, sh))
        return frames

    # ---------------------------------------------------------------- checkpoints
    def load_state_dict(self, state_dict, strict: bool = True):
        # the six CDF buffer sets take the checkpoint's sizes
        for prefix, prior in self._priors():
            for child, extra in (("gaussian_conditional", ["scale_table"]), ("entropy_bottleneck", [])):
                update_registered_buffers(getattr(prior, child), f"{prefix}_hyperprior.{child}",
                                          ["_quantized_cdf", "_offset", "_cdf_length"] + extra, state_dict)
        return nn.Module.load_state_dict(self, state_dict, strict=strict)

    @classmethod
    def from_state_dict(cls, state_dict):
        net = cls()
        net.load_state_dict(state_dict)
        return net

    def update(self, scale_table=None, force=False):
        table = get_scale_table() if scale_table is None else scale_table
        changed = False
        for _, prior in self._priors():
            changed |= prior.gaussian_conditional.update_scale_table(table, force=force)
            changed |= prior.entropy_bottleneck.update(force=force)
        return changed
