"""EntropyModel / EntropyBottleneck / GaussianConditional on the HIP kernels.

Reference: compressai/entropy_models/entropy_models.py (quantize :157-182,
EntropyBottleneck :330-574, GaussianConditional :577-740).  Parameters,
buffers, constructor arguments, ValueError checks and the
``forward(...) -> (outputs, likelihoods)`` contract are kept; the forward
and backward of the likelihood path are single fused kernels
(cai_eb_fwd/_bwd, cai_gc_fwd/_bwd) instead of ~40 small torch ops, and
training-mode noise is U(-1/2, 1/2) as in the reference
(``empty_like(x).uniform_(-0.5, 0.5)``, entropy_models.py:170), drawn on the
device by cai_uniform_noise (Philox4x32-10, counter kept in device memory: a
captured graph draws new noise on every replay without torch's generator and
its per-replay re-seeding launches); seeded from torch.cuda.initial_seed(), so
torch.cuda.manual_seed() keeps runs reproducible.  By default no launch of its
own makes the draw: the first kernel that consumes it generates it in-register
(_ops.DeviceDraw, cai_noise_src DRAW) and the later ones regenerate it (REPLAY),
the same values cai_uniform_noise would have written (CAI_FUSED_NOISE=0: the
separate draw).  Tests inject their own draws (set_noise_source) to compare
against the CPU oracle.

The bitstream side follows the reference too:
update() evaluates the pmfs with the reference's torch expressions on the
module's device and quantizes them to CDF tables in libcai_coder.so
(cai_pmf_to_quantized_cdf_rows); compress() takes its integer symbols from
the quantize kernel (SYMBOLS mode) and codes one rANS stream per image on
host threads (cai_rans_encode_batch), byte-identical to compressai.ans;
decompress() decodes them (cai_rans_decode_batch) and dequantizes.

compress_deferred() / decompress_deferred() are the same coding with the host
part left pending: one launch of the coding front end (csrc/code_front.hip)
writes symbols and indexes in the coder's order plus x_hat, non-blocking copies
take the integers to pinned memory, and the returned pending object runs the
host coder when its result is asked for -- on a worker thread when a frame
pipeline (utils/video/pipeline.py) runs it.  Same bytes as compress().
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Any, Callable, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

import scipy.stats

from .. import _coder
from .._native import F32, NOISE_STATE_WORDS, Q_DEQUANTIZE, Q_NOISE, Q_SYMBOLS, lib
from .._ops import (BottleneckAuxFn, BottleneckFn, DeviceDraw, GaussianFn, _check_cuda, _p, _stream, as_rows,
                    code_back, code_front, code_front_channels, code_indexes, dcode, empty_rows_like, noise_src)
from ..ops import LowerBound

__all__ = ["EntropyModel", "EntropyBottleneck", "GaussianConditional", "set_noise_source", "seed_noise"]

# ---------------------------------------------------------------------------
# noise source: torch's generator by default; tests inject identical tensors
# into this build and into the CPU oracle.
# ---------------------------------------------------------------------------
_noise_source: Optional[Callable[[torch.Tensor], torch.Tensor]] = None


def set_noise_source(fn: Optional[Callable[[torch.Tensor], torch.Tensor]]):
    """fn(x) -> fp32 noise tensor of x's logical shape (None restores U(-1/2,1/2))."""
    global _noise_source
    _noise_source = fn


# on-device generator state per GPU: [seed, draw index, arrival ticket, ..., the DRAW launches' per-XCD arrival
# shards] (NOISE_STATE_WORDS uint64 bit patterns, include/cai.h).  ONE state per device: draws that use it must
# be ordered (one stream, or event-ordered) -- two concurrent launches would read the same draw index and mix
# their arrival tickets.  The models' hyper-branch fork therefore draws z's noise on the caller's stream before
# forking (models/google.py, _z_noise).
_noise_states: dict = {}
# A/B knobs (read once): CAI_TORCH_NOISE=1 draws with torch's generator instead (`uniform_`, as the reference);
# CAI_FUSED_NOISE=0 draws into a buffer with cai_uniform_noise instead of inside the consuming kernel
_TORCH_NOISE = os.environ.get("CAI_TORCH_NOISE", "0") == "1"
_FUSED_NOISE = os.environ.get("CAI_FUSED_NOISE", "1") == "1"


def _as_i64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def seed_noise(seed: int, device=None) -> None:
    """Seed the training-noise generator of `device` (default: the current GPU) and restart its stream."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _noise_states.get(idx)
    if st is None:
        st = [None, None]
        _noise_states[idx] = st
    if st[0] is None:
        st[0] = torch.zeros(NOISE_STATE_WORDS, dtype=torch.int64, device=torch.device("cuda", idx))
    st[0].zero_()
    st[0][0].fill_(_as_i64(seed))
    with torch.cuda.device(idx):
        st[1] = torch.cuda.initial_seed()   # torch's seed at this point: a later manual_seed() re-seeds


def _noise_state(dev: torch.device) -> torch.Tensor:
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _noise_states.get(idx)
    seed = None
    if not torch.cuda.is_current_stream_capturing():
        with torch.cuda.device(idx):
            seed = torch.cuda.initial_seed()
    # (re)seed on first use and whenever torch.cuda.manual_seed() changed the device seed (eager mode; a
    # capture keeps the state it finds)
    if st is None and seed is None:
        raise RuntimeError("training noise: run one eager training-mode forward (or call seed_noise()) before "
                           "capturing a graph; the generator state must exist outside the capture")
    if st is None or (seed is not None and seed != st[1]):
        seed_noise(seed, torch.device("cuda", idx))
        st = _noise_states[idx]
    return st[0]


def _draw_noise(x: torch.Tensor) -> torch.Tensor:
    if _noise_source is not None:
        n = _noise_source(x)
        if tuple(n.shape) != tuple(x.shape):
            raise ValueError(f"noise source returned shape {tuple(n.shape)}, expected {tuple(x.shape)}")
        return n.to(device=x.device, dtype=torch.float32)
    if _TORCH_NOISE:
        return torch.empty_like(x, dtype=torch.float32).uniform_(-0.5, 0.5)
    _check_cuda(x)
    out = torch.empty_like(x, dtype=torch.float32)   # dense storage: numel() values from data_ptr()
    lib.cai_uniform_noise(_p(out), out.numel(), _p(_noise_state(x.device)), _stream())
    return out


def _noise_for(x: torch.Tensor):
    """Training noise for x, to hand to a noise-mode entropy kernel: a DeviceDraw (drawn inside that kernel),
    or -- with an injected source, torch's generator, or CAI_FUSED_NOISE=0 -- a tensor from _draw_noise."""
    if _noise_source is not None or _TORCH_NOISE or not _FUSED_NOISE:
        return _draw_noise(x)
    _check_cuda(x)
    return DeviceDraw(x.shape, _noise_state(x.device))


class _QuantizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, means, noise, mode: int):
        """noise: None, an fp32 tensor, or a DeviceDraw (NOISE mode)."""
        draw = isinstance(noise, DeviceDraw)
        _check_cuda(x, means, None if draw else noise)
        xr, xld, npix, C = as_rows(x)
        m = None
        mld, mpc = 0, 0
        if means is not None:
            if means.numel() == C and means.dim() != x.dim():
                m, mld, mpc = means.float().contiguous().reshape(C), 0, 1
            else:
                m, mld = as_rows(means.float().expand_as(x))[:2]
        nr, nld = (None, 0) if noise is None or draw else as_rows(noise)[:2]
        odt = torch.int32 if mode == Q_SYMBOLS else x.dtype
        out, obuf = empty_rows_like(x.shape, odt, x.device)
        lib.cai_quantize(mode, npix, C, _p(xr), dcode(x.dtype), xld, _p(m), mld, mpc, noise_src(noise, nr, nld),
                         _p(obuf), dcode(x.dtype) if mode != Q_SYMBOLS else F32, C, _stream())
        ctx.mode = mode
        ctx.has_means = means is not None
        ctx.mshape = None if means is None else means.shape
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.mode == Q_NOISE:
            return g, None, None, None
        gm = None
        if ctx.has_means:
            gm = g.float()
            if tuple(gm.shape) != tuple(ctx.mshape):
                gm = gm.sum_to_size(ctx.mshape)
        return torch.zeros_like(g), gm, None, None


# ---------------------------------------------------------------------------
# deferred coding: the device side returns at once, the host coder runs when (and where) the pending object is run
# ---------------------------------------------------------------------------
def _staging(slot, key, numel: int) -> torch.Tensor:
    """A pinned int32 host tensor of numel elements: the slot's (utils.video.pipeline.StagingSlot), or a new one."""
    if slot is not None:
        return slot.buffer(key, numel)
    return torch.empty(max(1, numel), dtype=torch.int32, pin_memory=True)[:numel]


def _fused_coding(*ts) -> bool:
    """The coding front / back end kernels take 4-D fp32 CUDA tensors; anything else goes through the composed ops."""
    return all(t.is_cuda and t.dim() == 4 and t.dtype == torch.float32 for t in ts)


class _TablesCache:
    """An entropy model's host tables and what they were built from.  The tables hold raw pointers into their own
    arrays, so a copy or a pickle of the module starts with an empty cache instead of a copied one."""

    __slots__ = ("key", "tables")

    def __init__(self, key=None, tables=None):
        self.key, self.tables = key, tables

    def __deepcopy__(self, memo):
        return _TablesCache()

    def __reduce__(self):
        return (_TablesCache, ())


class _Pending:
    """A host-coder job.  ``run()`` may be called from a worker thread: it waits for the device event, then calls
    libcai_coder through ctypes -- no launch, no allocation on the device, no tensor operation.  ``result()`` runs
    it on the calling thread if nobody has, and re-raises what it raised."""

    def __init__(self):
        self._lock = threading.Lock()       # run() from two threads: the second waits and takes the first's outcome
        self._done = False
        self._value = None
        self._error: Optional[BaseException] = None

    def _work(self):
        raise NotImplementedError

    def run(self):
        with self._lock:
            if not self._done:
                try:
                    self._value = self._work()
                except BaseException as e:      # kept for result(); a pool re-raises it from its future as well
                    self._error = e
                self._done = True
        if self._error is not None:
            raise self._error
        return self._value

    def result(self):
        return self.run()


class PendingStrings(_Pending):
    """The strings of one deferred ``compress``: symbols and indexes are on their way into pinned host memory
    (``event`` follows the copies); ``result()`` is the list of ``bytes``, one per batch element."""

    def __init__(self, sym: torch.Tensor, idx: torch.Tensor, event, tables: "_coder.Tables", nstreams: int,
                 threads: int = 1):
        super().__init__()
        self._host = (sym, idx)             # pinned tensors, kept alive until the coder has read them
        self._np = (sym.numpy(), idx.numpy())     # views made here: the worker touches no tensor
        self._event, self._tables, self._n, self._threads = event, tables, int(nstreams), int(threads)

    def _work(self):
        if self._event is not None:
            self._event.synchronize()
        sym, idx = self._np
        return _coder.encode_streams(sym, idx, self._tables, self._n, self._threads)


class PendingSymbols(_Pending):
    """The symbols of one deferred ``decompress``: ``run()`` decodes the strings into pinned host memory (the
    indexes arrive there behind ``event``); ``finish()`` -- main thread -- copies them to the device and dequantizes."""

    def __init__(self, strings, idx: torch.Tensor, out: torch.Tensor, event, tables: "_coder.Tables", finish,
                 threads: int = 1, slot=None):
        super().__init__()
        self._slot = slot
        self._strings = [bytes(s) for s in strings]
        self._idx, self._out, self._event, self._tables = idx, out, event, tables
        self._np = (idx.numpy(), out.numpy())     # views made here: the worker touches no tensor
        self._finish, self._threads = finish, int(threads)

    def _work(self):
        if self._event is not None:
            self._event.synchronize()
        _coder.decode_streams_into(self._strings, self._np[0], self._tables, self._np[1], self._threads)
        return True

    def finish(self) -> torch.Tensor:
        self.result()
        x_hat = self._finish(self._out)
        if self._slot is not None and x_hat.is_cuda:
            # the staging slot may be written again only after the copy issued above has read it
            self._slot.busy = torch.cuda.Event(blocking=True)
            self._slot.busy.record()
        return x_hat


class EntropyModel(nn.Module):
    def __init__(self, likelihood_bound: float = 1e-9, entropy_coder: Optional[str] = None,
                 entropy_coder_precision: int = 16):
        super().__init__()
        from .. import available_entropy_coders, get_entropy_coder

        if entropy_coder is None:
            entropy_coder = get_entropy_coder()
        if not isinstance(entropy_coder, str):
            raise ValueError(f'Invalid method type "{type(entropy_coder)}"')
        if entropy_coder not in available_entropy_coders():
            raise ValueError(f'Unknown entropy coder "{entropy_coder}" (available: {", ".join(available_entropy_coders())})')
        self.entropy_coder = entropy_coder
        self.entropy_coder_precision = int(entropy_coder_precision)
        self.use_likelihood_bound = likelihood_bound > 0
        # python-side copy: kernels take the bound by value (no .item() sync, graph-capturable)
        self._lik_bound_value = float(likelihood_bound) if self.use_likelihood_bound else 0.0
        if self.use_likelihood_bound:
            self.likelihood_lower_bound = LowerBound(likelihood_bound)
        self.register_buffer("_offset", torch.IntTensor())
        self.register_buffer("_quantized_cdf", torch.IntTensor())
        self.register_buffer("_cdf_length", torch.IntTensor())

    @property
    def offset(self):
        return self._offset

    @property
    def quantized_cdf(self):
        return self._quantized_cdf

    @property
    def cdf_length(self):
        return self._cdf_length

    def _lik_bound(self) -> float:
        return self._lik_bound_value

    def forward(self, *args: Any) -> Any:
        raise NotImplementedError()

    def quantize(self, inputs: torch.Tensor, mode: str, means: Optional[torch.Tensor] = None) -> torch.Tensor:
        if mode not in ("noise", "dequantize", "symbols"):
            raise ValueError(f'Invalid quantization mode: "{mode}"')
        if mode == "noise":
            return _QuantizeFn.apply(inputs, None, _noise_for(inputs), Q_NOISE)
        if mode == "dequantize":
            return _QuantizeFn.apply(inputs, means, None, Q_DEQUANTIZE)
        return _QuantizeFn.apply(inputs, means, None, Q_SYMBOLS)

    @staticmethod
    def dequantize(inputs: torch.Tensor, means: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float):
        if means is not None:
            out = inputs.type_as(means)
            out += means
            return out
        return inputs.type(dtype)

    # ---- bitstream side (entropy_models.py:206-327) --------------------------

    def _pmf_to_cdf(self, pmf, tail_mass, pmf_length, max_length):
        """entropy_models.py:206-214: row i = quantized CDF of [pmf[i, :pmf_length[i]], tail_mass[i]]
        in a zero-filled [rows, max_length + 2] int32 table (libcai_coder.so, rows on host threads)."""
        lengths = pmf_length.detach().reshape(-1).to("cpu", torch.int64).numpy()
        rows = lengths.size
        p = pmf.detach().float().reshape(rows, -1).cpu().numpy()
        tail = tail_mass.detach().float().reshape(rows, -1)[:, 0].cpu().numpy()
        table = np.zeros((rows, max_length + 1), dtype=np.float32)
        keep = np.arange(p.shape[1])[None, :] < lengths[:, None]
        table[:, :p.shape[1]] = np.where(keep, p, 0.0)
        table[np.arange(rows), lengths] = tail
        cdf = _coder.pmf_to_quantized_cdf_rows(table, lengths + 1, self.entropy_coder_precision, max_length + 2)
        return torch.from_numpy(cdf).to(pmf.device)

    def _check_cdf_size(self):
        if self._quantized_cdf.numel() == 0:
            raise ValueError("Uninitialized CDFs. Run update() first")
        if len(self._quantized_cdf.size()) != 2:
            raise ValueError(f"Invalid CDF size {self._quantized_cdf.size()}")

    def _check_offsets_size(self):
        if self._offset.numel() == 0:
            raise ValueError("Uninitialized offsets. Run update() first")
        if len(self._offset.size()) != 1:
            raise ValueError(f"Invalid offsets size {self._offset.size()}")

    def _check_cdf_length(self):
        if self._cdf_length.numel() == 0:
            raise ValueError("Uninitialized CDF lengths. Run update() first")
        if len(self._cdf_length.size()) != 1:
            raise ValueError(f"Invalid offsets size {self._cdf_length.size()}")

    def _tables(self) -> "_coder.Tables":
        return _coder.Tables(self._quantized_cdf.cpu().numpy(), self._cdf_length.reshape(-1).cpu().numpy(),
                             self._offset.reshape(-1).cpu().numpy())

    def _host_tables(self) -> "_coder.Tables":
        """_tables(), cached: the three CDF buffers are copied to the host once and again only after one of them
        was replaced (update(), load_state_dict's resize, .to()) or written in place (load_state_dict's copy_).
        The cache holds the tensors it was built from, so an `is` test cannot be fooled by a recycled id."""
        bufs = (self._quantized_cdf, self._cdf_length, self._offset)
        cache = self.__dict__.get("_tables_cache")
        if cache is not None and cache.key is not None and all(a is b and a._version == v
                                                               for a, (b, v) in zip(bufs, cache.key)):
            return cache.tables
        tables = self._tables()
        self.__dict__["_tables_cache"] = _TablesCache([(t, t._version) for t in bufs], tables)
        return tables

    def _check_coding_state(self):
        self._check_cdf_size()
        self._check_cdf_length()
        self._check_offsets_size()

    def _stage_out(self, symbols: torch.Tensor, indexes: torch.Tensor, slot, key, threads: int) -> PendingStrings:
        """Non-blocking copies of dense int32 [B, n] device symbols / indexes into pinned memory, an event behind
        them, and the pending strings."""
        B, n = symbols.shape
        host = [_staging(slot, (key, name), B * n).reshape(B, n) for name in ("symbols", "indexes")]
        host[0].copy_(symbols, non_blocking=True)
        host[1].copy_(indexes, non_blocking=True)
        event = torch.cuda.Event(blocking=True)     # a waiting worker sleeps, it does not spin
        event.record()
        return PendingStrings(host[0], host[1], event, self._host_tables(), B, threads)

    def _compress_deferred(self, inputs, scales, means, slot=None, key=None, threads: int = 1):
        """(x_hat, PendingStrings).  scales given: the GaussianConditional's form (indexes from the scales, means per
        element); scales None: the EntropyBottleneck's (means = the per-channel medians [C], index = channel).
        4-D fp32 CUDA inputs take one launch of the coding front end; other inputs take the composed ops, so that
        their bytes stay those of compress()."""
        _check_cuda(inputs)
        if inputs.dim() < 2:
            raise ValueError("Invalid `inputs` size. Expected a tensor with at least 2 dimensions.")
        self._check_coding_state()
        B = inputs.size(0)
        per_channel = scales is None
        if _fused_coding(inputs) and (per_channel or _fused_coding(scales, means)):
            n = inputs.numel() // B
            symbols = torch.empty((B, n), dtype=torch.int32, device=inputs.device)
            indexes = torch.empty((B, n), dtype=torch.int32, device=inputs.device)
            if per_channel:
                x_hat = code_front_channels(inputs, means, symbols, indexes)
            else:
                x_hat = code_front(inputs, scales, means, self.scale_table, self._scale_bound_value, symbols, indexes)
        else:
            if per_channel:
                indexes = self._build_indexes(inputs.size()).to(inputs.device)
                medians = self._extend_ndims(means, inputs.dim() - 2).expand(B, *([-1] * (inputs.dim() - 1)))
                sym = self.quantize(inputs, "symbols", medians)
                x_hat = self.dequantize(sym, medians)        # what decompress(compress(x)) returns
            else:
                indexes = self.build_indexes(scales)
                sym = self.quantize(inputs, "symbols", means)
                x_hat = self.quantize(inputs, "dequantize", means)
            symbols = sym.reshape(B, -1).contiguous()
            indexes = indexes.reshape(B, -1).int().contiguous()
        return x_hat, self._stage_out(symbols, indexes, slot, key, threads)

    def _decompress_deferred(self, strings, indexes: torch.Tensor, finish, slot=None, key=None,
                             threads: int = 1) -> PendingSymbols:
        """indexes: dense int32 [B, n] on the device (or a host tensor); finish(host symbols [B, n]) -> x_hat."""
        if not isinstance(strings, (tuple, list)):
            raise ValueError("Invalid `strings` parameter type.")
        if len(strings) != indexes.size(0):
            raise ValueError("Invalid strings or indexes parameters")
        self._check_coding_state()
        B, n = indexes.shape
        event = None
        if indexes.is_cuda:
            host_idx = _staging(slot, (key, "indexes"), B * n).reshape(B, n)
            host_idx.copy_(indexes, non_blocking=True)
            event = torch.cuda.Event(blocking=True)     # a waiting worker sleeps, it does not spin
            event.record()
        else:
            host_idx = indexes
        out = _staging(slot, (key, "symbols"), B * n).reshape(B, n)
        return PendingSymbols(strings, host_idx, out, event, self._host_tables(), finish, threads, slot)

    def compress(self, inputs, indexes, means=None):
        """entropy_models.py:237-270: one rANS string per batch element."""
        if len(inputs.size()) < 2:
            raise ValueError("Invalid `inputs` size. Expected a tensor with at least 2 dimensions.")
        if inputs.size() != indexes.size():
            raise ValueError("`inputs` and `indexes` should have the same size.")
        self._check_cdf_size()
        self._check_cdf_length()
        self._check_offsets_size()
        symbols = self.quantize(inputs, "symbols", means)
        B = symbols.size(0)
        sym = symbols.reshape(B, -1).cpu().numpy()
        idx = indexes.reshape(B, -1).int().cpu().numpy()
        return _coder.encode_streams(sym, idx, self._tables(), B)

    def decompress(self, strings, indexes, dtype: torch.dtype = torch.float, means: torch.Tensor = None):
        """entropy_models.py:272-327."""
        if not isinstance(strings, (tuple, list)):
            raise ValueError("Invalid `strings` parameter type.")
        if not len(strings) == indexes.size(0):
            raise ValueError("Invalid strings or indexes parameters")
        if len(indexes.size()) < 2:
            raise ValueError("Invalid `indexes` size. Expected a tensor with at least 2 dimensions.")
        self._check_cdf_size()
        self._check_cdf_length()
        self._check_offsets_size()
        if means is not None:
            if means.size()[:2] != indexes.size()[:2]:
                raise ValueError("Invalid means or indexes parameters")
            if means.size() != indexes.size():
                for i in range(2, len(indexes.size())):
                    if means.size(i) != 1:
                        raise ValueError("Invalid means parameters")
        vals = _coder.decode_streams(strings, indexes.reshape(len(strings), -1).int().cpu().numpy(), self._tables())
        outputs = torch.from_numpy(vals).to(self._quantized_cdf.device).reshape(indexes.size())
        return self.dequantize(outputs, means, dtype)


class EntropyBottleneck(EntropyModel):
    _offset: torch.Tensor

    def __init__(self, channels: int, *args: Any, tail_mass: float = 1e-9, init_scale: float = 10,
                 filters: Tuple[int, ...] = (3, 3, 3, 3), **kwargs: Any):
        super().__init__(*args, **kwargs)
        self.channels = int(channels)
        self.filters = tuple(int(f) for f in filters)
        if self.filters != (3, 3, 3, 3):
            raise ValueError("the fused EntropyBottleneck kernel implements filters=(3, 3, 3, 3)")
        self.init_scale = float(init_scale)
        self.tail_mass = float(tail_mass)
        widths = (1,) + self.filters + (1,)
        scale = self.init_scale ** (1 / (len(self.filters) + 1))
        for i in range(len(self.filters) + 1):
            init = np.log(np.expm1(1 / scale / widths[i + 1]))
            self.register_parameter(f"_matrix{i:d}",
                                    nn.Parameter(torch.Tensor(self.channels, widths[i + 1], widths[i]).fill_(init)))
            b = torch.Tensor(self.channels, widths[i + 1], 1)
            nn.init.uniform_(b, -0.5, 0.5)
            self.register_parameter(f"_bias{i:d}", nn.Parameter(b))
            if i < len(self.filters):
                self.register_parameter(f"_factor{i:d}", nn.Parameter(torch.zeros(self.channels, widths[i + 1], 1)))
        self.quantiles = nn.Parameter(
            torch.Tensor([-self.init_scale, 0, self.init_scale]).repeat(self.channels, 1, 1))
        target = np.log(2 / self.tail_mass - 1)
        self.register_buffer("target", torch.Tensor([-target, 0, target]))

    def _params(self) -> List[torch.Tensor]:
        return ([getattr(self, f"_matrix{i}") for i in range(5)] + [getattr(self, f"_bias{i}") for i in range(5)]
                + [getattr(self, f"_factor{i}") for i in range(4)])

    def _get_medians(self) -> torch.Tensor:
        return self.quantiles[:, :, 1:2]

    def loss(self) -> torch.Tensor:
        return BottleneckAuxFn.apply(self.quantiles, self.target, *self._params())

    def forward(self, x: torch.Tensor, training: Optional[bool] = None, noise: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """noise: the U(-1/2, 1/2) draw to use in training mode (the models' concurrent forward draws it on the
        caller's stream before forking the hyper branch, so every draw of a step runs on one stream); None
        draws it here, as the reference does (entropy_models.py:495-540)."""
        if training is None:
            training = self.training
        if x.dim() < 2 or x.shape[1] != self.channels:
            raise ValueError(f"expected [B, {self.channels}, ...] input, got {tuple(x.shape)}")
        if training and noise is None:
            noise = _noise_for(x)
        elif training and tuple(noise.shape) != tuple(x.shape):
            raise ValueError(f"noise shape {tuple(noise.shape)} does not match the input's {tuple(x.shape)}")
        elif not training:
            noise = None
        return BottleneckFn.apply(x, self.quantiles, noise, Q_NOISE if training else Q_DEQUANTIZE,
                                  self._lik_bound(), *self._params())

    @staticmethod
    def _build_indexes(size):
        dims = len(size)
        view_dims = np.ones((dims,), dtype=np.int64)
        view_dims[1] = -1
        return torch.arange(size[1]).view(*view_dims).int().repeat(size[0], 1, *size[2:])

    @staticmethod
    def _extend_ndims(tensor, n):
        return tensor.reshape(-1, *([1] * n)) if n > 0 else tensor.reshape(-1)

    def _logits_cumulative(self, inputs: torch.Tensor, stop_gradient: bool) -> torch.Tensor:
        """entropy_models.py:457-477 in torch ops, for update() only (the training / eval
        forward runs the fused cai_eb_* kernels)."""
        logits = inputs
        for i in range(len(self.filters) + 1):
            matrix = getattr(self, f"_matrix{i:d}")
            bias = getattr(self, f"_bias{i:d}")
            if stop_gradient:
                matrix, bias = matrix.detach(), bias.detach()
            logits = torch.matmul(torch.nn.functional.softplus(matrix), logits) + bias
            if i < len(self.filters):
                factor = getattr(self, f"_factor{i:d}")
                if stop_gradient:
                    factor = factor.detach()
                logits = logits + torch.tanh(factor) * torch.tanh(logits)
        return logits

    @torch.no_grad()
    def update(self, force: bool = False) -> bool:
        """entropy_models.py:396-441."""
        if self._offset.numel() > 0 and not force:
            return False
        medians = self.quantiles[:, 0, 1]
        minima = torch.clamp(torch.ceil(medians - self.quantiles[:, 0, 0]).int(), min=0)
        maxima = torch.clamp(torch.ceil(self.quantiles[:, 0, 2] - medians).int(), min=0)
        self._offset = -minima
        pmf_start = medians - minima
        pmf_length = maxima + minima + 1
        max_length = int(pmf_length.max().item())
        samples = torch.arange(max_length, device=pmf_start.device)
        samples = samples[None, :] + pmf_start[:, None, None]
        half = float(0.5)
        lower = self._logits_cumulative(samples - half, stop_gradient=True)
        upper = self._logits_cumulative(samples + half, stop_gradient=True)
        sign = -torch.sign(lower + upper)
        pmf = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower))[:, 0, :]
        tail_mass = torch.sigmoid(lower[:, 0, :1]) + torch.sigmoid(-upper[:, 0, -1:])
        self._quantized_cdf = self._pmf_to_cdf(pmf, tail_mass, pmf_length, max_length)
        self._cdf_length = pmf_length + 2
        return True

    def compress(self, x):
        """entropy_models.py:559-567."""
        indexes = self._build_indexes(x.size()).to(x.device)
        medians = self._get_medians().detach()
        spatial_dims = len(x.size()) - 2
        medians = self._extend_ndims(medians, spatial_dims)
        medians = medians.expand(x.size(0), *([-1] * (spatial_dims + 1)))
        return super().compress(x, indexes, medians)

    def decompress(self, strings, size):
        """entropy_models.py:569-574."""
        output_size = (len(strings), self._quantized_cdf.size(0), *size)
        indexes = self._build_indexes(output_size).to(self._quantized_cdf.device)
        medians = self._extend_ndims(self._get_medians().detach(), len(size))
        medians = medians.expand(len(strings), *([-1] * (len(size) + 1)))
        return super().decompress(strings, indexes, medians.dtype, medians)

    def compress_deferred(self, x, slot=None, key="z", threads: int = 1):
        """(x_hat, PendingStrings): x_hat -- what decompress(compress(x), x.size()[2:]) returns -- comes from the
        device at once (the coding front end for 4-D fp32 inputs); pending.result() is compress(x)."""
        return self._compress_deferred(x, None, self._get_medians().detach().reshape(-1), slot, key, threads)

    def _host_indexes(self, B: int, size) -> torch.Tensor:
        """_build_indexes on the host, int32 [B, C prod(size)], cached per shape: no device round trip."""
        C = int(self._quantized_cdf.size(0))
        shape = (int(B), C, int(np.prod(size)) if len(size) else 1)
        cache = self.__dict__.setdefault("_host_index_cache", {})
        idx = cache.get(shape)
        if idx is None:
            if len(cache) > 8:
                cache.clear()
            a = np.broadcast_to(np.arange(C, dtype=np.int32)[None, :, None], shape)
            idx = cache[shape] = torch.from_numpy(np.array(a).reshape(shape[0], -1))     # a copy: writable, dense
        return idx

    def decompress_host(self, strings, size, slot=None, key="z", threads: Optional[int] = None):
        """decompress(strings, size) without a device round trip before the coder: host-built indexes, cached
        tables, the decoded symbols through pinned memory and the coding back end (2-D sizes)."""
        size = tuple(int(s) for s in size)
        B = len(strings)
        C = int(self._quantized_cdf.size(0))
        device = self._quantized_cdf.device
        medians = self._get_medians().detach()

        def finish(host):
            sym = host.to(device, non_blocking=True)
            if len(size) == 2 and sym.is_cuda and medians.dtype == torch.float32:
                return code_back(sym, medians.reshape(-1), (B, C) + size)
            m = self._extend_ndims(medians, len(size)).expand(B, *([-1] * (len(size) + 1)))
            return self.dequantize(sym.reshape((B, C) + size), m, m.dtype)

        if threads is None:
            threads = _coder.default_threads()
        return self._decompress_deferred(strings, self._host_indexes(B, size), finish, slot, key, threads).finish()


class GaussianConditional(EntropyModel):
    def __init__(self, scale_table: Optional[Union[List, Tuple]], *args: Any, scale_bound: float = 0.11,
                 tail_mass: float = 1e-9, **kwargs: Any):
        super().__init__(*args, **kwargs)
        if not isinstance(scale_table, (type(None), list, tuple)):
            raise ValueError(f'Invalid type for scale_table "{type(scale_table)}"')
        if isinstance(scale_table, (list, tuple)) and len(scale_table) < 1:
            raise ValueError(f'Invalid scale_table length "{len(scale_table)}"')
        if scale_table and (list(scale_table) != sorted(scale_table) or any(s <= 0 for s in scale_table)):
            raise ValueError(f'Invalid scale_table "({scale_table})"')
        self.tail_mass = float(tail_mass)
        if scale_bound is None and scale_table:
            scale_bound = scale_table[0]
        if scale_bound is None or scale_bound <= 0:
            raise ValueError("Invalid parameters")
        self.lower_bound_scale = LowerBound(scale_bound)
        self._scale_bound_value = float(scale_bound)
        self.register_buffer("scale_table",
                             torch.Tensor(tuple(float(s) for s in scale_table)) if scale_table else torch.Tensor())
        self.register_buffer("scale_bound", torch.Tensor([float(scale_bound)]))

    @staticmethod
    def _prepare_scale_table(scale_table):
        return torch.Tensor(tuple(float(s) for s in scale_table))

    def forward(self, inputs: torch.Tensor, scales: torch.Tensor, means: Optional[torch.Tensor] = None,
                training: Optional[bool] = None, noise: Optional[torch.Tensor] = None, scales_relu: bool = False
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """noise: the U(-1/2, 1/2) draw to use in training mode (the models' concurrent forward shares one
        draw between g_s's input and this likelihood); None draws it here, as the reference does.
        scales_relu: the scales are the output of a ReLU whose backward mask this op applies (the producer ran
        with act_bwd_downstream: ScaleHyperprior's h_s)."""
        if training is None:
            training = self.training
        # the reference's _likelihood broadcasts scales / means against the inputs (entropy_models.py:692-709)
        try:
            if scales.shape != inputs.shape:
                scales = scales.expand_as(inputs)
            if means is not None and means.shape != inputs.shape:
                means = means.expand_as(inputs)
        except RuntimeError as e:
            raise ValueError(f"scales / means do not broadcast to the inputs' shape {tuple(inputs.shape)}") from e
        if training and noise is None:
            noise = _noise_for(inputs)
        elif not training:
            noise = None
        sb = self._scale_bound_value
        return GaussianFn.apply(inputs, scales, means, noise, Q_NOISE if training else Q_DEQUANTIZE, sb,
                                self._lik_bound(), bool(scales_relu))

    def build_indexes(self, scales: torch.Tensor) -> torch.Tensor:
        scales = torch.clamp_min(scales, self._scale_bound_value)
        indexes = scales.new_full(scales.size(), len(self.scale_table) - 1).int()
        for s in self.scale_table[:-1]:
            indexes -= (scales <= s).int()
        return indexes

    def compress_deferred(self, inputs, scales, means, slot=None, key="y", threads: int = 1):
        """(x_hat, PendingStrings): x_hat = quantize(inputs, "dequantize", means) at once; pending.result() is
        compress(inputs, build_indexes(scales), means).  4-D fp32 inputs: one launch of the coding front end."""
        if scales.size() != inputs.size() or means is None or means.size() != inputs.size():
            raise ValueError("`inputs`, `scales` and `means` should have the same size.")
        return self._compress_deferred(inputs, scales, means, slot, key, threads)

    def decompress_deferred(self, strings, scales, means, dtype: torch.dtype = torch.float, slot=None, key="y",
                            threads: int = 1) -> PendingSymbols:
        """The pending form of decompress(strings, build_indexes(scales), dtype, means): the index launch and the
        copy of the indexes are issued here, ``run()`` decodes on whichever thread calls it, ``finish()`` (main
        thread) copies the symbols to the device and returns x_hat."""
        _check_cuda(scales, means)
        if means is None or means.size() != scales.size():
            raise ValueError("Invalid means or indexes parameters")
        B = scales.size(0)
        device = scales.device
        if _fused_coding(scales, means):
            shape = tuple(scales.shape)
            indexes = torch.empty((B, scales.numel() // B), dtype=torch.int32, device=device)
            code_indexes(scales, self.scale_table, self._scale_bound_value, indexes)

            def finish(host):
                return code_back(host.to(device, non_blocking=True), means, shape)
        else:
            full = self.build_indexes(scales)
            indexes = full.reshape(B, -1).int().contiguous()

            def finish(host):
                return self.dequantize(host.to(device, non_blocking=True).reshape(full.size()), means, dtype)
        return self._decompress_deferred(strings, indexes, finish, slot, key, threads)

    @staticmethod
    def _standardized_cumulative(inputs: torch.Tensor) -> torch.Tensor:
        """entropy_models.py:629-635 (update() only; the likelihood kernels use the same erfc form)."""
        half = float(0.5)
        const = float(-(2 ** -0.5))
        return half * torch.erfc(const * inputs)

    @staticmethod
    def _standardized_quantile(quantile):
        return scipy.stats.norm.ppf(quantile)

    def update_scale_table(self, scale_table, force=False):
        """entropy_models.py:643-652."""
        if self._offset.numel() > 0 and not force:
            return False
        device = self.scale_table.device
        self.scale_table = self._prepare_scale_table(scale_table).to(device)
        self.update()
        return True

    @torch.no_grad()
    def update(self):
        """entropy_models.py:655-678 (without the reference's debug prints, :680-689)."""
        multiplier = -self._standardized_quantile(self.tail_mass / 2)
        pmf_center = torch.ceil(self.scale_table * multiplier).int()
        pmf_length = 2 * pmf_center + 1
        max_length = int(torch.max(pmf_length).item())
        device = pmf_center.device
        samples = torch.abs(torch.arange(max_length, device=device).int() - pmf_center[:, None]).float()
        samples_scale = self.scale_table.unsqueeze(1).float()
        upper = self._standardized_cumulative((0.5 - samples) / samples_scale)
        lower = self._standardized_cumulative((-0.5 - samples) / samples_scale)
        pmf = upper - lower
        tail_mass = 2 * lower[:, :1]
        self._quantized_cdf = self._pmf_to_cdf(pmf, tail_mass, pmf_length, max_length)
        self._offset = -pmf_center
        self._cdf_length = pmf_length + 2
