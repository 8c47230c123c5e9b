"""Frames in flight on the GPU: the coding front end / back end kernels (csrc/code_front.hip) against the composed
ops they replace, the cached CDF tables, one livened _StreamPrior, and the video codec end to end.

Kernels.  Everything is an equality: the integers must be the ones ``quantize("symbols")``, ``build_indexes`` /
``_build_indexes`` and ``.reshape(B, -1)`` produce today and x_hat must pass ``torch.equal`` against
``quantize("dequantize")`` / ``EntropyModel.dequantize``, otherwise the bytes change.  Shapes: B in {1, 2}, C in
{1, 5, 64, 192}, (H, W) in {(1, 1), (3, 5), (8, 8), (17, 33)} -- one element, a partial tile on both axes with no
16-byte access possible, exactly one pixel tile, and 561 pixels (nine pixel tiles, the last one partial; with C = 192
three channel tiles; with C = 5 and 1 a partial channel tile).  C = 64 / 192 with H W % 4 == 0 take the 16-byte
accesses on both sides, (17, 33) and (3, 5) the scalar integer side, C = 1 / 5 the scalar float side.  Strides: ld = C,
and ld = 2 C with scales and means the two halves of one buffer (for C = 5 and 1 the means half is not 16-byte
aligned).  Inputs are seeded and hit the edges: scales below the bound, equal to table entries (the ``<=``), above
the last entry; x - mean at exact .5 ties (round half to even); magnitudes beyond every CDF (bypass escapes).

End to end: the livened ssf2020(1) and the moving clip of test_codec_video_gpu.py, 5 frames of 208 x 176 at 8 bit and 3
at 10 bit.  Files, decoded files, the evaluation's dictionary and ``net.compress`` / ``decompress`` under
frames_in_flight = W must equal W = 1 exactly.  A truncated stream under W = 4 ends in the reader's ValueError with no
worker thread left (a host-side error path: nothing on the device is provoked).
"""
import contextlib
import ctypes
import signal
import threading
import time

import pytest
import torch

import video_reference as R
from test_video_eval_gpu import NAMES, H, W, liven

pytestmark = pytest.mark.gpu

BATCHES = (1, 2)
CHANNELS = (1, 5, 64, 192)
GRIDS = ((1, 1), (3, 5), (8, 8), (17, 33))


# ---------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gc(cuda):
    from compressai.entropy_models import GaussianConditional
    from compressai.models.google import get_scale_table

    m = GaussianConditional(None).to(cuda)
    m.update_scale_table(get_scale_table())
    return m


def _residuals(g, shape):
    """x - mean values: ordinary ones, exact .5 ties of both signs, and escapes far outside every CDF."""
    r = torch.randn(shape, generator=g) * 3.0
    kind = torch.randint(0, 10, shape, generator=g)
    ties = torch.randint(-6, 6, shape, generator=g).float() + 0.5
    r = torch.where(kind == 0, ties, r)
    r = torch.where(kind == 1, torch.full(shape, 1.0e5), r)
    r = torch.where(kind == 2, torch.full(shape, -float(1 << 20)), r)
    r = torch.where(kind == 3, torch.full(shape, 300.49), r)
    return r


def _latent(cuda, gc, B, C, Hh, Ww, seed):
    """(x, scales, means) as pixel-major [B, C, H, W] views; means on a 1/8 grid so that x - mean is exact."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, Hh, Ww, C)
    table = gc.scale_table.cpu()
    scales = torch.exp(torch.randn(shape, generator=g) * 2.0)
    kind = torch.randint(0, 8, shape, generator=g)
    scales = torch.where(kind == 0, torch.full(shape, 0.05), scales)                    # below the bound
    scales = torch.where(kind == 1, torch.full(shape, 0.11), scales)                    # the bound = table[0]
    entries = table[torch.randint(0, table.numel(), shape, generator=g)]
    scales = torch.where(kind == 2, entries, scales)                                    # exactly an entry: the <=
    scales = torch.where(kind == 3, torch.full(shape, 300.0), scales)                   # above the last entry
    scales = torch.where(kind == 4, torch.full(shape, float(table[-1])), scales)
    means = torch.randint(-40, 40, shape, generator=g).float() / 8.0
    res = _residuals(g, shape)
    x = means + res
    d = x - means
    tie = res.abs() % 1 == 0.5
    assert torch.equal(d[tie], res[tie])        # exact in fp32 (means on a 1/8 grid): the ties are ties
    assert res.numel() < 64 or (tie.any() and (d.abs() > 1000).any())
    return tuple(t.to(cuda).permute(0, 3, 1, 2) for t in (x, scales, means))


def _halves(scales, means):
    """scales and means as the channel halves of one pixel-major buffer (ld = 2 C)."""
    B, C, Hh, Ww = scales.shape
    buf = torch.empty((B, Hh, Ww, 2 * C), dtype=torch.float32, device=scales.device)
    buf[..., :C] = scales.permute(0, 2, 3, 1)
    buf[..., C:] = means.permute(0, 2, 3, 1)
    v = buf.permute(0, 3, 1, 2)
    return v[:, :C], v[:, C:]


def _ints(cuda, B, n):
    return torch.full((B, n), -7, dtype=torch.int32, device=cuda), torch.full((B, n), -7, dtype=torch.int32, device=cuda)


# ---------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("C", CHANNELS)
def test_front_end_per_element_matches_the_composed_ops(cuda, gc, C, grid):
    from compressai import _ops

    Hh, Ww = grid
    for B in BATCHES:
        x, scales, means = _latent(cuda, gc, B, C, Hh, Ww, seed=1000 * C + 10 * Hh + B)
        want_sym = gc.quantize(x, "symbols", means).reshape(B, -1)
        want_idx = gc.build_indexes(scales).reshape(B, -1)
        want_hat = gc.quantize(x, "dequantize", means)
        assert torch.equal(want_hat, gc.dequantize(gc.quantize(x, "symbols", means), means))
        for name, (s, m) in (("ld = C", (scales, means)), ("ld = 2C", _halves(scales, means))):
            assert _ops.pixel_major_ld(s) == (C if name == "ld = C" else 2 * C) or Hh * Ww * B == 1
            sym, idx = _ints(cuda, B, C * Hh * Ww)
            x_hat = _ops.code_front(x, s, m, gc.scale_table, gc._scale_bound_value, sym, idx)
            assert torch.equal(sym, want_sym), (name, B)
            assert torch.equal(idx, want_idx), (name, B)
            assert tuple(x_hat.shape) == tuple(x.shape) and torch.equal(x_hat, want_hat), (name, B)
            only = torch.full_like(idx, -7)
            _ops.code_indexes(s, gc.scale_table, gc._scale_bound_value, only)
            assert torch.equal(only, want_idx), (name, B)
        # the edges were there
        assert Hh * Ww * C * B < 64 or ((want_idx == 0).any() and (want_idx == 63).any() and (want_sym.abs() > 1000).any())


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("C", CHANNELS)
def test_front_end_per_channel_matches_the_composed_ops(cuda, C, grid):
    from compressai import _ops
    from compressai.entropy_models import EntropyBottleneck

    Hh, Ww = grid
    g = torch.Generator().manual_seed(77 + C)
    eb = EntropyBottleneck(C).to(cuda)
    with torch.no_grad():
        eb.quantiles[:, 0, 1] = (torch.randint(-20, 20, (C,), generator=g).float() / 8.0).to(cuda)
    medians = eb._get_medians().detach()
    for B in BATCHES:
        z = (medians.cpu().reshape(1, 1, 1, C) + _residuals(g, (B, Hh, Ww, C))).to(cuda).permute(0, 3, 1, 2)
        m = medians.reshape(1, C, 1, 1).expand(B, C, Hh, Ww)
        want_sym = eb.quantize(z, "symbols", m)
        want_hat = eb.dequantize(want_sym, m)
        assert torch.equal(want_hat, eb.quantize(z, "dequantize", m))
        sym, idx = _ints(cuda, B, C * Hh * Ww)
        z_hat = _ops.code_front_channels(z, medians, sym, idx)
        assert torch.equal(sym, want_sym.reshape(B, -1)), B
        assert torch.equal(idx, eb._build_indexes(z.size()).to(cuda).reshape(B, -1)), B
        assert torch.equal(z_hat, want_hat), B
        back = _ops.code_back(sym, medians, tuple(z.shape))
        assert torch.equal(back, want_hat), B


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("C", CHANNELS)
def test_back_end_matches_dequantize(cuda, gc, C, grid):
    from compressai import _ops

    Hh, Ww = grid
    for B in BATCHES:
        _, scales, means = _latent(cuda, gc, B, C, Hh, Ww, seed=5000 + 1000 * C + 10 * Hh + B)
        g = torch.Generator().manual_seed(C + Hh + B)
        sym = torch.randint(-300, 300, (B, C, Hh, Ww), generator=g, dtype=torch.int32)
        sym[torch.rand(sym.shape, generator=g) < 0.05] = 1 << 20
        sym = sym.to(cuda)
        want = gc.dequantize(sym, means)
        flat = sym.reshape(B, -1).contiguous()
        for name, m in (("ld = C", means), ("ld = 2C", _halves(scales, means)[1])):
            got = _ops.code_back(flat, m, (B, C, Hh, Ww))
            assert got.dtype == torch.float32 and torch.equal(got, want), (name, B)


def test_einval_through_the_c_abi():
    """Validation precedes any device work: the pointers are not device memory, so a call that got past it to a
    launch could not return CAI_EINVAL."""
    from compressai import _native

    lib = _native.lib.load()
    P = ctypes.c_void_p(4096)

    def front(x=P, x_ld=8, scales=P, s_ld=8, means=P, m_ld=8, tab=P, L=64, B=1, Hh=2, Ww=2, C=8, x_hat=P, xh_ld=8,
              sym=P, idx=P):
        return lib.cai_code_front(x, x_ld, scales, s_ld, means, m_ld, tab, L, 0.11, B, Hh, Ww, C, x_hat, xh_ld, sym,
                                  idx, None)

    def back(sym=P, means=P, m_ld=8, B=1, Hh=2, Ww=2, C=8, x_hat=P, xh_ld=8):
        return lib.cai_code_back(sym, means, m_ld, B, Hh, Ww, C, x_hat, xh_ld, None)

    bad = [
        (lambda: front(idx=None), b"null pointer"), (lambda: front(sym=None), b"null pointer"),
        (lambda: front(x_hat=None), b"null pointer"), (lambda: front(means=None), b"null pointer"),
        (lambda: front(tab=None), b"null pointer"), (lambda: front(x=None, scales=None), b"null pointer"),
        (lambda: front(x_ld=7), b"pitch"), (lambda: front(m_ld=4), b"pitch"), (lambda: front(xh_ld=0), b"pitch"),
        (lambda: front(s_ld=7), b"scales pitch"), (lambda: front(L=0), b"scale table"),
        (lambda: front(B=0), b"bad shape"), (lambda: front(Hh=-1), b"bad shape"), (lambda: front(C=0), b"bad shape"),
        (lambda: front(B=1 << 11, Hh=1 << 10, Ww=1 << 10, C=8, x_ld=8), b"2^31"),
        (lambda: front(B=2, Hh=1 << 15, Ww=1 << 15, C=1), b"2^31"),
        (lambda: lib.cai_code_indexes(None, 8, P, 64, 0.11, 1, 2, 2, 8, P, None), b"null pointer"),
        (lambda: lib.cai_code_indexes(P, 8, P, 64, 0.11, 1, 2, 2, 8, None, None), b"null pointer"),
        (lambda: lib.cai_code_indexes(P, 4, P, 64, 0.11, 1, 2, 2, 8, P, None), b"pitch"),
        (lambda: back(sym=None), b"null pointer"), (lambda: back(means=None), b"null pointer"),
        (lambda: back(x_hat=None), b"null pointer"), (lambda: back(m_ld=4), b"pitch"), (lambda: back(xh_ld=7), b"pitch"),
        (lambda: back(Ww=0), b"bad shape"), (lambda: back(B=1 << 12, Hh=1 << 10, Ww=1 << 10, C=8), b"2^31"),
    ]
    for k, (call, fragment) in enumerate(bad):
        rc = call()
        msg = lib.cai_last_error()
        assert rc == _native.CAI_EINVAL, (k, rc, msg)
        assert fragment in msg and b"code_" in msg, (k, msg)
    with pytest.raises(ValueError, match="pitch"):
        _native.lib.cai_code_back(P, P, 4, 1, 2, 2, 8, P, 8, None)


# ---------------------------------------------------------------------------------------------------------
# entropy models: deferred forms and the table cache
# ---------------------------------------------------------------------------------------------------------
def test_deferred_entropy_models_give_the_blocking_bytes(cuda, gc):
    from compressai.entropy_models import EntropyBottleneck

    B, C, Hh, Ww = 2, 64, 17, 33
    x, scales, means = _latent(cuda, gc, B, C, Hh, Ww, seed=31)
    want = gc.compress(x, gc.build_indexes(scales), means)
    x_hat, pending = gc.compress_deferred(x, scales, means)
    assert torch.equal(x_hat, gc.quantize(x, "dequantize", means))
    assert pending.result() == want and pending.result() is pending.result()
    dec = gc.decompress_deferred(want, scales, means)
    assert torch.equal(dec.finish(), gc.decompress(want, gc.build_indexes(scales), torch.float, means))
    # other dtypes keep today's ops (and today's bytes): bf16 inputs
    xb, mb = x.bfloat16(), means.bfloat16()
    want_b = gc.compress(xb, gc.build_indexes(scales), mb)
    xb_hat, pend_b = gc.compress_deferred(xb, scales, mb)
    assert pend_b.result() == want_b and torch.equal(xb_hat, gc.quantize(xb, "dequantize", mb))
    dec_b = gc.decompress_deferred(want_b, scales, mb, torch.bfloat16)
    assert torch.equal(dec_b.finish(), gc.decompress(want_b, gc.build_indexes(scales), torch.bfloat16, mb))

    torch.manual_seed(3)
    eb = EntropyBottleneck(C).to(cuda)
    eb.update(force=True)
    z = torch.randn(B, C, 3, 5, device=cuda) * 4
    want_z = eb.compress(z)
    z_hat, pend_z = eb.compress_deferred(z)
    assert pend_z.result() == want_z
    assert torch.equal(z_hat, eb.decompress(want_z, (3, 5)))
    assert torch.equal(eb.decompress_host(want_z, (3, 5)), z_hat)


def test_cached_tables_are_not_copied_again(cuda, gc, monkeypatch):
    from compressai import _coder
    from compressai.entropy_models import EntropyBottleneck
    from compressai.entropy_models.entropy_models import EntropyModel

    built = []
    real = EntropyModel._tables

    def counting(self):
        built.append(type(self).__name__)
        return real(self)

    monkeypatch.setattr(EntropyModel, "_tables", counting)
    x, scales, means = _latent(cuda, gc, 1, 64, 8, 8, seed=5)
    gc.__dict__.pop("_tables_cache", None)
    first = gc.compress_deferred(x, scales, means)[1].result()           # the warm call
    assert built == ["GaussianConditional"]
    tables = gc._host_tables()
    assert isinstance(tables, _coder.Tables)
    for _ in range(3):
        assert gc.compress_deferred(x, scales, means)[1].result() == first
        gc.decompress_deferred(first, scales, means).finish()
    assert built == ["GaussianConditional"] and gc._host_tables() is tables     # no copy of _quantized_cdf
    gc.update_scale_table(gc.scale_table.tolist(), force=True)                      # replaces the buffers
    assert gc.compress_deferred(x, scales, means)[1].result() == first
    assert built == ["GaussianConditional"] * 2 and gc._host_tables() is not tables
    gc._quantized_cdf.add_(0)                                                        # written in place
    gc._host_tables()
    assert len(built) == 3

    torch.manual_seed(4)
    eb = EntropyBottleneck(8).to(cuda)
    eb.update(force=True)
    z = torch.randn(1, 8, 4, 4, device=cuda) * 3
    built.clear()
    a = eb.compress_deferred(z)[1].result()
    eb.decompress_host(a, (4, 4))
    assert eb.compress_deferred(z)[1].result() == a and built == ["EntropyBottleneck"]
    assert eb.update(force=True)
    assert eb.compress_deferred(z)[1].result() == a and built == ["EntropyBottleneck"] * 2
    eb.load_state_dict(eb.state_dict())                                              # copy_ in place
    eb._host_tables()
    assert len(built) == 3


# ---------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(cuda):
    from compressai.zoo import ssf2020

    torch.manual_seed(0)
    model = liven(ssf2020(1)).to(cuda).eval()
    model.update(force=True)
    return model


@pytest.mark.parametrize("shape", [(1, 192, 8, 16), (2, 192, 8, 8)], ids=str)
def test_stream_prior_deferred_equals_blocking(cuda, net, shape):
    from compressai._prepack import prepacked_forward

    prior = net.motion_hyperprior
    y = torch.randn(shape, generator=torch.Generator().manual_seed(shape[0]), dtype=torch.float32).mul(6.0).to(cuda)
    with torch.no_grad(), prepacked_forward(net):
        y_hat, coded = prior.compress(y)
        y_hat_d, pending = prior.compress_deferred(y)
        got = pending.result()
        assert [[bytes(s) for s in part] for part in got["strings"]] == coded["strings"]
        assert tuple(got["shape"]) == tuple(coded["shape"])
        assert max(len(s) for s in coded["strings"][0]) > 64          # a livened latent: real strings
        assert torch.equal(y_hat_d, y_hat)
        want = prior.decompress(coded["strings"], coded["shape"])
        begun = prior.decompress_begin(coded["strings"], coded["shape"])
        assert torch.equal(begun.finish(), want) and torch.equal(want, y_hat)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """{bitdepth: path}: 5 frames at 8 bit, 3 at 10 bit."""
    root = tmp_path_factory.mktemp("pipeline_clips")
    out = {}
    for bitdepth, n in ((8, 5), (10, 3)):
        path = root / NAMES[bitdepth]
        R.write_clip(path, R.moving_clip(H, W, n, bitdepth, seed=bitdepth), bitdepth)
        out[bitdepth] = (path, n)
    return out


@pytest.fixture(scope="module")
def serial(net, clips, tmp_path_factory):
    """What W = 1 leaves behind, computed once."""
    from compressai.utils.codec_rgbt import decode_video, encode_video
    from compressai.utils.video.eval_model.__main__ import eval_model

    root = tmp_path_factory.mktemp("pipeline_serial")
    out = {}
    for bitdepth, (path, n) in clips.items():
        a, rec, b = root / f"a{bitdepth}.bin", root / f"rec{bitdepth}_{W}x{H}.yuv", root / f"b{bitdepth}.bin"
        enc = encode_video(str(path), net, str(a), "mse", 3)
        hdr, last = decode_video(str(a), net, str(rec))
        results = eval_model(net, path, b, keep_binaries=True)
        assert enc["frames"] == hdr.frames == n
        out[bitdepth] = {"a": a.read_bytes(), "rec": rec.read_bytes(), "last": last, "results": results,
                         "b": b.read_bytes(), "path_a": a}
    return out


@pytest.mark.parametrize("window", [2, 4, 8])
@pytest.mark.parametrize("bitdepth", [8, 10])
def test_files_are_byte_identical_across_windows(net, clips, serial, tmp_path, bitdepth, window):
    from compressai.utils.codec_rgbt import decode_video, encode_video

    path, n = clips[bitdepth]
    before = threading.active_count()
    a, rec = tmp_path / "a.bin", tmp_path / f"rec_{W}x{H}.yuv"
    enc = encode_video(str(path), net, str(a), "mse", 3, frames_in_flight=window)
    assert a.read_bytes() == serial[bitdepth]["a"]
    assert enc["frames"] == n and enc["avg_frm_enc_time"] > 0
    hdr, last = decode_video(str(serial[bitdepth]["path_a"]), net, str(rec), frames_in_flight=window)
    assert rec.read_bytes() == serial[bitdepth]["rec"]
    assert hdr.frames == n and torch.equal(last, serial[bitdepth]["last"])
    assert threading.active_count() == before


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_evaluation_is_the_serial_runs(net, clips, serial, tmp_path, bitdepth):
    from compressai.utils.video.eval_model.__main__ import decode_sequence, eval_model

    path, _ = clips[bitdepth]
    b = tmp_path / "b.bin"
    results = eval_model(net, path, b, keep_binaries=True, frames_in_flight=4)
    assert results == serial[bitdepth]["results"]
    assert b.read_bytes() == serial[bitdepth]["b"]
    one, four = decode_sequence(net, b), decode_sequence(net, b, frames_in_flight=4)
    assert len(one) == len(four) and all(torch.equal(x, y) for x, y in zip(one, four))


def test_half_runs_keep_their_bytes(net, clips, tmp_path):
    from compressai.utils.video.eval_model.__main__ import decode_sequence, eval_model

    path, _ = clips[8]
    b1, b4 = tmp_path / "h1.bin", tmp_path / "h4.bin"
    want = eval_model(net, path, b1, keep_binaries=True, half=True)
    got = eval_model(net, path, b4, keep_binaries=True, half=True, frames_in_flight=4)
    assert got == want and b4.read_bytes() == b1.read_bytes()
    one, four = decode_sequence(net, b1, half=True), decode_sequence(net, b1, half=True, frames_in_flight=4)
    assert len(one) == len(four) == 5 and all(torch.equal(x, y) for x, y in zip(one, four))


def test_model_compress_and_decompress_in_flight(cuda, net):
    g = torch.Generator().manual_seed(12)
    frames = [torch.rand(2, 3, 128, 128, generator=g).to(cuda) for _ in range(3)]
    strings, shapes = net.compress(frames)
    strings4, shapes4 = net.compress(frames, frames_in_flight=4)
    assert strings4 == strings
    assert shapes4 == shapes
    want = net.decompress(strings, shapes)
    for window in (2, 4):
        got = net.decompress(strings, shapes, frames_in_flight=window)
        assert len(got) == len(want) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))


@contextlib.contextmanager
def _within(seconds):
    """Fail -- not stall -- if the body is still running after `seconds`: SIGALRM raises in the main thread, also
    while it waits for a worker, and the pipeline's exit then drains the pool."""
    def expired(signum, frame):
        raise TimeoutError(f"still running after {seconds} s")

    old = signal.signal(signal.SIGALRM, expired)
    signal.setitimer(signal.ITIMER_REAL, seconds)
    t0 = time.perf_counter()
    try:
        yield
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)
        signal.signal(signal.SIGALRM, old)
    assert time.perf_counter() - t0 < seconds


def test_fp32_frames_take_the_coding_kernels(cuda, net):
    """An in-flight inter frame in fp32 goes through cai_code_front / _indexes / _back, not through the composed
    ops: two streams, each with a z and a y latent."""
    from compressai import _ledger
    from compressai._prepack import prepacked_forward

    g = torch.Generator().manual_seed(3)
    x_ref, x_cur = (torch.rand(1, 3, 128, 128, generator=g).to(cuda) for _ in range(2))
    with torch.no_grad(), prepacked_forward(net):
        with _ledger.recording(keep_replay=False) as led:
            x_rec, pending = net.encode_inter_deferred(x_cur, x_ref)
        kinds = [e.kind for e in led.entries]
        assert kinds.count("code_front") == 4 and "code_indexes" not in kinds and "code_back" not in kinds
        info = pending.result()
        with _ledger.recording(keep_replay=False) as led:
            begun = net.decode_inter_begin(info["strings"], info["shape"])
            x_dec = begun.finish(x_ref)
        kinds = [e.kind for e in led.entries]
        assert kinds.count("code_indexes") == 2 and kinds.count("code_back") == 4 and "code_front" not in kinds
        assert torch.equal(x_dec, net.decode_inter(x_ref, info["strings"], info["shape"]))
        assert torch.equal(x_rec, net.encode_inter(x_cur, x_ref)[0])


def test_truncated_stream_in_flight(net, serial, tmp_path):
    """The reader's ValueError reaches the caller through the pipeline, with the pool drained and joined, within the
    test's normal time.  The error is raised by the file reader on the host; nothing is launched for the frame that
    cannot be read.  The bound: the whole five-frame decode takes well under a second (the serial fixture decodes it
    several times in that), so 20 s is two orders of magnitude of slack and still far from a stalled suite."""
    from compressai.utils.codec_rgbt import decode_video

    before = threading.active_count()
    short = tmp_path / "short.bin"
    short.write_bytes(serial[8]["a"][:-3])
    with _within(20.0):
        with pytest.raises(ValueError, match="truncated"):
            decode_video(str(short), net, str(tmp_path / f"short_{W}x{H}.yuv"), frames_in_flight=4)
    assert threading.active_count() == before
    assert not [t for t in threading.enumerate() if t.name.startswith("cai-coder")]
    # a stream cut inside the header fails before the pipeline starts
    short.write_bytes(serial[8]["a"][:9])
    with pytest.raises(ValueError, match="truncated"):
        decode_video(str(short), net, None, frames_in_flight=4)
    assert threading.active_count() == before
