"""Frames in flight without a GPU: the scheduler of compressai/utils/video/pipeline.py on fake jobs, the host coder
called from several threads at once, and the command-line flags.

Scheduler (fake jobs that sleep a few milliseconds of seeded jitter, so completion order differs from frame order):
results arrive in frame order; never more than W frames are between issue and delivery (counted by the test's own
issue / deliver callbacks, and by the pipeline's high-water mark); W above the frame count works; a job that raises
at frame k surfaces at frame k, no later frame is delivered, and the worker threads are gone when the exception
reaches the caller; the same for an exception of the caller's own issue callback; W < 1 is a ValueError.

Host coder: cai_rans_encode / cai_rans_decode of libcai_coder.so, entered from 8 threads at once through ctypes
(which releases the GIL) on seeded symbol lists that include bypass escapes, return the bytes and the symbols of the
serial calls.  This is what the pool relies on: the coder keeps no state between calls.
"""
import random
import threading
import time

import numpy as np
import pytest

from compressai import _coder
from compressai.utils.video import pipeline as P


# ---------------------------------------------------------------------------------------------------------
# the scheduler
# ---------------------------------------------------------------------------------------------------------
class Recorder:
    """issue / deliver callbacks around fake jobs; counts what is in flight."""

    def __init__(self, jobs_per_frame=3, fail_at=None, fail_in_issue=None, seed=0):
        self.rng = random.Random(seed)
        self.jobs_per_frame, self.fail_at, self.fail_in_issue = jobs_per_frame, fail_at, fail_in_issue
        self.issued, self.delivered, self.in_flight, self.max_in_flight = [], [], 0, 0
        self.events = []
        self.worker_threads = set()

    def job(self, i, j, delay):
        def run():
            self.worker_threads.add(threading.current_thread().name)
            time.sleep(delay)
            if self.fail_at == i and j == 1:
                raise OSError(f"job {j} of frame {i} failed")
            return (i, j)
        return run

    def issue(self, i):
        if self.fail_in_issue == i:
            raise KeyError(f"issue {i}")
        self.issued.append(i)
        self.events.append(("issue", i))
        self.in_flight += 1
        self.max_in_flight = max(self.max_in_flight, self.in_flight)
        # earlier frames sleep longer: they finish after the later ones unless the order is enforced
        delays = [self.rng.uniform(0.0, 0.004) + (0.006 if i % 3 == 0 else 0.0) for _ in range(self.jobs_per_frame)]
        return {"frame": i}, [self.job(i, j, d) for j, d in enumerate(delays)]

    def deliver(self, i, payload, results):
        assert payload == {"frame": i}
        assert results == [(i, j) for j in range(self.jobs_per_frame)]
        self.in_flight -= 1
        self.delivered.append(i)
        self.events.append(("deliver", i))


@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_results_arrive_in_frame_order_and_the_window_holds(W):
    n = 13
    before = threading.active_count()
    r = Recorder(seed=W)
    P.run_ordered(n, W, r.issue, r.deliver)
    assert r.issued == r.delivered == list(range(n))
    assert r.max_in_flight == min(W, n)
    assert r.in_flight == 0
    # frame i is delivered before frame i + W is issued, and not before frame i + W - 1 is (the window is used)
    pos = {e: k for k, e in enumerate(r.events)}
    for i in range(n):
        if i + W < n:
            assert pos[("deliver", i)] < pos[("issue", i + W)]
        if W > 1 and i + W - 1 < n:
            assert pos[("issue", i + W - 1)] < pos[("deliver", i)]
    assert threading.active_count() == before
    assert threading.current_thread().name not in r.worker_threads
    assert len(r.worker_threads) <= _coder.default_threads()


def test_window_larger_than_the_clip_and_empty_frames():
    r = Recorder()
    P.run_ordered(3, 8, r.issue, r.deliver)
    assert r.delivered == [0, 1, 2] and r.max_in_flight == 3
    r = Recorder(jobs_per_frame=0)
    P.run_ordered(2, 4, r.issue, r.deliver)
    assert r.delivered == [0, 1]
    P.run_ordered(0, 4, r.issue, r.deliver)
    assert r.delivered == [0, 1]


def test_pending_run_from_two_threads_works_once():
    """result() on one thread while another is inside run(): the work is done once and both get its outcome."""
    from compressai.entropy_models.entropy_models import _Pending

    calls, release = [], threading.Event()

    class Slow(_Pending):
        def _work(self):
            calls.append(threading.current_thread().name)
            release.wait(10)
            return "done"

    p = Slow()
    got = []
    t = threading.Thread(target=lambda: got.append(p.run()))
    t.start()
    while not calls:
        time.sleep(0.001)
    threading.Timer(0.02, release.set).start()
    assert p.result() == "done"          # waits for the worker instead of starting the work again
    t.join(10)
    assert got == ["done"] and len(calls) == 1


def test_encode_video_checks_the_window_before_it_creates_the_file(tmp_path):
    from compressai.utils.codec_rgbt import encode_video

    out = tmp_path / "never.bin"
    with pytest.raises(ValueError, match="frames_in_flight"):
        encode_video(str(tmp_path / "clip_16x16_30Hz_8bit_P420.yuv"), None, str(out), frames_in_flight=0)
    assert not out.exists()


def test_pipeline_high_water_and_misuse():
    with P.FramePipeline(2) as pipe:
        pipe.submit(0, "a", [lambda: 1])
        pipe.submit(1, "b", [lambda: 2, lambda: 3])
        assert pipe.full() and len(pipe) == 2
        with pytest.raises(RuntimeError, match="in flight"):
            pipe.submit(2, "c", [])
        assert pipe.take() == (0, "a", [1])
        assert pipe.take() == (1, "b", [2, 3])
        assert pipe.high_water == 2
    with pytest.raises(RuntimeError, match="not open"):
        P.FramePipeline(2).submit(0, None, [])


def test_pool_is_bounded_by_the_coders_threads(monkeypatch):
    assert P.pool_threads(1000) == _coder.default_threads() <= 16
    assert P.pool_threads(1) == min(4, _coder.default_threads())
    assert P.pool_threads(8, threads=10 ** 6) == _coder.default_threads()
    monkeypatch.setattr(_coder.os, "cpu_count", lambda: 512)
    assert P.pool_threads(1000) == 16
    assert P.FramePipeline(64).threads == 16


@pytest.mark.parametrize("W", [2, 4, 8])
def test_a_failing_job_surfaces_at_its_frame(W):
    n, k = 12, 5
    before = threading.active_count()
    r = Recorder(fail_at=k, seed=7)
    with pytest.raises(OSError, match=f"frame {k} failed"):
        P.run_ordered(n, W, r.issue, r.deliver)
    assert r.delivered == list(range(k))                 # nothing of frame k or later
    assert max(r.issued) <= k + W - 1
    assert threading.active_count() == before            # drained and joined before the exception got here


def test_an_exception_of_the_caller_drains_the_pool():
    before = threading.active_count()
    r = Recorder(fail_in_issue=6)
    with pytest.raises(KeyError, match="issue 6"):
        P.run_ordered(10, 4, r.issue, r.deliver)
    assert r.delivered == [0, 1, 2]                      # 3, 4, 5 were in flight and are dropped
    assert threading.active_count() == before

    class Stop(BaseException):                           # what KeyboardInterrupt is: not an Exception
        pass

    def deliver(i, payload, results):
        if i == 2:
            raise Stop()
        r2.deliver(i, payload, results)

    r2 = Recorder()
    with pytest.raises(Stop):
        P.run_ordered(10, 4, r2.issue, deliver)
    assert r2.delivered == [0, 1]
    assert threading.active_count() == before


@pytest.mark.parametrize("bad", [0, -1, 2.0, None, True])
def test_frames_in_flight_below_one_is_a_value_error(bad):
    with pytest.raises(ValueError, match="frames_in_flight"):
        P.run_ordered(3, bad, lambda i: (None, []), lambda *a: None)
    with pytest.raises(ValueError, match="frames_in_flight"):
        P.FramePipeline(bad)
    with pytest.raises(ValueError, match="frames_in_flight"):
        P.StagingRing(bad)


def test_frame_loops_refuse_a_bad_window_before_any_work():
    """encode_frames / decode_frames / the model check the window first: no file is touched, no GPU is needed."""
    import torch

    from compressai.models.video import ScaleSpaceFlow
    from compressai.utils.video.eval_model.__main__ import decode_frames, encode_frames

    net = ScaleSpaceFlow()

    class Seq:
        bitdepth, height, width = 8, 128, 128

    class NoFile:
        def write(self, *_):
            raise AssertionError("written before the check")
        read = write

    with pytest.raises(ValueError, match="frames_in_flight"):
        encode_frames(net, Seq(), NoFile(), 2, frames_in_flight=0)
    with pytest.raises(ValueError, match="frames_in_flight"):
        decode_frames(net, NoFile(), 128, 128, 2, lambda *a: None, frames_in_flight=0)
    with pytest.raises(ValueError, match="frames_in_flight"):
        net.compress([torch.zeros(1, 3, 128, 128)], frames_in_flight=0)
    with pytest.raises(ValueError, match="frames_in_flight"):
        net.decompress([[]], [[]], frames_in_flight=-2)


# ---------------------------------------------------------------------------------------------------------
# the host coder from several threads
# ---------------------------------------------------------------------------------------------------------
def _tables(rng, ncdf=6):
    width = 40
    lengths = rng.integers(2, width - 2, size=ncdf).astype(np.int32)
    pmf = np.zeros((ncdf, width), dtype=np.float32)
    for r, n in enumerate(lengths):
        q = rng.random(n).astype(np.float32) + 1e-3
        q[-1] = 1e-6                                     # the tail-mass slot
        pmf[r, :n] = q / q.sum()
    cdf = _coder.pmf_to_quantized_cdf_rows(pmf, lengths, 16, width + 2)
    offsets = -rng.integers(0, lengths - 1).astype(np.int32)
    return _coder.Tables(cdf, lengths + 1, offsets)


def test_host_coder_from_eight_threads_matches_the_serial_calls():
    try:
        lib = _coder.lib.load()
    except RuntimeError:
        pytest.skip("libcai_coder.so not built")
    rng = np.random.default_rng(2020)
    tables = _tables(rng)
    cases = []
    for t in range(8):
        n = int(rng.integers(2000, 20000))
        sym = rng.integers(-12, 12, size=n).astype(np.int32)
        sym[rng.random(n) < 0.01] = 1 << 20              # long bypass escapes
        sym[rng.random(n) < 0.01] = -(1 << 20)
        sym[rng.random(n) < 0.02] = 37                   # short ones, just outside the tables
        idx = rng.integers(0, tables.cdfs.shape[0], size=n).astype(np.int32)
        cases.append((sym, idx))
    assert any((np.abs(s) > 1000).any() for s, _ in cases)

    def encode(sym, idx):
        cap = int(lib.cai_rans_max_bytes(sym.size))
        out = np.empty(cap, dtype=np.uint8)
        nbytes = np.zeros(1, dtype=np.int64)
        rc = lib.cai_rans_encode(_coder._ptr(sym), _coder._ptr(idx), sym.size, tables.ref(), _coder._ptr(out), cap,
                                 _coder._ptr(nbytes))
        assert rc == _coder.CAI_OK
        return out[:int(nbytes[0])].tobytes()

    def decode(data, idx):
        buf = np.frombuffer(data, dtype=np.uint8)
        out = np.empty(idx.size, dtype=np.int32)
        rc = lib.cai_rans_decode(_coder._ptr(buf), len(data), _coder._ptr(idx), idx.size, tables.ref(), _coder._ptr(out))
        assert rc == _coder.CAI_OK
        return out

    serial = [encode(s, i) for s, i in cases]
    for data, (s, i) in zip(serial, cases):
        assert np.array_equal(decode(data, i), s)

    start = threading.Barrier(len(cases))
    got, errors = [None] * len(cases), []

    def work(k):
        try:
            start.wait(timeout=30)
            for _ in range(3):
                data = encode(*cases[k])
                back = decode(data, cases[k][1])
            got[k] = (data, back)
        except BaseException as e:       # noqa: BLE001 - reported below, on the main thread
            errors.append((k, e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(cases))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors, errors
    for k, (data, back) in enumerate(got):
        assert data == serial[k], f"thread {k}: bytes differ from the serial call"
        assert np.array_equal(back, cases[k][0]), f"thread {k}: symbols differ"


def test_pending_strings_run_on_a_worker_thread_without_a_device():
    """PendingStrings / PendingSymbols with no event: the jobs the pool runs, here on host arrays only."""
    import torch

    from compressai.entropy_models.entropy_models import PendingStrings, PendingSymbols

    try:
        _coder.lib.load()
    except RuntimeError:
        pytest.skip("libcai_coder.so not built")
    rng = np.random.default_rng(7)
    tables = _tables(rng)
    B, n = 2, 5000
    sym = torch.from_numpy(rng.integers(-9, 9, size=(B, n)).astype(np.int32))
    idx = torch.from_numpy(rng.integers(0, tables.cdfs.shape[0], size=(B, n)).astype(np.int32))
    want = _coder.encode_streams(sym.numpy(), idx.numpy(), tables, B)
    pend = [PendingStrings(sym, idx, None, tables, B) for _ in range(4)]
    outs = [torch.empty((B, n), dtype=torch.int32) for _ in range(4)]

    def issue(i):
        return pend[i], [pend[i].run]

    strings = []
    P.run_ordered(4, 4, issue, lambda i, p, res: strings.append((p.result(), res[0])))
    assert all(a == want and b == want for a, b in strings)
    dec = [PendingSymbols(want, idx, outs[i], None, tables, lambda host: host.clone()) for i in range(4)]
    got = []
    P.run_ordered(4, 2, lambda i: (dec[i], [dec[i].run]), lambda i, p, res: got.append(p.finish()))
    assert all(torch.equal(g, sym) for g in got)
    bad = PendingSymbols([want[0][:8], want[1]], idx, outs[0], None, tables, lambda host: host)
    with pytest.raises(ValueError, match="truncated or corrupt stream|shorter than"):
        P.run_ordered(1, 2, lambda i: (bad, [bad.run]), lambda i, p, res: None)
    with pytest.raises(ValueError, match="truncated or corrupt stream|shorter than"):
        bad.result()                                     # kept: the same error again, not a second decode


# ---------------------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------------------
def test_parsers_accept_frames_in_flight_and_default_to_one():
    from compressai.utils import codec_rgbt
    from compressai.utils.video.eval_model.__main__ import create_parser

    common = ["--model", "ssf2020", "--path", "x.pth", "-o", "out"]
    for parser in (codec_rgbt.encode_parser(), codec_rgbt.decode_parser()):
        assert parser.parse_args(["in"] + common).frames_in_flight == 1
        assert parser.parse_args(["in"] + common + ["--frames-in-flight", "4"]).frames_in_flight == 4
    ev = create_parser()
    base = ["checkpoint", "data", "out", "-a", "ssf2020", "-p", "x.pth"]
    assert ev.parse_args(base).frames_in_flight == 1
    assert ev.parse_args(base + ["--frames-in-flight", "8"]).frames_in_flight == 8
    with pytest.raises(SystemExit):
        ev.parse_args(base + ["--frames-in-flight", "many"])
