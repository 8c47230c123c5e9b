"""Frames in flight: a bounded, ordered window of frames whose host-coder jobs run on worker threads.

The bitstream of this package is one serial rANS state per string, so a string cannot be coded in parallel without
changing its bytes.  What can overlap is the coding of *different* frames with each other and with the device work of
the frames after them: the encoder knows ``y_hat`` / ``z_hat`` on the device as soon as a latent is quantised, and
the decoder's entropy parameters depend on a frame's own ``z`` strings only.  ``FramePipeline`` is that overlap:

* ``submit(tag, payload, jobs)`` hands the jobs of one frame (zero-argument callables) to the pool and returns at
  once; ``take()`` blocks on the *oldest* frame in flight and returns ``(tag, payload, [job results])``.  Results
  therefore leave strictly in frame order, and never more than ``frames_in_flight`` frames are between the two calls.
* The pool has at most ``_coder.default_threads()`` threads (never sized by ``os.cpu_count()`` alone), started as
  jobs arrive.  A job waits for a device event and calls the host coder through ``ctypes`` (which releases the GIL);
  it issues no launch, allocation or tensor operation -- only the thread that owns the pipeline touches torch.
* An exception of a job is re-raised by the ``take()`` of its frame.  Leaving the ``with`` block -- normally, by
  that exception, by ``KeyboardInterrupt`` or by an exception of the caller's own code -- cancels what has not
  started, waits for what has, and joins every thread before the exception propagates: nothing of a later frame is
  delivered.

``run_ordered`` is the loop both frame loops use; ``StagingRing`` holds the pinned host buffers, one slot per
frame in flight, reused.  This module imports torch only when a staging buffer is allocated, so the scheduler can
be tested without a GPU.
"""
from __future__ import annotations

from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Callable, Deque, Dict, List, Optional, Sequence, Tuple

from ... import _coder

__all__ = ["FramePipeline", "StagingRing", "StagingSlot", "check_frames_in_flight", "run_ordered"]


def check_frames_in_flight(frames_in_flight) -> int:
    if isinstance(frames_in_flight, bool) or not isinstance(frames_in_flight, int) or frames_in_flight < 1:
        raise ValueError(f"frames_in_flight must be an integer >= 1, got {frames_in_flight!r}")
    return frames_in_flight


def pool_threads(frames_in_flight: int, threads: Optional[int] = None) -> int:
    """Worker threads of a window of ``frames_in_flight`` frames: a frame has at most four strings to code, and the
    pool never exceeds the host coder's own bound."""
    cap = _coder.default_threads()
    want = 4 * frames_in_flight if threads is None else int(threads)
    return max(1, min(cap, want))


class FramePipeline:
    """See the module docstring.  Use as a context manager."""

    def __init__(self, frames_in_flight: int = 1, threads: Optional[int] = None):
        self.frames_in_flight = check_frames_in_flight(frames_in_flight)
        self.threads = pool_threads(self.frames_in_flight, threads)
        self.high_water = 0                 # most frames ever in flight (tests read it)
        self._window: Deque[Tuple[Any, Any, list]] = deque()
        self._pool: Optional[ThreadPoolExecutor] = None

    def __enter__(self) -> "FramePipeline":
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="cai-coder")
        return self

    def __exit__(self, exc_type, exc, tb) -> bool:
        self.close()
        return False

    def close(self) -> None:
        """Cancel the jobs that have not started, wait for the running ones, join the threads."""
        pool, self._pool = self._pool, None
        self._window.clear()
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)

    def __len__(self) -> int:
        return len(self._window)

    def full(self) -> bool:
        return len(self._window) >= self.frames_in_flight

    def submit(self, tag, payload, jobs: Sequence[Callable[[], Any]]) -> None:
        if self._pool is None:
            raise RuntimeError("FramePipeline is not open (use it as a context manager)")
        if self.full():
            raise RuntimeError(f"{self.frames_in_flight} frames are in flight already: take() the oldest first")
        self._window.append((tag, payload, [self._pool.submit(job) for job in jobs]))
        self.high_water = max(self.high_water, len(self._window))

    def take(self) -> Tuple[Any, Any, List[Any]]:
        """(tag, payload, job results) of the oldest frame in flight; re-raises the first exception of its jobs."""
        tag, payload, futures = self._window.popleft()
        return tag, payload, [f.result() for f in futures]


def run_ordered(num_frames: int, frames_in_flight: int, issue: Callable[[int], Tuple[Any, Sequence[Callable]]],
                deliver: Callable[[int, Any, List[Any]], None], threads: Optional[int] = None) -> None:
    """``issue(i) -> (payload, jobs)`` for i = 0 .. num_frames - 1 in order, each followed -- at most
    ``frames_in_flight`` frames later -- by ``deliver(i, payload, results)``, also in order.  Both run on the
    calling thread; only the jobs run on the pool.  The calling thread blocks on the oldest frame alone."""
    with FramePipeline(frames_in_flight, threads) as pipe:
        for i in range(num_frames):
            if pipe.full():
                deliver(*pipe.take())
            payload, jobs = issue(i)
            pipe.submit(i, payload, jobs)
        while len(pipe):
            deliver(*pipe.take())


class StagingSlot:
    """The pinned host buffers of one frame in flight, by name; a buffer is kept and reused while it is large enough.
    ``busy`` is the device event after which the slot's buffers are no longer read by a copy (set by the decoder's
    second half); ``wait_free()`` is called before the slot's next frame writes them."""

    def __init__(self):
        self._buffers: Dict[Any, Any] = {}
        self.busy = None

    def buffer(self, key, numel: int):
        """A pinned int32 host tensor of ``numel`` elements (main thread only)."""
        import torch

        buf = self._buffers.get(key)
        if buf is None or buf.numel() < numel:
            buf = self._buffers[key] = torch.empty(max(1, numel), dtype=torch.int32, pin_memory=True)
        return buf[:numel]

    def wait_free(self) -> None:
        busy, self.busy = self.busy, None
        if busy is not None:
            busy.synchronize()


class StagingRing:
    """``frames_in_flight`` staging slots; frame i uses slot i % frames_in_flight, which the window guarantees was
    delivered before frame i is issued."""

    def __init__(self, frames_in_flight: int):
        self.slots = [StagingSlot() for _ in range(check_frames_in_flight(frames_in_flight))]

    def slot(self, i: int) -> StagingSlot:
        s = self.slots[i % len(self.slots)]
        s.wait_free()
        return s
