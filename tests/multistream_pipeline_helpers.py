"""Picklable sources for the multi-stream pipeline tests (the producer runs under the ``spawn`` start method).  Every source
checks, before it hands out a step, that its process - the producer - has neither loaded the HIP library nor initialised the
GPU: the failed check travels to the consumer as a ``ProducerError``."""
import numpy as np

SMALL_SHAPES = ((24, 32), (30, 20))   # (h, w): landscape and portrait, small enough to keep the queue's shared memory tiny


def _producer_is_host_only():
    import sys
    import torch
    from millieye_amd import hip
    assert hip._lib is None, "the producer loaded the HIP library"
    assert not torch.cuda.is_initialized(), "the producer initialised the GPU"
    assert "millieye_amd.my_models" not in sys.modules, "the producer imported the model code"


def small_frame(s):
    from millieye_amd import synth
    h, w = SMALL_SHAPES[s % 2]
    return (synth.uniform(f"multipipe/frame{s}", (h, w, 3)) * 255).astype(np.uint8)


class StreamSource:
    """``n`` steps of ``streams`` frames + radar lists: small frames of two shapes (``real=False``) or the frames of
    tests/multistream_helpers (``real=True``), with that module's radar streams.  ``short_at``: that step lacks one stream.
    ``progress``: a shared counter (:func:`progress_counter`) that holds the number of steps handed out so far - step ``f``
    is handed out only after step ``f - 1`` was queued - and a value past every step once the source is exhausted."""

    def __init__(self, n, streams, real=False, short_at=None, progress=None):
        self.n, self.streams, self.real, self.short_at, self.progress = n, streams, real, short_at, progress
        self._frames = None

    def step(self, f):
        from tests import multistream_helpers as mh
        k = self.streams - 1 if f == self.short_at else self.streams
        if self._frames is None:   # the same frames every step
            self._frames = [mh.stream_frame(s) if self.real else small_frame(s) for s in range(self.streams)]
        return self._frames[:k], [mh.stream_radar(s, f) for s in range(k)]

    def __call__(self):
        for f in range(self.n):
            _producer_is_host_only()
            if self.progress is not None:
                self.progress.value = f + 1
            yield self.step(f)
        _producer_is_host_only()
        if self.progress is not None:
            self.progress.value = self.n + 100


def progress_counter():
    import multiprocessing as mp
    return mp.get_context("spawn").Value("i", 0)


def wait_for_backlog(progress, idx, limit=10.0):
    """Called by a consumer stand-in while it holds step ``idx`` > 0: returns once the producer has queued the next two steps
    (it has handed out step ``idx + 3``) or is done - so that the consumer's next look at the queue finds steps to skip
    without the test relying on who is faster.  (Step 0 is the rendezvous: the producer waits for the consumer there.)"""
    import time
    t0 = time.perf_counter()
    while idx > 0 and progress.value < idx + 4:
        assert time.perf_counter() - t0 < limit, \
            f"the producer queued no two further steps within {limit} s of step {idx} (it handed out {progress.value} steps)"
        time.sleep(0.001)
    time.sleep(0.005)   # the queue's feeder thread hands the queued payloads to the pipe


class BrokenStreamSource:
    def __call__(self):
        raise RuntimeError("camera unplugged")


class KilledStreamSource(StreamSource):
    """Two steps, then the producer dies without an exception and without the END payload."""

    def __call__(self):
        import os
        import time
        for f in range(2):
            yield self.step(f)
        time.sleep(0.3)   # let the queue's feeder thread flush what was queued
        os._exit(7)
