"""Picklable pieces of the hand-over tests (tests/test_handover_cpu.py, tests/test_gpu_handover.py): what runs inside a
spawned process has to be importable there."""
import numpy as np

from tests.multistream_pipeline_helpers import StreamSource, _producer_is_host_only, small_frame

BIG_SHAPE = (80, 80)   # (h, w) of the one frame of OversizeSource that no small slot holds


def varying_frame(s, f):
    """Stream ``s``'s small frame with other bytes at every step ``f`` (every byte moves by ``37 f + 1`` mod 256)."""
    return (small_frame(s).astype(np.int64) + 37 * f + 1).astype(np.uint8)


class VaryingSource(StreamSource):
    """``StreamSource`` whose small frames differ from step to step: a slot that is overwritten too early, or read after it
    was given to another step, shows as other bytes."""

    def step(self, f):
        from tests import multistream_helpers as mh
        return [varying_frame(s, f) for s in range(self.streams)], [mh.stream_radar(s, f) for s in range(self.streams)]


class OversizeSource(VaryingSource):
    """``VaryingSource`` whose step ``big_at`` carries one ``BIG_SHAPE`` frame in stream 0."""

    def __init__(self, n, streams, big_at, progress=None):
        super().__init__(n, streams, progress=progress)
        self.big_at = big_at

    def step(self, f):
        frames, radar = super().step(f)
        if f == self.big_at:
            h, w = BIG_SHAPE
            frames[0] = ((np.arange(h * w * 3, dtype=np.int64) * 7 + f) % 251).astype(np.uint8).reshape(h, w, 3)
        return frames, radar


def write_pattern(ring, k, seed):
    """Child of the ``FrameRing`` test: ``ring`` arrived here through pickle, so it is attached, not owned."""
    import torch
    _producer_is_host_only()
    assert not ring.owner and not ring.registered
    ring.slot(k).copy_(pattern(ring.slot_bytes, seed))
    assert not torch.cuda.is_initialized()
    ring.close()
    ring.close()


def pattern(nbytes, seed):
    import torch
    return ((torch.arange(nbytes, dtype=torch.int64) * 131 + seed) % 253).to(torch.uint8)
