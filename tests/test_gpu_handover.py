"""-m gpu: the pinned hand-over on the device - ``handover.FrameRing`` registered with the HIP runtime and uploaded from,
staged objects bound to a ring slot against the same objects on their own buffers (``torch.equal``), and the whole two-process
pipeline with ``handover="pinned"`` against the in-process ``MultiStreamFuser`` on the same steps."""
import pickle
from multiprocessing import shared_memory

import pytest
import torch

from millieye_amd.handover import FrameRing
from tests import multistream_helpers as mh, pixel_format_refs as pf
from tests.golden.make_golden import RADAR_CALIB
from tests.multistream_pipeline_helpers import StreamSource
from tests.test_gpu_area_resize import _net, _same_step

pytestmark = pytest.mark.gpu


def _gone(name):
    with pytest.raises(FileNotFoundError):
        shared_memory.SharedMemory(name=name)
    return True


def test_register_and_upload(hip_lib):
    ring = FrameRing(3, 10000)
    try:
        assert ring.register() == 0 and ring.registered and ring.register_status == 0
        assert ring.register() is None and ring.registered          # twice: nothing
        for i in range(3):
            ring.slot(i).copy_(((torch.arange(ring.slot_bytes) * (7 + i) + i) % 251).to(torch.uint8))
        slot = ring.slot(1)
        assert slot.is_pinned(), "torch does not see the registered mapping as pinned"
        on_device = slot.to("cuda", non_blocking=True)
        part = ring.slot(2)[5:9001].to("cuda", non_blocking=True)      # an odd offset inside a slot
        torch.cuda.synchronize()
        assert torch.equal(on_device.cpu(), slot) and torch.equal(part.cpu(), ring.slot(2)[5:9001])
        assert ring.unregister() == 0 and not ring.registered
        assert ring.unregister() is None
        assert ring.register() == 0                                   # and again, after an unregister
        del slot
    finally:
        ring.close()
        ring.close()
    assert not ring.registered and _gone(ring.name)


_FMTS = ["nv12", "bgr", "yuyv", "rgb"]
_HW = [(32, 48), (40, 36), (30, 44), (7, 9)]
_FLIPS = [0, 1, 0, 1]


def _staged(kind):
    from millieye_amd.utils.datasets import StagedRaggedImages
    if kind == "default":
        frames = [torch.from_numpy(pf.native_frame("rgb", h, w, seed=930 + i)) for i, (h, w) in enumerate(_HW)]
        return StagedRaggedImages(frames, 16, _FLIPS)
    frames = [torch.from_numpy(pf.native_frame(f, h, w, seed=940 + i)) for i, (f, (h, w)) in enumerate(zip(_FMTS, _HW))]
    if kind == "formats":
        return StagedRaggedImages(frames, 16, _FLIPS, formats=_FMTS)
    if kind == "area":
        return StagedRaggedImages(frames, 16, _FLIPS, formats=_FMTS, resize="area")
    return StagedRaggedImages(frames, (64, 96), _FLIPS, formats=_FMTS)


@pytest.mark.parametrize("kind", ["default", "formats", "area", "rect"])
def test_a_staged_object_bound_to_a_slot_gives_the_unbound_tensor(hip_lib, kind):
    want = _staged(kind).pack().to("cuda")
    side = (64, 96) if kind == "rect" else (16, 16)
    assert want.is_cuda and tuple(want.shape) == (4, 3) + side and float(want.abs().sum()) > 0
    ring = FrameRing(2, 16384)
    try:
        ring.register()
        ring.slot(0).fill_(255)
        ring.slot(1).fill_(255)
        staged = _staged(kind).pack(keep_frames=False, out=ring.slot(1)).lend_to_ring(1)
        arrived = pickle.loads(pickle.dumps(staged))          # what the consumer gets: no bytes
        assert arrived.packed is None and arrived.frames == []
        arrived.bind(ring)
        got = arrived.to("cuda")
        torch.cuda.synchronize()
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
        arrived.unbind()
        staged.unbind()
    finally:
        ring.close()
    assert _gone(ring.name)


def _local_steps(net, n, steps):
    from millieye_amd.demo import MultiStreamFuser
    fuser = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS)
    source = StreamSource(steps, n, real=True)
    return [fuser(*source.step(f)) for f in range(steps)]


_runs = {}


def _whole_pipeline():
    """The one full run of this file (shared: a run costs the producer's start-up)."""
    if "first" not in _runs:
        from millieye_amd.demo import MultiStreamFuser
        from millieye_amd.pipeline import QUEUE_SIZE, FusionPipeline
        n = 3
        fuser = MultiStreamFuser(_net(), RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS)
        ring_slots = FusionPipeline(fuser, StreamSource(1, n, real=True), handover="pinned").ring_slots
        assert ring_slots == QUEUE_SIZE + 2
        steps = 2 * ring_slots + 1
        pipe = FusionPipeline(fuser, StreamSource(steps, n, real=True), handover="pinned", skip_to_newest=False)
        _runs["first"] = (pipe, list(pipe), steps)
    return _runs["first"]


def test_the_pinned_pipeline_gives_the_in_process_rows(hip_lib):
    n = 3
    pipe, got, steps = _whole_pipeline()
    assert [info["frame_idx"] for _r, info in got] == list(range(steps))
    want = _local_steps(_net(), n, steps)
    for f, (results, _info) in enumerate(got):
        _same_step(results, want[f], f"step {f}")
    assert sum(len(rows) for results, _i in got for rows, _info in results) > 0
    total = sum(mh.stream_frame(s).size for s in range(n))
    slot_bytes = -(-(total + total // 4) // 4096) * 4096
    assert pipe.stats["handover"] == "pinned" and pipe.stats["slot_bytes"] == slot_bytes
    assert pipe.stats["handover_fallback"] == 0 and pipe.stats["frames"] == steps and _gone(pipe.ring_name)


def test_a_second_pipeline_in_the_same_process(hip_lib):
    from millieye_amd.demo import MultiStreamFuser
    from millieye_amd.pipeline import FusionPipeline
    first, _got, _steps = _whole_pipeline()
    assert _gone(first.ring_name)
    net = _net()
    n, steps = 3, 3
    total = sum(mh.stream_frame(s).size for s in range(n))
    want = _local_steps(net, n, steps)
    fuser = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS)
    pipe = FusionPipeline(fuser, StreamSource(steps, n, real=True), handover="pinned", skip_to_newest=False, ring_slots=2,
                          slot_bytes=total)
    got = list(pipe)
    assert len(got) == steps
    for f, (results, _info) in enumerate(got):
        _same_step(results, want[f], f"step {f}")
    assert pipe.stats["handover_fallback"] == 0 and pipe.stats["slot_bytes"] == -(-total // 4096) * 4096
    assert pipe.ring_name != first.ring_name and _gone(pipe.ring_name)
