"""CPU: the pinned hand-over of the two-process multi-stream pipeline without a GPU - ``handover.FrameRing`` across processes,
``StagedRaggedImages.pack(out=)`` and ``FusionPipeline(handover="pinned")`` with stand-ins for the device halves.  Without a
CUDA device ``FrameRing.register()`` does nothing, everything else - the ring, the free-slot queue, the binding of a payload to
the consumer's mapping, the teardown - is what runs on the GPU box.  The sources check that the producer stays host-only."""
import multiprocessing as mp
import pickle
import time
from collections import Counter
from multiprocessing import shared_memory

import numpy as np
import pytest
import torch

from millieye_amd import hip
from millieye_amd.demo import FrameFuser, MultiStreamFuser, prepare_streams
from millieye_amd.handover import FrameRing
from millieye_amd.pipeline import QUEUE_SIZE, FusionPipeline, ProducerError
from millieye_amd.utils.datasets import StagedRaggedImages
from tests import multistream_helpers as mh, pixel_format_refs as pf
from tests.golden.make_golden import RADAR_CALIB
from tests.handover_helpers import BIG_SHAPE, OversizeSource, VaryingSource, pattern, write_pattern
from tests.multistream_pipeline_helpers import (BrokenStreamSource, KilledStreamSource, StreamSource, progress_counter,
                                                wait_for_backlog)

S = 4
SMALL_TOTAL = 2 * 24 * 32 * 3 + 2 * 30 * 20 * 3     # the bytes of a step of S small frames
SENTINEL = 0xA5


def _fuser():
    return MultiStreamFuser(None, RADAR_CALIB, S, model_mode=0, min_hits=2)


def _gone(name):
    with pytest.raises(FileNotFoundError):
        shared_memory.SharedMemory(name=name)
    return True


# ------------------------------------------------------------------------------------------------------------ FrameRing
def test_frame_ring_across_processes():
    ring = FrameRing(3, 5000)
    name = ring.name
    try:
        assert ring.owner and ring.slot_bytes == 8192 and ring.handle == (name, 3, 8192)
        blob = pickle.dumps(ring)
        assert len(blob) < 1024
        for i in range(3):
            view = ring.slot(i)
            assert view.dtype == torch.uint8 and tuple(view.shape) == (8192,) and view.data_ptr() == ring.slot(0).data_ptr() + i * 8192
            view.fill_(i)
        k = 1
        child = mp.get_context("spawn").Process(target=write_pattern, args=(ring, k, 11))
        child.start()
        child.join(60)
        assert child.exitcode == 0
        assert torch.equal(ring.slot(k), pattern(8192, 11))
        assert bool((ring.slot(0) == 0).all()) and bool((ring.slot(2) == 2).all())
        ring.register()                      # no device here: nothing; on a GPU box: the real thing
        assert ring.registered == torch.cuda.is_available()
        del view
    finally:
        ring.close()
        ring.close()
    assert ring.closed and not ring.registered and _gone(name)
    with pytest.raises(hip.MeError, match="closed"):
        ring.slot(0)


def test_frame_ring_attach_and_refusals():
    ring = FrameRing(2, 4096)
    try:
        other = pickle.loads(pickle.dumps(ring))
        assert not other.owner and other.handle == ring.handle
        other.slot(1)[:4] = torch.tensor([1, 2, 3, 4], dtype=torch.uint8)
        assert ring.slot(1)[:4].tolist() == [1, 2, 3, 4]
        with pytest.raises(hip.MeError, match="only the process that created"):
            other.register()
        with pytest.raises(hip.MeError, match="slot 2 of 2"):
            ring.slot(2)
        other.close()
        assert ring.slot(1)[:4].tolist() == [1, 2, 3, 4]      # the attached side leaving changes nothing for the owner
    finally:
        ring.close()
    assert _gone(ring.name)
    with pytest.raises(ValueError):
        FrameRing(0, 4096)


# ------------------------------------------------------------------------------------------------------------ pack(out=)
_FMTS = ["nv12", "bgr", "yuyv", "rgb"]
_HW = [(24, 32), (30, 20), (12, 38), (7, 9)]
_FLIPS = [0, 1, 1, 0]


def _staged(kind):
    if kind == "default":
        frames = [torch.from_numpy(pf.native_frame("rgb", h, w, seed=900 + i)) for i, (h, w) in enumerate(_HW)]
        return StagedRaggedImages(frames, 16, _FLIPS)
    frames = [torch.from_numpy(pf.native_frame(f, h, w, seed=910 + i)) for i, (f, (h, w)) in enumerate(zip(_FMTS, _HW))]
    if kind == "formats":
        return StagedRaggedImages(frames, 16, _FLIPS, formats=_FMTS)
    if kind == "area":
        return StagedRaggedImages(frames, 16, _FLIPS, formats=_FMTS, resize="area")
    return StagedRaggedImages(frames, (32, 64), _FLIPS, formats=_FMTS)


@pytest.mark.parametrize("kind", ["default", "formats", "area", "rect"])
def test_pack_into_out_gives_the_bytes_and_descriptor_of_pack(kind):
    want = _staged(kind).pack()
    total = int(want.packed.numel())
    out = torch.full((total + 100,), SENTINEL, dtype=torch.uint8)
    got = _staged(kind).pack(out=out, keep_frames=False)
    assert got.packed.dtype == torch.uint8 and torch.equal(got.packed, want.packed) and torch.equal(got.desc, want.desc)
    assert got.desc.shape[1] == (4 if kind == "default" else 5) and got.frames == []
    assert got.packed.data_ptr() == out.data_ptr() and int(got.packed.numel()) == total, "packed is out[:total]"
    assert bool((out[total:] == SENTINEL).all()), "bytes behind total were touched"
    exact = torch.full((total,), SENTINEL, dtype=torch.uint8)
    assert torch.equal(_staged(kind).pack(out=exact).packed, want.packed)
    # an object that does not lie in a ring pickles with its bytes, as ever
    back = pickle.loads(pickle.dumps(got))
    assert torch.equal(back.packed, want.packed) and back.ring_slot is None


@pytest.mark.parametrize("kind", ["default", "formats", "area", "rect"])
def test_pack_into_an_out_one_byte_too_small(kind):
    total = int(_staged(kind).pack().packed.numel())
    out = torch.full((total - 1,), SENTINEL, dtype=torch.uint8)
    staged = _staged(kind)
    with pytest.raises(hip.MeError, match=rf"{total} bytes.*{total - 1}"):
        staged.pack(out=out)
    assert bool((out == SENTINEL).all()) and staged.packed is None
    with pytest.raises(hip.MeError, match="1-D contiguous uint8"):
        staged.pack(out=torch.zeros((total,), dtype=torch.int8))
    with pytest.raises(hip.MeError, match="out= needs pack=True"):
        prepare_streams([np.zeros((4, 4, 3), np.uint8)], [[]], 1, out=torch.zeros(64, dtype=torch.uint8))


def test_a_staged_object_in_a_ring_pickles_without_its_bytes():
    ring = FrameRing(2, 4 * 480 * 640 * 3)
    try:
        frames = [pf.native_frame("rgb", 480, 640, seed=920 + s) for s in range(S)]
        radar = [mh.stream_radar(s, 0) for s in range(S)]
        payload = prepare_streams(frames, radar, S, pack=True, out=ring.slot(1))
        plain = prepare_streams(frames, radar, S, pack=True)
        assert len(pickle.dumps(plain)) > 4 * 480 * 640 * 3
        payload["img"].lend_to_ring(1)
        payload["frame_idx"] = 5
        blob = pickle.dumps(payload)
        assert len(blob) < 16 * 1024, len(blob)
        back = pickle.loads(blob)
        img = back["img"]
        assert img.packed is None and img.ring_slot == 1 and img.ring_total == 4 * 480 * 640 * 3
        with pytest.raises(hip.MeError, match="bind"):
            img.to("cuda")
        img.bind(ring)
        assert img.packed.data_ptr() == ring.slot(1).data_ptr()
        assert torch.equal(img.packed, plain["img"].packed) and torch.equal(img.desc, plain["img"].desc)
        img.unbind()
        assert img.packed is None
        payload["img"].unbind()
        with pytest.raises(hip.MeError, match="do not lie in a ring"):
            plain["img"].bind(ring)
    finally:
        ring.close()
    assert _gone(ring.name)


# -------------------------------------------------------------------------------------------------------------- pipeline
def _checking_infer(source, seen, sleep_s=0.02, progress=None):
    """A stand-in for ``infer`` that compares the bound payload with a local ``prepare_streams`` of the same step."""
    def infer(payload):
        f = payload["frame_idx"]
        want = prepare_streams(*source.step(f), streams=S, pack=True)
        img = payload["img"]
        assert torch.equal(img.packed, want["img"].packed), f"step {f}: the packed bytes are not this step's"
        assert torch.equal(img.desc, want["img"].desc) and payload["hw"] == want["hw"] and img.frames == []
        seen.append((f, img.ring_slot, len(pickle.dumps(img))))
        if progress is not None:
            wait_for_backlog(progress, f)
        time.sleep(sleep_s)          # the producer runs ahead and has to wait for a slot
        return f
    return infer


def test_every_slot_is_reused_and_every_step_carries_its_own_bytes():
    ring_slots = 2
    n = 3 * ring_slots + 1
    source, seen = VaryingSource(n, S), []
    assert not np.array_equal(source.step(0)[0][0], source.step(1)[0][0])
    pipe = FusionPipeline(_fuser(), source, infer=_checking_infer(source, seen), advance=lambda p: None,
                          skip_to_newest=False, handover="pinned", ring_slots=ring_slots, slot_bytes=SMALL_TOTAL)
    assert pipe.handover == "pinned"
    got = list(pipe)
    assert [r for r, _i in got] == [i["frame_idx"] for _r, i in got] == list(range(n)) == [f for f, _s, _b in seen]
    used = Counter(slot for _f, slot, _b in seen)
    assert set(used) == set(range(ring_slots)) and min(used.values()) >= 3, used
    assert all(nbytes < 4096 for _f, _s, nbytes in seen), "a ring step's staged object pickles without its bytes"
    assert pipe.stats["handover"] == "pinned" and pipe.stats["ring_slots"] == ring_slots
    assert pipe.stats["slot_bytes"] == 12288 and pipe.stats["handover_fallback"] == 0
    assert pipe.stats["frames"] == n and pipe.stats["dropped"] == 0
    assert _gone(pipe.ring_name)


def test_skipping_to_the_newest_loses_no_slot():
    ring_slots = 3
    n = 3 * ring_slots + 1
    progress = progress_counter()
    source, seen, advanced = VaryingSource(n, S, progress=progress), [], []
    calls = []

    def advance(payload):
        want = prepare_streams(*source.step(payload["frame_idx"]), streams=S, pack=True)
        assert torch.equal(payload["img"].packed, want["img"].packed)
        calls.append(("advance", payload["frame_idx"]))

    check = _checking_infer(source, seen, sleep_s=0.0, progress=progress)

    def infer(payload):
        calls.append(("infer", payload["frame_idx"]))
        return check(payload)

    pipe = FusionPipeline(_fuser(), source, infer=infer, advance=advance, handover="pinned", ring_slots=ring_slots,
                          slot_bytes=SMALL_TOTAL)
    got, t0 = [], time.perf_counter()
    for r, info in pipe:
        got.append((r, info))
        assert time.perf_counter() - t0 < 60, "the pipeline stalls: a slot was lost"
    assert [idx for _w, idx in calls] == list(range(n)), "advance + infer see every step exactly once, in order"
    inferred = [f for f, _s, _b in seen]
    assert inferred[0] == 0 and inferred[-1] == n - 1 and len(inferred) < n
    assert [i for _r, info in got for i in info["skipped"]] == [idx for w, idx in calls if w == "advance"]
    assert pipe.stats["dropped"] == n - len(inferred) and pipe.stats["handover_fallback"] == 0
    assert _gone(pipe.ring_name)


def test_step_zero_sizes_the_ring_when_slot_bytes_is_none():
    ring_slots = 2
    n = 3 * ring_slots + 1
    source, seen = VaryingSource(n, S), []
    pipe = FusionPipeline(_fuser(), source, infer=_checking_infer(source, seen, sleep_s=0.0), advance=lambda p: None,
                          skip_to_newest=False, handover="pinned", ring_slots=ring_slots)
    assert [r for r, _i in pipe] == list(range(n))
    assert seen[0][1] is None and seen[0][2] > SMALL_TOTAL, "step 0 travels through the queue, bytes and all"
    assert all(slot is not None and nbytes < 4096 for _f, slot, nbytes in seen[1:])
    want = SMALL_TOTAL + SMALL_TOTAL // 4
    assert pipe.stats["slot_bytes"] == -(-want // 4096) * 4096 and pipe.stats["handover_fallback"] == 0
    assert _gone(pipe.ring_name)


def test_a_step_that_does_not_fit_a_slot_travels_through_the_queue():
    n, big_at = 6, 3
    source, seen = OversizeSource(n, S, big_at), []
    assert BIG_SHAPE[0] * BIG_SHAPE[1] * 3 > 12288
    pipe = FusionPipeline(_fuser(), source, infer=_checking_infer(source, seen, sleep_s=0.0), advance=lambda p: None,
                          skip_to_newest=False, handover="pinned", ring_slots=2, slot_bytes=SMALL_TOTAL)
    assert [r for r, _i in pipe] == list(range(n))
    assert [slot is None for _f, slot, _b in seen] == [f == big_at for f in range(n)]
    assert seen[big_at][2] > BIG_SHAPE[0] * BIG_SHAPE[1] * 3
    assert pipe.stats["handover_fallback"] == 1 and pipe.stats["frames"] == n
    assert _gone(pipe.ring_name)


def _pinned(source, infer, **kw):
    return FusionPipeline(_fuser(), source, infer=infer, advance=lambda p: None, skip_to_newest=False, handover="pinned",
                          ring_slots=2, slot_bytes=SMALL_TOTAL, **kw)


def _failing(payload):
    if payload["frame_idx"] == 2:
        raise ZeroDivisionError("infer failed")
    return payload["frame_idx"]


@pytest.mark.parametrize("ending", ["broken source", "killed producer", "early break", "infer raises"])
def test_endings_leave_no_segment_behind(ending):
    got = []
    if ending == "broken source":
        pipe = _pinned(BrokenStreamSource(), lambda p: p["frame_idx"])
        with pytest.raises(ProducerError, match="camera unplugged"):
            list(pipe)
    elif ending == "killed producer":
        pipe = _pinned(KilledStreamSource(5, S), lambda p: p["frame_idx"])
        with pytest.raises(ProducerError, match="exit code 7"):
            for r, _info in pipe:
                got.append(r)
        assert got == [0, 1]
    elif ending == "early break":
        pipe = _pinned(VaryingSource(50, S), lambda p: p["frame_idx"])
        for r, _info in pipe:      # (the loop drops the generator at the break: its finally runs there)
            got.append(r)
            if r == 2:
                break
        assert got == [0, 1, 2] and pipe.stats["frames"] == 3
    else:
        pipe = _pinned(VaryingSource(50, S), _failing)
        with pytest.raises(ZeroDivisionError):
            for r, _info in pipe:
                got.append(r)
        assert got == [0, 1] and pipe.stats["frames"] == 2
    assert pipe.ring_name is not None and _gone(pipe.ring_name)
    assert pipe.stats["handover"] == "pinned" and pipe.stats["slot_bytes"] == 12288


def test_refusals_and_the_default():
    fuser = _fuser()
    with pytest.raises(ValueError, match="unknown handover"):
        FusionPipeline(fuser, StreamSource(1, S), handover="mapped")
    with pytest.raises(ValueError, match="multi-stream"):
        FusionPipeline(FrameFuser(None, RADAR_CALIB, model_mode=0), StreamSource(1, 1), handover="pinned")
    for bad in (1, 0):
        with pytest.raises(ValueError, match="ring_slots"):
            FusionPipeline(fuser, StreamSource(1, S), handover="pinned", ring_slots=bad)
    with pytest.raises(ValueError, match="need handover"):
        FusionPipeline(fuser, StreamSource(1, S), ring_slots=3)
    assert FusionPipeline(fuser, StreamSource(1, S), handover="pinned").ring_slots == QUEUE_SIZE + 2
    pipe = FusionPipeline(fuser, StreamSource(2, S), infer=lambda p: p, advance=lambda p: None, skip_to_newest=False)
    assert pipe.handover is None and pipe.ring_slots is None and pipe.slot_bytes is None
    got = [p for p, _i in pipe]
    assert set(pipe.stats) == {"dropped", "frames", "seconds"}
    for payload in got:
        assert type(payload) is dict and set(payload) == {"hw", "img", "radar_frames", "frame_idx"}
        img = payload["img"]
        assert type(img) is StagedRaggedImages and img.ring_slot is None
        assert set(img.__getstate__()) == {"frames", "size", "flips", "shape", "dtype", "rect", "resize", "packed", "desc"}
        assert isinstance(img.packed, torch.Tensor) and int(img.packed.numel()) == SMALL_TOTAL
