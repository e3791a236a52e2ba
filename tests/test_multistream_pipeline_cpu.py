"""CPU: the two-process pipeline for S streams (millieye_amd/pipeline.py with a ``demo.MultiStreamFuser``): the real producer
and the real consumer loop, with stand-ins for the device halves ``infer`` / ``advance``.  The fuser builds its device
generator on first use, so none of this touches a GPU; the sources check that the producer never loads the HIP library."""

import pytest
import torch

from millieye_amd.demo import MultiStreamFuser, prepare_streams
from millieye_amd.pipeline import FusionPipeline, ProducerError
from tests.golden.make_golden import RADAR_CALIB
from tests.multistream_pipeline_helpers import (BrokenStreamSource, KilledStreamSource, StreamSource, progress_counter,
                                                wait_for_backlog)

S = 4


def _fuser():
    return MultiStreamFuser(None, RADAR_CALIB, S, model_mode=0, min_hits=2)


def _echo(payload):
    return payload


def test_every_step_in_order_and_the_payload_is_the_host_half():
    n = 6
    fuser = _fuser()
    advanced = []
    pipe = FusionPipeline(fuser, StreamSource(n, S), infer=_echo, advance=advanced.append, skip_to_newest=False)
    got = list(pipe)
    assert [info["frame_idx"] for _p, info in got] == list(range(n)) and all(info["skipped"] == [] for _p, info in got)
    assert advanced == [] and pipe.stats["dropped"] == 0 and pipe.stats["frames"] == n
    source = StreamSource(n, S)
    for f, (payload, _info) in enumerate(got):
        frames, radar = source.step(f)
        want = fuser.prepare(frames, radar, pack=True)
        assert payload["hw"] == want["hw"] == [tuple(fr.shape[:2]) for fr in frames]
        img, img_w = payload["img"], want["img"]
        assert img.packed.dtype == torch.uint8 and torch.equal(img.packed, img_w.packed), f"step {f}: packed bytes"
        assert torch.equal(img.desc, img_w.desc) and tuple(img.shape) == tuple(img_w.shape) == (S, 3, 416, 416)
        assert img.frames == [] and len(img) == S
        # the packed bytes are the frames, one after the other, at the descriptor's offsets
        for s, fr in enumerate(frames):
            off, h, w, flip = (int(v) for v in img.desc[s])
            assert (h, w, flip) == (fr.shape[0], fr.shape[1], 0)
            assert torch.equal(img.packed[off:off + h * w * 3], torch.from_numpy(fr).reshape(-1))
        assert len(payload["radar_frames"]) == S
        for a, b in zip(payload["radar_frames"], want["radar_frames"]):
            assert len(a) == len(b) and all((x == y).all() for x, y in zip(a, b))
    # the unpacked host half of MultiStreamFuser.prepare carries the same frames
    frames, radar = source.step(0)
    plain = fuser.prepare(frames, radar)
    assert plain["img"].packed is None and len(plain["img"].frames) == S
    assert torch.equal(plain["img"].pack().packed, got[0][0]["img"].packed)


def test_a_slow_consumer_skips_to_the_newest_and_the_trackers_see_every_step():
    n = 30
    calls = []
    progress = progress_counter()

    def infer(payload):
        calls.append(("infer", payload["frame_idx"]))
        wait_for_backlog(progress, payload["frame_idx"])   # "slow": until the producer has queued the next two steps
        return payload["frame_idx"]

    def advance(payload):
        calls.append(("advance", payload["frame_idx"]))

    pipe = FusionPipeline(_fuser(), StreamSource(n, S, progress=progress), infer=infer, advance=advance)
    got = list(pipe)
    seen = [info["frame_idx"] for _r, info in got]
    assert [r for r, _i in got] == seen
    assert seen[0] == 0 and all(a < b for a, b in zip(seen, seen[1:])) and seen[-1] == n - 1
    assert [idx for _what, idx in calls] == list(range(n)), "advance + infer see every step exactly once, in order"
    assert [idx for what, idx in calls if what == "infer"] == seen
    skipped = [idx for what, idx in calls if what == "advance"]
    assert [i for _r, info in got for i in info["skipped"]] == skipped
    assert pipe.stats["dropped"] == len(skipped) == n - len(seen) and pipe.stats["frames"] == len(seen)
    assert len(seen) < n, "a consumer that finds two more steps queued after every inference must skip"


def test_source_failure_raises_producer_error():
    with pytest.raises(ProducerError) as err:
        list(FusionPipeline(_fuser(), BrokenStreamSource(), infer=_echo, advance=_echo))
    assert "camera unplugged" in str(err.value)


def test_a_producer_killed_hard_raises_instead_of_hanging():
    pipe = FusionPipeline(_fuser(), KilledStreamSource(5, S), infer=lambda p: p["frame_idx"], advance=_echo, skip_to_newest=False)
    got = []
    with pytest.raises(ProducerError) as err:
        for r, _info in pipe:
            got.append(r)
    assert "exit code 7" in str(err.value), str(err.value)
    assert got == [0, 1]


def test_a_wrong_stream_count_is_reported():
    pipe = FusionPipeline(_fuser(), StreamSource(5, S, short_at=2), infer=lambda p: p["frame_idx"], advance=_echo,
                          skip_to_newest=False)
    got = []
    with pytest.raises(ProducerError) as err:
        for r, _info in pipe:
            got.append(r)
    assert f"{S - 1} frames" in str(err.value) and f"{S} streams" in str(err.value)
    assert got == [0, 1]
    with pytest.raises(Exception, match="streams"):
        prepare_streams([], [], S)


def test_frame_fuser_pipelines_are_untouched():
    """A FrameFuser still takes the single-stream path (no ``streams`` / ``advance``)."""
    from millieye_amd.demo import FrameFuser
    pipe = FusionPipeline(FrameFuser(None, RADAR_CALIB, model_mode=0), StreamSource(1, 1), infer=_echo)
    assert not pipe.multi
