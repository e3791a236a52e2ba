"""The device ranging kernel (csrc/box_ranges.hip: me_box_ranges_f64; detection_range.DeviceDetectionRanges, hip.box_ranges,
hip.stream_tail_ranges, MultiStreamFuser(ranging=)) against its specification detection_range.range_detections: every
comparison is bit-equal (NaN payloads apart).  The synthetic cases build the network rows, the cloud slots and the radar
counts themselves; the largest deviation seen is printed (0 is the only value that passes)."""
import numpy as np
import pytest
import torch

from tests import box_tracks_refs as br
from tests import detection_range_refs as dr

pytestmark = pytest.mark.gpu

MARK = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _deviation(got, want):
    """Largest |got - want| over the places where both are numbers; inf where one is NaN and the other is not."""
    if got.shape != want.shape:
        return float("inf")
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    both = ~np.isnan(want)
    return float(np.abs(got[both] - want[both]).max()) if both.any() else 0.0


def _through_the_tail(scenes, params, what, tracker=None):
    """``scenes``: per stream ``(dets, cloud)``.  The rows go through ``hip.stream_tail_ranges`` (identity rescale, every row a
    class of its own: the second NMS keeps all) and every stream's ranges are compared with ``range_detections`` on the rows
    the tail returned.  Returns the whole result."""
    from millieye_amd import hip
    from millieye_amd.detection_range import DeviceDetectionRanges, range_detections
    S = len(scenes)
    rows = _dev(dr.network_rows([d for d, _c in scenes]))
    slots, words = dr.radar_buffers([c for _d, c in scenes])
    ranger = DeviceDetectionRanges(S, **params)
    out = hip.stream_tail_ranges(rows, S, _dev(dr.identity_scalars(S)), 0.3, ranger, _dev(slots), _dev(words), tracker=tracker)
    per_stream, ranges, status = out[0], out[-2], out[-1]
    assert status == [hip.RANGES_OK] * S and ranger.host_status.tolist() == status
    worst = 0.0
    for s, (dets, cloud) in enumerate(scenes):
        kept = per_stream[s].numpy()
        assert len(kept) == len(dets), f"{what} stream {s}: the tail kept {len(kept)} of {len(dets)} rows"
        want = range_detections(kept, cloud, **params)
        worst = max(worst, _deviation(ranges[s], want))
        assert dr.same(ranges[s], want), f"{what} stream {s}:\n{ranges[s]}\nvs\n{want}"
    print(f"{what}: largest deviation {worst:.3e}")
    return out


@pytest.mark.parametrize("name", sorted(dr.edge_scenes()))
def test_edge_scenes(hip_lib, name):
    dets, cloud, params = dr.edge_scenes()[name]
    out = _through_the_tail([(dets, cloud)], params, name)
    if name == "nan_coordinate":
        assert np.isnan(out[0][0].numpy()[:, 0]).sum() == 1, "the NaN row must come through the tail"
    if name == "all_256_inside":
        assert out[-2][0][0, 3] == 256


def test_no_rows_at_all(hip_lib):
    out = _through_the_tail([(dr.dets_of([]), dr.cloud_of([(1, 2, 3.0, 0.5)]))], {}, "m = 0")
    assert out[-2][0].shape == (0, 4)


def test_empty_stream_in_the_middle_and_a_stream_without_points(hip_lib):
    a, c = dr.random_scene(0), dr.random_scene(1)
    scenes = [(a[0], a[1]), (dr.dets_of([]), a[1]), (c[0], dr.cloud_of([])), (c[0], c[1])]
    out = _through_the_tail(scenes, {}, "S = 4")
    assert out[-2][1].shape == (0, 4) and np.isnan(out[-2][2][:, 0]).all() and (out[-2][2][:, 3] == 0).all()
    assert (out[-2][0][:, 2] > 0).any() and (out[-2][3][:, 2] > 0).any()


def _crowd(k, seed, points=256):
    """``k`` boxes on a grid over a cloud of ``points`` returns: every box holds some."""
    rng = np.random.default_rng(seed)
    boxes = [(20 + 45 * (i % 13), 20 + 44 * (i // 13), 20 + 45 * (i % 13) + rng.uniform(30, 80), 20 + 44 * (i // 13) + rng.uniform(40, 90))
             for i in range(k)]
    cloud = np.stack([rng.uniform(0, 640, points), rng.uniform(0, 480, points), np.round(rng.uniform(1.0, 9.0, points), 2),
                      rng.normal(0, 1, points)], 1)
    return dr.dets_of(boxes), dr.cloud_of(cloud)


def test_130_detections_in_one_stream(hip_lib):
    """More rows than one workgroup has waves, more than the tracker's 64, beside a small stream."""
    dets, cloud = _crowd(130, 5)
    small = dr.random_scene(2)
    out = _through_the_tail([(dets, cloud), (small[0], small[1])], dict(gate=0.6), "130 detections")
    ranged = int((out[-2][0][:, 2] > 0).sum())
    assert 20 < ranged and (out[-2][0][:, 2] == 0).any()


def test_256_points_random_boxes(hip_lib):
    dets, cloud = _crowd(40, 6)
    _through_the_tail([(dets, cloud)], dict(shrink=1.0, gate=2.5, min_points=3), "256 points")


@pytest.mark.parametrize("seeds", [dr.RANDOM_SEEDS[:6], dr.RANDOM_SEEDS[6:]])
def test_random_scenes(hip_lib, seeds):
    scenes = [dr.random_scene(seed)[:2] for seed in seeds]
    out = _through_the_tail(scenes, {}, f"random scenes {seeds[0]} - {seeds[-1]}")
    assert all((r[:, 2] > 0).any() and (r[:, 2] == 0).any() for r in out[-2])


def test_300_streams(hip_lib):
    scenes = []
    for s in range(300):
        dets, cloud, _p = dr.random_scene(100 + s % 7)
        scenes.append((dets[:1 + s % 3], cloud[:(s * 37) % 257]))
    out = _through_the_tail(scenes, {}, "S = 300")
    assert sum(int((r[:, 2] > 0).sum()) for r in out[-2]) > 100


def _bare(per_stream, clouds, gaps=None, flag=0, counts=None, **params):
    """``hip.box_ranges`` on a hand-built tail buffer and marker-filled outputs; returns (ranges [m,4], status, m)."""
    from millieye_amd import hip
    buf, m = br.tail_buffer(per_stream, gaps, flag)
    slots, words = dr.radar_buffers(clouds, counts)
    ranges = torch.full((m, 4), float(MARK), dtype=torch.float64, device="cuda")
    status = torch.full((len(per_stream),), MARK, dtype=torch.int32, device="cuda")
    hip.box_ranges(_dev(buf), m, len(per_stream), _dev(slots), _dev(words), ranges, status, **params)
    return ranges.cpu().numpy(), status.cpu().tolist(), m


def _three_streams():
    scenes = [dr.random_scene(seed) for seed in (3, 4, 5)]
    return [d for d, _c, _p in scenes], [c for _d, c, _p in scenes]


def test_only_kept_rows_are_written(hip_lib):
    from millieye_amd.detection_range import range_detections
    dets, clouds = _three_streams()
    gaps = [2, 0, 3]
    got, status, m = _bare(dets, clouds, gaps)
    assert status == [0, 0, 0] and m == sum(len(d) for d in dets) + 5
    start = 0
    for s in range(3):
        k = len(dets[s])
        assert dr.same(got[start:start + k], range_detections(dets[s], clouds[s])), f"stream {s}"
        assert (got[start + k:start + k + gaps[s]] == MARK).all(), f"stream {s}: wrote a row the tail did not keep"
        start += k + gaps[s]
    assert start == m


def test_flagged_and_inconsistent_tails(hip_lib):
    from millieye_amd import hip
    dets, clouds = _three_streams()
    got, status, _m = _bare(dets, clouds, flag=1)
    assert status == [hip.RANGES_E_INPUT] * 3 and (got == MARK).all()
    # the rows of the streams add up to more than m
    buf, m = br.tail_buffer(dets)
    slots, words = dr.radar_buffers(clouds)
    ranges = torch.full((m, 4), float(MARK), dtype=torch.float64, device="cuda")
    status = torch.full((3,), MARK, dtype=torch.int32, device="cuda")
    hip.box_ranges(_dev(buf), m - 1, 3, _dev(slots), _dev(words), ranges[:m - 1], status)
    assert status.cpu().tolist() == [hip.RANGES_E_INPUT] * 3 and (ranges.cpu().numpy() == MARK).all()
    # more kept rows than rows in one stream
    ints = buf[:32].view(np.int32)   # (8 head words for 3 streams)
    ints[1 + 3 + 1] = ints[1 + 1] + 1
    hip.box_ranges(_dev(buf), m, 3, _dev(slots), _dev(words), ranges, status)
    assert status.cpu().tolist() == [hip.RANGES_E_INPUT] * 3 and (ranges.cpu().numpy() == MARK).all()


@pytest.mark.parametrize("count", [257, -1])
def test_a_point_count_out_of_range_in_one_stream(hip_lib, count):
    from millieye_amd import hip
    from millieye_amd.detection_range import range_detections
    dets, clouds = _three_streams()
    got, status, _m = _bare(dets, clouds, gaps=[1, 1, 1], counts=[len(clouds[0]), count, len(clouds[2])])
    assert status == [hip.RANGES_OK, hip.RANGES_E_POINTS, hip.RANGES_OK]
    start = 0
    for s in range(3):
        k = len(dets[s])
        if s == 1:
            assert (got[start:start + k + 1] == MARK).all()
        else:
            assert dr.same(got[start:start + k], range_detections(dets[s], clouds[s])) and (got[start + k] == MARK).all()
        start += k + 1


def test_with_and_without_ranging_and_tracking(hip_lib):
    """The rows with and without ranging are torch.equal; with a tracker as well, the tracks, the rows and the ranges equal
    what each gives alone."""
    from millieye_amd import hip
    from millieye_amd.detection_tracks import DeviceDetectionTracks
    S = 3
    walks = [br.scene(40 + s, steps=8, people=3 + s) for s in range(S)]
    steps = [[walks[s][f] for s in range(S)] for f in range(3)]
    clouds = [dr.random_scene(8 + s)[1] for s in range(S)]
    scal = _dev(dr.identity_scalars(S))
    alone, both = DeviceDetectionTracks(S, min_hits=1), DeviceDetectionTracks(S, min_hits=1)
    total = 0
    for f in range(3):
        scenes = [(steps[f][s], clouds[s]) for s in range(S)]
        rows = _dev(dr.network_rows([steps[f][s] for s in range(S)]))
        plain = hip.stream_tail(rows, S, scal, 0.3)
        tracked = hip.stream_tail_tracks(rows, S, scal, 0.3, alone)
        # (people of one class overlap: the second NMS may drop rows here, unlike in the scenes above)
        slots, words = dr.radar_buffers(clouds)
        from millieye_amd.detection_range import DeviceDetectionRanges, range_detections
        ranger = DeviceDetectionRanges(S)
        ranged = hip.stream_tail_ranges(rows, S, scal, 0.3, ranger, _dev(slots), _dev(words))
        everything = hip.stream_tail_ranges(rows, S, scal, 0.3, ranger, _dev(slots), _dev(words), tracker=both)
        assert len(plain) == 2 and len(tracked) == 4 and len(ranged) == 4 and len(everything) == 6
        assert plain[1] == tracked[1] == ranged[1] == everything[1]
        assert tracked[3] == everything[3] == [0] * S and ranged[3] == everything[5] == [0] * S
        for s in range(S):
            assert torch.equal(plain[0][s], ranged[0][s]) and torch.equal(plain[0][s], everything[0][s]), f"step {f} stream {s}"
            assert torch.equal(plain[0][s], tracked[0][s])
            assert np.array_equal(tracked[2][s], everything[2][s]), f"step {f} stream {s}: tracks differ with ranging"
            want = range_detections(plain[0][s].numpy(), scenes[s][1])
            assert dr.same(ranged[2][s], want) and dr.same(everything[4][s], want), f"step {f} stream {s}"
            total += len(want)
    assert total > 10 and int(both.host_counts[:, 2].sum()) > 0


def test_binding_refuses_bad_tensors(hip_lib):
    from millieye_amd import hip
    from millieye_amd.detection_range import DeviceDetectionRanges
    dets, clouds = _three_streams()
    buf, m = br.tail_buffer(dets)
    slots, words = dr.radar_buffers(clouds)
    ranges = torch.zeros((m, 4), dtype=torch.float64, device="cuda")
    status = torch.zeros((3,), dtype=torch.int32, device="cuda")
    with pytest.raises(hip.MeError):
        hip.box_ranges(_dev(buf)[:-8], m, 3, _dev(slots), _dev(words), ranges, status)
    with pytest.raises(hip.MeError):
        hip.box_ranges(_dev(buf), m, 3, _dev(slots)[:2], _dev(words), ranges, status)
    with pytest.raises(hip.MeError):
        hip.box_ranges(_dev(buf), m, 3, _dev(slots), _dev(words), ranges.float(), status)
    with pytest.raises(hip.MeError):
        hip.box_ranges(_dev(buf), m, 3, _dev(slots), _dev(words), ranges, status, min_points=0)
    with pytest.raises(hip.MeError):
        DeviceDetectionRanges(3, gate=float("nan"))
    with pytest.raises(hip.MeError):
        hip.stream_tail_ranges(_dev(dr.network_rows(dets)), 3, _dev(dr.identity_scalars(3)), 0.3, DeviceDetectionRanges(2),
                               _dev(slots), _dev(words))
    got, st = DeviceDetectionRanges(3).step(_dev(buf), m, _dev(slots), _dev(words))
    assert st == [0, 0, 0] and got.shape == (m, 4) and not np.isnan(got[:, 3]).any()


# ------------------------------------------------------------------------------------------------------------- the fusers
def _fuser_inputs(S):
    from tests import multistream_helpers as mh
    return mh, [mh.stream_frame(s) for s in range(S)]


def _check_info(fuser, got, what):
    """Every stream's ``info["ranges"]`` against the specification on the returned rows and the device cloud."""
    from millieye_amd.detection_range import range_detections
    rows_total = ranged = 0
    for s, (rows, info) in enumerate(got):
        want = range_detections(rows.numpy(), fuser.generator.cloud(s), **fuser.range_params)
        assert info["range_status"] == 0 and dr.same(info["ranges"], want), f"{what} stream {s}"
        assert len(info["ranges"]) == len(rows)
        rows_total += len(rows)
        ranged += int((want[:, 2] > 0).sum())
    return rows_total, ranged


def test_fuser_ranges_and_tracks(hip_lib):
    from millieye_amd import hip
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    from tests.golden.make_golden import RADAR_CALIB
    from tests.test_gpu_multistream import _net
    net = _net()
    S = 2
    mh, frames = _fuser_inputs(S)
    kw = dict(model_mode=3, min_hits=mh.MIN_HITS)
    track_params = dict(min_hits=1, iou_min=0.2)
    plain = MultiStreamFuser(net, RADAR_CALIB, S, **kw)
    both = MultiStreamFuser(net, RADAR_CALIB, S, tracks=track_params, ranging=True, **kw)
    single = FrameFuser(net, RADAR_CALIB, ranging=True, **kw)
    assert plain.ranger is None
    rows_total = ranged = tracks_total = 0
    for f in range(3):
        radar = [mh.stream_radar(s, f) for s in range(S)]
        want, got = plain(frames, radar), both(frames, radar)
        for s in range(S):
            assert torch.equal(got[s][0], want[s][0]), f"step {f} stream {s}: rows differ with ranging"
            assert set(got[s][1]) == set(want[s][1]) | {"tracks", "track_status", "ranges", "range_status", "track_ranges"}
            info = got[s][1]
            det = info["tracks"][:, 9].astype(np.int64)
            assert info["track_ranges"].shape == (len(det), 4) and info["track_ranges"].dtype == np.float64
            for t, k in enumerate(det):
                expect = info["ranges"][k] if k >= 0 else np.array([np.nan, np.nan, 0.0, 0.0])
                assert np.array_equal(info["track_ranges"][t], expect, equal_nan=True), f"step {f} stream {s} track {t}"
            tracks_total += len(det)
        a, b = _check_info(both, got, f"step {f}")
        rows_total, ranged = rows_total + a, ranged + b
        if f == 0:   # the host fuser on stream 0's inputs: the same rows (up to the order of ties), the same ranges
            rows_h, info_h = single(frames[0], radar[0])
            assert info_h["range_status"] == 0 and info_h["ranges"].shape == (len(rows_h), 4)
            rows_d, ranges_d = got[0][0].numpy(), got[0][1]["ranges"]
            assert len(rows_h) == len(rows_d)
            order_h, order_d = np.lexsort(rows_h.numpy().T[::-1]), np.lexsort(rows_d.T[::-1])
            assert dr.same(info_h["ranges"][order_h], ranges_d[order_d]), "FrameFuser(ranging=True) vs stream 0"
    print(f"fuser: {rows_total} detections, {ranged} with a range, {tracks_total} track rows")
    assert rows_total > 0 and tracks_total > 0 and ranged > 0
    with pytest.raises(hip.MeError):
        MultiStreamFuser(net, RADAR_CALIB, S, tail="host", ranging=True)


def test_fuser_ranges_on_a_rectangular_canvas(hip_lib):
    from millieye_amd.demo import MultiStreamFuser
    from tests.golden.make_golden import RADAR_CALIB
    from tests.test_gpu_multistream import _net
    net = _net()
    S = 2
    mh, frames = _fuser_inputs(S)
    kw = dict(model_mode=3, min_hits=mh.MIN_HITS, img_size=(64, 96))
    plain = MultiStreamFuser(net, RADAR_CALIB, S, **kw)
    ranged = MultiStreamFuser(net, RADAR_CALIB, S, ranging=dict(shrink=1.0, gate=0.5), **kw)
    radar = [mh.stream_radar(s, 0) for s in range(S)]
    want, got = plain(frames, radar), ranged(frames, radar)
    for s in range(S):
        assert torch.equal(got[s][0], want[s][0]) and "track_ranges" not in got[s][1]
    rows_total, with_range = _check_info(ranged, got, "rectangular")
    print(f"rectangular fuser: {rows_total} detections, {with_range} with a range")
    assert rows_total > 0 and with_range > 0
