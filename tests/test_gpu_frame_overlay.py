"""The device overlay kernel (csrc/frame_overlay.hip: me_frame_overlay_u8; frame_overlay.DeviceFrameOverlay, hip.frame_overlay,
hip.stream_tail_overlay, MultiStreamFuser(overlay=)) against its specification frame_overlay.draw_detections.  The pictures of a
case lie in ONE poisoned buffer, pitched, at odd offsets; the whole buffer is compared, so every comparison is bit-equal on the
pictures AND on every byte around and between them.  The number of differing bytes is printed (0 is the only value that
passes)."""
import numpy as np
import pytest
import torch

from millieye_amd import frame_overlay as fo
from tests import box_tracks_refs as br
from tests import frame_overlay_refs as fr

pytestmark = pytest.mark.gpu

MARK = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _layout(pictures, seed=0):
    """``pictures``: ``(fmt, h, w)`` per stream -> (layout, poisoned buffer): odd offsets, odd row padding, NV12's chroma plane
    at a distance with a pitch of its own."""
    layout, end = [], 7
    for n, (fmt, h, w) in enumerate(pictures):
        end = fr.place(layout, fmt, h, w, offset=end | 1, pad=1 + 2 * (n % 3), uv_gap=5 + n % 4, uv_pad=3 + n % 2) + 3 + n % 5
    return layout, fr.poisoned(end + 9, seed)


def _paint(layout, buf, scenes, what, gaps=None, flag=0, track_status=None, range_status=None, **style):
    """One launch on the pictures of ``layout`` in ``buf`` with ``scenes[s] = (rows, tracks, ranges)``; returns
    (buffer after, status per stream)."""
    S = len(layout)
    tail, m = br.tail_buffer([sc[0] for sc in scenes], gaps, flag)
    d_buf = _dev(buf)
    surfaces = [fr.surface_on(d_buf, e) for e in layout]
    tracker = ranger = None
    if any(sc[1] is not None for sc in scenes):
        table, counts = fr.tracks_buffers([sc[1] for sc in scenes], track_status)
        tracker = (_dev(table), _dev(counts))
    if any(sc[2] is not None for sc in scenes):
        ranges = fr.ranges_buffer([sc[0] for sc in scenes], [sc[2] for sc in scenes], gaps)
        ranger = (_dev(ranges), None if range_status is None else _dev(np.asarray(range_status, np.int32)))
    painter = fo.DeviceFrameOverlay(S, **style)
    status = painter.draw(_dev(tail), m, surfaces, tracker=tracker, ranger=ranger)
    return d_buf.cpu().numpy(), status.cpu().tolist()


def _check(layout, buf, scenes, what, expect=None, **kw):
    """:func:`_paint` against ``draw_detections`` picture by picture, over the whole buffer."""
    style = {k: v for k, v in kw.items() if k in fo.DEFAULTS}
    got, status = _paint(layout, buf, scenes, what, **kw)
    want, want_status = fr.expected_buffer(buf, layout, scenes if expect is None else expect, **style)
    differing = int((got != want).sum())
    print(f"{what}: {len(layout)} pictures, {len(buf)} bytes, {int((want != buf).sum())} changed, {differing} differ")
    assert status == want_status, f"{what}: status {status} vs {want_status}"
    assert differing == 0, f"{what}: first differing byte {int(np.nonzero(got != want)[0][0])}"
    return got


@pytest.mark.parametrize("fmt", ["rgb", "bgr", "nv12", "yuyv"])
def test_formats_on_small_pitched_pictures(hip_lib, fmt):
    sizes = [(48, 64), (40, 36)] + ([(31, 45)] if fmt in ("rgb", "bgr") else [])
    layout, buf = _layout([(fmt, h, w) for h, w in sizes], seed=1)
    scenes = [fr.random_scene(10 + n, h, w) for n, (h, w) in enumerate(sizes)]
    got = _check(layout, buf, scenes, f"{fmt} small")
    assert (got != buf).sum() > 500


@pytest.mark.parametrize("streams", [1, 5, 33])
def test_mixed_streams_in_one_launch(hip_lib, streams):
    kinds = [("rgb", 31, 45), ("nv12", 40, 36), ("yuyv", 26, 52), ("bgr", 48, 64), ("nv12", 22, 30)]
    pictures = [kinds[s % len(kinds)] for s in range(streams)]
    layout, buf = _layout(pictures, seed=streams)
    scenes = []
    for s, (_fmt, h, w) in enumerate(pictures):
        k = 0 if s % 4 == 1 else 64 if s % 7 == 2 else None
        scenes.append(fr.random_scene(100 + s, h, w, k=k) if k != 0 else (fr.rows_of([]), None, None))
    if streams == 1:
        scenes = [fr.random_scene(100, 31, 45, k=64)]
    gaps = [s % 3 for s in range(streams)]
    _check(layout, buf, scenes, f"S = {streams}", gaps=gaps)


def test_heavily_overlapping_boxes_have_one_writer(hip_lib):
    """Forty boxes of ten colours around one spot, with labels: every pixel has many candidates and one owner."""
    h, w = 60, 90
    rng = np.random.default_rng(5)
    boxes = [(30 + rng.integers(-14, 15), 20 + rng.integers(-10, 11), 55 + rng.integers(-14, 15), 45 + rng.integers(-10, 11))
             for _ in range(40)]
    rows = fr.rows_of(boxes, cls=rng.integers(0, 10, 40))
    for fmt in ("rgb", "nv12"):
        layout, buf = _layout([(fmt, h, w)], seed=2)
        _check(layout, buf, [(rows, fr.tracks_of([(i + 1, i) for i in range(0, 40, 2)]), None)], f"overlap {fmt}", thickness=3)


@pytest.mark.parametrize("style", [dict(thickness=1, font_scale=1), dict(thickness=8, font_scale=4), dict(thickness=8, font_scale=1),
                                   dict(thickness=1, font_scale=4)])
def test_thickness_and_scale(hip_lib, style):
    pictures = [("rgb", 48, 64), ("nv12", 40, 36), ("yuyv", 31, 44)]
    layout, buf = _layout(pictures, seed=3)
    scenes = [fr.random_scene(20 + n, h, w, k=6) for n, (_f, h, w) in enumerate(pictures)]
    _check(layout, buf, scenes, f"style {style}", **style)


def test_edges_outside_and_non_finite_rows(hip_lib):
    h, w = 40, 36
    boxes = [(-5, 4, 7, 30), (28, 2, 50, 14), (4, -6, 15, 6), (5, 33, 16, 49), (-4, -4, 39, 43), (-30, 2, -12, 12), (40, 3, 60, 15),
             (3, -25, 14, -10), (3, 41, 14, 52), (0, 0, 35, 39), (10.5, 11.5, 12.5, 13.5), (20, 20, 20, 20), (25, 30, 22, 35),
             (3e9, 1, 4e9, 5), (-4e9, -4e9, 4e9, 4e9), (1e38, 2, 3, 4)]
    rows = fr.rows_of(boxes, cls=np.arange(len(boxes)) % 10)
    bad = fr.rows_of([(1, 1, 9, 9)] * 4, cls=[1, 2, np.nan, 3e9])
    bad[0, 1], bad[1, 2] = np.nan, -np.inf
    rows = np.concatenate([rows[:6], bad, rows[6:]], 0)
    for fmt in ("bgr", "nv12", "yuyv"):
        layout, buf = _layout([(fmt, h, w)], seed=4)
        _check(layout, buf, [(rows, None, None)], f"edges {fmt}")


def test_tracks_ranges_and_their_status_words(hip_lib):
    pictures = [("rgb", 48, 64), ("yuyv", 40, 36), ("nv12", 40, 36)]
    layout, buf = _layout(pictures, seed=6)
    scenes = []
    for n, (_f, h, w) in enumerate(pictures):
        rows, _t, _r = fr.random_scene(30 + n, h, w, k=8)
        tracks = fr.tracks_of([(41, 0), (7, -1), (123456, 3), (9, 3), (2147483647, 5), (-2, 6), (2.0 ** 31, 7), (3.7, 1)])
        ranges = fr.ranges_of([0.04, fr.NAN, 999.94, 999.95, np.inf, -0.04, 12.345, 60.0])
        scenes.append((rows, tracks, ranges))
    scenes[1] = (scenes[1][0], None, scenes[1][2])            # a stream without track rows
    _check(layout, buf, scenes, "tracks and ranges")
    _check(layout, buf, scenes, "colour by track", color_by="track")
    # a refused tracker step (status != 0) and a refused ranging stream have no ids / no ranges
    expect = [scenes[0], (scenes[1][0], None, None), (scenes[2][0], None, scenes[2][2])]
    _check(layout, buf, scenes, "status words", expect=expect, track_status=[0, 0, 3], range_status=[0, 2, 0])


def test_class_filter(hip_lib):
    layout, buf = _layout([("rgb", 48, 64), ("nv12", 40, 36)], seed=7)
    scenes = [fr.random_scene(40 + n, e["h"], e["w"], k=12) for n, e in enumerate(layout)]
    scenes[0][0][:3, 6] = [-1, -1.5, 13]
    got = _check(layout, buf, scenes, "classes", classes=[-1, 2, 3, 5, 13])
    assert (got != buf).any()
    _check(layout, buf, scenes, "no class listed", classes=[])
    _check(layout, buf, scenes, "no labels", labels=False, classes=[1, 4])


def test_a_crop_of_a_larger_device_picture(hip_lib):
    for fmt in ("rgb", "nv12", "yuyv"):
        layout, buf = _layout([(fmt, 60, 80)], seed=8)
        d_buf = _dev(buf)
        full = fr.surface_on(d_buf, layout[0])
        crop = full.crop(22, 14, 40, 30)
        rows, tracks, ranges = fr.random_scene(50, 30, 40, k=6)
        tail, m = br.tail_buffer([rows])
        table, counts = fr.tracks_buffers([tracks])
        status = fo.DeviceFrameOverlay(1).draw(_dev(tail), m, [crop], tracker=(_dev(table), _dev(counts)),
                                               ranger=(_dev(fr.ranges_buffer([rows], [ranges])), None))
        got = d_buf.cpu().numpy()
        # the expectation: the crop's pixels of the dense picture, drawn, put back
        e = dict(layout[0], h=30, w=40, offset=crop.offset, uv_offset=crop.uv_offset if fmt == "nv12" else None)
        want, want_status = fr.expected_buffer(buf, [e], [(rows, tracks, ranges)])
        print(f"crop {fmt}: {int((want != buf).sum())} changed, {int((got != want).sum())} differ")
        assert status.cpu().tolist() == want_status == [0] and np.array_equal(got, want) and not np.array_equal(got, buf)


def test_65_drawn_rows_leave_one_stream_untouched(hip_lib):
    pictures = [("rgb", 40, 40), ("nv12", 40, 40), ("yuyv", 40, 40)]
    layout, buf = _layout(pictures, seed=9)
    boxes = [(2 + i % 8 * 4, 2 + i // 8 * 3, 5 + i % 8 * 4, 4 + i // 8 * 3) for i in range(66)]
    many = fr.rows_of(boxes, cls=[1] * 64 + [2, 2])
    many[3, 0] = np.nan                                     # 65 drawn rows
    scenes = [fr.random_scene(60, 40, 40), (many, None, None), (many[:65], None, None)]   # 64 drawn rows in the last
    _after, status = _paint(layout, buf, scenes, "65 rows")
    assert status == [fo.OK, fo.E_BOXES, fo.OK]
    _check(layout, buf, scenes, "65 rows")
    got = _check(layout, buf, scenes, "65 rows, filtered", classes=[1])   # the filter comes before the count
    e = layout[1]
    assert not np.array_equal(fr.dense_of(got, e), fr.dense_of(buf, e))


def test_a_flagged_or_inconsistent_tail_draws_nothing(hip_lib):
    from millieye_amd import hip
    layout, buf = _layout([("rgb", 40, 36), ("nv12", 40, 36)], seed=10)
    scenes = [fr.random_scene(70 + n, 40, 36, k=5) for n in range(2)]
    got, status = _paint(layout, buf, scenes, "flagged", flag=1)
    assert status == [hip.OVERLAY_E_INPUT] * 2 and np.array_equal(got, buf)
    tail, m = br.tail_buffer([sc[0] for sc in scenes])
    d_buf = _dev(buf)
    surfaces = [fr.surface_on(d_buf, e) for e in layout]
    status = fo.DeviceFrameOverlay(2).draw(_dev(tail), m - 1, surfaces)          # the rows add up to more than m
    assert status.cpu().tolist() == [hip.OVERLAY_E_INPUT] * 2 and np.array_equal(d_buf.cpu().numpy(), buf)


def test_an_invalid_descriptor_is_refused_without_a_launch(hip_lib):
    from millieye_amd import hip
    layout, buf = _layout([("rgb", 40, 36), ("nv12", 40, 36), ("yuyv", 20, 36)], seed=11)
    scenes = [fr.random_scene(80 + n, e["h"], e["w"], k=5) for n, e in enumerate(layout)]
    tail, m = br.tail_buffer([sc[0] for sc in scenes])
    d_buf, d_tail = _dev(buf), _dev(tail)
    painter = fo.DeviceFrameOverlay(3)
    good = painter.descriptor([fr.surface_on(d_buf, e) for e in layout])
    status = torch.full((3,), MARK, dtype=torch.int32, device="cuda")
    broken = {"pitch below the row": (0, 7, 3 * 36 - 1), "last row beyond the buffer": (0, 1, layout[0]["offset"] + 40 * layout[0]["pitch"] - 2),
              "negative offset": (2, 2, -1), "odd nv12 width": (1, 4, 35), "unknown format": (2, 6, 4), "null base": (0, 0, 0),
              "chroma rows beyond the buffer": (1, 8, len(buf) - 36 * 2), "zero height": (2, 3, 0)}
    for name, (s, col, value) in broken.items():
        desc = good.clone()
        desc[s, col] = value
        with pytest.raises(hip.MeError):
            painter.draw(d_tail, m, desc, status=status.data_ptr())
        assert status.cpu().tolist() == [MARK] * 3, f"{name}: something was launched"
    assert np.array_equal(d_buf.cpu().numpy(), buf)
    # the device copy of the descriptor is checked again by the kernel: that stream alone is refused, nothing of it is written
    bad = good.clone()
    bad[1, 9] = 35
    hip.frame_overlay(d_tail, m, 3, bad.to("cuda"), good, painter.palette, painter.glyphs, status)
    want, _ = fr.expected_buffer(buf, [layout[0], layout[2]], [(scenes[0][0], None, None), (scenes[2][0], None, None)])
    assert status.cpu().tolist() == [hip.OVERLAY_OK, hip.OVERLAY_E_SURFACE, hip.OVERLAY_OK]
    assert np.array_equal(d_buf.cpu().numpy(), want)


def test_binding_refuses_bad_arguments(hip_lib):
    from millieye_amd import hip
    layout, buf = _layout([("rgb", 40, 36)], seed=12)
    rows = fr.random_scene(90, 40, 36, k=3)[0]
    tail, m = br.tail_buffer([rows])
    d_buf, d_tail = _dev(buf), _dev(tail)
    painter = fo.DeviceFrameOverlay(1)
    surface = fr.surface_on(d_buf, layout[0])
    with pytest.raises(hip.MeError):
        painter.draw(d_tail[:-8], m, [surface])
    with pytest.raises(hip.MeError):
        painter.draw(d_tail, m, [surface, surface])
    with pytest.raises(hip.MeError):
        painter.draw(d_tail, m, [fr.surface_on(torch.from_numpy(buf.copy()), layout[0])])      # a picture in host memory
    with pytest.raises(hip.MeError):
        painter.draw(d_tail, m, [surface], tracker=(torch.zeros((1, 64, 9), dtype=torch.float64, device="cuda"),
                                                    torch.zeros((1, 4), dtype=torch.int32, device="cuda")))
    with pytest.raises(hip.MeError):
        painter.draw(d_tail, m, [surface], ranger=(torch.zeros((m + 1, 4), dtype=torch.float64, device="cuda"), None))
    with pytest.raises(hip.MeError):
        fo.DeviceFrameOverlay(1, thickness=9)
    with pytest.raises(hip.MeError):
        fo.DeviceFrameOverlay(0)
    desc = painter.descriptor([surface])
    with pytest.raises(hip.MeError):
        hip.frame_overlay(d_tail, m, 1, desc.to("cuda"), desc, painter.palette, painter.glyphs,
                          torch.zeros((1,), dtype=torch.int32, device="cuda"), thickness=0)
    assert np.array_equal(d_buf.cpu().numpy(), buf)


# ------------------------------------------------------------------------------------------------------------- the fusers
def _fresh_surface(frame):
    """The frame in device memory as a decoder would leave it: pitched, at an odd offset."""
    h, w = frame.shape[:2]
    layout = []
    end = fr.place(layout, "rgb", h, w, offset=33, pad=7)
    host = fr.poisoned(end + 5, seed=h)
    fr.store(host, layout[0], frame)
    return fr.surface_on(_dev(host), layout[0]), host, layout[0]


def test_fuser_overlay_in_place_and_on_host_frames(hip_lib):
    from millieye_amd import hip
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    from tests import multistream_helpers as mh
    from tests.golden.make_golden import RADAR_CALIB
    from tests.test_gpu_multistream import _net
    net = _net()
    S = 2
    frames = [mh.stream_frame(s) for s in range(S)]
    kw = dict(model_mode=3, min_hits=mh.MIN_HITS, tracks=dict(min_hits=1, iou_min=0.2), ranging=True)
    style = dict(thickness=3, font_scale=2)
    plain = MultiStreamFuser(net, RADAR_CALIB, S, **kw)
    drawn = MultiStreamFuser(net, RADAR_CALIB, S, overlay=style, **kw)
    assert plain.painter is None
    rows_total = changed = 0
    for f in range(3):
        radar = [mh.stream_radar(s, f) for s in range(S)]
        surface, host, entry = _fresh_surface(frames[0])     # stream 0: device-resident, drawn in place; stream 1: a host frame
        want = plain([_fresh_surface(frames[0])[0], torch.from_numpy(frames[1])], radar)
        got = drawn([surface, torch.from_numpy(frames[1])], radar)
        for s in range(S):
            assert torch.equal(got[s][0], want[s][0]), f"step {f} stream {s}: rows differ with overlay"
            assert set(got[s][1]) == set(want[s][1]) | {"overlay", "overlay_status"}
            info = got[s][1]
            assert np.array_equal(info["tracks"], want[s][1]["tracks"]) and info["overlay_status"] == 0
            assert np.array_equal(info["ranges"], want[s][1]["ranges"], equal_nan=True)
            expect = frames[s].copy()
            assert fo.draw_detections(expect, "rgb", got[s][0].numpy(), info["tracks"], info["ranges"], **style) == fo.OK
            assert info["overlay"].buffer.is_cuda and np.array_equal(fo.dense_frame(info["overlay"]), expect), f"step {f} stream {s}"
            rows_total += len(got[s][0])
            changed += int((expect != frames[s]).sum())
        assert got[0][1]["overlay"] is surface
        after = surface.buffer.cpu().numpy()                 # in place: the padding and the bytes around stay
        expect = host.copy()
        fr.store(expect, entry, fo.dense_frame(surface))
        assert np.array_equal(after, expect)
        if f == 0:   # the host fuser draws the same rules on a copy
            single = FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=mh.MIN_HITS, ranging=True, overlay=style)
            before = frames[1].copy()
            rows_h, info_h = single(frames[1], radar[1])
            expect = frames[1].copy()
            fo.draw_detections(expect, "rgb", rows_h.numpy(), None, info_h["ranges"], **style)
            assert info_h["overlay_status"] == 0 and np.array_equal(info_h["overlay"], expect) and np.array_equal(frames[1], before)
    print(f"fuser: {rows_total} detections, {changed} bytes drawn")
    assert rows_total > 0 and changed > 0
    with pytest.raises(hip.MeError):
        MultiStreamFuser(net, RADAR_CALIB, S, tail="host", overlay=True)
    with pytest.raises(hip.MeError):
        MultiStreamFuser(net, RADAR_CALIB, S, overlay=dict(thickness=0))


def test_fuser_overlay_on_packed_native_frames(hip_lib):
    """Host frames in native formats through the packed path (no surfaces): the uploaded bytes are drawn into."""
    from millieye_amd.demo import MultiStreamFuser
    from tests import multistream_helpers as mh
    from tests import pixel_format_refs as pf
    from tests.golden.make_golden import RADAR_CALIB
    from tests.test_gpu_multistream import _net
    net = _net()
    S = 2
    names = ["bgr", "nv12"]
    frames = [np.ascontiguousarray(mh.stream_frame(0)[:, :, ::-1]), pf.native_frame("nv12", *mh.FRAME_SIZES[1], seed=1)]
    kw = dict(model_mode=3, min_hits=mh.MIN_HITS, pixel_format=names)
    plain, drawn = MultiStreamFuser(net, RADAR_CALIB, S, **kw), MultiStreamFuser(net, RADAR_CALIB, S, overlay=True, **kw)
    radar = [mh.stream_radar(s, 0) for s in range(S)]
    tensors = [torch.from_numpy(f) for f in frames]
    want, got = plain(tensors, radar), drawn(tensors, radar)
    total = 0
    for s in range(S):
        assert torch.equal(got[s][0], want[s][0]) and "tracks" not in got[s][1]
        expect = frames[s].copy()
        assert fo.draw_detections(expect, names[s], got[s][0].numpy()) == got[s][1]["overlay_status"] == 0
        assert np.array_equal(fo.dense_frame(got[s][1]["overlay"]), expect), f"stream {s}"
        total += len(got[s][0])
    print(f"packed native frames: {total} detections drawn")
