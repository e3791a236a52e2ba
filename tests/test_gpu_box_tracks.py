"""The device detection tracker (csrc/box_tracks.hip: me_box_tracks_f64; detection_tracks.DeviceDetectionTracks,
hip.stream_tail_tracks, MultiStreamFuser(tracks=)) against the float64 reference of tests/box_tracks_refs.py.

Decisions (ids, det, counters, matches, row counts, statuses) are exact.  Boxes and the read-back state are compared under
16 x the deviation that the reference's general 8 x 8 Kalman filter and its decoupled restatement show on the very scenes of
the test (box_tracks_refs.reorder_deviation; tests/test_box_tracks_cpu.py measures the same on its scenes: 1.1e-13 px for the
boxes, 7.8e-13 for the state, whose covariance entries reach 1e4)."""
import math

import numpy as np
import pytest
import torch

from tests import box_tracks_refs as br

pytestmark = pytest.mark.gpu

NAN = float("nan")
MARK = -77   # pre-fill of the matches slots


def _tracker(streams, **kw):
    from millieye_amd.detection_tracks import DeviceDetectionTracks
    return DeviceDetectionTracks(streams, debug=True, **kw)


def _dev_tail(per_stream, gaps=None, status=0):
    buf, m = br.tail_buffer(per_stream, gaps, status)
    return torch.from_numpy(buf).to("cuda"), m


def _prefill(trk):
    trk._tracks.fill_(NAN)
    trk._cost.fill_(NAN)
    trk._matches.fill_(MARK)
    trk._counts.fill_(MARK)


def _state_bytes(trk, s):
    per = trk._state.numel() // trk.streams
    return trk._state[s * per:(s + 1) * per].cpu().numpy().copy()


def _check_stream(trk, s, got, status, rec, ref, bars, what, worst):
    """One stream of one step against its reference record ``rec`` (and reference tracker ``ref`` after the step)."""
    assert status == rec["status"], f"{what}: status {status} vs {rec['status']}"
    want = rec["rows"]
    assert got.shape == want.shape, f"{what}: {got.shape[0]} rows vs {want.shape[0]}"
    exact = [0, 5, 6, 7, 8, 9]   # id, conf, cls, hit_streak, age, det
    assert np.array_equal(got[:, exact], want[:, exact]), f"{what}: ids / counters / det differ"
    if len(want):
        dev = float(np.abs(got[:, 1:5] - want[:, 1:5]).max())
        worst[0] = max(worst[0], dev)
        assert dev <= bars[0], f"{what}: boxes off by {dev:.3e} > {bars[0]:.3e}"
    counts = trk.host_counts[s]
    tracks_ref, frame_count = ref.state()
    assert counts[0] == rec["status"] and counts[1] == len(want)
    assert counts[2] == len(tracks_ref) and counts[3] == frame_count, f"{what}: live tracks / frame_count {counts}"
    # nothing behind the row count, nothing outside [tracks before, detections]
    assert torch.isnan(trk._tracks[s, len(want):]).all(), f"{what}: wrote behind its rows"
    T, D = rec["tracks_before"], rec["dets"]
    if rec["status"] == br.OK:
        cost = trk.cost(s)
        assert np.isnan(cost[T:]).all() and np.isnan(cost[:, D:]).all(), f"{what}: cost outside [{T}, {D}]"
        matches = trk.matches(s)
        assert np.array_equal(matches[:T], rec["matches"]), f"{what}: matches {matches[:T]} vs {rec['matches']}"
        assert (matches[T:] == MARK).all(), f"{what}: matches behind {T}"
        if T and D:
            dc = float(np.abs(cost[:T, :D] - rec["iou"]).max())
            assert dc <= bars[0], f"{what}: iou off by {dc:.3e}"   # (dimensionless, in [0, 1]: far inside the pixel bar)
    else:
        assert np.isnan(trk.cost(s)).all() and (trk.matches(s) == MARK).all(), f"{what}: outputs of a refused step"


def _check_state(trk, s, ref, bars, what, worst):
    got, (frame_count, next_id) = trk.track_state(s)
    want, fc = ref.state()
    assert frame_count == fc and next_id == ref.next_id, f"{what}: frame_count / next_id"
    assert len(got) == len(want), f"{what}: {len(got)} live tracks vs {len(want)}"
    for g, w in zip(got, want):
        for key in ("id", "cls", "conf", "time_since_update", "hits", "hit_streak", "age", "det"):
            assert g[key] == w[key], f"{what}: track {w['id']} {key} {g[key]} vs {w[key]}"
    if want:
        dev = br.state_deviation(got, want)
        worst[1] = max(worst[1], dev)
        assert dev <= bars[1], f"{what}: state off by {dev:.3e} > {bars[1]:.3e}"


def _run(scenes, what, state_every=1, gaps=None, **params):
    """All streams of ``scenes`` (per stream a list of per-step rows, equally long) through one device tracker, every step
    against one reference per stream.  Returns the tracker, the references and the worst deviations."""
    S, steps = len(scenes), len(scenes[0])
    box_dev, state_dev = br.reorder_deviation(scenes, **params)
    bars = (16 * box_dev, 16 * state_dev)
    trk = _tracker(S, **params)
    refs = [br.RefTracker(**params) for _ in range(S)]
    worst = [0.0, 0.0]
    for f in range(steps):
        per_stream = [scenes[s][f] for s in range(S)]
        recs = [refs[s].step(per_stream[s]) for s in range(S)]
        out, m = _dev_tail(per_stream, None if gaps is None else [gaps(s, f) for s in range(S)])
        _prefill(trk)
        got, status = trk.step(out, m)
        for s in range(S):
            _check_stream(trk, s, got[s], status[s], recs[s], refs[s], bars, f"{what} stream {s} step {f}", worst)
            if f % state_every == state_every - 1 or f == steps - 1:
                _check_state(trk, s, refs[s], bars, f"{what} stream {s} step {f}", worst)
    print(f"{what}: worst box deviation {worst[0]:.3e} px (bar {bars[0]:.3e}), worst state deviation {worst[1]:.3e} "
          f"(bar {bars[1]:.3e})")
    return trk, refs, worst


LOADS = (0, 1, 2, 4, 6, 9)


def test_scenes(hip_lib):
    """33 streams x 40 steps: different seeds and loads, every sixth stream always empty, rows of each stream behind a
    different number of rows that the tail did not keep."""
    scenes = [br.scene(s, people=LOADS[s % 6]) for s in range(33)]
    assert sum(len(r) for sc in scenes for r in sc) > 2000 and all(len(r) == 0 for r in scenes[6])
    trk, refs, _worst = _run(scenes, "scenes", state_every=8, gaps=lambda s, f: (s + f) % 3)
    assert sum(r.next_id - 1 for r in refs) > 300


def test_step2_cost_bits(hip_lib):
    """After a birth-only step the predicted boxes are exactly the step-1 detections (velocity 0, centre and size exact in
    float64): the step-2 cost output is the reference's IoU matrix bit for bit."""
    first = br.grid_rows(20, 1, jitter=3.0)
    second = br.grid_rows(23, 2, jitter=3.0)
    second[:, 6] = np.arange(23) % 2 == 0   # a second class: exact zeros across classes
    first[:, 6] = np.arange(20) % 3 == 0
    trk, refs, _w = _run([[first, second]], "step 2")
    cost = np.ascontiguousarray(trk.cost(0, 20, 23))
    ref = br.RefTracker()
    ref.step(first)
    rec = ref.step(second)
    assert rec["tracks_before"] == 20 and (rec["iou"] > 0).sum() > 40
    assert cost.tobytes() == rec["iou"].tobytes()


def _capacity_scenes():
    first = br.grid_rows(64, 3, jitter=2.0)
    second = br.grid_rows(64, 4, jitter=2.0)       # the same 64 places, other jitter, other order: a near-permutation
    third = br.grid_rows(64, 5, jitter=6.0)
    return [first, second, third]


@pytest.mark.parametrize("streams", [1, 4])
def test_capacity(hip_lib, streams):
    """64 tracks x 64 detections per stream (neighbours on the grid overlap: about 250 non-zero IoUs besides the diagonal)."""
    scenes = [_capacity_scenes() for _ in range(streams)]
    for s in range(1, streams):   # other orders in the other streams
        scenes[s] = [r[np.random.default_rng(50 + s).permutation(len(r))] for r in scenes[s]]
    trk, refs, _w = _run(scenes, f"capacity S={streams}", min_hits=1)
    assert all(len(r.tracks) == 64 for r in refs)
    assert trk.host_counts[:, 1].tolist() == [64] * streams


def test_capacity_refusals(hip_lib):
    """65 detections -> E_DETS; 40 live tracks + 25 births -> E_TRACKS: the stream's state is bit-identical before and after,
    its neighbours advance."""
    forty = br.grid_rows(40, 6, spacing=70.0)
    far = br.grid_rows(25, 7, spacing=70.0, origin=(2000.0, 2000.0))
    sixty_five = np.concatenate([br.grid_rows(64, 8, spacing=70.0), br.grid_rows(1, 9, origin=(5000.0, 5000.0))])
    few = br.grid_rows(5, 10, spacing=70.0)
    S = 4
    trk = _tracker(S)
    refs = [br.RefTracker() for _ in range(S)]
    box_dev, state_dev = br.reorder_deviation([[forty, forty, forty]])
    bars = (16 * box_dev, 16 * state_dev)
    worst = [0.0, 0.0]

    def step(per_stream, what):
        recs = [refs[s].step(per_stream[s]) for s in range(S)]
        out, m = _dev_tail(per_stream)
        _prefill(trk)
        got, status = trk.step(out, m)
        for s in range(S):
            _check_stream(trk, s, got[s], status[s], recs[s], refs[s], bars, f"{what} stream {s}", worst)
            _check_state(trk, s, refs[s], bars, f"{what} stream {s}", worst)
        return status

    assert step([forty, forty, few, forty], "first") == [0, 0, 0, 0]
    before = [_state_bytes(trk, s) for s in range(S)]
    status = step([forty, far, sixty_five, sixty_five], "refusals")
    assert status == [br.OK, br.E_TRACKS, br.E_DETS, br.E_DETS]
    after = [_state_bytes(trk, s) for s in range(S)]
    for s in (1, 2, 3):
        assert np.array_equal(before[s], after[s]), f"stream {s}: a refused step changed the state"
    assert not np.array_equal(before[0], after[0])
    assert step([forty, forty, few, forty], "after the refusals") == [0, 0, 0, 0]


@pytest.mark.parametrize("tracks,dets", [(1, 64), (64, 1), (37, 12), (12, 37)])
def test_rectangular_assignments(hip_lib, tracks, dets):
    """More detections than tracks and the transposed problem: ``tracks`` births, then ``dets`` detections on the same grid."""
    first = br.grid_rows(tracks, 11, jitter=2.0)
    second = br.grid_rows(64, 12, jitter=2.0, shuffle=False)[np.random.default_rng(13).permutation(64)[:dets]]
    if dets == 1:
        second = br.grid_rows(64, 12, jitter=2.0, shuffle=False)[27:28]
    if tracks == 1:
        first = br.grid_rows(64, 11, jitter=2.0, shuffle=False)[27:28]
    _trk, refs, _w = _run([[first, second, second]], f"{tracks} x {dets}", min_hits=1)
    assert refs[0].next_id - 1 >= max(tracks, dets)


def test_exact_ties(hip_lib):
    """Duplicated detections, duplicated tracks and an all-equal 5 x 5 block: the duplicated rows' costs are bit-equal and the
    matches are scipy's."""
    a, b, c = br.grid_rows(3, 14, spacing=200.0, shuffle=False)
    five = np.stack([c] * 5)
    first = np.stack([a, a, b] + [c] * 5)            # tracks 0, 1 identical; tracks 3..7 identical
    second = np.concatenate([np.stack([a, b, b]), five]).astype(np.float32)   # one detection for two tracks; two for one
    second[:, :4] += np.float32(1.5)
    third = second[[7, 3, 0, 5, 1, 6, 2, 4]]
    ref = br.RefTracker()
    ref.step(first)
    rec = ref.step(second)
    iou = rec["iou"]
    assert iou[0].tobytes() == iou[1].tobytes() and iou[:, 1].tobytes() == iou[:, 2].tobytes()
    assert len({iou[i, j].tobytes() for i in range(3, 8) for j in range(3, 8)}) == 1 and iou[3, 3] > 0.3
    trk, refs, _w = _run([[first, second, third, third]], "ties", min_hits=1)
    cost = trk.cost(0)
    assert not np.isnan(cost[:8, :8]).any()


def test_bad_input(hip_lib):
    """A NaN or infinite coordinate -> E_INPUT for that stream alone; a set status word of the tail -> E_INPUT for all; in both
    cases no state changes and no output slot of the refused streams is written."""
    good = br.grid_rows(6, 15, spacing=90.0)
    S = 3
    trk = _tracker(S)
    refs = [br.RefTracker() for _ in range(S)]
    bars = tuple(16 * v for v in br.reorder_deviation([[good, good, good]]))
    worst = [0.0, 0.0]

    def step(per_stream, what, flag=0):
        recs = [refs[s].step(per_stream[s]) if not flag else refs[s]._refuse(br.E_INPUT, len(per_stream[s])) for s in range(S)]
        out, m = _dev_tail(per_stream, gaps=[2, 0, 1], status=flag)
        _prefill(trk)
        got, status = trk.step(out, m)
        for s in range(S):
            _check_stream(trk, s, got[s], status[s], recs[s], refs[s], bars, f"{what} stream {s}", worst)
            _check_state(trk, s, refs[s], bars, f"{what} stream {s}", worst)
        return status

    assert step([good, good, good], "first") == [0, 0, 0]
    nan_row, inf_row = good.copy(), good.copy()
    nan_row[4, 2] = np.nan
    inf_row[0, 1] = -np.inf
    before = [_state_bytes(trk, s) for s in range(S)]
    assert step([good, nan_row, inf_row], "non-finite") == [br.OK, br.E_INPUT, br.E_INPUT]
    assert all(np.array_equal(before[s], _state_bytes(trk, s)) for s in (1, 2))
    before = [_state_bytes(trk, s) for s in range(S)]
    assert step([good, good, good], "flagged tail", flag=1) == [br.E_INPUT] * 3
    assert all(np.array_equal(before[s], _state_bytes(trk, s)) for s in range(S))
    assert step([good, good, good], "after the refusals") == [0, 0, 0]


def test_reset_and_many_streams(hip_lib):
    """300 streams in one launch; reset(stream) restarts that stream alone and its ids start again at 1; m = 0 is a step."""
    S = 300
    rows = [br.grid_rows(1 + s % 5, 100 + s, spacing=90.0) for s in range(S)]
    scenes = [[rows[s], rows[s], np.zeros((0, 7), np.float32)] for s in range(S)]
    params = dict(min_hits=1)
    trk = _tracker(S, **params)
    refs = [br.RefTracker(**params) for _ in range(S)]
    bars = tuple(16 * v for v in br.reorder_deviation(scenes[:5], **params))
    worst = [0.0, 0.0]
    for f in range(3):
        per_stream = [scenes[s][f] for s in range(S)]
        if f == 2:
            trk.reset(7)
            refs[7] = br.RefTracker(**params)
        recs = [refs[s].step(per_stream[s]) for s in range(S)]
        out, m = _dev_tail(per_stream)
        assert (m == 0) == (f == 2)
        _prefill(trk)
        got, status = trk.step(out, m)
        for s in range(S):
            _check_stream(trk, s, got[s], status[s], recs[s], refs[s], bars, f"S=300 stream {s} step {f}", worst)
        for s in (0, 6, 7, 8, 299):
            _check_state(trk, s, refs[s], bars, f"S=300 stream {s} step {f}", worst)
    assert trk.track_state(7) == ([], (1, 1)) and trk.track_state(8)[1] == (3, refs[8].next_id)
    # ids start again at 1
    per_stream = [rows[s] for s in range(S)]
    out, m = _dev_tail(per_stream)
    got, _status = trk.step(out, m)
    assert [t["id"] for t in trk.track_state(7)[0]] == list(range(1, 2 + 7 % 5)) and trk.host_counts[7, 3] == 2
    assert len(got[7]) == 0 and len(got[8]) == 1 + 8 % 5
    with pytest.raises(hip_mod().MeError):
        trk.reset(S)
    trk.reset()
    assert trk.track_state(0) == ([], (0, 1)) and trk.track_state(299) == ([], (0, 1))


def hip_mod():
    from millieye_amd import hip
    return hip


def test_fuser_tracks(hip_lib):
    """MultiStreamFuser(tracks=True): the detection rows are those of tracks=None, info["tracks"] is the reference fed the
    fuser's own rows, tail="host" refuses."""
    from millieye_amd import hip
    from millieye_amd.demo import MultiStreamFuser
    from tests import multistream_helpers as mh
    from tests.golden.make_golden import RADAR_CALIB
    from tests.test_gpu_multistream import _net
    net = _net()
    S = 3
    params = dict(min_hits=2, iou_min=0.2)
    frames = [mh.stream_frame(s) for s in range(S)]
    plain = MultiStreamFuser(net, RADAR_CALIB, S, model_mode=3, min_hits=mh.MIN_HITS)
    tracked = MultiStreamFuser(net, RADAR_CALIB, S, model_mode=3, min_hits=mh.MIN_HITS, tracks=params)
    assert plain.tracker is None
    steps = []
    for f in range(6):
        radar = [mh.stream_radar(s, f) for s in range(S)]
        want, got = plain(frames, radar), tracked(frames, radar)
        for s in range(S):
            assert torch.equal(got[s][0], want[s][0]), f"step {f} stream {s}: rows differ with tracks"
            assert "tracks" not in want[s][1] and set(got[s][1]) == set(want[s][1]) | {"tracks", "track_status"}
        steps.append(got)
    scenes = [[steps[f][s][0].numpy() for f in range(6)] for s in range(S)]
    assert sum(len(r) for sc in scenes for r in sc) > 0
    bars = tuple(16 * v for v in br.reorder_deviation(scenes, **params))
    total = 0
    for s in range(S):
        ref = br.RefTracker(**params)
        for f in range(6):
            rec, info = ref.step(scenes[s][f]), steps[f][s][1]
            got = info["tracks"]
            assert info["track_status"] == rec["status"] == 0
            assert got.dtype == np.float64 and got.shape == rec["rows"].shape, f"step {f} stream {s}"
            assert np.array_equal(got[:, [0, 5, 6, 7, 8, 9]], rec["rows"][:, [0, 5, 6, 7, 8, 9]])
            if len(got):
                assert float(np.abs(got[:, 1:5] - rec["rows"][:, 1:5]).max()) <= bars[0]
            total += len(got)
    assert total > 0
    with pytest.raises(hip.MeError):
        MultiStreamFuser(net, RADAR_CALIB, S, tail="host", tracks=True)
    assert math.isfinite(bars[0])
