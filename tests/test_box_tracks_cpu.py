"""The host detection tracker (millieye_amd/detection_tracks.py:DetectionTracker) against the independent float64 reference of
tests/box_tracks_refs.py, the checks on the scenes both suites use, the reordering scale the GPU test's bar is built from, the
tracker's life cycle and the C ABI of the device tracker.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from millieye_amd import detection_tracks as dt
from tests import box_tracks_refs as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(20)
LOADS = (0, 1, 2, 4, 6, 9)


@pytest.fixture(scope="module")
def scenes():
    return [br.scene(s, people=LOADS[s % 6]) for s in SEEDS]


@pytest.fixture(scope="module")
def records(scenes):
    """One reference run per scene: the records of every step."""
    out = []
    for sc in scenes:
        ref = br.RefTracker()
        out.append(([ref.step(rows) for rows in sc], ref))
    return out


def _same_state(host, ref):
    a, fc = host.state()
    b, fc_ref = ref.state()
    assert fc == fc_ref and host.next_id == ref.next_id and len(a) == len(b)
    for ta, tb in zip(a, b):
        for key in ("id", "cls", "conf", "time_since_update", "hits", "hit_streak", "age", "det"):
            assert ta[key] == tb[key], key
        assert np.array_equal(ta["x"], tb["x"]) and np.array_equal(ta["P"], tb["P"])


def test_host_tracker_equals_the_reference(scenes, records):
    ids = 0
    for sc, (recs, ref_done) in zip(scenes, records):
        host, ref = dt.DetectionTracker(), br.RefTracker()
        for rows, rec in zip(sc, recs):
            got = host.step(rows)
            again = ref.step(rows)
            assert host.status == rec["status"] == br.OK
            assert np.array_equal(got, rec["rows"]) and np.array_equal(again["rows"], rec["rows"])
            assert np.array_equal(host.matches, rec["matches"]) and np.array_equal(host.iou, rec["iou"])
            _same_state(host, ref)
        ids += ref_done.next_id - 1
    assert ids > 300


def test_scene_margins(records):
    """No decision of the scenes sits on a rounding boundary: every pair the assignment chose is at least 1e-6 from iou_min,
    and forbidding any matched pair costs the assignment real IoU (the optimum's matches are unique)."""
    gate = margin = math.inf
    for recs, _ref in records:
        for rec in recs:
            gate = min(gate, br.gate_distance(rec, 0.3))
            margin = min(margin, br.decision_margin(rec["iou"], 0.3))
    print(f"smallest gate distance {gate:.3e}, smallest assignment margin {margin:.3e}")
    assert gate >= 1e-6
    assert margin >= 1e-6


def test_tie_scene_has_a_second_optimum():
    """The margin helper sees the ties of the GPU suite's tie scene."""
    a = br.grid_rows(1, 14, shuffle=False)[0]
    ref = br.RefTracker()
    ref.step(np.stack([a, a]))
    rec = ref.step(np.stack([a, a]))
    assert rec["iou"].shape == (2, 2) and br.decision_margin(rec["iou"], 0.3) == 0.0


def test_reordering_bar(scenes):
    """The general 8 x 8 filter and four 2-state filters agree on every decision; their largest deviation is the scale a
    reordering of the filter's arithmetic costs.  The GPU suite asserts 16 x this number, measured on its own scenes
    (profiles/box_tracks_errors.txt)."""
    box, state = br.reorder_deviation(scenes)
    print(f"general vs decoupled Kalman on {len(scenes)} scenes: boxes {box:.3e} px, state {state:.3e}")
    assert 0 < box < 1e-9 and 0 < state < 1e-8   # rounding, not a disagreement: boxes are hundreds of pixels, P reaches 1e4


def _row(x1, y1, x2, y2, conf=0.8, cls=0.0):
    return [x1, y1, x2, y2, conf, 0.9, cls]


def _rows(*rows):
    return np.asarray(rows, dtype=np.float32).reshape(-1, 7)


@pytest.mark.parametrize("make", [dt.DetectionTracker, br.RefTracker])
def test_life_cycle(make):
    """Coasting and death, the hit_streak reset, the first-frames window - on both host implementations."""
    def step(trk, rows):
        out = trk.step(rows)
        return out["rows"] if isinstance(out, dict) else out

    def tracks(trk):
        return trk.state()[0]

    trk = make(max_age=2, min_hits=2)
    box = lambda k: _rows(_row(100 + 2 * k, 100, 150 + 2 * k, 220))
    none = _rows()
    out = step(trk, box(0))                       # frame 1: born, reported inside the window, hit_streak 0
    assert out.shape == (1, 10) and out[0, 0] == 1 and out[0, 7] == 0 and out[0, 9] == 0
    out = step(trk, box(1))                       # frame 2: hit_streak 1 < min_hits, still inside the window
    assert len(out) == 1 and out[0, 7] == 1
    out = step(trk, box(2))                       # frame 3: hit_streak 2
    assert len(out) == 1 and out[0, 7] == 2 and out[0, 8] == 2
    for k in range(2):                            # coasts max_age steps ..
        assert len(step(trk, none)) == 0 and len(tracks(trk)) == 1 and tracks(trk)[0]["time_since_update"] == k + 1
    assert tracks(trk)[0]["hit_streak"] == 0      # .. with the streak gone after the first miss
    assert len(step(trk, none)) == 0 and len(tracks(trk)) == 0   # .. and dies
    # a miss resets the streak: after it the track is silent until min_hits updates in a row
    trk = make(max_age=3, min_hits=2)
    for k in range(3):
        step(trk, box(k))
    step(trk, none)
    out = step(trk, box(4))
    assert len(out) == 0 and tracks(trk)[0]["hit_streak"] == 1 and tracks(trk)[0]["id"] == 1
    out = step(trk, box(5))
    assert len(out) == 1 and out[0, 0] == 1 and out[0, 7] == 2
    # outside the window a fresh track is silent
    out = step(trk, _rows(box(6)[0], _row(400, 300, 440, 380)))
    assert out[:, 0].tolist() == [1.0] and [t["id"] for t in tracks(trk)] == [1, 2]


@pytest.mark.parametrize("make", [dt.DetectionTracker, br.RefTracker])
def test_gates_and_clamp(make):
    def step(trk, rows):
        out = trk.step(rows)
        return out["rows"] if isinstance(out, dict) else out

    # birth_conf: weak detections start no track but update one
    trk = make(birth_conf=0.5, min_hits=1)
    assert len(step(trk, _rows(_row(10, 10, 60, 110, conf=0.49)))) == 0 and len(trk.state()[0]) == 0
    step(trk, _rows(_row(10, 10, 60, 110, conf=0.5)))
    out = step(trk, _rows(_row(11, 10, 61, 110, conf=0.2)))
    assert len(out) == 1 and out[0, 0] == 1 and out[0, 5] == np.float32(0.2)
    # the class gate: the same box in another class is another track
    trk = make(min_hits=1)
    step(trk, _rows(_row(10, 10, 60, 110, cls=0.0)))
    out = step(trk, _rows(_row(10, 10, 60, 110, cls=1.0)))
    tracks = trk.state()[0]
    assert len(out) == 0 and [(t["id"], t["cls"], t["time_since_update"]) for t in tracks] == [(1, 0.0, 1), (2, 1.0, 0)]
    # iou_min: a box that overlaps too little starts a track of its own
    trk = make(min_hits=1, iou_min=0.5)
    step(trk, _rows(_row(0, 0, 100, 100)))
    step(trk, _rows(_row(50, 0, 150, 100)))      # IoU 1/3
    assert [t["id"] for t in trk.state()[0]] == [1, 2]
    # the clamp: a width that shrinks fast stops at the step that would take it to zero, and never goes negative
    trk = make(max_age=10, min_hits=1)
    for w in (200, 170, 140, 110):
        step(trk, _rows(_row(300 - w / 2, 100, 300 + w / 2, 300)))
    widths = []
    for _ in range(6):
        step(trk, _rows())
        t = trk.state()[0][0]
        widths.append(float(t["x"][2]))
        assert t["x"][2] > 0
    assert t["x"][6] == 0.0 and widths[-1] == widths[-2] and widths[0] > widths[-1]


@pytest.mark.parametrize("make", [dt.DetectionTracker, br.RefTracker])
def test_statuses_leave_the_state_untouched(make):
    def status(trk, rows):
        out = trk.step(rows)
        return (out["status"], len(out["rows"])) if isinstance(out, dict) else (trk.status, len(out))

    def snapshot(trk):
        tracks, fc = trk.state()
        return fc, trk.next_id, [(t["id"], t["x"].tobytes(), t["P"].tobytes(), t["time_since_update"], t["hits"], t["hit_streak"],
                                  t["age"], t["det"], t["conf"]) for t in tracks]

    trk = make()
    assert status(trk, br.grid_rows(40, 6, spacing=70.0)) == (br.OK, 40)
    before = snapshot(trk)
    too_many = np.concatenate([br.grid_rows(64, 8, spacing=70.0), br.grid_rows(1, 9, origin=(5000.0, 5000.0))])
    assert status(trk, too_many) == (br.E_DETS, 0) and snapshot(trk) == before
    for bad in (np.nan, np.inf, -np.inf):
        rows = br.grid_rows(5, 10, spacing=70.0)
        rows[3, 1] = bad
        assert status(trk, rows) == (br.E_INPUT, 0) and snapshot(trk) == before
    assert status(trk, br.grid_rows(25, 7, spacing=70.0, origin=(2000.0, 2000.0))) == (br.E_TRACKS, 0)
    assert snapshot(trk) == before
    assert status(trk, br.grid_rows(24, 7, spacing=70.0, origin=(2000.0, 2000.0))) == (br.OK, 24)   # frame 2 <= min_hits
    assert snapshot(trk)[0] == before[0] + 1 and len(snapshot(trk)[2]) == 64


def test_c_abi_of_the_tracker():
    """Header, exports and hip.SIGNATURES agree for the new names; the descriptor and the state layout are the binding's."""
    import __graft_entry__ as g
    from millieye_amd import hip
    g.build()
    header = open(os.path.join(ROOT, "include", "millieye_hip.h")).read()
    names = {"me_box_tracks_capacity", "me_box_tracks_state_bytes", "me_box_tracks_reset", "me_box_tracks_f64"}
    declared = set(re.findall(r"\b(me_box_tracks_[a-z0-9_]+)\s*\(", header))
    assert declared == names and names <= set(hip.SIGNATURES)
    lib = hip.load()
    for name in names:
        assert hasattr(lib, name)
    assert lib.me_abi_version() == 13 and "#define ME_ABI_VERSION 13" in header
    assert lib.me_sizeof(13) == ctypes.sizeof(hip.BoxTracksDesc) == 80 and hip._STRUCTS[13] is hip.BoxTracksDesc
    defines = dict(re.findall(r"#define (ME_TRACKS_[A-Z_]+) (\d+)", header))
    assert {k: int(v) for k, v in defines.items()} == dict(
        ME_TRACKS_MAX_DETS=hip.TRACKS_MAX_DETS, ME_TRACKS_MAX_TRACKS=hip.TRACKS_MAX_TRACKS, ME_TRACKS_ROW_COLS=hip.TRACKS_ROW_COLS,
        ME_TRACKS_COUNT_COLS=hip.TRACKS_COUNT_COLS, ME_TRACKS_OK=hip.TRACKS_OK, ME_TRACKS_E_DETS=hip.TRACKS_E_DETS,
        ME_TRACKS_E_INPUT=hip.TRACKS_E_INPUT, ME_TRACKS_E_TRACKS=hip.TRACKS_E_TRACKS)
    assert (dt.MAX_DETS, dt.MAX_TRACKS, dt.ROW_COLS) == (hip.TRACKS_MAX_DETS, hip.TRACKS_MAX_TRACKS, hip.TRACKS_ROW_COLS)
    assert (dt.OK, dt.E_DETS, dt.E_INPUT, dt.E_TRACKS) == (br.OK, br.E_DETS, br.E_INPUT, br.E_TRACKS) == (0, 1, 2, 3)
    got = [lib.me_box_tracks_capacity(i) for i in range(7)]
    assert got == [64, 64, 10, 4, hip.TRACKS_STATE_HEADER_BYTES, hip.TRACKS_TRACK_BYTES, -1]
    assert lib.me_box_tracks_state_bytes(3) == 3 * (32 + 64 * 224) and lib.me_box_tracks_state_bytes(0) == 0
    # argument checks need no GPU
    assert lib.me_box_tracks_f64(None, None) != 0 and b"null descriptor" in lib.me_last_error()
    d = hip.BoxTracksDesc()
    assert lib.me_box_tracks_f64(ctypes.byref(d), None) != 0 and b"null pointer" in lib.me_last_error()
    assert lib.me_box_tracks_reset(None, 1, 0, None) != 0


def test_fuser_refuses_tracks_on_the_host_tail():
    from millieye_amd import hip
    from millieye_amd.demo import MultiStreamFuser
    with pytest.raises(hip.MeError):
        MultiStreamFuser(None, None, 2, tail="host", tracks=True)
    with pytest.raises(hip.MeError):
        MultiStreamFuser(None, None, 2, tracks="yes")
    assert MultiStreamFuser(None, None, 2).track_params is None
    assert MultiStreamFuser(None, None, 2, tracks=dict(max_age=2)).track_params == dict(max_age=2)
