"""CPU: the scenes of tests/radar_scene_helpers.py are what tests/test_gpu_radar_chain.py needs them to be - they reach the
designed counts exactly (256 kept points, 32 clusters, 32 tracks; 257 and 33 in the refused cases), and no decision of the chain
sits on a rounding boundary, so that an exact comparison between the device chain and the host ``RadarProposalGenerator`` is
meaningful.  These are conditions on the inputs alone (the host generator runs here, no kernel).  If a seed violates one,
another seed is chosen - the conditions are not loosened."""
import numpy as np
import pytest

from millieye_amd import hip
from tests import multistream_helpers as mh, radar_scene_helpers as sh


def _run(radar, streams, frames, tie=False, **kw):
    """Host records ``[stream][frame]`` of a family, every step through :func:`radar_scene_helpers.check_step`; and the
    relative assignment margins met."""
    out, margins = [], []
    for s in range(streams):
        h = mh.HostStream(**kw)
        out.append([])
        for f in range(frames):
            r = h.step(radar(s, f))
            m = sh.check_step(r, h.gen, tie=tie)
            if m is not None:
                margins.append(m)
            out[-1].append(r)
    return out, margins


def test_capacities_are_the_librarys():
    assert (sh.MAXP, sh.MAXC, sh.MAXT) == (hip.RADAR_MAX_POINTS, hip.RADAR_MAX_CLUSTERS, hip.RADAR_MAX_TRACKS)


def test_capacity_grid_counts_deaths_and_margins():
    runs, margins = _run(sh.grid_radar, sh.GRID_STREAMS, sh.GRID_FRAMES)
    # stream 0: full capacity in every frame
    for f, r in enumerate(runs[0]):
        assert (len(r["xyzv"]), len(r["fresh"]), len(r["state"]), len(r["proposals"])) == (256, 32, 32, 32), f"frame {f}"
        assert (r["labels"] >= 0).all() and np.array_equal(np.bincount(r["labels"]), np.full(32, 8))
    assert len(margins) == sh.GRID_STREAMS * (sh.GRID_FRAMES - 1) and min(margins) > 1e-6
    for s in (1, 2):
        per = sh.GRID_POINTS if s == 1 else sh.GRID_POINTS - 1
        alive = [len(r["state"]) for r in runs[s]]
        assert alive == [32] * 7 + [28, 28, 29, 29, 29], f"stream {s}: live tracks {alive}"
        assert [len(r["fresh"]) for r in runs[s]] == [32] * 3 + [28] * 6 + [29] * 3
        assert [len(r["xyzv"]) for r in runs[s]] == [32 * per] * 3 + [28 * per] * 6 + [29 * per] * 3
        # the four tracks die in the same frame, at list positions that are not adjacent: the compaction has to move tracks by
        # 2, by 3 and (none behind position 31) drop the last
        before = runs[s][6]["state"]
        dying = [k for k, t in enumerate(before) if t["time_since_update"] == 4]
        assert dying == list(sh.GRID_DROPPED) and len(runs[s][7]["state"]) == len(before) - 4
        assert any(b - a > 1 for a, b in zip(dying, dying[1:]))
        # more tracks than clusters, and more clusters than tracks, at size
        shapes = [r["cost"].shape for r in runs[s] if r["cost"].size]
        assert any(t > c >= 28 for t, c in shapes) and any(c > t >= 28 for t, c in shapes), shapes
        # the returning reflector founds a new track behind the compacted list; it is confirmed two frames later
        assert runs[s][9]["tracks_before"] == 28 and runs[s][9]["matches"].min() >= 0
        assert len(runs[s][9]["tracked"]) == 28 and len(runs[s][11]["tracked"]) == 29


def test_chain_scenes():
    runs, _ = _run(sh.chain_radar, len(sh.CHAIN_ORDERS), 1)
    for s, order in enumerate(sh.CHAIN_ORDERS):
        r = runs[s][0]
        assert len(r["xyzv"]) == 256
        if order == "interleaved":
            assert np.array_equal(r["labels"], np.arange(256) % 2) and list(r["fresh"]["num_points"]) == [128, 128]
        else:
            assert not r["labels"].any() and list(r["fresh"]["num_points"]) == [256]
    # the chain is a chain: every point has its one or two neighbours only, so a label needs up to 255 rounds to travel
    vel = np.sort(sh.chain_frame("index")[3])
    assert np.allclose(np.diff(vel), sh.CHAIN_STEP) and sh.CHAIN_STEP < 1.5 < 2 * sh.CHAIN_STEP


def test_mean_velocity_scenes():
    runs, _ = _run(sh.meanv_radar, len(sh.MEANV_SIZES), 1, **sh.MEANV_KW)
    one_level = 0
    for s, n in enumerate(sh.MEANV_SIZES):
        r = runs[s][0]
        assert len(r["xyzv"]) == n and list(r["fresh"]["num_points"]) == [n], "one cluster that passes the filter shows the mean"
        m = sh.mean_variants(r["xyzv"][:, 3])
        print(n, {k: float(v) for k, v in m.items()})
        assert r["fresh"]["avgV"][0] == m["numpy"]
        assert m["pairwise"] == m["numpy"], "the plain-Python pairwise rule is numpy's"
        assert m["numpy"] != m["sequential"] and m["numpy"] != m["exact"], f"n = {n}: the order of the sum must show"
        one_level += n > 128 and m["numpy"] != m["one_level"]
    assert one_level >= 3
    # the rule itself, bit for bit in float64, beyond the scenes
    rng = np.random.RandomState(0)
    for n in (1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 500, 512):
        a = rng.randn(n) * 10.0 ** rng.uniform(-3, 3, n)
        assert sh.pairwise_sum(a) == float(np.sum(a)), n


def test_filter_edge_scenes():
    r = mh.HostStream().step([sh.edge_frame()])
    sh.check_step(r, mh.HostStream().gen)
    sizes = np.bincount(r["labels"])
    assert (r["labels"] >= 0).all() and len(sizes) == sh.EDGE_PASS + sh.EDGE_FAIL
    assert list(sizes[:2 * sh.EDGE_FAIL]) == [5, 4] * sh.EDGE_FAIL and (sizes[2 * sh.EDGE_FAIL:] == 5).all()
    assert len(r["fresh"]) == 32 == hip.RADAR_MAX_CLUSTERS
    host = mh.HostStream(num_pts_filter=2)
    r = host.step([sh.pairs_frame()])
    sh.check_step(r, host.gen)
    assert len(r["xyzv"]) == 256 and len(r["fresh"]) == 128 and (r["fresh"]["num_points"] == 2).all()


def test_over_capacity_scenes():
    for frame, want in ((sh.grid_frame(2), (256, 32)), (sh.grid_frame(2, extra_point=True), (257, 32)),
                        (sh.grid_frame(2, points=7, extra_cluster=True), (231, 33))):
        host = mh.HostStream()
        r = host.step([frame])
        sh.check_step(r, host.gen)
        assert (len(r["xyzv"]), len(r["fresh"])) == want
    host = mh.HostStream()
    r = host.step([sh.huge_velocity_frame()])
    assert len(r["fresh"]) == 4 and (r["fresh"]["avgV"] == np.float32(1e21)).all()
    with np.errstate(over="ignore"), pytest.raises(ValueError):   # scipy refuses the non-finite cost matrix
        host.step(sh.grid_radar(0, 1))


def test_many_streams_scene():
    runs, margins = _run(sh.many_radar, sh.MANY_STREAMS, sh.MANY_FRAMES)
    kept = np.array([[len(r["xyzv"]) for r in stream] for stream in runs])
    given = np.array([[len(r["keep"]) for r in stream] for stream in runs])
    assert kept.max() < hip.RADAR_MAX_POINTS and max(len(r["fresh"]) for stream in runs for r in stream) < 32
    assert (given[0::5] == 0).all() and (given[1::5] > 0).all() and (kept[1::5] == 0).all(), "empty and all-filtered streams"
    assert (kept[2::5] > 0).all() and kept[4::5].mean() > 2 * kept[2::5].mean(), "1 and 3 overlaid frames"
    assert len(set(kept[:, 0])) > 20, "ragged"
    assert len(margins) > sh.MANY_STREAMS and sum(len(r["proposals"]) for stream in runs for r in stream) > sh.MANY_STREAMS
    # streams behind the 256th have kept points and boxes in front of them: the pack kernel's prefix sums run more than once
    assert kept[:256].sum() > 0 and kept[256:].sum() > 0


def test_proposals_and_boxes_scene():
    from millieye_amd.demo import radar_boxes_for_network
    runs, _ = _run(sh.boxes_radar, len(sh.BOXES_FRAME_HW), sh.BOXES_FRAMES, **sh.BOXES_KW)
    kinds = [np.sign(h - w) for h, w in sh.BOXES_FRAME_HW]
    assert sorted(kinds) == [-1, 0, 1], "landscape, square and portrait"
    for s, hw in enumerate(sh.BOXES_FRAME_HW):
        skipped = empty = 0
        for r in runs[s]:
            size = r["tracked"]["size"].max(1).astype(np.float64)
            assert np.abs(size - sh.BOXES_KW["max_size"]).min() > 1e-6, "a tracked size within 1e-6 of max_size"
            assert len(r["proposals"]) == int((size < sh.BOXES_KW["max_size"]).sum())
            skipped += len(r["tracked"]) - len(r["proposals"])
            boxes = radar_boxes_for_network(r["proposals"], hw)
            empty += len(r["proposals"]) - len(boxes)
            # no box edge near a clamping edge (0 and the padded side), in pixels of the padded frame
            side, (left, right, top, bottom) = float(max(hw)), _pads(hw)
            px = r["proposals"] + np.array([left, top, right, bottom])
            assert min(np.abs(px).min(), np.abs(px - side).min()) > 1e-3
        assert skipped > 0 and empty > 0, f"stream {s}: {skipped} skipped, {empty} empty"
        assert len(runs[s][-1]["proposals"]) > 0 and len(radar_boxes_for_network(runs[s][-1]["proposals"], hw)) > 0


def _pads(hw):
    from millieye_amd.utils.datasets import _pad_amounts
    return _pad_amounts(*hw)


def test_tie_scene():
    runs, margins = _run(sh.tie_radar, sh.TIE_STREAMS, 2, tie=True)
    shapes = []
    for s in range(sh.TIE_STREAMS):
        first, second = runs[s][0], runs[s][1]
        # dyadic coordinates: the cluster means are exact, and the tracks hold them when frame 1 is associated
        assert np.array_equal(first["fresh"]["center"] * 16, np.rint(first["fresh"]["center"] * 16))
        cost = second["cost"]
        shapes.append(cost.shape)
        assert cost.dtype == np.float64 and np.array_equal(cost, cost.astype(np.float32)), "the float32 cost matrix"
        margin, total = sh.assignment_margin(cost)
        assert margin == 0.0 and total > 0.0, "two optimal assignments, exactly tied"
        tied = cost[:-1, :-1]
        assert tied.size >= 2 and (tied == tied.flat[0]).all()
    assert shapes == [(3, 3), (3, 2), (2, 3)]
    assert margins == [0.0] * 3


def test_assignment_margin():
    cost = np.array([[1.0, 2.0, 9.0], [2.0, 1.0, 9.0]])
    assert sh.assignment_margin(cost) == (2.0, 2.0)
    assert sh.assignment_margin(np.array([[1.0, 1.0], [1.0, 1.0]]))[0] == 0.0
    assert sh.assignment_margin(cost.T) == (2.0, 2.0)


def test_kalman_bars_are_measured_and_small():
    """The bars of the float64 comparison are 16 x the deviation between two equally valid roundings of the host tracker on the
    family's own scenes; they have to exist (> 0: the two runs do differ) and to stay rounding-level quantities.  The defaults of
    the generalised helper still give the figure of tests/test_gpu_multistream.py."""
    grid, boxes, dev_grid = sh.grid_runs()
    assert len(grid) == sh.GRID_FRAMES and len(grid[0]) == sh.GRID_STREAMS and len(boxes) == sh.BOXES_FRAMES
    dev_many = sh.kalman_deviation(sh.many_radar, sh.MANY_BAR_STREAMS, sh.MANY_FRAMES)
    dev_tie = sh.kalman_deviation(sh.tie_radar, sh.TIE_STREAMS, 2)
    print(f"inv vs solve: grid {dev_grid:.3e}, many streams {dev_many:.3e}, tie {dev_tie:.3e}")
    assert 0.0 < dev_grid < 1e-9 and 0.0 < dev_many < 1e-9 and 0.0 <= dev_tie < 1e-9
    assert mh.kalman_deviation(2, 3) == mh.kalman_deviation(2, 3, radar=mh.stream_radar, host=mh.HostStream)
    assert sh.kalman_bar(mh.stream_radar, 2, 3) == 16.0 * mh.kalman_deviation(2, 3)
