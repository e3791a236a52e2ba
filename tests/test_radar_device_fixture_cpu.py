"""CPU: the inputs of tests/test_gpu_multistream.py are such that an exact comparison between the device radar chain and
the host ``RadarProposalGenerator`` is meaningful.  These are conditions on the inputs alone (the host generator runs here,
no kernel): no decision of the chain sits on a rounding boundary.  If a seed violates one, other seeds are chosen - the
conditions are not loosened."""
import itertools

import numpy as np

from millieye_amd import hip
from tests import multistream_helpers as mh


def _runs():
    hosts = [mh.HostStream() for _ in range(mh.STREAMS)]
    return [[hosts[s].step(mh.stream_radar(s, f)) for s in range(mh.STREAMS)] for f in range(mh.FRAMES)], hosts[0].gen


def _assignment_totals(cost):
    """Totals of every complete assignment of the smaller side of ``cost`` (brute force)."""
    if cost.shape[0] > cost.shape[1]:
        cost = cost.T
    rows = range(cost.shape[0])
    return sorted(sum(cost[i, j] for i, j in zip(rows, perm)) for perm in itertools.permutations(range(cost.shape[1]), len(rows)))


def test_streams_keep_every_decision_off_the_rounding_boundaries():
    steps, gen = _runs()
    weights, eps = np.array(gen.dbscan_weights, dtype=float), gen.dbscan_eps
    width, height = gen.image_size
    associations = 0
    for step in steps:
        for r in step:
            # projection: truncation to the pixel and the FOV edges (integers), depth and velocity edges of the filter
            for name in ("u", "v"):
                val = r[name]
                assert np.isfinite(val).all()
                assert np.abs(val - np.rint(val)).min() > 1e-6, f"a projected {name} lies within 1e-6 of an integer"
            assert np.abs(r["xyzv_all"][:, 2] - gen.max_depth).min() > 1e-6
            assert np.abs(np.abs(r["xyzv_all"][:, 3]) - gen.min_velocity).min() > 1e-6
            # DBSCAN: no pair at eps
            x = r["xyzv"] * weights
            dist = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
            assert np.abs(dist - eps).min() > 1e-9, "a pairwise weighted distance lies within 1e-9 of eps"
            # association: a unique optimum with a margin
            cost = r["cost"]
            if cost.size and min(cost.shape) > 0 and max(cost.shape) > 1:
                totals = _assignment_totals(cost)
                assert totals[1] - totals[0] > 1e-6 * abs(totals[1]), f"assignment margin {totals[:2]}"
                associations += 1
            # capacities
            assert len(r["xyzv"]) < hip.RADAR_MAX_POINTS
            assert len(r["fresh"]) < hip.RADAR_MAX_CLUSTERS
            assert r["tracks_peak"] < hip.RADAR_MAX_TRACKS
    assert associations > mh.STREAMS, "the streams must exercise the assignment"
    assert any(len(r["proposals"]) for r in steps[-1]), "the streams must produce proposals"
    assert any(t["time_since_update"] > 0 for step in steps for r in step for t in r["state"]), "a track must coast"


def test_frames_stay_clear_of_the_dark_threshold():
    dark, bright = 0, 0
    for s in range(mh.STREAMS):
        for forced in (None, False):
            mean = mh.frame_mean(mh.stream_frame(s, dark=forced))
            assert abs(mean - mh.DARK_THRESHOLD) > 1e-3, f"stream {s}: frame mean {mean}"
            dark, bright = dark + (mean < mh.DARK_THRESHOLD), bright + (mean >= mh.DARK_THRESHOLD)
    assert dark and bright
    first_six = [mh.frame_mean(mh.stream_frame(s)) < mh.DARK_THRESHOLD for s in range(6)]
    assert any(first_six) and not all(first_six), "the fuser test needs both sub-batches"


def test_kalman_bar_is_measured_and_small():
    """The bar of the float64 comparison is 16 x the deviation between two equally valid roundings of the host tracker; it
    has to exist (> 0: the two runs do differ) and to stay a rounding-level quantity."""
    dev = mh.kalman_deviation()
    print(f"kalman deviation inv vs solve: {dev:.3e}; bar {16 * dev:.3e}")
    assert 0.0 < dev < 1e-9
