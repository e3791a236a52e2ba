"""Shared inputs and host-side yardsticks of the multi-stream tests (tests/test_radar_device_fixture_cpu.py guards them,
tests/test_gpu_multistream.py uses them): seeded radar streams ``radar_points(f + 7 * s + SEED_OFFSET)``, mixed dark / bright frames of two
sizes, a host ``RadarProposalGenerator`` per stream that records every intermediate the device chain has to reproduce, and
the measured bar for the float64 Kalman state."""
import contextlib

import numpy as np
import torch

from millieye_amd import radar_proposals as rp, synth
from oracle import datasets_ref
from tests.golden.make_golden import RADAR_CALIB, radar_points

STREAMS, FRAMES, MIN_HITS = 8, 10, 2
FRAME_SIZES = ((480, 640), (360, 480))   # (h, w)
DARK_THRESHOLD = 0.08
# radar_points(46) holds a point a few millimetres from the camera plane that projects to u = -4.8e15, an exact integer: the
# fixture conditions (no projected coordinate within 1e-6 of an integer) exclude that seed, so the streams use the seeds
# f + 7 * s - 13 = -13 .. 45 (the reflectors are 1.7 - 9.3 m away over that span: inside the filter's depth range)
SEED_OFFSET = -13


def stream_radar(s, f):
    """The radar frames stream ``s`` overlays at step ``f``."""
    return [radar_points(f + 7 * s + SEED_OFFSET)]


def stream_frame(s, dark=None):
    """uint8 ``[h,w,3]`` camera frame of stream ``s``: two sizes alternate; streams 0, 3, 6, .. are bright, the others dark
    (``dark`` overrides)."""
    h, w = FRAME_SIZES[s % 2]
    frame = (synth.uniform(f"multistream/frame{s}", (h, w, 3)) * 255).astype(np.uint8)
    if dark is None:
        dark = s % 3 != 0
    return (frame.astype(np.float32) * 0.1).astype(np.uint8) if dark else frame


def frame_mean(frame, img_size=416):
    """``img.mean()`` of the network input of ``frame`` (ToTensor, pad_to_square, nearest resize), on the host."""
    img, _ = datasets_ref.pad_to_square(datasets_ref.to_tensor(frame), 0)
    return float(datasets_ref.resize(img, img_size).mean())


class HostStream:
    """One stream's host generator; :meth:`step` returns every intermediate of that frame."""

    def __init__(self, **kwargs):
        kwargs.setdefault("min_hits", MIN_HITS)
        self.gen = rp.RadarProposalGenerator(RADAR_CALIB, **kwargs)

    def step(self, radar_frames):
        g = self.gen
        points = np.concatenate([np.asarray(f, dtype=float).reshape(4, -1) for f in radar_frames], 1) \
            if len(radar_frames) else np.zeros((4, 0))
        uv_all, xyzv_all = rp.from_3d_to_2d(points, g.calib_param)
        u_all, v_all = rp.projection_xyr_to_uv([points[0], -points[2], points[1]], g.calib_param)
        keep = rp.fov_velocity_filter(uv_all, xyzv_all, g.max_depth, g.min_velocity, *g.image_size)
        xyzv = xyzv_all[keep]
        clusters, labels = rp.radar_dbscan(xyzv, rp.CLUSTER_DTYPE, g.dbscan_weights, g.dbscan_eps)
        fresh = clusters[clusters["num_points"] >= g.num_pts_filter]
        tracks_before = len(g.tracker.trackers)
        costs, pairs = [], []
        orig_lsa, orig_assoc = rp.linear_sum_assignment, rp.associate_clusters

        def spy_lsa(cost):
            costs.append(np.array(cost, dtype=np.float64))
            return orig_lsa(cost)

        def spy_assoc(old, new):
            out = orig_assoc(old, new)
            pairs.append(out)
            return out

        rp.linear_sum_assignment, rp.associate_clusters = spy_lsa, spy_assoc
        try:
            proposals, cloud = g(radar_frames)
        finally:
            rp.linear_sum_assignment, rp.associate_clusters = orig_lsa, orig_assoc
        unmatched_new = pairs[0][1]
        matches = np.full(tracks_before, -1, np.int32)
        matches[np.asarray(pairs[0][2][0], dtype=np.int64)] = np.asarray(pairs[0][2][1], dtype=np.int32)
        trk = g.tracker
        tracked = [t.cluster.copy() for t in trk.trackers
                   if max(t.hit_streak, t.prev_hit_streak) >= trk.min_hits or trk.frame_count <= trk.min_hits]
        state = [dict(x=t.kf.x.reshape(9).copy(), P=t.kf.P.copy(), cluster=t.cluster.copy(),
                      time_since_update=t.time_since_update, hit_streak=t.hit_streak, prev_hit_streak=t.prev_hit_streak)
                 for t in trk.trackers]
        return dict(u=u_all, v=v_all, xyzv_all=xyzv_all, keep=keep, xyzv=xyzv, cloud=cloud, labels=np.asarray(labels, np.int32),
                    fresh=fresh, cost=costs[0], matches=matches, tracks_before=tracks_before,
                    tracks_peak=tracks_before + len(unmatched_new), tracked=np.array(tracked, dtype=rp.CLUSTER_DTYPE),
                    state=state, frame_count=trk.frame_count, proposals=proposals)


def _update_solve(self, z):
    """``LinearKalmanFilter.update`` with the gain from ``np.linalg.solve`` instead of ``np.linalg.inv``: the same equations,
    an equally valid rounding."""
    z = np.asarray(z, dtype=float).reshape(self.dim_z, 1)
    residual = z - self.H @ self.x
    pht = self.P @ self.H.T
    gain = np.linalg.solve((self.H @ pht + self.R).T, pht.T).T
    self.x = self.x + gain @ residual
    i_kh = np.eye(self.dim_x) - gain @ self.H
    self.P = i_kh @ self.P @ i_kh.T + gain @ self.R @ gain.T


@contextlib.contextmanager
def solve_gain():
    orig = rp.LinearKalmanFilter.update
    rp.LinearKalmanFilter.update = _update_solve
    try:
        yield
    finally:
        rp.LinearKalmanFilter.update = orig


def rel_dev(got, ref):
    """Largest ``|got - ref| / max(1, |ref|)``."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def kalman_runs(streams=STREAMS, frames=FRAMES, radar=None, host=None):
    """The host tracker over the streams of a scene twice - as committed, and with :func:`solve_gain`.  ``radar(s, f)``: the
    scene (default :func:`stream_radar`); ``host()``: builds one stream's :class:`HostStream` (default: its defaults).  Returns
    the records ``[frame][stream]`` of the committed run and the largest deviation (:func:`rel_dev`) of the Kalman state
    ``x`` / ``P`` and of the pixel proposals between the two runs."""
    radar, host = radar or stream_radar, host or HostStream
    runs = []
    for solve in (False, True):
        with (solve_gain() if solve else contextlib.nullcontext()):
            hosts = [host() for _ in range(streams)]
            runs.append([[hosts[s].step(radar(s, f)) for s in range(streams)] for f in range(frames)])
    worst = 0.0
    for step_a, step_b in zip(*runs):
        for a, b in zip(step_a, step_b):
            assert len(a["state"]) == len(b["state"]) and a["proposals"].shape == b["proposals"].shape
            worst = max(worst, rel_dev(b["proposals"], a["proposals"]))
            for ta, tb in zip(a["state"], b["state"]):
                worst = max(worst, rel_dev(tb["x"], ta["x"]), rel_dev(tb["P"], ta["P"]))
    return runs[0], worst


def kalman_deviation(streams=STREAMS, frames=FRAMES, radar=None, host=None):
    """The deviation of :func:`kalman_runs` (by default: over the streams of tests/test_gpu_multistream.py)."""
    return kalman_runs(streams, frames, radar, host)[1]


def kalman_bar(streams=STREAMS, frames=FRAMES, radar=None, host=None):
    """16 x the measured deviation: headroom for fused multiply-add contraction in the host BLAS and another elimination
    order on the device."""
    return 16.0 * kalman_deviation(streams, frames, radar, host)


def rows8(rows7, frame_hw, img_size=416):
    """``[m,7]`` fuser rows in frame pixels -> the ``[m,8]`` layout ``tests.test_gpu_network._cmp_rows_ties`` reads (a zero
    image column in front), with the box scaled back by the frame side to network-input units."""
    rows7 = torch.as_tensor(rows7).clone().reshape(-1, 7)
    rows7[:, :4] *= img_size / float(max(frame_hw))
    return torch.cat([torch.zeros((len(rows7), 1)), rows7], 1)
