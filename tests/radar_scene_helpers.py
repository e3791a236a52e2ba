"""Seeded radar scenes that drive the device proposal chain (csrc/radar.hip) to its capacities and edges - 256 kept points,
32 clusters, 32 tracks per stream - and the conditions under which an exact comparison with the host
``RadarProposalGenerator`` means something.  tests/test_radar_scenes_cpu.py guards every scene; tests/test_gpu_radar_chain.py
runs them on the device.  Everything here is host work: no GPU, and the HIP library is not loaded.

A scene function returns the list of ``[4, k]`` radar frames (x right, y depth, z up, radial velocity) a stream overlays at
one step.  All scenes keep the demo's calibration (``RADAR_CALIB``); the generator parameters a family needs beside the
defaults are in ``*_KW``."""
import math

import numpy as np

from tests import multistream_helpers as mh
from tests.golden.make_golden import radar_points

MAXP, MAXC, MAXT = 256, 32, 32     # the library's capacities (millieye_amd.hip.RADAR_MAX_*; the CPU test compares them)
MIN_HITS = mh.MIN_HITS

# ------------------------------------------------------------------------------------------------------ capacity grid
GRID_RINGS, GRID_LATERAL, GRID_POINTS = 8, (-0.42, -0.14, 0.14, 0.42), 8
GRID_FRAMES = 12
GRID_DROPPED, GRID_DROP_FROM, GRID_READD, GRID_READD_FROM = (3, 4, 10, 31), 3, 10, 9
GRID_SEED = 0


def grid_centres(frame):
    """``[32, 4]`` (x, y, z, v) of the grid's reflectors at ``frame``: 8 range rings from 3.0 m in steps of 0.85 m, 4 lateral
    positions each, scaled with the range; every reflector drifts slowly and has its own height and velocity."""
    out = []
    for ring in range(GRID_RINGS):
        for k, lat in enumerate(GRID_LATERAL):
            c = ring * len(GRID_LATERAL) + k
            rng_ = 3.0 + 0.85 * ring + 0.012 * frame * (1 if c % 2 else -1)
            x = lat * rng_ + 0.01 * frame * (1 if c % 3 else -1)
            z = 0.15 * ((c * 7) % 5 - 2) / 2.0
            v = (0.5 + 0.11 * (c % 7)) * (1 if c % 2 else -1)
            out.append((x, rng_, z, v))
    return np.array(out)


def grid_frame(frame, drop=(), points=GRID_POINTS, seed=GRID_SEED, extra_cluster=False, extra_point=False):
    """One radar frame of the grid: ``points`` per reflector with jitter sigma 0.05 m (0.02 m/s), the reflectors in ``drop``
    left out.  ``extra_cluster`` adds a 33rd reflector (reflector 0 again, 5 m/s faster: its own component through the velocity
    axis); ``extra_point`` adds one isolated point that passes the filter."""
    cols = []
    centres = grid_centres(frame)
    for c, (x, y, z, v) in enumerate(centres):
        rng = np.random.RandomState(100000 * seed + 1000 * frame + c)   # (a reflector's points do not depend on `drop`)
        jitter = rng.randn(4, GRID_POINTS)[:, :points] * np.array([[0.05], [0.05], [0.05], [0.02]])
        if c not in drop:
            cols.append(np.array([[x], [y], [z], [v]]) + jitter)
    if extra_cluster:
        x, y, z, v = centres[0]
        rng = np.random.RandomState(100000 * seed + 1000 * frame + 900)
        cols.append(np.array([[x], [y], [z], [v + 5.0]]) + rng.randn(4, points) * np.array([[0.05], [0.05], [0.05], [0.02]]))
    if extra_point:
        cols.append(np.array([[0.3], [5.2], [0.4], [9.0]]))
    return np.concatenate(cols, 1)


def grid_radar(s, f):
    """The capacity-grid family, stream ``s`` at step ``f``.  Stream 0: all 32 reflectors, every frame (256 kept points,
    32 clusters, 32 tracks).  Stream 1: reflectors {3, 4, 10, 31} vanish from frame 3 on - their tracks coast and die together
    at frame 7 out of the middle and the end of the list - and reflector 10 returns at frame 9: a new track behind the compacted
    list.  Stream 2: as stream 1 with another seed and 7 points per reflector."""
    if s == 0:
        return [grid_frame(f)]
    drop = ()
    if f >= GRID_DROP_FROM:
        drop = tuple(c for c in GRID_DROPPED if not (c == GRID_READD and f >= GRID_READD_FROM))
    return [grid_frame(f, drop, seed=GRID_SEED + (s - 1), points=GRID_POINTS if s == 1 else GRID_POINTS - 1)]


GRID_STREAMS = 3

# ------------------------------------------------------------------------------------------------------------- chains
CHAIN_STEP = 1.4      # along the velocity axis (weight 1, no upper bound in the filter): neighbours 1.4 apart, next ones 2.8
CHAIN_ORDERS = ("index", "reverse", "shuffle", "interleaved")


def chain_frame(order, n=MAXP, seed=3):
    """``n`` points at one place whose velocities step by 1.4: with ``eps`` 1.5 one component, a chain as long as the point
    list.  ``order``: the position of chain link k in the point list - "index" (k), "reverse", "shuffle" (a fixed permutation),
    or "interleaved": two chains of n / 2 links on the even and the odd indices, 2 m apart in range."""
    rng = np.random.RandomState(seed)
    pts = np.array([[0.35], [4.1], [0.12], [0.0]]) + rng.randn(4, n) * np.array([[0.02], [0.02], [0.02], [0.0]])
    if order == "interleaved":
        link = np.arange(n) // 2
        pts[1, 1::2] += 2.0
    else:
        link = {"index": np.arange(n), "reverse": np.arange(n)[::-1], "shuffle": np.random.RandomState(seed + 1).permutation(n)}[order]
    pts[3] = 0.7 + CHAIN_STEP * link
    return pts


def chain_radar(s, f=0):
    return [chain_frame(CHAIN_ORDERS[s])]


# ------------------------------------------------------------------------------------------------------ mean velocity
MEANV_SIZES = (127, 128, 129, 136, 200, 255, 256)
MEANV_KW = dict(dbscan_weights=(2, 1, 3, 0))   # the velocity does not separate the points: one blob, one cluster
MEANV_SEED = 1


def cancelling_velocities(n, seed=MEANV_SEED):
    """n / 4 values 2^20 .. 2^40, their negatives and n - 2 (n / 4) values in 0.2 .. 1.5, shuffled: the large terms cancel, and
    what is left of the small ones depends on the order of the additions - numpy's pairwise order, the sequential one and the
    exact sum all round to different float32 means."""
    rng = np.random.RandomState(1000 * seed + n)
    big = 2.0 ** rng.uniform(20.0, 40.0, n // 4)
    vals = np.concatenate([big, -big, rng.uniform(0.2, 1.5, n - 2 * (n // 4))])
    return vals[rng.permutation(n)]


def meanv_frame(n, seed=MEANV_SEED):
    rng = np.random.RandomState(2000 * seed + n)
    pts = np.array([[-0.4], [3.7], [0.05], [0.0]]) + rng.randn(4, n) * np.array([[0.08], [0.08], [0.08], [0.0]])
    pts[3] = cancelling_velocities(n, seed)
    return pts


def meanv_radar(s, f=0):
    return [meanv_frame(MEANV_SIZES[s])]


def _leaf(a):
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res += v
        return res
    r = [a[j] for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] += a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res += a[i]
        i += 1
    return res


def pairwise_sum(a):
    """numpy's pairwise summation of a 1-D float64 reduction in plain Python: at most 128 elements in eight interleaved
    accumulators, longer runs split in halves at a multiple of eight."""
    a = [float(v) for v in a]
    if len(a) <= 128:
        return _leaf(a)
    n2 = len(a) // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def mean_variants(vel):
    """float32 means of ``vel`` by numpy, the plain-Python pairwise rule, one 128-element leaf rule applied to the whole run
    ("one level"), the sequential sum and the exact sum."""
    vel = np.asarray(vel, dtype=np.float64)
    n = len(vel)
    seq = 0.0
    for v in vel:
        seq += float(v)
    f32 = np.float32
    return dict(numpy=f32(np.mean(vel)), pairwise=f32(pairwise_sum(vel) / n), one_level=f32(_leaf([float(v) for v in vel]) / n),
                sequential=f32(seq / n), exact=f32(math.fsum(vel) / n))


# -------------------------------------------------------------------------------------------------------- filter edge
EDGE_PASS, EDGE_FAIL = 32, 20


def edge_frame(num_pts_filter=5, seed=5):
    """Components of ``num_pts_filter`` and ``num_pts_filter - 1`` points alternate (pass, fail, pass, ..: 20 pairs, then 12
    more that pass), 3 m/s apart along the velocity axis and each at its own place: exactly 32 clusters pass the
    ``num_pts_filter`` beside 20 that fail, and the 32 keep their order."""
    rng = np.random.RandomState(seed)
    sizes = []
    for k in range(EDGE_FAIL):
        sizes += [num_pts_filter, num_pts_filter - 1]
    sizes += [num_pts_filter] * (EDGE_PASS - EDGE_FAIL)
    cols = []
    for k, m in enumerate(sizes):
        centre = np.array([[-1.0 + 0.04 * k], [3.5 + 0.03 * k], [0.1 - 0.005 * k], [0.6 + 3.0 * k]])
        cols.append(centre + rng.randn(4, m) * np.array([[0.04], [0.04], [0.04], [0.02]]))
    return np.concatenate(cols, 1)


def pairs_frame(seed=6):
    """128 two-point components 3 m/s apart: with ``num_pts_filter`` 2 every one is a cluster - 128 of them."""
    rng = np.random.RandomState(seed)
    cols = [np.array([[0.2], [4.4], [-0.1], [0.6 + 3.0 * k]]) + rng.randn(4, 2) * np.array([[0.04], [0.04], [0.04], [0.02]])
            for k in range(MAXP // 2)]
    return np.concatenate(cols, 1)


# ----------------------------------------------------------------------------------------------------------- statuses
def huge_velocity_frame():
    """A frame whose velocities are 1e21: its clusters' ``avgV`` makes every later association cost overflow float32."""
    full = grid_frame(0)
    pts = np.concatenate([full[:, GRID_POINTS * c:GRID_POINTS * (c + 1)] for c in (0, 2, 13, 27)], 1)   # four well-separated reflectors
    pts[3] = 1e21
    return pts


# ------------------------------------------------------------------------------------------------------- many streams
MANY_STREAMS, MANY_FRAMES = 300, 3
_SEEDS = 59   # radar_points(-13 .. 45): the seeds tests/test_radar_device_fixture_cpu.py has cleared (46 is not)


def filtered_frame(s, f):
    """Points that all fail the filter: static, too far, or outside the field of view."""
    rng = np.random.RandomState(7000 + 10 * s + f)
    static = np.stack([rng.uniform(-1, 1, 5), rng.uniform(3, 8, 5), rng.uniform(-0.5, 0.5, 5), rng.uniform(-0.05, 0.05, 5)])
    far = np.stack([rng.uniform(-1, 1, 4), rng.uniform(11, 15, 4), rng.uniform(-0.5, 0.5, 4), rng.uniform(0.5, 2, 4)])
    depth = rng.uniform(2, 6, 3)
    side = np.stack([rng.uniform(0.9, 1.2, 3) * depth, depth, rng.uniform(-0.5, 0.5, 3), rng.uniform(0.5, 2, 3)])
    return np.concatenate([static, far, side], 1)


def many_radar(s, f):
    """Stream ``s`` of the 300: s % 5 == 0 has no radar frame at all, s % 5 == 1 only points the filter drops, the others
    overlay 1, 2 or 3 of the synthetic frames."""
    kind = s % 5
    if kind == 0:
        return []
    if kind == 1:
        return [filtered_frame(s, f)]
    return [radar_points((f + 7 * s + 23 * j) % _SEEDS + mh.SEED_OFFSET) for j in range(kind - 1)]


# ------------------------------------------------------------------------------------------------ proposals and boxes
BOXES_KW = dict(max_size=0.16)
BOXES_FRAME_HW = ((240, 320), (320, 240), (256, 256))   # landscape, portrait, square: smaller than the 640 x 480 field of view
BOXES_FRAMES = 4


def boxes_radar(s, f):
    return [grid_frame(f, seed=20 + s)]


# ---------------------------------------------------------------------------------------------------------------- tie
TIE_STREAMS = 3


def _cube(x, y, z, v):
    """Eight points on the corners of a cube of side 1/8 around camera-frame (x, y, z): dyadic, so the mean is exact."""
    d = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64).T / 16.0
    cam = np.array([[x], [y], [z]]) + d
    return np.stack([cam[0], cam[2], -cam[1], np.full(8, v)])   # radar (x, y = range, z = -camera y, v)


def tie_radar(s, f):
    """Two frames whose second association has an exact tie between two optimal assignments.  Frame 0 founds the tracks; they
    still hold frame 0's clusters, exactly, when frame 1 is associated.  Tracks A / B sit at x = -1 / +1, clusters C / D at
    y = -1 / +1 on the axis between them: every cost of {A, B} x {C, D} is the same float32 number.
    Stream 0: A, B against C, D (square).  Stream 1: A, B against C alone (more tracks than clusters).  Stream 2: a track at
    the origin against clusters at x = -1 / +1 (more clusters than tracks).  A far reflector E, matched without doubt, rides
    along."""
    v, z = 0.5, 4.0
    far = _cube(0.5, 0.25, 7.0, v)
    if s == 2:
        first, second = [_cube(0.0, 0.0, z, v)], [_cube(-1.0, 0.0, z, v), _cube(1.0, 0.0, z, v)]
    else:
        first = [_cube(-1.0, 0.0, z, v), _cube(1.0, 0.0, z, v)]
        second = [_cube(0.0, -1.0, z, v), _cube(0.0, 1.0, z, v)][:2 if s == 0 else 1]
    return [np.concatenate((first if f == 0 else second) + [far], 1)]


# ---------------------------------------------------------------------------------------------------- the input checks
def assignment_margin(cost):
    """How much the best complete assignment of ``cost`` loses when one of its pairs is forbidden: solve, then for every matched
    pair in turn add a large finite constant to that entry and solve again; the smallest increase of the total.  Zero means a
    second optimum exists; brute force over the permutations is out of reach at 32 x 32.  Returns ``(margin, total)``."""
    from scipy.optimize import linear_sum_assignment
    cost = np.asarray(cost, dtype=np.float64)
    rows, cols = linear_sum_assignment(cost)
    total = float(cost[rows, cols].sum())
    big = 1e6 * (1.0 + float(np.abs(cost).max()))
    margin = math.inf
    for i, j in zip(rows, cols):
        other = cost.copy()
        other[i, j] += big
        r2, c2 = linear_sum_assignment(other)
        margin = min(margin, float(other[r2, c2].sum()) - total)
    return margin, total


def check_step(r, gen, eps_margin=1e-9, tie=False):
    """The conditions of tests/test_radar_device_fixture_cpu.py on one host record ``r`` (``HostStream.step``) of generator
    ``gen``: no decision on a rounding boundary.  Returns the assignment margin relative to the total (None: no association)."""
    weights, eps = np.array(gen.dbscan_weights, dtype=float), gen.dbscan_eps
    if len(r["u"]):
        for name in ("u", "v"):
            val = r[name]
            assert np.isfinite(val).all()
            assert np.abs(val - np.rint(val)).min() > 1e-6, f"a projected {name} lies within 1e-6 of an integer"
        assert np.abs(r["xyzv_all"][:, 2] - gen.max_depth).min() > 1e-6
        assert np.abs(np.abs(r["xyzv_all"][:, 3]) - gen.min_velocity).min() > 1e-6
    if len(r["xyzv"]) > 1:
        x = r["xyzv"] * weights
        dist = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
        assert np.abs(dist - eps).min() > eps_margin, "a pairwise weighted distance lies within the margin of eps"
    cost = r["cost"]
    if cost.size and max(cost.shape) > 1:
        margin, total = assignment_margin(cost)
        if not tie:
            assert margin > 1e-6 * total, f"assignment margin {margin} of {total}"
        return margin / total if total else math.inf
    return None


def host_kw(**kw):
    """A builder of host streams with other generator parameters, for :func:`kalman_runs`."""
    return lambda: mh.HostStream(**kw)


def kalman_runs(radar, streams, frames, host=mh.HostStream):
    """:func:`tests.multistream_helpers.kalman_runs` of the scene function ``radar(s, f)``: the host records
    ``[frame][stream]`` and the deviation between the host tracker's two roundings (gain through the inverse / solved for)."""
    return mh.kalman_runs(streams, frames, radar=radar, host=host)


def kalman_deviation(radar, streams, frames, host=mh.HostStream):
    return mh.kalman_deviation(streams, frames, radar=radar, host=host)


def kalman_bar(radar, streams, frames, host=mh.HostStream):
    """16 x the deviation, as in :func:`tests.multistream_helpers.kalman_bar`."""
    return mh.kalman_bar(streams, frames, radar=radar, host=host)


MANY_BAR_STREAMS = 60   # the bar of the 300 streams is measured on the first 60: the largest of fewer, never a wider bar


def grid_runs():
    """The capacity-grid family - the grid streams over their 12 frames and the proposals-versus-boxes streams (grid frames of
    other seeds, another ``max_size``) over their 4: ``(grid records, boxes records, deviation)``.  One bar for the family;
    the single-frame families (chains, mean velocity, filter edge) and the status sequences (grid frames) take it too, and so
    does a family whose own two host runs agree bit for bit (deviation 0: the tie scenes, with one Kalman update each)."""
    grid, dev_a = kalman_runs(grid_radar, GRID_STREAMS, GRID_FRAMES)
    boxes, dev_b = kalman_runs(boxes_radar, len(BOXES_FRAME_HW), BOXES_FRAMES, host_kw(**BOXES_KW))
    return grid, boxes, max(dev_a, dev_b)
