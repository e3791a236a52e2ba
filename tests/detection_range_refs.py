"""An independent restatement of millieye_amd/detection_range.py:range_detections (plain Python loops over Python floats,
``sorted`` with a tuple key; no code shared with the product) and the scenes of tests/test_detection_range_cpu.py and
tests/test_gpu_detection_range.py.

A scene is ``(dets [k,7] float32, cloud [p,4] float64, params)``: detection rows ``(x1, y1, x2, y2, conf, cls_score, cls)``
with every coordinate a float32 value, kept radar points ``(u, v, range, velocity)`` and the keyword parameters of
``range_detections``."""
import math

import numpy as np

NAN = float("nan")
BIG = float(2 ** 53)   # 1 + BIG == BIG, but (1 - BIG) + BIG == 1: a sum that shows its order


def range_rows_ref(dets, cloud, shrink=0.8, gate=1.0, min_points=2):
    """Section 1 of the specification, row by row."""
    points = [tuple(float(x) for x in p) for p in np.asarray(cloud, dtype=np.float64).reshape(-1, 4)]
    rows = []
    for d in np.asarray(dets).reshape(-1, np.asarray(dets).shape[-1] if np.asarray(dets).ndim > 1 else 4):
        x1, y1, x2, y2 = (float(v) for v in d[:4])
        cx = (x1 + x2) * 0.5
        cy = (y1 + y2) * 0.5
        hw = ((x2 - x1) * 0.5) * shrink
        hh = ((y2 - y1) * 0.5) * shrink
        inside = [(p[2], i) for i, p in enumerate(points) if abs(p[0] - cx) <= hw and abs(p[1] - cy) <= hh]
        ordered = sorted(inside, key=lambda t: (t[0], t[1]))
        n = len(ordered)
        row = [NAN, NAN, 0.0, float(n)]
        for j in range(n):
            limit = ordered[j][0] + gate
            c = sum(1 for i in range(j, n) if ordered[i][0] <= limit)
            if c >= min_points:
                sum_r, sum_v = ordered[j][0], points[ordered[j][1]][3]
                for i in range(j + 1, j + c):
                    sum_r = sum_r + ordered[i][0]
                    sum_v = sum_v + points[ordered[i][1]][3]
                row = [sum_r / c, sum_v / c, float(c), float(n)]
                break
        rows.append(row)
    return np.array(rows, dtype=np.float64).reshape(-1, 4)


def same(a, b):
    """Bit-equal apart from the payload of a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ----------------------------------------------------------------------------------------------------------- the scenes
def dets_of(boxes):
    """``[k,7]`` float32 rows for ``boxes`` [k,4]: falling confidences, every row a class of its own (a second NMS keeps all)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    k = len(boxes)
    rows = np.zeros((k, 7), np.float32)
    rows[:, :4] = boxes
    rows[:, 4] = 0.95 - 0.005 * np.arange(k)
    rows[:, 5] = 0.9
    rows[:, 6] = np.arange(k)
    return rows


def cloud_of(points):
    return np.asarray(points, dtype=np.float64).reshape(-1, 4)


def edge_scenes():
    """name -> scene; every case of the issue's list but the random ones."""
    up, down = (lambda x: float(np.nextafter(x, math.inf))), (lambda x: float(np.nextafter(x, -math.inf)))
    scenes = {}
    people = [(100, 100, 160, 260), (300, 120, 380, 300), (500, 90, 560, 250)]
    scenes["empty_cloud"] = (dets_of(people), cloud_of([]), {})
    scenes["no_detections"] = (dets_of([]), cloud_of([(130, 180, 5.0, 0.5), (131, 181, 5.2, 0.4)]), {})
    # box (10, 20, 50, 60), shrink 0.5: cx = 30, cy = 40, hw = hh = 10, all exact
    edge = [(20, 40, 5.0, 1.0), (40, 40, 5.1, 1.0), (30, 30, 5.2, 1.0), (30, 50, 5.3, 1.0), (20, 30, 5.4, 1.0), (40, 50, 5.5, 1.0),
            (down(20.0), 40, 5.0, 9.0), (up(40.0), 40, 5.0, 9.0), (30, down(30.0), 5.0, 9.0), (30, up(50.0), 5.0, 9.0)]
    scenes["on_the_shrunk_edge"] = (dets_of([(10, 20, 50, 60)]), cloud_of(edge), dict(shrink=0.5))
    # ordered: index 1 (range 4), then the tie at range 5 in cloud order: index 0 (-BIG), index 2 (+BIG)
    scenes["equal_ranges"] = (dets_of([people[0]]), cloud_of([(130, 180, 5.0, -BIG), (131, 181, 4.0, 1.0), (129, 179, 5.0, BIG)]),
                              dict(gate=2.0))
    scenes["gate_inclusive"] = (dets_of([people[0]]), cloud_of([(130, 180, 5.0, 0.5), (131, 181, 4.0, 0.25), (129, 179, up(5.0), 8.0)]),
                                {})
    scenes["lone_first_point"] = (dets_of([people[0]]), cloud_of([(130, 180, 6.5, 0.3), (131, 181, 2.0, 7.0), (129, 179, 6.0, 0.1),
                                                                 (128, 178, 6.3, 0.2)]), {})
    scenes["no_group"] = (dets_of([people[0]]), cloud_of([(130, 180, 2.0, 0.3), (131, 181, 4.0, 0.2), (129, 179, 6.0, 0.1)]), {})
    overlap = [(100, 100, 200, 300), (150, 100, 250, 300)]
    shared = [(175, 200, 4.0, 0.5), (176, 210, 4.2, 0.6), (120, 200, 3.0, -0.5), (121, 190, 3.1, -0.4), (230, 200, 7.0, 1.5),
              (231, 190, 7.5, 1.25)]
    scenes["overlapping_boxes"] = (dets_of(overlap), cloud_of(shared), dict(gate=0.5))
    nan_box = dets_of([people[0], people[0], people[1]])
    nan_box[1, 0] = NAN
    scenes["nan_coordinate"] = (nan_box, cloud_of([(130, 180, 5.0, 0.5), (131, 181, 5.2, 0.4), (340, 200, 3.0, 0.1),
                                                   (341, 201, 3.5, 0.2)]), {})
    scenes["shrink_one"] = (dets_of([(10, 20, 50, 60)]), cloud_of([(10, 20, 5.0, 1.0), (50, 60, 5.5, 2.0), (up(50.0), 60, 5.2, 9.0),
                                                                   (10, down(20.0), 5.2, 9.0)]), dict(shrink=1.0))
    rng = np.random.default_rng(256)
    full = np.stack([rng.uniform(210, 290, 256), rng.uniform(110, 290, 256), np.round(rng.uniform(2.0, 9.0, 256), 1),
                     rng.normal(0.0, 1.0, 256)], 1)   # ranges on a 0.1 m grid: many ties
    scenes["all_256_inside"] = (dets_of([(150, 50, 350, 350)]), cloud_of(full), dict(gate=0.35, min_points=9))
    return scenes


def random_scene(seed):
    """2 - 40 detections by 2 - 256 points in a 640 x 480 frame: people with a cluster of returns on them, background returns
    behind and between them; the first box always holds a close pair of returns and the last lies right of every return.  (One
    detection or fewer than two points cannot hold a ranged and an unranged detection; those counts have cases of their own.)"""
    rng = np.random.default_rng(7000 + seed)
    k, p = int(rng.integers(2, 41)), int(rng.integers(2, 257))
    boxes = []
    for _ in range(k - 1):
        w = rng.uniform(30, 90)
        h = w * rng.uniform(1.5, 2.6)
        cx, cy = rng.uniform(50, 540), rng.uniform(120, 360)
        boxes.append((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2))
    boxes.append((600, 100, 638, 300))
    boxes = np.asarray(boxes, dtype=np.float32)
    points = []
    bx = boxes[0].astype(np.float64)
    centre = ((bx[0] + bx[2]) / 2, (bx[1] + bx[3]) / 2)
    points += [(centre[0], centre[1], 4.0, 0.5), (centre[0] + 1, centre[1] - 1, 4.25, 0.75)]
    while len(points) < p:
        if rng.random() < 0.6:   # a return on somebody
            b = boxes[int(rng.integers(0, k - 1))].astype(np.float64)
            depth = 2.0 + 7.0 * ((b[0] * 0.37) % 1.0)
            points.append((rng.uniform(b[0], b[2]), rng.uniform(b[1], b[3]), depth + rng.normal(0, 0.3), rng.normal(0.8, 0.2)))
        else:
            points.append((rng.uniform(0, 590), rng.uniform(0, 480), rng.uniform(0.5, 10.0), rng.normal(0, 0.1)))
    points = np.asarray(points[:p], dtype=np.float64)
    return dets_of(boxes), cloud_of(points[rng.permutation(len(points))]), {}


RANDOM_SEEDS = tuple(range(12))


# --------------------------------------------------------------------------------------- device inputs of synthetic scenes
def network_rows(per_stream_dets):
    """The ``[m,8]`` float32 rows ``(stream, x1, y1, x2, y2, p, cls_score, cls)`` of ``Network.forward`` that carry the
    detections of every stream, streams interleaved; with :func:`identity_scalars` the tail returns the boxes as they are."""
    rows = [np.concatenate([np.full((len(d), 1), s, np.float32), d], 1) for s, d in enumerate(per_stream_dets)]
    rows = np.concatenate(rows, 0).astype(np.float32).reshape(-1, 8)
    return rows[np.random.default_rng(len(rows)).permutation(len(rows))]


def identity_scalars(streams):
    """``(a, b, c)`` for x and y with ``((v - a) / b) * c == v``."""
    return np.tile(np.array([0, 1, 1, 0, 1, 1], np.float32), (streams, 1))


def radar_buffers(clouds, counts=None):
    """``cloud_slots [S,256,4]`` float64 (NaN behind every stream's points) and ``radar_counts [S,8]`` int32 (column 1 = the
    points, -77 elsewhere) as the radar chain keeps them.  ``counts`` overrides column 1."""
    S = len(clouds)
    slots = np.full((S, 256, 4), NAN)
    words = np.full((S, 8), -77, np.int32)
    for s, c in enumerate(clouds):
        slots[s, :len(c)] = c
        words[s, 1] = len(c) if counts is None else counts[s]
    return slots, words
