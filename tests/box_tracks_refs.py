"""References and scenes for the per-stream detection tracker (millieye_amd/detection_tracks.py, csrc/box_tracks.hip;
tests/test_box_tracks_cpu.py and tests/test_gpu_box_tracks.py).

``RefTracker`` restates the tracker's step in float64 without looking at ``DetectionTracker``: dict tracks, general 8 x 8
matrices and ``scipy.optimize.linear_sum_assignment`` (``kalman="general"``), or the same decisions with the Kalman filter
written as four independent (coordinate, velocity) filters in plain Python floats (``kalman="decoupled"``) - the order of
operations the kernel follows.  The deviation between the two is the scale that reordering the filter's arithmetic may
legitimately cost; the GPU test's bar is 16 x what ``reorder_deviation`` measures on its own scenes.
"""
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

MAX_DETS = MAX_TRACKS = 64
OK, E_DETS, E_INPUT, E_TRACKS = 0, 1, 2, 3

F = np.eye(8)
F[0, 4] = F[1, 5] = F[2, 6] = F[3, 7] = 1.0
H = np.zeros((4, 8))
H[0, 0] = H[1, 1] = H[2, 2] = H[3, 3] = 1.0
Q = np.diag([1, 1, 1, 1, .01, .01, .01, .01]).astype(np.float64)
R = np.diag([1.0, 1.0, 10.0, 10.0])
P_BIRTH = np.diag([10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4, 1e4])
R_DIAG = (1.0, 1.0, 10.0, 10.0)


def iou_ref(x, cls, det):
    """The IoU of section 3, operation for operation: the predicted box (cx -+ w/2, cy -+ h/2) against detection ``det``
    (float32 widened to float64); plain areas; 0 where iw <= 0 or ih <= 0 or the classes differ."""
    cx, cy, w, h = float(x[0]), float(x[1]), float(x[2]), float(x[3])
    tx1 = cx - w / 2.0
    ty1 = cy - h / 2.0
    tx2 = cx + w / 2.0
    ty2 = cy + h / 2.0
    dx1, dy1, dx2, dy2 = float(det[0]), float(det[1]), float(det[2]), float(det[3])
    ix1 = tx1 if tx1 > dx1 else dx1
    iy1 = ty1 if ty1 > dy1 else dy1
    ix2 = tx2 if tx2 < dx2 else dx2
    iy2 = ty2 if ty2 < dy2 else dy2
    iw = ix2 - ix1
    ih = iy2 - iy1
    if iw <= 0.0 or ih <= 0.0 or float(cls) != float(det[6]):
        return 0.0
    inter = iw * ih
    area_t = (tx2 - tx1) * (ty2 - ty1)
    area_d = (dx2 - dx1) * (dy2 - dy1)
    return inter / ((area_t + area_d) - inter)


# ---------------------------------------------------------------------------------------- the two Kalman filters
def predict_general(t):
    t["x"] = F @ t["x"]
    t["P"] = F @ t["P"] @ F.T + Q


def update_general(t, z):
    x, P = t["x"], t["P"]
    y = z - H @ x
    S = H @ P @ H.T + R
    K = P @ H.T @ np.linalg.inv(S)
    t["x"] = x + K @ y
    A = np.eye(8) - K @ H
    t["P"] = A @ P @ A.T + K @ R @ K.T


def predict_decoupled(t):
    x, P = t["x"], t["P"]
    for c in range(4):
        pos, vel = float(x[c]), float(x[c + 4])
        a, b, cc, d = float(P[c, c]), float(P[c, c + 4]), float(P[c + 4, c]), float(P[c + 4, c + 4])
        x[c] = pos + vel
        fa = a + cc
        fb = b + d
        P[c, c] = (fa + fb) + 1.0
        P[c, c + 4] = fb
        P[c + 4, c] = cc + d
        P[c + 4, c + 4] = d + 0.01


def update_decoupled(t, z):
    x, P = t["x"], t["P"]
    for c in range(4):
        rn = R_DIAG[c]
        pos, vel = float(x[c]), float(x[c + 4])
        a, b, cc, d = float(P[c, c]), float(P[c, c + 4]), float(P[c + 4, c]), float(P[c + 4, c + 4])
        y = float(z[c]) - pos
        s = a + rn
        k0 = a / s
        k1 = cc / s
        x[c] = pos + k0 * y
        x[c + 4] = vel + k1 * y
        a00 = 1.0 - k0
        a10 = -k1
        m00 = a00 * a
        m01 = a00 * b
        m10 = a10 * a + cc
        m11 = a10 * b + d
        P[c, c] = m00 * a00 + (k0 * rn) * k0
        P[c, c + 4] = (m00 * a10 + m01) + (k0 * rn) * k1
        P[c + 4, c] = m10 * a00 + (k1 * rn) * k0
        P[c + 4, c + 4] = (m10 * a10 + m11) + (k1 * rn) * k1


KALMAN = {"general": (predict_general, update_general), "decoupled": (predict_decoupled, update_decoupled)}


# ---------------------------------------------------------------------------------------------------- the tracker
class RefTracker:
    """The float64 reference of one stream.  ``step(rows)`` returns a record: ``rows`` [n,10], ``status``, ``iou`` [T,D] (the
    tracks before the step against the detections), ``matches`` [T], ``tracks_before``, ``dets``."""

    def __init__(self, max_age=4, min_hits=3, iou_min=0.3, birth_conf=0.0, kalman="general"):
        self.max_age, self.min_hits, self.iou_min, self.birth_conf = max_age, min_hits, iou_min, birth_conf
        self.predict, self.update = KALMAN[kalman]
        self.tracks, self.frame_count, self.next_id = [], 0, 1

    def _refuse(self, status, n_d):
        return dict(rows=np.zeros((0, 10)), status=status, iou=np.zeros((0, 0)), matches=np.zeros((0,), np.int64),
                    tracks_before=len(self.tracks), dets=n_d)

    def step(self, rows):
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, 7)
        n_d = rows.shape[0]
        if n_d > MAX_DETS:
            return self._refuse(E_DETS, n_d)
        if not all(math.isfinite(float(v)) for v in rows[:, :4].reshape(-1)):
            return self._refuse(E_INPUT, n_d)
        # work on a copy: a status leaves the stream as it was
        trk = [dict(t, x=t["x"].copy(), P=t["P"].copy()) for t in self.tracks]
        frame_count = self.frame_count + 1
        for t in trk:
            if t["x"][2] + t["x"][6] <= 0:
                t["x"][6] = 0.0
            if t["x"][3] + t["x"][7] <= 0:
                t["x"][7] = 0.0
            self.predict(t)
            if t["time_since_update"] > 0:
                t["hit_streak"] = 0
            t["time_since_update"] += 1
            t["age"] += 1
        n_t = len(trk)
        iou = np.zeros((n_t, n_d), dtype=np.float64)
        for i in range(n_t):
            for j in range(n_d):
                iou[i, j] = iou_ref(trk[i]["x"], trk[i]["cls"], rows[j])
        det_of = np.full(n_t, -1, dtype=np.int64)
        trk_of = np.full(n_d, -1, dtype=np.int64)
        if n_t > 0 and n_d > 0:
            ri, ci = linear_sum_assignment(-iou)
            for i, j in zip(ri, ci):
                if not iou[i, j] < self.iou_min:
                    det_of[i] = j
                    trk_of[j] = i
        new = [j for j in range(n_d) if trk_of[j] < 0 and float(rows[j, 4]) >= self.birth_conf]
        if n_t + len(new) > MAX_TRACKS:
            return self._refuse(E_TRACKS, n_d)
        for j in range(n_d):
            i = trk_of[j]
            if i < 0:
                continue
            r = [float(v) for v in rows[j, :4]]
            z = np.array([(r[0] + r[2]) / 2.0, (r[1] + r[3]) / 2.0, r[2] - r[0], r[3] - r[1]])
            self.update(trk[i], z)
            trk[i].update(time_since_update=0, hits=trk[i]["hits"] + 1, hit_streak=trk[i]["hit_streak"] + 1,
                          conf=float(rows[j, 4]), det=j)
        for j in new:
            r = [float(v) for v in rows[j, :4]]
            x = np.array([(r[0] + r[2]) / 2.0, (r[1] + r[3]) / 2.0, r[2] - r[0], r[3] - r[1], 0.0, 0.0, 0.0, 0.0])
            trk.append(dict(x=x, P=P_BIRTH.copy(), id=self.next_id, cls=float(rows[j, 6]), conf=float(rows[j, 4]),
                            time_since_update=0, hits=0, hit_streak=0, age=0, det=j))
            self.next_id += 1
        self.frame_count = frame_count
        self.tracks = [t for t in trk if not t["time_since_update"] > self.max_age]
        out = []
        for t in self.tracks:
            if t["time_since_update"] == 0 and (t["hit_streak"] >= self.min_hits or frame_count <= self.min_hits):
                cx, cy, w, h = (float(v) for v in t["x"][:4])
                out.append([t["id"], cx - w / 2.0, cy - h / 2.0, cx + w / 2.0, cy + h / 2.0, t["conf"], t["cls"],
                            t["hit_streak"], t["age"], t["det"]])
        return dict(rows=np.array(out, dtype=np.float64).reshape(-1, 10), status=OK, iou=iou, matches=det_of,
                    tracks_before=n_t, dets=n_d)

    def state(self):
        return [dict(t, x=t["x"].copy(), P=t["P"].copy()) for t in self.tracks], self.frame_count


# ---------------------------------------------------------------------------------------------- the input checks
def gate_distance(rec, iou_min):
    """The smallest |iou - iou_min| over the pairs the assignment chose (inf without pairs)."""
    iou = rec["iou"]
    if iou.size == 0:
        return math.inf
    ri, ci = linear_sum_assignment(-iou)
    return min((abs(float(iou[i, j]) - iou_min) for i, j in zip(ri, ci)), default=math.inf)


def decision_margin(iou, iou_min):
    """How much total IoU the best assignment loses when one of its pairs that pass the gate is forbidden (the idea of
    ``radar_scene_helpers.assignment_margin``; pairs under the gate are no decisions - all-zero rows tie freely and are dropped
    anyway).  0 means a second optimum with other matches exists; inf: no gated pair."""
    iou = np.asarray(iou, dtype=np.float64)
    if iou.size == 0:
        return math.inf
    ri, ci = linear_sum_assignment(-iou)
    total = float(iou[ri, ci].sum())
    margin = math.inf
    for i, j in zip(ri, ci):
        if iou[i, j] < iou_min:
            continue
        other = iou.copy()
        other[i, j] = -1e6
        r2, c2 = linear_sum_assignment(-other)
        margin = min(margin, total - float(other[r2, c2].sum()))
    return margin


def state_deviation(a, b):
    """Largest absolute difference of x and P between two track lists with the same tracks."""
    worst = 0.0
    for ta, tb in zip(a, b):
        worst = max(worst, float(np.abs(ta["x"] - tb["x"]).max()), float(np.abs(ta["P"] - tb["P"]).max()))
    return worst


def reorder_deviation(scenes, **params):
    """Run the general and the decoupled reference over ``scenes`` (lists of per-step rows): assert that they agree on every
    decision and return the largest deviation of (boxes, state) between them."""
    worst_box = worst_state = 0.0
    for steps in scenes:
        g, d = RefTracker(kalman="general", **params), RefTracker(kalman="decoupled", **params)
        for rows in steps:
            rg, rd = g.step(rows), d.step(rows)
            assert rg["status"] == rd["status"] and rg["rows"].shape == rd["rows"].shape
            assert np.array_equal(rg["matches"], rd["matches"])
            if len(rg["rows"]):
                assert np.array_equal(rg["rows"][:, [0, 5, 6, 7, 8, 9]], rd["rows"][:, [0, 5, 6, 7, 8, 9]])
                worst_box = max(worst_box, float(np.abs(rg["rows"][:, 1:5] - rd["rows"][:, 1:5]).max()))
            sg, sd = g.state()[0], d.state()[0]
            assert [t["id"] for t in sg] == [t["id"] for t in sd]
            worst_state = max(worst_state, state_deviation(sg, sd))
    return worst_box, worst_state


# ------------------------------------------------------------------------------------------------------ the scenes
def scene(seed, steps=40, people=4, false_rate=0.4, miss=0.15, frame=(640, 480)):
    """``steps`` lists of float32 rows [k,7]: people of two classes walking with constant velocity plus jitter, 15 % missed
    detections, people who arrive and leave, false positives, rows shuffled.  ``people = 0``: always empty."""
    rng = np.random.default_rng(1000 + seed)
    W, Hh = frame
    persons = []

    def person(born):
        w = rng.uniform(30, 70)
        h = w * rng.uniform(1.8, 2.6)
        return dict(c=np.array([rng.uniform(60, W - 60), rng.uniform(120, Hh - 120)]), v=rng.uniform(-5, 5, 2),
                    size=np.array([w, h]), cls=float(rng.integers(0, 2)), born=born, dies=born + int(rng.integers(8, steps + 8)))

    for _ in range(people):
        persons.append(person(0 if rng.random() < 0.7 else int(rng.integers(1, steps // 2))))
    out = []
    for f in range(steps):
        if people and rng.random() < 0.08:
            persons.append(person(f))
        rows = []
        for p in persons:
            if not p["born"] <= f < p["dies"]:
                continue
            c = p["c"] + p["v"] * (f - p["born"]) + rng.normal(0, 1.5, 2)
            sz = p["size"] * (1 + rng.normal(0, 0.02, 2))
            if rng.random() < miss:
                continue
            rows.append([c[0] - sz[0] / 2, c[1] - sz[1] / 2, c[0] + sz[0] / 2, c[1] + sz[1] / 2, rng.uniform(0.3, 0.95),
                         rng.uniform(0.5, 1.0), p["cls"]])
        for _ in range(int(rng.poisson(false_rate)) if people else 0):
            c = np.array([rng.uniform(0, W), rng.uniform(0, Hh)])
            sz = rng.uniform(15, 90, 2)
            rows.append([c[0] - sz[0] / 2, c[1] - sz[1] / 2, c[0] + sz[0] / 2, c[1] + sz[1] / 2, rng.uniform(0.05, 0.5),
                         rng.uniform(0.5, 1.0), float(rng.integers(0, 2))])
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, 7)
        out.append(rows[rng.permutation(len(rows))])
    return out


def grid_rows(n, seed, spacing=40.0, size=60.0, jitter=0.0, cls=0.0, origin=(100.0, 100.0), shuffle=True):
    """``n`` boxes of ``size`` on an 8-wide grid with ``spacing`` (neighbours overlap when spacing < size), jittered, shuffled."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        cx, cy = origin[0] + spacing * (k % 8), origin[1] + spacing * (k // 8)
        cx, cy = cx + rng.normal(0, jitter), cy + rng.normal(0, jitter)
        rows.append([cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2, rng.uniform(0.3, 0.9), 0.9, cls])
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 7)
    return rows[rng.permutation(n)] if shuffle else rows


def tail_buffer(per_stream, gaps=None, status=0):
    """The output buffer of ``me_stream_tail_f32`` as bytes, for the kept rows ``per_stream`` (list of [k,7] float32):
    int32 words [status | rows per stream | kept rows per stream | padding to 4 words], then the float32 [m,7] table in which
    stream s's kept rows start behind the rows of the streams before it.  ``gaps[s]``: rows stream s had that were not kept;
    their table rows are filled with NaN, like anything a tracker must not read.  Returns ``(uint8 array, m)``."""
    S = len(per_stream)
    gaps = [0] * S if gaps is None else list(gaps)
    kept = [len(r) for r in per_stream]
    rows_in = [k + g for k, g in zip(kept, gaps)]
    m = int(sum(rows_in))
    head = (1 + 2 * S + 3) & ~3
    ints = np.zeros(head, np.int32)
    ints[0] = status
    ints[1:1 + S] = rows_in
    ints[1 + S:1 + 2 * S] = kept
    table = np.full((m, 7), np.nan, np.float32)
    start = 0
    for s in range(S):
        if kept[s]:
            table[start:start + kept[s]] = np.asarray(per_stream[s], np.float32).reshape(-1, 7)
        start += rows_in[s]
    return np.concatenate([ints.view(np.uint8), table.reshape(-1).view(np.uint8)]), m
