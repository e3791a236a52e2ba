"""Track ids for the detections a fuser returns, one tracker per stream.

The fusers return a fresh list of boxes per step; a consumer wants to know which box of this step is the person of the last
one, most of all in the dark scenes where single-frame detections flicker.  The tracker is SORT-shaped (Bewley et al. 2016,
"Simple online and realtime tracking"): a constant-velocity Kalman filter on ``(cx, cy, w, h)`` per track, association by
IoU solved exactly (``scipy.optimize.linear_sum_assignment``), births from unmatched detections, deaths after ``max_age``
missed steps and the ``min_hits`` rule for what is reported.

:class:`DetectionTracker` is the host implementation for one stream and the specification of the device one;
:class:`DeviceDetectionTracks` runs S of them in one launch (``me_box_tracks_f64``, csrc/box_tracks.hip) straight on the output
buffer of the stream tail.  Everything is float64.
"""
import numpy as np

MAX_DETS = MAX_TRACKS = 64
OK, E_DETS, E_INPUT, E_TRACKS = 0, 1, 2, 3
ROW_COLS = 10   # id, x1, y1, x2, y2, conf, cls, hit_streak, age, det

_F = np.eye(8)
for _c in range(4):
    _F[_c, _c + 4] = 1.0
_H = np.eye(4, 8)
_Q = np.diag([1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.01, 0.01])
_R = np.diag([1.0, 1.0, 10.0, 10.0])
_P0 = np.diag([10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4, 1e4])
_I8 = np.eye(8)


def box_iou(track_x, cls, det):
    """IoU of a track's box ``(cx -+ w/2, cy -+ h/2)`` with a detection row (coordinates widened to float64): plain areas, no
    +1; 0 for an empty intersection and across classes."""
    cx, cy, w, h = (float(v) for v in track_x[:4])
    tx1, ty1, tx2, ty2 = cx - w / 2.0, cy - h / 2.0, cx + w / 2.0, cy + h / 2.0
    dx1, dy1, dx2, dy2 = (float(v) for v in det[:4])
    iw = min(tx2, dx2) - max(tx1, dx1)
    ih = min(ty2, dy2) - max(ty1, dy1)
    if iw <= 0.0 or ih <= 0.0 or float(cls) != float(det[6]):
        return 0.0
    inter = iw * ih
    return inter / (((tx2 - tx1) * (ty2 - ty1) + (dx2 - dx1) * (dy2 - dy1)) - inter)


class _Track:
    __slots__ = ("x", "P", "id", "cls", "conf", "time_since_update", "hits", "hit_streak", "age", "det")

    def __init__(self, z, tid, cls, conf, det):
        self.x = np.concatenate([z, np.zeros(4)])
        self.P = _P0.copy()
        self.id, self.cls, self.conf, self.det = tid, cls, conf, det
        self.time_since_update = self.hits = self.hit_streak = self.age = 0

    def predict(self):
        if self.x[2] + self.x[6] <= 0.0:
            self.x[6] = 0.0
        if self.x[3] + self.x[7] <= 0.0:
            self.x[7] = 0.0
        self.x = _F @ self.x
        self.P = _F @ self.P @ _F.T + _Q
        if self.time_since_update > 0:
            self.hit_streak = 0
        self.time_since_update += 1
        self.age += 1

    def update(self, z, conf, det):
        y = z - _H @ self.x
        S = _H @ self.P @ _H.T + _R
        K = self.P @ _H.T @ np.linalg.inv(S)
        self.x = self.x + K @ y
        A = _I8 - K @ _H
        self.P = A @ self.P @ A.T + K @ _R @ K.T
        self.time_since_update = 0
        self.hits += 1
        self.hit_streak += 1
        self.conf, self.det = conf, det

    def box(self):
        cx, cy, w, h = (float(v) for v in self.x[:4])
        return [cx - w / 2.0, cy - h / 2.0, cx + w / 2.0, cy + h / 2.0]


def _measurement(det):
    x1, y1, x2, y2 = (float(v) for v in det[:4])
    return np.array([(x1 + x2) / 2.0, (y1 + y2) / 2.0, x2 - x1, y2 - y1])


class DetectionTracker:
    """One stream's tracker.  ``step(rows)`` takes the stream's ``[k,7]`` float32 rows ``(x1, y1, x2, y2, conf, cls_score,
    cls_pred)`` of one step (frame pixels, the fuser's order) and returns ``[n,10]`` float64 rows ``(id, x1, y1, x2, y2, conf,
    cls, hit_streak, age, det)``: the tracks that were updated or born in this step and have been updated in ``min_hits``
    consecutive steps (or any, during the first ``min_hits`` steps), in birth order; ``det`` is the row of ``rows`` behind the
    track.  ``self.status`` is ``OK`` or, with the state left exactly as it was and no rows returned, ``E_DETS`` (more than
    64 rows), ``E_INPUT`` (a coordinate that is not finite) or ``E_TRACKS`` (more than 64 tracks).

    The steps, in order: count the frame; predict every track (``x <- F x``, ``P <- F P F' + Q``; a width or height about to
    reach zero stops shrinking); IoU of every predicted box with every detection of its class; ``linear_sum_assignment(-iou)``
    and the ``iou_min`` gate; Joseph-form update of the matched tracks; a new track (``id`` counting up from 1) for every
    unmatched detection with ``conf >= birth_conf``; tracks with ``time_since_update > max_age`` are dropped."""

    def __init__(self, max_age=4, min_hits=3, iou_min=0.3, birth_conf=0.0):
        self.max_age, self.min_hits, self.iou_min, self.birth_conf = int(max_age), int(min_hits), float(iou_min), float(birth_conf)
        self.reset()

    def reset(self):
        self.tracks, self.frame_count, self.next_id, self.status = [], 0, 1, OK
        self.iou = np.zeros((0, 0))
        self.matches = np.zeros((0,), np.int64)

    def step(self, rows):
        from scipy.optimize import linear_sum_assignment
        import copy
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, 7)
        empty = np.zeros((0, ROW_COLS))
        if len(rows) > MAX_DETS:
            self.status = E_DETS
            return empty
        if not np.isfinite(rows[:, :4]).all():
            self.status = E_INPUT
            return empty
        tracks = copy.deepcopy(self.tracks)   # a refused step leaves the state as it was
        for t in tracks:
            t.predict()
        n_t, n_d = len(tracks), len(rows)
        iou = np.zeros((n_t, n_d))
        for i, t in enumerate(tracks):
            for j in range(n_d):
                iou[i, j] = box_iou(t.x, t.cls, rows[j])
        match_t = np.full(n_t, -1, np.int64)
        match_d = np.full(n_d, -1, np.int64)
        if n_t and n_d:
            for i, j in zip(*linear_sum_assignment(-iou)):
                if iou[i, j] >= self.iou_min:
                    match_t[i], match_d[j] = j, i
        births = [j for j in range(n_d) if match_d[j] < 0 and float(rows[j, 4]) >= self.birth_conf]
        if n_t + len(births) > MAX_TRACKS:
            self.status = E_TRACKS
            return empty
        for j in range(n_d):
            if match_d[j] >= 0:
                tracks[match_d[j]].update(_measurement(rows[j]), float(rows[j, 4]), j)
        next_id = self.next_id
        for j in births:
            tracks.append(_Track(_measurement(rows[j]), next_id, float(rows[j, 6]), float(rows[j, 4]), j))
            next_id += 1
        self.frame_count += 1
        self.next_id, self.status, self.iou, self.matches = next_id, OK, iou, match_t
        self.tracks = [t for t in tracks if t.time_since_update <= self.max_age]
        out = [[t.id] + t.box() + [t.conf, t.cls, t.hit_streak, t.age, t.det] for t in self.tracks
               if t.time_since_update == 0 and (t.hit_streak >= self.min_hits or self.frame_count <= self.min_hits)]
        return np.asarray(out, dtype=np.float64).reshape(-1, ROW_COLS)

    def state(self):
        """The live tracks as dicts (the layout of ``DeviceDetectionTracks.track_state``) and the frame count."""
        return [dict(x=t.x.copy(), P=t.P.copy(), id=t.id, cls=t.cls, conf=t.conf, time_since_update=t.time_since_update,
                     hits=t.hits, hit_streak=t.hit_streak, age=t.age, det=t.det) for t in self.tracks], self.frame_count


class DeviceDetectionTracks:
    """:class:`DetectionTracker` for ``streams`` independent streams in one launch (``me_box_tracks_f64``): one workgroup per
    stream reads that stream's kept rows from the output buffer of ``me_stream_tail_f32`` on the device, runs the step above
    with the tracker state in device memory and writes the stream's track rows.  Keyword parameters: ``max_age``,
    ``min_hits``, ``iou_min``, ``birth_conf``.  Capacities per stream: 64 detections, 64 tracks; a stream over one, or with a
    coordinate that is not finite, gets a status (``hip.TRACKS_*``), keeps its state and returns no rows, and the other
    streams are not affected.  ``debug=True`` also keeps the IoU matrix and the matches of every step (:meth:`cost`,
    :meth:`matches`)."""

    def __init__(self, streams, device=None, max_age=4, min_hits=3, iou_min=0.3, birth_conf=0.0, debug=False):
        import ctypes
        import torch
        from . import hip
        self._hip, self._torch, self._ct = hip, torch, ctypes
        self.streams = s = int(streams)
        if s <= 0 or s > 65535:
            raise hip.MeError(f"DeviceDetectionTracks: streams must be in 1 .. 65535 (got {streams})")
        if int(max_age) < 0 or int(min_hits) < 0 or iou_min != iou_min or birth_conf != birth_conf:
            raise hip.MeError("DeviceDetectionTracks: max_age and min_hits must not be negative, iou_min and birth_conf not NaN")
        self.device = dev = torch.device(device) if device is not None else hip.default_device()
        self.params = dict(max_age=int(max_age), min_hits=int(min_hits), iou_min=float(iou_min), birth_conf=float(birth_conf))
        lib = hip.lib()
        T, D = hip.TRACKS_MAX_TRACKS, hip.TRACKS_MAX_DETS
        with torch.cuda.device(dev):
            self._state = torch.zeros((int(lib.me_box_tracks_state_bytes(s)),), dtype=torch.uint8, device=dev)
            self._tracks = torch.zeros((s, T, hip.TRACKS_ROW_COLS), dtype=torch.float64, device=dev)
            self._counts = torch.zeros((s, hip.TRACKS_COUNT_COLS), dtype=torch.int32, device=dev)
            self._cost = torch.zeros((s, T, D), dtype=torch.float64, device=dev) if debug else None
            self._matches = torch.full((s, T), -1, dtype=torch.int32, device=dev) if debug else None
        self.host_counts = np.zeros((s, hip.TRACKS_COUNT_COLS), np.int32)
        d = self._desc = hip.BoxTracksDesc()
        d.state = self._state.data_ptr()
        d.cost = self._cost.data_ptr() if debug else None
        d.matches = self._matches.data_ptr() if debug else None
        d.iou_min, d.birth_conf = self.params["iou_min"], self.params["birth_conf"]
        d.streams, d.max_age, d.min_hits = s, self.params["max_age"], self.params["min_hits"]

    def reset(self, stream=None):
        """Forget the tracks of one stream (or of all of them): its ids start again at 1 and its next step is a first step."""
        hip = self._hip
        which = -1 if stream is None else int(stream)
        if which >= self.streams or (stream is not None and which < 0):
            raise hip.MeError(f"DeviceDetectionTracks.reset: stream {stream} of {self.streams}")
        with self._torch.cuda.device(self.device):
            hip.check(hip.lib().me_box_tracks_reset(self._state.data_ptr(), self.streams, which, hip.stream_ptr()),
                      "me_box_tracks_reset")

    def launch(self, tail_out, m, tracks_ptr=None, counts_ptr=None):
        """The launch of :meth:`step` without its read-back (asynchronous).  ``tail_out``: the tail's output buffer (a CUDA
        uint8 tensor or its address); ``tracks_ptr`` / ``counts_ptr``: other device buffers for the rows and the counts than the
        tracker's own (``hip.stream_tail_tracks`` has them behind the tail's buffer so that one copy brings everything)."""
        hip, d = self._hip, self._desc
        d.tail_out = tail_out if isinstance(tail_out, int) else tail_out.data_ptr()
        d.m = int(m)
        d.tracks = self._tracks.data_ptr() if tracks_ptr is None else tracks_ptr
        d.counts = self._counts.data_ptr() if counts_ptr is None else counts_ptr
        with self._torch.cuda.device(self.device):
            hip.check(hip.lib().me_box_tracks_f64(self._ct.byref(d), hip.stream_ptr()), "me_box_tracks_f64")

    def step(self, tail_out, m):
        """One step of every stream on ``tail_out``, the device output buffer of ``me_stream_tail_f32`` for this tracker's
        ``streams`` and ``m`` input rows.  Returns ``(tracks, status)``: per stream the ``[k,10]`` float64 rows and the status
        word.  One launch, two small copies."""
        self.launch(tail_out, m)
        self.host_counts = counts = self._counts.cpu().numpy()
        table = self._tracks.cpu().numpy()
        return [table[s, :int(counts[s, 1])].copy() for s in range(self.streams)], counts[:, 0].tolist()

    # ---- read-backs of one stream, for tests and debugging -------------------------------------------------------------------
    def tracks(self, stream):
        """The track rows of the last :meth:`step` (not of ``hip.stream_tail_tracks``, which has its own buffer)."""
        return self._tracks[stream, :int(self.host_counts[stream, 1])].cpu().numpy()

    def cost(self, stream, tracks=None, dets=None):
        """The IoU matrix of the last step (``debug=True``): the ``tracks`` tracks the stream had BEFORE the step against its
        ``dets`` detections; only those entries of the ``[64, 64]`` slot are written by a step (default: the whole slot)."""
        c = self._cost[stream].cpu().numpy()
        return c[:c.shape[0] if tracks is None else int(tracks), :c.shape[1] if dets is None else int(dets)]

    def matches(self, stream, tracks=None):
        """For the ``tracks`` tracks the stream had BEFORE the last step: the detection matched to each (-1 = none); only those
        entries of the slot are written by a step (default: the whole slot)."""
        mt = self._matches[stream].cpu().numpy()
        return mt[:len(mt) if tracks is None else int(tracks)]

    def track_state(self, stream):
        """The live tracks of a stream, in order: dicts of ``x`` [8], ``P`` [8,8], ``id``, ``cls``, ``conf``,
        ``time_since_update``, ``hits``, ``hit_streak``, ``age``, ``det``; and ``(frame_count, next_id)``."""
        hip = self._hip
        per = self._state.numel() // self.streams
        raw = self._state[stream * per:(stream + 1) * per].cpu().numpy()
        frame_count, n, given = (int(v) for v in raw[:12].view(np.int32))
        head, size = hip.TRACKS_STATE_HEADER_BYTES, hip.TRACKS_TRACK_BYTES   # (checked against the library at load)
        out = []
        for k in range(n):
            t = raw[head + size * k:head + size * (k + 1)]
            x = t[:64].view(np.float64).copy()
            blocks = t[64:192].view(np.float64).reshape(4, 2, 2)
            P = np.zeros((8, 8))
            for c in range(4):
                P[c, c], P[c, c + 4], P[c + 4, c], P[c + 4, c + 4] = blocks[c].reshape(4)
            ints = t[192:224].view(np.int32)
            flts = t[192:224].view(np.float32)
            out.append(dict(x=x, P=P, id=int(ints[0]), cls=float(flts[1]), conf=float(flts[2]), time_since_update=int(ints[3]),
                            hits=int(ints[4]), hit_streak=int(ints[5]), age=int(ints[6]), det=int(ints[7])))
        return out, (frame_count, given + 1)
