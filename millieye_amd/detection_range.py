"""Radar range and radial speed for the detections a fuser returns.

The radar chain proposes boxes and paints the heat map; this module gives its measurements back to the consumer: for every
detection the range and the radial speed of the radar returns that belong to its box - "this person is 6.4 m away and
approaching at 1.1 m/s".  The returns inside a shrunk copy of the box are ordered by range, and the nearest group of at least
``min_points`` returns within ``gate`` metres of its first one is the object that owns the box: what lies behind it is
background, or somebody it occludes.

:func:`range_detections` is the host implementation for one stream and the specification of the device one;
:class:`DeviceDetectionRanges` runs it for S streams in one launch (``me_box_ranges_f64``, csrc/box_ranges.hip) straight on the
output buffer of the stream tail and the kept points of ``radar_proposals.DeviceRadarProposals``.  Everything is float64, every
operation rounded on its own, and the two agree bit for bit.
"""
import numpy as np

MAX_POINTS = 256
ROW_COLS = 4   # range, velocity, points used, points inside
OK, E_INPUT, E_POINTS = 0, 1, 2
DEFAULTS = dict(shrink=0.8, gate=1.0, min_points=2)


def ranging_params(ranging, who):
    """The parameters behind a fuser's ``ranging=`` argument: ``None`` for ``None`` / ``False``, the defaults for ``True``,
    the defaults updated by a dict of ``shrink``, ``gate``, ``min_points``; anything else raises ``hip.MeError``."""
    from . import hip
    if ranging is None or ranging is False:
        return None
    if ranging is not True and not isinstance(ranging, dict):
        raise hip.MeError(f"{who}: ranging must be None, True or a dict of ranging parameters (got {ranging!r})")
    params = dict(DEFAULTS)
    if ranging is not True:
        unknown = sorted(set(ranging) - set(DEFAULTS))
        if unknown:
            raise hip.MeError(f"{who}: unknown ranging parameters {unknown} (known: {sorted(DEFAULTS)})")
        params.update(ranging)
    _check_params(who, **params)
    return params


def _check_params(who, shrink, gate, min_points):
    from . import hip
    if shrink != shrink or gate != gate or int(min_points) != min_points or int(min_points) < 1:
        raise hip.MeError(f"{who}: shrink and gate must not be NaN, min_points must be an integer >= 1 (got shrink={shrink!r}, "
                          f"gate={gate!r}, min_points={min_points!r})")


def range_detections(dets, cloud, shrink=0.8, gate=1.0, min_points=2):
    """``dets`` ``[k, >=4]`` rows with the box ``(x1, y1, x2, y2)`` in columns 0-3, frame pixels (float32 is widened exactly);
    ``cloud`` ``[p, 4]`` float64 kept radar points ``(u, v, range, velocity)`` of the same frame, ``p <= 256``, ranges and
    velocities finite.  Returns ``[k, 4]`` float64 rows ``(range, velocity, c, n)``.

    Per detection, in float64, every operation rounded on its own: ``cx = (x1 + x2) * 0.5``, ``cy`` likewise,
    ``hw = ((x2 - x1) * 0.5) * shrink``, ``hh`` likewise; a point is inside when ``|u - cx| <= hw and |v - cy| <= hh`` (a NaN
    in the box: nothing is inside); the ``n`` inside points are ordered by (range, cloud index); ``c_j`` = the ordered points
    ``i >= j`` with ``r_i <= r_j + gate``; the first ``j`` with ``c_j >= min_points`` gives the front group
    ``j .. j + c_j - 1``, whose ranges and velocities are summed left to right in that order and divided by ``c = c_j``.
    Without such a ``j`` the row is ``(NaN, NaN, 0, n)``.  A point may serve several detections."""
    dets = np.asarray(dets)
    if dets.ndim != 2:
        dets = dets.reshape(-1, 4) if dets.size == 0 else np.atleast_2d(dets)
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 4)
    if dets.ndim != 2 or dets.shape[1] < 4 or len(cloud) > MAX_POINTS:
        from . import hip
        raise hip.MeError(f"range_detections: dets [k, >=4] and at most {MAX_POINTS} points (got {dets.shape}, {cloud.shape})")
    _check_params("range_detections", shrink, gate, min_points)
    box = dets[:, :4].astype(np.float64)
    shrink, gate, min_points = np.float64(shrink), np.float64(gate), int(min_points)
    out = np.zeros((len(box), ROW_COLS))
    out[:, :2] = np.nan
    if not len(box):
        return out
    cx, cy = (box[:, 0] + box[:, 2]) * 0.5, (box[:, 1] + box[:, 3]) * 0.5
    hw, hh = ((box[:, 2] - box[:, 0]) * 0.5) * shrink, ((box[:, 3] - box[:, 1]) * 0.5) * shrink
    with np.errstate(invalid="ignore"):
        inside = (np.abs(cloud[None, :, 0] - cx[:, None]) <= hw[:, None]) & (np.abs(cloud[None, :, 1] - cy[:, None]) <= hh[:, None])
    out[:, 3] = inside.sum(1)
    for k in np.nonzero(out[:, 3] >= min_points)[0]:
        idx = np.nonzero(inside[k])[0]
        order = idx[np.argsort(cloud[idx, 2], kind="stable")]   # by (range, cloud index)
        r, v = cloud[order, 2], cloud[order, 3]
        c = np.searchsorted(r, r + gate, side="right") - np.arange(len(r))   # r ascending: the points from j on up to r_j + gate
        first = np.nonzero(c >= min_points)[0]
        if len(first):
            j = int(first[0])
            n = int(c[j])
            # np.add.accumulate adds one element at a time, left to right
            out[k, 0] = np.add.accumulate(r[j:j + n])[-1] / n
            out[k, 1] = np.add.accumulate(v[j:j + n])[-1] / n
            out[k, 2] = n
    return out


class DeviceDetectionRanges:
    """:func:`range_detections` for ``streams`` independent streams in one launch (``me_box_ranges_f64``): one wave per kept
    row of the output buffer of ``me_stream_tail_f32``, the stream's kept radar points staged in LDS from the buffers of
    ``radar_proposals.DeviceRadarProposals`` (``_cloud_slots`` [S,256,4] float64, ``_counts`` [S,8] int32).  No state, no
    capacity on detections.  A stream whose point count is outside [0, 256] gets ``hip.RANGES_E_POINTS`` and no rows, a flagged
    or inconsistent tail buffer gives every stream ``hip.RANGES_E_INPUT``; ``host_status`` holds the words of the last step."""

    def __init__(self, streams, shrink=0.8, gate=1.0, min_points=2, device=None):
        import ctypes
        import torch
        from . import hip
        self._hip, self._torch, self._ct = hip, torch, ctypes
        self.streams = s = int(streams)
        if s <= 0 or s > 65535:
            raise hip.MeError(f"DeviceDetectionRanges: streams must be in 1 .. 65535 (got {streams})")
        _check_params("DeviceDetectionRanges", shrink, gate, min_points)
        self.device = torch.device(device) if device is not None else hip.default_device()
        self.params = dict(shrink=float(shrink), gate=float(gate), min_points=int(min_points))
        self.shrink, self.gate, self.min_points = self.params["shrink"], self.params["gate"], self.params["min_points"]
        self._ranges = self._status = None   # step()'s own buffers
        self.host_status = np.zeros((s,), np.int32)
        d = self._desc = hip.BoxRangesDesc()
        d.shrink, d.gate, d.streams, d.min_points = self.shrink, self.gate, s, self.min_points

    def launch(self, tail_out, m, cloud_slots, radar_counts, ranges_ptr, status_ptr):
        """The launch without a read-back (asynchronous).  ``tail_out``: the tail's output buffer (a CUDA uint8 tensor or its
        address) for this object's ``streams`` and ``m`` rows; ``cloud_slots`` / ``radar_counts``: the radar chain's device
        tensors (or their addresses); ``ranges_ptr`` / ``status_ptr``: the addresses of ``[m,4]`` float64 and ``[streams]``
        int32 device buffers (``hip.stream_tail_ranges`` has them behind the tail's buffer so that one copy brings everything)."""
        hip, d = self._hip, self._desc

        def ptr(t):
            return t if isinstance(t, int) else t.data_ptr()

        d.tail_out, d.cloud_slots, d.radar_counts = ptr(tail_out), ptr(cloud_slots), ptr(radar_counts)
        d.m = int(m)
        d.ranges, d.status = (ranges_ptr if d.m else None), status_ptr
        with self._torch.cuda.device(self.device):
            hip.check(hip.lib().me_box_ranges_f64(self._ct.byref(d), hip.stream_ptr()), "me_box_ranges_f64")

    def step(self, tail_out, m, cloud_slots, radar_counts):
        """The ranges of every table row of ``tail_out`` (``[m,4]`` float64 numpy, NaN where the tail kept no row) and the
        status word of every stream.  One launch, two small copies."""
        torch, m = self._torch, int(m)
        if self._ranges is None or self._ranges.shape[0] < m:
            self._ranges = torch.empty((max(m, 1), ROW_COLS), dtype=torch.float64, device=self.device)
            self._status = torch.zeros((self.streams,), dtype=torch.int32, device=self.device)
        self._ranges.fill_(float("nan"))
        self.launch(tail_out, m, cloud_slots, radar_counts, self._ranges.data_ptr(), self._status.data_ptr())
        self.host_status = self._status.cpu().numpy()
        return self._ranges[:m].cpu().numpy(), self.host_status.tolist()
