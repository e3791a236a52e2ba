"""An independent sequential painter for millieye_amd/frame_overlay.py (pixel by pixel, item after item, plain Python loops;
it shares the item list and the glyph drawings with the product, not its slicing, clipping or chroma code) and the scenes and
surface helpers of tests/test_frame_overlay_cpu.py and tests/test_gpu_frame_overlay.py."""
import numpy as np

from millieye_amd import frame_overlay as fo

NAN = float("nan")
POISON = 0xA5


# -------------------------------------------------------------------------------------------------- the sequential painter
def _put(frame, fmt, h, x, y, rgb):
    """Pixel (x, y) takes ``rgb``: its own luma / packed bytes, and the chroma sample it owns."""
    col = fo.stored_colour(rgb, fmt)
    if fmt in ("rgb", "bgr"):
        frame[y, x] = col
    elif fmt == "nv12":
        frame[y, x] = col[0]
        if x % 2 == 0 and y % 2 == 0:
            frame[h + y // 2, x], frame[h + y // 2, x + 1] = col[1], col[2]
    else:
        frame[y, x, 0] = col[0]
        if x % 2 == 0:
            frame[y, x, 1], frame[y, x + 1, 1] = col[1], col[2]


def paint_ref(frame, fmt, rows, tracks=None, ranges=None, **style):
    """``draw_detections`` restated: every item visits every pixel of the picture."""
    style = fo.check_style("paint_ref", **style)
    h, w = (frame.shape[0] // 3 * 2, frame.shape[1]) if fmt == "nv12" else frame.shape[:2]
    items, drawn = fo.build_items(rows, tracks, ranges, **style)
    if drawn > fo.MAX_BOXES:
        return fo.E_BOXES
    t, s = style["thickness"], style["font_scale"]
    for item in items:
        for y in range(h):
            for x in range(w):
                if item[0] == "box":
                    _, x1, y1, x2, y2, rgb = item
                    if x1 <= x <= x2 and y1 <= y <= y2 and not (x1 + t <= x <= x2 - t and y1 + t <= y <= y2 - t):
                        _put(frame, fmt, h, x, y, rgb)
                else:
                    _, x0, y0, text, rgb = item
                    lx, ly = x - x0, y - y0
                    if 0 <= lx < 6 * s * len(text) and 0 <= ly < 8 * s:
                        art = fo._GLYPH_ART[text[lx // (6 * s)]]
                        px, py = lx % (6 * s) // s, ly // s
                        ink = 1 <= px <= 5 and 1 <= py <= 7 and art[py - 1][px - 1] == "#"
                        _put(frame, fmt, h, x, y, fo.text_colour(rgb) if ink else rgb)
    return fo.OK


# ---------------------------------------------------------------------------------------------------------------- scenes
def rows_of(boxes, conf=None, cls=None):
    """``[k,7]`` float32 detection rows for ``boxes`` [k,4]."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    k = len(boxes)
    rows = np.zeros((k, 7), np.float32)
    rows[:, :4] = boxes
    rows[:, 4] = 0.95 - 0.01 * np.arange(k) if conf is None else conf
    rows[:, 5] = 0.9
    rows[:, 6] = np.arange(k) if cls is None else cls
    return rows


def tracks_of(pairs):
    """``[t,10]`` float64 track rows from ``(id, det)`` pairs."""
    out = np.zeros((len(pairs), 10))
    for n, (tid, det) in enumerate(pairs):
        out[n, 0], out[n, 9] = tid, det
    return out


def ranges_of(values):
    out = np.zeros((len(values), 4))
    out[:, 0] = values
    return out


def random_scene(seed, h, w, k=None):
    """``(rows, tracks, ranges)``: ``k`` (default 1 .. 12) boxes that overlap heavily, cross every edge or lie outside, with
    half-pixel corners, some tracked, some ranged, one of them with a NaN coordinate when there are at least four."""
    rng = np.random.default_rng(9000 + seed)
    k = int(rng.integers(1, 13)) if k is None else k
    cx, cy = rng.uniform(-0.2 * w, 1.2 * w, k), rng.uniform(-0.2 * h, 1.2 * h, k)
    bw, bh = rng.uniform(1, 0.7 * w, k), rng.uniform(1, 0.7 * h, k)
    boxes = np.round(np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1) * 2) / 2   # corners on x.0 and x.5
    rows = rows_of(boxes, conf=rng.uniform(0, 1, k).astype(np.float32), cls=rng.integers(0, 14, k))
    if k >= 4:
        rows[2, int(rng.integers(0, 4))] = NAN
    tracked = [i for i in range(k) if rng.random() < 0.6]
    tracks = tracks_of([(int(rng.integers(1, 5000)), i) for i in tracked] + [(77, -1)])
    ranges = ranges_of(np.where(rng.random(k) < 0.3, NAN, rng.uniform(0, 60, k)))
    return rows, tracks[rng.permutation(len(tracks))], ranges


# -------------------------------------------------------------------------------------------------------------- surfaces
def poisoned(nbytes, seed=0):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def place(layout, fmt, h, w, offset, pad=0, uv_gap=0, uv_pad=None):
    """Adds the picture to ``layout`` (a list) and returns the first free byte behind it: rows ``pad`` bytes longer than the
    picture's, NV12's chroma plane ``uv_gap`` bytes behind the luma plane with rows ``uv_pad`` bytes longer."""
    bpp = {"rgb": 3, "bgr": 3, "yuyv": 2, "nv12": 1}[fmt]
    pitch = bpp * w + pad
    end = offset + h * pitch
    entry = dict(fmt=fmt, h=h, w=w, offset=offset, pitch=pitch, uv_offset=None, uv_pitch=None)
    if fmt == "nv12":
        entry["uv_offset"] = end + uv_gap
        entry["uv_pitch"] = w + (pad if uv_pad is None else uv_pad)
        end = entry["uv_offset"] + (h // 2) * entry["uv_pitch"]
    layout.append(entry)
    return end


def surface_on(buffer, e):
    """The ``FrameSurface`` of a layout entry on ``buffer`` (a 1-D uint8 torch tensor on any device)."""
    from millieye_amd.utils.datasets import FrameSurface
    return FrameSurface(buffer, e["h"], e["w"], e["fmt"], e["offset"], e["pitch"], e["uv_offset"], e["uv_pitch"])


def view_of(buf, e):
    """The picture of a layout entry as writable numpy views into ``buf`` (1-D uint8): the ``[h,w,c]`` view, or for NV12 the
    pair (Y ``[h,w]``, UV ``[h/2,w]``)."""
    h, w = e["h"], e["w"]
    if e["fmt"] == "nv12":
        return (np.ndarray((h, w), np.uint8, buffer=buf, offset=e["offset"], strides=(e["pitch"], 1)),
                np.ndarray((h // 2, w), np.uint8, buffer=buf, offset=e["uv_offset"], strides=(e["uv_pitch"], 1)))
    c = 2 if e["fmt"] == "yuyv" else 3
    return np.ndarray((h, w, c), np.uint8, buffer=buf, offset=e["offset"], strides=(e["pitch"], c, 1))


def dense_of(buf, e):
    """A dense copy of the picture in the layout ``draw_detections`` takes."""
    v = view_of(buf, e)
    return np.concatenate([v[0], v[1]], 0) if e["fmt"] == "nv12" else v.copy()


def store(buf, e, dense):
    """Writes a dense picture back over its bytes in ``buf`` - and over nothing else."""
    v = view_of(buf, e)
    if e["fmt"] == "nv12":
        v[0][...] = dense[:e["h"]]
        v[1][...] = dense[e["h"]:]
    else:
        v[...] = dense


def expected_buffer(buf, layout, scenes, **style):
    """``buf`` after ``draw_detections`` of ``scenes[i] = (rows, tracks, ranges)`` on the picture of ``layout[i]``; returns
    ``(buffer, status per picture)``.  Every byte outside the pictures is the input's."""
    out = buf.copy()
    status = []
    for e, (rows, tracks, ranges) in zip(layout, scenes):
        dense = dense_of(buf, e)
        status.append(fo.draw_detections(dense, e["fmt"], rows, tracks, ranges, **style))
        store(out, e, dense)
    return out, status


def tracks_buffers(per_stream, status=None):
    """``tracks [S,64,10]`` float64 (NaN behind every stream's rows) and ``counts [S,4]`` int32 = (status, rows, -77, -77) as
    ``me_box_tracks_f64`` leaves them."""
    S = len(per_stream)
    table = np.full((S, 64, 10), NAN)
    counts = np.full((S, 4), -77, np.int32)
    for s, t in enumerate(per_stream):
        t = np.zeros((0, 10)) if t is None else np.asarray(t, dtype=np.float64).reshape(-1, 10)
        table[s, :len(t)] = t
        counts[s, 0], counts[s, 1] = 0 if status is None else status[s], len(t)
    return table, counts


def ranges_buffer(per_stream_rows, per_stream_ranges, gaps=None):
    """``ranges [m,4]`` float64 indexed like the tail's table (NaN in the rows the tail did not keep)."""
    gaps = [0] * len(per_stream_rows) if gaps is None else gaps
    blocks = []
    for rows, ranges, gap in zip(per_stream_rows, per_stream_ranges, gaps):
        block = np.full((len(rows) + gap, 4), NAN)
        if ranges is not None and len(rows):
            block[:len(rows)] = np.asarray(ranges, dtype=np.float64).reshape(-1, 4)
        blocks.append(block)
    return np.concatenate(blocks, 0) if blocks else np.zeros((0, 4))
