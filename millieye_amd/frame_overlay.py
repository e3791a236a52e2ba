"""Boxes and labels drawn onto the frames a fuser was given - what the reference's demos do with a result
(``cv2.rectangle`` + ``cv2.putText`` per kept detection) for frames in their native pixel format, where they lie.

:func:`draw_detections` is the host implementation for one frame (plain numpy, what ``FrameFuser(overlay=)`` runs) and the
specification of the device one; :class:`DeviceFrameOverlay` paints the pictures of S streams in one launch
(``me_frame_overlay_u8``, csrc/frame_overlay.hip) straight from the output buffer of the stream tail, the tracker's rows and the
ranger's rows.  The two agree bit for bit.

Items.  Detection row ``i`` is ``(x1, y1, x2, y2, conf, cls_conf, cls)``.  With ``k = int(cls)`` (truncated), row ``i`` is DRAWN
when its four coordinates are finite, ``cls`` is finite with ``|cls| < 2^31``, and the ``classes`` filter is ``None`` or
contains ``k``.  A drawn row gives one box item and, with ``labels=True``, one label item; painter's order is row 0's box, row
0's label, row 1's box, ...  Every pixel ends with the colour of the last item that covers it.  More than
:data:`MAX_BOXES` (64) drawn rows: nothing is drawn and the status is :data:`E_BOXES`.

Box.  The corners are ``rint`` (half to even) of the float32 coordinates, then limited to ``+-(2^30 + 1024)`` (no pixel of a
picture of up to 2^30 pixels a side can tell).  A row with ``x2 < x1`` or ``y2 < y1`` after rounding gives no item at all, box
or label (it still counts as drawn).  The outline covers the pixels of ``[x1, x2] x [y1, y2]`` (inclusive) that are not in
``[x1 + t, x2 - t] x [y1 + t, y2 - t]``, ``t = thickness`` (1 .. 8, default 2): a box with ``x2 - x1 < 2 t`` or
``y2 - y1 < 2 t`` is filled.  Everything is clipped to the picture.

Colour.  ``palette[k mod len(palette)]`` (the non-negative remainder) with ``color_by="class"``; with ``color_by="track"`` and
a track id behind the row ``palette[id mod len(palette)]``.  The palette is a tuple of RGB triples.  ``rgb`` stores the triple,
``bgr`` stores it reversed, ``nv12`` / ``yuyv`` store its integer limited-range BT.601 transform (``>>`` arithmetic)::

    Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16
    U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128
    V = ((112 R - 94 G - 18 B + 128) >> 8) + 128

Subsampled chroma.  A luma byte belongs to its own pixel.  The NV12 chroma pair ``(cx, cy)`` is written when pixel
``(2 cx, 2 cy)`` is covered and takes the chroma of that pixel's last item; a YUYV pair's ``U, V`` follow its even pixel the
same way.  So every byte has one possible writer, and bytes of uncovered pixels are never written.

Label.  Up to three parts joined by one space: ``#<id>`` when ``tracks`` has a row with ``det == i`` (the first such row; its
id, truncated, must lie in ``[0, 2^31 - 1]``, else there is no id part and no track colour); the confidence as ``d.dd`` from
``q = clamp(floor(conf * 100 + 0.5), 0, 100)`` (a NaN gives 0); ``<r>m`` when ``ranges[i, 0]`` is finite and
``0 <= d <= 9999`` for ``d = floor(range * 10 + 0.5)``, printed as ``d // 10``, a point and ``d % 10``.  All float64, every
operation rounded on its own.  The glyphs ``0-9 . # m`` and space are 5 x 7 bitmaps (:data:`GLYPH_ROWS`) at columns 1 .. 5,
rows 1 .. 7 of a 6 x 8 cell, replicated ``font_scale`` (1 .. 4, default 1) times.  The plate is a filled rectangle in the
box's colour, ``6 s n`` wide and ``8 s`` high for ``n`` characters, its left edge at ``x1``, its rows ``[y1 - 8 s, y1 - 1]``:
it stands on the box's top edge.  If ``y1 - 8 s < 0`` its rows are ``[y1, y1 + 8 s - 1]`` instead.  The glyph pixels are black
when the RGB colour's ``(299 R + 587 G + 114 B) // 1000 >= 128``, else white.  The plate is clipped to the picture.
"""
import math

import numpy as np

MAX_BOXES = 64
MAX_CHARS = 24            # '#' + 10 digits, ' ', 'd.dd', ' ', 'ddd.dm'
COORD_LIMIT = (1 << 30) + 1024
CELL_W, CELL_H = 6, 8
OK, E_BOXES, E_INPUT, E_SURFACE = 0, 1, 2, 3
GLYPHS = "0123456789.#m "
DEFAULT_PALETTE = ((255, 255, 0), (0, 255, 0), (255, 0, 0), (0, 128, 255), (255, 0, 255), (0, 255, 255), (255, 128, 0),
                   (128, 0, 255), (255, 255, 255), (0, 0, 160))
DEFAULTS = dict(thickness=2, font_scale=1, labels=True, color_by="class", classes=None, palette=DEFAULT_PALETTE)
FORMATS = ("rgb", "bgr", "nv12", "yuyv")   # in the order of utils.datasets.PIXEL_FORMATS

_GLYPH_ART = {
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    "3": ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    "6": ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    "7": ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
    ".": (".....", ".....", ".....", ".....", ".....", ".##..", ".##.."),
    "#": (".#.#.", ".#.#.", "#####", ".#.#.", "#####", ".#.#.", ".#.#."),
    "m": (".....", ".....", "##.#.", "#.#.#", "#.#.#", "#.#.#", "#.#.#"),
    " ": (".....",) * 7,
}
# [14, 8] uint8: glyph g's row r (0 .. 6; row 7 is zero) with column c in bit 4 - c - the table the kernel is handed
GLYPH_ROWS = np.array([[sum(1 << (4 - c) for c in range(5) if row[c] == "#") for row in _GLYPH_ART[ch]] + [0] for ch in GLYPHS],
                      dtype=np.uint8)


def overlay_params(overlay, who):
    """The style behind a fuser's ``overlay=`` argument: ``None`` for ``None`` / ``False``, the defaults for ``True``, the
    defaults updated by a dict of style parameters; anything else raises ``hip.MeError``."""
    from . import hip
    if overlay is None or overlay is False:
        return None
    if overlay is not True and not isinstance(overlay, dict):
        raise hip.MeError(f"{who}: overlay must be None, True or a dict of style parameters (got {overlay!r})")
    params = dict(DEFAULTS)
    if overlay is not True:
        unknown = sorted(set(overlay) - set(DEFAULTS))
        if unknown:
            raise hip.MeError(f"{who}: unknown overlay parameters {unknown} (known: {sorted(DEFAULTS)})")
        params.update(overlay)
    return check_style(who, **params)


def check_style(who, thickness=2, font_scale=1, labels=True, color_by="class", classes=None, palette=DEFAULT_PALETTE):
    """The checked style as a dict (``palette`` a tuple of int triples, ``classes`` ``None`` or a sorted tuple of ints)."""
    from . import hip

    def whole(v, lo, hi):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= v <= hi

    if not whole(thickness, 1, 8):
        raise hip.MeError(f"{who}: thickness must be an integer in 1 .. 8 (got {thickness!r})")
    if not whole(font_scale, 1, 4):
        raise hip.MeError(f"{who}: font_scale must be an integer in 1 .. 4 (got {font_scale!r})")
    if color_by not in ("class", "track"):
        raise hip.MeError(f"{who}: color_by must be 'class' or 'track' (got {color_by!r})")
    try:
        pal = tuple(tuple(int(c) for c in entry) for entry in palette)
        ok = 1 <= len(pal) <= 256 and all(len(e) == 3 and all(0 <= c <= 255 for c in e) for e in pal) \
            and all(int(c) == c for entry in palette for c in entry)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise hip.MeError(f"{who}: palette must hold 1 .. 256 RGB triples of integers in 0 .. 255 (got {palette!r})")
    if classes is not None:
        try:
            cls = tuple(sorted({int(c) for c in classes}))
            ok = len(cls) <= 64 and all(int(c) == c for c in classes) and all(-2 ** 31 < c < 2 ** 31 for c in cls)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise hip.MeError(f"{who}: classes must be None or at most 64 integer class ids (got {classes!r})")
        classes = cls
    return dict(thickness=int(thickness), font_scale=int(font_scale), labels=bool(labels), color_by=color_by, classes=classes,
                palette=pal)


def rgb_to_yuv(rgb):
    """The integer limited-range BT.601 forward transform of an RGB triple (the counterpart of the input kernels' inverse)."""
    r, g, b = (int(c) for c in rgb)
    return (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128,
            ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128)


def stored_colour(rgb, pixel_format):
    """The three bytes ``pixel_format`` stores for an RGB triple: ``rgb`` as it is, ``bgr`` reversed, ``nv12`` / ``yuyv`` (Y, U, V)."""
    rgb = tuple(int(c) for c in rgb)
    return rgb if pixel_format == "rgb" else rgb[::-1] if pixel_format == "bgr" else rgb_to_yuv(rgb)


def text_colour(rgb):
    """Black on a light plate, white on a dark one."""
    r, g, b = (int(c) for c in rgb)
    return (0, 0, 0) if (299 * r + 587 * g + 114 * b) // 1000 >= 128 else (255, 255, 255)


def palette_table(palette):
    """``[4, len(palette), 3]`` uint8: the palette in the stored byte order of every format (:data:`FORMATS`)."""
    return np.array([[stored_colour(c, fmt) for c in palette] for fmt in FORMATS], dtype=np.uint8).reshape(4, len(palette), 3)


def track_id(i, tracks):
    """The id of the first row of ``tracks`` ``[t,10]`` with ``det == i`` (column 9), truncated; ``None`` without such a row or
    with an id outside ``[0, 2^31 - 1]``."""
    if tracks is None:
        return None
    for t in np.asarray(tracks, dtype=np.float64).reshape(-1, 10):
        if t[9] == i:
            return int(t[0]) if 0 <= t[0] <= 2147483647 else None
    return None


def label_text(conf, tid=None, range_m=None):
    """The label of a row: ``[#<id> ]d.dd[ <r>m]`` (module docstring).  float64, one rounding per operation, no float formatting."""
    v = float(np.float64(conf)) * 100.0 + 0.5
    q = 100 if v >= 100.0 else int(math.floor(v)) if v >= 0.0 else 0   # (a NaN fails both comparisons)
    text = f"{q // 100}.{q // 10 % 10}{q % 10}"
    if tid is not None:
        text = f"#{int(tid)} " + text
    if range_m is not None:
        r = float(np.float64(range_m))
        if math.isfinite(r):
            v = r * 10.0 + 0.5
            if 0.0 <= v < 10000.0:   # 0 <= floor(v) <= 9999
                d = int(math.floor(v))
                text += f" {d // 10}.{d % 10}m"
    return text


def text_mask(text, font_scale=1):
    """bool ``[8 s, 6 s n]``: the glyph pixels of ``text`` on its plate."""
    cells = np.zeros((CELL_H, CELL_W * len(text)), dtype=bool)
    for n, ch in enumerate(text):
        rows = GLYPH_ROWS[GLYPHS.index(ch)]
        for r in range(7):
            for c in range(5):
                cells[1 + r, CELL_W * n + 1 + c] = bool((int(rows[r]) >> (4 - c)) & 1)
    return np.kron(cells, np.ones((font_scale, font_scale), dtype=bool))


def build_items(rows, tracks=None, ranges=None, thickness=2, font_scale=1, labels=True, color_by="class", classes=None,
                palette=DEFAULT_PALETTE):
    """``(items, drawn)``: the items of a frame in painter's order and the number of drawn rows.  A box item is
    ``("box", x1, y1, x2, y2, rgb)``, a label item ``("label", x0, y0, text, rgb)`` with the plate's top-left corner."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 7)
    ranges = None if ranges is None else np.asarray(ranges, dtype=np.float64).reshape(-1, 4)
    items, drawn = [], 0
    for i, row in enumerate(rows):
        if not np.isfinite(row[:4]).all() or not np.isfinite(row[6]) or not abs(float(row[6])) < 2.0 ** 31:
            continue
        k = int(row[6])
        if classes is not None and k not in classes:
            continue
        drawn += 1
        x1, y1, x2, y2 = (int(min(max(float(np.rint(np.float64(v))), -COORD_LIMIT), COORD_LIMIT)) for v in row[:4])
        if x2 < x1 or y2 < y1:
            continue
        tid = track_id(i, tracks)
        rgb = palette[(tid if color_by == "track" and tid is not None else k) % len(palette)]
        items.append(("box", x1, y1, x2, y2, rgb))
        if labels:
            text = label_text(row[4], tid, None if ranges is None or i >= len(ranges) else ranges[i, 0])
            top = y1 - CELL_H * font_scale
            items.append(("label", x1, top if top >= 0 else y1, text, rgb))
    return items, drawn


def _paint(frame, pixel_format, h, w, x0, y0, sel, rgb):
    """``sel`` bool ``[hh, ww]`` for the pixels from ``(x0, y0)`` on, all inside the picture: the selected ones take ``rgb``."""
    hh, ww = sel.shape
    col = stored_colour(rgb, pixel_format)
    if pixel_format in ("rgb", "bgr"):
        frame[y0:y0 + hh, x0:x0 + ww][sel] = col
        return
    ys, xs = y0 + (y0 & 1), x0 + (x0 & 1)   # the first even row / column of the region
    if pixel_format == "nv12":
        frame[y0:y0 + hh, x0:x0 + ww][sel] = col[0]
        sub = sel[ys - y0::2, xs - x0::2]   # the region's pixels (even x, even y): they own their chroma pair
        uv = frame[h:]
        uv[ys // 2:ys // 2 + sub.shape[0], xs:xs + 2 * sub.shape[1]:2][sub] = col[1]
        uv[ys // 2:ys // 2 + sub.shape[0], xs + 1:xs + 1 + 2 * sub.shape[1]:2][sub] = col[2]
    else:   # yuyv: Y0 U Y1 V
        frame[y0:y0 + hh, x0:x0 + ww, 0][sel] = col[0]
        sub = sel[:, xs - x0::2]
        frame[y0:y0 + hh, xs:xs + 2 * sub.shape[1]:2, 1][sub] = col[1]
        frame[y0:y0 + hh, xs + 1:xs + 1 + 2 * sub.shape[1]:2, 1][sub] = col[2]


def _clip(x0, y0, x1, y1, h, w):
    return max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)


def draw_detections(frame, pixel_format, rows, tracks=None, ranges=None, **style):
    """Draws the detections ``rows`` ``[k,7]`` into ``frame``, a writable numpy uint8 array (or a strided view) in the native
    layout of ``pixel_format`` - ``[h,w,3]`` for ``rgb`` / ``bgr``, ``[h*3//2, w]`` for ``nv12``, ``[h,w,2]`` for ``yuyv`` - by
    the rules of the module docstring, one item after the other.  ``tracks`` ``[t,10]`` and ``ranges`` ``[k,4]`` are a
    fuser's ``info["tracks"]`` / ``info["ranges"]``; ``style``: ``thickness``, ``font_scale``, ``labels``, ``color_by``,
    ``classes``, ``palette``.  Returns :data:`OK`, or :data:`E_BOXES` (nothing drawn) for more than 64 drawn rows."""
    from .utils.datasets import picture_hw
    style = check_style("draw_detections", **style)
    if not isinstance(frame, np.ndarray):
        from . import hip
        raise hip.MeError(f"draw_detections: frame must be a numpy uint8 array (got {type(frame).__name__})")
    h, w = picture_hw(frame, pixel_format, "draw_detections")
    items, drawn = build_items(rows, tracks, ranges, **style)
    if drawn > MAX_BOXES:
        return E_BOXES
    t, s = style["thickness"], style["font_scale"]
    for item in items:
        if item[0] == "box":
            _, x1, y1, x2, y2, rgb = item
            cx0, cy0, cx1, cy1 = _clip(x1, y1, x2, y2, h, w)
            if cx0 > cx1 or cy0 > cy1:
                continue
            sel = np.ones((cy1 - cy0 + 1, cx1 - cx0 + 1), dtype=bool)
            hx0, hy0, hx1, hy1 = _clip(x1 + t, y1 + t, x2 - t, y2 - t, h, w)
            if hx0 <= hx1 and hy0 <= hy1:
                sel[hy0 - cy0:hy1 - cy0 + 1, hx0 - cx0:hx1 - cx0 + 1] = False
            _paint(frame, pixel_format, h, w, cx0, cy0, sel, rgb)
        else:
            _, x0, y0, text, rgb = item
            glyph = text_mask(text, s)
            cx0, cy0, cx1, cy1 = _clip(x0, y0, x0 + glyph.shape[1] - 1, y0 + glyph.shape[0] - 1, h, w)
            if cx0 > cx1 or cy0 > cy1:
                continue
            glyph = glyph[cy0 - y0:cy1 - y0 + 1, cx0 - x0:cx1 - x0 + 1]
            _paint(frame, pixel_format, h, w, cx0, cy0, np.ones_like(glyph), rgb)
            _paint(frame, pixel_format, h, w, cx0, cy0, glyph, text_colour(rgb))
    return OK


def dense_frame(surface):
    """A numpy copy of the picture of a ``utils.datasets.FrameSurface`` (on any device) in the dense native layout
    :func:`draw_detections` takes."""
    buf = surface.buffer.detach().cpu().numpy()
    h, w, fmt = surface.h, surface.w, surface.pixel_format

    def plane(offset, rows, row_bytes, pitch):
        return np.ndarray((rows, row_bytes), np.uint8, buffer=buf, offset=offset, strides=(pitch if rows > 1 else row_bytes, 1)).copy()

    if fmt == "nv12":
        return np.concatenate([plane(surface.offset, h, w, surface.pitch), plane(surface.uv_offset, h // 2, w, surface.uv_pitch)], 0)
    c = 2 if fmt == "yuyv" else 3
    return plane(surface.offset, h, c * w, surface.pitch).reshape(h, w, c)


class DeviceFrameOverlay:
    """:func:`draw_detections` for ``streams`` pictures in one launch (``me_frame_overlay_u8``): the items are built, the labels
    formatted and the pixels painted on the device, from the output buffer of ``me_stream_tail_f32`` and, optionally, the
    tracker's and the ranger's device rows.  The object holds the style, uploaded once: the palette in the stored byte order
    of every format, the glyph table and the class filter.  A workgroup walks the pixels of an item and writes a pixel only
    when no later item of the stream covers it, so every byte has one writer whatever the scheduling.

    Status per stream: :data:`OK`; :data:`E_BOXES` (more than 64 drawn rows: the stream's picture is untouched);
    :data:`E_INPUT` for every stream when the tail's buffer is flagged or inconsistent; :data:`E_SURFACE` for a stream whose
    descriptor row fails the rules of ``me_image_batch_surfaces_u8_f32`` on the device (the host copy of the descriptor is
    checked before the launch, which is then refused with ``hip.MeError``)."""

    def __init__(self, streams, device=None, **style):
        import torch
        from . import hip
        self._hip, self._torch = hip, torch
        self.streams = s = int(streams)
        if s <= 0 or s > 65535:
            raise hip.MeError(f"DeviceFrameOverlay: streams must be in 1 .. 65535 (got {streams})")
        self.style = check_style("DeviceFrameOverlay", **style)
        self.device = torch.device(device) if device is not None else hip.default_device()
        self.palette = torch.from_numpy(palette_table(self.style["palette"])).to(self.device)
        self.glyphs = torch.from_numpy(GLYPH_ROWS.copy()).to(self.device)
        cls = self.style["classes"]
        self.classes = None if cls is None else torch.tensor(list(cls) or [0], dtype=torch.int32).to(self.device)
        self._status = None
        self._keep = None   # the descriptor of the launch in flight

    def descriptor(self, surfaces):
        """The ``[streams,10]`` int64 CPU descriptor of ``surfaces``: such a tensor as it is, or a list of
        ``utils.datasets.FrameSurface`` on CUDA buffers of this device."""
        hip, torch = self._hip, self._torch
        if isinstance(surfaces, torch.Tensor):
            if surfaces.device.type != "cpu" or surfaces.dtype != torch.int64 or tuple(surfaces.shape) != (self.streams, 10):
                raise hip.MeError(f"DeviceFrameOverlay: surfaces must be a CPU int64 tensor [{self.streams}, 10] (got "
                                  f"{surfaces.dtype} {tuple(surfaces.shape)} on {surfaces.device})")
            return surfaces.contiguous()
        surfaces = list(surfaces)
        if len(surfaces) != self.streams:
            raise hip.MeError(f"DeviceFrameOverlay: {len(surfaces)} surfaces for {self.streams} streams")
        for i, s in enumerate(surfaces):
            where = getattr(getattr(s, "buffer", None), "device", None)
            if where is None or where.type != "cuda" or (self.device.index is not None and where.index != self.device.index):
                raise hip.MeError(f"DeviceFrameOverlay: surface {i} does not lie on {self.device} (it lies on {where})")
        return torch.tensor([s.row(s.buffer.data_ptr(), s.buffer.numel()) for s in surfaces], dtype=torch.int64).reshape(-1, 10)

    def draw(self, tail_out, m, surfaces, tracker=None, ranger=None, status=None):
        """The launch on the current stream (asynchronous).  ``tail_out``: the tail's output buffer (a CUDA uint8 tensor or
        its address) for this object's ``streams`` and ``m`` rows; ``surfaces``: see :meth:`descriptor`; ``tracker``:
        ``(tracks, counts)`` - the ``[streams,64,10]`` float64 rows and ``[streams,4]`` int32 counts of ``me_box_tracks_f64``
        on the device (tensors or addresses); ``ranger``: ``(ranges, status)`` - the ``[m,4]`` float64 rows and ``[streams]``
        int32 words of ``me_box_ranges_f64``; ``status``: the address of ``[streams]`` int32 device words (default: a buffer of
        this object).  Returns the status words as a device tensor, or ``None`` when ``status`` was given."""
        hip, torch = self._hip, self._torch
        desc = self.descriptor(surfaces)
        d_desc = desc.pin_memory().to(self.device, non_blocking=True)
        own = status is None
        if own:
            if self._status is None:
                self._status = torch.zeros((self.streams,), dtype=torch.int32, device=self.device)
            status = self._status
        st = self.style
        hip.frame_overlay(tail_out, m, self.streams, d_desc, desc, self.palette, self.glyphs, status, tracks=tracker,
                          ranges=ranger, classes=self.classes if st["classes"] is not None else None,
                          class_count=-1 if st["classes"] is None else len(st["classes"]), thickness=st["thickness"],
                          font_scale=st["font_scale"], labels=st["labels"], color_by_track=st["color_by"] == "track")
        self._keep = d_desc
        return self._status if own else None
