"""The pure half of the detector engine's plan builder: cfg graph -> op list -> byte offsets in one arena.

Integer and graph logic only (no torch, no library): ``lower`` turns the cfg's ``module_defs`` into the ops the engine will
launch, ``place`` decides which activations may share bytes.  ``engine.DarknetEngine._build`` allocates the arena and fills the
launch descriptors from the result.  tests/test_planner_cpu.py runs both on a CPU in milliseconds.
"""

__all__ = ["lower", "place", "pick_tap_module"]

_ALIGN = 256  # bytes
ACT_LINEAR, ACT_LEAKY = 0, 1  # hip.ACT_* (me_act of include/millieye_hip.h)


def _resolve(idx, current):
    """darknet layer reference -> absolute module index (negative = relative to ``current``)."""
    idx = int(idx)
    return current + idx if idx < 0 else idx


def pick_tap_module(module_defs):
    """Index of the module whose output is ``Darknet.featuremap``.

    Reference rule (models.py:254-255): the ``nn.Sequential`` whose first child is named
    ``conv_8`` - i.e. module 8 when it is convolutional (true for the tiny cfgs).  For cfgs where
    module 8 is not a convolution (yolov3.cfg: a shortcut) the reference raises AttributeError;
    documented extension: the last 256-filter convolution before the second
    ``[yolo]`` block (yolov3.cfg module 91: 512->256 @ stride 16) - the only tensor compatible
    with ``cnn_layers_1((256, 490))`` and ``spatial_scale = 1/16`` (my_models.py:427,495).
    Returns ``None`` when no such module exists."""
    if len(module_defs) > 8 and module_defs[8]["type"] == "convolutional":
        return 8
    yolos = [i for i, d in enumerate(module_defs) if d["type"] == "yolo"]
    if len(yolos) < 2:
        return None
    tap = None
    for i in range(yolos[0] + 1, yolos[1]):
        d = module_defs[i]
        if d["type"] == "convolutional" and int(d["filters"]) == 256:
            tap = i
    return tap


class _Tensor:
    __slots__ = ("h", "w", "c", "parent", "chan_off", "producers", "readers", "offset", "pinned", "external", "esize",
                 "padded")

    def __init__(self, h, w, c, esize=4):
        self.h, self.w, self.c = h, w, c
        self.esize = esize    # bytes per element (4 = float32, 2 = bfloat16)
        self.padded = 0       # zero channels appended behind the logical ones (bf16 mode, tiny cfgs' 16-channel stem)
        self.parent = None
        self.chan_off = 0
        self.producers = []
        self.readers = []
        self.offset = None
        self.pinned = False
        self.external = False  # the network input (NCHW, caller owned)

    def root(self):
        t, off = self, 0
        while t.parent is not None:
            off += t.chan_off
            t = t.parent
        return t, off


def _in_family(cat, p):
    """True if ``cat`` is (transitively) a slice of ``p`` - guards against cyclic concat parents."""
    t = cat
    while t is not None:
        if t is p:
            return True
        t = t.parent
    return False


def _sources(module_defs):
    """``(srcs, readers)``: the modules each module reads, and who reads module k."""
    readers = [[] for _ in module_defs]
    srcs = [None] * len(module_defs)
    for i, d in enumerate(module_defs):
        t = d["type"]
        if t in ("convolutional", "upsample", "maxpool", "yolo"):
            srcs[i] = [i - 1]
        elif t == "route":
            srcs[i] = [_resolve(x, i) for x in d["layers"].split(",")]
        elif t == "shortcut":
            srcs[i] = [i - 1, _resolve(d["from"], i)]
        else:
            raise ValueError(f"unsupported cfg block [{t}] at module {i}")
        for s in srcs[i]:
            if s >= 0:
                readers[s].append(i)
    return srcs, readers


def max_stride(module_defs):
    """The largest downsampling factor a ``[yolo]`` block of the cfg sees (32 for every cfg in ``cfgs.py``): rectangular inputs
    must be multiples of it in both axes, or the scales would not share one stride per axis."""
    srcs, _readers = _sources(module_defs)
    factor, best = [], 1
    for i, d in enumerate(module_defs):
        f = factor[srcs[i][0]] if srcs[i][0] >= 0 else 1
        t = d["type"]
        if t == "convolutional" or (t == "maxpool" and int(d["stride"]) > 1):
            f = f * int(d["stride"])
        elif t == "upsample":
            f = f / int(d["stride"])
        elif t == "yolo":
            best = max(best, int(f))
        factor.append(f)
    return best


def lower(module_defs, channels, h, w, tap, half, keep_raw, decode_last=True, rect=False):
    """cfg blocks -> ``(ops, tensors, out, yolo_rows)``: the op dicts in launch order, every ``_Tensor`` they touch (the network
    input first), ``out[i]`` = the tensor module ``i`` leaves behind (None: fused away / decoded rows) and the rows per [yolo].

    ``conv -> [shortcut]`` and ``conv -> [upsample x2]`` become one op when nobody else reads the intermediate (``tap`` counts as
    a reader); a multi-layer ``[route]`` makes its parts channel slices of one wider tensor (a ``copy`` op where a part already is
    a slice of another).  ``half`` (16-bit storage): activations take 2 bytes, channel counts are padded to multiples of 32 and the
    maps that feed only ``[yolo]`` stay fp32.  ``decode_last``: the [yolo] ops go behind the last convolution.  ``rect``: accept
    ``h != w`` (a yolo op then carries ``gh, gw``, and ``g`` only when the two are equal; every scale must keep one stride,
    ``h / gh == w / gw``); without it a non-square input is refused, as the reference's ``grid_size`` would."""
    defs, L = module_defs, len(module_defs)
    srcs, readers = _sources(defs)
    if half and keep_raw:
        raise NotImplementedError("a 16-bit ENGINE PLAN keeps no raw maps (the loss value of an evaluation call comes from the fp32 engine; "
                                  "training in a 16-bit storage mode is millieye_amd/detector_train16.py, not an engine plan)")
    act_esize = 2 if half else 4
    tensors = []

    def new_tensor(hh, ww, cc, esize=None):
        t = _Tensor(hh, ww, cc, act_esize if esize is None else esize)
        tensors.append(t)
        return t

    t_in = new_tensor(h, w, channels, 4)
    t_in.external = True
    out = [None] * L  # layer index -> _Tensor
    ops = []  # dicts
    yolo_rows = []
    i = 0
    while i < L:
        d = defs[i]
        t = d["type"]
        if t == "convolutional":
            x = t_in if i == 0 else out[i - 1]
            if x is None:
                raise RuntimeError(f"module {i} reads a fused-away tensor")
            feeds_yolo_only = bool(readers[i]) and all(defs[r]["type"] == "yolo" for r in readers[i])
            only_next = readers[i] == [i + 1] and i != tap
            res = out[srcs[i + 1][1]] if i + 1 < L and defs[i + 1]["type"] == "shortcut" and srcs[i + 1][1] != i else None
            op = _lower_conv(i, d, x, defs[i + 1] if i + 1 < L else None, only_next, res, feeds_yolo_only, half, new_tensor)
            ops.append(op)
            out[op["covers"][-1]] = op["y"]
            i = op["covers"][-1]
        elif t == "maxpool":
            x = out[i - 1]
            k, s = int(d["size"]), int(d["stride"])
            pad = (k - 1) // 2
            ext = 1 if (k == 2 and s == 1) else 0
            ho = (x.h + ext + 2 * pad - k) // s + 1
            wo = (x.w + ext + 2 * pad - k) // s + 1
            y = new_tensor(ho, wo, x.c, x.esize)
            y.padded = x.padded
            ops.append(dict(kind="pool", module=i, x=x, y=y, k=k, s=s, pad=pad, zero_ext=ext, ho=ho, wo=wo))
            out[i] = y
        elif t == "upsample":
            x = out[i - 1]
            f = int(d["stride"])
            y = new_tensor(x.h * f, x.w * f, x.c, x.esize)
            y.padded = x.padded
            ops.append(dict(kind="upsample", module=i, x=x, y=y, f=f))
            out[i] = y
        elif t == "shortcut":
            a, b = out[srcs[i][0]], out[srcs[i][1]]
            if a.esize != b.esize or a.padded or b.padded:
                raise NotImplementedError(f"shortcut {i}: mixed storage types / padded channels")
            y = new_tensor(a.h, a.w, a.c, a.esize)
            ops.append(dict(kind="add", module=i, a=a, b=b, y=y))
            out[i] = y
        elif t == "route":
            out[i] = _lower_route(i, [out[s] for s in srcs[i]], ops, new_tensor)
        elif t == "yolo":
            x = out[i - 1]
            if not rect and (x.h != x.w or h != w):
                raise ValueError("YOLO decode needs square inputs (the reference uses one grid_size)")
            if h * x.w != w * x.h:  # one stride for both axes: H / gh == W / gw (Darknet's rectangular rule)
                raise ValueError(f"yolo {i}: a {x.h} x {x.w} detection map of a {h} x {w} input has two strides "
                                 f"({h / x.h} and {w / x.w})")
            if x.esize != 4:
                raise RuntimeError(f"yolo {i}: the detection map is shared with another reader (bf16 mode)")
            op = dict(kind="yolo", module=i, x=x, gh=x.h, gw=x.w, row_offset=sum(yolo_rows))
            if x.h == x.w:
                op["g"] = x.h
            ops.append(op)
            yolo_rows.append(len(d["mask"].split(",")) * x.h * x.w)
            out[i] = None  # decoded rows are never routed
        i += 1

    # the [yolo] decodes go behind the last convolution: one launch for all scales (me_yolo_decode_cand_multi_f32) instead of
    # three small ones in the middle of the dependent chain; the detection maps stay live until then (liveness in ``place``)
    if decode_last:
        ops = [op for op in ops if op["kind"] != "yolo"] + [op for op in ops if op["kind"] == "yolo"]
    return ops, tensors, out, yolo_rows


def _lower_conv(i, d, x, nxt, only_next, res, feeds_yolo_only, half, new_tensor):
    """One ``[convolutional]`` block -> its op; ``op["covers"]`` is ``(i, i + 1)`` when the next block (``nxt``, read by nobody
    else: ``only_next``) rides in the epilogue - a ``[shortcut]`` adding ``res``, or an ``[upsample]`` by 2."""
    k, s = int(d["size"]), int(d["stride"])
    pad = (k - 1) // 2
    cout = int(d["filters"])
    ho = (x.h + 2 * pad - k) // s + 1
    wo = (x.w + 2 * pad - k) // s + 1
    act = ACT_LEAKY if d["activation"] == "leaky" else ACT_LINEAR
    op = dict(kind="conv", module=i, x=x, res=None, k=k, s=s, pad=pad, act=act, ups=1, ho=ho, wo=wo, cout=cout)
    y_esize, y_c = (2 if half else 4), cout
    if half:
        if x.esize != (4 if x.external else 2):
            raise RuntimeError(f"module {i}: a convolution reads an fp32 detection map in bf16 mode")
        if feeds_yolo_only:
            y_esize = 4   # raw detection maps stay fp32 for the YOLO decode
        elif cout % 32:
            y_c = -(-cout // 32) * 32  # the next MFMA conv needs cin % 32 == 0: zero channels behind the real ones
    fusable = nxt is not None and only_next and x.c > 4 and y_c == cout
    if (fusable and nxt["type"] == "shortcut" and res is not None
            and (res.h, res.w, res.c) == (ho, wo, cout) and y_esize == res.esize):
        op.update(res=res, y=new_tensor(ho, wo, cout, y_esize), covers=(i, i + 1))
    elif fusable and nxt["type"] == "upsample" and int(nxt["stride"]) == 2:
        op.update(ups=2, y=new_tensor(ho * 2, wo * 2, cout, y_esize), covers=(i, i + 1))
    else:
        op.update(y=new_tensor(ho, wo, y_c, y_esize), covers=(i,))
        op["y"].padded = y_c - cout
    return op


def _lower_route(i, parts, ops, new_tensor):
    """``[route]``: one source is an alias; several become channel slices of one new tensor, which is returned."""
    if any(p is None for p in parts):
        raise RuntimeError(f"route {i} reads a fused-away tensor")
    if len(parts) == 1:
        return parts[0]
    if any(p.padded or p.esize != parts[0].esize for p in parts):
        raise NotImplementedError(f"route {i}: mixed storage types / padded channels")
    cat = new_tensor(parts[0].h, parts[0].w, sum(p.c for p in parts), parts[0].esize)
    off = 0
    for p in parts:
        if (p.h, p.w) != (cat.h, cat.w):
            raise ValueError(f"route {i}: spatial size mismatch")
        if p.parent is None and not p.external and p is not cat and not _in_family(cat, p):
            p.parent, p.chan_off = cat, off
        else:  # already part of another concat: materialise a copy
            piece = new_tensor(p.h, p.w, p.c, p.esize)
            piece.parent, piece.chan_off = cat, off
            ops.append(dict(kind="copy", module=i, x=p, y=piece))
        off += p.c
    return cat


def place(ops, tensors, n, tap_tensor, keep_raw):
    """Liveness at op granularity, then first-fit packing of the root tensors into one arena at 256-byte alignment: sets
    ``readers`` / ``producers`` / ``pinned`` on the tensors and ``offset`` on the roots, returns the arena's size in bytes.
    A concat family lives from its first producer to its last reader; the feature tap (and with ``keep_raw`` the raw detection
    maps, which the YOLO loss reads after the run) is read by the caller, so its bytes are never reused."""
    for oi, op in enumerate(ops):
        for key in ("x", "res", "a", "b"):
            tt = op.get(key)
            if tt is not None:
                tt.readers.append(oi)
        if op.get("y") is not None:
            op["y"].producers.append(oi)
    if tap_tensor is not None:
        tap_tensor.pinned = True
    if keep_raw:
        for op in ops:
            if op["kind"] == "yolo":
                op["x"].pinned = True

    fam = {}
    for tt in tensors:
        if tt.external:
            continue
        root, _ = tt.root()
        first, last, pin = fam.get(id(root), (10 ** 9, -1, False))
        if tt.producers:
            first = min(first, min(tt.producers))
        if tt.readers:
            last = max(last, max(tt.readers))
        pin = pin or tt.pinned
        fam[id(root)] = (first, last, pin)
    roots = []
    for tt in tensors:
        if tt.external or tt.parent is not None or id(tt) not in fam:
            continue
        first, last, pin = fam[id(tt)]
        if first == 10 ** 9:
            continue  # never produced (should not happen)
        if pin:
            last = len(ops)
        last = max(last, first)
        size = -(-(n * tt.h * tt.w * tt.c * tt.esize) // _ALIGN) * _ALIGN  # bytes
        roots.append((first, last, size, tt))
    roots.sort(key=lambda r: (r[0], -r[2]))
    placed = []  # (offset, size, first, last)
    total = 0
    for first, last, size, tt in roots:
        busy = sorted((o, s) for (o, s, f, l) in placed if not (l < first or f > last))
        off = 0
        for o, s in busy:
            if off + size <= o:
                break
            off = max(off, o + s)
        tt.offset = off
        placed.append((off, size, first, last))
        total = max(total, off + size)
    return total
