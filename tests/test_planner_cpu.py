"""CPU (-m "not gpu"): the detector engine's plan builder - lowering of the cfg graph (millieye_amd/planner.py: fusion, 16-bit
channel padding, concat slices, decode-last), liveness-based arena placement, and the descriptors ``DarknetEngine._build``
emits from them.

``tests/golden/engine_plans.json`` pins the plans: it was recorded from the ``_build`` that preceded the split into phases,
run on the CPU under the four stubs of :func:`stubbed` (``describe_plan`` below is the recorder's format).  Arena pointers are
stored as offsets from the arena base; weight pointers are not stored (they are no part of the plan)."""
import contextlib
import ctypes as C
import functools
import json
import os
import tempfile

import pytest
import torch

from millieye_amd import cfgs, engine, hip, planner
from millieye_amd.utils.parse_config import parse_model_config
from tests import parity_helpers as ph

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_plans.json")

# (cfg, dtype, n, size, keep_raw, decode_last)
CASES = [(name, dtype, 2, 96, False, True) for name in cfgs.KNOWN for dtype in ("f32", "bf16", "f16")]
CASES += [("yolov3", "f32", 2, 96, True, True), ("yolov3-tiny-12", "f32", 2, 96, True, True)]
CASES += [("yolov3", "f32", 1, 416, False, True), ("yolov3", "bf16", 1, 416, False, True)]
CASES += [("yolov3", "f32", 2, 96, False, False)]


def case_id(case):
    name, dtype, n, size, keep_raw, decode_last = case
    return f"{name}-{dtype}-n{n}-{size}" + ("-raw" if keep_raw else "") + ("" if decode_last else "-decode_in_place")


# ------------------------------------------------------------------------------------------ _build on a CPU
class _NullLib:
    """``hip.lib()`` without the library: every entry point returns 0 (no workspace, no error)."""

    def __getattr__(self, name):
        return lambda *args: 0


class _StubWeights:
    """What ``_build`` reads of a ``ConvWeights``: the packed shapes (padded like the real ones) and stable pointers."""
    wgt_tiled = None

    def __init__(self, conv, cin_pad, cout_pad):
        cout, cin, k, _ = conv.weight.shape
        cout = max(cout, cout_pad)
        self.wgt = torch.empty((cout, k, k, max(cin, cin_pad)))
        self.scale, self.shift = torch.empty(cout), torch.empty(cout)

    def refresh(self, device):
        return False


@contextlib.contextmanager
def stubbed(decode_last=True):
    """The four stubs under which ``DarknetEngine._build`` runs without a GPU: a null library, shape-only weights, no autotuner,
    and a 256-byte aligned arena (a CPU ``torch.empty`` often is not: over-allocate and slice)."""
    real_empty = torch.empty

    def empty(*size, **kw):
        if kw.get("dtype") is torch.uint8 and len(size) == 1 and isinstance(size[0], int):
            buf = real_empty(size[0] + 256, **kw)
            off = -buf.data_ptr() % 256
            return buf[off:off + size[0]]
        return real_empty(*size, **kw)

    def conv_weights(self, i, cin_pad=0, cout_pad=0):
        return _StubWeights(self.model.module_list[i][0], cin_pad, cout_pad)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, "lib", lambda: _NullLib())
        mp.setattr(engine.DarknetEngine, "_conv_weights", conv_weights)
        mp.setenv("MILLIEYE_AUTOTUNE", "0")
        mp.setenv("MILLIEYE_DECODE_LAST", "1" if decode_last else "0")
        mp.delenv("MILLIEYE_INLAUNCH_REDUCE", raising=False)
        mp.setattr(torch, "empty", empty)
        yield


@functools.lru_cache(maxsize=None)
def darknet(name):
    """Module tree of a known cfg (weights as constructed: a plan depends on shapes only)."""
    from millieye_amd.yolov3.models import Darknet
    return Darknet(ph.cfg_path(name)).eval()


def build_plan(case):
    name, dtype, n, size, keep_raw, decode_last = case
    with stubbed(decode_last):
        return engine.DarknetEngine(darknet(name), dtype)._build(n, size, size, torch.device("cpu"), keep_raw)


# ------------------------------------------------------------------------------------------ the recorded format
_ARENA_PTRS = ("x", "res", "y")            # stored as offsets from the arena base
_WEIGHT_PTRS = ("wgt", "scale", "shift")   # not stored
_ARG_PTRS = {"pool": (0, 2), "upsample": (0, 2), "copy": (0, 2), "add": (0, 2, 4)}  # pointer slots of the argument-tuple launches


def split_fields(struct):
    """``(pointer fields, value fields)`` of a descriptor in the order ``describe_launch`` stores them."""
    kept = [(f, t) for f, t in struct._fields_ if f not in _WEIGHT_PTRS]
    return [f for f, t in kept if t is C.c_void_p], [f for f, t in kept if t is not C.c_void_p]


def describe_launch(launch, base):
    """``[name, pointers, values]``: arena pointers relative to ``base`` (None stays None), then every other field / argument."""
    _fn, args, dsc, name = launch
    rel = lambda p: None if p is None else p - base  # noqa: E731
    if dsc is None:
        at = _ARG_PTRS[name.rstrip("0123456789")]
        return [name, [rel(args[k]) for k in at], [a for k, a in enumerate(args) if k not in at]]
    ptr_fields, val_fields = split_fields(type(dsc))
    ptrs = []
    for f in ptr_fields:
        v = getattr(dsc, f)
        assert f in _ARENA_PTRS or v is None, (name, f)  # (out / workspace / wgt_tiled / tile_counters: unset under the stubs)
        ptrs.append(rel(v))
    vals = [getattr(dsc, f) for f in val_fields]
    return [name, ptrs, [list(v) if hasattr(v, "__len__") else v for v in vals]]


def describe_plan(plan):
    base = plan.arena.data_ptr()
    return {"arena_bytes": plan.arena_bytes, "rows": plan.rows, "conv_flops": plan.conv_flops,
            "tap_shape": list(plan.tap_shape), "tap_offset": plan.tap_ptr - base, "tap_pitch": plan.tap_pitch,
            "launches": [describe_launch(entry, base) for entry in plan.launches]}


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------ the pure phases
def plan_case(case):
    """Lowering + placement of a case, no library, no module tree: ``(ops, tensors, out, yolo_rows, tap_tensor, total)``."""
    name, dtype, n, size, keep_raw, decode_last = case
    defs = parse_model_config(ph.cfg_path(name))
    net = defs.pop(0)
    return plan_defs(defs, int(net["channels"]), n, size, size, engine.pick_tap_module(defs), dtype != "f32", keep_raw, decode_last)


def plan_defs(defs, channels, n, h, w, tap, half, keep_raw=False, decode_last=True):
    ops, tensors, out, yolo_rows = planner.lower(defs, channels, h, w, tap, half, keep_raw, decode_last)
    tap_tensor = out[tap] if tap is not None else None
    total = planner.place(ops, tensors, n, tap_tensor, keep_raw)
    return ops, tensors, out, yolo_rows, tap_tensor, total


def emit(build):
    """cfg text from calls on a ``cfgs._Emitter`` -> module_defs (the [net] block dropped)."""
    e = cfgs._Emitter(64)
    build(e)
    with tempfile.NamedTemporaryFile("w", suffix=".cfg") as fh:
        fh.write(e.text())
        fh.flush()
        return parse_model_config(fh.name)[1:]


def where(t):
    """``(byte offset in the arena, pitch in elements)`` of a planned tensor; the caller-owned input has no offset."""
    root, coff = t.root()
    return (None if t.external else root.offset + coff * t.esize), root.c


def planner_facts(ops, n, half):
    """What the op list alone says about each launch, as ``{field: value}`` (descriptor launches) or ``(pointers, pitches)``."""
    facts = []
    for op in ops:
        kind, name = op["kind"], op["kind"] + str(op["module"])
        x, y = op.get("x"), op.get("y")
        if kind == "conv":
            (xp, xpitch), (yp, ypitch) = where(x), where(y)
            rp, rpitch = where(op["res"]) if op["res"] is not None else (None, 0)
            facts.append((name, dict(x=xp, res=rp, y=yp, x_pitch=xpitch, res_pitch=rpitch, y_pitch=ypitch, n=n, h=x.h, w=x.w, cin=x.c,
                                     cout=y.c, ksize=op["k"], stride=op["s"], pad=op["pad"], ho=op["ho"], wo=op["wo"], act=op["act"],
                                     upsample=op["ups"], x_nchw=int(x.external))))
        elif kind == "pool" and not half:
            (xp, xpitch), (yp, ypitch) = where(x), where(y)
            facts.append((name, dict(x=xp, y=yp, x_pitch=xpitch, y_pitch=ypitch, n=n, h=x.h, w=x.w, c=x.c, size=op["k"],
                                     stride=op["s"], zero_ext=op["zero_ext"], ho=op["ho"], wo=op["wo"])))
        elif kind == "yolo":
            xp, xpitch = where(x)
            facts.append((name, dict(x=xp, x_pitch=xpitch, n=n, g=op["g"], row_offset=op["row_offset"])))
        else:
            reads = [where(op[k]) for k in (("a", "b") if kind == "add" else ("x",))] + [where(y)]
            facts.append((name, ([p for p, _ in reads], [pitch for _, pitch in reads])))
    return facts


def struct_of(name, half):
    kind = name.rstrip("0123456789")
    if kind == "conv":
        return hip.Conv16Desc if half else hip.ConvDesc
    return {"pool": None if half else hip.PoolDesc, "yolo": hip.YoloDesc}.get(kind)


def named(entry, half):
    """A recorded launch as ``{field: value}`` (descriptor launches) or ``(pointers, pitches)`` (argument tuples)."""
    name, ptrs, vals = entry
    struct = struct_of(name, half)
    if struct is None:
        return ptrs, vals[:len(ptrs)]  # (x, x_pitch, y, y_pitch, ...): the pitches lead the values
    ptr_fields, val_fields = split_fields(struct)
    return dict(zip(ptr_fields + val_fields, ptrs + vals))


# ------------------------------------------------------------------------------------------ A. same plan as before the split
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lowering_and_placement_give_the_recorded_plan(case):
    want = fixture()[case_id(case)]
    half = case[1] != "f32"
    ops, _tensors, _out, yolo_rows, tap_tensor, total = plan_case(case)
    assert total == want["arena_bytes"] and sum(yolo_rows) == want["rows"]
    assert (where(tap_tensor)[0], where(tap_tensor)[1]) == (want["tap_offset"], want["tap_pitch"])
    assert [tap_tensor.h, tap_tensor.w, tap_tensor.c] == want["tap_shape"]
    facts = planner_facts(ops, case[2], half)
    assert [name for name, _ in facts] == [entry[0] for entry in want["launches"]]
    for (name, got), entry in zip(facts, want["launches"]):
        rec = named(entry, half)
        if isinstance(got, dict):
            assert got == {k: rec[k] for k in got}, name
        else:
            assert (got[0], got[1]) == (rec[0], rec[1]), name


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_build_emits_the_recorded_descriptors(case):
    got, want = describe_plan(build_plan(case)), fixture()[case_id(case)]
    assert len(got["launches"]) == len(want["launches"])
    half = case[1] != "f32"
    for a, b in zip(got["launches"], want["launches"]):
        assert a == b, (a[0], named(a, half), named(b, half))
    assert got == want


def test_fixture_holds_the_figures_of_the_issue():
    fx = fixture()
    assert sorted(fx) == sorted(case_id(c) for c in CASES)
    assert (fx["yolov3-f32-n2-96"]["arena_bytes"], len(fx["yolov3-f32-n2-96"]["launches"])) == (3538944, 78)
    for dtype in ("f32", "bf16"):
        rec = fx[f"yolov3-tiny-12-{dtype}-n2-96"]
        assert (rec["arena_bytes"], len(rec["launches"])) == (1474560, 21)


def test_activation_ids_are_the_library_s():
    assert (planner.ACT_LINEAR, planner.ACT_LEAKY) == (hip.ACT_LINEAR, hip.ACT_LEAKY)


# ------------------------------------------------------------------------------------------ B. nobody writes bytes that are still to be read
def _concat_copy(e):
    e.conv(32, 3)        # 0
    e.conv(32, 3)        # 1
    e.route(-1, -2)      # 2: [1, 0] - both become slices
    e.conv(32, 1)        # 3
    e.route(-1, 0)       # 4: module 0 already belongs to concat 2 -> a copy
    e.conv(64, 3)        # 5
    e.route(-1)          # 6: alias of 5
    e.conv(32, 1)        # 7


def _two_scales_16(e):
    """A yolov3-tiny in small: 16-channel stem (padded in the 16-bit modes), pools, two detection maps, upsample + route."""
    e.conv(16, 3)                                   # 0
    e.maxpool(2, 2)                                 # 1
    e.conv(32, 3)                                   # 2
    e.maxpool(2, 2)                                 # 3
    e.conv(64, 3)                                   # 4
    e.conv(27, 1, bn=False, act="linear")           # 5
    e.yolo((3, 4, 5), cfgs._TINY_ANCHORS, 4, 6)     # 6
    e.route(-3)                                     # 7
    e.conv(32, 1)                                   # 8
    e.upsample(2)                                   # 9
    e.route(-1, 2)                                  # 10
    e.conv(27, 1, bn=False, act="linear")           # 11
    e.yolo((0, 1, 2), cfgs._TINY_ANCHORS, 4, 6)     # 12


# build, tap, half, keep_raw, decode_last
HAND = {"concat_copy-f32": (_concat_copy, None, False, False, True), "two_scales-f32": (_two_scales_16, 4, False, False, True),
        "two_scales-bf16": (_two_scales_16, 4, True, False, True), "two_scales-f32-raw": (_two_scales_16, 4, False, True, True),
        "two_scales-f32-decode_in_place-raw": (_two_scales_16, 4, False, True, False)}  # (only the pin keeps these maps alive)


def _planned(key):
    if key in HAND:
        build, tap, half, keep_raw, decode_last = HAND[key]
        return (2,) + plan_defs(emit(build), 3, 2, 64, 64, tap, half, keep_raw, decode_last)
    case = next(c for c in CASES if case_id(c) == key)
    return (case[2],) + plan_case(case)


def _family(t):
    chain = [t]
    while chain[-1].parent is not None:
        chain.append(chain[-1].parent)
    return chain


def _span(t, n):
    root = _family(t)[-1]
    return root, root.offset, root.offset + n * root.h * root.w * root.c * root.esize


@pytest.mark.parametrize("key", [case_id(c) for c in CASES] + list(HAND))
def test_no_op_writes_bytes_that_are_still_to_be_read(key):
    """Walks the launch order itself (not the placer's intervals): between the last producer of a tensor and each of its readers
    (pinned tensors: the end of the plan) no op may write a root that shares bytes with the tensor's root."""
    n, ops, tensors, _out, _rows, tap_tensor, total = _planned(key)
    pinned = [t for t in [tap_tensor] if t is not None]
    if key.endswith("-raw"):
        pinned += [op["x"] for op in ops if op["kind"] == "yolo"]
        assert len(pinned) > 1
    reads = [(r, op[k]) for r, op in enumerate(ops) for k in ("x", "res", "a", "b") if op.get(k) is not None]
    reads += [(len(ops), t) for t in pinned]
    checked = 0
    for r, t in reads:
        if t.external:
            continue
        root, lo, hi = _span(t, n)
        produced = [j for j in range(r) if ops[j].get("y") is not None and any(f is t for f in _family(ops[j]["y"]))]
        assert produced, f"op {r} reads a tensor nobody wrote"
        for j in range(max(produced) + 1, min(r + 1, len(ops))):
            y = ops[j].get("y")
            if y is None:
                continue
            yroot, ylo, yhi = _span(y, n)
            assert yroot is root or yhi <= lo or hi <= ylo, f"op {j} ({ops[j]['kind']}{ops[j]['module']}) overwrites what op {r} reads"
            checked += 1
    assert checked > 0
    roots = [t for t in tensors if not t.external and t.parent is None and t.offset is not None]
    assert all(t.offset % 256 == 0 for t in roots)
    assert total == max(_span(t, n)[2] for t in roots)


# ------------------------------------------------------------------------------------------ C. lowering facts
def _lower(build, half=False, keep_raw=False, tap=None, h=64, w=64, decode_last=True):
    return planner.lower(emit(build), 3, h, w, tap, half, keep_raw, decode_last)


@pytest.mark.parametrize("half", [True, False])
def test_16bit_modes_pad_the_stem_and_keep_detection_maps_fp32(half):
    ops, _tensors, out, _rows = _lower(_two_scales_16, half=half)
    stem = ops[0]["y"]
    assert (stem.c, stem.padded, stem.esize) == ((32, 16, 2) if half else (16, 0, 4))
    assert (out[1].c, out[1].padded) == (stem.c, stem.padded)  # the pool carries the padding along
    assert ops[1]["kind"] == "pool" and ops[2]["x"].c == stem.c  # ... and the next convolution reads cin % 32 == 0
    for op in ops:
        if op["kind"] == "yolo":
            assert (op["x"].esize, op["x"].c, op["x"].padded) == (4, 27, 0)
        elif op.get("y") is not None and all(o["kind"] != "yolo" or o["x"] is not op["y"] for o in ops):
            assert op["y"].esize == (2 if half else 4)


def test_route_slices_copies_and_aliases():
    ops, _tensors, out, _rows = _lower(_concat_copy)
    cat2, cat4 = out[2], out[4]
    assert (out[1].parent, out[1].chan_off, out[0].parent, out[0].chan_off) == (cat2, 0, cat2, 32) and cat2.c == 64
    copies = [op for op in ops if op["kind"] == "copy"]
    assert len(copies) == 1 and copies[0]["module"] == 4 and copies[0]["x"] is out[0]
    piece = copies[0]["y"]
    assert (piece.parent, piece.chan_off, piece.c) == (cat4, 32, 32) and (out[3].parent, out[3].chan_off) == (cat4, 0)
    assert out[6] is out[5]  # a single-layer route is its source
    assert [op["kind"] for op in ops] == ["conv", "conv", "conv", "copy", "conv", "conv"]


def test_decodes_go_last_with_cumulative_rows():
    ops, _tensors, _out, rows = _lower(_two_scales_16)
    assert [op["kind"] for op in ops[-2:]] == ["yolo", "yolo"] and all(op["kind"] != "yolo" for op in ops[:-2])
    assert [(op["module"], op["row_offset"]) for op in ops[-2:]] == [(6, 0), (12, 3 * 16 * 16)]
    assert rows == [3 * 16 * 16, 3 * 32 * 32]
    in_place, _t, _o, rows2 = _lower(_two_scales_16, decode_last=False)
    assert [op["module"] for op in in_place] == sorted(op["module"] for op in in_place) and rows2 == rows
    assert [op["row_offset"] for op in in_place if op["kind"] == "yolo"] == [0, 3 * 16 * 16]
    for name in cfgs.KNOWN:
        case = (name, "f32", 2, 96, False, True)
        ops = plan_case(case)[0]
        k = sum(op["kind"] == "yolo" for op in ops)
        offsets = [op["row_offset"] for op in ops[-k:]]
        assert all(op["kind"] == "yolo" for op in ops[-k:]) and offsets == sorted(offsets) and offsets[0] == 0
        assert [op["module"] for op in ops[-k:]] == sorted(op["module"] for op in ops[-k:])


def _dropout(e):
    e.conv(32, 3)
    e._block("dropout", [("probability", ".5")])


def _conv_after_yolo(e):
    e.conv(27, 1, bn=False, act="linear")
    e.yolo((0, 1, 2), cfgs._TINY_ANCHORS, 4, 6)
    e.conv(32, 3)


def _route_ahead(e):
    e.conv(32, 3)
    e.route(-3)   # resolves in front of module 0: an index that wraps to a module not lowered yet
    e.conv(32, 3)


def _padded_shortcut(e):
    e.conv(16, 3)
    e.conv(16, 3)
    e.shortcut(-2)


def _padded_route(e):
    e.conv(16, 3)
    e.conv(16, 3)
    e.route(-1, -2)


def _ragged_route(e):
    e.conv(32, 3)
    e.conv(32, 3, stride=2)
    e.route(-1, -2)


def _one_scale(e):
    e.conv(32, 3)
    e.conv(27, 1, bn=False, act="linear")
    e.yolo((0, 1, 2), cfgs._TINY_ANCHORS, 4, 6)


@pytest.mark.parametrize("build, kw, exc, message", [
    (_dropout, {}, ValueError, "unsupported cfg block [dropout] at module 1"),
    (_conv_after_yolo, {}, RuntimeError, "module 2 reads a fused-away tensor"),
    (_route_ahead, {}, RuntimeError, "route 1 reads a fused-away tensor"),
    (_padded_shortcut, {"half": True}, NotImplementedError, "shortcut 2: mixed storage types / padded channels"),
    (_padded_route, {"half": True}, NotImplementedError, "route 2: mixed storage types / padded channels"),
    (_ragged_route, {}, ValueError, "route 2: spatial size mismatch"),
    (_one_scale, {"h": 64, "w": 96}, ValueError, "YOLO decode needs square inputs (the reference uses one grid_size)"),
    (_one_scale, {"half": True, "keep_raw": True}, NotImplementedError,
     "a 16-bit ENGINE PLAN keeps no raw maps (the loss value of an evaluation call comes from the fp32 engine; "
     "training in a 16-bit storage mode is millieye_amd/detector_train16.py, not an engine plan)"),
], ids=["block", "conv_reads_none", "route_reads_none", "shortcut_padded", "route_padded", "route_ragged", "yolo_square", "raw_16bit"])
def test_lowering_errors_keep_their_messages(build, kw, exc, message):
    with pytest.raises(exc) as info:
        _lower(build, **kw)
    assert str(info.value) == message


def test_emission_still_checks_the_yolo_channels():
    """The lowering takes no module tree: the check of the detection map against the layer object is the emission's."""
    model = darknet("yolov3-tiny-12")
    layer = model.module_list[16][0]
    classes = layer.num_classes
    layer.num_classes = classes + 1
    try:
        with pytest.raises(ValueError) as info, stubbed():
            engine.DarknetEngine(model)._build(1, 96, 96, torch.device("cpu"))
        assert str(info.value) == f"yolo 16: 51 channels != 3*({classes + 1}+5)"
    finally:
        layer.num_classes = classes
