"""planner.lower(..., rect=True): rectangular inputs (Darknet's rule - every [yolo] scale keeps one stride for both axes).  Pure
host code: no GPU, no library."""
import tempfile

import pytest

from millieye_amd import cfgs, planner
from millieye_amd.utils.parse_config import parse_model_config

SQUARE_ONLY = "YOLO decode needs square inputs (the reference uses one grid_size)"


def _emit(build):
    e = cfgs._Emitter(64)
    build(e)
    with tempfile.NamedTemporaryFile("w", suffix=".cfg") as fh:
        fh.write(e.text())
        fh.flush()
        return parse_model_config(fh.name)[1:]


def _one_scale(e):
    """One detection scale at stride 32: five stride-2 convolutions, then the detection convolution."""
    for width in (8, 16, 32, 32, 64):
        e.conv(width, 3, stride=2)
    e.conv(27, 1, bn=False, act="linear")
    e.yolo((0, 1, 2), cfgs._TINY_ANCHORS, 4, 6)


def _two_scales(e):
    """Strides 32 and 16 joined by upsample + route, pools instead of strided convolutions (yolov3-tiny in small)."""
    e.conv(16, 3)                                   # 0
    e.maxpool(2, 2)                                 # 1
    e.conv(16, 3, stride=2)                         # 2
    e.maxpool(2, 2)                                 # 3
    e.conv(32, 3, stride=2)                         # 4   stride 16
    e.maxpool(2, 2)                                 # 5   stride 32
    e.conv(27, 1, bn=False, act="linear")           # 6
    e.yolo((3, 4, 5), cfgs._TINY_ANCHORS, 4, 6)     # 7
    e.route(-3)                                     # 8
    e.upsample(2)                                   # 9
    e.route(-1, 4)                                  # 10
    e.conv(27, 1, bn=False, act="linear")           # 11
    e.yolo((0, 1, 2), cfgs._TINY_ANCHORS, 4, 6)     # 12


def _lower(build, h, w, **kw):
    return planner.lower(_emit(build), 3, h, w, None, kw.pop("half", False), False, **kw)


def test_rect_lowering_carries_gh_gw_and_places():
    ops, tensors, _out, rows = _lower(_one_scale, 64, 96, rect=True)
    yolo = [op for op in ops if op["kind"] == "yolo"]
    assert len(yolo) == 1 and (yolo[0]["gh"], yolo[0]["gw"]) == (2, 3) and "g" not in yolo[0]
    assert rows == [18] and yolo[0]["row_offset"] == 0
    assert (yolo[0]["x"].h, yolo[0]["x"].w, yolo[0]["x"].c) == (2, 3, 27)
    total = planner.place(ops, tensors, 2, None, False)
    assert total > 0 and all(t.offset is not None for t in tensors if not t.external and t.parent is None)
    # the transposed frame
    ops, _t, _o, rows = _lower(_one_scale, 96, 64, rect=True)
    assert [(op["gh"], op["gw"]) for op in ops if op["kind"] == "yolo"] == [(3, 2)] and rows == [18]


@pytest.mark.parametrize("half", [False, True])
def test_rect_two_scales_rows_and_offsets(half):
    ops, tensors, _out, rows = _lower(_two_scales, 64, 128, rect=True, half=half)
    yolo = [op for op in ops if op["kind"] == "yolo"]
    assert [(op["gh"], op["gw"], op["row_offset"]) for op in yolo] == [(2, 4, 0), (4, 8, 24)]
    assert rows == [3 * 2 * 4, 3 * 4 * 8] and all(op["x"].esize == 4 for op in yolo)
    assert planner.place(ops, tensors, 3, None, False) > 0


def test_square_lowering_is_what_it_was_with_and_without_rect():
    """``g`` stays where the two sides are equal; ``rect=True`` changes nothing else for a square input."""
    plain = _lower(_two_scales, 64, 64)
    rect = _lower(_two_scales, 64, 64, rect=True)
    for a, b in zip(plain[0], rect[0]):
        assert a["kind"] == b["kind"] and a["module"] == b["module"]
        if a["kind"] == "yolo":
            assert a["g"] == b["g"] == a["gh"] == a["gw"] == b["gh"] == b["gw"] and a["row_offset"] == b["row_offset"]
    assert plain[3] == rect[3] == [3 * 2 * 2, 3 * 4 * 4]


def test_default_call_still_refuses_with_the_old_message():
    with pytest.raises(ValueError) as info:
        _lower(_one_scale, 64, 96)
    assert str(info.value) == SQUARE_ONLY
    with pytest.raises(ValueError) as info:
        _lower(_one_scale, 64, 96, rect=False)
    assert str(info.value) == SQUARE_ONLY


@pytest.mark.parametrize("h,w", [(64, 80), (80, 64), (64, 48), (96, 72)])
def test_two_strides_are_refused(h, w):
    """A side that is no multiple of the stride rounds up on its own: 80 / 32 -> 3 cells, 26.67 pixels each, beside 32."""
    with pytest.raises(ValueError) as info:
        _lower(_one_scale, h, w, rect=True)
    assert "two strides" in str(info.value) and f"{h} x {w}" in str(info.value)


def test_max_stride():
    assert planner.max_stride(_emit(_one_scale)) == 32
    assert planner.max_stride(_emit(_two_scales)) == 32
    for name in cfgs.KNOWN:
        with tempfile.TemporaryDirectory() as tmp:
            assert planner.max_stride(parse_model_config(cfgs.write_cfg(name, tmp))[1:]) == 32, name
