"""No GPU: what the launcher of ``me_conv_wgrad_mfma_f32`` / ``me_conv_wgrad_mfma_oihw_f32`` chooses, asked through
``me_conv_wgrad_form`` - the function the launcher itself decides by (csrc/train.hip ``wgrad_plan``), which makes no HIP call.

* every threshold of the choice from both sides: the kernel form, the number of slices and the reduction form;
* every convolution of yolov3.cfg at 416 x 416, batch 8 hits exactly the six default forms;
* every case of tests/wgrad_cases.py (the tables tests/test_gpu_wgrad_blocks.py runs on the GPU) maps to the form it names -
  the switch-only forms in a child process that sets the switch, like on the GPU.  A retuned threshold that takes a kernel's
  coverage away fails here.

The expected slice counts are worked out from the rules in the comments of csrc/train.hip / csrc/wgrad9.hip: per-tap kernels
s = ceil(target / tiles) with target 2048 (1024 for 128 x 128 tiles), at most ceil(P / 256) and 256; nine-tap kernel
ceil(256 / tiles), at most ceil(Mp / 256) over the Mp = n (h + 1)(w + 1) padded positions, then re-cut into slices of a
multiple of 32 positions."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (the child below runs this file as a script)
    sys.path.insert(0, ROOT)

from tests import wgrad_cases as W  # noqa: E402
from tests.wgrad_cases import case  # noqa: E402


@pytest.fixture(scope="module")
def hip(hip_lib):
    from millieye_amd import hip as hip_
    for name in ("MILLIEYE_WGRAD_TILE", "MILLIEYE_WGRAD_DEPTH", "MILLIEYE_WGRAD9", "MILLIEYE_WGRAD9_NG", "MILLIEYE_WGRAD_WGS",
                 "MILLIEYE_WGRAD_MINPX", "MILLIEYE_WGRAD9_WGS"):
        assert name not in os.environ, f"{name} is set: the default choice cannot be tested in this process"
    return hip_


def _is(hip, c, form, splits, reduce, **kw):
    got = W.query(hip, c, **kw)
    assert got == (form, splits, reduce), f"{c['name']}: {got}, expected {(form, splits, reduce)}"


def test_pixel_count_threshold(hip):
    """k >= 3, cin and cout >= 128: 64 x 64 tiles below 16384 output pixels, 128 x 128 from there on (cin 132: off the nine-tap
    kernel).  16383 = 3 * 43 * 127: 3 * 2 * 9 = 54 tiles -> ceil(2048 / 54) = 38 slices; 16384: 2 * 1 * 9 = 18 tiles of
    128 x 128 -> ceil(1024 / 18) = 57."""
    _is(hip, case("p16383", None, 3, 43, 127, 132, 128, 3), "mfma_vec", 38, "flat_v4")
    _is(hip, case("p16384", None, 4, 64, 64, 132, 128, 3), "tile_128_128", 57, "flat_v4")
    _is(hip, case("p16384_c124", None, 4, 64, 64, 124, 128, 3), "mfma_vec", 57, "flat_v4")     # 2 * 2 * 9 = 36 tiles
    _is(hip, case("p16384_co124", None, 4, 64, 64, 132, 124, 3), "mfma_vec", 38, "flat_v4")    # 3 * 2 * 9 = 54 tiles
    _is(hip, case("p16384_k1", None, 4, 64, 64, 132, 128, 1), "mfma_vec", 64, "flat_v4")       # 6 tiles -> 342, at most P / 256


def test_narrow_input_threshold(hip):
    """cin <= 32: the half-wide pipelined tile.  286 pixels: at most ceil(286 / 256) = 2 slices."""
    _is(hip, case("cin32", None, 2, 13, 11, 32, 68, 3), "pipe_64_32", 2, "flat_v4")
    _is(hip, case("cin36", None, 2, 13, 11, 36, 68, 3), "mfma_vec", 2, "flat_v4")
    _is(hip, case("cin32_scalar", None, 2, 13, 11, 32, 66, 3), "mfma_scalar", 2, "flat_v4")


@pytest.mark.parametrize("k64", [64, 128])
def test_nine_tap_channel_threshold(hip, k64):
    """3 x 3 / stride 1 / pad 1 with cin and cout multiples of 64: all nine taps in one workgroup.  2 x 13 x 13: 392 padded
    positions -> at most 2 slices (224 positions each); the per-tap neighbours: 338 pixels -> 2 slices."""
    _is(hip, case("nine", None, 2, 13, 13, k64, 64, 3), "nine_tap", 2, "flat_v4")
    _is(hip, case("nine_t", None, 2, 13, 13, 64, k64, 3), "nine_tap", 2, "flat_v4")
    _is(hip, case("cin+4", None, 2, 13, 13, k64 + 4, 64, 3), "mfma_vec", 2, "flat_v4")
    _is(hip, case("cout+4", None, 2, 13, 13, 64, k64 + 4, 3), "mfma_vec", 2, "flat_v4")
    _is(hip, case("nine_oihw", None, 2, 13, 13, k64, 64, 3, oihw=True), "nine_tap", 2, "oihw_v4")


def test_vector_path_conditions(hip):
    """16-byte loads need cin, cout and both pitches % 4 == 0 and both pointers 16-byte aligned; the flat 16-byte reduction needs
    count % 4 == 0 and dw and the workspace aligned."""
    base = dict(n=3, h=13, w=11, cin=36, cout=100, k=1)   # 429 pixels: 2 slices
    mk = lambda **kw: case("vec", None, **{**base, **{k: v for k, v in kw.items() if k in base}},  # noqa: E731
                           **{k: v for k, v in kw.items() if k not in base})
    _is(hip, mk(), "mfma_vec", 2, "flat_v4")
    _is(hip, mk(cin=38), "mfma_scalar", 2, "flat_v4")
    _is(hip, mk(cin=37, cout=101), "mfma_scalar", 2, "flat")       # count % 4 != 0
    _is(hip, mk(cout=102), "mfma_scalar", 2, "flat_v4")
    _is(hip, mk(xr=1), "mfma_scalar", 2, "flat_v4")
    _is(hip, mk(yr=2), "mfma_scalar", 2, "flat_v4")
    _is(hip, mk(xl=1, xr=3), "mfma_scalar", 2, "flat_v4")          # pitch 40, pointer 4 bytes off
    _is(hip, mk(yl=1, yr=3), "mfma_scalar", 2, "flat_v4")
    _is(hip, mk(xl=4), "mfma_vec", 2, "flat_v4")
    _is(hip, mk(), "mfma_vec", 2, "flat", dw_ptr=W.DW_BASE + 4)
    _is(hip, mk(), "mfma_vec", 2, "flat", ws_ptr=W.WS_BASE + 4)
    _is(hip, mk(k=3, oihw=True), "mfma_vec", 2, "oihw_v4")
    _is(hip, mk(k=3, oihw=True), "mfma_vec", 2, "oihw", ws_ptr=W.WS_BASE + 8)
    _is(hip, mk(k=3, cin=10, cout=255, oihw=True), "mfma_scalar", 2, "oihw")
    _is(hip, mk(oihw=True), "mfma_vec", 2, "flat_v4")              # 1 x 1: the two layouts coincide
    # the nine-tap kernel has no scalar loads: a pitch or a pointer off sends the shape to the per-tap scalar kernel
    nine = dict(n=2, h=13, w=13, cin=64, cout=64, k=3)
    _is(hip, case("nine_pitch", None, **nine, xr=2), "mfma_scalar", 2, "flat_v4")
    _is(hip, case("nine_dy_pitch", None, **nine, yr=1), "mfma_scalar", 2, "flat_v4")
    _is(hip, case("nine_ptr", None, **nine, xl=1, xr=3), "mfma_scalar", 2, "flat_v4")
    _is(hip, case("nine_dy_ptr", None, **nine, yl=2, yr=2), "mfma_scalar", 2, "flat_v4")
    _is(hip, case("nine_sliced", None, **nine, xl=4, yr=4), "nine_tap", 2, "flat_v4")


def test_nine_tap_ring_edges(hip):
    """Halo rounds 1 -> 2 between W = 14 and 15 (both on the nine-tap kernel); the LDS ring of 2 hb + 4 (+ 1) slots of 4 KB and
    8 KB of dy fills 156 KB of 160 at W = 238 and would need 164 KB at W = 239; a halo of 16 hb positions must be shorter than
    one padded image: (1, 16) has 34 positions against 32, (1, 15) has 32."""
    _is(hip, case("w14", None, 2, 3, 14, 64, 64, 3), "nine_tap", 1, "flat_v4")      # 120 padded positions: one slice
    _is(hip, case("w15", None, 2, 3, 15, 64, 64, 3), "nine_tap", 1, "flat_v4")
    _is(hip, case("w238", None, 1, 2, 238, 64, 64, 3), "nine_tap", 3, "flat_v4")    # 717 positions: 3 slices of 256
    _is(hip, case("w239", None, 1, 2, 239, 64, 64, 3), "mfma_vec", 2, "flat_v4")    # 478 pixels
    _is(hip, case("1x16", None, 1, 1, 16, 64, 64, 3), "nine_tap", 1, "flat_v4")
    _is(hip, case("1x15", None, 1, 1, 15, 64, 64, 3), "mfma_vec", 1, "none")
    _is(hip, case("1x15_oihw", None, 1, 1, 15, 64, 64, 3, oihw=True), "mfma_vec", 1, "oihw_v4")


def test_nine_tap_stride_and_padding(hip):
    _is(hip, case("s2", None, 2, 13, 13, 64, 64, 3, s=2), "mfma_vec", 1, "none")       # 98 pixels
    _is(hip, case("pad0", None, 2, 13, 13, 64, 64, 3, pad=0), "mfma_vec", 1, "none")   # 242 pixels
    _is(hip, case("pad2", None, 2, 13, 13, 64, 64, 3, pad=2), "mfma_vec", 2, "flat_v4")
    _is(hip, case("k1", None, 2, 13, 13, 64, 64, 1), "mfma_vec", 2, "flat_v4")
    _is(hip, case("k5", None, 2, 13, 13, 64, 64, 5), "mfma_vec", 2, "flat_v4")


def test_workspace_thresholds(hip):
    """Too small a workspace never fails an OHWI call: nine-tap falls back to per-tap, sliced to one pass writing dw itself.
    OIHW with k > 1 goes through at least one slab, and is refused without."""
    lib = hip.lib()
    nine = case("nine", None, 2, 13, 13, 64, 64, 3)
    cnt = W.count(nine)
    assert W.full_workspace_bytes(lib, nine) == 2 * 4 * cnt
    _is(hip, nine, "nine_tap", 2, "flat_v4")
    _is(hip, nine, "mfma_vec", 1, "none", ws_bytes=2 * 4 * cnt - 4)
    _is(hip, nine, "mfma_vec", 1, "none", ws_bytes=0)
    _is(hip, dict(nine, oihw=True), "mfma_vec", 1, "oihw_v4", ws_bytes=2 * 4 * cnt - 4)
    _is(hip, dict(nine, oihw=True), "mfma_vec", 1, "oihw_v4", ws_bytes=4 * cnt)
    assert W.query(hip, dict(nine, oihw=True), ws_bytes=4 * cnt - 4)[0] == W.BADARG
    assert W.query(hip, dict(nine, oihw=True), ws_bytes=0)[0] == W.BADARG
    sliced = case("sliced", None, 5, 23, 21, 48, 100, 3, s=2)   # 660 pixels: 3 slices
    cnt = W.count(sliced)
    assert W.full_workspace_bytes(lib, sliced) == 3 * 4 * cnt
    _is(hip, sliced, "mfma_vec", 3, "flat_v4")
    _is(hip, sliced, "mfma_vec", 1, "none", ws_bytes=3 * 4 * cnt - 4)
    _is(hip, sliced, "mfma_vec", 1, "none", ws_bytes=0)
    _is(hip, dict(sliced, oihw=True), "mfma_vec", 3, "oihw_v4")
    _is(hip, dict(sliced, oihw=True), "mfma_vec", 1, "oihw_v4", ws_bytes=3 * 4 * cnt - 4)
    assert W.query(hip, dict(sliced, oihw=True), ws_bytes=4 * cnt - 4)[0] == W.BADARG
    assert W.query(hip, dict(sliced, oihw=True, k=1, pad=0), ws_bytes=0)[0] == "mfma_vec"


def test_stem_conditions(hip):
    """cin == 3, 3 x 3, cout % 4 == 0, dy rows 16-byte aligned and a workspace of 768 partial sums per weight; anything else is
    the generic scalar kernel (cin = 3 has no 16-byte loads)."""
    stem = case("stem", None, 2, 9, 13, 3, 32, 3)
    need = W.SW_BLOCKS * W.count(stem) * 4
    assert W.full_workspace_bytes(hip.lib(), stem) == need
    _is(hip, stem, "stem", W.SW_BLOCKS, "stem")
    _is(hip, dict(stem, oihw=True, s=2), "stem", W.SW_BLOCKS, "stem")
    _is(hip, dict(stem, xl=1, xr=1), "stem", W.SW_BLOCKS, "stem")          # x is read element by element
    _is(hip, dict(stem, cout=34), "mfma_scalar", 1, "none")                # 234 pixels: one slice
    _is(hip, dict(stem, k=1, pad=0), "mfma_scalar", 1, "none")
    _is(hip, dict(stem, k=5, pad=2), "mfma_scalar", 1, "none")
    _is(hip, dict(stem, cin=4), "pipe_64_32", 1, "none")
    _is(hip, dict(stem, yr=2), "mfma_scalar", 1, "none")
    _is(hip, dict(stem, yl=1, yr=3), "mfma_scalar", 1, "none")
    _is(hip, stem, "mfma_scalar", 1, "none", ws_bytes=need - 4)
    _is(hip, stem, "mfma_scalar", 1, "none", ws_bytes=0)
    _is(hip, dict(stem, oihw=True), "mfma_scalar", 1, "oihw", ws_bytes=need - 4)
    assert W.query(hip, dict(stem, oihw=True), ws_bytes=0)[0] == W.BADARG


def test_refusals(hip):
    ok = case("ok", None, 2, 13, 11, 36, 100, 3)
    assert W.query(hip, ok)[0] == "mfma_vec"
    assert W.query(hip, ok, x_ptr=0)[0] == W.NULLPTR
    assert W.query(hip, ok, dy_ptr=0)[0] == W.NULLPTR
    assert W.query(hip, ok, dw_ptr=0)[0] == W.NULLPTR
    for bad in (dict(k=8), dict(k=0), dict(n=0), dict(h=0), dict(cin=0), dict(cout=0), dict(s=0), dict(pad=-1)):
        assert W.query(hip, dict(ok, **bad), ws_bytes=1 << 24)[0] == W.BADARG, bad
    # a filter larger than the padded map has no output pixel (and (-3) * (-3) "pixels" would pass for a size)
    assert W.query(hip, dict(ok, h=3, w=3, k=7, pad=0))[0] == W.BADARG
    assert W.query(hip, dict(ok, h=3, w=13, k=7, pad=1))[0] == W.BADARG
    assert W.query(hip, dict(ok, h=7, w=7, k=7, pad=0))[0] == "mfma_vec"
    # the workspace query answers 0 for sizes the call refuses (it used to divide by a tile count of zero)
    for args in ((0, 13, 11, 36, 100, 3), (2, 0, 11, 36, 100, 3), (2, 13, -1, 36, 100, 3), (2, 13, 11, 0, 100, 3),
                 (2, 13, 11, 36, 0, 3), (2, 13, 11, 36, 100, 0)):
        assert hip.lib().me_conv_wgrad_workspace_bytes(*args) == 0, args


def test_every_yolov3_layer_runs_one_of_the_six_default_forms(hip):
    """The convolutions of yolov3.cfg at 416 x 416, batch 8, as the fp32 detector step calls them (OIHW, the full workspace, x on
    the pitch of the tensor it is a channel slice of): together they reach exactly the six default forms."""
    from millieye_amd import planner
    from millieye_amd.utils.parse_config import parse_model_config
    from tests import parity_helpers as ph
    defs = parse_model_config(ph.cfg_path("yolov3"))
    net = defs.pop(0)
    ops, _tensors, _out, _rows = planner.lower(defs, int(net["channels"]), 416, 416, None, False, True)
    seen, lines = {}, []
    for op in ops:
        if op["kind"] != "conv":
            continue
        x = op["x"]
        root, off = x.root()
        c = case(f"module {op['module']}", None, 8, x.h, x.w, x.c, op["cout"], op["k"], s=op["s"], pad=op["pad"], xl=off,
                 xr=root.c - off - x.c, oihw=True)
        form, splits, reduce = W.query(hip, c)
        assert isinstance(form, str), (c, form)
        seen.setdefault(form, []).append(op["module"])
        lines.append(f"module {op['module']}: {x.h}x{x.w} cin {x.c} (pitch {root.c}) cout {op['cout']} k {op['k']} s {op['s']} -> "
                     f"{form}, {splits} slices, {reduce}")
    assert len(lines) == 75
    want = {"stem", "nine_tap", "pipe_64_32", "tile_128_128", "mfma_vec", "mfma_scalar"}
    assert set(seen) == want, "\n".join(lines)


def _default_tables():
    return W.PART_A + W.PART_B + W.PART_C


def test_every_gpu_case_maps_to_the_form_it_names(hip):
    names = [c["name"] for c in _default_tables()]
    assert len(set(names)) == len(names)
    for c in _default_tables():
        W.assert_form(hip, c)
    assert {c["form"] for c in W.PART_A} == {"stem", "nine_tap", "pipe_64_32", "tile_128_128", "mfma_vec", "mfma_scalar"}
    assert {c["reduce"] for c in W.PART_B} == {"none", "flat", "flat_v4", "oihw", "oihw_v4", "stem"}
    for name in W.PART_A_REAL + W.LOCALITY:
        assert name in names
    assert {c["form"] for c in W.PART_A if c["name"] in W.PART_A_REAL} == {c["form"] for c in W.PART_A}
    for c in _default_tables():   # exact inputs stay exact: P * 16 < 2^24
        assert W.pixels(c) < 2 ** 20


def _child(name):
    """Runs in a fresh process with the child's switches set: prints the forms its cases do NOT map to."""
    from millieye_amd import hip as hip_
    env, cases = W.CHILDREN[name]
    assert all(os.environ.get(k) == v for k, v in env.items())
    bad = []
    for c in cases:
        got = W.query(hip_, c)
        if got[0] != c["form"]:
            bad.append([c["name"], c["form"], str(got)])
    print("WGRAD_FORMS " + json.dumps(bad))


@pytest.mark.parametrize("name", sorted(W.CHILDREN))
def test_every_switch_only_case_maps_to_the_form_it_names(hip, name):
    """The switches are read once per process: a child process with the switch set asks the same query."""
    env, cases = W.CHILDREN[name]
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), name], cwd=ROOT, env=dict(os.environ, **env), timeout=120,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = proc.stdout.decode(errors="replace")
    assert proc.returncode == 0, out[-4000:]
    bad = json.loads([line for line in out.splitlines() if line.startswith("WGRAD_FORMS ")][-1][len("WGRAD_FORMS "):])
    assert not bad, bad


def test_the_switch_only_tables_name_every_switch_only_form():
    forms = {c["form"] for _env, cases in W.CHILDREN.values() for c in cases}
    assert {"tile_128_64", "tile_64_128", "pipe_128_128", "pipe_128_64", "pipe_64_128", "pipe_64_64", "nine_tap_4w"} <= forms
    assert {c["form"] for c in W.CHILDREN["per_tap"][1]} == {"mfma_vec", "tile_128_128"}


if __name__ == "__main__":
    _child(sys.argv[1])
