"""-m gpu: ``me_image_batch_area_u8_f32`` - the area-averaging resize of the multi-stream input path - on the device, through
the C ABI and through ``resize="area"`` of the staging class, the fusers and the two-process pipeline.  The governing property
is exact: every output equals the integer reference of tests/area_resize_refs.py (pinned to torch's float64 ``area``
interpolation by tests/test_area_resize_cpu.py) under ``torch.equal``, no tolerance.

Every output buffer is pre-filled with NaN between two sentinel margins that must come back untouched; the packed source lies
at an odd offset inside a larger device buffer of 255s, so that a read outside ``[src, src + src_bytes)`` changes a sum
instead of faulting.

The range rule ``P <= 255 S`` makes the 1 x 4099 frame of the mixed launch (sides 8 and 6) an invalid descriptor there: it comes
out all zero, as the header says.  ``test_rows_longer_than_a_segment`` runs rows of that length inside the range (sides 20 and
18), and ``test_window_at_the_limit`` adds 2 x 2039 -> 8, whose windows are 256 wide (2 x 2040 -> 8 gives exactly 255)."""
import numpy as np
import pytest
import torch

from millieye_amd import synth
from tests import area_resize_refs as ar, multistream_helpers as mh, pixel_format_refs as pf
from tests.golden.make_golden import RADAR_CALIB

pytestmark = pytest.mark.gpu

FMT_ID = {"rgb": 0, "bgr": 1, "nv12": 2, "yuyv": 3}
E_BADARG, E_NULLPTR, E_ALIGN, E_TOOBIG = -1, -2, -3, -4      # include/millieye_hip.h
FRONT, BACK = 4099, 4096       # bytes of 255 around the packed source (an odd offset: src itself is not aligned)
MARGIN, SENTINEL = 64, -7.0    # floats around the output (a multiple of 4: the output stays 16-byte aligned)


def _launch(entry, packed, desc, n, side, src_bytes=None):
    """One call of ``entry`` on host ``packed`` bytes / ``desc`` rows: ``[n,3,side,side]`` on the host, NaN where nothing was
    written.  Asserts that the sentinel margins around the output are untouched."""
    from millieye_amd import hip
    src_bytes = int(packed.numel()) if src_bytes is None else int(src_bytes)
    big = torch.full((FRONT + int(packed.numel()) + BACK,), 255, dtype=torch.uint8)
    big[FRONT:FRONT + packed.numel()] = packed
    d_big = big.cuda()
    d_desc = desc.contiguous().cuda()
    count = n * 3 * side * side
    buf = torch.full((MARGIN + count + MARGIN,), SENTINEL, device="cuda", dtype=torch.float32)
    buf[MARGIN:MARGIN + count] = float("nan")
    hip.check(getattr(hip.lib(), entry)(d_big.data_ptr() + FRONT, src_bytes, d_desc.data_ptr(), n,
                                        buf.data_ptr() + 4 * MARGIN, side, hip.stream_ptr()), entry)
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:MARGIN] == SENTINEL).all()) and bool((host[MARGIN + count:] == SENTINEL).all()), \
        f"{entry}: wrote outside the output"
    return host[MARGIN:MARGIN + count].reshape(n, 3, side, side).clone()


def _stage(frames, fmts, side, flips=None):
    from millieye_amd.utils.datasets import StagedRaggedImages
    return StagedRaggedImages([torch.from_numpy(f) for f in frames], side, flips, formats=fmts, resize="area").pack()


def _area(frames, fmts, side, flips=None):
    staged = _stage(frames, fmts, side, flips)
    return _launch("me_image_batch_area_u8_f32", staged.packed, staged.desc, len(frames), side)


def _reference(frames, fmts, side, flips=None):
    flips = flips or [0] * len(frames)
    return torch.from_numpy(np.stack([ar.area_resize_native(f, fmt, side, bool(flip))
                                      for f, fmt, flip in zip(frames, fmts, flips)]))


def _equal(got, want, what):
    assert not torch.isnan(want).any()
    assert not torch.isnan(got).any(), f"{what}: elements left unwritten"
    assert got.dtype == want.dtype and got.shape == want.shape
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: {got[i].item()!r} vs "
                             f"{want[i].item()!r}")


# (format, h, w, flip): the first frame has 105 bytes, every other one an even number, so every later frame starts at an odd
# byte offset; the 1 x 4099 frame (12297 bytes) is the last one
MIXED = [("rgb", 5, 7, 0),       # P < 8, P = 6 + 1
         ("bgr", 9, 8, 1),       # P = 8 + 1, portrait, odd pad difference
         ("nv12", 8, 6, 0),      # P == 8, portrait
         ("yuyv", 37, 54, 1),    # landscape, odd pad difference, a non-integer ratio
         ("rgb", 1000, 3, 1),    # vertical windows of 125 / 167 rows
         ("yuyv", 6, 6, 0),      # square, P == 6
         ("bgr", 53, 36, 0),     # portrait, odd pad difference
         ("nv12", 40, 64, 1),    # landscape
         ("rgb", 6, 4, 0),       # P == 6, P < 8
         ("rgb", 8, 8, 1),       # square, P == 8
         ("bgr", 4, 2, 1),       # P < 6
         ("rgb", 4, 6, 0),       # -> its descriptor will point outside the buffer
         ("nv12", 4, 6, 0),      # -> its descriptor will claim an odd h
         ("rgb", 1, 4099, 0)]    # a row longer than any segment, w no multiple of 4; beyond the range at sides 8 and 6
OUTSIDE, ODD_H, LONG = 11, 12, 13


@pytest.mark.parametrize("side", [8, 6])
def test_one_ragged_launch_of_everything(hip_lib, side):
    """Side 8: the float4 stores; side 6: the scalar ones."""
    fmts = [m[0] for m in MIXED]
    flips = [m[3] for m in MIXED]
    frames = [pf.native_frame(f, h, w, seed=700 + i) for i, (f, h, w, _flip) in enumerate(MIXED)]
    assert frames[0].size == 105
    from millieye_amd.utils.datasets import StagedRaggedImages
    # (packed without resize=: pack() itself refuses the 1 x 4099 frame for the area resize; the bytes and rows are the same)
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], side, flips, formats=fmts).pack()
    desc, total = staged.desc.clone(), int(staged.packed.numel())
    assert all(int(o) % 2 == 1 for o in desc[1:, 0]) and desc[:, 4].tolist() == [FMT_ID[f] for f in fmts]
    desc[OUTSIDE, 0] = total - 71          # 72 bytes from there: one byte past the end
    desc[ODD_H, 1] = 5
    want = _reference(frames, fmts, side, flips)
    assert all(float(want[i].abs().sum()) > 0 for i in range(len(MIXED)))
    assert 4099 > 255 * side
    for i in (OUTSIDE, ODD_H, LONG):       # invalid descriptors and the frame beyond P <= 255 S: never read, all zero
        want[i] = 0
    got = _launch("me_image_batch_area_u8_f32", staged.packed, desc, len(MIXED), side)
    for i, m in enumerate(MIXED):
        _equal(got[i], want[i], f"frame {i} {m} -> {side}")
    again = _launch("me_image_batch_area_u8_f32", staged.packed, desc, len(MIXED), side)
    assert torch.equal(again, got), "a second launch gives other bits"
    # a frame of the batch equals its own launch
    for i in (0, 3, 7):
        one = _area([frames[i]], [fmts[i]], side, [flips[i]])
        assert torch.equal(one[0], got[i]), f"frame {i} of the batch differs from its own launch"


@pytest.mark.parametrize("side", [20, 18])
def test_rows_longer_than_a_segment(hip_lib, side):
    """Rows of 4099 / 4100 pixels inside the range (P <= 255 * 18): several column segments per output row, for the 16-byte
    RGB lanes and for both YUV layouts; windows of 205 .. 229 pixels."""
    cases = [("rgb", 5, 7, 0), ("rgb", 1, 4099, 0), ("bgr", 3, 4099, 1), ("yuyv", 2, 4100, 1), ("nv12", 2, 4100, 0),
             ("yuyv", 4098, 2, 0), ("nv12", 4098, 2, 1)]
    fmts, flips = [c[0] for c in cases], [c[3] for c in cases]
    frames = [pf.native_frame(f, h, w, seed=800 + i) for i, (f, h, w, _flip) in enumerate(cases)]
    got = _area(frames, fmts, side, flips)
    want = _reference(frames, fmts, side, flips)
    for i, c in enumerate(cases):
        assert float(want[i].abs().sum()) > 0
        _equal(got[i], want[i], f"frame {i} {c} -> {side}")


def test_window_at_the_limit(hip_lib):
    """2 x 2040 -> 8 (P = 255 S, the limit of the range) with all pixels 255: the two picture rows fall into output rows 3
    and 4, every window there holds one row of 255 pixels of 255 among 255 x 255: (float)65025 / (float)(255 * 65025).
    2 x 2039 -> 8: windows of 256 x 256, the largest there are; 2039 x 2 of 255s and an NV12 frame of 2038 x 2 fill windows of
    256 rows, the largest column sums."""
    white = np.full((2, 2040, 3), 255, np.uint8)
    got = _area([white], ["rgb"], 8)
    _equal(got, _reference([white], ["rgb"], 8), "2 x 2040 white")
    quotient = float(np.float32(65025) / np.float32(255 * 65025))
    assert got[0, :, 3:5].unique().tolist() == [quotient] and float(got[0, :, :3].abs().sum()) == 0 \
        and float(got[0, :, 5:].abs().sum()) == 0
    a, b = ar.windows(2039, 8)
    assert int((b - a).max()) == 256
    frames = [pf.native_frame(f, 2, 2039 + (f != "rgb"), seed=810 + i) for i, f in enumerate(("rgb", "yuyv"))]
    frames.append(np.full((2, 2039, 3), 255, np.uint8))
    frames.append(np.full((2039, 2, 3), 255, np.uint8))     # column sums of 256 rows of 255: the largest there are
    frames.append(np.full((2038 * 3 // 2, 2), 235, np.uint8))   # NV12, 2038 x 2
    fmts, flips = ["rgb", "yuyv", "bgr", "rgb", "nv12"], [1, 0, 0, 1, 0]
    _equal(_area(frames, fmts, 8, flips), _reference(frames, fmts, 8, flips), "2 x 2039 / 2040")


def test_1080p_to_416(hip_lib):
    frames = [pf.native_frame("rgb", 1080, 1920, seed=820), pf.native_frame("nv12", 1080, 1920, seed=821)]
    fmts, flips = ["rgb", "nv12"], [0, 1]
    _equal(_area(frames, fmts, 416, flips), _reference(frames, fmts, 416, flips), "1080 x 1920 -> 416")


@pytest.mark.parametrize("side", [8, 6])
def test_identity_size_equals_the_nearest_entry_point(hip_lib, side):
    from millieye_amd.utils.datasets import StagedRaggedImages
    sizes = {"rgb": (side, side - 3), "bgr": (side - 1, side), "nv12": (side, side - 2), "yuyv": (side - 2, side)}
    fmts = list(sizes)
    frames = [pf.native_frame(f, *sizes[f], seed=830 + i) for i, f in enumerate(fmts)]
    flips = [0, 1, 1, 0]
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], side, flips, formats=fmts).pack()
    nearest = _launch("me_image_batch_formats_u8_f32", staged.packed, staged.desc, 4, side)
    got = _launch("me_image_batch_area_u8_f32", staged.packed, staged.desc, 4, side)
    _equal(got, nearest, f"P == {side}")
    _equal(got, _reference(frames, fmts, side, flips), f"P == {side} against the reference")


def test_argument_checks_are_those_of_the_other_batch_entry_points(hip_lib):
    from millieye_amd import hip
    fn = hip.lib().me_image_batch_area_u8_f32
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    desc = torch.tensor([[0, 2, 2, 0, 0]], dtype=torch.int64, device="cuda")
    out = torch.zeros(3 * 8 * 8 + 4, dtype=torch.float32, device="cuda")
    assert fn(src.data_ptr(), 64, desc.data_ptr(), 0, out.data_ptr(), 8, None) == 0             # n = 0: nothing to do
    assert fn(None, 64, desc.data_ptr(), 1, out.data_ptr(), 8, None) == E_NULLPTR
    assert fn(src.data_ptr(), 0, desc.data_ptr(), 1, out.data_ptr(), 8, None) == E_BADARG
    assert fn(src.data_ptr(), 64, desc.data_ptr(), 65536, out.data_ptr(), 8, None) == E_BADARG
    assert fn(src.data_ptr(), 64, desc.data_ptr(), 1, out.data_ptr(), 1 << 15, None) == E_TOOBIG
    assert fn(src.data_ptr(), 64, desc.data_ptr(), 1, out.data_ptr() + 4, 8, None) == E_ALIGN
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0


def test_staged_ragged_images_to_and_refusals(hip_lib):
    from millieye_amd import hip
    from millieye_amd.utils.datasets import StagedRaggedImages
    fmts = ["nv12", "bgr", "yuyv", "rgb"]
    frames = [pf.native_frame(f, h, w, seed=840 + i) for i, (f, (h, w)) in enumerate(zip(fmts, [(32, 48), (40, 36), (30, 44), (7, 9)]))]
    flips = [0, 1, 0, 1]
    want = _reference(frames, fmts, 16, flips)
    got = StagedRaggedImages(frames, 16, flips, formats=fmts, resize="area").to("cuda")
    packed = StagedRaggedImages(frames, 16, flips, formats=fmts, resize="area").pack(keep_frames=False).to("cuda")
    assert got.is_cuda and torch.equal(got.cpu(), want) and torch.equal(packed.cpu(), want)
    rgb = [torch.from_numpy(pf.to_rgb_u8(f, fmt)) for f, fmt in zip(frames, fmts)]
    assert torch.equal(StagedRaggedImages(rgb, 16, flips, resize="area").to("cuda").cpu(), want)      # formats=None: all RGB
    nearest = StagedRaggedImages(rgb, 16, flips, resize="nearest").to("cuda")
    assert torch.equal(nearest, StagedRaggedImages(rgb, 16, flips).to("cuda")) and not torch.equal(nearest.cpu(), want)
    for bad in ("", "bilinear", 1):
        with pytest.raises(hip.MeError, match="resize"):
            StagedRaggedImages(rgb, 16, resize=bad)
    with pytest.raises(hip.MeError, match="CUDA device required"):
        StagedRaggedImages(rgb, 16, resize="area").to("cpu")
    empty = StagedRaggedImages([], 16, resize="area").to("cuda")
    assert empty.is_cuda and tuple(empty.shape) == (0, 3, 16, 16) and empty.dtype == torch.float32


# ------------------------------------------------------------------------------------------------- fusers and pipeline
_shared = {}


def _net():
    if "net" not in _shared:
        from tests.test_gpu_network import _build
        net = _build("demo", "yolov3-tiny-12", 0.1).eval()
        synth.fill_network_(net, "demo", cls0_bias=3.0, cls_bias=-4.0)
        _shared["net"] = net.to(net.device)
    return _shared["net"]


def _stream_reference(streams):
    if ("want", streams) not in _shared:
        _shared[("want", streams)] = torch.from_numpy(np.stack([ar.area_resize(mh.stream_frame(s), 416) for s in range(streams)]))
    return _shared[("want", streams)]


def _same_step(got, want, what):
    assert len(got) == len(want)
    for s, ((rows, info), (rows_w, info_w)) in enumerate(zip(got, want)):
        assert rows.dtype == rows_w.dtype and tuple(rows.shape) == tuple(rows_w.shape) and torch.equal(rows, rows_w), \
            f"{what} stream {s}: rows differ"
        for key in ("mode", "points", "radar_boxes"):
            assert info[key] == info_w[key], f"{what} stream {s}: {key}"


def test_multi_stream_fuser_at_the_identity_size(hip_lib):
    """416 x 300 and 300 x 416 frames: P == S, where ``"area"`` gives the bits of the nearest path - the rows are the default
    fuser's."""
    from millieye_amd.demo import MultiStreamFuser
    net = _net()
    n = 3
    frames = [pf.native_frame("rgb", *hw, seed=850 + s, dark=s != 1) for s, hw in enumerate([(416, 300), (300, 416), (416, 300)])]
    area = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, resize="area")
    plain = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS)
    rows_total = 0
    for f in range(3):
        radar = [mh.stream_radar(s, f) for s in range(n)]
        got, want = area(frames, radar), plain(frames, radar)
        _same_step(got, want, f"step {f}")
        assert [info["mode"] for _r, info in got] == [0, 1, 0]
        rows_total += sum(len(r) for r, _i in got)
    assert rows_total > 0


def test_multi_stream_fuser_image_is_the_area_image(hip_lib):
    """480 x 640 and 360 x 480 frames: the staged image is the reference's, not the nearest one, and a step runs on it."""
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    net = _net()
    n = 3
    frames = [mh.stream_frame(s) for s in range(n)]
    fuser = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, resize="area")
    payload = fuser.prepare(frames, [mh.stream_radar(s, 0) for s in range(n)])
    img = payload["img"].to(fuser.device)
    assert img.is_cuda and torch.equal(img.cpu(), _stream_reference(n))
    nearest = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS).prepare(frames, [[]] * n)["img"].to(fuser.device)
    assert nearest.shape == img.shape and not torch.equal(nearest, img)
    results = fuser.infer(payload)
    assert len(results) == n and all(rows.shape[1] == 7 for rows, _info in results)
    # the auto mode's mean is that of the area-resized image
    assert [info["mode"] for _r, info in results] == [0 if float(_stream_reference(n)[s].mean()) < 0.08 else 1 for s in range(n)]
    single = FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=mh.MIN_HITS, resize="area")
    one = single.prepare(frames[1], mh.stream_radar(1, 0))
    assert torch.equal(one["img"].to(fuser.device).cpu()[0], _stream_reference(n)[1])
    rows, info = single.infer(one)
    assert rows.shape[1] == 7 and info["mode"] == results[1][1]["mode"]


def test_pipeline_carries_resize_to_its_producer(hip_lib):
    from millieye_amd.demo import MultiStreamFuser
    from millieye_amd.pipeline import FusionPipeline
    net = _net()
    n = 2
    source = ar.StreamSource(1, n)
    fuser = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, resize="area")
    seen = []

    def infer(payload):
        seen.append((payload["img"].resize, payload["img"].frames, payload["img"].to(fuser.device).cpu()))
        return fuser.infer(payload)

    got = list(FusionPipeline(fuser, source, infer=infer, skip_to_newest=False))
    assert len(got) == 1 and len(seen) == 1
    resize, frames, img = seen[0]
    assert resize == "area" and frames == []          # packed by the producer process
    assert torch.equal(img, _stream_reference(n))
    local = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, resize="area")(*source.step(0))
    _same_step(got[0][0], local, "piped step")
