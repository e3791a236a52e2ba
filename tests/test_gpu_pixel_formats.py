"""-m gpu: the pixel formats of the multi-stream input path on the device.  The governing property is exact:

    me_image_batch_formats_u8_f32 on a frame in format F  is torch.equal to
    the EXISTING me_image_batch_pad_resize_flip_u8_f32 on tests.pixel_format_refs.to_rgb_u8(frame, F)

for every format x picture size x output side x flip, for one ragged batch of all formats, and for every (Y, U, V) value class
(both clamps of each channel, the negative arithmetic shift).  Every output buffer is pre-filled with NaN; the source buffer
is allocated at exactly ``src_bytes``.  Invalid descriptors give an all-zero frame beside correct neighbours.  Then the option
through ``MultiStreamFuser`` (both splits), ``FrameFuser`` and ``FusionPipeline``: rows equal to those of the converted frames."""
import numpy as np
import pytest
import torch

from millieye_amd import synth
from tests import multistream_helpers as mh, pixel_format_refs as pf
from tests.golden.make_golden import RADAR_CALIB

pytestmark = pytest.mark.gpu

SIZES = ((2, 2), (2, 4), (4, 2), (4, 6), (6, 4), (8, 10))   # picture (h, w)
FMT_ID = {"rgb": 0, "bgr": 1, "nv12": 2, "yuyv": 3}
E_BADARG, E_NULLPTR, E_ALIGN, E_TOOBIG = -1, -2, -3, -4      # include/millieye_hip.h


def _launch(entry, packed, desc, n, side, src_bytes=None):
    """One call of ``entry`` on host ``packed`` bytes / ``desc`` rows: ``[n,3,side,side]`` on the host, NaN where nothing was
    written.  The device source holds exactly ``src_bytes`` bytes (default: all of ``packed``)."""
    from millieye_amd import hip
    src_bytes = int(packed.numel()) if src_bytes is None else int(src_bytes)
    d_src = packed[:src_bytes].contiguous().cuda()
    assert d_src.numel() == src_bytes
    d_desc = desc.contiguous().cuda()
    out = torch.full((n, 3, side, side), float("nan"), device="cuda", dtype=torch.float32)
    hip.check(getattr(hip.lib(), entry)(d_src.data_ptr(), src_bytes, d_desc.data_ptr(), n, out.data_ptr(), side,
                                        hip.stream_ptr()), entry)
    torch.cuda.synchronize()
    return out.cpu()


def _native(frames, fmts, side, flips=None):
    from millieye_amd.utils.datasets import StagedRaggedImages
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], side, flips, formats=fmts).pack()
    return _launch("me_image_batch_formats_u8_f32", staged.packed, staged.desc, len(frames), side), staged


def _converted(frames, fmts, side, flips=None):
    """The yardstick: the existing ragged-batch entry point on the frames converted to RGB by the numpy reference."""
    from millieye_amd.utils.datasets import StagedRaggedImages
    rgb = [torch.from_numpy(pf.to_rgb_u8(f, fmt)) for f, fmt in zip(frames, fmts)]
    staged = StagedRaggedImages(rgb, side, flips).pack()
    assert tuple(staged.desc.shape) == (len(frames), 4)
    return _launch("me_image_batch_pad_resize_flip_u8_f32", staged.packed, staged.desc, len(frames), side)


def _equal(got, want, what):
    assert not torch.isnan(want).any(), f"{what}: the yardstick left elements unwritten"
    assert not torch.isnan(got).any(), f"{what}: elements left unwritten"
    assert got.dtype == want.dtype and got.shape == want.shape
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: {got[i].item()!r} vs "
                             f"{want[i].item()!r} (x 255: {got[i].item() * 255:.3f} vs {want[i].item() * 255:.3f})")


@pytest.mark.parametrize("fmt", pf.FORMATS)
def test_every_format_shape_side_and_flip(hip_lib, fmt):
    """Sides 4 and 8: the float4 path, down and up; 6: the scalar path; max(h, w): the identity branch (2, 10: scalar too)."""
    for k, (h, w) in enumerate(SIZES):
        frame = pf.native_frame(fmt, h, w, seed=100 + k)
        for side in sorted({4, 6, 8, max(h, w)}):
            for flip in (0, 1):
                got, _ = _native([frame], [fmt], side, [flip])
                _equal(got, _converted([frame], [fmt], side, [flip]), f"{fmt} {h}x{w} -> {side} flip {flip}")


@pytest.mark.parametrize("side", [8, 6])
def test_one_ragged_batch_of_all_formats(hip_lib, side):
    fmts = ["nv12", "rgb", "yuyv", "bgr", "yuyv", "nv12", "bgr"]
    sizes = [(4, 6), (3, 5), (5, 2), (2, 7), (8, 10), (6, 4), (9, 9)]
    flips = [0, 1, 1, 0, 0, 1, 1]
    frames = [pf.native_frame(f, h, w, seed=200 + i) for i, (f, (h, w)) in enumerate(zip(fmts, sizes))]
    got, staged = _native(frames, fmts, side, flips)
    assert staged.desc[:, 4].tolist() == [FMT_ID[f] for f in fmts]
    _equal(got, _converted(frames, fmts, side, flips), f"batch -> {side}")
    for i in range(len(frames)):   # ... and the per-frame results
        one, _ = _native([frames[i]], [fmts[i]], side, [flips[i]])
        assert torch.equal(got[i], one[0]), f"frame {i} ({fmts[i]}) of the batch differs from its own launch"


def _pairs_frame(luma0, luma1, u, v, w):
    """YUYV frame of width ``w`` whose pixel pairs are ``(luma0[k], u[k], luma1[k], v[k])``, in raster order."""
    quad = np.stack([luma0, u, luma1, v], 1).astype(np.uint8)
    assert quad.shape[0] % (w // 2) == 0
    return quad.reshape(-1, w, 2)


def _value_frames():
    a, b = np.divmod(np.arange(65536), 256)
    mid = np.full(65536, 128)
    yield "all (Y, V) at U = 128", _pairs_frame(a, a, mid, b, 512)
    yield "all (Y, U) at V = 128", _pairs_frame(a, a, b, mid, 512)
    lumas = np.array([0, 15, 16, 17, 128, 235, 255])
    k = np.arange(8 * 65536)                                  # 7 x 65536 pairs, the eighth block repeats the first
    luma = lumas[(k // 65536) % 7]
    yield "all (U, V) at 7 lumas", _pairs_frame(luma, luma, (k // 256) % 256, k % 256, 1024)


def test_value_coverage(hip_lib):
    """Three YUYV frames holding every (Y, V) pair at U = 128, every (Y, U) pair at V = 128 and every (U, V) pair at Y in
    {0, 15, 16, 17, 128, 235, 255}, at the identity size: every source pixel reaches the output."""
    for what, frame in _value_frames():
        h, w = frame.shape[:2]
        yuv = pf.yuv444(frame, "yuyv").reshape(-1, 3)
        seen = len(np.unique(yuv.astype(np.int64) @ np.array([65536, 256, 1])))
        assert seen == (7 * 65536 if "lumas" in what else 65536), what
        rgb = pf.to_rgb_u8(frame, "yuyv").astype(np.int64)
        assert rgb.min() == 0 and rgb.max() == 255
        side = max(h, w)
        got, _ = _native([frame], ["yuyv"], side)
        _equal(got, _converted([frame], ["yuyv"], side), what)


def _neighbours():
    fmts = ["yuyv", "nv12", "bgr"]
    frames = [pf.native_frame("yuyv", 4, 6, seed=300), pf.native_frame("nv12", 4, 6, seed=301),
              pf.native_frame("bgr", 5, 3, seed=302)]
    return frames, fmts


INVALID = {
    "offset past the buffer": lambda desc, total: desc[1].__setitem__(0, total + 5),
    "negative offset": lambda desc, total: desc[1].__setitem__(0, -1),
    "unknown format id 4": lambda desc, total: desc[1].__setitem__(4, 4),
    "unknown format id -1": lambda desc, total: desc[1].__setitem__(4, -1),
    "unknown format id 2^32 + 2": lambda desc, total: desc[1].__setitem__(4, (1 << 32) + 2),
    "odd w for yuyv": lambda desc, total: (desc[1].__setitem__(4, 3), desc[1].__setitem__(2, 5)),
    "odd w for nv12": lambda desc, total: desc[1].__setitem__(2, 5),
    "odd h for nv12": lambda desc, total: desc[1].__setitem__(1, 3),
    "h = w = 2^30": lambda desc, total: (desc[1].__setitem__(1, 1 << 30), desc[1].__setitem__(2, 1 << 30)),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_descriptor_gives_padding(hip_lib, case):
    """Frame 1 of 3 gets a bad descriptor: it comes out all zero (never read), frames 0 and 2 as without it."""
    from millieye_amd.utils.datasets import StagedRaggedImages
    frames, fmts = _neighbours()
    side = 8
    want = _converted(frames, fmts, side)
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], side, formats=fmts).pack()
    desc, total = staged.desc.clone(), int(staged.packed.numel())
    INVALID[case](desc, total)
    assert not torch.equal(desc, staged.desc)
    got = _launch("me_image_batch_formats_u8_f32", staged.packed, desc, 3, side)
    assert not torch.isnan(got).any()
    assert torch.equal(got[1], torch.zeros_like(got[1])), f"{case}: the frame is not padding"
    assert want[1].abs().sum() > 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), f"{case}: a neighbour changed"


def test_nv12_plane_one_byte_past_the_buffer(hip_lib):
    """The last frame is NV12 and ``src_bytes`` (and the buffer) end one byte before its UV plane does."""
    from millieye_amd.utils.datasets import StagedRaggedImages
    frames, fmts = _neighbours()
    frames, fmts = [frames[0], frames[2], frames[1]], [fmts[0], fmts[2], fmts[1]]
    side = 8
    want = _converted(frames, fmts, side)
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], side, formats=fmts).pack()
    total = int(staged.packed.numel())
    assert int(staged.desc[2, 0]) + 4 * 6 * 3 // 2 == total
    whole = _launch("me_image_batch_formats_u8_f32", staged.packed, staged.desc, 3, side)
    _equal(whole, want, "the whole buffer")
    short = _launch("me_image_batch_formats_u8_f32", staged.packed, staged.desc, 3, side, src_bytes=total - 1)
    assert torch.equal(short[2], torch.zeros_like(short[2])) and want[2].abs().sum() > 0
    assert torch.equal(short[0], want[0]) and torch.equal(short[1], want[1])


def test_argument_checks_are_those_of_the_rgb_entry_point(hip_lib):
    from millieye_amd import hip
    lib = hip.lib()
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    desc = torch.tensor([[0, 2, 2, 0, 0]], dtype=torch.int64, device="cuda")
    out = torch.zeros(3 * 8 * 8 + 4, dtype=torch.float32, device="cuda")
    for entry in ("me_image_batch_formats_u8_f32", "me_image_batch_pad_resize_flip_u8_f32"):
        fn = getattr(lib, entry)
        assert fn(src.data_ptr(), 64, desc.data_ptr(), 0, out.data_ptr(), 8, None) == 0             # n = 0: nothing to do
        assert fn(None, 64, desc.data_ptr(), 1, out.data_ptr(), 8, None) == E_NULLPTR
        assert fn(src.data_ptr(), 0, desc.data_ptr(), 1, out.data_ptr(), 8, None) == E_BADARG
        assert fn(src.data_ptr(), 64, desc.data_ptr(), 65536, out.data_ptr(), 8, None) == E_BADARG
        assert fn(src.data_ptr(), 64, desc.data_ptr(), 1, out.data_ptr(), 1 << 15, None) == E_TOOBIG
        assert fn(src.data_ptr(), 64, desc.data_ptr(), 1, out.data_ptr() + 4, 8, None) == E_ALIGN
    torch.cuda.synchronize()


def test_staged_ragged_images_to(hip_lib):
    """``.to()`` of the packed and of the unpacked object, against the default path on the converted frames."""
    from millieye_amd.utils.datasets import StagedRaggedImages
    fmts = ["nv12", "bgr", "yuyv", "rgb"]
    frames = [pf.native_frame(f, h, w, seed=400 + i) for i, (f, (h, w)) in enumerate(zip(fmts, [(32, 48), (40, 36), (30, 44), (7, 9)]))]
    want = StagedRaggedImages([torch.from_numpy(pf.to_rgb_u8(f, fmt)) for f, fmt in zip(frames, fmts)], 64, [0, 1, 0, 1]).to("cuda")
    got = StagedRaggedImages(frames, 64, [0, 1, 0, 1], formats=fmts).to("cuda")
    packed = StagedRaggedImages(frames, 64, [0, 1, 0, 1], formats=fmts).pack(keep_frames=False).to("cuda")
    assert torch.equal(got, want) and torch.equal(packed, want) and float(want.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------- fusers and pipeline
_shared = {}


def _net():
    if "net" not in _shared:
        from tests.test_gpu_network import _build
        net = _build("demo", "yolov3-tiny-12", 0.1).eval()
        synth.fill_network_(net, "demo", cls0_bias=3.0, cls_bias=-4.0)
        _shared["net"] = net.to(net.device)
    return _shared["net"]


def _same_step(got, want, what):
    assert len(got) == len(want)
    for s, ((rows, info), (rows_w, info_w)) in enumerate(zip(got, want)):
        assert rows.dtype == rows_w.dtype and tuple(rows.shape) == tuple(rows_w.shape) and torch.equal(rows, rows_w), \
            f"{what} stream {s}: rows differ"
        assert sorted(info) == sorted(info_w)
        for key in ("mode", "points", "radar_boxes"):
            assert info[key] == info_w[key], f"{what} stream {s}: {key}"
        assert np.array_equal(info["proposals"], info_w["proposals"])


FUSER_FORMATS = ["nv12", "bgr", "yuyv"]


@pytest.mark.parametrize("split", ["forwards", "frame_modes"])
def test_multi_stream_fuser(hip_lib, split):
    from millieye_amd.demo import MultiStreamFuser
    from tests import radar_scene_helpers as rs
    net = _net()
    sizes = [(32, 48), (40, 36), (30, 44)]
    frames = [pf.native_frame(fmt, h, w, seed=500 + s, dark=s != 1) for s, (fmt, (h, w)) in enumerate(zip(FUSER_FORMATS, sizes))]
    rgb = [pf.to_rgb_u8(f, fmt) for f, fmt in zip(frames, FUSER_FORMATS)]
    native = MultiStreamFuser(net, RADAR_CALIB, 3, model_mode=3, min_hits=mh.MIN_HITS, split=split, pixel_format=FUSER_FORMATS)
    plain = MultiStreamFuser(net, RADAR_CALIB, 3, model_mode=3, min_hits=mh.MIN_HITS, split=split)
    rows_total = 0
    for f in range(3):
        radar = [rs.grid_radar(s, f) for s in range(3)]
        got, want = native(frames, radar), plain(rgb, radar)
        _same_step(got, want, f"{split} step {f}")
        assert [info["mode"] for _r, info in got] == [0, 1, 0]
        rows_total += sum(len(r) for r, _i in got)
    assert rows_total > 0


def test_frame_fuser_nv12(hip_lib):
    from millieye_amd.demo import FrameFuser
    net = _net()
    rows_total = 0
    for k, dark in enumerate((True, False)):
        frame = pf.native_frame("nv12", 32, 48, seed=600 + k, dark=dark)
        native = FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=mh.MIN_HITS, pixel_format="nv12")
        plain = FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=mh.MIN_HITS)
        for f in range(2):
            got, want = native(frame, mh.stream_radar(0, f)), plain(pf.to_rgb_u8(frame, "nv12"), mh.stream_radar(0, f))
            _same_step([got], [want], f"dark={dark} step {f}")
            assert got[1]["mode"] == (0 if dark else 1)
            rows_total += len(got[0])
    assert rows_total > 0


def test_pipeline_nv12(hip_lib):
    from millieye_amd.demo import MultiStreamFuser
    from millieye_amd.pipeline import FusionPipeline
    net = _net()
    steps, n = 3, 2
    source = pf.NativeSource(steps, ["nv12"] * n)
    local = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, pixel_format="nv12")
    want = [local(*source.step(f)) for f in range(steps)]
    piped = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, pixel_format="nv12")
    pipe = FusionPipeline(piped, source, skip_to_newest=False)
    got = list(pipe)
    assert [info["frame_idx"] for _r, info in got] == list(range(steps)) and pipe.stats["dropped"] == 0
    for f, (results, _info) in enumerate(got):
        _same_step(results, want[f], f"step {f}")
    assert sum(len(r) for step in want for r, _i in step) > 0
