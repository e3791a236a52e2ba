"""The area-averaging resize of the multi-stream input path, host side (no GPU): the integer reference of
tests/area_resize_refs.py pinned to torch's float64 ``F.interpolate(mode="area")`` of the padded ``u8 / 255`` square, and the
plumbing of ``resize=`` through ``StagedRaggedImages``, ``prepare_streams``, the fusers and the pipeline's producer recipes.

The bound: the reference divides two integers that float32 holds exactly (sum <= 255 cnt < 2^24), so it is the real quotient,
a value in [0, 1], rounded once to float32: at most half an ulp of a value <= 1, 2^-25.  float64 evaluates the same quotient
to about 1e-16; 1e-12 covers that.  torch's own float32 ``area`` kernel is farther from float64 than that and is not used."""
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import area_resize_refs as ar, pixel_format_refs as pf

BOUND = 2.0 ** -25 + 1e-12

# (h, w, S): landscape, portrait, square; odd h - w; P < S, P == S, P == S + 1; a non-integer ratio; a window side of 63
CASES = [(480, 640, 416), (640, 480, 416), (37, 53, 8), (53, 37, 8), (9, 9, 8), (8, 8, 8), (5, 8, 8), (5, 7, 8), (3, 4, 8),
         (417, 417, 416), (300, 416, 416), (1000, 3, 16), (3, 1000, 16), (720, 1280, 608)]


def _frame(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _torch_area64(rgb, S, flip):
    square = torch.from_numpy(np.ascontiguousarray(ar.padded_square(rgb, flip))).permute(2, 0, 1)[None].double() / 255
    return F.interpolate(square, size=S, mode="area")[0].numpy()


@pytest.mark.parametrize("h, w, S", CASES)
@pytest.mark.parametrize("flip", [False, True])
def test_reference_is_float64_area_interpolation_rounded_once(h, w, S, flip):
    rgb = _frame(h, w, seed=h * 7 + w)
    got = ar.area_resize(rgb, S, flip)
    want = _torch_area64(rgb, S, flip)
    assert got.dtype == np.float32 and got.shape == (3, S, S)
    dev = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{h}x{w} -> {S} flip {flip}: max deviation {dev:.3e} (bound {BOUND:.3e})")
    assert dev <= BOUND
    assert np.array_equal(got, want.astype(np.float32)), "not the float64 result rounded to float32"


def test_windows():
    a, b = ar.windows(53, 8)
    assert a.tolist() == [0, 6, 13, 19, 26, 33, 39, 46] and b.tolist() == [7, 14, 20, 27, 34, 40, 47, 53]
    a, b = ar.windows(8, 8)
    assert (b - a).tolist() == [1] * 8 and a.tolist() == list(range(8))
    a, b = ar.windows(5, 8)                                   # P < S: one or two pixels
    assert set((b - a).tolist()) <= {1, 2} and a[0] == 0 and b[-1] == 5
    a, b = ar.windows(1000, 16)
    assert int((b - a).max()) == 63
    a, b = ar.windows(2039, 8)                                # the largest window the range rule P <= 255 S allows
    assert int((b - a).max()) == 256
    a, b = ar.windows(2040, 8)
    assert (b - a).tolist() == [255] * 8


@pytest.mark.parametrize("h, w", [(8, 8), (5, 8), (8, 3)])
def test_identity_size_is_u8_over_255(h, w):
    rgb = _frame(h, w, seed=3)
    for flip in (False, True):
        want = (torch.from_numpy(np.ascontiguousarray(ar.padded_square(rgb, flip))).permute(2, 0, 1).float() / 255).numpy()
        assert np.array_equal(ar.area_resize(rgb, 8, flip), want)


@pytest.mark.parametrize("h, w, S", [(37, 53, 8), (53, 36, 8), (5, 7, 8)])
def test_flip_is_the_resize_of_the_mirrored_square(h, w, S):
    rgb = _frame(h, w, seed=4)
    mirrored = np.ascontiguousarray(ar.padded_square(rgb, True))      # a square frame: no padding of its own
    assert mirrored.shape[0] == mirrored.shape[1]
    assert np.array_equal(ar.area_resize(rgb, S, True), ar.area_resize(mirrored, S, False))
    assert not np.array_equal(ar.area_resize(rgb, S, True), ar.area_resize(rgb, S, False))


def test_other_formats_go_through_their_rgb_conversion():
    for fmt in ("bgr", "nv12", "yuyv"):
        frame = pf.native_frame(fmt, 12, 10, seed=5)
        assert np.array_equal(ar.area_resize_native(frame, fmt, 8, True), ar.area_resize(pf.to_rgb_u8(frame, fmt), 8, True))


# ----------------------------------------------------------------------------------------------------------- plumbing
BAD_NAMES = ["", "bilinear", "AREA", 1, ("area",)]


@pytest.mark.parametrize("bad", BAD_NAMES)
def test_unknown_resize_is_refused_at_construction(bad):
    from millieye_amd import hip
    from millieye_amd.demo import FrameFuser, MultiStreamFuser, prepare_streams
    from millieye_amd.utils.datasets import StagedRaggedImages
    from tests.golden.make_golden import RADAR_CALIB
    frame = torch.zeros((4, 6, 3), dtype=torch.uint8)
    with pytest.raises(hip.MeError, match="resize"):
        StagedRaggedImages([frame], 8, resize=bad)
    with pytest.raises(hip.MeError, match="resize"):
        prepare_streams([frame], [[]], 1, img_size=8, resize=bad)
    with pytest.raises(hip.MeError, match="resize"):
        FrameFuser(None, RADAR_CALIB, resize=bad)
    with pytest.raises(hip.MeError, match="resize"):
        MultiStreamFuser(None, RADAR_CALIB, 2, resize=bad)


def test_resize_modes_are_exported():
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    from millieye_amd.utils import datasets
    from tests.golden.make_golden import RADAR_CALIB
    assert datasets.RESIZE_MODES == ("nearest", "area") and "RESIZE_MODES" in datasets.__all__
    for name in (None, "nearest", "area"):
        assert FrameFuser(None, RADAR_CALIB, resize=name).resize == name
        assert MultiStreamFuser(None, RADAR_CALIB, 2, resize=name).resize == name


def test_frame_beyond_the_range_is_refused_by_pack_naming_the_frame():
    from millieye_amd import hip
    from millieye_amd.utils.datasets import StagedRaggedImages
    ok = torch.zeros((2, 2040, 3), dtype=torch.uint8)          # P = 255 * 8: the limit
    bad = torch.zeros((2, 2041, 3), dtype=torch.uint8)
    StagedRaggedImages([ok, ok], 8, resize="area").pack()
    staged = StagedRaggedImages([ok, bad], 8, resize="area")   # (the constructor does not look at the frames)
    with pytest.raises(hip.MeError, match="frame 1.*255"):
        staged.pack()
    nv12 = torch.zeros((2042 * 3 // 2, 2), dtype=torch.uint8)   # a portrait picture of 2042 x 2 in its native layout
    with pytest.raises(hip.MeError, match="frame 0.*255"):
        StagedRaggedImages([nv12], 8, formats="nv12", resize="area").pack()
    # the nearest path has no such rule
    StagedRaggedImages([bad], 8).pack()
    StagedRaggedImages([bad], 8, resize="nearest").pack()


def test_resize_survives_pack_and_pickle():
    from millieye_amd.utils.datasets import StagedRaggedImages
    frames = [torch.from_numpy(_frame(5, 7, 1)), torch.from_numpy(_frame(6, 4, 2))]
    staged = StagedRaggedImages(frames, 8, [0, 1], resize="area")
    assert staged.resize == "area" and staged.formats is None
    back = pickle.loads(pickle.dumps(staged.pack(keep_frames=False)))
    assert back.resize == "area" and back.formats is None and back.frames == []
    assert back.desc.tolist() == [[0, 5, 7, 0, 0], [105, 6, 4, 1, 0]]      # [n,5], all RGB
    assert torch.equal(back.packed, torch.cat([f.reshape(-1) for f in frames]))
    for name in (None, "nearest"):
        assert pickle.loads(pickle.dumps(StagedRaggedImages(frames, 8, resize=name).pack())).resize == name


def test_area_with_formats_keeps_the_format_descriptor():
    from millieye_amd.utils.datasets import StagedRaggedImages
    fmts = ["nv12", "bgr", "yuyv", "rgb"]
    frames = [pf.native_frame(f, 4, 6, seed=i) for i, f in enumerate(fmts)]
    plain = StagedRaggedImages(frames, 8, [1, 0, 0, 1], formats=fmts).pack()
    area = StagedRaggedImages(frames, 8, [1, 0, 0, 1], formats=fmts, resize="area").pack()
    assert torch.equal(area.desc, plain.desc) and torch.equal(area.packed, plain.packed)
    assert area.desc[:, 4].tolist() == [2, 1, 3, 0]


def test_default_and_nearest_pack_as_before():
    """``resize=None`` and ``"nearest"``: the [n,4] descriptor without formats, the [n,5] one with them, the same bytes."""
    from millieye_amd.utils.datasets import StagedRaggedImages
    rgb = [torch.from_numpy(_frame(5, 7, 1)), torch.from_numpy(_frame(6, 4, 2)), torch.from_numpy(_frame(3, 3, 3))]
    want_desc = torch.tensor([[0, 5, 7, 0], [105, 6, 4, 1], [177, 3, 3, 0]], dtype=torch.int64)
    want_bytes = torch.cat([f.reshape(-1) for f in rgb])
    for name in (None, "nearest"):
        staged = StagedRaggedImages(rgb, 8, [0, 1, 0], resize=name).pack()
        assert staged.desc.dtype == torch.int64 and torch.equal(staged.desc, want_desc)
        assert staged.packed.dtype == torch.uint8 and torch.equal(staged.packed, want_bytes)
        assert staged.formats is None
    positional = StagedRaggedImages(rgb, 8, [0, 1, 0]).pack()
    assert torch.equal(positional.desc, want_desc) and torch.equal(positional.packed, want_bytes)
    fmts = ["yuyv", "nv12"]
    native = [pf.native_frame("yuyv", 4, 6, seed=1), pf.native_frame("nv12", 4, 6, seed=2)]
    want5 = torch.tensor([[0, 4, 6, 0, 3], [48, 4, 6, 1, 2]], dtype=torch.int64)
    for name in (None, "nearest"):
        staged = StagedRaggedImages(native, 8, [0, 1], formats=fmts, resize=name).pack()
        assert torch.equal(staged.desc, want5)
        assert torch.equal(staged.packed, torch.cat([torch.from_numpy(f).reshape(-1) for f in native]))


def test_to_cpu_still_raises():
    from millieye_amd import hip
    from millieye_amd.utils.datasets import StagedRaggedImages
    frame = torch.from_numpy(_frame(5, 7, 1))
    for name in (None, "nearest", "area"):
        with pytest.raises(hip.MeError, match="CUDA device required"):
            StagedRaggedImages([frame], 8, resize=name).to("cpu")
        with pytest.raises(hip.MeError, match="CUDA device required"):
            StagedRaggedImages([frame], 8, resize=name).pack().to(torch.device("cpu"))


def test_prepare_streams_and_fusers_stage_the_option():
    from millieye_amd.demo import FrameFuser, MultiStreamFuser, prepare_streams
    from tests.golden.make_golden import RADAR_CALIB
    frames = [_frame(30, 44, 1), _frame(40, 36, 2)]
    payload = prepare_streams(frames, [[], []], 2, img_size=16, pack=True, resize="area")
    assert payload["hw"] == [(30, 44), (40, 36)] and payload["img"].resize == "area"
    assert tuple(payload["img"].desc.shape) == (2, 5) and payload["img"].desc[:, 4].tolist() == [0, 0]
    default = prepare_streams(frames, [[], []], 2, img_size=16, pack=True)
    assert default["img"].resize is None and tuple(default["img"].desc.shape) == (2, 4)
    fuser = MultiStreamFuser(None, RADAR_CALIB, 2, img_size=16, resize="area", pixel_format=["rgb", "bgr"])
    img = fuser.prepare(frames, [[], []], pack=True)["img"]
    assert img.resize == "area" and img.desc[:, 4].tolist() == [0, 1]
    one = FrameFuser(None, RADAR_CALIB, img_size=16, resize="area").prepare(frames[0], [])
    assert one["hw"] == (30, 44) and one["img"].resize == "area" and one["img"].desc.tolist() == [[0, 30, 44, 0, 0]]
    nearest = FrameFuser(None, RADAR_CALIB, img_size=16, resize="nearest").prepare(frames[0], [])
    assert type(nearest["img"]).__name__ == "StagedImages"          # today's per-frame path
    with pytest.raises(Exception, match="frame 0.*255"):
        FrameFuser(None, RADAR_CALIB, img_size=1, resize="area").prepare(_frame(2, 256, 0), [])


def test_pipeline_hands_resize_to_its_producer():
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    from millieye_amd.pipeline import FusionPipeline
    from tests.golden.make_golden import RADAR_CALIB
    source = pf.NativeSource(1, ["nv12", "yuyv"])
    pipe = FusionPipeline(MultiStreamFuser(None, RADAR_CALIB, 2, img_size=64, pixel_format=["nv12", "yuyv"], resize="area"), source)
    factory = pickle.loads(pickle.dumps(pipe.prepare_factory))          # it travels to the producer by pickle
    payload = factory()(*source.step(0))
    assert payload["img"].resize == "area" and payload["img"].desc[:, 4].tolist() == [2, 3]
    plain = FusionPipeline(MultiStreamFuser(None, RADAR_CALIB, 2, img_size=64, pixel_format=["nv12", "yuyv"]), source)
    assert plain.prepare_factory()(*source.step(0))["img"].resize is None
    frames, radar = source.step(0)
    single = FusionPipeline(FrameFuser(None, RADAR_CALIB, img_size=64, pixel_format="nv12", resize="area"), source)
    one = pickle.loads(pickle.dumps(single.prepare_factory))()(frames[0], radar[0])
    assert one["img"].resize == "area" and one["img"].desc.tolist() == [[0, 32, 48, 0, 2]]
