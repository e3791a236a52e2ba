"""The pixel formats of the multi-stream input path, host side (no GPU): the numpy reference of tests/pixel_format_refs.py
pinned by known answers, the float formula and hand-written chroma addressing tables; ``StagedRaggedImages.pack`` with
``formats=``; the picture-size helper; ``prepare_streams(pixel_format=)``; every refused case.

Known answers, each worked out by hand from the definition (``>> 20`` of the sums below, then the clamp):
  (16,128,128)   y = 0:            R = G = B = 524288 >> 20 = 0
  (235,128,128)  y = 267298698:    267822986 >> 20 = 255 (255.42)
  (81,90,240)    y = 79335230, u = -38, v = 112:   R = 267294542 >> 20 = 254 (254.91), G = -39852 >> 20 = -1 -> 0,
                 B = -549470 >> 20 = -1 -> 0.  Pure red of the float matrix comes out as 254, not 255: the conversion truncates
                 after adding one half, and 254.41 + 0.5 stays under 255.
  (145,54,34)    y = 157449918, u = -74, v = -94:  R = 662668 >> 20 = 0, G = 268447936 >> 20 = 256 -> 255,
                 B = 1388282 >> 20 = 1 (0.82 + 0.5 = 1.32).  Pure green comes out with blue 1, not 0.
  (41,240,110)   y = 30513550, u = 112, v = -18:   R = 914352 >> 20 = 0, G = 463478 >> 20 = 0, B = 268032750 >> 20 = 255.
The two expected values that differ from the round figures (254 and 1) were corrected here, not the reference."""
import numpy as np
import pytest
import torch

from tests import pixel_format_refs as pf


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("yuv, rgb", [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)),
                                      ((81, 90, 240), (254, 0, 0)), ((145, 54, 34), (0, 255, 1)),
                                      ((41, 240, 110), (0, 0, 255))])
def test_known_answers(yuv, rgb):
    assert tuple(pf.yuv_to_rgb([yuv])[0].tolist()) == rgb


def test_luma_below_16_behaves_as_16():
    rng = np.random.RandomState(0)
    uv = rng.randint(0, 256, (4096, 2))
    at16 = pf.yuv_to_rgb(np.concatenate([np.full((4096, 1), 16), uv], 1))
    for luma in (0, 1, 7, 15):
        assert np.array_equal(pf.yuv_to_rgb(np.concatenate([np.full((4096, 1), luma), uv], 1)), at16)


def test_reference_agrees_with_the_float_formula():
    """R = 1.164 (Y - 16) + 1.596 (V - 128), G = 1.164 (Y - 16) - 0.813 (V - 128) - 0.391 (U - 128), B = 1.164 (Y - 16) +
    2.018 (U - 128), rounded and clamped, within +/- 1 (the integer coefficients are these times 2^20, rounded; Y below 16
    counts as 16, checked on its own above)."""
    rng = np.random.RandomState(1)
    yuv = rng.randint(0, 256, (100000, 3))
    y = 1.164 * (np.maximum(yuv[:, 0], 16) - 16.0)
    u, v = yuv[:, 1] - 128.0, yuv[:, 2] - 128.0
    want = np.stack([y + 1.596 * v, y - 0.813 * v - 0.391 * u, y + 2.018 * u], 1)
    want = np.clip(np.floor(want + 0.5), 0, 255)
    got = pf.yuv_to_rgb(yuv).astype(np.float64)
    assert np.abs(got - want).max() <= 1
    assert (got == want).mean() > 0.99


def test_bgr_and_rgb():
    frame = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    assert np.array_equal(pf.to_rgb_u8(frame, "rgb"), frame)
    assert np.array_equal(pf.to_rgb_u8(frame, "bgr")[1, 2], [17, 16, 15])


def _table(rows):
    return np.array(rows, dtype=np.uint8).reshape(4, 4, 3)


def test_nv12_chroma_addressing():
    """4x4 picture, bytes 0 .. 23: Y plane rows 0-3 (bytes 0 .. 15), UV plane rows ``16 17 18 19`` and ``20 21 22 23``."""
    frame = np.arange(24, dtype=np.uint8).reshape(6, 4)
    want = _table([
        (0, 16, 17), (1, 16, 17), (2, 18, 19), (3, 18, 19),
        (4, 16, 17), (5, 16, 17), (6, 18, 19), (7, 18, 19),
        (8, 20, 21), (9, 20, 21), (10, 22, 23), (11, 22, 23),
        (12, 20, 21), (13, 20, 21), (14, 22, 23), (15, 22, 23)])
    assert np.array_equal(pf.yuv444(frame, "nv12"), want)
    assert np.array_equal(pf.to_rgb_u8(frame, "nv12"), pf.yuv_to_rgb(want))


def test_yuyv_chroma_addressing():
    """4x4 picture, bytes 0 .. 31: row y is ``Y0 U Y1 V Y2 U Y3 V`` = bytes 8y .. 8y + 7."""
    frame = np.arange(32, dtype=np.uint8).reshape(4, 4, 2)
    want = _table([
        (0, 1, 3), (2, 1, 3), (4, 5, 7), (6, 5, 7),
        (8, 9, 11), (10, 9, 11), (12, 13, 15), (14, 13, 15),
        (16, 17, 19), (18, 17, 19), (20, 21, 23), (22, 21, 23),
        (24, 25, 27), (26, 25, 27), (28, 29, 31), (30, 29, 31)])
    assert np.array_equal(pf.yuv444(frame, "yuyv"), want)
    assert np.array_equal(pf.to_rgb_u8(frame, "yuyv"), pf.yuv_to_rgb(want))


def test_reference_against_cv2():
    """The pin against OpenCV itself, on machines that have it."""
    cv2 = pytest.importorskip("cv2", reason="cv2 is not installed on this box")
    rng = np.random.RandomState(2)
    for h, w in ((2, 2), (4, 6), (16, 10), (30, 44)):
        nv12 = rng.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)
        assert np.array_equal(pf.to_rgb_u8(nv12, "nv12"), cv2.cvtColor(nv12, cv2.COLOR_YUV2RGB_NV12))
        yuyv = rng.randint(0, 256, (h, w, 2)).astype(np.uint8)
        assert np.array_equal(pf.to_rgb_u8(yuyv, "yuyv"), cv2.cvtColor(yuyv, cv2.COLOR_YUV2RGB_YUY2))


# ------------------------------------------------------------------------------------------------------------- pack()
def _mixed():
    fmts = ["nv12", "rgb", "yuyv", "bgr"]
    sizes = [(4, 6), (3, 5), (5, 2), (2, 7)]
    frames = [torch.from_numpy(pf.native_frame(f, h, w, seed=i)) for i, (f, (h, w)) in enumerate(zip(fmts, sizes))]
    return fmts, sizes, frames


def test_pack_descriptor_and_bytes_of_mixed_formats():
    from millieye_amd.utils.datasets import PIXEL_FORMATS, StagedRaggedImages
    assert PIXEL_FORMATS == {"rgb": 0, "bgr": 1, "nv12": 2, "yuyv": 3}
    fmts, sizes, frames = _mixed()
    staged = StagedRaggedImages(frames, 8, flips=[0, 1, 0, 1], formats=fmts).pack()
    nbytes = [4 * 6 * 3 // 2, 3 * 5 * 3, 5 * 2 * 2, 2 * 7 * 3]
    assert nbytes == [36, 45, 20, 42] and [f.numel() for f in frames] == nbytes
    want = [[0, 4, 6, 0, 2], [36, 3, 5, 1, 0], [81, 5, 2, 0, 3], [101, 2, 7, 1, 1]]
    assert staged.desc.dtype == torch.int64 and staged.desc.tolist() == want
    assert staged.packed.dtype == torch.uint8 and staged.packed.numel() == sum(nbytes) == 143
    assert torch.equal(staged.packed, torch.cat([f.reshape(-1) for f in frames]))
    assert tuple(staged.shape) == (4, 3, 8, 8) and len(staged) == 4
    # one name for every frame; numpy frames; keep_frames=False drops the tensors
    one = StagedRaggedImages([pf.native_frame("yuyv", 2, 4, 0), pf.native_frame("yuyv", 6, 2, 1)], 4, formats="yuyv")
    one.pack(keep_frames=False)
    assert one.formats == ["yuyv", "yuyv"] and one.desc.tolist() == [[0, 2, 4, 0, 3], [16, 6, 2, 0, 3]] and one.frames == []
    assert len(one) == 2 and one.packed.numel() == 40


def test_default_pack_is_unchanged():
    """``formats=None``: exactly the ``[n,4]`` descriptor and the bytes of the code before the option."""
    from millieye_amd.utils.datasets import StagedRaggedImages
    frames = [torch.from_numpy(pf.native_frame("rgb", h, w, seed=h)) for h, w in ((3, 5), (4, 2))]
    staged = StagedRaggedImages(frames, 8, flips=[1, 0]).pack()
    assert staged.formats is None
    assert tuple(staged.desc.shape) == (2, 4) and staged.desc.tolist() == [[0, 3, 5, 1], [45, 4, 2, 0]]
    assert torch.equal(staged.packed, torch.cat([f.reshape(-1) for f in frames]))
    named = StagedRaggedImages(frames, 8, flips=[1, 0], formats="rgb").pack()
    assert named.desc[:, :4].tolist() == staged.desc.tolist() and named.desc[:, 4].tolist() == [0, 0]
    assert torch.equal(named.packed, staged.packed)


def test_picture_hw():
    from millieye_amd.utils.datasets import picture_hw
    for fmt in pf.FORMATS:
        for h, w in ((2, 2), (4, 6), (480, 640)):
            frame = torch.zeros(pf.native_shape(fmt, h, w), dtype=torch.uint8)
            assert picture_hw(frame, fmt) == (h, w)
            assert picture_hw(frame.numpy(), fmt) == (h, w)
    assert picture_hw(torch.zeros((3, 5, 3), dtype=torch.uint8)) == (3, 5)          # rgb / bgr need no even side
    assert picture_hw(torch.zeros((3, 4, 2), dtype=torch.uint8), "yuyv") == (3, 4)  # yuyv: only w


REFUSED = [
    ("rgb", (4, 4, 2), torch.uint8), ("rgb", (4, 4), torch.uint8), ("bgr", (4, 4, 3), torch.float32),
    ("bgr", (0, 4, 3), torch.uint8),
    ("yuyv", (4, 4, 3), torch.uint8), ("yuyv", (4, 5, 2), torch.uint8), ("yuyv", (4, 4, 2), torch.int8),
    ("nv12", (6, 4, 1), torch.uint8), ("nv12", (6, 5), torch.uint8), ("nv12", (4, 4), torch.uint8),   # 4 rows: no 3h/2
    ("nv12", (6, 4), torch.int16), ("nv12", (0, 4), torch.uint8),
    ("i420", (6, 4), torch.uint8), ("RGB", (4, 4, 3), torch.uint8), (2, (6, 4), torch.uint8),
]


@pytest.mark.parametrize("fmt, shape, dtype", REFUSED)
def test_refused_frames_raise_and_name_the_frame(fmt, shape, dtype):
    from millieye_amd import hip
    from millieye_amd.demo import FrameFuser, prepare_streams
    from millieye_amd.utils.datasets import StagedRaggedImages, picture_hw
    from tests.golden.make_golden import RADAR_CALIB
    good = torch.zeros((2, 2, 3), dtype=torch.uint8)
    bad = torch.zeros(shape, dtype=dtype)
    known = isinstance(fmt, str) and fmt in pf.FORMATS
    with pytest.raises(hip.MeError, match="frame 1" if known else "unknown pixel format"):
        StagedRaggedImages([good, bad], 8, formats=["rgb", fmt]).pack()
    with pytest.raises(hip.MeError):
        picture_hw(bad, fmt)
    with pytest.raises(hip.MeError, match="stream 1"):
        prepare_streams([good, bad], [[], []], 2, pixel_format=["bgr", fmt])
    with pytest.raises(hip.MeError):
        FrameFuser(None, RADAR_CALIB, pixel_format=fmt).prepare(bad, [])


def test_wrong_number_of_formats_is_refused():
    from millieye_amd import hip
    from millieye_amd.demo import prepare_streams
    from millieye_amd.utils.datasets import StagedRaggedImages
    good = torch.zeros((2, 2, 3), dtype=torch.uint8)
    with pytest.raises(hip.MeError):
        StagedRaggedImages([good, good], 8, formats=["rgb"])
    with pytest.raises(hip.MeError):
        prepare_streams([good, good], [[], []], 2, pixel_format=["rgb", "bgr", "rgb"])
    from millieye_amd.demo import MultiStreamFuser
    from tests.golden.make_golden import RADAR_CALIB
    for bad in (["rgb"], "i420", ["nv12", 3]):   # refused when the fuser is built, before any frame
        with pytest.raises(hip.MeError):
            MultiStreamFuser(None, RADAR_CALIB, 2, pixel_format=bad)
    assert MultiStreamFuser(None, RADAR_CALIB, 2, pixel_format="nv12").pixel_format == ["nv12", "nv12"]


# ------------------------------------------------------------------------------------------------- fusers and pipeline
def test_prepare_streams_gives_the_picture_size():
    from millieye_amd.demo import MultiStreamFuser, prepare_streams
    from tests.golden.make_golden import RADAR_CALIB
    fmts = ["nv12", "bgr", "yuyv"]
    sizes = [(32, 48), (40, 36), (30, 44)]
    frames = [pf.native_frame(f, h, w, seed=i) for i, (f, (h, w)) in enumerate(zip(fmts, sizes))]
    assert frames[0].shape == (48, 48)                      # the NV12 tensor is [h*3//2, w]
    payload = prepare_streams(frames, [[], [], []], 3, img_size=64, pixel_format=fmts, pack=True)
    assert payload["hw"] == sizes
    img = payload["img"]
    assert img.formats == fmts and img.desc[:, 1:3].tolist() == [list(s) for s in sizes] and img.desc[:, 4].tolist() == [2, 1, 3]
    assert img.packed.numel() == 32 * 48 * 3 // 2 + 40 * 36 * 3 + 30 * 44 * 2 and img.frames == []
    fuser = MultiStreamFuser(None, RADAR_CALIB, 3, img_size=64, pixel_format=fmts)
    assert fuser.prepare(frames, [[], [], []])["hw"] == sizes
    # the default stays packed RGB with the [n,4] descriptor
    rgb = [pf.to_rgb_u8(f, fmt) for f, fmt in zip(frames, fmts)]
    default = prepare_streams(rgb, [[], [], []], 3, img_size=64, pack=True)
    assert default["hw"] == sizes and default["img"].formats is None and tuple(default["img"].desc.shape) == (3, 4)
    assert MultiStreamFuser(None, RADAR_CALIB, 3).pixel_format is None


def test_pipeline_hands_the_format_to_its_producer():
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    from millieye_amd.pipeline import FusionPipeline
    from tests.golden.make_golden import RADAR_CALIB
    source = pf.NativeSource(1, ["nv12", "yuyv"])
    pipe = FusionPipeline(MultiStreamFuser(None, RADAR_CALIB, 2, img_size=64, pixel_format=["nv12", "yuyv"]), source)
    payload = pipe.prepare_factory()(*source.step(0))     # what the producer process runs
    assert payload["hw"] == [(32, 48), (40, 36)] and payload["img"].desc[:, 4].tolist() == [2, 3]
    assert payload["img"].packed.numel() == 32 * 48 * 3 // 2 + 40 * 36 * 2
    single = FusionPipeline(FrameFuser(None, RADAR_CALIB, img_size=64, pixel_format="nv12"), source)
    frames, radar = source.step(0)
    one = single.prepare_factory()(frames[0], radar[0])
    assert one["hw"] == (32, 48) and one["img"].desc.tolist() == [[0, 32, 48, 0, 2]]
