"""CPU (-m "not gpu"): the host half of the rectangular input path - ``utils.utils.letterbox_geometry``, the tuple forms of
``rescale_terms`` / ``rescale_boxes`` / ``rescale_scalars``, ``StagedRaggedImages(size=(H, W))`` packing,
``demo.radar_boxes_for_network(canvas=)``, the refusals - and the references of tests/letterbox_refs.py themselves (the kernel's
index rule restated in numpy against torch's ``F.pad`` + ``F.interpolate``)."""
import pickle
import random

import numpy as np
import pytest
import torch

from millieye_amd import hip
from millieye_amd.utils.datasets import StagedRadarMaps, StagedRaggedImages, _pad_amounts
from millieye_amd.utils.utils import letterbox_geometry, rescale_boxes, rescale_scalars, rescale_terms
from tests import letterbox_refs as lr, pixel_format_refs as pf

CANVASES = ((32, 64), (64, 32), (32, 96), (96, 30), (64, 96), (256, 416), (416, 256), (32, 32), (416, 416), (6, 4), (26, 16))


def _random_shapes(n, seed):
    rng = random.Random(seed)
    for _ in range(n):
        yield (rng.randint(1, 2200), rng.randint(1, 2200)), rng.choice(CANVASES)


# ------------------------------------------------------------------------------------------------------------- geometry
def test_geometry_properties():
    """Ph W == Pw H; the rectangle holds the picture and the next smaller one of that aspect ratio does not; the pads are
    floor(diff / 2) in front; the loop of the definition agrees."""
    import math
    cases = [(hw, c) for hw, c in lr.SHAPES] + list(_random_shapes(3000, 1))
    for (h, w), (H, W) in cases:
        Ph, Pw, top, left = letterbox_geometry((h, w), (H, W))
        g = math.gcd(H, W)
        a, b = H // g, W // g
        assert Ph * W == Pw * H and Ph % a == 0 and Pw % b == 0 and Ph // a == Pw // b
        assert Ph >= h and Pw >= w, "holds the picture"
        assert Ph - a < h or Pw - b < w, "minimal"
        assert top == (Ph - h) // 2 and left == (Pw - w) // 2
        assert (Ph, Pw, top, left) == tuple(lr.geometry_fast((h, w), (H, W))[i] for i in (0, 1, 2, 4))
    for (h, w), canvas in cases[:len(lr.SHAPES) + 200]:
        if max(h, w) < 400:
            assert lr.geometry((h, w), canvas) == lr.geometry_fast((h, w), canvas)
    assert letterbox_geometry((1080, 1920), (256, 416)) == (1184, 1924, 52, 2)
    assert letterbox_geometry((33, 97), (32, 96)) == (33, 99, 0, 1)


def test_geometry_square_is_pad_to_square():
    for (h, w), _c in _random_shapes(2000, 2):
        for S in (416, (416, 416), (96, 96)):
            Ph, Pw, top, left = letterbox_geometry((h, w), S)
            pl, pr, pt, pb = _pad_amounts(h, w)
            assert Ph == Pw == max(h, w) and (left, Pw - w - left, top, Ph - h - top) == (pl, pr, pt, pb)


def test_geometry_refuses_empty_sizes():
    for hw, canvas in (((0, 5), (32, 64)), ((5, 5), (0, 64))):
        with pytest.raises(hip.MeError):
            letterbox_geometry(hw, canvas)


# ---------------------------------------------------------------------------------------------------------- rescale terms
def test_tuple_terms_equal_the_int_form():
    """``(S, S)``: exactly the int form's python floats (==, not close), for the terms, the scalars and the boxes."""
    rng = random.Random(3)
    for _ in range(20000):
        hw, S = (rng.randint(1, 2200), rng.randint(1, 2200)), 32 * rng.randint(1, 40)
        assert rescale_terms((S, S), hw) == rescale_terms(S, hw), (hw, S)
    hws = [(480, 640), (1080, 1920), (97, 61), (512, 512)]
    assert torch.equal(rescale_scalars((416, 416), hws), rescale_scalars(416, hws))
    boxes = torch.rand(7, 4) * 416
    assert torch.equal(rescale_boxes(boxes.clone(), (416, 416), (480, 640)), rescale_boxes(boxes.clone(), 416, (480, 640)))


def test_tuple_terms_against_the_reference():
    for hw, canvas in list(_random_shapes(2000, 4)) + list(lr.SHAPES):
        t = rescale_terms(canvas, hw)
        assert list(t["x"]) + list(t["y"]) == lr.rescale_terms(canvas, hw), (hw, canvas)
    hws = [(1080, 1920), (480, 640), (97, 33)]
    want = torch.tensor([lr.rescale_terms((256, 416), hw) for hw in hws], dtype=torch.float64).to(torch.float32)
    assert torch.equal(rescale_scalars((256, 416), hws), want)
    boxes = torch.rand(9, 4) * 256
    assert torch.equal(rescale_boxes(boxes.clone(), (256, 416), (1080, 1920)), lr.rescale(boxes, (256, 416), (1080, 1920)))


def test_round_trip_error_bound():
    """A source coordinate x in [0, w] goes to the canvas as (x + left) (W / Pw) and comes back through ``rescale_boxes``.
    ``rescale_boxes`` subtracts ``pad // 2`` where the forward map added ``left * (W / Pw)``: the floor of ``pad // 2`` loses up
    to one canvas pixel = Pw / W source pixels and the ``// 2`` of an odd pad the half source pixel ``left`` dropped, and
    ``canvas - pad`` is ``w W / Pw`` exactly, so the error is at most 0.5 + Pw / W source pixels (float64 here)."""
    worst = 0.0
    for (h, w), (H, W) in list(_random_shapes(1500, 5)) + list(lr.SHAPES):
        Ph, Pw, top, left = letterbox_geometry((h, w), (H, W))
        xs = torch.linspace(0, w, 23, dtype=torch.float64)
        ys = torch.linspace(0, h, 23, dtype=torch.float64)
        canvas = torch.stack([(xs + left) * (W / Pw), (ys + top) * (H / Ph), (xs + left) * (W / Pw), (ys + top) * (H / Ph)], 1)
        back = rescale_boxes(canvas.clone(), (H, W), (h, w))
        bound = 0.5 + Pw / W
        err = max(float((back[:, 0] - xs).abs().max()), float((back[:, 1] - ys).abs().max()))
        worst = max(worst, err / bound)
        assert err <= bound, f"{h}x{w} -> {H}x{W}: {err} > {bound}"
    print(f"largest round-trip error: {worst:.3f} of the bound")
    assert worst > 0.5, "the sweep must come near the bound to mean anything"


# ------------------------------------------------------------------------------------------------------------ index rule
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_index_rule_is_torch_nearest(shape):
    (h, w), canvas = shape
    rgb = np.random.RandomState(h * 7 + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    for flip in (False, True):
        want = lr.letterbox_nearest(rgb, canvas, "rgb", flip)
        got = lr.gather_by_rule(rgb, canvas, flip)
        assert want.shape == (3,) + tuple(canvas) and torch.equal(got, want), f"{shape} flip {flip}"
    if h * w > 1:
        assert float(want.abs().sum()) > 0
    if (h, w) == tuple(canvas):
        assert torch.equal(lr.letterbox_nearest(rgb, canvas), torch.from_numpy(rgb).permute(2, 0, 1).float() / 255)


def test_reference_square_case_is_the_oracle():
    from oracle import datasets_ref
    rgb = np.random.RandomState(11).randint(0, 256, (10, 300, 3)).astype(np.uint8)
    img, _ = datasets_ref.pad_to_square(datasets_ref.to_tensor(rgb), 0)
    assert torch.equal(lr.letterbox_nearest(rgb, (32, 32)), datasets_ref.resize(img, 32))


# --------------------------------------------------------------------------------------------------------------- staging
def test_staged_pack_shape_descriptor_and_pickle():
    fmts = ["nv12", "rgb", "yuyv", "bgr"]
    sizes = [(4, 6), (7, 5), (5, 2), (33, 97)]
    frames = [torch.from_numpy(pf.native_frame(f, h, w, seed=30 + i)) for i, (f, (h, w)) in enumerate(zip(fmts, sizes))]
    flips = [0, 1, 0, 1]
    staged = StagedRaggedImages(frames, (32, 96), flips, formats=fmts)
    assert tuple(staged.shape) == (4, 3, 32, 96) and len(staged) == 4 and staged.rect == (32, 96)
    staged.pack()
    offsets = np.concatenate([[0], np.cumsum([f.numel() for f in frames])])
    want = [[int(offsets[i]), h, w, flips[i], hip_fmt] for i, ((h, w), hip_fmt) in enumerate(zip(sizes, (2, 0, 3, 1)))]
    assert staged.desc.tolist() == want and staged.desc.dtype == torch.int64
    assert staged.packed.numel() == offsets[-1]
    assert torch.equal(staged.packed[offsets[3]:], frames[3].reshape(-1))
    # plain RGB frames take the [n,5] descriptor too
    rgb = StagedRaggedImages([frames[1], frames[3]], (64, 32)).pack(keep_frames=False)
    assert tuple(rgb.desc.shape) == (2, 5) and rgb.desc[:, 4].tolist() == [0, 0] and rgb.frames == []
    back = pickle.loads(pickle.dumps(rgb))
    assert back.rect == (64, 32) and tuple(back.shape) == (2, 3, 64, 32)
    assert torch.equal(back.packed, rgb.packed) and torch.equal(back.desc, rgb.desc)
    with pytest.raises(hip.MeError, match="CUDA"):
        back.to("cpu")


def test_square_tuple_is_the_int_path():
    frame = torch.zeros((4, 6, 3), dtype=torch.uint8)
    staged = StagedRaggedImages([frame], (32, 32)).pack()
    assert staged.rect is None and staged.size == 32 and tuple(staged.desc.shape) == (1, 4) and tuple(staged.shape) == (1, 3, 32, 32)
    maps = StagedRadarMaps([np.zeros((0, 4))], [(6, 4)], (4, 4))
    assert maps.map_size == 4 and tuple(maps.shape) == (1, 3, 4, 4)
    assert tuple(StagedRadarMaps([np.zeros((0, 4))], [(6, 4)], (4, 6)).shape) == (1, 3, 4, 6)


# ------------------------------------------------------------------------------------------------------------ host boxes
def test_radar_boxes_for_network_canvas():
    from millieye_amd.demo import radar_boxes_for_network
    rng = np.random.RandomState(6)
    for hw, canvas in (((240, 320), (64, 96)), ((320, 240), (64, 96)), ((256, 256), (96, 64)), ((1080, 1920), (256, 416)),
                       ((33, 97), (32, 96))):
        h, w = hw
        xy = rng.uniform(-0.3, 1.3, (40, 2)) * [w, h]
        wh = rng.uniform(-0.05, 0.5, (40, 2)) * [w, h]    # some reversed, some clamped on each side, some emptied by the clamp
        boxes = np.concatenate([xy, xy + wh], 1)
        got = radar_boxes_for_network(boxes, hw, canvas)
        want = lr.radar_boxes(boxes, hw, canvas)
        assert 0 < len(want) < 40 and torch.equal(got, want), (hw, canvas)
        assert torch.equal(radar_boxes_for_network(boxes, hw, (96, 96)), radar_boxes_for_network(boxes, hw))
    assert radar_boxes_for_network(np.zeros((0, 4)), (240, 320), (64, 96)).shape == (0, 5)
    # hand-worked: 1080 x 1920 in 256 x 416 is padded to 1184 x 1924, top 52, left 2
    rb = radar_boxes_for_network([[0, 0, 1920, 1080]], (1080, 1920), (256, 416))
    assert torch.equal(rb, torch.tensor([[0, 2 / 1924, 52 / 1184, 1922 / 1924, 1132 / 1184]], dtype=torch.float32))


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from millieye_amd.demo import FrameFuser, MultiStreamFuser, prepare_streams
    calib = np.arange(12, dtype=np.float64)
    frame = torch.zeros((4, 6, 3), dtype=torch.uint8)
    for bad in ((64, 100), (0, 64), (-32, 64), (48, 64), (64, 96, 32)):
        what = "x".join(str(v) for v in bad[:2]) if len(bad) == 2 else "64, 96, 32"
        for build in (lambda: FrameFuser(None, calib, img_size=bad), lambda: MultiStreamFuser(None, calib, 2, img_size=bad),
                      lambda: prepare_streams([frame], [[]], 1, img_size=bad)):
            with pytest.raises(hip.MeError, match=what.replace("x", " x ")):
                build()
    with pytest.raises(hip.MeError, match=r"frame_modes.*64 x 96"):
        MultiStreamFuser(None, calib, 2, img_size=(64, 96), split="frame_modes")
    for build in (lambda: StagedRaggedImages([frame], (64, 96), resize="area"),
                  lambda: FrameFuser(None, calib, img_size=(64, 96), resize="area"),
                  lambda: MultiStreamFuser(None, calib, 2, img_size=(64, 96), resize="area"),
                  lambda: prepare_streams([frame], [[]], 1, img_size=(64, 96), resize="area")):
        with pytest.raises(hip.MeError, match=r"area.*64 x 96"):
            build()
    # (S, S) is S: everything a square fuser may do
    fuser = MultiStreamFuser(None, calib, 2, img_size=(64, 64), split="frame_modes", resize="area")
    assert fuser.img_size == 64 and not fuser.rect
    assert FrameFuser(None, calib, img_size=(64, 96)).img_size == (64, 96)
    payload = prepare_streams([frame, frame], [[], []], 2, img_size=(64, 96), pack=True)
    assert tuple(payload["img"].shape) == (2, 3, 64, 96) and tuple(payload["img"].desc.shape) == (2, 5)
    assert pickle.loads(pickle.dumps(payload))["img"].rect == (64, 96)
