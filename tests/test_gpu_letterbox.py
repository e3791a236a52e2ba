"""-m gpu: the rectangular input path on the device against the stock torch CPU references of tests/letterbox_refs.py
(guarded by tests/test_letterbox_cpu.py):

* ``me_image_batch_letterbox_u8_f32``: ragged launches of all four formats, flips and invalid descriptors under ``torch.equal``
  with ``F.pad`` + ``F.interpolate(nearest)``; NaN-filled outputs between sentinels; the square contract;
* ``me_radar_boxes_letterbox_f32``: ``torch.equal`` with the per-axis float32 arithmetic on the device's own pixel proposals,
  clamped on every side (the top by a tall reflector of its own: the helper scenes' boxes are 10 - 20 pixels tall and sit below
  the frame's top edge), and on hand-written proposals in the device's buffers (all four sides, NaN, a full track list);
* ``me_radar_heatmap_rect_f32`` at the bar of tests/test_gpu_datasets.py's square heat-map test (1e-6 absolute: aten's CPU
  bilinear kernel contracts multiply-adds, the kernel rounds every operation);
* ``FrameFuser`` / ``MultiStreamFuser`` / ``prepare_streams`` / ``FusionPipeline`` with ``img_size=(64, 96)``."""
import pickle

import numpy as np
import pytest
import torch

from millieye_amd import radar_proposals as rp, synth
from tests import letterbox_refs as lr, multistream_helpers as mh, pixel_format_refs as pf, radar_scene_helpers as sh
from tests.golden.make_golden import RADAR_CALIB

pytestmark = pytest.mark.gpu

E_BADARG, E_NULLPTR, E_ALIGN, E_TOOBIG = -1, -2, -3, -4      # include/millieye_hip.h
GUARD, SENTINEL = 64, 12345.0                                # floats in front of and behind dst (64: dst stays 16-byte aligned)


def _launch(packed, desc, n, H, W):
    """One ``me_image_batch_letterbox_u8_f32`` call: ``[n,3,H,W]`` on the host.  dst is NaN between two sentinel blocks; the
    sentinels must survive and no NaN may remain."""
    from millieye_amd import hip
    d_src, d_desc = packed.contiguous().cuda(), desc.contiguous().cuda()
    buf = torch.full((2 * GUARD + n * 3 * H * W,), float("nan"), device="cuda", dtype=torch.float32)
    buf[:GUARD] = SENTINEL
    buf[-GUARD:] = SENTINEL
    dst = buf[GUARD:-GUARD]
    hip.check(hip.lib().me_image_batch_letterbox_u8_f32(d_src.data_ptr(), int(d_src.numel()), d_desc.data_ptr(), n, dst.data_ptr(),
                                                        H, W, hip.stream_ptr()), "me_image_batch_letterbox_u8_f32")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[-GUARD:] == SENTINEL).all()), "a sentinel was overwritten"
    out = host[GUARD:-GUARD].reshape(n, 3, H, W)
    assert not torch.isnan(out).any(), "elements left unwritten"
    return out


def _even(v):
    return v + (v & 1)


def _batch(pictures, seed):
    """For every picture size of a canvas: the RGB frame plain and mirrored, a BGR frame, and YUYV / NV12 frames of the next
    even size.  Returns ``(frames, formats, flips)``."""
    frames, fmts, flips = [], [], []
    for i, (h, w) in enumerate(pictures):
        rgb = pf.native_frame("rgb", h, w, seed=seed + 10 * i)
        for frame, fmt, flip in ((rgb, "rgb", 0), (rgb, "rgb", 1), (pf.native_frame("bgr", h, w, seed=seed + 10 * i + 1), "bgr", 1),
                                 (pf.native_frame("yuyv", h, _even(w), seed=seed + 10 * i + 2), "yuyv", i & 1),
                                 (pf.native_frame("nv12", _even(h), _even(w), seed=seed + 10 * i + 3), "nv12", 1 - (i & 1))):
            frames.append(frame), fmts.append(fmt), flips.append(flip)
    return frames, fmts, flips


def _equal(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: {got[i].item()!r} vs "
                             f"{want[i].item()!r}")


# (canvas, picture sizes): pad on either axis (an axis swap shows exactly), 1 x 1, k from the width with left = 1 and the
# remainder behind, W % 4 != 0 (scalar stores), the identity
CASES = (((32, 64), ((7, 5),)), ((64, 32), ((5, 7),)), ((32, 96), ((1, 1), (33, 97))), ((96, 30), ((97, 33),)),
         ((64, 96), ((64, 96),)))


@pytest.mark.parametrize("canvas,pictures", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else None)
def test_letterbox_ragged_launch(hip_lib, canvas, pictures):
    """One ragged launch per canvas: all four formats, flips, and three invalid descriptors (offset out of range, odd NV12
    height, unknown format) that must give all-zero frames beside untouched neighbours."""
    from millieye_amd.utils.datasets import StagedRaggedImages
    H, W = canvas
    frames, fmts, flips = _batch(pictures, seed=500 + H + W)
    n = len(frames)
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], canvas, flips, formats=fmts).pack()
    total = int(staged.packed.numel())
    nv12 = fmts.index("nv12")
    bad = torch.stack([staged.desc[0].clone(), staged.desc[nv12].clone(), staged.desc[0].clone()])
    bad[0, 0] = total + 5                  # offset out of range
    bad[1, 1] = int(bad[1, 1]) - 1         # odd NV12 height
    bad[2, 4] = 7                          # unknown format
    desc = torch.cat([staged.desc, bad], 0)
    got = _launch(staged.packed, desc, n + 3, H, W)
    for i, (frame, fmt, flip) in enumerate(zip(frames, fmts, flips)):
        want = lr.letterbox_nearest(frame, canvas, fmt, bool(flip))
        _equal(got[i], want, f"{canvas} frame {i} ({fmt} {pf.picture_hw(frame, fmt)}, flip {flip})")
        assert float(want.abs().sum()) > 0
    for k in range(3):
        assert torch.equal(got[n + k], torch.zeros(3, H, W)), f"invalid descriptor {k} is not padding"
    if tuple(pictures[0]) == tuple(canvas):   # the identity: u8 / 255
        assert torch.equal(got[0], torch.from_numpy(frames[0]).permute(2, 0, 1).float() / 255)
    # ... and through the staged object, packed and not
    dev = StagedRaggedImages([torch.from_numpy(f) for f in frames], canvas, flips, formats=fmts).to("cuda").cpu()
    assert torch.equal(dev, got[:n]) and torch.equal(staged.to("cuda").cpu(), got[:n])


def test_letterbox_square_contract(hip_lib):
    """10 x 300 -> 32 x 32 (and the other formats) next to the same frames through ``me_image_batch_formats_u8_f32``."""
    from millieye_amd import hip
    from millieye_amd.utils.datasets import StagedRaggedImages
    frames, fmts, flips = _batch(((10, 300), (33, 20)), seed=700)
    n = len(frames)
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], 32, flips, formats=fmts).pack()
    got = _launch(staged.packed, staged.desc, n, 32, 32)
    square = torch.full((n, 3, 32, 32), float("nan"), device="cuda")
    d_src, d_desc = staged.packed.cuda(), staged.desc.cuda()
    hip.check(hip.lib().me_image_batch_formats_u8_f32(d_src.data_ptr(), int(d_src.numel()), d_desc.data_ptr(), n,
                                                      square.data_ptr(), 32, hip.stream_ptr()), "me_image_batch_formats_u8_f32")
    _equal(got, square.cpu(), "square contract")
    _equal(got[0], lr.letterbox_nearest(frames[0], (32, 32)), "10x300 -> 32x32 vs torch")


def test_letterbox_1080p(hip_lib):
    from millieye_amd.utils.datasets import StagedRaggedImages
    frames = [pf.native_frame("rgb", 1080, 1920, seed=801), pf.native_frame("nv12", 1080, 1920, seed=802)]
    fmts, flips = ["rgb", "nv12"], [0, 1]
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], (256, 416), flips, formats=fmts).pack()
    got = _launch(staged.packed, staged.desc, 2, 256, 416)
    for i in range(2):
        _equal(got[i], lr.letterbox_nearest(frames[i], (256, 416), fmts[i], bool(flips[i])), f"1080p {fmts[i]}")
    assert torch.equal(got[0, :, :11], torch.zeros(3, 11, 416)) and float(got[0, :, 12].abs().sum()) > 0   # top = 52 of 1184


def test_letterbox_padded_size_limit(hip_lib):
    """Canvas 1 x 2^20 (a = 1, b = 2^20): a mirrored 1024 x 1 picture pads to 1024 x 2^30, the largest rectangle allowed, and
    lands on exactly one output pixel (the index rule of tests/letterbox_refs.py; torch cannot pad to 2^40 elements); a
    1025 x 1 picture would pad to 1025 x 2^20 columns, above 2^30: invalid, all zero."""
    from millieye_amd.utils.datasets import StagedRaggedImages
    H, W = 1, 1 << 20
    frames = [np.full((1024, 1, 3), 255, np.uint8), np.full((1025, 1, 3), 255, np.uint8)]
    staged = StagedRaggedImages([torch.from_numpy(f) for f in frames], (H, W), [1, 1]).pack()
    got = _launch(staged.packed, staged.desc, 2, H, W)
    sy, sx = lr.kernel_index_rule((1024, 1), (H, W), flip=True)
    assert sy.tolist() == [0] and np.flatnonzero(sx >= 0).tolist() == [1 << 19]
    _equal(got[0], lr.gather_by_rule(frames[0], (H, W), flip=True), "1024 x 1 -> 1 x 2^20")
    assert float(got[0].sum()) == 3.0 and torch.equal(got[1], torch.zeros(3, H, W))


def test_letterbox_argument_checks(hip_lib):
    """Every refusal returns before a launch (``out`` is never written by them).  The one accepted call - ``W % 4 != 0``, so a
    dst that is only 4-byte aligned is fine - runs on a buffer sized for it, between sentinels, and is compared."""
    from millieye_amd import hip
    fn = hip.lib().me_image_batch_letterbox_u8_f32
    frame = pf.native_frame("rgb", 2, 2, seed=900)
    src = torch.from_numpy(frame).reshape(-1).cuda()
    nbytes = int(src.numel())
    desc = torch.tensor([[0, 2, 2, 0, 0]], dtype=torch.int64, device="cuda")
    H, W = 12, 9
    elems = 3 * H * W
    buf = torch.full((GUARD + 1 + elems + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    buf[:GUARD + 1] = SENTINEL
    buf[-GUARD:] = SENTINEL
    out = buf[GUARD:]            # 16-byte aligned (GUARD floats behind the allocation's start), holds 1 + elems + GUARD floats
    assert out.data_ptr() % 16 == 0
    assert fn(src.data_ptr(), nbytes, desc.data_ptr(), 0, out.data_ptr(), 8, 12, None) == 0             # n = 0: nothing to do
    assert fn(None, nbytes, desc.data_ptr(), 1, out.data_ptr(), 8, 12, None) == E_NULLPTR
    assert fn(src.data_ptr(), 0, desc.data_ptr(), 1, out.data_ptr(), 8, 12, None) == E_BADARG
    assert fn(src.data_ptr(), nbytes, desc.data_ptr(), 1, out.data_ptr(), 0, 12, None) == E_BADARG
    assert fn(src.data_ptr(), nbytes, desc.data_ptr(), 65536, out.data_ptr(), 8, 12, None) == E_BADARG
    assert fn(src.data_ptr(), nbytes, desc.data_ptr(), 1, out.data_ptr(), 1 << 15, 1 << 15, None) == E_TOOBIG
    assert fn(src.data_ptr(), nbytes, desc.data_ptr(), 1, out.data_ptr() + 4, 8, 12, None) == E_ALIGN   # W % 4 == 0: float4 stores
    torch.cuda.synchronize()
    untouched = buf.cpu()
    assert bool((untouched[:GUARD + 1] == SENTINEL).all()) and bool(torch.isnan(untouched[GUARD + 1:-GUARD]).all())
    # W % 4 != 0: scalar stores to a dst one float behind the aligned address, exactly ``elems`` floats
    assert fn(src.data_ptr(), nbytes, desc.data_ptr(), 1, out.data_ptr() + 4, H, W, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:GUARD + 1] == SENTINEL).all()) and bool((host[-GUARD:] == SENTINEL).all()), "a sentinel was overwritten"
    _equal(host[GUARD + 1:-GUARD].reshape(3, H, W), lr.letterbox_nearest(frame, (H, W)), "2x2 -> 12x9 at a 4-byte aligned dst")


# ---------------------------------------------------------------------------------------------------------- radar boxes
CANVASES = ((64, 96), (96, 64), (256, 416))


def _shifted_radar(f):
    """The boxes scene moved 1.5 m to the left and 0.8 m up: proposals that cross the frame's left edge."""
    frame = sh.grid_frame(f, seed=23).copy()
    frame[0] -= 1.5
    frame[2] += 0.8
    return [frame]


def _tall_radar(f):
    """One reflector 3.5 m away, 1.6 m tall, whose top lies 1.77 m above the radar: its ten points project inside the frame
    (the topmost a few pixels below the top edge) and its proposal, 1.4 x as tall, starts 2 - 8 pixels above it."""
    rng = np.random.RandomState(31 + f)
    n = 10
    return [np.stack([-0.3 + rng.randn(n) * 0.03, 3.5 + rng.randn(n) * 0.01, 1.77 + np.linspace(-1.6, 0, n),
                      1.0 + rng.randn(n) * 0.02])]


def _reference_rows(dev, hw, canvas):
    rows = [lr.radar_boxes(dev.proposals(s), hw[s], canvas, s) for s in range(dev.streams)]
    return torch.cat(rows, 0), np.array([len(r) for r in rows])


def test_radar_boxes_on_device_proposals(hip_lib):
    """Streams 0 - 2: the proposals-versus-boxes scene (landscape, portrait, square frames smaller than the field of view);
    stream 3: the shifted scene; stream 4: no radar frame at all.  Then a generator of one stream with the tall reflector."""
    hw = list(sh.BOXES_FRAME_HW) + [(240, 320), (480, 640)]
    n = len(hw)
    dev = rp.DeviceRadarProposals(RADAR_CALIB, n, min_hits=sh.MIN_HITS, **sh.BOXES_KW)
    clamped = np.zeros(4, bool)
    emptied = False
    for f in range(sh.BOXES_FRAMES):
        res = dev.gen([sh.boxes_radar(s, f) for s in range(3)] + [_shifted_radar(f), []], hw)
        assert res.host_counts[4, 7] == 0
        for canvas in CANVASES:
            rows, counts = dev.letterbox_boxes(canvas)
            want, want_counts = _reference_rows(dev, hw, canvas)
            assert np.array_equal(counts, want_counts), f"frame {f} {canvas}: counts {counts} vs {want_counts}"
            assert rows.shape == want.shape and torch.equal(rows.cpu(), want), f"frame {f} {canvas}: rows differ"
            assert counts.sum() >= 1 and counts[4] == 0, "the scene must keep a box on every canvas"
            clamped |= [bool((want[:, 1] == 0).any()), bool((want[:, 2] == 0).any()), bool((want[:, 3] == 1).any()),
                        bool((want[:, 4] == 1).any())]
            emptied |= bool((counts < res.host_counts[:, 7]).any())
        # a square canvas: the chain's own rows and counts
        rows, counts = dev.letterbox_boxes((96, 96))
        assert np.array_equal(counts, res.host_counts[:, 4]) and torch.equal(rows, res.radar_box)
    # the tall reflector (the generator's default max_size: the scene above skips clusters this large): the top clamp, S = 1
    tall = rp.DeviceRadarProposals(RADAR_CALIB, 1, min_hits=sh.MIN_HITS)
    for f in range(3):
        res = tall.gen([_tall_radar(f)], [(480, 640)])
        assert res.host_counts[0, 1] == 10 and res.host_counts[0, 7] == 1 and tall.proposals(0)[0, 1] < 0 < tall.proposals(0)[0, 3]
        for canvas in CANVASES:
            rows, counts = tall.letterbox_boxes(canvas)
            want, want_counts = _reference_rows(tall, [(480, 640)], canvas)
            assert counts[0] == 1 and np.array_equal(counts, want_counts) and torch.equal(rows.cpu(), want), f"tall {f} {canvas}"
            clamped[1] |= bool((want[:, 2] == 0).any())
        rows, counts = tall.letterbox_boxes((96, 96))
        assert np.array_equal(counts, res.host_counts[:, 4]) and torch.equal(rows, res.radar_box)
    assert clamped.all() and emptied, f"clamped (left, top, right, bottom) {clamped}, emptied {emptied}"
    # S = 1
    one = rp.DeviceRadarProposals(RADAR_CALIB, 1, min_hits=sh.MIN_HITS, **sh.BOXES_KW)
    for f in range(3):
        res = one.gen([sh.boxes_radar(1, f)], [hw[1]])
    rows, counts = one.letterbox_boxes((64, 96))
    want, want_counts = _reference_rows(one, [hw[1]], (64, 96))
    assert counts[0] >= 1 and np.array_equal(counts, want_counts) and torch.equal(rows.cpu(), want)
    rows, counts = one.letterbox_boxes((64, 64))
    assert np.array_equal(counts, res.host_counts[:, 4]) and torch.equal(rows, res.radar_box)


def test_radar_boxes_on_written_proposals(hip_lib):
    """Proposals written into the generator's device buffers: every side clamped, a box emptied by the clamp, reversed boxes, NaN
    (kept by the clamp, dropped by the comparison), a full list of 32, an empty one."""
    from millieye_amd import hip
    hw = [(240, 320), (320, 240), (33, 97), (1080, 1920)]
    n = len(hw)
    dev = rp.DeviceRadarProposals(RADAR_CALIB, n, min_hits=sh.MIN_HITS)
    dev.gen([[] for _ in range(n)], hw)           # (uploads the frame sizes)
    rng = np.random.RandomState(9)
    props = np.zeros((n, hip.RADAR_MAX_TRACKS, 4))
    nprop = [32, 9, 0, 20]
    for s, (h, w) in enumerate(hw):
        xy = rng.uniform(-0.4, 1.2, (32, 2)) * [w, h]
        wh = rng.uniform(-0.1, 0.6, (32, 2)) * [w, h]
        props[s] = np.concatenate([xy, xy + wh], 1)
    props[0, :6] = [[-500, 10, 50, 60], [10, -500, 50, 60], [300, 10, 4000, 60], [10, 200, 50, 3000], [-3000, 10, -2500, 60],
                    [float("nan"), 10, 50, 60]]
    counts = dev._counts.clone()
    counts[:, 7] = torch.tensor(nprop, dtype=torch.int32)
    dev._proposals.copy_(torch.from_numpy(props))
    dev._counts.copy_(counts)
    dev.host_counts = counts.cpu().numpy()
    for canvas in CANVASES + ((32, 96), (96, 96)):
        rows, got = dev.letterbox_boxes(canvas)
        want, want_counts = _reference_rows(dev, hw, canvas)
        assert np.array_equal(got, want_counts) and torch.equal(rows.cpu(), want), f"{canvas}: {got} vs {want_counts}"
        assert got[2] == 0 and 0 < got[0] < 32
        first = want[want[:, 0] == 0][:4, 1:]
        assert first[0, 0] == 0 and first[1, 1] == 0 and first[2, 2] == 1 and first[3, 3] == 1, f"{canvas}: the four clamps"
        assert not torch.isnan(want).any()


# ------------------------------------------------------------------------------------------------------------ heat maps
def _clouds():
    pts, sizes = [], []
    for i, (w, h, n) in enumerate([(1600, 900, 25), (900, 1600, 60), (640, 640, 0), (1280, 720, 300), (64, 48, 5)]):
        u = synth.uniform(f"lb/hm/{i}/u", (n,), -20, w + 20).astype(np.float64)
        v = synth.uniform(f"lb/hm/{i}/v", (n,), -20, h + 20).astype(np.float64)
        d = synth.uniform(f"lb/hm/{i}/d", (n,), 0.1, 15).astype(np.float64)
        s = synth.uniform(f"lb/hm/{i}/s", (n,), -6, 6).astype(np.float64)
        if n >= 5:
            u[:4], v[:4] = [0.0, w, w / 2.0, w / 4.0], [0.0, h, h / 2.0, h / 4.0]
        pts.append(np.stack([u, v, d, s], 1))
        sizes.append((w, h))
    return pts, sizes


@pytest.mark.parametrize("map_hw", [(4, 6), (6, 4), (26, 16)])
def test_heatmap_rect_vs_torch(hip_lib, map_hw):
    from millieye_amd.utils.datasets import StagedRadarMaps
    pts, sizes = _clouds()
    got = StagedRadarMaps(pts, sizes, map_hw).to("cuda").cpu()
    assert got.shape == (len(pts), 3) + map_hw and float(got.abs().sum()) > 0
    for i, (p, wh) in enumerate(zip(pts, sizes)):
        ref = lr.heatmap_rect(p, wh, map_hw)
        err = float((got[i] - ref).abs().max())
        print(f"map {map_hw} frame {i}: max abs error {err:.3e}")
        assert err <= 1e-6, (map_hw, i, err)


def test_heatmap_rect_square_is_the_square_kernel(hip_lib):
    from millieye_amd import hip
    from millieye_amd.utils.datasets import StagedRadarMaps
    pts, sizes = _clouds()
    n = len(pts)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(p) for p in pts])
    d_pts = torch.from_numpy(np.concatenate(pts, 0)).cuda()
    d_off, d_sz = torch.from_numpy(offsets).cuda(), torch.tensor(sizes, dtype=torch.int32).cuda()
    for ms in (26, 10, 32, 1):
        got = torch.full((n, 3, ms, ms), float("nan"), device="cuda")
        hip.check(hip.lib().me_radar_heatmap_rect_f32(d_pts.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), n, 32, got.data_ptr(),
                                                      ms, ms, hip.stream_ptr()), "me_radar_heatmap_rect_f32")
        want = StagedRadarMaps(pts, sizes, ms).to("cuda")
        assert torch.equal(got, want), f"map {ms} x {ms}"
    # an aspect ratio that would pad the 64-bin map beyond 2^30 (b = 2^27) is refused before any launch
    fn = hip.lib().me_radar_heatmap_rect_f32
    assert fn(d_pts.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), n, 32, got.data_ptr(), 1, 1 << 27, None) == E_TOOBIG
    assert "2^30" in hip.lib().me_last_error().decode()
    assert fn(d_pts.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), n, 32, got.data_ptr(), 0, 4, None) == E_BADARG


# --------------------------------------------------------------------------------------------------------------- fusers
CANVAS, STREAMS = (64, 96), 3


def _nets():
    from tests.test_gpu_network import _build
    nets = []
    for _ in range(2):
        net = _build("demo", "yolov3-tiny-12", 0.1).eval()
        synth.fill_network_(net, "demo", cls0_bias=3.0, cls_bias=-4.0)
        nets.append(net)
    return nets[0], nets[1].to(nets[1].device)


def _rows8(rows, hw):
    """Fuser rows in frame pixels -> canvas units with a zero image column (the layout tests/test_gpu_network.py compares)."""
    return mh.rows8(rows, hw, img_size=max(CANVAS))


def test_fusers_on_a_rectangular_canvas(hip_lib):
    """MultiStreamFuser(img_size=(64, 96)) against three FrameFusers (the comparisons of test_fuser_equivalence), the device
    tail against the host tail and a pickled packed payload against the unpacked one (torch.equal), FrameFuser against the
    host composition of tests/letterbox_refs.py (the bar of tests/test_gpu_rect.py's network test)."""
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    from tests.test_gpu_network import _cmp_rows, _cmp_rows_ties
    cpu_net, net = _nets()
    n = STREAMS
    frames = [mh.stream_frame(s) for s in range(n)]
    assert len({f.shape for f in frames}) == 2
    kw = dict(model_mode=3, min_hits=mh.MIN_HITS, img_size=CANVAS)
    singles = [FrameFuser(net, RADAR_CALIB, **kw) for _ in range(n)]
    multi = MultiStreamFuser(net, RADAR_CALIB, n, **kw)
    host_tail = MultiStreamFuser(net, RADAR_CALIB, n, tail="host", **kw)
    rows_total = boxes_total = composed = 0
    for f in range(5):
        radar = [mh.stream_radar(s, f) for s in range(n)]
        payloads = [singles[s].prepare(frames[s], radar[s]) for s in range(n)]
        want = [singles[s].infer(payloads[s]) for s in range(n)]
        got = multi(frames, radar)
        modes = [info["mode"] for _r, info in got]
        assert 0 in modes and 1 in modes, "both modes must be present"
        for s, ((rows, info), (rows_w, info_w)) in enumerate(zip(got, want)):
            for key in ("mode", "points", "radar_boxes"):
                assert info[key] == info_w[key], f"step {f} stream {s}: {key} {info[key]} vs {info_w[key]}"
            assert info["proposals"].shape == info_w["proposals"].shape
            hw = frames[s].shape[:2]
            _cmp_rows_ties(_rows8(rows, hw), _rows8(rows_w, hw), f"step {f} stream {s}")
            # FrameFuser against the host composition
            cloud = payloads[s]["radar_map"].points[0]
            ref, mode, nbox = lr.fuser_step(cpu_net, frames[s], cloud, payloads[s]["proposals"], CANVAS, conf=0.1)
            assert mode == info_w["mode"] and nbox == info_w["radar_boxes"]
            _cmp_rows(_rows8(rows_w, hw), _rows8(ref, hw), f"step {f} stream {s} vs the host composition")
            composed += len(ref)
        rows_total += sum(len(r) for r, _i in got)
        boxes_total += sum(i["radar_boxes"] for _r, i in got if i["mode"] == 0)
        # host tail, fed with the pickled packed payload
        payload = pickle.loads(pickle.dumps(host_tail.prepare(frames, radar, pack=True)))
        assert payload["img"].frames == [] and tuple(payload["img"].shape) == (n, 3) + CANVAS
        got_host = host_tail.infer(payload)
        for (rows, info), (rows_h, info_h) in zip(got, got_host):
            assert torch.equal(rows, rows_h) and info["mode"] == info_h["mode"] and info["radar_boxes"] == info_h["radar_boxes"]
    assert rows_total > 0 and boxes_total > 0 and composed > 0


def test_square_tuple_is_the_int_fuser(hip_lib):
    from millieye_amd.demo import MultiStreamFuser
    _cpu, net = _nets()
    n = STREAMS
    frames = [mh.stream_frame(s) for s in range(n)]
    kw = dict(model_mode=3, min_hits=mh.MIN_HITS)
    a, b = MultiStreamFuser(net, RADAR_CALIB, n, img_size=(64, 64), **kw), MultiStreamFuser(net, RADAR_CALIB, n, img_size=64, **kw)
    rows_total = 0
    for f in range(4):
        radar = [mh.stream_radar(s, f) for s in range(n)]
        for (rows_a, info_a), (rows_b, info_b) in zip(a(frames, radar), b(frames, radar)):
            assert torch.equal(rows_a, rows_b) and info_a["mode"] == info_b["mode"] and info_a["radar_boxes"] == info_b["radar_boxes"]
            rows_total += len(rows_a)
    assert rows_total > 0


def test_pipeline_carries_the_rectangular_size_to_its_producer(hip_lib):
    """``FusionPipeline`` with a rectangular fuser: the producer process packs for the letterbox kernel (``prepare_streams`` with
    ``img_size=(64, 96)``), the rows equal the in-process fuser's."""
    from millieye_amd.demo import MultiStreamFuser
    from millieye_amd.pipeline import FusionPipeline
    _cpu, net = _nets()
    steps, n = 3, 2
    source = pf.NativeSource(steps, ["rgb"] * n)
    kw = dict(model_mode=3, min_hits=mh.MIN_HITS, img_size=CANVAS)
    local = MultiStreamFuser(net, RADAR_CALIB, n, **kw)
    want = [local(*source.step(f)) for f in range(steps)]
    seen = []
    piped = MultiStreamFuser(net, RADAR_CALIB, n, **kw)

    def infer(payload):
        seen.append((payload["img"].rect, payload["img"].frames, tuple(payload["img"].desc.shape)))
        return piped.infer(payload)

    pipe = FusionPipeline(piped, source, infer=infer, skip_to_newest=False)
    got = list(pipe)
    assert [info["frame_idx"] for _r, info in got] == list(range(steps)) and pipe.stats["dropped"] == 0
    assert seen == [(CANVAS, [], (n, 5))] * steps, "the producer must pack for the rectangular canvas"
    for f, (results, _info) in enumerate(got):
        for (rows, info), (rows_w, info_w) in zip(results, want[f]):
            assert torch.equal(rows, rows_w) and info["mode"] == info_w["mode"] and info["radar_boxes"] == info_w["radar_boxes"]
    assert sum(len(r) for step in want for r, _i in step) > 0
