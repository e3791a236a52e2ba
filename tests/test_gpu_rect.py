"""-m gpu: rectangular inputs [n,3,H,W] (H, W multiples of 32) through the decode kernels, the engine, ``Darknet.forward`` and
``Network.forward``.  Decode rule (Darknet's; the reference's YOLOLayer has one grid_size): one stride = H / gh = W / gw, row
``row_offset + a * gh * gw + gy * gw + gx``.  References: the square entry points bit for bit where a rectangular call has a square
twin, tests/rect_refs.py (float64, pinned to the oracle at square shapes by tests/test_rect_refs_cpu.py) elsewhere.  Every output
buffer the tests hand to the library is pre-filled with NaN."""
import copy
import ctypes as C
import functools

import pytest
import torch

from millieye_amd import synth
from tests import parity_helpers as ph
from tests import rect_refs

pytestmark = pytest.mark.gpu
TOL = 1e-3   # tests/test_gpu_darknet.py's bar (ph.assert_close)
TINY = "yolov3-tiny-12"
TINY_SHAPES = [(64, 96), (96, 64), (32, 128), (128, 32)]
DETECTOR_CASES = [(TINY, n, h, w) for h, w in TINY_SHAPES for n in (1, 3)] + [("yolov3", 1, 64, 96)]
ANCHORS = [(10, 14), (23, 27), (37, 58)]


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


# ---------------------------------------------------------------------------------------------- 1, 2: the entry points
def _desc(rect, x_ptr, pitch, n, grid, nc, rows_total, row_offset, out_ptr, stride=32.0, anchors=ANCHORS):
    from millieye_amd import hip
    d = hip.YoloRectDesc() if rect else hip.YoloDesc()
    d.x, d.x_pitch, d.out = x_ptr, pitch, out_ptr
    d.n, d.num_anchors, d.num_classes = n, len(anchors), nc
    if rect:
        d.gh, d.gw = grid
    else:
        d.g = grid
    d.rows_total, d.row_offset, d.stride = rows_total, row_offset, stride
    for k, (aw, ah) in enumerate(anchors):
        d.anchors[2 * k], d.anchors[2 * k + 1] = aw / stride, ah / stride
    return d


def _decode(d, rect):
    from millieye_amd import hip
    fn = hip.lib().me_yolo_decode_rect_f32 if rect else hip.lib().me_yolo_decode_f32
    hip.check(fn(C.byref(d), hip.stream_ptr()), "decode")


@pytest.mark.parametrize("nc", [12, 80])   # 3 * 17 = 51 and 3 * 85 = 255 channels: rows of one and of two 64-lane halves
def test_rect_decode_equals_the_square_decode_on_crops(hip_lib, nc):
    """A crop [:, :gh, :gw] of a square 6 x 6 map through me_yolo_decode_rect_f32 gives, bit for bit, the rows that
    me_yolo_decode_f32 gives for those cells of the whole map (same stride, same anchors): contiguous, and - the kernels know
    one pitch, the pixel's - in a buffer with the parent's pixel pitch (wider than the channels, padding NaN).  Non-zero
    row_offset, rows_total larger than the scale: the rows around the scale stay NaN."""
    n, g, na = 2, 6, 3
    ch = na * (5 + nc)
    pitch = ch + 9
    parent = _nan(n, g, g, pitch)
    parent[..., :ch] = torch.from_numpy(synth.normal(f"rect/decode/{nc}", (n, g, g, ch)) * 1.5).cuda()
    whole = _nan(n, na * g * g, 5 + nc)
    _decode(_desc(False, parent.data_ptr(), pitch, n, g, nc, na * g * g, 0, whole.data_ptr()), False)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(whole).all())
    whole5 = whole.view(n, na, g, g, 5 + nc)
    for gh, gw in [(1, 4), (4, 1), (2, 3), (3, 2), (5, 6), (6, 6), (3, 3)]:
        rows_scale, off, extra = na * gh * gw, 5, 7
        expect = whole5[:, :, :gh, :gw].reshape(n, rows_scale, 5 + nc)
        dense = parent[:, :gh, :gw, :ch].contiguous()
        pitched = _nan(n, gh, gw, pitch)
        pitched[..., :ch] = dense
        for x, xp, what in ((dense, ch, "contiguous"), (pitched, pitch, "parent's pitch")):
            out = _nan(n, off + rows_scale + extra, 5 + nc)
            _decode(_desc(True, x.data_ptr(), xp, n, (gh, gw), nc, off + rows_scale + extra, off, out.data_ptr()), True)
            torch.cuda.synchronize()
            assert torch.equal(out[:, off:off + rows_scale], expect), f"{gh}x{gw} {what}"
            assert bool(torch.isnan(out[:, :off]).all()) and bool(torch.isnan(out[:, off + rows_scale:]).all()), f"{gh}x{gw} {what}"
        if gh == gw:   # the square entry point on the same crop: the two entry points are one kernel
            out_sq, out_re = _nan(n, rows_scale, 5 + nc), _nan(n, rows_scale, 5 + nc)
            _decode(_desc(False, dense.data_ptr(), ch, n, gh, nc, rows_scale, 0, out_sq.data_ptr()), False)
            _decode(_desc(True, dense.data_ptr(), ch, n, (gh, gw), nc, rows_scale, 0, out_re.data_ptr()), True)
            torch.cuda.synchronize()
            assert torch.equal(out_sq, out_re) and torch.equal(out_sq, expect)


def test_python_decode_takes_an_int_or_a_pair(hip_lib):
    """hip.yolo_decode / YOLOLayer.forward(img_dim=(H, W)) stand-alone against the float64 restatement; a square call through
    the pair form is the int form bit for bit."""
    from millieye_amd import hip
    from millieye_amd.yolov3.models import YOLOLayer
    nc, n = 4, 2
    raw = torch.from_numpy(synth.normal("rect/pydecode", (n, 3 * (5 + nc), 3, 5)))
    ref, _frac = rect_refs.yolo_decode_rect(raw.double(), ANCHORS, nc, (96, 160))
    layer = YOLOLayer(ANCHORS, nc, img_dim=416)
    out, zero = layer(raw.cuda(), img_dim=(96, 160))
    assert zero == 0 and layer.grid_size == (3, 5) and layer.img_dim == (96, 160) and layer.stride == 32
    ph.assert_close(out.cpu().double(), ref, 1e-5, "YOLOLayer.forward(img_dim=(H, W))")   # (one decode: float32 rounding only)
    nhwc = raw.permute(0, 2, 3, 1).contiguous().cuda()
    assert torch.equal(hip.yolo_decode(nhwc, ANCHORS, nc, (96, 160)), out)
    sq = raw[:, :, :, :3].contiguous().cuda()
    a, _ = layer(sq, img_dim=96)
    assert layer.grid_size == 3 and layer.img_dim == 96
    b, _ = layer(sq, img_dim=(96, 96))
    assert torch.equal(a, b) and layer.grid_size == 3 and layer.img_dim == 96


CAND_SMALL2 = [(2, 3), (4, 6)]
CAND_SMALL3 = [(1, 2), (2, 4), (4, 8)]
CAND_416x320 = [(13, 10), (26, 20), (52, 40)]


@pytest.mark.parametrize("n,grids", [(2, CAND_SMALL2), (2, CAND_SMALL3), (1, CAND_416x320), (6, CAND_416x320), (24, CAND_416x320)],
                         ids=["2scales", "3scales", "416x320-rpw1", "416x320-rpw4", "416x320-rpw16"])
def test_rect_candidate_decode_equals_decode_plus_nms(hip_lib, n, grids):
    """me_yolo_decode_cand_multi_rect_f32 (and me_yolo_decode_cand_rect_f32 scale by scale) + me_nms_batched_prepped_f32 against
    me_yolo_decode_rect_f32 + me_nms_batched_f32: the same rows, counts and detections, bit for bit - the identity the header
    states for the square pair.  416 x 320 at batch 1, 6 and 24: one, four and sixteen rows per wave."""
    from millieye_amd import hip
    nc, na = 12, 3
    anchors = [[(116, 90), (156, 198), (373, 326)], [(30, 61), (62, 45), (59, 119)], [(10, 13), (16, 30), (33, 23)]][-len(grids):]
    rows = sum(na * gh * gw for gh, gw in grids)
    img_h = grids[-1][0] * 8 if grids is CAND_416x320 else grids[0][0] * 32
    pitch = 64  # >= 3 * 17 channels
    raws = [torch.from_numpy(synth.normal(f"rect/cand/{n}/{gh}x{gw}", (n, gh, gw, pitch)) * 2.0 - 1.5).cuda().contiguous()
            for gh, gw in grids]
    plain = _nan(n, rows, 5 + nc)
    descs, off = [], 0
    for (gh, gw), raw, an in zip(grids, raws, anchors):
        d = _desc(True, raw.data_ptr(), pitch, n, (gh, gw), nc, rows, off, plain.data_ptr(), stride=img_h / gh, anchors=an)
        _decode(d, True)
        descs.append(d)
        off += na * gh * gw
    torch.cuda.synchronize()
    assert bool(torch.isfinite(plain).all())
    det0, cnt0 = hip.nms_batched(plain.clone(), 0.3, 0.4, 200, writeback_xyxy=False)
    ws, _keep = hip.nms_workspace(n, rows, torch.device("cuda"))
    for multi in (True, False):
        out = _nan(n, rows, 5 + nc)
        for d in descs:
            d.out = out.data_ptr()
        if multi:
            ptrs = (C.c_void_p * len(descs))(*[C.addressof(d) for d in descs])
            hip.check(hip.lib().me_yolo_decode_cand_multi_rect_f32(ptrs, len(descs), 0.3, ws, 1, hip.stream_ptr()), "multi")
        else:
            for i, d in enumerate(descs):
                hip.check(hip.lib().me_yolo_decode_cand_rect_f32(C.byref(d), 0.3, ws, int(i == 0), hip.stream_ptr()), "single")
        det, cnt = hip.nms_batched(out, 0.3, 0.4, 200, writeback_xyxy=False, prepped=True)
        torch.cuda.synchronize()
        assert torch.equal(out, plain), "decoded rows differ from me_yolo_decode_rect_f32"
        assert torch.equal(cnt, cnt0) and int(cnt0.min()) > 0
        for i in range(n):
            k = int(cnt0[i])
            assert torch.equal(det[i, :k], det0[i, :k]), f"image {i}: kept rows differ"
    # the argument checks of the square twin, plus gh, gw > 0
    ptrs = (C.c_void_p * len(descs))(*[C.addressof(d) for d in descs])
    lib, sp = hip.lib(), hip.stream_ptr()
    assert lib.me_yolo_decode_cand_multi_rect_f32(ptrs, 4, 0.3, ws, 1, sp) != 0
    for field in ("gh", "gw"):
        keep = getattr(descs[0], field)
        setattr(descs[0], field, 0)
        assert lib.me_yolo_decode_cand_multi_rect_f32(ptrs, len(descs), 0.3, ws, 1, sp) != 0
        assert lib.me_yolo_decode_cand_rect_f32(C.byref(descs[0]), 0.3, ws, 1, sp) != 0
        assert lib.me_yolo_decode_rect_f32(C.byref(descs[0]), sp) != 0
        setattr(descs[0], field, keep)
    descs[-1].gw += 1   # one column more than rows_total holds
    assert lib.me_yolo_decode_cand_multi_rect_f32(ptrs, len(descs), 0.3, ws, 1, sp) != 0
    assert lib.me_yolo_decode_rect_f32(C.byref(descs[-1]), sp) != 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3 - 7: Darknet.forward
_MODELS = {}


def _model(name, dtype="f32"):
    """One device copy per (cfg, storage mode) for the whole module: its plans (and their tuned tiles) are built once."""
    key = (name, dtype)
    if key not in _MODELS:
        m = copy.deepcopy(rect_refs.detector_case(name, 1, 64, 96)[0]).cuda()
        m.compute_dtype = dtype
        _MODELS[key] = m
    return _MODELS[key]


@functools.lru_cache(maxsize=None)
def _forward(name, n, h, w, dtype="f32", tag=None):
    """``(featuremap, rows)`` of the seeded case on the device, once per session (square shapes: ``tag`` names the frames)."""
    x = rect_refs.frames(tag, n, h, w) if tag else rect_refs.detector_case(name, n, h, w)[1]
    with torch.no_grad():
        fm, rows = _model(name, dtype)(x.cuda())
    torch.cuda.synchronize()
    return fm.cpu(), rows.cpu()


def _assert_cells(name, n, h, w, rows):
    """floor(x / stride), floor(y / stride) are the (gx, gy) the row index implies - exactly: stride is a power of two and the
    sigmoid lies in (0, 1).  Rows whose sigmoid rounded to 0 or 1 sit exactly on a cell border and are left out, 1 % at most."""
    stride, gx, gy = rect_refs.row_cells(rect_refs.detector_case(name, n, h, w)[0], h, w)
    stride, gx, gy = stride.float(), gx.float().expand(n, -1), gy.float().expand(n, -1)
    assert rows.shape[1] == stride.numel()
    cx, cy = rows[..., 0] / stride, rows[..., 1] / stride
    border = (cx == torch.floor(cx)) | (cy == torch.floor(cy))
    assert float(border.float().mean()) <= 0.01, f"{int(border.sum())} of {border.numel()} rows on a cell border"
    assert torch.equal(torch.floor(cx)[~border], gx[~border]), "x does not lie in the cell column the row index implies"
    assert torch.equal(torch.floor(cy)[~border], gy[~border]), "y does not lie in the cell row the row index implies"


@pytest.mark.parametrize("name,n,h,w", DETECTOR_CASES)
def test_rows_lie_in_the_cells_their_index_implies(hip_lib, name, n, h, w):
    _fm, rows = _forward(name, n, h, w)
    assert bool(torch.isfinite(rows).all())
    _assert_cells(name, n, h, w, rows)


@pytest.mark.parametrize("name,n,h,w", DETECTOR_CASES)
def test_values_vs_the_float64_restatement(hip_lib, name, n, h, w):
    _model_cpu, _x, ref_fm, ref_rows, _frac = rect_refs.detector_case(name, n, h, w)
    fm, rows = _forward(name, n, h, w)
    assert tuple(fm.shape) == tuple(ref_fm.shape) == (n, ref_fm.shape[1], h // 16, w // 16)
    e1 = ph.assert_close(fm.double(), ref_fm, TOL, f"{name} {h}x{w} featuremap")
    e2 = ph.assert_close(rows.double(), ref_rows, TOL, f"{name} {h}x{w} rows")
    print(f"{name} n={n} {h}x{w}: featuremap err {e1:.2e}, rows err {e2:.2e}")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name,n", [(TINY, 3), ("yolov3", 1)])
def test_16bit_storage_modes(hip_lib, name, n, dtype):
    """64 x 96 in the 16-bit storage modes: the cell structure exactly; the values by their largest deviation from the fp32
    rows of the same frames, which may be at most twice what the unchanged square path shows at 96 x 96 (other frames and map
    sizes, the same algorithm)."""
    h, w = 64, 96
    _fm, rows16 = _forward(name, n, h, w, dtype)
    _fm, rows32 = _forward(name, n, h, w)
    assert bool(torch.isfinite(rows16).all())
    _assert_cells(name, n, h, w, rows16)
    rect = ph.max_rel_err(rows16, rows32)
    tag = f"rect/square96/{name}/{n}"
    _fm, sq16 = _forward(name, n, 96, 96, dtype, tag)
    _fm, sq32 = _forward(name, n, 96, 96, "f32", tag)
    square = ph.max_rel_err(sq16, sq32)
    print(f"RECT16 {name} n={n} {dtype}: 64x96 max deviation from fp32 {rect:.4e}, 96x96 (square path) {square:.4e}, "
          f"ratio {rect / square:.3f}")
    assert rect <= 2 * square, f"64x96 deviates {rect:.3e} from fp32, the square path at 96x96 {square:.3e}"


@pytest.mark.parametrize("h,w", [(64, 96), (128, 32)])
def test_frames_do_not_depend_on_their_batch(hip_lib, h, w):
    """Each frame of the 3-frame batch against its own batch-1 run, by test_frames_are_independent_across_batch_sizes'
    criterion: 1e-4 of max(1, |ref|)."""
    x = rect_refs.detector_case(TINY, 3, h, w)[1]
    fm3, rows3 = _forward(TINY, 3, h, w)
    model = _model(TINY)
    for i in range(3):
        with torch.no_grad():
            fm1, rows1 = model(x[i:i + 1].contiguous().cuda())
        for got, ref in ((rows1.cpu()[0], rows3[i]), (fm1.cpu()[0], fm3[i])):
            err = (got - ref).abs() / ref.abs().clamp(min=1.0)
            assert float(err.max()) <= 1e-4, (i, float(err.max()))


def test_graph_replay_gives_the_eager_rows(hip_lib):
    """Three runs of one plan under engine.graph_replay(): two eager, the third through the capture."""
    from millieye_amd import engine
    model = copy.deepcopy(rect_refs.detector_case(TINY, 1, 64, 96)[0]).cuda()
    x = rect_refs.detector_case(TINY, 3, 64, 96)[1].cuda()
    with torch.no_grad():
        fm0, rows0 = model(x)
        with engine.graph_replay():
            for _ in range(3):
                fm, rows = model(x)
    torch.cuda.synchronize()
    plan = next(iter(model.engine._plans.values()))
    assert isinstance(plan.graph, dict) and any(rec["graph"] is not None for rec in plan.graph.values()), "no capture happened"
    assert plan.yolo_rect and torch.equal(rows, rows0) and torch.equal(fm, fm0)
    # the layer attributes the reference's YOLOLayer.forward leaves behind: pairs for a rectangular plan
    assert [(l.grid_size, l.img_dim, l.stride) for l in model.yolo_layers] == [((2, 3), (64, 96), 32.0), ((4, 6), (64, 96), 16.0)]


# ---------------------------------------------------------------------------------------------- 8: Network.forward
def _network(tag, conf=0.2):
    from millieye_amd.my_models import Network, define_yolo
    net = Network(define_yolo(ph.cfg_path(TINY)), conf).eval()
    synth.fill_network_(net, tag)
    return net


def _network_inputs(tag, n, h, w):
    side = max(h, w) // 16
    maps, rboxes = synth.radar_inputs(tag + "/radar", n, side)
    maps = torch.from_numpy(maps)[:, :, : h // 16, : w // 16].contiguous()
    return rect_refs.frames(tag + "/x", n, h, w), maps, torch.from_numpy(rboxes)


@pytest.mark.parametrize("h,w", [(64, 96), (96, 64)])
def test_network_modes_vs_the_restatement(hip_lib, h, w):
    """Modes 0, 1 and 2 (mode 2 on its own Network: its threshold is sticky, quirk q3), batch 2, radar boxes in both frames,
    maps [2,3,H/16,W/16]; the comparison and the bar of tests/test_gpu_network.py's network-vs-oracle tests."""
    from tests.test_gpu_network import _cmp_rows
    n, conf, tag = 2, 0.2, f"rect/net/{h}x{w}"
    x, maps, rboxes = _network_inputs(tag, n, h, w)
    assert tuple(maps.shape) == (n, 3, h // 16, w // 16) and sorted(set(rboxes[:, 0].tolist())) == [0.0, 1.0]
    cpu_net = _network(tag, conf)
    scale = torch.tensor([w, h, w, h], dtype=torch.float32)
    xd, md = x.cuda(), maps.cuda()
    net, net2 = _network(tag, conf).cuda(), _network(tag, conf).cuda()
    with torch.no_grad():
        out1 = net(xd, md, rboxes.clone().cuda(), 1)
        rb = rboxes.clone().cuda()
        out0 = net(xd, md, rb, 0)
        rb2 = rboxes.clone().cuda()
        out2 = net2(xd, md, rb2, 2)
    torch.cuda.synchronize()
    assert net2.refine_threshold_img == 1 and net.refine_threshold_img != 1
    for got in (rb, rb2):   # the caller's tensor, scaled in place: x by W, y by H
        assert torch.equal(got[:, 1:].cpu(), rboxes[:, 1:] * scale) and torch.equal(got[:, 0].cpu(), rboxes[:, 0])
    for mode, out in ((1, out1), (0, out0), (2, out2)):
        ref, scaled = rect_refs.network_forward_rect(cpu_net, x, maps, rboxes, mode, conf_thresh=conf)
        assert ref.shape[0] > 0, f"mode {mode}: the case has no output rows"
        assert torch.equal(scaled[:, 1:], rboxes[:, 1:] * scale)
        _cmp_rows(out, ref, f"{h}x{w} mode {mode} vs the restatement")
    assert out0.shape[1] == 8 and out0.device.type == "cuda"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_network_square_rows_through_both_sets_of_entry_points(hip_lib, mode):
    """64 x 64: the call through the rect descriptors and entry points (``DarknetEngine.force_rect``, the cross-check switch)
    gives the rows of the call through the unchanged square ones, bit for bit."""
    n, conf, tag = 2, 0.2, "rect/net/64x64/c"   # (a seed with image proposals: mode 1 has rows too)
    x, maps, rboxes = _network_inputs(tag, n, 64, 64)
    outs = []
    for force in (False, True):
        net = _network(tag, conf).cuda()
        eng = net.base_detector.engine_for(net.base_detector.compute_dtype)
        eng.force_rect = force
        with torch.no_grad():
            outs.append(net(x.cuda(), maps.cuda(), rboxes.clone().cuda(), mode))
        torch.cuda.synchronize()
        plan = next(iter(eng._plans.values()))
        assert plan.yolo_rect is force and type(plan.yolo_descs[0]).__name__ == ("YoloRectDesc" if force else "YoloDesc")
    assert outs[0].shape[0] > 0 and torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------- 9: refusals
def test_what_is_out_of_scope_is_refused_loudly(hip_lib):
    from millieye_amd import hip
    from millieye_amd.detector_train import DetectorTrainer
    from millieye_amd.detector_train16 import DetectorTrainer16
    from millieye_amd.yolov3.models import YOLOLayer
    model = copy.deepcopy(rect_refs.detector_case(TINY, 1, 64, 96)[0]).cuda()
    x = rect_refs.detector_case(TINY, 1, 64, 96)[1].cuda()
    targets = torch.tensor([[0, 1, 0.5, 0.5, 0.2, 0.2]])

    def refused(call, *needles):
        with pytest.raises(hip.MeError) as info:
            with torch.no_grad():
                call()
        for needle in needles:
            assert needle in str(info.value), str(info.value)

    refused(lambda: model(x, targets), "64 x 96")                                   # targets: the YOLO loss
    with pytest.raises(hip.MeError, match="64 x 96"):                               # ... under autograd as well
        model(x, targets)
    refused(lambda: DetectorTrainer(model).forward(x), "64 x 96")                   # detector_train*.py
    model.compute_dtype = "bf16"
    refused(lambda: DetectorTrainer16(model).forward(x), "64 x 96")
    model.compute_dtype = "f32"
    model.train()
    refused(lambda: model(x), "64 x 96")                                            # train-mode BatchNorm (_forward_batch_stats)
    model.eval()
    for h, w in ((64, 80), (48, 64), (100, 64)):                                    # not a multiple of 32
        refused(lambda: model(torch.rand(1, 3, h, w, device="cuda")), f"{h} x {w}")
    layer = YOLOLayer(ANCHORS, 4, img_dim=96)
    raw = torch.randn(1, 27, 2, 3, device="cuda")
    refused(lambda: layer(raw), "2 x 3")                                            # a non-square map with an int img_dim
    refused(lambda: hip.yolo_decode(raw.permute(0, 2, 3, 1).contiguous(), ANCHORS, 4, 96), "2 x 3")
    refused(lambda: hip.yolo_decode(raw.permute(0, 2, 3, 1).contiguous(), ANCHORS, 4, (64, 64)), "2 x 3")   # two strides
    refused(lambda: layer(raw, targets, img_dim=(64, 96)), "2 x 3")                 # whatever reaches loss_from_raw
    layer.img_dim = (64, 96)
    refused(lambda: layer.loss_from_raw(raw.permute(0, 2, 3, 1).contiguous(), targets), "2 x 3")
    # Network.forward: targets (either call form) and frame_modes
    tag = "rect/net/64x96"
    net = _network(tag).cuda()
    xn, maps, rboxes = _network_inputs(tag, 2, 64, 96)
    args = (xn.cuda(), maps.cuda())
    net_targets = torch.tensor([[0, 0, 0.5, 0.5, 0.2, 0.2]])
    refused(lambda: net(*args, rboxes.clone().cuda(), 0, net_targets), "64 x 96")
    refused(lambda: net(*args, rboxes.clone().cuda(), net_targets), "64 x 96")
    refused(lambda: net(*args, rboxes.clone().cuda(), frame_modes=[0, 1]), "64 x 96")
    net.train()
    refused(lambda: net(*args, rboxes.clone().cuda(), 0), "64 x 96")                # train-mode heads (forward_train)
    torch.cuda.synchronize()
