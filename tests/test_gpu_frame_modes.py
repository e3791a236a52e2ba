"""-m gpu: per-frame modes - ``me_roi_heads_modes_f32``, ``me_compact_sort_rows_modes_f32``, ``me_frame_modes_f32`` through the C
ABI, ``Network.forward(..., frame_modes=)`` and ``MultiStreamFuser(split="frame_modes")``.

Every comparison is bitwise (``torch.equal``, float arrays through their int32 views so that the NaN poison compares too): the
feature adds no arithmetic.  A mode-0 RoI runs the code ``me_roi_heads_f32`` runs for it (the rows of the 32-RoI MFMA tile are
independent), a skipped RoI is copied or dropped, and the two-segment order is a permutation.  The only tolerant comparison is
the existing one of ``tests.test_gpu_multistream`` between the batched fuser and the batch-1 ``FrameFuser``s (another detector
plan), with that file's own helpers."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from millieye_amd import synth
from tests import frame_modes_refs as refs
from tests import multistream_helpers as mh
from tests.golden.make_golden import RADAR_CALIB

pytestmark = pytest.mark.gpu


def _i32(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def net(hip_lib):
    from tests.test_gpu_multistream import _net
    return _net()


# ---- heads ---------------------------------------------------------------------------------------------------------------------
N_FRAMES, MAP = 3, 10
ARRAYS = (("regress", 4), ("refine", 2), ("mask1", 0), ("rows", 8), ("key", 0), ("pooled", 980))


def _boxes(tag, per_frame):
    """``[k,5]`` valid boxes (frame, x1, y1, x2, y2) in pixels of the 160-pixel input, frame-major."""
    k = sum(per_frame)
    size = 16.0 * MAP
    c = synth.uniform(tag + "/c", (k, 2), 0.15 * size, 0.85 * size)
    half = synth.uniform(tag + "/h", (k, 2), 3.0, 0.4 * size)
    idx = np.repeat(np.arange(len(per_frame), dtype=np.float32), per_frame)[:, None]
    return torch.from_numpy(np.concatenate([idx, c - half, c + half], 1).astype(np.float32))


class _Heads:
    """One heads problem on the device: synthetic score maps of three 10 x 10 frames, ``img_per_frame`` image proposals and
    ``rad_per_frame`` radar boxes; ``run(frame_mode)`` fills fresh poisoned outputs."""

    def __init__(self, net, tag, img_per_frame, rad_per_frame, slack=21):
        from millieye_amd import hip
        dev = torch.device("cuda")
        self.dev, self.hip = dev, hip
        self.k_img, self.k_rad = sum(img_per_frame), sum(rad_per_frame)
        self.cols = 8 + net.class_num
        self.cap_img = self.k_img + slack   # slots behind the last proposal, like n * detections_per_img
        self.cap = self.cap_img + self.k_rad
        self.img_map = torch.from_numpy(synth.uniform(tag + "/m490", (N_FRAMES, MAP, MAP, 490), -1, 1)).to(dev)
        rad_map = torch.zeros((N_FRAMES, MAP, MAP, 12))
        rad_map[..., :10] = torch.from_numpy(synth.uniform(tag + "/m10", (N_FRAMES, MAP, MAP, 10), 0, 1))
        self.rad_map = rad_map.to(dev)
        boxes = torch.zeros((self.cap_img, self.cols))
        if self.k_img:
            boxes[:self.k_img, :5] = _boxes(tag + "/img", img_per_frame)
            boxes[:self.k_img, 5:] = torch.from_numpy(synth.uniform(tag + "/conf", (self.k_img, self.cols - 5), 0.05, 0.95))
            boxes[:self.k_img, 7] = 0.0
        self.img_boxes = boxes.to(dev)
        self.n_img = torch.tensor([self.k_img], dtype=torch.int32, device=dev)
        self.rad = _boxes(tag + "/rad", rad_per_frame).to(dev) if self.k_rad else None
        # the frame of every RoI slot (image proposals, then radar boxes)
        frames = [self.img_boxes[:self.k_img, 0]] + ([self.rad[:, 0]] if self.k_rad else [])
        self.frame_of = torch.cat(frames).long().cpu()
        assert int(self.frame_of.min()) >= 0 and int(self.frame_of.max()) < N_FRAMES   # only valid frame indices are fed
        self.weights = net._get_packs()["heads"].refresh(dev)
        self.thr = (0.0, 0.0)

    def split_thresholds(self):
        """Put each threshold at the median foreground score of its kind of RoI, so that ``keep`` holds zeros and ones."""
        mask1 = self.run(None)["mask1"]
        img, rad = mask1[:self.k_img], mask1[self.k_img:self.k_img + self.k_rad]
        self.thr = (float(img.median()) if self.k_img else 0.0, float(rad.median()) if self.k_rad else 0.0)

    def run(self, frame_mode):
        """``frame_mode``: None -> ``me_roi_heads_f32``; a list of N_FRAMES ints -> ``me_roi_heads_modes_f32``."""
        hip, dev, cap = self.hip, self.dev, self.cap
        out = {name: torch.full((cap, w) if w else (cap,), float("nan"), device=dev) for name, w in ARRAYS}
        out["keep"] = torch.full((cap,), 0xFF, dtype=torch.uint8, device=dev)
        d = hip.HeadsDesc()
        d.img_map, d.radar_map = self.img_map.data_ptr(), self.rad_map.data_ptr()
        d.img_pitch, d.radar_pitch, d.img_bin_major = 490, 12, 1
        d.n, d.fh, d.fw, d.spatial_scale, d.rh, d.rw = N_FRAMES, MAP, MAP, 1.0 / 16, MAP, MAP
        d.img_boxes, d.n_img, d.n_img_cap, d.box_cols = self.img_boxes.data_ptr(), self.n_img.data_ptr(), self.cap_img, self.cols
        d.radar_boxes, d.n_radar = (self.rad.data_ptr() if self.k_rad else None), self.k_rad
        d.thr_img, d.thr_radar, d.regress = self.thr[0], self.thr[1], 1
        for nm in ("w0t", "b0", "w1", "b1", "w2", "b2", "rw", "rscale", "rshift", "rw2", "rb2", "e1w", "e1b", "e2w", "e2b"):
            setattr(d.wts, nm, self.weights[nm].data_ptr())
        d.regress_out, d.refine_out, d.mask1_out = out["regress"].data_ptr(), out["refine"].data_ptr(), out["mask1"].data_ptr()
        d.out_rows, d.keep, d.sort_key = out["rows"].data_ptr(), out["keep"].data_ptr(), out["key"].data_ptr()
        d.pool_scratch = out["pooled"].data_ptr()
        lib = hip.lib()
        if frame_mode is None:
            hip.check(lib.me_roi_heads_f32(C.byref(d), hip.stream_ptr()), "me_roi_heads_f32")
        else:
            modes = torch.tensor(frame_mode, dtype=torch.int32, device=dev)
            hip.check(lib.me_roi_heads_modes_f32(C.byref(d), modes.data_ptr(), hip.stream_ptr()), "me_roi_heads_modes_f32")
        torch.cuda.synchronize()
        self.desc = d
        return {k: v.cpu() for k, v in out.items()}

    def expected(self, ref, frame_mode):
        """What ``me_roi_heads_modes_f32`` must leave in the poisoned arrays, from the ``me_roi_heads_f32`` result ``ref``."""
        k = self.k_img + self.k_rad
        live = torch.zeros(self.cap, dtype=torch.bool)
        live[:k] = torch.tensor(frame_mode)[self.frame_of] == 0
        skipped_img = ~live & (torch.arange(self.cap) < self.k_img)
        want = {name: torch.full_like(ref[name], float("nan")) for name, _w in ARRAYS}
        want["keep"] = torch.full_like(ref["keep"], 0xFF)
        for name in want:
            want[name][live] = ref[name][live]
        want["rows"][skipped_img] = self.img_boxes.cpu()[:, :8][skipped_img[:self.cap_img]]
        want["keep"][skipped_img] = 2
        want["keep"][self.k_img:k][~live[self.k_img:k]] = 0          # skipped radar RoIs
        want["keep"][k:] = 0                                         # slots behind the last RoI
        return want, live


def _check_heads(h, ref, frame_mode):
    got = h.run(list(frame_mode))
    want, live = h.expected(ref, frame_mode)
    for name in want:
        assert torch.equal(_i32(got[name]), _i32(want[name])), f"modes {frame_mode}: {name} differs"
    return live


def test_heads_every_mode_pattern_vs_plain_call(net):
    h = _Heads(net, "fm/heads", (40, 20, 15), (3, 3, 3))
    assert (h.k_img, h.k_rad, h.cap) == (75, 9, 105)
    h.split_thresholds()
    ref = h.run(None)
    k = h.k_img + h.k_rad
    assert not ref["rows"][:k].isnan().any() and set(ref["keep"][:k].tolist()) == {0, 1}, "the reference must keep some, drop some"
    assert bool((ref["keep"][k:] == 0).all())
    shapes = set()
    for frame_mode in itertools.product((0, 1), repeat=N_FRAMES):
        live = _check_heads(h, ref, frame_mode)
        for g in range(0, k, 32):   # what the 32-RoI workgroups of this pattern look like
            tile = live[g:min(g + 32, k)]
            shapes.add("all skipped" if not tile.any() else "all live" if tile.all() else "mixed")
    assert shapes == {"all skipped", "all live", "mixed"}
    # any non-zero value is camera only
    want, _ = h.expected(ref, (0, 1, 1))
    got = h.run([0, 7, -1])
    for name in want:
        assert torch.equal(_i32(got[name]), _i32(want[name])), f"non-zero modes: {name} differs"


@pytest.mark.parametrize("img_per_frame,rad_per_frame", [((0, 0, 0), (3, 3, 3)), ((40, 20, 15), (0, 0, 0))])
def test_heads_without_image_proposals_or_radar_boxes(net, img_per_frame, rad_per_frame):
    h = _Heads(net, "fm/heads-edge", img_per_frame, rad_per_frame, slack=8)
    h.split_thresholds()
    ref = h.run(None)
    for frame_mode in ((0, 0, 0), (1, 0, 1), (1, 1, 1)):
        _check_heads(h, ref, frame_mode)


def test_heads_refusals(net):
    from millieye_amd import hip
    h = _Heads(net, "fm/heads-edge", (4, 0, 0), (1, 0, 0), slack=3)
    h.run([0, 0, 0])
    d, lib = h.desc, hip.lib()
    modes = torch.zeros(N_FRAMES, dtype=torch.int32, device="cuda")
    scratch = torch.empty((h.cap, 980), device="cuda")
    bad_arg, null_ptr = -1, -2   # ME_E_BADARG, ME_E_NULLPTR
    d.pool_scratch = None
    assert lib.me_roi_heads_modes_f32(C.byref(d), modes.data_ptr(), hip.stream_ptr()) == bad_arg
    d.pool_scratch = scratch.data_ptr()
    save = torch.empty((h.cap, 256), device="cuda")
    d.save_hidden = save.data_ptr()
    assert lib.me_roi_heads_modes_f32(C.byref(d), modes.data_ptr(), hip.stream_ptr()) == bad_arg
    d.save_hidden = None
    assert lib.me_roi_heads_modes_f32(C.byref(d), None, hip.stream_ptr()) == null_ptr
    with pytest.raises(hip.MeError, match="pool_scratch"):
        d.pool_scratch = None
        hip.check(lib.me_roi_heads_modes_f32(C.byref(d), modes.data_ptr(), hip.stream_ptr()), "me_roi_heads_modes_f32")


# ---- compaction ------------------------------------------------------------------------------------------------------------------
def _compact(lib_fn, rows, keep, key, n_counts):
    from millieye_amd import hip
    cap = rows.shape[0]
    out = torch.full((cap, 8), float("nan"), device="cuda")
    cnt = torch.full((n_counts,), -1, dtype=torch.int32, device="cuda")
    hip.check(lib_fn(rows.data_ptr(), keep.data_ptr(), key.data_ptr(), cap, 8, out.data_ptr(), cnt.data_ptr(), hip.stream_ptr()),
              "compaction")
    return out.cpu(), cnt.tolist()


@pytest.mark.parametrize("values", [(0, 1, 2), (0, 2), (0, 1), (0,)], ids=["mixed", "no ranked", "no passed", "neither"])
def test_compaction_two_segments_across_the_key_tile(hip_lib, values):
    from millieye_amd import hip
    lib, cap = hip.lib(), 2100   # (one 2048-key LDS tile and 52 keys of the next)
    g = torch.Generator().manual_seed(5 + len(values))
    keep = torch.tensor(values, dtype=torch.uint8)[torch.randint(0, len(values), (cap,), generator=g)]
    key = torch.randint(0, 40, (cap,), generator=g).float() / 40   # exact ties
    rows = torch.randn((cap, 8), generator=g)
    for v in values:   # every value on both sides of the tile boundary
        assert (keep[:2048] == v).any() and (keep[2048:] == v).any()
    out, counts = _compact(lib.me_compact_sort_rows_modes_f32, rows.cuda(), keep.cuda(), key.cuda(), 2)
    order, want_counts = refs.two_segment_order(keep.numpy(), key.numpy())
    assert tuple(counts) == want_counts
    m = sum(want_counts)
    assert torch.equal(_i32(out[:m]), _i32(rows[torch.from_numpy(order)])), "rows / order differ"
    assert bool(out[m:].isnan().all()), "rows behind the last one were written"
    if 2 not in values:   # keep in {0, 1}: the bits and the count of me_compact_sort_rows_f32
        plain, plain_count = _compact(lib.me_compact_sort_rows_f32, rows.cuda(), keep.cuda(), key.cuda(), 1)
        assert plain_count[0] == counts[0] and counts[1] == 0
        assert torch.equal(_i32(plain), _i32(out))
    if len(values) == 3:   # the segments are non-trivial and the ranked one holds ties
        assert want_counts[0] > 40 and want_counts[1] > 40


def test_compaction_empty(hip_lib):
    from millieye_amd import hip
    none = torch.empty((0, 8), device="cuda")
    _out, counts = _compact(hip.lib().me_compact_sort_rows_modes_f32, none, none[:, 0].to(torch.uint8), none[:, 0], 2)
    assert counts == [0, 0]


# ---- hip.frame_modes ----------------------------------------------------------------------------------------------------------------
def test_frame_modes_means_and_rule(hip_lib):
    from millieye_amd import hip
    x = torch.from_numpy(synth.uniform("fm/means", (5, 3, 97, 61), 0.0, 0.16)).cuda()
    x[0] *= 0.1
    modes, means = hip.frame_modes(x, 0.08)
    assert modes.dtype == torch.int32 and modes.is_cuda and tuple(modes.shape) == (5,)
    assert torch.equal(means, hip.frame_means(x))
    assert np.array_equal(modes.cpu().numpy(), refs.mode_rule(means.cpu().numpy(), 0.08))
    assert int(modes[0]) == 0
    # the edge: constant frames of four pixels have their value as mean, exactly
    edge = np.float32(0.08)
    vals = np.array([edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1)), 0.0, 1.0], dtype=np.float32)
    frames = torch.from_numpy(np.repeat(vals[:, None], 4, 1)).cuda()
    modes, means = hip.frame_modes(frames, 0.08)
    assert torch.equal(means.cpu(), torch.from_numpy(vals)) and torch.equal(means, hip.frame_means(frames))
    assert modes.cpu().tolist() == [0, 0, 1, 0, 1] == refs.mode_rule(vals, 0.08).tolist()
    with pytest.raises(hip.MeError):
        hip.frame_modes(frames.cpu(), 0.08)
    with pytest.raises(hip.MeError):
        hip.frame_modes(frames.t(), 0.08)


# ---- Network.forward ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forward_case(net):
    """N = 5 frames at 160 x 160 with two radar boxes each, and the two whole-batch scalar calls every vector is compared with."""
    n, s = 5, 160
    x = torch.from_numpy(synth.uniform("fm/net/x", (n, 3, s, s))).to(net.device)
    maps, rboxes = synth.radar_inputs("fm/net/radar", n, s // 16)
    maps, rboxes = torch.from_numpy(maps).to(net.device), torch.from_numpy(rboxes).to(net.device)
    with torch.no_grad():
        net(x, maps, rboxes.clone(), 0)   # (builds and tunes the batch-5 plan)
        rows0 = net(x, maps, rboxes.clone(), 0).clone()
        rows1 = net(x, maps, rboxes.clone(), 1).clone()
    assert len(rows0) and len(rows1)
    return dict(n=n, s=s, x=x, maps=maps, rboxes=rboxes, rows0=rows0, rows1=rows1)


@pytest.mark.parametrize("on_device", [False, True], ids=["host vector", "device tensor"])
@pytest.mark.parametrize("modes", [(0, 1, 0, 1, 1), (0, 0, 0, 0, 0), (1, 1, 1, 1, 1)])
def test_network_forward_frame_modes(net, forward_case, modes, on_device):
    c = forward_case
    m = torch.tensor(modes, device=net.device)
    want0 = c["rows0"][m[c["rows0"][:, 0].long()] == 0]
    want1 = c["rows1"][m[c["rows1"][:, 0].long()] == 1]
    arg = torch.tensor(modes, dtype=torch.int32, device=net.device) if on_device else list(modes)
    rb = c["rboxes"].clone()
    with torch.no_grad():
        got = net(c["x"], c["maps"], rb, frame_modes=arg)
    assert torch.equal(got, torch.cat([want0, want1])), f"modes {modes}"
    assert net._last["counts"] == (len(want0), len(want1))
    if 0 in modes and 1 in modes:
        assert len(want0) and len(want1) and len(want0) < len(c["rows0"]) and len(want1) < len(c["rows1"])
    # the caller's radar boxes: scaled in place, exactly once - also when no frame refines
    assert torch.equal(rb[:, 0], c["rboxes"][:, 0]) and torch.equal(rb[:, 1:], c["rboxes"][:, 1:] * c["s"])
    if not on_device:   # numpy vectors are host sequences too
        with torch.no_grad():
            again = net(c["x"], c["maps"], c["rboxes"].clone(), frame_modes=np.array(modes))
        assert torch.equal(again, got)


def test_network_forward_frame_modes_refusals(net, forward_case):
    from millieye_amd import hip
    c = forward_case

    def call(frame_modes, *args, **kwargs):
        rb = c["rboxes"].clone()
        with pytest.raises(hip.MeError):
            net(c["x"], c["maps"], rb, *args, frame_modes=frame_modes, **kwargs)
        assert torch.equal(rb, c["rboxes"]), "a refused call must leave the radar boxes alone"

    ok = [0, 1, 0, 1, 1]
    call(ok[:4])                                                              # wrong length
    call(torch.tensor(ok[:4], dtype=torch.int32, device=net.device))
    call([0, 1, 2, 0, 1])                                                     # a host value that is neither 0 nor 1
    call(torch.tensor(ok, dtype=torch.int64, device=net.device))              # a device tensor of another type
    call(ok, targets=torch.zeros((0, 6), device=net.device))                  # with targets
    call(ok, torch.zeros((0, 6), device=net.device))                          # ... in the model_mode slot (train.py's call form)
    call(ok, 1)                                                               # with a model_mode
    call(ok, 2)
    net.train()
    try:
        call(ok)                                                              # head BatchNorms in train() mode
    finally:
        net.eval()


# ---- MultiStreamFuser(split="frame_modes") ---------------------------------------------------------------------------------------
STREAMS_N = 6


@pytest.fixture(scope="module")
def fuser_refs(net):
    """The scenario of tests.test_gpu_multistream.test_fuser_equivalence, computed once: per step the frames, the radar frames,
    the per-stream ``FrameFuser`` results, and the results of two ``MultiStreamFuser``s at fixed ``model_mode`` 0 / 1 (the
    two-forward code path never splits there) fed the same steps."""
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    n = STREAMS_N
    dark = [mh.stream_frame(s) for s in range(n)]
    bright = [mh.stream_frame(s, dark=False) for s in range(n)]
    assert len({f.shape for f in dark}) == 2
    singles = [FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=mh.MIN_HITS) for _ in range(n)]
    fixed = [MultiStreamFuser(net, RADAR_CALIB, n, model_mode=m, min_hits=mh.MIN_HITS) for m in (0, 1)]
    steps = []
    for f in range(7):   # six mixed steps, then all streams bright
        frames = dark if f < 6 else bright
        radar = [mh.stream_radar(s, f) for s in range(n)]
        steps.append(dict(frames=frames, radar=radar, single=[singles[s](frames[s], radar[s]) for s in range(n)],
                          fixed=[fu(frames, radar) for fu in fixed]))
    single = FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=mh.MIN_HITS)
    one = [single(dark[1], mh.stream_radar(1, f)) for f in range(3)]
    return dict(steps=steps, one=one, frame1=dark[1])


@pytest.mark.parametrize("tail", ["device", "host"])
def test_fuser_frame_modes_split(net, fuser_refs, tail):
    from millieye_amd.demo import MultiStreamFuser
    from tests.test_gpu_multistream import _cmp_step
    n = STREAMS_N
    multi = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, tail=tail, split="frame_modes")
    rows_total = boxes_total = 0
    for f, step in enumerate(fuser_refs["steps"]):
        got = multi(step["frames"], step["radar"])
        modes = [info["mode"] for _r, info in got]
        if f < 6:
            assert 0 in modes and 1 in modes, "both modes must be present"
        else:
            assert all(m == 1 for m in modes)
        _cmp_step(got, step["single"], step["frames"], f"{tail} tail, step {f}")
        for s in range(n):   # bit for bit what the whole batch gives at this stream's mode
            rows_w, info_w = step["fixed"][modes[s]][s]
            assert torch.equal(got[s][0], rows_w), f"{tail} tail, step {f}, stream {s} (mode {modes[s]})"
            assert np.array_equal(got[s][1]["proposals"], info_w["proposals"])
        rows_total += sum(len(r) for r, _i in got)
        boxes_total += sum(i["radar_boxes"] for _r, i in got if i["mode"] == 0)
    assert rows_total > 0 and boxes_total > 0
    one = MultiStreamFuser(net, RADAR_CALIB, 1, model_mode=3, min_hits=mh.MIN_HITS, tail=tail, split="frame_modes")
    frame = fuser_refs["frame1"]
    for f in range(3):
        _cmp_step(one([frame], [mh.stream_radar(1, f)]), [fuser_refs["one"][f]], [frame], f"{tail} tail, S=1 step {f}")


def test_fuser_fixed_modes_and_bad_split(net, fuser_refs):
    from millieye_amd import hip
    from millieye_amd.demo import MultiStreamFuser
    n = STREAMS_N
    with pytest.raises(hip.MeError):
        MultiStreamFuser(net, RADAR_CALIB, n, split="modes")
    step = fuser_refs["steps"][0]   # (fresh trackers: the first step of the scenario)
    for mode in (0, 1):
        fuser = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=mode, min_hits=mh.MIN_HITS, split="frame_modes")
        got = fuser(step["frames"], step["radar"])
        for s in range(n):
            assert got[s][1]["mode"] == mode and torch.equal(got[s][0], step["fixed"][mode][s][0])


def test_fuser_frame_modes_builds_one_plan(hip_lib):
    """Three steps with three different numbers of dark streams: one detector plan (the two-forward split builds one per
    sub-batch size)."""
    from millieye_amd.demo import MultiStreamFuser
    from tests.test_gpu_multistream import _net
    fresh, n = _net(), 4
    plans = fresh.base_detector.engine_for(fresh.base_detector.compute_dtype)._plans
    assert len(plans) == 0
    multi = MultiStreamFuser(fresh, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, split="frame_modes")
    seen = set()
    for f, dark_count in enumerate((1, 3, 2)):
        frames = [mh.stream_frame(s, dark=s < dark_count) for s in range(n)]
        got = multi(frames, [mh.stream_radar(s, f) for s in range(n)])
        assert [info["mode"] for _r, info in got] == [0 if s < dark_count else 1 for s in range(n)]
        seen.add(dark_count)
    assert len(seen) == 3 and len(plans) == 1
