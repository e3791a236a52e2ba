"""-m gpu: the multi-stream output tail.  me_nms_boxes_grouped_f32 against me_nms_boxes_f32 per group (the contract: equal bit
for bit and in order) and against the oracle's batched_nms per group; me_stream_tail_f32 against the CPU restatement
(tests/stream_tail_refs.py) and against the "host" path; MultiStreamFuser(tail="device") against tail="host"; the two-process
pipeline for S streams against the in-process fuser.  Every comparison is exact.  tests/test_stream_tail_cpu.py guards the inputs."""
import numpy as np
import pytest
import torch

from tests import multistream_helpers as mh
from tests import stream_tail_refs as refs
from tests.golden.make_golden import RADAR_CALIB

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


def _cluster_group(n, seed, classes=4):
    """``n`` clustered boxes in network-input pixels with score ties."""
    rows = refs.synthetic_rows(1, [n], seed, classes=classes)
    return rows[:, 1:5].copy(), rows[:, 5].copy(), rows[:, 7].copy()


def _check_groups(groups, iou, use_labels=True, oracle_scores=None):
    """The grouped call on ``groups`` (a list of (boxes, scores, labels)) against the per-group device call and the oracle."""
    from millieye_amd import hip
    from oracle import tv_ops
    sizes = [len(g[0]) for g in groups]
    boxes = torch.from_numpy(np.concatenate([g[0] for g in groups], 0).astype(np.float32).reshape(-1, 4)).cuda()
    scores = torch.from_numpy(np.concatenate([g[1] for g in groups], 0).astype(np.float32)).cuda()
    labels = torch.from_numpy(np.concatenate([g[2] for g in groups], 0).astype(np.float32)).cuda() if use_labels else None
    got = hip.nms_indices_segmented(boxes, scores, labels, sizes, iou)
    assert len(got) == len(groups)
    start = 0
    for g, size in enumerate(sizes):
        rows = slice(start, start + size)
        alone = hip.nms_indices(boxes[rows], scores[rows], labels[rows] if use_labels else None, iou).cpu() + start
        assert got[g].dtype == torch.int64 and torch.equal(got[g], alone), \
            f"group {g} ({size} rows): the grouped call differs from me_nms_boxes_f32 on the group alone"
        b, s = boxes[rows].cpu(), (scores[rows].cpu() if oracle_scores is None else torch.from_numpy(oracle_scores[g]))
        want = (tv_ops.batched_nms(b, s, labels[rows].cpu(), iou) if use_labels else tv_ops.nms(b, s, iou)) + start
        assert torch.equal(got[g], want), f"group {g} ({size} rows): the grouped call differs from the oracle"
        start += size
    return got


@pytest.mark.parametrize("iou", [0.3, 0.5])
def test_grouped_nms_small_and_empty_groups(hip_lib, iou):
    sizes = [0, 1, 65, 0, 300, 7, 0]
    got = _check_groups([_cluster_group(n, 20 + i) for i, n in enumerate(sizes)], iou)
    assert [len(k) for k in got][0::3] == [0, 0, 0] and 0 < len(got[4]) < 300
    _check_groups([_cluster_group(n, 30 + i) for i, n in enumerate(sizes)], iou, use_labels=False)


@pytest.mark.parametrize("big", [800, 1100, 4200])  # past MAT_CANDS (768), MATN (1024) and LDS_CANDS (4096)
def test_grouped_nms_a_large_group_beside_small_ones(hip_lib, big):
    got = _check_groups([_cluster_group(40, 1), _cluster_group(big, big), _cluster_group(0, 2), _cluster_group(130, 3)], 0.3)
    assert 0 < len(got[1]) < big


def test_grouped_nms_keeps_one_maximum_per_group(hip_lib):
    """The A / B fixture: B's coordinates reach 1e5; with a maximum shared between the groups A's kept set changes
    (tests/test_stream_tail_cpu.py measures by how many rows)."""
    b = refs.group_b()
    for n, seed in ((65, 1), (300, 2)):
        a = refs.group_a(n, seed)
        for iou in (0.3, 0.5):
            got = _check_groups([a, b], iou)
            _check_groups([b, a], iou)
        joint = refs.joint_call_kept(a, b, 0.5)
        assert set(got[0].tolist()) != set(joint.tolist()), "the fixture no longer tells a shared maximum apart"


def test_grouped_nms_nan_and_ties(hip_lib):
    # a NaN coordinate in ONE group: torch's max is NaN for that group only - it keeps every row, its neighbours do not
    a, b, c = _cluster_group(90, 41), _cluster_group(120, 42), _cluster_group(65, 43)
    b[0][17, 2] = np.nan
    got = _check_groups([a, b, c], 0.3)
    assert len(got[1]) == 120 and len(got[0]) < 90 and len(got[2]) < 65
    # a NaN score sorts first (torch.sort, descending); the oracle's comparator is not defined for NaN, so it gets +inf in
    # that place - the same position in the order, and scores take no part in the IoU test
    a, b = _cluster_group(100, 44), _cluster_group(70, 45)
    a[1][33] = np.nan
    inf_scores = a[1].copy()
    inf_scores[33] = np.inf
    got = _check_groups([a, b], 0.3, oracle_scores=[inf_scores, b[1]])
    assert int(got[0][0]) == 33
    # all scores equal: the lower row first
    a, b = _cluster_group(150, 46), _cluster_group(64, 47)
    a[1][:] = 0.5
    b[1][:] = 0.25
    got = _check_groups([a, b], 0.5)
    assert int(got[0][0]) == 0 and int(got[1][0]) == 150
    assert torch.equal(got[0], torch.sort(got[0]).values), "equal scores: kept rows in row order"


def test_grouped_nms_refuses_a_group_over_cap_without_writing_past_its_slots(hip_lib):
    from millieye_amd import hip
    sizes = [30, 200, 12]
    groups = [_cluster_group(n, 50 + i) for i, n in enumerate(sizes)]
    boxes = torch.from_numpy(np.concatenate([g[0] for g in groups], 0)).cuda()
    scores = torch.from_numpy(np.concatenate([g[1] for g in groups], 0)).cuda()
    labels = torch.from_numpy(np.concatenate([g[2] for g in groups], 0)).cuda()
    with pytest.raises(hip.MeError, match=r"group 1 .*200 rows.*cap = 64"):
        hip.nms_indices_segmented(boxes, scores, labels, sizes, 0.3, cap=64)
    # the raw call: guard words around keep / keep_count and behind the workspace stay intact, the other groups are served
    m, n, cap, pad = sum(sizes), len(sizes), 64, 64
    keep = torch.full((pad + m + pad,), GUARD, dtype=torch.int64, device="cuda")
    count = torch.full((pad + n + pad,), GUARD, dtype=torch.int32, device="cuda")
    nbytes = int(hip.lib().me_nms_workspace_bytes(n, cap))
    ws = torch.full((nbytes // 4 + 64 + pad,), GUARD, dtype=torch.int32, device="cuda")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    ws_off = (ws_ptr - ws.data_ptr()) // 4
    start = torch.tensor([0, 30, 230, 242], dtype=torch.int32).cuda()
    hip.check(hip.lib().me_nms_boxes_grouped_f32(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), start.data_ptr(), n, m,
                                                 cap, 0.3, keep[pad:].data_ptr(), count[pad:].data_ptr(), ws_ptr,
                                                 hip.stream_ptr()), "me_nms_boxes_grouped_f32")
    torch.cuda.synchronize()
    keep_h, count_h, ws_h = keep.cpu(), count.cpu(), ws.cpu()
    assert bool((keep_h[:pad] == GUARD).all()) and bool((keep_h[pad + m:] == GUARD).all())
    assert bool((count_h[:pad] == GUARD).all()) and bool((count_h[pad + n:] == GUARD).all())
    assert bool((ws_h[:ws_off] == GUARD).all()) and bool((ws_h[ws_off + nbytes // 4:] == GUARD).all())
    assert bool((keep_h[pad + 30:pad + 230] == GUARD).all()), "the refused group's keep rows must stay untouched"
    counts = count_h[pad:pad + n].tolist()
    assert counts[1] == -1
    for g, lo, size in ((0, 0, 30), (2, 230, 12)):
        rows = slice(lo, lo + size)
        alone = hip.nms_indices(boxes[rows], scores[rows], labels[rows], 0.3).cpu() + lo
        assert counts[g] == len(alone) and torch.equal(keep_h[pad + lo:pad + lo + counts[g]], alone)


def _tail_inputs(per, seed):
    streams = len(per)
    hws = [((480, 640), (360, 480), (640, 480))[s % 3] for s in range(streams)]   # two landscape shapes and a portrait one
    return refs.synthetic_rows(streams, per, seed), hws


def _host_and_device_tail(rows, streams, hws, iou=0.3):
    from millieye_amd.demo import MultiStreamFuser
    d_rows = torch.from_numpy(rows).cuda()
    out = []
    for tail in ("host", "device"):
        fuser = MultiStreamFuser(None, RADAR_CALIB, streams, nms_iou=iou, tail=tail)
        out.append(fuser._tail(d_rows.clone(), hws))
    return out


def test_stream_tail_against_the_restatement_and_the_host_path(hip_lib):
    from oracle import tv_ops
    per = [37, 0, 65, 12, 300, 1]
    rows, hws = _tail_inputs(per, seed=61)
    assert not np.all(np.diff(rows[:, 0]) >= 0), "interleaved stream order"

    def oracle_nms(b, s, lab, iou):
        return tv_ops.batched_nms(torch.from_numpy(b.copy()), torch.from_numpy(s.copy()), torch.from_numpy(lab.copy()), iou).numpy()

    want = refs.tail_ref(rows, len(per), hws, 416, 0.3, nms=oracle_nms)
    host, dev = _host_and_device_tail(rows, len(per), hws)
    kept_total = 0
    for s in range(len(per)):
        assert dev[s].dtype == torch.float32 and tuple(dev[s].shape) == want[s].shape == tuple(host[s].shape), f"stream {s}"
        assert torch.equal(dev[s], host[s]), f"stream {s}: device tail differs from the host path"
        assert np.array_equal(dev[s].numpy().view(np.uint32), want[s].view(np.uint32)), f"stream {s}: differs from the restatement"
        kept_total += len(want[s])
    assert tuple(dev[1].shape) == (0, 7) and 0 < kept_total < sum(per)
    # in_counts, and the portrait stream really was rescaled with a left / right pad
    from millieye_amd import hip
    from millieye_amd.utils.utils import rescale_scalars
    _per_stream, in_counts = hip.stream_tail(torch.from_numpy(rows).cuda(), len(per), rescale_scalars(416, hws).cuda(), 0.3)
    assert in_counts == per
    assert float(rescale_scalars(416, hws)[2, 0]) > 0 and float(rescale_scalars(416, hws)[0, 3]) > 0
    # no rows at all
    host, dev = _host_and_device_tail(np.zeros((0, 8), np.float32), 3, hws[:3])
    assert all(tuple(d.shape) == tuple(h.shape) == (0, 7) for d, h in zip(dev, host))


def test_stream_tail_refuses_a_bad_stream_column_without_writing_out_of_range(hip_lib):
    from millieye_amd import hip
    from millieye_amd.utils.utils import rescale_scalars
    per = [20, 30, 10]
    rows, hws = _tail_inputs(per, seed=62)
    scal = rescale_scalars(416, hws).cuda()
    for bad in (3.0, -1.0, 1.5, np.nan, 1.0e9):
        r = rows.copy()
        r[25, 0] = bad
        with pytest.raises(hip.MeError, match="stream column"):
            hip.stream_tail(torch.from_numpy(r).cuda(), 3, scal, 0.3)
    m, streams, pad = len(rows), 3, 64
    r = rows.copy()
    r[25, 0], r[41, 0] = 7.0, -2.0
    d_rows = torch.from_numpy(r).cuda()
    nbytes = int(hip.lib().me_stream_tail_out_bytes(streams, m))
    assert nbytes % 4 == 0
    out = torch.full((pad + nbytes // 4 + pad,), GUARD, dtype=torch.int32, device="cuda")
    assert (out.data_ptr() + 4 * pad) % 16 == 0
    ws_bytes = int(hip.lib().me_nms_workspace_bytes(streams, m))
    ws = torch.full((ws_bytes // 4 + 64 + pad,), GUARD, dtype=torch.int32, device="cuda")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    ws_off = (ws_ptr - ws.data_ptr()) // 4
    hip.check(hip.lib().me_stream_tail_f32(d_rows.data_ptr(), m, streams, scal.data_ptr(), 0.3, out[pad:].data_ptr(), ws_ptr,
                                           hip.stream_ptr()), "me_stream_tail_f32")
    torch.cuda.synchronize()
    out_h, ws_h = out.cpu(), ws.cpu()
    assert bool((out_h[:pad] == GUARD).all()) and bool((out_h[pad + nbytes // 4:] == GUARD).all())
    assert bool((ws_h[:ws_off] == GUARD).all()) and bool((ws_h[ws_off + ws_bytes // 4:] == GUARD).all())
    assert int(out_h[pad]) == 1, "status"
    assert sum(out_h[pad + 1:pad + 1 + streams].tolist()) == m - 2, "the two bad rows are left out"
    assert torch.equal(d_rows.cpu(), torch.from_numpy(r)), "the input rows are read only"


def _net():
    from millieye_amd import synth
    from millieye_amd.my_models import Network, define_yolo
    from tests import parity_helpers as ph
    net = Network(define_yolo(ph.cfg_path("yolov3-tiny-12")), 0.1).eval()
    synth.fill_network_(net, "demo", cls0_bias=3.0, cls_bias=-4.0)
    return net.to(net.device)


def _same_step(got, want, what):
    assert len(got) == len(want)
    for s, ((rows, info), (rows_w, info_w)) in enumerate(zip(got, want)):
        assert rows.dtype == rows_w.dtype and tuple(rows.shape) == tuple(rows_w.shape) and torch.equal(rows, rows_w), \
            f"{what} stream {s}: rows differ"
        for key in ("mode", "points", "radar_boxes"):
            assert info[key] == info_w[key], f"{what} stream {s}: {key}"
        assert np.array_equal(info["proposals"], info_w["proposals"])


def test_the_device_tail_is_the_default():
    from millieye_amd.demo import MultiStreamFuser
    assert MultiStreamFuser(None, RADAR_CALIB, 2).tail == "device"


def test_fuser_device_tail_equals_host_tail(hip_lib):
    from millieye_amd.demo import MultiStreamFuser
    net = _net()
    n = 6
    frames = [mh.stream_frame(s) for s in range(n)]
    assert len({f.shape for f in frames}) == 2
    fusers = {tail: MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS, tail=tail) for tail in ("host", "device")}
    rows_total = 0
    for f in range(6):
        radar = [mh.stream_radar(s, f) for s in range(n)]
        want = fusers["host"](frames, radar)
        got = fusers["device"](frames, radar)
        modes = [info["mode"] for _r, info in got]
        assert 0 in modes and 1 in modes, "both sub-batches must be non-empty"
        _same_step(got, want, f"step {f}")
        rows_total += sum(len(r) for r, _i in got)
    assert rows_total > 0
    # bright frames of the tiny synthetic net: streams without rows return [0,7]
    empty = [tuple(r.shape) for r, _i in got if len(r) == 0]
    assert all(shape == (0, 7) for shape in empty)


def _track_states(fuser):
    out = []
    for s in range(fuser.streams):
        state, frame_count = fuser.generator.track_state(s)
        out.append((frame_count, [(t["x"].copy(), t["P"].copy(), t["time_since_update"], t["hit_streak"]) for t in state]))
    return out


def _same_states(a, b):
    assert len(a) == len(b)
    for s, ((fc_a, tr_a), (fc_b, tr_b)) in enumerate(zip(a, b)):
        assert fc_a == fc_b and len(tr_a) == len(tr_b), f"stream {s}: {fc_a} / {len(tr_a)} vs {fc_b} / {len(tr_b)}"
        for ta, tb in zip(tr_a, tr_b):
            assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1]) and ta[2:] == tb[2:], f"stream {s}"


N_STREAMS, STEPS = 4, 8
_shared = {}


def _in_process_run():
    """The reference of the pipeline tests, computed once: the net, the source, every step of the in-process fuser and its
    final tracks."""
    if not _shared:
        from millieye_amd.demo import MultiStreamFuser
        from tests.multistream_pipeline_helpers import StreamSource
        net = _net()
        source = StreamSource(STEPS, N_STREAMS, real=True)
        local = MultiStreamFuser(net, RADAR_CALIB, N_STREAMS, model_mode=3, min_hits=mh.MIN_HITS, tail="host")
        want = [local(*source.step(f)) for f in range(STEPS)]
        _shared.update(net=net, source=source, want=want, states=_track_states(local))
    return _shared["net"], _shared["source"], _shared["want"], _shared["states"]


def test_pipeline_for_streams_equals_the_in_process_fuser(hip_lib):
    from millieye_amd.demo import MultiStreamFuser
    from millieye_amd.pipeline import FusionPipeline
    net, source, want, states = _in_process_run()
    fuser = MultiStreamFuser(net, RADAR_CALIB, N_STREAMS, model_mode=3, min_hits=mh.MIN_HITS, tail="device")
    pipe = FusionPipeline(fuser, source, skip_to_newest=False)
    got = list(pipe)
    assert [info["frame_idx"] for _r, info in got] == list(range(STEPS)) and pipe.stats["dropped"] == 0
    for f, (results, _info) in enumerate(got):
        _same_step(results, want[f], f"step {f}")
    assert sum(len(r) for r, _i in got[-1][0]) > 0
    _same_states(_track_states(fuser), states)


def test_advance_keeps_the_trackers_of_skipped_steps(hip_lib):
    """advance() in place of infer() on some steps: the inferred steps and the final tracks are those of the full run."""
    from millieye_amd.demo import MultiStreamFuser
    net, source, want, states = _in_process_run()
    skipping = MultiStreamFuser(net, RADAR_CALIB, N_STREAMS, model_mode=3, min_hits=mh.MIN_HITS, tail="device")
    for f in range(STEPS):
        payload = skipping.prepare(*source.step(f), pack=f % 2 == 0)
        if f in (1, 2, 4, 6):
            skipping.advance(payload)
        else:
            _same_step(skipping.infer(payload), want[f], f"advance on other steps, step {f}")
    _same_states(_track_states(skipping), states)


def test_pipeline_with_a_slowed_consumer(hip_lib):
    """The consumer skips to the newest step; the skipped ones still reach the trackers."""
    from millieye_amd.demo import MultiStreamFuser
    from millieye_amd.pipeline import FusionPipeline
    from tests.multistream_pipeline_helpers import StreamSource, progress_counter, wait_for_backlog
    net, _source, want, states = _in_process_run()
    slow = MultiStreamFuser(net, RADAR_CALIB, N_STREAMS, model_mode=3, min_hits=mh.MIN_HITS, tail="device")
    progress = progress_counter()

    def slow_infer(payload):
        wait_for_backlog(progress, payload["frame_idx"])   # until the producer has queued the next two steps
        return slow.infer(payload)

    pipe = FusionPipeline(slow, StreamSource(STEPS, N_STREAMS, real=True, progress=progress), infer=slow_infer)
    seen = []
    for results, info in pipe:
        seen.append(info["frame_idx"])
        _same_step(results, want[info["frame_idx"]], f"slow consumer, step {info['frame_idx']}")
    assert seen[0] == 0 and seen[-1] == STEPS - 1 and all(a < b for a, b in zip(seen, seen[1:]))
    assert pipe.stats["dropped"] == STEPS - len(seen) > 0, "with two more steps queued after every inference, steps are skipped"
    print(f"slow consumer: inferred steps {seen}, {pipe.stats['dropped']} only advanced")
    _same_states(_track_states(slow), states)
