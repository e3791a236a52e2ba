"""-m gpu: the multi-stream front (csrc/radar.hip: me_radar_proposals_f64, me_frame_means_f32;
radar_proposals.DeviceRadarProposals, demo.MultiStreamFuser) against the host code it restates: one host
``RadarProposalGenerator`` / ``FrameFuser`` per stream.  tests/test_radar_device_fixture_cpu.py guards the inputs.

Bar of the float64 comparisons (Kalman state ``x`` / ``P``, pixel proposals), measured, not guessed: the host tracker run
over the same streams twice - as committed (gain through ``np.linalg.inv``) and with the gain from ``np.linalg.solve`` -
deviates by at most 8.327e-17 (``|a - b| / max(1, |b|)``, tests.multistream_helpers.kalman_deviation; numpy 2.2.6 with
its bundled OpenBLAS); the bar is 16 x that = 1.332e-15.  The test recomputes both figures on the machine it runs on.

Measured on an MI355X over all 8 streams x 10 frames (x, P of every live track and the pixel proposals): the largest
deviation of the device from the host is 1.678e-16.  The gain is formed the way the host forms it - the explicit inverse of S,
then the product (P H') S^-1: a gain solved for directly rounds the rows of the unobserved velocities, sums of large cancelling
terms, differently (measured: up to 2.1e-15 on a lateral-velocity element, outside the bar)."""
import numpy as np
import pytest
import torch

from millieye_amd import radar_proposals as rp, synth
from tests import multistream_helpers as mh
from tests.golden.make_golden import RADAR_CALIB

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_stream(dev, res, s, h, bar, what, worst, frame_hw=None):
    """Stream ``s`` of the device step ``res`` against the host record ``h`` of the same frame."""
    from millieye_amd.demo import radar_boxes_for_network
    counts = res.host_counts[s]
    # kept points, uv, cloud: exact
    cloud = dev.cloud(s)
    assert counts[1] == len(h["cloud"]), f"{what}: kept points {counts[1]} vs {len(h['cloud'])}"
    assert np.array_equal(cloud, h["cloud"]), f"{what}: cloud (uv, range, velocity) differs"
    # DBSCAN membership, fresh clusters
    assert np.array_equal(dev.labels(s), h["labels"]), f"{what}: DBSCAN labels differ"
    fresh = dev.clusters(s)
    assert len(fresh) == len(h["fresh"]) and np.array_equal(fresh["num_points"], h["fresh"]["num_points"]), f"{what}: clusters"
    for field in ("center", "size", "avgV"):
        assert np.array_equal(_bits(fresh[field]), _bits(h["fresh"][field])), \
            f"{what}: fresh cluster {field} differs in bits: {fresh[field]} vs {h['fresh'][field]}"
    # the assignment
    assert np.array_equal(dev.matches(s, h["tracks_before"]), h["matches"]), f"{what}: assignment differs"
    # tracks: life-cycle counters exact, Kalman state within the measured bar
    state, frame_count = dev.track_state(s)
    assert frame_count == h["frame_count"] and len(state) == len(h["state"]), f"{what}: {len(state)} tracks vs {len(h['state'])}"
    for k, (t, th) in enumerate(zip(state, h["state"])):
        for key in ("time_since_update", "hit_streak", "prev_hit_streak"):
            assert t[key] == th[key], f"{what}: track {k} {key} {t[key]} vs {th[key]}"
        assert t["cluster"]["num_points"] == th["cluster"]["num_points"]
        for key in ("x", "P"):
            dev_ = mh.rel_dev(t[key], th[key])
            worst[0] = max(worst[0], dev_)
            print(f"{what}: track {k} {key} deviation {dev_:.3e} (bar {bar:.3e})")
            assert dev_ <= bar, f"{what}: track {k} {key} deviates by {dev_:.3e} > {bar:.3e}"
    # tracked clusters: number and order; float32 fields are roundings of float64 values inside the bar
    tracked = dev.tracked(s)
    assert len(tracked) == len(h["tracked"]) and np.array_equal(tracked["num_points"], h["tracked"]["num_points"]), \
        f"{what}: tracked clusters"
    for field in ("center", "size", "avgV"):
        assert np.allclose(tracked[field], h["tracked"][field], rtol=2.0 ** -22, atol=1e-30), f"{what}: tracked {field}"
    # pixel proposals, network boxes
    prop = dev.proposals(s)
    assert prop.shape == h["proposals"].shape, f"{what}: {prop.shape} proposals vs {h['proposals'].shape}"
    dev_ = mh.rel_dev(prop, h["proposals"])
    worst[0] = max(worst[0], dev_)
    print(f"{what}: proposals deviation {dev_:.3e} (bar {bar:.3e})")
    assert dev_ <= bar, f"{what}: proposals deviate by {dev_:.3e} > {bar:.3e}"
    want = radar_boxes_for_network(h["proposals"], frame_hw or (dev.image_size[s][1], dev.image_size[s][0]))
    rows = res.radar_box[res.radar_box[:, 0] == s].cpu()
    assert counts[4] == len(want) == len(rows), f"{what}: radar boxes {counts[4]} vs {len(want)}"
    assert torch.allclose(rows[:, 1:], want[:, 1:], rtol=2.0 ** -22, atol=1e-30), f"{what}: network boxes differ"


def test_chain_vs_host_generator(hip_lib):
    bar_dev = mh.kalman_deviation()
    bar = 16.0 * bar_dev
    print(f"host tracker inv vs solve: deviation {bar_dev:.3e}, bar {bar:.3e}")
    assert bar > 0.0
    dev = rp.DeviceRadarProposals(RADAR_CALIB, mh.STREAMS, min_hits=mh.MIN_HITS)
    hosts = [mh.HostStream() for _ in range(mh.STREAMS)]
    worst = [0.0]
    seen = dict(matched=0, tracked=0, boxes=0)
    # camera frames the boxes are padded / normalised for: landscape, portrait (pads left / right) and square
    hw = [((480, 640), (640, 480), (360, 480), (800, 600), (512, 512))[s % 5] for s in range(mh.STREAMS)]
    for f in range(mh.FRAMES):
        res = dev.gen([mh.stream_radar(s, f) for s in range(mh.STREAMS)], hw)
        assert res.radar_box.shape == (int(res.host_counts[:, 4].sum()), 5)
        assert torch.equal(res.radar_box[:, 0].cpu(), torch.repeat_interleave(
            torch.arange(mh.STREAMS, dtype=torch.float32), torch.as_tensor(res.host_counts[:, 4].astype(np.int64)))), "stream-major"
        for s in range(mh.STREAMS):
            h = hosts[s].step(mh.stream_radar(s, f))
            _check_stream(dev, res, s, h, bar, f"frame {f} stream {s}", worst, hw[s])
            seen["matched"] += int((h["matches"] >= 0).sum())
            seen["tracked"] += len(h["tracked"])
            seen["boxes"] += int(res.host_counts[s, 4])
    print(f"largest float64 deviation device vs host: {worst[0]:.3e} (bar {bar:.3e}); {seen}")
    assert seen["matched"] > 50 and seen["tracked"] > 50 and seen["boxes"] > 50


def test_cloud_and_heatmap(hip_lib):
    from millieye_amd.utils.datasets import StagedRadarMaps
    dev = rp.DeviceRadarProposals(RADAR_CALIB, mh.STREAMS, min_hits=mh.MIN_HITS)
    hosts = [mh.HostStream() for _ in range(mh.STREAMS)]
    hw = [mh.FRAME_SIZES[s % 2] for s in range(mh.STREAMS)]
    for f in range(3):
        res = dev.gen([mh.stream_radar(s, f) for s in range(mh.STREAMS)], hw)
        clouds = [hosts[s].step(mh.stream_radar(s, f))["cloud"] for s in range(mh.STREAMS)]
        packed = res.cloud[:int(res.host_counts[:, 1].sum())].cpu().numpy()
        assert np.array_equal(packed, np.concatenate(clouds, 0)), "packed device cloud differs from the host clouds"
        assert np.array_equal(res.cloud_offsets.cpu().numpy(), np.concatenate([[0], np.cumsum([len(c) for c in clouds])]))
        got = dev.heatmaps(32)
        want = StagedRadarMaps(clouds, [(w, h) for h, w in hw], map_size=32).to(got.device)
        assert got.shape == (mh.STREAMS, 3, 32, 32) and torch.equal(got, want), "radar maps differ"
        assert float(got.abs().sum()) > 0


@pytest.mark.parametrize("shape", [(8, 3, 416, 416), (3, 3, 97, 61), (1, 5)])
def test_frame_means(hip_lib, shape):
    from millieye_amd import hip
    x = torch.from_numpy(synth.uniform(f"multistream/means{shape}", shape)).cuda()
    if len(shape) == 4:
        x[0] *= 0.1
    got = hip.frame_means(x).cpu()
    for f in range(shape[0]):
        want = float(x[f].mean())
        print(f"frame {f}: {float(got[f])!r} vs {want!r}")
        assert abs(float(got[f]) - want) <= 1e-6
        assert abs(float(got[f]) - float(x[f].double().mean())) <= 1e-6


def _net():
    from tests.test_gpu_network import _build
    net = _build("demo", "yolov3-tiny-12", 0.1).eval()
    synth.fill_network_(net, "demo", cls0_bias=3.0, cls_bias=-4.0)
    return net.to(net.device)


def _cmp_step(got, want, frames, what):
    from tests.test_gpu_network import _cmp_rows_ties
    assert len(got) == len(want)
    for s, ((rows, info), (rows_w, info_w)) in enumerate(zip(got, want)):
        for key in ("mode", "points", "radar_boxes"):
            assert info[key] == info_w[key], f"{what} stream {s}: {key} {info[key]} vs {info_w[key]}"
        assert info["proposals"].shape == info_w["proposals"].shape
        hw = frames[s].shape[:2]
        _cmp_rows_ties(mh.rows8(rows, hw), mh.rows8(rows_w, hw), f"{what} stream {s}")


def test_fuser_equivalence(hip_lib):
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    net = _net()
    n = 6
    frames = [mh.stream_frame(s) for s in range(n)]
    assert len({f.shape for f in frames}) == 2
    singles = [FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=mh.MIN_HITS) for _ in range(n)]
    multi = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS)
    rows_total = boxes_total = 0
    for f in range(6):
        radar = [mh.stream_radar(s, f) for s in range(n)]
        want = [singles[s](frames[s], radar[s]) for s in range(n)]
        got = multi(frames, radar)
        modes = [info["mode"] for _r, info in got]
        assert 0 in modes and 1 in modes, "both sub-batches must be non-empty"
        _cmp_step(got, want, frames, f"step {f}")
        rows_total += sum(len(r) for r, _i in got)
        boxes_total += sum(i["radar_boxes"] for _r, i in got if i["mode"] == 0)
    assert rows_total > 0 and boxes_total > 0
    # all frames bright: no fusion sub-batch
    bright = [mh.stream_frame(s, dark=False) for s in range(n)]
    radar = [mh.stream_radar(s, 6) for s in range(n)]
    want = [singles[s](bright[s], radar[s]) for s in range(n)]
    got = multi(bright, radar)
    assert all(info["mode"] == 1 for _r, info in got)
    _cmp_step(got, want, bright, "all bright")
    # one stream
    single, one = FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=mh.MIN_HITS), \
        MultiStreamFuser(net, RADAR_CALIB, 1, model_mode=3, min_hits=mh.MIN_HITS)
    for f in range(3):
        _cmp_step(one([frames[1]], [mh.stream_radar(1, f)]), [single(frames[1], mh.stream_radar(1, f))], [frames[1]], f"S=1 step {f}")
    # fixed modes need no means and no split
    fixed = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=0, min_hits=mh.MIN_HITS)
    assert all(info["mode"] == 0 for _r, info in fixed(frames, radar))


def test_state_handling(hip_lib):
    from millieye_amd import hip
    n = 4
    dev = rp.DeviceRadarProposals(RADAR_CALIB, n, min_hits=mh.MIN_HITS)
    hosts = [mh.HostStream() for _ in range(n)]
    bar = mh.kalman_bar()
    worst = [0.0]

    def step(frames_of):
        res = dev.gen([frames_of(s) for s in range(n)])
        for s in range(n):
            _check_stream(dev, res, s, hosts[s].step(frames_of(s)), bar, f"stream {s}", worst)
        return res

    first = []
    for f in range(4):
        step(lambda s: mh.stream_radar(s, f))
        first.append((dev.tracked(1).copy(), dev.proposals(1).copy(), dev.track_state(1)))
    # reset(stream): that stream replays its first frames identically, the others continue
    dev.reset(1)
    hosts[1] = mh.HostStream()
    for f in range(4):
        step(lambda s: mh.stream_radar(s, f if s == 1 else f + 4))
        tracked, prop, (state, frame_count) = first[f]
        assert np.array_equal(dev.tracked(1).view(np.uint8), tracked.view(np.uint8)) and np.array_equal(dev.proposals(1), prop)
        state_now, frame_count_now = dev.track_state(1)
        assert frame_count_now == frame_count == f + 1 and len(state_now) == len(state)
        for a, b in zip(state_now, state):
            assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["P"], b["P"])
    # a stream over the point capacity: MeError names it, its state is untouched, the next normal step matches the host
    flood = [np.tile(mh.stream_radar(2, 8)[0], (1, 12))]
    kept = len(mh.HostStream().step(flood)["cloud"])
    assert kept > hip.RADAR_MAX_POINTS
    before = dev.track_state(2)
    with pytest.raises(hip.MeError, match=r"stream 2 .*256"):
        dev.gen([flood if s == 2 else mh.stream_radar(s, 8) for s in range(n)])
    after = dev.track_state(2)
    assert after[1] == before[1] and len(after[0]) == len(before[0])
    for a, b in zip(after[0], before[0]):
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["P"], b["P"]) and a["time_since_update"] == b["time_since_update"]
    for s in range(n):
        if s != 2:
            hosts[s].step(mh.stream_radar(s, 8))   # the other streams have advanced
    step(lambda s: mh.stream_radar(s, 8 if s == 2 else 9))
    dev.reset()
    assert all(dev.track_state(s) == ([], 0) for s in range(n))


def test_repeatability(hip_lib):
    from millieye_amd.demo import MultiStreamFuser
    net = _net()
    n = 6
    frames = [mh.stream_frame(s) for s in range(n)]
    runs = []
    for _ in range(2):
        fuser = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=mh.MIN_HITS)
        runs.append([fuser(frames, [mh.stream_radar(s, f) for s in range(n)]) for f in range(4)])
    for step_a, step_b in zip(*runs):
        for (rows_a, info_a), (rows_b, info_b) in zip(step_a, step_b):
            assert torch.equal(rows_a, rows_b) and info_a["mode"] == info_b["mode"]
            assert np.array_equal(info_a["proposals"], info_b["proposals"])
    assert sum(len(r) for r, _i in runs[0][-1]) > 0
