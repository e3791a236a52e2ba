"""-m gpu: the device radar proposal chain (csrc/radar.hip: radar_chain_kernel, radar_pack_kernel) at its capacities and
edges - 256 kept points, 32 clusters, 32 tracks per stream, chains of 256 points, assignments of 32 x 28, tracks dying out of
the middle of the list, the refused cases and their statuses, 300 streams - against one host ``RadarProposalGenerator`` per
stream, compared as ``tests.test_gpu_multistream._check_stream`` compares: cloud, labels, fresh clusters and matches bit for
bit, counters exactly, the Kalman state and the pixel proposals under a measured float64 bar, float32 records at 2^-22.
tests/radar_scene_helpers.py builds the scenes; tests/test_radar_scenes_cpu.py guards them.

The float64 bar, per scene family (radar_scene_helpers.grid_runs says which family takes which): the host tracker run on the
family's scenes twice - gain through ``np.linalg.inv`` as committed, and solved for - and 16 x the largest deviation
(``|a - b| / max(1, |b|)``) of ``x``, ``P`` and the proposals between the two.  Recomputed on the machine the test runs on; never
derived from the device's output.  Both figures and the device's own worst deviation per family go to
profiles/radar_chain_errors.txt.

Measured on an MI355X (numpy 2.2.6 with its bundled OpenBLAS): capacity grid - host inv vs solve 5.551e-17, bar 8.882e-16,
device 1.110e-16; many streams - 1.110e-16, 1.776e-15, device 2.131e-16; the single-frame families deviate by 0.  The file takes
about 7 s."""
import copy
import functools
import os
import types

import numpy as np
import pytest
import torch

from millieye_amd import radar_proposals as rp
from tests import multistream_helpers as mh, radar_scene_helpers as sh
from tests.golden.make_golden import RADAR_CALIB
from tests.test_gpu_multistream import _bits, _check_stream

pytestmark = pytest.mark.gpu

ERRORS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "radar_chain_errors.txt")
_LOG = {}
MARK_I, MARK_F = 0x5EA7BEEF, -98765.4321


@functools.lru_cache(maxsize=None)
def _grid():
    """Host records of the grid and the boxes streams and the family's deviation: computed once, shared, left unchanged."""
    return sh.grid_runs()


def _grid_bar():
    return 16.0 * _grid()[2]


def _record(family, host_dev, bar, worst):
    line = f"host inv vs solve {host_dev:.3e}  bar {bar:.3e}  device worst {worst:.3e}"
    print(f"{family}: {line}")
    _LOG[family] = line
    assert bar > 0.0 and worst <= bar


@pytest.fixture(scope="module", autouse=True)
def _write_errors_file():
    """Lines of profiles/radar_chain_errors.txt are replaced by the tests that ran; the others stay."""
    yield
    if not _LOG:
        return
    lines = {}
    if os.path.exists(ERRORS_FILE):
        for line in open(ERRORS_FILE).read().splitlines():
            if line.strip() and not line.startswith("#") and ":" in line:
                lines[line.split(":", 1)[0].strip()] = line.split(":", 1)[1].strip()
    lines.update(_LOG)
    head = ("# Measured by tests/test_gpu_radar_chain.py on an MI355X, per scene family: the largest deviation |a - b| / max(1, |b|)\n"
            "# of the Kalman state x / P and of the pixel proposals between the host tracker's two roundings (gain through\n"
            "# np.linalg.inv / solved for), the bar = 16 x that figure, and the device chain's largest deviation from the host.\n")
    try:
        with open(ERRORS_FILE, "w") as f:
            f.write(head)
            for name in sorted(lines):
                f.write(f"{name + ':':<24s}{lines[name]}\n")
    except OSError:
        pass


def _device(streams, **kw):
    kw.setdefault("min_hits", sh.MIN_HITS)
    return rp.DeviceRadarProposals(RADAR_CALIB, streams, **kw)


def _last_result(dev):
    """What ``gen`` would have returned, after a step that raised for one stream: both launches have run."""
    total = int(dev.host_counts[:, 4].sum())
    return types.SimpleNamespace(host_counts=dev.host_counts, radar_box=dev._boxes[:total].clone())


def _state_bytes(dev, s):
    per = dev._state.numel() // dev.streams
    return dev._state[s * per:(s + 1) * per].cpu().numpy().copy()


def _check_packed(dev, res, records, hw):
    """The pack kernel's outputs against the host records of all streams: boxes stream-major, cloud, offsets, totals."""
    from millieye_amd.demo import radar_boxes_for_network
    counts = res.host_counts
    want_rows = []
    for s, h in enumerate(records):
        rows = radar_boxes_for_network(h["proposals"], hw[s])
        rows[:, 0] = s
        want_rows.append(rows)
    want_rows = torch.cat(want_rows, 0)
    got_rows = res.radar_box.cpu()
    assert got_rows.shape == want_rows.shape, f"{got_rows.shape} packed boxes vs {want_rows.shape}"
    assert torch.equal(got_rows[:, 0], want_rows[:, 0]), "packed boxes are not stream-major"
    assert torch.allclose(got_rows[:, 1:], want_rows[:, 1:], rtol=2.0 ** -22, atol=1e-30)
    clouds = [h["cloud"] for h in records]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    assert np.array_equal(res.cloud_offsets.cpu().numpy(), offsets), "cloud offsets"
    assert np.array_equal(res.cloud[:offsets[-1]].cpu().numpy(), np.concatenate(clouds, 0)), "packed cloud"
    assert dev._totals.cpu().tolist() == [len(want_rows), int(offsets[-1])], "totals"
    assert np.array_equal(counts[:, 4], [int((want_rows[:, 0] == s).sum()) for s in range(len(records))])
    return clouds


def _check_heatmaps(dev, clouds, hw):
    from millieye_amd.utils.datasets import StagedRadarMaps
    got = dev.heatmaps(32)
    want = StagedRadarMaps(clouds, [(w, h) for h, w in hw], map_size=32).to(got.device)
    assert got.shape == (len(clouds), 3, 32, 32) and torch.equal(got, want), "radar maps differ"
    assert float(got.abs().sum()) > 0


# --------------------------------------------------------------------------------------------------------- capacity grid
def test_capacity_grid(hip_lib):
    """12 frames at 256 points / 32 clusters / 32 tracks; in streams 1 and 2 four tracks coast and die together out of the middle
    and the end of the list (32 x 28 assignments, in-place compaction), then a reflector returns (28 x 29, a track appended)."""
    records, _boxes, host_dev = _grid()
    bar = 16.0 * host_dev
    n = sh.GRID_STREAMS
    dev = _device(n)
    hw = [(480, 640), (640, 480), (512, 512)]
    worst, deaths, shapes = [0.0], [0] * n, set()
    for f in range(sh.GRID_FRAMES):
        res = dev.gen([sh.grid_radar(s, f) for s in range(n)], hw)
        for s in range(n):
            h = records[f][s]
            _check_stream(dev, res, s, h, bar, f"grid frame {f} stream {s}", worst, hw[s])
            deaths[s] += h["tracks_peak"] - int(res.host_counts[s, 5])
            shapes.add((h["tracks_before"], int(res.host_counts[s, 2])))
        assert tuple(res.host_counts[0, [1, 2, 3, 5, 7]]) == (256, 32, 32, 32, 32), "stream 0 runs at every capacity"
        _check_packed(dev, res, records[f], hw)
    assert deaths == [0, 4, 4], f"deaths {deaths}"
    assert (32, 28) in shapes and (28, 29) in shapes and (32, 32) in shapes
    # the track order after deaths, compaction and the appended track is the host's: every device track is nearest its namesake
    for s in range(n):
        state, _ = dev.track_state(s)
        want = np.array([t["x"] for t in records[-1][s]["state"]])
        got = np.array([t["x"] for t in state])
        nearest = np.abs(got[:, None, :3] - want[None, :, :3]).sum(-1).argmin(1)
        assert np.array_equal(nearest, np.arange(len(want))), f"stream {s}: track order {nearest}"
    _record("capacity grid", host_dev, bar, worst[0])


def test_capacity_grid_heatmaps(hip_lib):
    records, _boxes, _dev = _grid()
    n = sh.GRID_STREAMS
    dev = _device(n)
    hw = [(480, 640), (360, 480), (480, 640)]
    for f in range(2):
        res = dev.gen([sh.grid_radar(s, f) for s in range(n)], hw)
        assert int(res.host_counts[0, 1]) == 256
        clouds = [records[f][s]["cloud"] for s in range(n)]
        assert np.array_equal(res.cloud[:sum(len(c) for c in clouds)].cpu().numpy(), np.concatenate(clouds, 0))
        _check_heatmaps(dev, clouds, hw)


# ---------------------------------------------------------------------------------------------------------------- chains
def test_chains(hip_lib):
    """One component of 256 points whose label has to travel the whole chain - in index order, reversed, shuffled - and two
    interleaved chains of 128."""
    bar = _grid_bar()
    n = len(sh.CHAIN_ORDERS)
    dev = _device(n)
    hosts = [mh.HostStream() for _ in range(n)]
    res = dev.gen([sh.chain_radar(s) for s in range(n)])
    worst = [0.0]
    for s, order in enumerate(sh.CHAIN_ORDERS):
        h = hosts[s].step(sh.chain_radar(s))
        _check_stream(dev, res, s, h, bar, f"chain {order}", worst)
        labels, fresh = dev.labels(s), dev.clusters(s)
        two = order == "interleaved"
        assert np.array_equal(labels, np.arange(256) % 2 if two else np.zeros(256, np.int32)), f"chain {order}: labels"
        assert list(fresh["num_points"]) == ([128, 128] if two else [256])
        assert np.array_equal(_bits(fresh["center"]), _bits(h["fresh"]["center"]))
        assert np.array_equal(_bits(fresh["size"]), _bits(h["fresh"]["size"])) and (fresh["size"] > 0).all()
        assert tuple(res.host_counts[s, :4]) == (0, 256, 2 if two else 1, 2 if two else 1)
    _record("chains", _grid()[2], bar, worst[0])


# --------------------------------------------------------------------------------------------------------- mean velocity
def test_mean_velocity(hip_lib):
    """``avgV`` = float32(np.mean) of cancelling velocities: numpy's pairwise order of additions, at every kept-point count
    around its 128-element blocks."""
    bar = _grid_bar()
    n = len(sh.MEANV_SIZES)
    dev = _device(n, **sh.MEANV_KW)
    hosts = [mh.HostStream(**sh.MEANV_KW) for _ in range(n)]
    res = dev.gen([sh.meanv_radar(s) for s in range(n)])
    worst = [0.0]
    for s, size in enumerate(sh.MEANV_SIZES):
        h = hosts[s].step(sh.meanv_radar(s))
        got, want = dev.clusters(s)["avgV"], h["fresh"]["avgV"]
        print(f"n = {size}: avgV {got} vs {want}; other orders {sh.mean_variants(h['xyzv'][:, 3])}")
        assert int(res.host_counts[s, 1]) == size and len(got) == 1
        assert np.array_equal(_bits(got), _bits(want)), f"n = {size}: avgV {got[0]!r} vs numpy's {want[0]!r}"
        _check_stream(dev, res, s, h, bar, f"mean velocity n = {size}", worst)
    _record("mean velocity", _grid()[2], bar, worst[0])


# ----------------------------------------------------------------------------------------------------------- filter edge
def test_filter_edge(hip_lib):
    """Components one point under and exactly at ``num_pts_filter`` alternate: 32 pass, in order, beside 20 that fail."""
    bar = _grid_bar()
    dev = _device(1)
    h = mh.HostStream().step([sh.edge_frame()])
    res = dev.gen([[sh.edge_frame()]])
    worst = [0.0]
    _check_stream(dev, res, 0, h, bar, "filter edge", worst)
    assert int(dev.labels(0).max()) + 1 == sh.EDGE_PASS + sh.EDGE_FAIL
    assert tuple(res.host_counts[0, :4]) == (0, 240, 32, 32) and (dev.clusters(0)["num_points"] == 5).all()
    _record("filter edge", _grid()[2], bar, worst[0])


# -------------------------------------------------------------------------------------------------------------- statuses
def _bad_points(f):
    return [sh.grid_frame(f, extra_point=True)]


def _bad_clusters(f):
    return [sh.grid_frame(f, points=7, extra_cluster=True)]


def _bad_pairs(f):
    return [sh.pairs_frame()]


@pytest.mark.parametrize("bad_frame,status,pattern,kw", [
    (_bad_points, 1, r"stream 1 .*256 points", {}), (_bad_clusters, 2, r"stream 1 .*32 clusters", {}),
    (_bad_pairs, 2, r"stream 1 .*32 clusters", dict(num_pts_filter=2))], ids=["257-points", "33-clusters", "128-pairs"])
def test_capacity_statuses(hip_lib, bad_frame, status, pattern, kw):
    """A stream over a capacity: ``MeError`` names it, its state is untouched to the byte, the other streams have advanced, and
    its next normal frame continues as if the refused one had not been."""
    from millieye_amd import hip
    bar = _grid_bar()
    n = 3
    dev = _device(n, **kw)
    hosts = [mh.HostStream(**kw) for _ in range(n)]
    worst = [0.0]

    def step(frame_of, streams=range(n), res=None):
        res = res or dev.gen([sh.grid_radar(s, frame_of(s)) for s in range(n)])
        for s in streams:
            _check_stream(dev, res, s, hosts[s].step(sh.grid_radar(s, frame_of(s))), bar, f"stream {s} frame {frame_of(s)}", worst)
        return res

    for f in range(2):
        res = step(lambda s: f)
    assert int(res.host_counts[0, 1]) == 256, "exactly 256 kept points are accepted"
    before = _state_bytes(dev, 1)
    assert before.any()
    with pytest.raises(hip.MeError, match=pattern):
        dev.gen([bad_frame(2) if s == 1 else sh.grid_radar(s, 2) for s in range(n)])
    assert list(dev.host_counts[1]) == [status, 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(_state_bytes(dev, 1), before), "the refused stream's state changed"
    step(lambda s: 2, streams=(0, 2), res=_last_result(dev))   # the others have advanced
    step(lambda s: 2 if s == 1 else 3)
    step(lambda s: 3 if s == 1 else 4)
    _record(f"status {status} ({bad_frame.__name__[5:]})", _grid()[2], bar, worst[0])


def test_cost_status(hip_lib):
    """Tracks founded on velocities of 1e21 make every later float32 association cost overflow: the host's scipy raises
    ``ValueError``, the device answers status 4 and leaves the stream as it was.  The stream stays refused while those tracks
    live (no update ever reaches them), on the host and on the device alike; after ``reset`` it follows a fresh host."""
    from millieye_amd import hip
    bar = _grid_bar()
    n = 3
    dev = _device(n)
    hosts = [mh.HostStream() for _ in range(n)]
    worst = [0.0]

    def frames(f, s):
        return [sh.huge_velocity_frame()] if (s == 1 and f == 0) else sh.grid_radar(s, f)

    def check(f, streams, res):
        for s in streams:
            _check_stream(dev, res, s, hosts[s].step(frames(f, s)), bar, f"stream {s} frame {f}", worst)

    check(0, range(n), dev.gen([frames(0, s) for s in range(n)]))
    before = _state_bytes(dev, 1)
    for f in (1, 2):
        with np.errstate(over="ignore"), pytest.raises(ValueError):
            copy.deepcopy(hosts[1]).step(frames(f, 1))
        with pytest.raises(hip.MeError, match=r"stream 1: no finite association costs"):
            dev.gen([frames(f, s) for s in range(n)])
        assert list(dev.host_counts[1]) == [4, 0, 0, 0, 0, 0, 0, 0]
        assert np.array_equal(_state_bytes(dev, 1), before), "the refused stream's state changed"
        check(f, (0, 2), _last_result(dev))
    dev.reset(1)
    hosts[1] = mh.HostStream()
    for f in (3, 4):
        check(f, range(n), dev.gen([frames(f, s) for s in range(n)]))
    _record("status 4 (cost)", _grid()[2], bar, worst[0])


# ---------------------------------------------------------------------------------------------------------- many streams
def test_many_streams(hip_lib):
    """300 streams, ragged: the pack kernel's prefix sums over the streams in front run their strided loop more than once."""
    n = sh.MANY_STREAMS
    records, host_dev = sh.kalman_runs(sh.many_radar, sh.MANY_BAR_STREAMS, sh.MANY_FRAMES)
    bar = 16.0 * host_dev
    hosts = [mh.HostStream() for _ in range(sh.MANY_BAR_STREAMS, n)]
    dev = _device(n)
    hw = [((480, 640), (640, 480), (360, 480), (512, 512))[s % 4] for s in range(n)]
    worst = [0.0]
    for f in range(sh.MANY_FRAMES):
        radar = [sh.many_radar(s, f) for s in range(n)]
        step = records[f] + [hosts[s - sh.MANY_BAR_STREAMS].step(radar[s]) for s in range(sh.MANY_BAR_STREAMS, n)]
        res = dev.gen(radar, hw)
        clouds = _check_packed(dev, res, step, hw)
        for s in range(n):
            _check_stream(dev, res, s, step[s], bar, f"many frame {f} stream {s}", worst, hw[s])
    assert int(res.host_counts[256:, 4].sum()) > 0 and int(res.host_counts[256:, 1].sum()) > 0
    assert (res.host_counts[0::5, 1:6] == 0).all() and (res.host_counts[1::5, 1:6] == 0).all(), "empty / all-filtered streams"
    _check_heatmaps(dev, clouds, hw)
    _record("many streams", host_dev, bar, worst[0])


# ------------------------------------------------------------------------------------------------- proposals and boxes
def test_proposals_versus_boxes(hip_lib):
    """A small ``max_size`` skips proposals of clusters that stay tracked; frames smaller than the field of view clamp some
    proposals to empty boxes: tracked > pixel proposals > network boxes, on a landscape, a portrait and a square frame."""
    _grid_records, records, host_dev = _grid()
    bar = 16.0 * host_dev
    n = len(sh.BOXES_FRAME_HW)
    dev = _device(n, **sh.BOXES_KW)
    worst = [0.0]
    seen = np.zeros((n, 2), bool)
    for f in range(sh.BOXES_FRAMES):
        res = dev.gen([sh.boxes_radar(s, f) for s in range(n)], sh.BOXES_FRAME_HW)
        for s in range(n):
            _check_stream(dev, res, s, records[f][s], bar, f"boxes frame {f} stream {s}", worst, sh.BOXES_FRAME_HW[s])
            c = res.host_counts[s]
            assert c[3] >= c[7] >= c[4]
            seen[s] |= [c[3] > c[7], c[7] > c[4]]
        _check_packed(dev, res, records[f], sh.BOXES_FRAME_HW)
    assert seen.all(), f"skipped proposals / empty boxes seen per stream: {seen}"
    assert (res.host_counts[:, 4] > 0).all()
    _record("proposals vs boxes", host_dev, bar, worst[0])


# ------------------------------------------------------------------------------------------------------------------ tie
def test_assignment_tie(hip_lib):
    """Two optimal assignments with exactly the same float32 total - square, more tracks than clusters, more clusters than
    tracks: the device settles it as scipy does."""
    n = sh.TIE_STREAMS
    records, host_dev = sh.kalman_runs(sh.tie_radar, n, 2)
    host_dev = host_dev or _grid()[2]   # (one Kalman update per track: the two host runs may agree bit for bit)
    bar = 16.0 * host_dev
    dev = _device(n)
    worst = [0.0]
    for f in range(2):
        res = dev.gen([sh.tie_radar(s, f) for s in range(n)])
        for s in range(n):
            _check_stream(dev, res, s, records[f][s], bar, f"tie frame {f} stream {s}", worst)
    for s, want in enumerate(([0, 1, 2], [0, -1, 1], [0, 2])):
        h = records[1][s]
        assert sh.assignment_margin(h["cost"])[0] == 0.0
        assert list(h["matches"]) == want, "scipy's choice changed: the scene's comment is out of date"
        assert list(dev.matches(s, h["tracks_before"])) == want, f"stream {s}: the tie went another way"
    _record("tie", host_dev, bar, worst[0])


# ------------------------------------------------------------------------------------------------------------ sentinels
def test_sentinels(hip_lib):
    """Every output slot at or behind a stream's counts keeps the marker it held before the step; a refused stream's cluster,
    tracked and proposal slots are not touched at all (its cloud slots and labels are written before the chain can know)."""
    from millieye_amd import hip
    scenes = [lambda f: sh.grid_radar(1, f), lambda f: sh.tie_radar(1, f), lambda f: [], lambda f: sh.many_radar(7, f),
              lambda f: _bad_points(f) if f else sh.grid_radar(0, f), lambda f: _bad_clusters(f) if f else sh.grid_radar(2, f)]
    n = len(scenes)
    dev = _device(n)
    hosts = [mh.HostStream() for _ in range(n)]
    bar = _grid_bar()
    worst = [0.0]
    res = dev.gen([scene(0) for scene in scenes])
    for s in range(n):
        _check_stream(dev, res, s, hosts[s].step(scenes[s](0)), bar, f"sentinels frame 0 stream {s}", worst)
    T = hip.RADAR_MAX_TRACKS
    for buf in (dev._labels, dev._clusters, dev._tracked):
        buf.fill_(MARK_I)
    for buf in (dev._proposals, dev._cloud_slots, dev._cloud, dev._boxes[:n * T]):
        buf.fill_(MARK_F)
    with pytest.raises(hip.MeError, match=r"stream 4 .*256 points"):
        dev.gen([scene(1) for scene in scenes])
    counts = dev.host_counts
    assert list(counts[:, 0]) == [0, 0, 0, 0, 1, 2]
    res = _last_result(dev)
    for s in range(4):
        _check_stream(dev, res, s, hosts[s].step(scenes[s](1)), bar, f"sentinels frame 1 stream {s}", worst)
    mark_f32 = float(np.float32(MARK_F))
    for s in range(n):
        _st, pts, nclu, ntrk, _nb, _alive, _fc, nprop = (int(v) for v in counts[s])
        if counts[s, 0] == 0:
            assert (dev._labels[s, pts:] == MARK_I).all() and (dev._cloud_slots[s, pts:] == MARK_F).all(), f"stream {s}: points"
        assert (dev._clusters[s, nclu:] == MARK_I).all(), f"stream {s}: cluster slots behind {nclu}"
        assert (dev._tracked[s, ntrk:] == MARK_I).all(), f"stream {s}: tracked slots behind {ntrk}"
        assert (dev._proposals[s, nprop:] == MARK_F).all(), f"stream {s}: proposal slots behind {nprop}"
    assert counts[0, 1] > 0 and counts[0, 3] > 0 and counts[2, 1] == 0
    boxes, points = (int(v) for v in dev._totals.cpu())
    assert boxes == int(counts[:, 4].sum()) > 0 and points == int(counts[:, 1].sum())
    assert (dev._boxes[boxes:n * T] == mark_f32).all() and not (dev._boxes[:boxes] == mark_f32).any(), "packed boxes"
    assert (dev._cloud[points:] == MARK_F).all() and not (dev._cloud[:points] == MARK_F).any(), "packed cloud"
