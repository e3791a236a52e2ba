"""millieye_amd/detection_range.py:range_detections against the independent restatement of tests/detection_range_refs.py, bit
for bit (``np.array_equal(..., equal_nan=True)``), and the argument checks of ``ranging=`` on both fusers.  No GPU."""
import numpy as np
import pytest

from millieye_amd import hip
from millieye_amd.detection_range import range_detections, ranging_params
from tests import detection_range_refs as dr

SCENES = dr.edge_scenes()


def _both(name):
    dets, cloud, params = SCENES[name]
    got = range_detections(dets, cloud, **params)
    want = dr.range_rows_ref(dets, cloud, **params)
    assert dr.same(got, want), f"{name}:\n{got}\nvs\n{want}"
    return got


def test_empty_cloud():
    got = _both("empty_cloud")
    assert got.shape == (3, 4) and np.isnan(got[:, :2]).all() and (got[:, 2:] == 0).all()


def test_no_detections():
    assert _both("no_detections").shape == (0, 4)


def test_points_on_the_shrunk_edge_are_inside():
    got = _both("on_the_shrunk_edge")
    assert got[0, 3] == 6 and got[0, 2] == 6 and got[0, 1] == 1.0   # the four points one ulp outside carry velocity 9


def test_equal_ranges_sum_in_cloud_order():
    got = _both("equal_ranges")
    assert got[0, 2] == 3 and got[0, 1] == 1.0 / 3.0
    assert ((1.0 + dr.BIG) + -dr.BIG) / 3.0 == 0.0   # the other order of the tie gives another sum


def test_a_point_at_exactly_the_gate_belongs():
    got = _both("gate_inclusive")
    assert got[0].tolist() == [4.5, 0.375, 2.0, 3.0]


def test_a_lone_first_point_is_skipped():
    got = _both("lone_first_point")
    assert got[0, 2] == 3 and got[0, 3] == 4 and got[0, 0] == ((6.0 + 6.3) + 6.5) / 3


def test_no_group_reaches_min_points():
    got = _both("no_group")
    assert np.isnan(got[0, 0]) and np.isnan(got[0, 1]) and got[0, 2] == 0 and got[0, 3] == 3


def test_overlapping_boxes_share_points():
    got = _both("overlapping_boxes")
    assert got[:, 3].tolist() == [4.0, 4.0] and got[0, 0] == (3.0 + 3.1) / 2 and got[1, 0] == (4.0 + 4.2) / 2


def test_nan_box_coordinate():
    got = _both("nan_coordinate")
    assert np.isnan(got[1, :2]).all() and got[1, 2:].tolist() == [0.0, 0.0] and got[0, 2] == 2 and got[2, 2] == 2


def test_shrink_one():
    got = _both("shrink_one")
    assert got[0, 2:].tolist() == [2.0, 2.0] and got[0, 1] == 1.5


def test_256_points_inside_one_box():
    got = _both("all_256_inside")
    assert got[0, 3] == 256 and got[0, 2] >= 9


@pytest.mark.parametrize("seed", dr.RANDOM_SEEDS)
def test_random_scenes(seed):
    dets, cloud, params = dr.random_scene(seed)
    got = range_detections(dets, cloud, **params)
    assert dr.same(got, dr.range_rows_ref(dets, cloud, **params))
    assert (got[:, 2] > 0).any() and (got[:, 2] == 0).any(), "a scene needs a ranged and an unranged detection"


def test_random_scenes_cover_the_sizes():
    sizes = [(len(d), len(c)) for d, c, _p in map(dr.random_scene, dr.RANDOM_SEEDS)]
    assert min(k for k, _ in sizes) <= 8 and max(k for k, _ in sizes) >= 30
    assert min(p for _, p in sizes) <= 64 and max(p for _, p in sizes) >= 200


def test_parameters_and_inputs():
    dets, cloud, _ = SCENES["overlapping_boxes"]
    got = range_detections(dets, cloud, shrink=0.6, gate=0.05, min_points=1)
    assert dr.same(got, dr.range_rows_ref(dets, cloud, shrink=0.6, gate=0.05, min_points=1)) and (got[:, 2] == 1).all()
    assert dr.same(range_detections(dets[:, :4], cloud), range_detections(dets, cloud))
    import torch
    assert dr.same(range_detections(torch.from_numpy(dets), cloud), range_detections(dets, cloud))
    with pytest.raises(hip.MeError):
        range_detections(dets, np.zeros((257, 4)))
    with pytest.raises(hip.MeError):
        range_detections(dets, cloud, min_points=0)
    with pytest.raises(hip.MeError):
        range_detections(dets, cloud, gate=float("nan"))


def test_ranging_argument():
    assert ranging_params(None, "x") is None and ranging_params(False, "x") is None
    assert ranging_params(True, "x") == dict(shrink=0.8, gate=1.0, min_points=2)
    assert ranging_params(dict(gate=0.5), "x") == dict(shrink=0.8, gate=0.5, min_points=2)
    for bad in (1, "yes", [0.8], dict(gates=1.0), dict(min_points=0), dict(shrink=float("nan"))):
        with pytest.raises(hip.MeError):
            ranging_params(bad, "x")


def test_fusers_check_ranging():
    """Both fusers take ``ranging`` by name (it does not fall into the generator's arguments) and refuse what it cannot be; the
    multi-stream fuser builds its device objects lazily, so this needs no GPU."""
    from millieye_amd.demo import FrameFuser, MultiStreamFuser
    from tests.golden.make_golden import RADAR_CALIB
    multi = MultiStreamFuser(None, RADAR_CALIB, 2, ranging=True)
    assert multi.range_params == dict(shrink=0.8, gate=1.0, min_points=2) and "ranging" not in multi.generator_kwargs
    assert MultiStreamFuser(None, RADAR_CALIB, 2).range_params is None
    assert MultiStreamFuser(None, RADAR_CALIB, 2, ranging=dict(min_points=3), tracks=True).range_params["min_points"] == 3
    with pytest.raises(hip.MeError, match="ranging must be None, True or a dict"):
        MultiStreamFuser(None, RADAR_CALIB, 2, ranging="on")
    with pytest.raises(hip.MeError, match="tail='device'"):
        MultiStreamFuser(None, RADAR_CALIB, 2, tail="host", ranging=True)
    single = FrameFuser(None, RADAR_CALIB, ranging=dict(shrink=0.7))
    assert single.range_params == dict(shrink=0.7, gate=1.0, min_points=2)
    assert FrameFuser(None, RADAR_CALIB).range_params is None
    with pytest.raises(hip.MeError, match="ranging must be None, True or a dict"):
        FrameFuser(None, RADAR_CALIB, ranging=3)


def test_frame_fuser_payload_carries_the_cloud():
    """The host half hands the generator's cloud on, whichever fuser infers (``pipeline.FusionPipeline`` prepares in another
    process with a fuser of its own), and the payload stays picklable."""
    import pickle
    from millieye_amd.demo import FrameFuser
    from tests.golden.make_golden import RADAR_CALIB, radar_points
    fuser = FrameFuser(None, RADAR_CALIB, min_hits=1)
    frame = np.zeros((480, 640, 3), np.uint8)
    payload = fuser.prepare(frame, [radar_points(3)])
    assert payload["cloud"].dtype == np.float64 and payload["cloud"].shape == (payload["points"], 4)
    again = pickle.loads(pickle.dumps(payload))
    assert np.array_equal(again["cloud"], payload["cloud"])
