"""-m gpu: the reference's Python NMS on the device (me_nms_python_f32, csrc/nms_py.hip) through ``hip.nms_python``,
``utils.utils.non_max_suppression`` and ``yolov3.utils.utils.non_max_suppression``: against the goldens recorded from the real
reference (tests/golden/pynms.npz), against the numpy restatement (tests/pynms_refs.py) at the candidate counts where the
kernels change path, and on scenes whose answer is known in closed form.

Without merging every row is compared with ``torch.equal`` / ``np.array_equal``.  With merging the decisions and columns 4-6 are
exact and the boxes lie within 16 x the reference's own fp32 deviation from float64 (stored in the golden per scene and
setting); scenes outside the goldens take the bar written at their test.

Measured on an MI355X (profiles/pynms_errors.txt): the device's merged boxes deviate from the float64 restatement by at most
half an fp32 unit of the coordinate (the sums are float64, rounded once).
"""
import os

import numpy as np
import pytest
import torch

from millieye_amd import hip
from tests import pynms_refs as refs
from tests import pynms_scene_helpers as sh

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = {"m3": (0, False, False), "vend": (1, True, True)}  # score_mode, inclusive, merge
TILE, KCHUNK = hip.PYNMS_TILE, hip.PYNMS_KEEPER_CHUNK


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pynms.npz"))


def _wrapper(fn):
    if fn == "m3":
        from millieye_amd.utils.utils import non_max_suppression
    else:
        from millieye_amd.yolov3.utils.utils import non_max_suppression
    return non_max_suppression


def _device(pred_np, conf, thr, score_mode, inclusive, merge):
    """hip.nms_python on a copy of ``pred_np``: (list of numpy ``[k,7]`` rows or None, the prediction after the call)."""
    dev = torch.from_numpy(pred_np).cuda()
    det, cnt = hip.nms_python(dev, float(conf), float(thr), score_mode, inclusive, merge)
    counts = cnt.tolist()
    det = det.cpu().numpy()
    return [det[i, :k].copy() if k else None for i, k in enumerate(counts)], dev.cpu().numpy()


def _check(got, res, merge, bar=None, what=""):
    """Device rows of one image against the restatement's: exact, or (merge) decisions and columns 4-6 exact and boxes in ``bar``."""
    assert (got is None) == (res is None), what
    if got is None:
        return 0.0
    assert got.shape == res["rows"].shape, (what, got.shape, res["rows"].shape)
    if not merge:
        assert np.array_equal(got, res["rows"]), what
        return 0.0
    assert np.array_equal(got[:, 4:], res["rows"][:, 4:]), what
    dev = float(np.abs(got[:, :4].astype(np.float64) - res["merged"]).max())
    print(f"{what}: merged boxes deviate {dev:.3e} px from float64, bar {bar:.3e}")
    assert dev <= bar, (what, dev, bar)
    return dev


# ---- goldens ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", sorted(VARIANTS))
@pytest.mark.parametrize("name", sh.GOLDEN_SCENES)
def test_goldens(hip_lib, golden, name, fn):
    merge = VARIANTS[fn][2]
    pred = sh.golden_scene(name)
    assert sh.checksum(pred) == str(golden[f"{name}|checksum"])
    for conf, thr in sh.GOLDEN_SETTINGS:
        dev = torch.from_numpy(pred).cuda()  # (from_numpy shares memory; .cuda() copies)
        out = _wrapper(fn)(dev, conf, thr)
        xyxy = dev[..., :4].cpu().numpy()
        assert sh.checksum(xyxy) == str(golden[sh.golden_key(name, conf, thr, fn, "all", "xyxy_checksum")])  # in place, every row
        assert np.array_equal(dev[..., 4:].cpu().numpy(), pred[..., 4:])
        for img, rows in enumerate(out):
            want = golden[sh.golden_key(name, conf, thr, fn, img)]
            what = f"{name} {fn} conf {conf} thr {thr} image {img}"
            if rows is None:
                assert want.shape == (0, 7), what
                continue
            assert rows.is_cuda and rows.dtype == torch.float32
            if not merge:
                assert torch.equal(rows.cpu(), torch.from_numpy(want)), what
            else:
                rows = rows.cpu().numpy()
                assert rows.shape == want.shape and np.array_equal(rows[:, 4:], want[:, 4:]), what
                bar = 16 * float(golden[sh.golden_key(name, conf, thr, fn, "all", "ref_dev")])
                # the float64 boxes: the restatement's, whose decisions equal the golden's (tests/test_pynms_refs_cpu.py)
                res = refs.nms_python_ref(pred[img:img + 1].copy(), conf, thr, *VARIANTS[fn])[0]
                _check(rows, res, True, bar, what)


# ---- candidate counts where the kernels change path ---------------------------------------------------------------------------
EDGE_COUNTS = sorted({1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097,              # wave, MATN and LDS_CANDS of nms.hip
                      KCHUNK - 1, KCHUNK, KCHUNK + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1})


@pytest.fixture(scope="module")
def edge_base():
    return sh.scene("pynms/edges", 1, 4400, 5, obj_mean=2.0)


@pytest.mark.parametrize("count", EDGE_COUNTS)
def test_candidate_count_edges(hip_lib, edge_base, count):
    pred = sh.with_candidates(edge_base, 0.05, count)
    sh.assert_defined(pred, 0.5)
    for fn, args in VARIANTS.items():
        want_in = pred.copy()
        res = refs.nms_python_ref(want_in, 0.05, 0.5, *args)[0]
        assert res["cands"] == count
        got, after = _device(pred, 0.05, 0.5, *args)
        assert np.array_equal(after, want_in)
        # bar: the device rounds its float64 mean once to fp32 (half a unit of the coordinate; the float64 sums themselves differ
        # by their order, ~1e-13): one fp32 unit of a coordinate in [512, 1024) px, and the scene stays under 1024 px
        _check(got[0], res, args[2], float(np.spacing(np.float32(512))), f"{count} candidates {fn}")


@pytest.mark.parametrize("keepers", [KCHUNK - 1, KCHUNK, KCHUNK + 1, 2 * KCHUNK + 1])
def test_keeper_chunk_edges(hip_lib, keepers):
    """``keepers`` disjoint boxes and, behind them in score order, copies of each (shifted by a fraction of a pixel) that fill
    two more tiles: the first tile holds exactly ``keepers`` keepers when the later tiles are tested against them, and every
    later candidate is owned by one of them - the last keeper of a chunk included."""
    m = 2 * TILE + keepers + 7
    k = np.arange(m)
    site = k % keepers
    side = int(np.ceil(np.sqrt(keepers)))
    shift = (k // keepers) / 64.0  # exact
    boxes = np.stack([32.0 * (site % side) + 16.0 + shift, 32.0 * (site // side) + 16.0, np.full(m, 20.0), np.full(m, 20.0)], 1)
    obj = (np.float32(0.75) - k.astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)  # row order = score order
    pred = sh.rows_from(boxes, obj, np.zeros(m, np.int64))
    for fn, args in VARIANTS.items():
        res = refs.nms_python_ref(pred.copy(), 0.01, 0.5, *args)[0]
        assert list(res["index"]) == list(range(keepers))  # the closed-form answer: the first `keepers` rows
        got, _ = _device(pred, 0.01, 0.5, *args)
        _check(got[0], res, args[2], float(np.spacing(np.float32(512))), f"{keepers} keepers {fn}")


# ---- analytic scenes ------------------------------------------------------------------------------------------------------------
def test_32768_disjoint_candidates_are_all_kept(hip_lib):
    m = hip.PYNMS_MAX_ROWS
    pred = sh.grid_scene(m)
    xyxy = refs.xywh2xyxy(pred.copy())[0]
    order = np.argsort(-xyxy[:, 4], kind="stable")
    want = np.concatenate([xyxy[order, :5], np.full((m, 1), 0.75, np.float32), np.zeros((m, 1), np.float32)], 1)
    for args in VARIANTS.values():
        got, _ = _device(pred, 0.01, 0.5, *args)
        assert got[0].shape == (m, 7)  # no cap
        assert np.array_equal(got[0], want)  # (merging: clusters of one; obj * box / obj of these small integers is exact)


def test_pile_of_32768_gives_one_row(hip_lib):
    m = hip.PYNMS_MAX_ROWS
    pred = sh.pile_scene(m)
    xyxy = refs.xywh2xyxy(pred.copy())[0]
    top = int(np.argmax(xyxy[:, 4]))
    got, _ = _device(pred, 0.01, 0.5, *VARIANTS["m3"])
    assert np.array_equal(got[0], np.concatenate([xyxy[top, :5], [np.float32(0.75), np.float32(1)]])[None])
    got, _ = _device(pred, 0.01, 0.5, *VARIANTS["vend"])
    assert got[0].shape == (1, 7) and np.array_equal(got[0][0, 4:], [xyxy[top, 4], np.float32(0.75), np.float32(1)])
    wgt = xyxy[:, 4].astype(np.float64)
    mean = (wgt[:, None] * xyxy[:, :4].astype(np.float64)).sum(0) / wgt.sum()
    # bar: fp32 rounding of the same sum - both sides round a float64 mean (relative error ~1e-13, summed in different orders)
    # once to fp32, so they are at most one fp32 unit of the coordinate apart
    bar = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
    dev = np.abs(got[0][0, :4].astype(np.float64) - mean)
    print("pile: deviation", dev, "bar", bar)
    assert (dev <= bar).all()


@pytest.mark.parametrize("fillers", [TILE - 3, TILE - 2, TILE - 1, TILE, 2 * TILE - 1])
def test_chain_across_a_tile_boundary(hip_lib, fillers):
    """``fillers`` disjoint keepers of class 0, then the chain A, B, C of class 1: A removes B; B, removed, must not remove C -
    with A, B and C on either side of the boundary between two tiles."""
    grid = sh.grid_scene(fillers)[0]
    boxes, obj = sh.chain_rows()
    chain = sh.rows_from([(x + 5000.0, y, w, h) for x, y, w, h in boxes], np.array(obj, np.float32) * np.float32(0.25),
                         np.ones(3, np.int64))[0]
    pred = np.concatenate([grid, chain])[None]
    assert pred[0, :fillers, 4].min() > chain[:, 4].max()
    for fn, args in VARIANTS.items():
        res = refs.nms_python_ref(pred.copy(), 0.01, 0.5, *args)[0]
        assert len(res["index"]) == fillers + 2 and list(res["index"][-2:]) == [fillers, fillers + 2]  # A and C
        got, _ = _device(pred, 0.01, 0.5, *args)
        # (bar as in test_candidate_count_edges; the chain sits at x ~ 5000: one fp32 unit of [4096, 8192))
        _check(got[0], res, args[2], float(np.spacing(np.float32(4096))), f"chain behind {fillers} {fn}")


def test_equal_boxes_with_different_labels_are_all_kept(hip_lib):
    m = 70
    pred = sh.rows_from([(100.0, 100.0, 50.0, 50.0)] * m, sh.descending_obj(m), np.arange(m), num_classes=m)
    for args in VARIANTS.values():
        got, _ = _device(pred, 0.01, 0.5, *args)
        assert got[0].shape == (m, 7) and (np.diff(got[0][:, 4]) < 0).all()
        assert sorted(got[0][:, 6].tolist()) == list(range(m))
        assert (got[0][:, :4] == np.array([75, 75, 125, 125], np.float32)).all()


# ---- thresholds and order ---------------------------------------------------------------------------------------------------------
def test_exact_threshold_pair_under_both_comparisons(hip_lib):
    pred = sh.exact_pair_scene()
    got, _ = _device(pred, 0.01, 0.5, 0, False, False)
    assert np.array_equal(got[0][:, :4], np.array([[0, 0, 9, 9], [0, 0, 9, 4]], np.float32))
    got, _ = _device(pred, 0.01, 0.5, 0, True, False)
    assert np.array_equal(got[0][:, :4], np.array([[0, 0, 9, 9]], np.float32))
    out = _wrapper("m3")(torch.from_numpy(pred).cuda(), 0.01, 0.5)
    assert out[0].shape == (2, 7)
    out = _wrapper("vend")(torch.from_numpy(pred).cuda(), 0.01, 0.5)
    assert torch.equal(out[0].cpu(), torch.tensor([[0, 0, 9, 7, 0.75, 0.75, 0]], dtype=torch.float32))


def test_objectness_equal_to_the_threshold_is_kept(hip_lib):
    below = np.nextafter(np.float32(0.25), np.float32(0))
    pred = sh.rows_from([(10.0, 10.0, 8.0, 8.0), (100.0, 10.0, 8.0, 8.0)], np.array([0.25, below], np.float32), [0, 0])
    got, _ = _device(pred, 0.25, 0.5, 0, False, False)
    assert got[0].shape == (1, 7) and got[0][0, 4] == np.float32(0.25)


def test_score_mode_changes_the_order(hip_lib):
    pred = sh.rows_from([(10.0, 10.0, 8.0, 8.0), (100.0, 10.0, 8.0, 8.0)], np.array([0.9, 0.8], np.float32), [0, 1])
    pred[0, 0, 5] = 0.5  # row 0: 0.9 * 0.5 = 0.45; row 1: 0.8 * 0.75 = 0.6
    got, _ = _device(pred, 0.01, 0.5, 0, False, False)
    assert got[0][:, 4].tolist() == [np.float32(0.9), np.float32(0.8)] and got[0][:, 5].tolist() == [0.5, 0.75]
    got, _ = _device(pred, 0.01, 0.5, 1, False, False)
    assert got[0][:, 4].tolist() == [np.float32(0.8), np.float32(0.9)]


def test_exact_ties_go_to_the_lower_row(hip_lib):
    m = 130
    grid = sh.grid_scene(m)
    grid[0, :, 4] = 0.5
    twins = sh.rows_from([(3000.0, 10.0, 8.0, 8.0), (3000.0, 10.0, 8.0, 8.0)], np.array([0.5, 0.5], np.float32), [1, 1])
    pred = np.concatenate([grid[0], twins[0]])[None]
    want = refs.xywh2xyxy(pred.copy())[0]
    for score_mode in (0, 1):
        got, _ = _device(pred, 0.01, 0.5, score_mode, False, False)
        assert np.array_equal(got[0][:, :4], want[:m + 1, :4])  # rows 0 .. m - 1 in row order, then the first twin only
        assert np.array_equal(refs.nms_python_ref(pred.copy(), 0.01, 0.5, score_mode)[0]["index"], np.arange(m + 1))


# ---- special values ---------------------------------------------------------------------------------------------------------------
def test_nan_objectness_drops_out_and_nan_coordinates_remove_nothing(hip_lib):
    box = (50.0, 50.0, 40.0, 40.0)
    pred = sh.rows_from([box, box, box, box, box], np.array([0.9, 0.95, 0.8, 0.7, 0.6], np.float32), [0] * 5)
    pred[0, 0, 4] = np.nan   # row 0: NaN objectness - no candidate
    pred[0, 1, 0] = np.nan   # row 1: the best score and a NaN box - kept, removes nothing (the reference would not end here)
    pred[0, 3, 3] = np.nan   # row 3: a NaN box further down - row 2 does not remove it
    for args in VARIANTS.values():
        got, after = _device(pred, 0.01, 0.5, *args)
        rows = got[0]
        assert rows[:, 4].tolist() == [np.float32(0.95), np.float32(0.8), np.float32(0.7)]  # row 4 is removed by row 2
        assert np.isnan(rows[0, :4]).any() and np.isnan(rows[2, :4]).any()
        if not args[2]:
            assert np.array_equal(rows[1, :4], np.array([30, 30, 70, 70], np.float32))
        assert np.array_equal(after, refs.xywh2xyxy(pred.copy()), equal_nan=True)


# ---- empty inputs and refusals ------------------------------------------------------------------------------------------------------
def test_empty_inputs(hip_lib):
    for fn in VARIANTS:
        assert _wrapper(fn)(torch.empty((0, 10, 7), device="cuda"), 0.01, 0.5) == []
        assert _wrapper(fn)(torch.empty((2, 0, 7), device="cuda"), 0.01, 0.5) == [None, None]
        pred = sh.scene("pynms/none", 2, 100, 3)
        pred[1, :, 4] = 0.001
        out = _wrapper(fn)(torch.from_numpy(pred).cuda(), 0.01, 0.5)
        assert out[0] is not None and out[1] is None


def test_more_rows_than_the_capacity_are_refused(hip_lib):
    pred = torch.zeros((1, hip.PYNMS_MAX_ROWS + 1, 6), device="cuda")
    with pytest.raises(hip.MeError):
        hip.nms_python(pred, 0.01, 0.5, 0, False, False)
    assert hip.lib().me_nms_python_workspace_bytes(1, hip.PYNMS_MAX_ROWS) > 0


# ---- repeatability, workspace state, wrapper paths ----------------------------------------------------------------------------------
def test_two_calls_are_bit_identical_and_the_workspace_content_is_irrelevant(hip_lib):
    pred = sh.golden_scene("s2535")
    n, rows = pred.shape[:2]
    for args in VARIANTS.values():
        first, _ = _device(pred, 0.01, 0.5, *args)
        second, _ = _device(pred, 0.01, 0.5, *args)
        _ptr, ws = hip._workspace(hip.lib().me_nms_python_workspace_bytes(n, rows), torch.device("cuda", torch.cuda.current_device()),
                                  slot="nms_python")
        ws.fill_(0xFF)
        third, _ = _device(pred, 0.01, 0.5, *args)
        for a, b, c in zip(first, second, third):
            assert a.tobytes() == b.tobytes() == c.tobytes()


def test_cpu_prediction_goes_through_the_wrapper(hip_lib):
    pred = sh.golden_scene("gap")
    for fn, args in VARIANTS.items():
        cpu = torch.from_numpy(pred.copy())
        out = _wrapper(fn)(cpu, 0.2, 0.3)
        want_in = pred.copy()
        res = refs.nms_python_ref(want_in, 0.2, 0.3, *args)
        assert torch.equal(cpu, torch.from_numpy(want_in))  # the first four columns written back as xyxy
        for rows, r in zip(out, res):
            assert (rows is None) == (r is None)
            if rows is not None:
                assert rows.device.type == "cpu" and np.array_equal(rows.numpy()[:, 4:], r["rows"][:, 4:])
                if not args[2]:
                    assert np.array_equal(rows.numpy(), r["rows"])


def test_batch_of_32_equals_32_single_calls(hip_lib):
    pred = sh.scene("pynms/batch32", 32, 700, 6)
    for args in VARIANTS.values():
        batch, after = _device(pred, 0.01, 0.5, *args)
        for i in range(32):
            single, after1 = _device(pred[i:i + 1], 0.01, 0.5, *args)
            assert (batch[i] is None) == (single[0] is None)
            assert batch[i].tobytes() == single[0].tobytes()
            assert np.array_equal(after[i], after1[0])
