"""CPU: guards of the NMS scenes (tests/nms_scene_helpers.py) that tests/test_gpu_nms_regimes.py runs on the device - every scene
lands in the regime its name claims (the CPU model of nms.hip's dispatch) and still tells the right rule from the wrong one it
is there to catch, judged with the oracle alone.  Conditions on the inputs, not measurements."""
import numpy as np
import pytest

from tests import nms_scene_helpers as sh


def _kept(scene, thr, use_labels=True):
    boxes, scores, labels = scene
    return sh.oracle_keep(boxes, scores, labels if use_labels else None, thr)


def test_model_reaches_every_route_at_the_listed_sizes():
    for m, want in sh.BOXES_REGIMES.items():
        assert sh.regime(m, m, m) == want, m
    names = set(sh.BOXES_REGIMES.values())
    assert names == {"matrix/bulk", "matrix/bulk -> fallback/reg", "matrix/bulk -> fallback/lds", "matrix/bulk -> fallback/global",
                     "matrix/two-buffer -> fallback/global"}
    for cap, want in sh.GROUP_REGIMES.items():
        assert cap >= max(sh.GROUP_SIZES)
        assert tuple(sh.regime(c, cap, cap) for c in sh.GROUP_SIZES) == want, cap
    # the edges of the model itself
    assert sh.dispatch(129, 129, 129)["matn"] == 192 and sh.dispatch(129, 129, 129)["wc"] == 3
    assert sh.dispatch(5632, 5632, 5632)["bulk"] and not sh.dispatch(5633, 5633, 5633)["bulk"]
    assert [sh.select_mode(c) for c in (768, 769, 2048, 2049, 4096, 4097, 32768)] == \
        ["mat", "reg", "reg", "lds", "lds", "global", "global"]
    assert {sh.select_mode(m) for m in sh.SWITCH_BOXES} == {"mat", "reg", "lds", "global"}
    # the batched grid: max_det 1024 stays on the continuation side, 1025 and the clamped 2000 fall back
    rows = sh.BATCHED_ROWS
    for max_det in sh.BATCHED_MAX_DET:
        for cnt in sh.BATCHED_COUNTS:
            d = sh.dispatch(cnt, max_det, rows, top=0)
            assert d["max_det_eff"] == min(max_det, rows) and d["bulk"]
            assert d["fallback"] == (cnt > 1024 and max_det > 1024)
    assert sh.dispatch(1500, 2000, rows)["max_det_eff"] == rows


@pytest.mark.parametrize("m", [129, 1025, 3000, 5633])
def test_clustered_scene_suppresses_and_keeps_the_walk_short(m):
    for use_labels in (True, False):
        k = len(_kept(sh.clustered(m, m), 0.5, use_labels))
        assert 0 < k < m and k <= 1300, (m, use_labels, k)


def test_clustered_32768_keeps_the_walk_short():
    k = len(_kept(sh.clustered(sh.MAX_ROWS, sh.MAX_ROWS), 0.5))
    assert 300 < k <= 2000, k   # hundreds of winners, yet a couple of thousand serial steps at the most


def test_separated_scene_keeps_everything():
    scene = sh.separated(300)
    assert len(np.unique(scene[1])) == 300 and scene[1].min() >= sh.CONF
    for use_labels in (True, False):
        assert len(_kept(scene, 0.0, use_labels)) == 300


@pytest.mark.parametrize("thr", [0.5, 0.25])
def test_exact_threshold_scene(thr):
    boxes, scores, labels = sh.exact_threshold(thr)
    t = np.float32(thr)
    for use_labels in (True, False):
        ovr, _ = sh.iou_matrix(sh.shifted(boxes, labels if use_labels else None))
        iu = np.triu_indices(len(boxes), 1)
        v = ovr[iu]
        exact, above, below = int((v == t).sum()), int((v == np.nextafter(t, np.float32(1))).sum()), \
            int((v == np.nextafter(t, np.float32(0))).sum())
        print(f"thr {thr} labels {use_labels}: {exact} pairs at the threshold, {above} one step above, {below} one step below")
        assert exact >= 20 and above >= 1 and below >= 1
        order = sh.key_order(scores)
        b = sh.shifted(boxes, labels if use_labels else None)
        strict, inclusive = sh.greedy(b, order, thr), sh.greedy(b, order, thr, inclusive=True)
        assert np.array_equal(strict, _kept((boxes, scores, labels), thr, use_labels)), "the plain greedy walk is not the oracle's"
        assert set(strict.tolist()) != set(inclusive.tolist()) and len(strict) - len(inclusive) >= 20


@pytest.mark.parametrize("m", [1500, 3000, 4200])
def test_equal_scores_scene_depends_on_the_tie_rule(m):
    boxes, scores, labels = sh.equal_scores(m)
    assert len(np.unique(scores)) == 1
    want = _kept((boxes, scores, labels), 0.5)
    assert np.array_equal(want, np.sort(want)) and want[0] == 0, "lower row first"
    flipped = m - 1 - _kept((boxes[::-1], scores, labels[::-1]), 0.5)   # the kept set of a "higher row first" rule
    assert set(want.tolist()) != set(flipped.tolist())
    assert sh.regime(m, m, m) == {1500: "matrix/bulk -> fallback/reg", 3000: "matrix/bulk -> fallback/lds",
                                  4200: "matrix/bulk -> fallback/global"}[m]


def test_score_edges_scene():
    boxes, scores, labels = sh.score_edges()
    bits = scores.view(np.uint32)
    assert (bits == 0).sum() >= 10 and (bits == 0x80000000).sum() >= 10 and np.isneginf(scores).sum() >= 10
    sub = (np.abs(scores) > 0) & (np.abs(scores) < np.float32(1.1754944e-38))
    assert (sub & (scores > 0)).sum() >= 10 and (sub & (scores < 0)).sum() >= 10 and not np.isnan(scores).any()
    b = sh.shifted(boxes, labels)
    want = _kept((boxes, scores, labels), 0.5)
    assert np.array_equal(want, sh.greedy(b, sh.key_order(scores), 0.5))
    # the rule sortable() alone implements: -0 below +0
    s = scores.astype(np.float64)
    s[bits == 0x80000000] = -1e-300
    wrong = sh.greedy(b, np.lexsort((np.arange(len(s)), -s)), 0.5)
    assert set(want.tolist()) != set(wrong.tolist())
    assert 5 in want and 200 not in want and 200 in wrong and 5 not in wrong


def test_nan_scene_depends_on_where_nan_sorts():
    boxes, scores, labels = sh.nan_scores()
    r = sh.NAN_ROWS
    bits = scores.view(np.uint32)
    assert [int(bits[r[k]]) for k in ("plus", "sign", "payload_low_row", "payload_high_row")] == \
        [0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7FD00000]
    assert np.isnan(scores).sum() == 4 and not np.isposinf(scores).any()
    for use_labels in (True, False):
        b = sh.shifted(boxes, labels if use_labels else None)
        want = _kept((boxes, scores, labels), 0.5, use_labels)
        assert want[:3].tolist() == [r["plus"], r["sign"], r["payload_low_row"]], "NaN rows first, the lower row first"
        assert np.array_equal(want, sh.greedy(b, sh.key_order(scores), 0.5))
        # what sortable() alone gives: a sign-bit NaN below -inf, positive NaNs by payload
        sortable = np.where(bits & 0x80000000, ~bits, bits | 0x80000000).astype(np.int64)
        wrong = sh.greedy(b, np.lexsort((np.arange(len(bits)), -sortable)), 0.5)
        assert r["sign"] in want and r["sign"] not in wrong
        assert r["payload_low_row"] in want and r["payload_low_row"] not in wrong and r["payload_high_row"] in wrong


def test_degenerate_scenes():
    scenes = sh.degenerate()
    assert set(scenes) == {"plain", "huge", "inf", "nan"}
    boxes = scenes["plain"][0]
    ovr, inter = sh.iou_matrix(boxes)
    iu = np.triu_indices(len(boxes), 1)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    zero_over_zero = int((np.isnan(ovr[iu]) & (inter[iu] == 0)).sum())
    tiny = np.float32(1.1754944e-38)
    subnormal_inter = int(((inter[iu] > 0) & (inter[iu] < tiny)).sum())
    print(f"{zero_over_zero} 0 / 0 pairs, {subnormal_inter} subnormal intersections")
    assert zero_over_zero >= 1 and subnormal_inter >= 1
    assert (area == 0).sum() >= 16 and (area < 0).sum() >= 8 and ((area > 0) & (area < tiny)).sum() >= 30
    assert ((boxes[:, 0] > boxes[:, 2]).sum() >= 4) and ((boxes[:, 1] > boxes[:, 3]).sum() >= 4)
    # the subnormal clusters suppress: a device that flushes denormals (0 / 0) keeps every one of them
    kept = set(_kept(scenes["plain"], 0.5, False).tolist())
    assert 0 < len(kept & set(range(40, 80))) < 40
    with np.errstate(all="ignore"):
        h = scenes["huge"][0]
        assert np.abs(h).max() >= 1e30 and np.isinf((h[:, 2] - h[:, 0]) * (h[:, 3] - h[:, 1])).any()
    assert np.isposinf(scenes["inf"][0]).sum() == 1 and np.isneginf(scenes["inf"][0]).sum() == 1
    assert np.isnan(sh.shifted(scenes["inf"][0], scenes["inf"][2])[scenes["inf"][2] == 0]).all(), "label 0: 0 * inf"
    assert np.isnan(scenes["nan"][0]).sum() == 1
    assert len(_kept(scenes["nan"], 0.5)) == 200, "a NaN maximum shifts every box to NaN: all kept"
    assert len(_kept(scenes["nan"], 0.5, False)) < 200


def _continuation_facts(scene, max_det=sh.CONT_MAX_DET, thr=0.5):
    """Through the prediction tensor, as the device sees the scene: (candidates, top, position in key order of every winner of the
    uncapped walk)."""
    pred = sh.to_pred(scene, 3200)
    rows, boxes, scores, labels = sh.pred_candidates(pred)
    full = sh.oracle_keep(boxes, scores, labels, thr)
    order = sh.key_order(scores)
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order))
    return len(rows), sh.top_winners(boxes, scores, labels, thr, max_det), pos[full]


def test_continuation_scenes_meet_their_edges():
    scenes = sh.continuation_scenes()
    md = sh.CONT_MAX_DET
    # (a) one winner short behind the matrix; it sits in the second continuation block, not at a block edge
    cnt, top, pos = _continuation_facts(scenes["a"])
    assert cnt >= 3000 and top == md - 1 and sh.regime(cnt, md, 3200, top) == "matrix/bulk -> continuation"
    assert pos[md - 1] == 1024 + 70 and len(pos) > md
    # (b) max_det is reached in the middle of a continuation block, the uncapped list goes on
    cnt, top, pos = _continuation_facts(scenes["b"])
    assert cnt >= 3000 and top == 150 and sh.regime(cnt, md, 3200, top) == "matrix/bulk -> continuation"
    assert pos[md - 1] >= 1024 + 64 and 8 <= pos[md - 1] % 64 <= 55 and len(pos) > md + 100
    assert pos[md] // 64 == pos[md - 1] // 64, "a further winner waits in the same block"
    # (c) the walk runs off a list that is no multiple of 64 with fewer than max_det winners, the last candidate among them
    cnt, top, pos = _continuation_facts(scenes["c"])
    assert cnt == 3001 and cnt % 64 != 0 and top == 100 and sh.regime(cnt, md, 3200, top) == "matrix/bulk -> continuation"
    assert len(pos) == 130 < md and pos[-1] == cnt - 1
    # at max_det 1 and 65 the matrix part alone serves them; 65 ends on the first candidate of a block for the separated scene
    for max_det in (1, 65):
        for k in "abc":
            cnt, top, _ = _continuation_facts(scenes[k], max_det)
            assert top == max_det and sh.regime(cnt, max_det, 3200, top) == "matrix/bulk"


def test_pred_round_trip_keeps_labels_and_counts():
    for cnt in sh.BATCHED_COUNTS:
        rows, boxes, scores, labels = sh.pred_candidates(sh.batched_image(cnt, 70 + cnt))
        assert len(rows) == cnt
        if cnt:
            want = sh.clustered(cnt, 70 + cnt)
            assert np.array_equal(labels, want[2]) and np.array_equal(scores, want[1])
