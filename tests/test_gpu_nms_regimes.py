"""-m gpu: the NMS of csrc/nms.hip in every selection regime, at its boundaries and ties - the ranked bit matrix with the bulk and
the two-buffer scan, the continuation behind the 1024 best-scored candidates, the fallback into nms_select_kernel's register,
LDS-list and global-list modes, and its LDS-matrix mode under MILLIEYE_NMS_LEGACY=1.  Every comparison is exact, against
oracle/tv_ops (me_nms_boxes_f32, me_nms_boxes_grouped_f32) or the restatement of non_max_suppression_cpp in test_gpu_nms.py
(me_nms_batched_f32).  The C ABI is called directly with a workspace the test owns: poisoned with 0xFF bytes and again with
0x5A5A5A5A (both must give the same rows), guard words behind it and around every output.  After each call the candidate counts
and fallback flags the pipeline left are compared with the CPU model of the dispatch (tests/nms_scene_helpers.py), so a scene that
misses its regime fails; tests/test_nms_scenes_cpu.py guards the scenes themselves."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import nms_scene_helpers as sh
from tests.test_gpu_nms import _oracle_nms_cpp

pytestmark = pytest.mark.gpu

PAD = 64                              # guard words on either side of every buffer
GUARD = 0x5A5A5A5A
FILLS = (-1, 0x5A5A5A5A)              # the workspace poison as int32 words: 0xFF bytes, 0x5A5A5A5A


def _guarded(count, dtype):
    """``count`` elements of ``dtype`` (4 or 8 bytes) between PAD guard words: (whole int32 buffer, the view to hand out)."""
    words = count * torch.empty((), dtype=dtype).element_size() // 4
    full = torch.full((PAD + words + PAD,), GUARD, dtype=torch.int32, device="cuda")
    return full, full[PAD:PAD + words].view(dtype)


def _intact(full):
    h = full.cpu()
    return bool((h[:PAD] == GUARD).all()) and bool((h[-PAD:] == GUARD).all())


class _Workspace:
    """A 256-byte aligned workspace of me_nms_workspace_bytes(n, cap) bytes inside a buffer filled with ``fill`` words."""

    def __init__(self, n, cap, fill):
        from millieye_amd import hip
        self.n, self.cap, self.fill = n, cap, fill
        self.nbytes = int(hip.lib().me_nms_workspace_bytes(n, cap))
        assert self.nbytes > 0 and self.nbytes % 256 == 0
        self.buf = torch.full((self.nbytes // 4 + 64 + PAD,), fill, dtype=torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + (-self.buf.data_ptr()) % 256
        self.off = (self.ptr - self.buf.data_ptr()) // 4

    def intact(self):
        h = self.buf.cpu()
        return bool((h[:self.off] == self.fill).all()) and bool((h[self.off + self.nbytes // 4:] == self.fill).all())

    def counts(self):
        """(candidate counts, fallback flags) the finished pipeline left, through me_nms_candidate_counts."""
        from millieye_amd import hip
        full, out = _guarded(2 * self.n, torch.int32)
        hip.check(hip.lib().me_nms_candidate_counts(self.ptr, self.n, self.cap, out.data_ptr(), out[self.n:].data_ptr(),
                                                    hip.stream_ptr()), "me_nms_candidate_counts")
        torch.cuda.synchronize()
        assert _intact(full)
        h = out.cpu().tolist()
        return h[:self.n], h[self.n:]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# ---- me_nms_boxes_f32 ------------------------------------------------------------------------------------------------------------
def _boxes_call(scene, thr, use_labels, fill):
    from millieye_amd import hip
    boxes, scores, labels = (_dev(a) for a in scene)
    m = int(boxes.shape[0])
    ws = _Workspace(1, m, fill)
    keep_full, keep = _guarded(m, torch.int64)
    cnt_full, cnt = _guarded(1, torch.int32)
    hip.check(hip.lib().me_nms_boxes_f32(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr() if use_labels else None, m,
                                         float(thr), keep.data_ptr(), cnt.data_ptr(), ws.ptr, hip.stream_ptr()),
              "me_nms_boxes_f32")
    cand, fb = ws.counts()
    assert _intact(keep_full) and _intact(cnt_full) and ws.intact(), "guard words overwritten"
    k = int(cnt.cpu()[0])
    assert 0 <= k <= m
    return keep[:k].cpu(), cand[0], fb[0]


def _check_boxes(scene, thr, use_labels, what=""):
    """Both poisons give the oracle's rows; the counts and the fallback flag are the model's.  Returns the kept rows."""
    m = len(scene[0])
    want = torch.from_numpy(sh.oracle_keep(scene[0], scene[1], scene[2] if use_labels else None, thr))
    model = sh.dispatch(m, m, m)
    for fill in FILLS:
        got, cand, fb = _boxes_call(scene, thr, use_labels, fill)
        assert cand == m and fb == int(model["fallback"]), f"{what}: {cand} candidates, fallback {fb}; the model says {model}"
        assert got.dtype == torch.int64 and torch.equal(got, want), \
            f"{what} m={m} thr={thr} labels={use_labels} poison {fill:#x}: kept rows differ from the oracle " \
            f"({len(got)} vs {len(want)} kept)"
    return want


@pytest.mark.parametrize("m", [m for m in sh.BOXES_REGIMES if m < sh.MAX_ROWS])
def test_boxes_at_every_edge_of_the_dispatch(hip_lib, m):
    """64 / 65 (one / two blocks), 129 (matn 192, wc 3: a 16-byte piece of the scan's loads straddles two matrix rows), 768 / 769,
    1024 / 1025 (the matrix alone / the fallback), 2048 / 2049 (register / LDS-list mode), 4096 / 4097 (LDS / global lists),
    5632 / 5633 (bulk / two-buffer scan)."""
    assert sh.regime(m, m, m) == sh.BOXES_REGIMES[m]
    scene = sh.clustered(m, m)
    for use_labels in (True, False):
        want = _check_boxes(scene, 0.5, use_labels, "clustered")
        assert m == 1 or len(want) < m


def test_boxes_at_the_capacity(hip_lib):
    """32768 rows: 32 candidates per thread of the global-list mode, the last bit of its ``alive`` register."""
    m = sh.MAX_ROWS
    assert sh.regime(m, m, m) == sh.BOXES_REGIMES[m]
    scene = sh.clustered(m, m)
    for use_labels in (True, False):
        assert 100 < len(_check_boxes(scene, 0.5, use_labels, "clustered")) < 2500   # a short serial walk


# ---- me_nms_boxes_grouped_f32 ----------------------------------------------------------------------------------------------------
def _grouped_call(groups, thr, use_labels, cap, fill):
    from millieye_amd import hip
    sizes = [len(g[0]) for g in groups]
    n, m = len(sizes), sum(sizes)
    boxes = _dev(np.concatenate([g[0] for g in groups], 0).reshape(-1, 4))
    scores = _dev(np.concatenate([g[1] for g in groups], 0))
    labels = _dev(np.concatenate([g[2] for g in groups], 0))
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    d_start = torch.from_numpy(starts).cuda()
    ws = _Workspace(n, cap, fill)
    keep_full, keep = _guarded(m, torch.int64)
    cnt_full, cnt = _guarded(n, torch.int32)
    hip.check(hip.lib().me_nms_boxes_grouped_f32(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr() if use_labels else None,
                                                 d_start.data_ptr(), n, m, cap, float(thr), keep.data_ptr(), cnt.data_ptr(),
                                                 ws.ptr, hip.stream_ptr()), "me_nms_boxes_grouped_f32")
    cand, fb = ws.counts()
    assert _intact(keep_full) and _intact(cnt_full) and ws.intact(), "guard words overwritten"
    counts, keep_h = cnt.cpu().tolist(), keep.cpu()
    kept = [keep_h[starts[g]:starts[g] + counts[g]] for g in range(n)]
    return kept, counts, cand, fb


def _check_groups(groups, thr, use_labels, cap, names=None):
    sizes = [len(g[0]) for g in groups]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    want = [torch.from_numpy(sh.oracle_keep(g[0], g[1], g[2] if use_labels else None, thr)) + int(starts[i])
            if sizes[i] else torch.empty((0,), dtype=torch.int64) for i, g in enumerate(groups)]
    model = [sh.dispatch(c, cap, cap) for c in sizes]
    for fill in FILLS:
        kept, counts, cand, fb = _grouped_call(groups, thr, use_labels, cap, fill)
        assert cand == sizes and fb == [int(d["fallback"]) for d in model], f"counts {cand}, fallback flags {fb}"
        for g in range(len(groups)):
            assert counts[g] == len(want[g]) and torch.equal(kept[g], want[g]), \
                f"group {g} ({names[g] if names else sizes[g]}) thr={thr} labels={use_labels} cap={cap} poison {fill:#x}: " \
                f"kept rows differ from the oracle ({counts[g]} vs {len(want[g])} kept)"
    return want


@pytest.mark.parametrize("cap", sorted(sh.GROUP_REGIMES))
def test_grouped_regimes_side_by_side(hip_lib, cap):
    """Empty, matrix-only, register, LDS-list and global-list groups in one call; with cap 5633 the scan of every group runs
    through its two LDS buffers."""
    assert tuple(sh.regime(c, cap, cap) for c in sh.GROUP_SIZES) == sh.GROUP_REGIMES[cap]
    groups = [sh.clustered(c, 300 + c) for c in sh.GROUP_SIZES]
    for use_labels in (True, False):
        want = _check_groups(groups, 0.5, use_labels, cap)
        assert all(len(w) < c for w, c in zip(want[1:], sh.GROUP_SIZES[1:]))


# ---- thresholds, ties, score and box edges ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_scenes():
    scenes = {f"equal_scores_{m}": sh.equal_scores(m) for m in (1500, 3000, 4200)}
    scenes["score_edges"] = sh.score_edges()
    scenes["nan_scores"] = sh.nan_scores()
    for k, v in sh.degenerate().items():
        scenes["degenerate_" + k] = v
    return scenes


@pytest.mark.parametrize("thr", sh.THRESHOLDS)
def test_ties_score_edges_and_degenerate_boxes(hip_lib, thr):
    """Equal scores across wave and thread-stripe boundaries (lower row first), +0 / -0, negative, subnormal and -inf scores,
    NaN scores of either sign and any payload (first, in row order), zero-area, inverted, huge, infinite, NaN and subnormal
    boxes - at the usual thresholds, at 0 and 1, and below 0 (nms_matrix_kernel's other branch)."""
    scenes = _edge_scenes()
    for name, scene in scenes.items():
        for use_labels in (True, False):
            _check_boxes(scene, thr, use_labels, name)
    names = list(scenes)
    for use_labels in (True, False):
        _check_groups([scenes[k] for k in names], thr, use_labels, 4200, names)


def test_signed_nan_scores_sort_first_in_row_order(hip_lib):
    """The scene of its own for NaN scores: +NaN, the sign-bit NaN (0xFFC00000, what 0 / 0 gives on x86) and two payloads in one
    cluster.  make_key gives every NaN the top key, so they lead the kept rows, the lower row first - like torch.sort(descending)
    in torchvision's nms (the oracle, whose comparator is undefined for NaN, gets +inf in those places)."""
    scene, r = sh.nan_scores(), sh.NAN_ROWS
    for use_labels in (True, False):
        want = _check_boxes(scene, 0.5, use_labels, "nan_scores")
        assert want[:3].tolist() == [r["plus"], r["sign"], r["payload_low_row"]] and r["payload_high_row"] not in want.tolist()
    _check_groups([sh.clustered(65, 1), scene, sh.clustered(130, 2)], 0.5, True, 240)


@pytest.mark.parametrize("thr", [0.5, 0.25])
def test_iou_exactly_at_the_threshold_is_kept(hip_lib, thr):
    """``ovr > thr`` is strict: pairs whose float32 IoU equals the threshold bit for bit keep both boxes, their neighbours one
    float32 step above lose one - with the label offsets (exact: integer coordinates) and without."""
    scene = sh.exact_threshold(thr)
    for use_labels in (True, False):
        _check_boxes(scene, thr, use_labels, "exact_threshold")
    for use_labels in (True, False):
        _check_groups([scene, sh.clustered(65, 3), scene], thr, use_labels, len(scene[0]))


def test_stream_tail_with_nan_scores_score_edges_and_an_lds_list_stream(hip_lib):
    """me_stream_tail_f32 shares make_key and the selection with the grouped call: a stream of NaN scores (either sign, two
    payloads), one of +0 / -0 / subnormal / -inf scores and one of 2500 rows (the fallback's LDS-list mode), interleaved,
    against the restated tail with the oracle's batched_nms (+inf in the NaN places)."""
    from millieye_amd import hip
    from millieye_amd.utils.utils import rescale_scalars
    from tests import stream_tail_refs as refs
    scenes = [sh.nan_scores(), sh.score_edges(), sh.clustered(2500, 77)]
    assert sh.regime(2500, sum(len(s[0]) for s in scenes), sum(len(s[0]) for s in scenes)) == "matrix/bulk -> fallback/lds"
    rows = np.concatenate([np.concatenate([np.full((len(b), 1), i, np.float32), b, sc[:, None], np.full((len(b), 1), 0.75, np.float32),
                                           lab[:, None]], 1) for i, (b, sc, lab) in enumerate(scenes)], 0).astype(np.float32)
    rows = rows[np.random.RandomState(5).permutation(len(rows))]
    hws = [(480, 640), (360, 480), (640, 480)]
    for_oracle = rows.copy()
    for_oracle[:, 5] = sh.oracle_scores(rows[:, 5])
    want = refs.tail_ref(for_oracle, 3, hws, 416, 0.5, nms=lambda b, sc, lab, iou: sh.oracle_keep(b, sc, lab, iou))
    got, in_counts = hip.stream_tail(torch.from_numpy(rows).cuda(), 3, rescale_scalars(416, hws).cuda(), 0.5)
    assert in_counts == [len(s[0]) for s in scenes]
    for s in range(3):
        g, w = got[s].numpy().copy(), want[s].copy()
        assert g.shape == w.shape and 0 < len(w) < in_counts[s], f"stream {s}"
        nan_rows = np.isposinf(w[:, 4])
        assert nan_rows.sum() == (3 if s == 0 else 0) and np.isnan(g[nan_rows, 4]).all(), f"stream {s}: the NaN rows lead"
        g[nan_rows, 4] = w[nan_rows, 4] = 0
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"stream {s}: differs from the restatement"


# ---- me_nms_batched_f32 ----------------------------------------------------------------------------------------------------------
def _batched_call(pred, max_det, thr, writeback, fill):
    """pred: CPU tensor [n, rows, 5 + nc] (left unchanged).  Returns (det CPU [n, max_det, 7 + nc], counts, cand, fallback, the
    device's prediction tensor after the call)."""
    from millieye_amd import hip
    n, rows, per = pred.shape
    dev = pred.clone().cuda()
    ws = _Workspace(n, rows, fill)
    det_full, det = _guarded(n * max_det * (per + 2), torch.float32)
    cnt_full, cnt = _guarded(n, torch.int32)
    d = hip.NmsDesc()
    d.pred, d.det, d.count, d.workspace = dev.data_ptr(), det.data_ptr(), cnt.data_ptr(), ws.ptr
    d.n, d.rows, d.num_classes, d.max_det = n, rows, per - 5, max_det
    d.conf_thresh, d.iou_thresh, d.writeback_xyxy = sh.CONF, thr, 1 if writeback else 0
    hip.check(hip.lib().me_nms_batched_f32(C.byref(d), hip.stream_ptr()), "me_nms_batched_f32")
    cand, fb = ws.counts()
    assert _intact(det_full) and _intact(cnt_full) and ws.intact(), "guard words overwritten"
    return det.cpu().view(n, max_det, per + 2), cnt.cpu().tolist(), cand, fb, dev.cpu()


def _check_batched(pred, ref, ref_pred, max_det, thr=0.5):
    """``ref``: the uncapped oracle rows per image (or None) - the capped list is its prefix; ``ref_pred``: the xyxy rows."""
    n, rows, _ = pred.shape
    eff = min(max_det, rows)
    model = []
    for i in range(n):
        r, boxes, scores, labels = sh.pred_candidates(pred[i].numpy())
        top = sh.top_winners(boxes, scores, labels, thr, eff) if len(r) > sh.MATN and eff <= sh.CONT_KEEP else None
        model.append(sh.dispatch(len(r), max_det, rows, top))
    for fill, writeback in zip(FILLS, (True, False)):
        det, counts, cand, fb, after = _batched_call(pred, max_det, thr, writeback, fill)
        assert cand == [d["cnt"] for d in model] and fb == [int(d["fallback"]) for d in model], \
            f"counts {cand}, fallback flags {fb}; the model says {model}"
        assert torch.equal(after, ref_pred if writeback else pred), "the in-place xywh -> xyxy write-back"
        for i in range(n):
            want = ref[i][:max_det] if ref[i] is not None else torch.empty((0, det.shape[2]))
            assert counts[i] == want.shape[0], f"image {i} max_det {max_det}: kept {counts[i]} vs oracle {want.shape[0]}"
            assert torch.equal(det[i, :counts[i]], want), f"image {i} max_det {max_det} poison {fill:#x}: kept rows differ"
    return model


@functools.lru_cache(maxsize=None)
def _batched_grid(n):
    counts = [sh.BATCHED_COUNTS[i % len(sh.BATCHED_COUNTS)] for i in range(n)]
    pred = torch.from_numpy(np.stack([sh.batched_image(c, 500 + 10 * i) for i, c in enumerate(counts)]))
    ref, ref_pred = _oracle_nms_cpp(pred, sh.CONF, 0.5, sh.BATCHED_ROWS)
    return counts, pred, ref, ref_pred


@pytest.mark.parametrize("max_det", sh.BATCHED_MAX_DET)
@pytest.mark.parametrize("n", [7, 17])  # nms_matrix_kernel: four waves per 64 x 64 item / one
def test_batched_counts_and_max_det(hip_lib, n, max_det):
    """One image per candidate count - 0, 1, 64 / 65, 1024 / 1025, every row - against max_det 1, 65 (the first candidate of
    the second block), 200, 1024 / 1025 (CONT_KEEP: the continuation / the fallback) and 2000 (clamped to the 1500 rows)."""
    counts, pred, ref, ref_pred = _batched_grid(n)
    model = _check_batched(pred, ref, ref_pred, max_det)
    assert [d["cnt"] for d in model] == counts
    assert any(d["fallback"] for d in model) == (max_det > sh.CONT_KEEP)
    assert max_det != sh.CONT_KEEP or any(d["continuation"] for d in model)


@functools.lru_cache(maxsize=None)
def _continuation_batch():
    scenes = sh.continuation_scenes()
    pred = torch.from_numpy(np.stack([sh.to_pred(scenes[k], 3200) for k in "abc"] + [sh.to_pred(sh.separated(300), 3200)]))
    ref, ref_pred = _oracle_nms_cpp(pred, sh.CONF, 0.5, 3200)
    return pred, ref, ref_pred


@pytest.mark.parametrize("max_det", [1, 65, 200])
def test_batched_continuation_edges_and_the_walk_that_stops_at_max_det(hip_lib, max_det):
    """The three continuation edges (at max_det 200: one winner missing behind the matrix; max_det reached in the middle of a
    continuation block; the list exhausted at a count that is no multiple of 64) and 300 boxes of which none is suppressed,
    where only max_det ends the walk - in the middle of a block (200), on a block's first candidate (65), at once (1)."""
    pred, ref, ref_pred = _continuation_batch()
    model = _check_batched(pred, ref, ref_pred, max_det)
    assert [d["continuation"] for d in model] == [max_det == sh.CONT_MAX_DET] * 3 + [False]
    assert ref[3].shape[0] == 300 and ref[2].shape[0] == 130


# ---- the environment switches ----------------------------------------------------------------------------------------------------
def switch_scenes():
    """The compact scene list of the switch test, run in this process: name -> CPU tensor."""
    out = {}
    flags = []
    for m in sh.SWITCH_BOXES:
        kept, cand, fb = _boxes_call(sh.clustered(m, 900 + m), 0.5, True, FILLS[0])
        out[f"boxes_{m}"] = kept
        flags += [cand, fb]
    kept, cand, fb = _boxes_call(sh.equal_scores(1500), 0.5, True, FILLS[1])
    out["ties"] = kept
    flags += [cand, fb]
    pred = _continuation_batch()[0][1:2]
    det, counts, cand, fb, _ = _batched_call(pred, sh.CONT_MAX_DET, 0.5, False, FILLS[0])
    out["continuation_b"] = det[0, :counts[0]].clone()
    out["flags"] = torch.tensor(flags + cand + fb)
    return out


def switch_scenes_to(path):
    torch.save(switch_scenes(), path)


def test_legacy_and_two_buffer_switches_equal_the_default(hip_lib, tmp_path):
    """MILLIEYE_NMS_LEGACY=1 (nms_select_kernel alone: its LDS-matrix mode up to 768 candidates, and the other three) and
    MILLIEYE_NMS_BULK=0 (the two-buffer scan at every size) are read once per process - hence the two child processes, one
    after the other; the second is not started when the first fails.  Both must give the default run's rows, bit for bit, and
    those are the oracle's."""
    default = switch_scenes()
    for m in sh.SWITCH_BOXES:
        scene = sh.clustered(m, 900 + m)
        assert torch.equal(default[f"boxes_{m}"], torch.from_numpy(sh.oracle_keep(*scene, 0.5))), m
    assert torch.equal(default["ties"], torch.from_numpy(sh.oracle_keep(*sh.equal_scores(1500), 0.5)))
    _, ref, _ = _continuation_batch()
    assert torch.equal(default["continuation_b"], ref[1][:sh.CONT_MAX_DET])
    sizes = list(sh.SWITCH_BOXES) + [1500]
    want_flags = [v for m in sizes for v in (m, int(m > sh.MATN))] + [int((_continuation_batch()[0][1, :, 4] >= sh.CONF).sum()), 0]
    assert default["flags"].tolist() == want_flags
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_nms_regimes as t; t.switch_scenes_to(sys.argv[1])" % root
    for var in ("MILLIEYE_NMS_LEGACY", "MILLIEYE_NMS_BULK"):
        path = str(tmp_path / f"{var}.pt")
        env = dict(os.environ, **{var: "1" if var.endswith("LEGACY") else "0"})
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=300)   # (raises: no second child)
        got = torch.load(path)
        assert got.keys() == default.keys()
        for k in default:
            if k == "flags" and var.endswith("LEGACY"):   # the matrix path is off: nothing sets a fallback flag
                assert got[k].tolist() == [v if i % 2 == 0 else 0 for i, v in enumerate(want_flags)], "the legacy switch was not on"
            else:
                assert torch.equal(got[k], default[k]), f"{var}: {k} differs from the default run"
