"""Scenes and a CPU model of the dispatch for the NMS of csrc/nms.hip (me_nms_boxes_f32, me_nms_boxes_grouped_f32,
me_nms_batched_f32): tests/test_nms_scenes_cpu.py guards them with the oracle alone, tests/test_gpu_nms_regimes.py runs them.

Pure numpy; no device import.  Every scene is ``(boxes xyxy float32 [m,4], scores float32 [m], labels float32 [m])`` and is
deterministic.  The model restates, from the constants of nms.hip, which route a list of ``cnt`` candidates takes."""
import numpy as np

# ---- the constants of csrc/nms.hip ---------------------------------------------------------------------------------------------
MATN = 1024            # sorted candidates per image the bit matrix covers
MAT_CANDS = 768        # nms_select_kernel: LDS bit matrix up to this many candidates
REG_CANDS = 2048       # ... register mode up to 2 * SEL_THREADS
LDS_CANDS = 4096       # ... candidate lists in LDS up to this many
CONT_KEEP = 1024       # nms_scan_kernel: the continuation serves max_det up to this
SCAN_LDS = 150 * 1024  # launch_matrix_path: the whole matrix in LDS (bulk) when matn * wc * 8 + keep_cap * 4 fits this
MAX_ROWS = 32768

F32 = np.float32


def _f(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def bits_to_f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def matn_of(cap):
    return min((cap + 63) & ~63, MATN)


def select_mode(cnt):
    """The mode nms_select_kernel takes for ``cnt`` candidates (it runs for fallback images, and for all under the legacy switch)."""
    if cnt <= MAT_CANDS:
        return "mat"
    if cnt <= REG_CANDS:
        return "reg"
    if cnt <= LDS_CANDS:
        return "lds"
    return "global"


def dispatch(cnt, max_det, cap, top=None):
    """The route of one list: ``cnt`` candidates in a workspace of ``cap`` rows per list, ``max_det`` as the entry point passes it
    (me_nms_boxes_f32: m; the grouped call and the tail: cap; me_nms_batched_f32: its max_det).  ``top``: the winners among the MATN
    best-keyed candidates alone, stopped at the effective max_det (needed only when cnt > MATN and max_det <= CONT_KEEP)."""
    assert 0 <= cnt <= cap <= MAX_ROWS
    matn = matn_of(cap)
    wc = matn // 64
    eff = min(max_det, cap)
    out = {"cnt": cnt, "max_det_eff": eff, "matn": matn, "wc": wc,
           "bulk": matn * wc * 8 + eff * 4 <= SCAN_LDS,
           "fallback": cnt > MATN and eff > CONT_KEEP,
           "continuation": False, "select_mode": select_mode(cnt)}
    if cnt > MATN and eff <= CONT_KEEP:
        assert top is not None, "the continuation depends on the winners among the MATN best"
        out["continuation"] = top < eff
    return out


def regime(cnt, max_det, cap, top=None):
    """A one-line name of :func:`dispatch`'s answer."""
    if cnt == 0:
        return "empty"
    d = dispatch(cnt, max_det, cap, top)
    scan = "bulk" if d["bulk"] else "two-buffer"
    if d["fallback"]:
        return f"matrix/{scan} -> fallback/{d['select_mode']}"
    return f"matrix/{scan}" + (" -> continuation" if d["continuation"] else "")


# ---- orders and plain references -------------------------------------------------------------------------------------------------
def key_order(scores):
    """The visiting order: NaN scores first (torch.sort, descending), then descending score with -0 == +0, ties to the lower row."""
    s = _f(scores).astype(np.float64)
    nan = np.isnan(s)
    s = np.where(nan, 0.0, s)
    return np.lexsort((np.arange(len(s)), -s, ~nan))


def oracle_scores(scores):
    """Scores for the oracle, whose comparator is undefined for NaN: +inf in the NaN places (the scene holds no +inf) - the same
    position in the order, lower row first among them."""
    s = _f(scores).copy()
    assert not np.isposinf(s).any() or not np.isnan(s).any()
    s[np.isnan(s)] = np.inf
    return s


def shifted(boxes, labels):
    """batched_nms's offset trick in float32: boxes + label * (boxes.max() + 1), NaN propagating like torch's max."""
    b = _f(boxes)
    if labels is None:
        return b
    with np.errstate(all="ignore"):
        mx = F32(np.nan) if np.isnan(b).any() else b.max()
        off = _f(labels) * (mx + F32(1))
        return (b + off[:, None]).astype(np.float32)


def iou_matrix(b):
    """(ovr, inter) of all pairs [i, j] in float32 with nms_cpu_kernel's operation order (std::max(a, b) = a < b ? b : a)."""
    b = _f(b)
    with np.errstate(all="ignore"):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        ix1, jx1 = b[:, None, 0], b[None, :, 0]
        iy1, jy1 = b[:, None, 1], b[None, :, 1]
        ix2, jx2 = b[:, None, 2], b[None, :, 2]
        iy2, jy2 = b[:, None, 3], b[None, :, 3]
        xx1 = np.where(ix1 < jx1, jx1, ix1)
        yy1 = np.where(iy1 < jy1, jy1, iy1)
        xx2 = np.where(jx2 < ix2, jx2, ix2)
        yy2 = np.where(jy2 < iy2, jy2, iy2)
        dw, dh = xx2 - xx1, yy2 - yy1
        w = np.where(F32(0) < dw, dw, F32(0)).astype(np.float32)
        h = np.where(F32(0) < dh, dh, F32(0)).astype(np.float32)
        inter = (w * h).astype(np.float32)
        ovr = inter / ((area[:, None] + area[None, :]).astype(np.float32) - inter)
    return ovr.astype(np.float32), inter


def greedy(boxes, order, thr, inclusive=False, max_det=None):
    """Plain greedy NMS over ``order`` (for the alternative rules the guards compare with; small scenes only)."""
    ovr, _ = iou_matrix(boxes)
    hit = (ovr >= F32(thr)) if inclusive else (ovr > F32(thr))
    dead = np.zeros(len(order), dtype=bool)
    keep = []
    for a in order:
        if dead[a]:
            continue
        keep.append(int(a))
        if max_det is not None and len(keep) >= max_det:
            break
        dead |= hit[a]
        dead[a] = True
    return np.asarray(keep, dtype=np.int64)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def clustered(m, seed, classes=4, span=600.0):
    """``m`` 60-pixel boxes in tight clusters (a cluster keeps one box per label, so the serial walk stays short), scores on a grid
    of 1 / 4096 (ties), ``classes`` labels."""
    g = np.random.RandomState(seed)
    centres = g.uniform(40, span, size=(min(max(m // 40, 3), 300), 2))
    which = g.randint(0, len(centres), size=m)
    c = centres[which] + g.uniform(-1.5, 1.5, size=(m, 2))
    wh = g.uniform(56, 64, size=(m, 2))
    boxes = _f(np.concatenate([c - wh / 2, c + wh / 2], 1))
    scores = _f(g.randint(256, 4096, size=m) / 4096.0)
    labels = _f(g.randint(0, classes, size=m))
    return boxes, scores, labels


def separated(m, classes=4):
    """``m`` 8-pixel boxes on a grid of 10: nothing overlaps, every box is kept - the walk must stop at max_det."""
    i = np.arange(m)
    x, y = (i % 64) * 10.0, (i // 64) * 10.0
    boxes = _f(np.stack([x, y, x + 8, y + 8], 1))
    g = np.random.RandomState(m)
    scores = _f(g.permutation(m) / float(m + 1) * 0.8 + 0.15)   # distinct, in row-scrambled order
    labels = _f(i % classes)
    return boxes, scores, labels


def equal_scores(m, seed=7):
    boxes, _, labels = clustered(m, seed)
    return boxes, np.full(m, 0.5, dtype=np.float32), labels


_EXACT_SHAPES = {
    # (box A, box B) with integer coordinates and IoU(A, B) == thr exactly; s scales both
    0.5: [((0, 0, 2, 1), (0, 0, 1, 1)), ((0, 0, 3, 1), (1, 0, 4, 1)), ((0, 0, 3, 2), (0, 0, 3, 1)), ((0, 0, 1, 2), (0, 1, 1, 2))],
    0.25: [((0, 0, 4, 1), (0, 0, 1, 1)), ((0, 0, 2, 1), (1, 0, 4, 1)), ((0, 0, 2, 2), (0, 0, 1, 1)), ((0, 0, 1, 4), (0, 3, 1, 4))],
}


# neighbours of those pairs one float32 step of IoU off the threshold: (shape, coordinate of the concatenated pair A | B, ulps to
# move it by) at x offset 0, where an ulp is small enough - found by search, guarded by tests/test_nms_scenes_cpu.py
_ULP_NEIGHBOURS = {
    0.5: [(0, 2, -2), (1, 6, -2), (0, 6, -1), (1, 4, 1), (2, 2, -1), (3, 6, -1)],     # two above, four below
    0.25: [(0, 2, -2), (0, 6, 1), (1, 4, -2), (0, 6, -1), (2, 6, -1), (3, 2, -1)],    # three above, three below
}


def exact_threshold(thr):
    """Pairs of small integer boxes, one pair per 8 x 8 cell of a 64 x 64 field, whose float32 IoU is exactly ``thr`` (the strict
    ``ovr > thr`` keeps both), in four labels (the maximum coordinate is 64, so label * (max + 1) shifts by multiples of 65 -
    exact); and, in label 0 in the cells of the column x = 0, neighbours of those pairs with one x coordinate moved by an ulp or
    two, whose IoU lands one float32 step above or below ``thr``.  In every pair the first box has the higher score; rows are
    scrambled."""
    shapes = _EXACT_SHAPES[thr]
    boxes, scores, labels = [], [], []

    def add(pair, lab):
        for q, box in enumerate(pair):
            boxes.append([float(v) for v in box])
            scores.append(0.9 - 0.001 * len(scores) if q == 0 else 0.4 - 0.001 * len(scores))
            labels.append(lab)

    cell = 0
    for lab in range(4):
        for k in range(12):
            a, b = shapes[(k + lab) % len(shapes)]
            s = 1 + (k % 2)   # scale 1 or 2: the pair stays inside its cell (extent <= 8)
            ox, oy = (1 + cell % 7) * 8, (cell // 7) * 8
            cell += 1
            add([(ox + s * box[0], oy + s * box[1], ox + s * box[2], oy + s * box[3]) for box in (a, b)], lab)
    for k, (shape, coord, ulps) in enumerate(_ULP_NEIGHBOURS[thr]):
        a, b = shapes[shape]
        pair = _f([a[0], 8 * k + a[1], a[2], 8 * k + a[3], b[0], 8 * k + b[1], b[2], 8 * k + b[3]])
        for _ in range(abs(ulps)):
            pair[coord] = np.nextafter(pair[coord], F32(np.inf) if ulps > 0 else F32(-np.inf))
        add([pair[:4], pair[4:]], 0)
    boxes.append([62, 62, 64, 64])   # the maximum is the integer 64: label * 65 shifts the integer pairs exactly
    scores.append(0.95)
    labels.append(3)
    boxes, scores, labels = _f(boxes), _f(scores), _f(labels)
    assert boxes.max() == 64
    perm = np.random.RandomState(11).permutation(len(boxes))
    return boxes[perm], scores[perm], labels[perm]


def score_edges(m=320, seed=21):
    """Clustered boxes whose scores are +0 / -0 (the lower row of an overlapping pair holds -0), negative, subnormal and -inf
    values next to ordinary ones."""
    boxes, scores, labels = clustered(m, seed, classes=2, span=300.0)
    g = np.random.RandomState(seed + 1)
    kinds = g.randint(0, 8, size=m)
    sub = bits_to_f32(g.randint(1, 0x7FFFFF, size=m))                # positive subnormals
    scores = np.where(kinds == 0, F32(0.0), scores)
    scores = np.where(kinds == 1, F32(-0.0), scores)
    scores = np.where(kinds == 2, -scores, scores)
    scores = np.where(kinds == 3, sub, scores)
    scores = np.where(kinds == 4, -sub, scores)
    scores = np.where(kinds == 5, F32(-np.inf), scores)
    scores = _f(scores)
    # one pinned pair: identical boxes far from the rest, -0 in the lower row, +0 in the higher one
    boxes[5] = boxes[200] = _f([900, 900, 960, 960])
    labels[5] = labels[200] = 0
    scores[5], scores[200] = F32(-0.0), F32(0.0)
    return boxes, scores, labels


NAN_ROWS = {"plus": 40, "sign": 90, "payload_low_row": 120, "payload_high_row": 160}


def nan_scores(m=240, seed=31):
    """Four NaN scores, no +inf: +NaN (0x7FC00000), the sign-bit NaN 0 / 0 gives on x86 (0xFFC00000), and two NaNs in ONE
    cluster whose payloads order them against their rows (the lower row holds the smaller payload).  Each NaN row shares its
    cluster and label with better-scored ordinary rows, so its place in the order shows in the kept set."""
    boxes, scores, labels = clustered(m, seed, classes=2, span=300.0)
    scores = scores.copy()
    r = NAN_ROWS
    far = [(1000, 1000), (1200, 1000), (1400, 1000)]
    for (cx, cy), rows in zip(far, ([r["plus"], 41, 42], [r["sign"], 91, 12], [r["payload_low_row"], r["payload_high_row"], 13])):
        for k, row in enumerate(rows):
            boxes[row] = _f([cx - 30 + k, cy - 30, cx + 30 + k, cy + 30])
            labels[row] = 1
    scores[r["plus"]] = bits_to_f32(0x7FC00000)
    scores[r["sign"]] = bits_to_f32(0xFFC00000)
    scores[r["payload_low_row"]] = bits_to_f32(0x7FC00001)
    scores[r["payload_high_row"]] = bits_to_f32(0x7FD00000)
    return boxes, scores, labels


def degenerate():
    """Four scenes, by name (a huge, infinite or NaN coordinate changes the label offsets of the whole list, so each has a scene
    of its own):
    ``plain``  zero-area boxes (identical ones included: 0 / 0), boxes inverted in x or y, and clusters at scale 1e-20 whose areas
               and intersections are subnormal, among ordinary clusters;
    ``huge``   the same plus coordinates of magnitude 1e30 (areas overflow to inf);
    ``inf``    the same plus one +inf and one -inf coordinate (the maximum is inf: label 0 shifts by 0 * inf = NaN);
    ``nan``    the same plus one NaN coordinate."""
    boxes, scores, labels = clustered(200, 51, classes=3, span=300.0)
    boxes, scores = boxes.copy(), scores.copy()
    g = np.random.RandomState(52)
    for r in range(0, 24, 3):                       # zero area: points and lines, identical pairs (rows r and r + 1)
        p = boxes[r + 100, :2]
        boxes[r] = boxes[r + 1] = _f([p[0], p[1], p[0], p[1]])
        boxes[r + 2] = _f([p[0], p[1], p[0] + 30, p[1]])
        labels[r] = labels[r + 1] = labels[r + 2] = labels[r + 100]
    for r in range(24, 40):                         # inverted in x (even rows) or y (odd rows)
        c = 0 if r % 2 == 0 else 1
        boxes[r, c], boxes[r, c + 2] = boxes[r, c + 2], boxes[r, c]
    origin = g.randint(0, 3, size=(40, 1)) * 8.0 + g.uniform(0, 1.0, size=(40, 2))   # three clusters
    boxes[40:80] = _f(np.concatenate([origin, origin + g.uniform(0.5, 6, size=(40, 2))], 1) * 1e-20)
    labels[40:80] = 0
    out = {"plain": (boxes, scores, labels)}
    huge = boxes.copy()
    huge[80] = _f([-1e30, -1e30, 1e30, 1e30])
    huge[81] = _f([1e30, 1e30, 2e30, 2e30])
    huge[82] = _f([-1e30, 10, 1e30, 70])
    out["huge"] = (huge, scores, labels)
    inf = boxes.copy()
    inf[80, 2] = np.inf
    inf[81, 0] = -np.inf
    out["inf"] = (inf, scores, labels)
    nan = boxes.copy()
    nan[80, 1] = np.nan
    out["nan"] = (nan, scores, labels)
    return out


# ---- batched scenes: prediction tensors ----------------------------------------------------------------------------------------
CONF = 0.05   # the confidence threshold of every batched scene; rows that are no candidates hold 0.01


def to_pred(scene, rows, nc=4, seed=0):
    """One image of a prediction tensor ``[rows, 5 + nc]`` (xywh, objectness, class scores) holding the scene's boxes as its
    candidates, scattered over the rows in a fixed scramble; the class maximum sits at the box's label.  The device and the oracle
    both convert xywh back to xyxy, so the candidates' boxes are those conversions, not the scene's bits."""
    boxes, scores, labels = scene
    m = len(boxes)
    assert m <= rows and (m == 0 or (np.asarray(scores) >= CONF).all())
    g = np.random.RandomState(seed + rows)
    pred = np.zeros((rows, 5 + nc), dtype=np.float32)
    pred[:, 0:2] = g.uniform(0, 400, size=(rows, 2))
    pred[:, 2:4] = g.uniform(8, 60, size=(rows, 2))
    pred[:, 4] = 0.01
    pred[:, 5:] = g.uniform(0, 0.5, size=(rows, nc))
    at = np.sort(g.permutation(rows)[:m])
    b = np.asarray(boxes, dtype=np.float64)
    pred[at, 0], pred[at, 1] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    pred[at, 2], pred[at, 3] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    pred[at, 4] = scores
    pred[at, 5 + np.asarray(labels, dtype=np.int64) % nc] = 0.9
    return pred


def pred_candidates(pred):
    """The candidates of one image as the kernel lists them: (rows, boxes xyxy float32 with the half extents as w / 2, scores,
    labels = first class maximum)."""
    p = _f(pred)
    rows = np.nonzero(p[:, 4] >= F32(CONF))[0]
    c = p[rows]
    boxes = np.stack([c[:, 0] - c[:, 2] / 2, c[:, 1] - c[:, 3] / 2, c[:, 0] + c[:, 2] / 2, c[:, 1] + c[:, 3] / 2], 1)
    return rows, _f(boxes), c[:, 4].copy(), _f(np.argmax(c[:, 5:], 1))


def sequence_scene(ids, seed, classes=4):
    """Candidates in descending score order: position p is a 60-pixel box of cluster ``ids[p]`` (clusters sit on a grid of 100,
    members differ by at most a pixel: IoU > 0.9 inside a cluster, 0 between clusters, one label per cluster), so the kept
    boxes are the first members of the distinct clusters.  Returned in a scrambled row order."""
    ids = np.asarray(ids, dtype=np.int64)
    m = len(ids)
    g = np.random.RandomState(seed)
    c = np.stack([(ids % 20) * 100.0 + 50, (ids // 20) * 100.0 + 50], 1) + g.randint(-1, 2, size=(m, 2)) * 0.5
    boxes = _f(np.concatenate([c - 30, c + 30], 1))
    scores = _f(0.98 - np.arange(m) * 2.0e-4)
    labels = _f(ids % classes)
    perm = g.permutation(m)
    return boxes[perm], scores[perm], labels[perm]


CONT_MAX_DET = 200


def continuation_scenes():
    """The three edges of nms_scan_kernel's continuation at max_det = 200, as cluster-id sequences (see :func:`sequence_scene`):
    ``a``  199 = max_det - 1 winners among the 1024 best; the 200th is the 71st candidate behind them (block 17, lane 6), after
           70 members of earlier winners' clusters;
    ``b``  150 winners among the 1024 best; behind them every third candidate opens a new cluster, the others repeat an earlier
           or the just-opened one: the 200th winner falls in the middle of a continuation block, the uncapped list is longer;
    ``c``  100 winners among the 1024 best, 30 new clusters behind them, 3001 candidates (3001 % 64 = 57): the walk runs off
           the end of the list with 130 < max_det winners, the last candidate being one of them."""
    out = {}
    head = np.arange(MATN) % 199
    tail = np.concatenate([np.arange(70) % 199, [199], 200 + np.arange(2100) % 190])
    out["a"] = sequence_scene(np.concatenate([head, tail]), 61)
    head = np.arange(MATN) % 150
    p = np.arange(2100)
    new = 150 + p // 3
    g = np.random.RandomState(62)
    rep = np.where(p % 3 == 1, new, g.randint(0, 150, size=len(p)))   # the cluster opened just before / an old one
    tail = np.where(p % 3 == 0, new, rep)
    out["b"] = sequence_scene(np.concatenate([head, tail]), 63)
    head = np.arange(MATN) % 100
    tail = np.arange(1977) % 100
    at = np.linspace(5, 1976, 30).astype(np.int64)
    tail[at] = 100 + np.arange(30)
    out["c"] = sequence_scene(np.concatenate([head, tail]), 64)
    return out


# ---- the sizes the device tests run, with the regime each is there for -----------------------------------------------------------
BOXES_REGIMES = {   # me_nms_boxes_f32 on m boxes: cnt = max_det = cap = m
    1: "matrix/bulk", 63: "matrix/bulk", 64: "matrix/bulk", 65: "matrix/bulk", 129: "matrix/bulk", 767: "matrix/bulk",
    768: "matrix/bulk", 769: "matrix/bulk", 1023: "matrix/bulk", 1024: "matrix/bulk",
    1025: "matrix/bulk -> fallback/reg", 2048: "matrix/bulk -> fallback/reg",
    2049: "matrix/bulk -> fallback/lds", 3000: "matrix/bulk -> fallback/lds", 4096: "matrix/bulk -> fallback/lds",
    4097: "matrix/bulk -> fallback/global", 5632: "matrix/bulk -> fallback/global",
    5633: "matrix/two-buffer -> fallback/global", 32768: "matrix/two-buffer -> fallback/global",
}
GROUP_SIZES = (0, 65, 769, 1025, 2049, 3000, 4097)
GROUP_REGIMES = {   # me_nms_boxes_grouped_f32: max_det = cap for every group
    4097: ("empty", "matrix/bulk", "matrix/bulk", "matrix/bulk -> fallback/reg", "matrix/bulk -> fallback/lds",
           "matrix/bulk -> fallback/lds", "matrix/bulk -> fallback/global"),
    5633: ("empty", "matrix/two-buffer", "matrix/two-buffer", "matrix/two-buffer -> fallback/reg",
           "matrix/two-buffer -> fallback/lds", "matrix/two-buffer -> fallback/lds", "matrix/two-buffer -> fallback/global"),
}
BATCHED_ROWS = 1500
BATCHED_COUNTS = (0, 1, 64, 65, 1024, 1025, 1500)
BATCHED_MAX_DET = (1, 65, 200, 1024, 1025, 2000)
SWITCH_BOXES = (1, 64, 65, 128, 129, 768, 769, 2048, 2049, 4096, 4097)   # the sizes of the environment-switch runs
THRESHOLDS = (0.5, 0.25, 0.0, 1.0, -1.0)


def oracle_keep(boxes, scores, labels, thr):
    """The oracle's nms / batched_nms (oracle/tv_ops.c) on numpy arrays; NaN scores as :func:`oracle_scores` gives them."""
    import torch
    from oracle import tv_ops
    b, s = torch.from_numpy(_f(boxes)), torch.from_numpy(oracle_scores(scores))
    if labels is None:
        return tv_ops.nms(b, s, thr).numpy()
    return tv_ops.batched_nms(b, s, torch.from_numpy(_f(labels)), thr).numpy()


def top_winners(boxes, scores, labels, thr, eff):
    """The model's ``top``: the winners among the MATN best-keyed candidates alone, stopped at ``eff`` (a greedy prefix equals
    the NMS of the prefix; the label offsets come from the whole list's maximum)."""
    first = key_order(scores)[:MATN]
    kept = oracle_keep(shifted(boxes, labels)[first], _f(scores)[first], None, thr)
    return min(len(kept), eff)


def batched_image(cnt, seed, rows=BATCHED_ROWS):
    """One image of ``rows`` rows with exactly ``cnt`` clustered candidates."""
    boxes, scores, labels = clustered(cnt, seed) if cnt else (np.zeros((0, 4), np.float32), np.zeros(0, np.float32),
                                                              np.zeros(0, np.float32))
    return to_pred((boxes, scores, labels), rows, seed=seed)
