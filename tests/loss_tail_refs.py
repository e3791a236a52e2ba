"""Plain numpy references and the shared cases for csrc/yolo_loss.hip, csrc/evaltail.hip and csrc/optim.hip (no torch ops; a
python loop wherever the reference code loops).  Pinned by tests/test_loss_tail_refs_cpu.py to the oracle's torch restatement
(``oracle/darknet_ref.py:yolo_loss_terms``), to the host ``get_batch_statistics`` and to ``torch.optim.Adam`` / ``AdamW``; used by
tests/test_gpu_loss_tail.py as what the kernels must compute.

* ``yolo_loss_fwd_ref``      build_targets + the six loss terms + the metrics of one detection scale, in ``dtype``: float64 is the
                             reference, float32 (every element-wise operation rounded to fp32, sums in double like the kernel) is
                             the yardstick of the rounding error.
* ``batch_statistics_ref``   the greedy true-positive assignment in float32, one rounding per operation.
* ``adam_step_ref``          one Adam / AdamW step in float32, one rounding per operation, in the order csrc/optim.hip lists.
"""
import functools

import numpy as np

U = 2.0 ** -24
MARGIN = 1e-4    # every decision of a yolo case clears its threshold by this much (relative), the planted exact ties apart
SCALARS = ("loss", "x", "y", "w", "h", "conf", "cls", "cls_acc", "recall50", "recall75", "precision", "conf_obj", "conf_noobj")
DENSE = ("obj", "noobj", "tx", "ty", "tw", "th", "tcls", "tconf", "class_mask", "iou_scores")


# ---------------------------------------------------------------------------------------------------------------------
# YOLO loss forward
# ---------------------------------------------------------------------------------------------------------------------
def _exp(x):
    """exp rounded once to x's type (fp32: evaluated in double and rounded, so the float32 form does not inherit the last-bit
    habits of one library's expf)."""
    with np.errstate(over="ignore"):
        return np.exp(np.asarray(x, np.float64)).astype(x.dtype)


def _log(x):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(x, np.float64)).astype(x.dtype)


def _sig(x):
    one = x.dtype.type(1)
    return one / (one + _exp(-x))


def _bce(p, t):
    """nn.BCELoss element: both logs clamped at -100."""
    one, lo = p.dtype.type(1), p.dtype.type(-100)
    lp, lq = np.maximum(_log(p), lo), np.maximum(_log(one - p), lo)
    return -(t * lp + (one - t) * lq)


def _anchor_ious(anc, gw, gh):
    """bbox_wh_iou of every anchor with one target shape."""
    inter = np.minimum(anc[:, 0], gw) * np.minimum(anc[:, 1], gh)
    return inter / ((anc[:, 0] * anc[:, 1] + anc.dtype.type(1e-16)) + gw * gh - inter)


def _pred_iou(r, anc_wh, gi, gj, gx, gy, gw, gh):
    """bbox_iou(pred_box, target_box, x1y1x2y2=False) of one cell's decoded prediction, boxes in grid units (+1 convention)."""
    D = r.dtype.type
    one, two, zero = D(1), D(2), D(0)
    with np.errstate(over="ignore", invalid="ignore"):
        sx, sy = _sig(r[0:2])
        px, py = sx + D(gi), sy + D(gj)
        pw, ph = _exp(r[2])[()] * anc_wh[0], _exp(r[3])[()] * anc_wh[1]
        b1x1, b1x2, b1y1, b1y2 = px - pw / two, px + pw / two, py - ph / two, py + ph / two
        b2x1, b2x2, b2y1, b2y2 = gx - gw / two, gx + gw / two, gy - gh / two, gy + gh / two
        inter = max(min(b1x2, b2x2) - max(b1x1, b2x1) + one, zero) * max(min(b1y2, b2y2) - max(b1y1, b2y1) + one, zero)
        a1, a2 = (b1x2 - b1x1 + one) * (b1y2 - b1y1 + one), (b2x2 - b2x1 + one) * (b2y2 - b2y1 + one)
        return inter / (a1 + a2 - inter + D(1e-16))


def yolo_loss_fwd_ref(raw, anchors_scaled, nc, targets, ignore, obj_scale, noobj_scale, dtype):
    """``raw`` [N, G, G, A*(5+C)] fp32, ``anchors_scaled`` [A, 2] fp32 in grid units, ``targets`` [m, 6] fp32 (image, class, cx,
    cy, w, h in [0, 1]).  The fp32 inputs are used as given; ``target * G`` is formed in fp32 (as the kernel and the reference
    project form it) and only then widened to ``dtype``.  One loop over the targets in order: a later target overwrites the
    scalar targets of an earlier one with the same owner (image, anchor, cell), tcls accumulates the labels.  Then one pass over
    the cells.  A target outside the grid or the batch, or a label outside the classes, sets ``bad`` (the reference raises).
    Returns a dict: the dense tensors [N, A, G, G(, C)], ``n_obj`` / ``n_noobj``, ``scalars`` (the 13 of SCALARS, float64 array
    holding ``dtype`` values), ``counts`` (the integer sums behind the four ratio metrics), ``winner`` (row index per target: the
    row whose scalar targets its owner cell holds, -1 for a row outside the grid), ``owner`` (b, anchor, gj, gi per target)."""
    D = np.dtype(dtype).type
    raw = np.asarray(raw, np.float32)
    n, g = raw.shape[0], raw.shape[1]
    anc = np.asarray(anchors_scaled, np.float32).reshape(-1, 2).astype(D)
    na, per = len(anc), nc + 5
    pred = raw.reshape(n, g, g, na, per).transpose(0, 3, 1, 2, 4).astype(D)
    tg = np.asarray(targets, np.float32).reshape(-1, 6)
    tb = (tg[:, 2:6] * np.float32(g)).astype(D)
    cells = (n, na, g, g)
    obj, noobj = np.zeros(cells, bool), np.ones(cells, bool)
    tx, ty, tw, th, class_mask, iou_scores = (np.zeros(cells, D) for _ in range(6))
    tcls = np.zeros(cells + (nc,), D)
    held = np.full(cells, -1, np.int64)
    owner = np.full((len(tg), 4), -1, np.int64)
    bad = 0
    eps = D(1e-16)
    for k in range(len(tg)):
        b, label = int(tg[k, 0]), int(tg[k, 1])
        gx, gy, gw, gh = tb[k]
        gi, gj = int(gx), int(gy)   # .long(): truncation
        if not (0 <= b < n and 0 <= gi < g and 0 <= gj < g):
            bad = 1
            continue
        ious = _anchor_ious(anc, gw, gh)
        best = int(np.argmax(ious))   # first maximum
        at = (b, best, gj, gi)
        owner[k] = at
        obj[at], noobj[at] = True, False
        noobj[b, ious > D(ignore), gj, gi] = False
        if 0 <= label < nc:
            tcls[at + (label,)] = 1
        else:
            bad = 1
        tx[at], ty[at] = gx - np.floor(gx), gy - np.floor(gy)
        tw[at], th[at] = _log(gw / anc[best, 0] + eps), _log(gh / anc[best, 1] + eps)
        r = pred[at]
        class_mask[at] = 1 if int(np.argmax(_sig(r[5:]))) == label else 0
        iou_scores[at] = _pred_iou(r, anc[best], gi, gj, gx, gy, gw, gh)
        held[at] = k
    winner = np.array([held[tuple(o)] if o[0] >= 0 else -1 for o in owner], np.int64)
    # the pass over the cells
    pc = _sig(pred[..., 4])
    tconf = obj.astype(D)
    f64 = np.float64
    dx, dy = _sig(pred[..., 0])[obj] - tx[obj], _sig(pred[..., 1])[obj] - ty[obj]
    dw, dh = pred[..., 2][obj] - tw[obj], pred[..., 3][obj] - th[obj]
    sums = dict(x=(dx * dx).sum(dtype=f64), y=(dy * dy).sum(dtype=f64), w=(dw * dw).sum(dtype=f64), h=(dh * dh).sum(dtype=f64),
                cobj=_bce(pc[obj], D(1)).sum(dtype=f64), cnoobj=_bce(pc[noobj], D(0)).sum(dtype=f64),
                cls=_bce(_sig(pred[..., 5:][obj]), tcls[obj]).sum(dtype=f64),
                confobj=pc[obj].sum(dtype=f64), confnoobj=pc[noobj].sum(dtype=f64))
    n_obj, n_noobj = int(obj.sum()), int(noobj.sum())
    conf50 = pc > D(0.5)
    detected = conf50 & (class_mask == 1) & obj
    counts = dict(clsmask=int((class_mask[obj] == 1).sum()), r50=int((detected & (iou_scores > D(0.5))).sum()),
                  r75=int((detected & (iou_scores > D(0.75))).sum()), conf50=int(conf50.sum()))
    with np.errstate(invalid="ignore", divide="ignore"):
        no, nn = D(n_obj), D(n_noobj)
        lx, ly, lw, lh = D(sums["x"]) / no, D(sums["y"]) / no, D(sums["w"]) / no, D(sums["h"]) / no
        lconf = D(obj_scale) * (D(sums["cobj"]) / no) + D(noobj_scale) * (D(sums["cnoobj"]) / nn)
        lcls = D(sums["cls"]) / (no * D(nc))
        loss = ((((lx + ly) + lw) + lh) + lconf) + lcls
        scalars = [loss, lx, ly, lw, lh, lconf, lcls, D(100) * (D(counts["clsmask"]) / no), D(counts["r50"]) / (no + eps),
                   D(counts["r75"]) / (no + eps), D(counts["r50"]) / (D(counts["conf50"]) + eps), D(sums["confobj"]) / no,
                   D(sums["confnoobj"]) / nn]
    return dict(obj=obj.astype(np.uint8), noobj=noobj.astype(np.uint8), tx=tx, ty=ty, tw=tw, th=th, tcls=tcls, tconf=tconf,
                class_mask=class_mask, iou_scores=iou_scores, n_obj=n_obj, n_noobj=n_noobj,
                scalars=np.array([float(s) for s in scalars], np.float64), counts=counts, bad=bad, winner=winner, owner=owner)


def ratio_metrics32(ref):
    """cls_acc, recall50, recall75, precision formed in fp32 from a reference's integer counts."""
    f, c = np.float32, ref["counts"]
    with np.errstate(invalid="ignore", divide="ignore"):
        no = f(ref["n_obj"])
        return [f(100) * (f(c["clsmask"]) / no), f(c["r50"]) / (no + f(1e-16)), f(c["r75"]) / (no + f(1e-16)),
                f(c["r50"]) / (f(c["conf50"]) + f(1e-16))]


def yolo_input_violations(raw, anchors_scaled, nc, targets, ignore, planted=()):
    """The condition on a case's inputs, from float64 alone: every decision the kernel takes clears its threshold by MARGIN
    (relative) - the best anchor against the runner-up, each anchor IoU against ``ignore``, the class argmax against the
    runner-up, the objectness of every cell against 0.5, iou_scores against 0.5 and 0.75, the cell index against the cell borders.
    ``planted`` names the exact ties a case plants on purpose: ("anchor", row), ("ignore", row), ("class", row) or ("class",
    "all"), ("conf", (b, anchor, gj, gi)), ("iou", row), ("cell", row).  Returns the list of everything else that is too close."""
    D = np.float64
    planted = set(planted)
    raw = np.asarray(raw, np.float32)
    n, g = raw.shape[0], raw.shape[1]
    anc = np.asarray(anchors_scaled, np.float32).reshape(-1, 2).astype(D)
    na, per = len(anc), nc + 5
    pred = raw.reshape(n, g, g, na, per).transpose(0, 3, 1, 2, 4).astype(D)
    tg = np.asarray(targets, np.float32).reshape(-1, 6)
    tb = (tg[:, 2:6] * np.float32(g)).astype(D)
    out = []
    for k in range(len(tg)):
        gx, gy, gw, gh = tb[k]
        b, label, gi, gj = int(tg[k, 0]), int(tg[k, 1]), int(gx), int(gy)
        for v in (gx, gy):
            if abs(v - np.round(v)) <= MARGIN * max(1.0, abs(v)) and ("cell", k) not in planted:
                out.append(("cell", k))
        if not (0 <= b < n and 0 <= gi < g and 0 <= gj < g):
            continue
        ious = _anchor_ious(anc, gw, gh)
        order = np.sort(ious)[::-1]
        if na > 1 and order[0] - order[1] <= MARGIN * order[0] and ("anchor", k) not in planted:
            out.append(("anchor", k))
        if (np.abs(ious - ignore) <= MARGIN * ignore).any() and ("ignore", k) not in planted:
            out.append(("ignore", k))
        best = int(np.argmax(ious))
        r = pred[b, best, gj, gi]
        p = np.sort(_sig(r[5:]))[::-1]
        if nc > 1 and p[0] - p[1] <= MARGIN * p[0] and ("class", k) not in planted and ("class", "all") not in planted:
            out.append(("class", k))
        iou = _pred_iou(r, anc[best], gi, gj, gx, gy, gw, gh)
        if (abs(iou - 0.5) <= MARGIN * 0.5 or abs(iou - 0.75) <= MARGIN * 0.75) and ("iou", k) not in planted:
            out.append(("iou", k))
    pc = _sig(pred[..., 4])
    for at in np.argwhere(np.abs(pc - 0.5) <= MARGIN * 0.5):
        if ("conf", tuple(int(v) for v in at)) not in planted:
            out.append(("conf", tuple(int(v) for v in at)))
    return out


ANCHORS3 = (np.array([(10, 13), (33, 23), (62, 45)], np.float32) / np.float32(32)).astype(np.float32)


def _wide_anchors():
    """16 shapes in grid units; anchors 2 and 9 are the same (and the smallest) shape."""
    a = []
    for j in range(14):
        s = 2.0 * 1.23 ** j
        a.append(((s * 1.3, s / 1.3), (s, s), (s / 1.3, s * 1.3))[j % 3])
    a.insert(2, (1.25, 1.25))
    a.insert(9, (1.25, 1.25))
    return np.array(a, np.float32)


def legacy_yolo_case(n, g, nc, m):
    """The inputs of tests/test_gpu_darknet.py:test_yolo_loss_kernel_vs_the_torch_restatement."""
    rng = np.random.RandomState(100 * g + m)
    raw = rng.normal(0, 1.5, (n, g, g, 3 * (5 + nc))).astype(np.float32)
    tg = np.zeros((m, 6), np.float32)
    if m:
        tg[:, 0] = rng.randint(0, n, m)
        tg[:, 1] = rng.randint(0, nc, m)
        tg[:, 2:4] = rng.uniform(0.02, 0.98, (m, 2))
        tg[:, 4:6] = rng.uniform(0.03, 0.5, (m, 2))
    if m >= 9:
        tg[3] = tg[1]
        tg[3, 1] = (tg[1, 1] + 1) % nc
        tg[3, 2] += 0.2 / g
        tg[5, 2:4] = (np.floor(tg[5, 2:4] * g) + 0.0) / g
    return dict(raw=raw, anchors=ANCHORS3, n=n, g=g, na=3, nc=nc, targets=tg, planted=())


LEGACY = ((2, 13, 12, 9), (3, 26, 80, 40), (1, 7, 3, 1), (2, 10, 12, 0))
# case: n, g, na, nc, m, seed (chosen so that yolo_input_violations is empty)
YOLO_SHAPES = {"min": (1, 1, 1, 1, 1, 1), "base": (2, 13, 3, 12, 9, 1), "base16": (2, 16, 3, 12, 9, 1), "base64": (2, 64, 3, 12, 9, 1),
               "mid": (3, 26, 3, 80, 40, 2), "wide": (1, 65, 16, 16, 300, 1), "empty": (2, 10, 3, 12, 0, 1), "sat": (2, 13, 3, 12, 9, 1)}
# the planted rows (all in image 0): role -> rows, cell (gi, gj), anchor the target's shape is cut to
PAIR, CELLMATES, CLASS_TIE, THRESH, NEG, LAST = (1, 3), (4, 5), (6, 7), 8, 0, 2
PAIR2, TRIPLE, TIE_HI, TIE_LO = (255, 256), (10, 200, 290), 11, 12


def _place(tg, k, g, anchors, cell, frac, an, fw, fh, label=None):
    tg[k, 0] = 0
    tg[k, 2], tg[k, 3] = (cell[0] + frac[0]) / g, (cell[1] + frac[1]) / g
    tg[k, 4], tg[k, 5] = anchors[an, 0] * fw / g, anchors[an, 1] * fh / g
    if label is not None:
        tg[k, 1] = label


def _owner_cell(case, k):
    """(image, best anchor, gj, gi) of target row ``k``."""
    row = case["targets"][k]
    tb = (row[2:6] * np.float32(case["g"])).astype(np.float64)
    best = int(np.argmax(_anchor_ious(case["anchors"].astype(np.float64), tb[2], tb[3])))
    return int(row[0]), best, int(tb[1]), int(tb[0])


@functools.lru_cache(maxsize=None)
def yolo_case(name):
    n, g, na, nc, m, seed = YOLO_SHAPES[name]
    rng = np.random.RandomState(seed)
    per = nc + 5
    anchors = {1: np.array([(0.8, 0.9)], np.float32), 3: ANCHORS3 * np.float32(g / 13.0), 16: _wide_anchors()}[na]
    raw = rng.normal(0, 1.5, (n, g, g, na, per)).astype(np.float32)
    raw[..., 4] += np.where(raw[..., 4] >= 0, 0.01, -0.01).astype(np.float32)   # objectness clear of the 0.5 threshold
    tg = np.zeros((m, 6), np.float32)
    if m:
        tg[:, 0] = rng.randint(0, n, m)
        tg[:, 1] = rng.randint(0, nc, m)
        tg[:, 2:4] = (rng.randint(0, g, (m, 2)) + rng.uniform(0.05, 0.95, (m, 2))) / g   # centres clear of the cell borders
        tg[:, 4:6] = rng.uniform(0.03, 0.5, (m, 2))
    planted = []
    case = dict(raw=None, anchors=anchors, n=n, g=g, na=na, nc=nc, targets=tg, planted=None, background=None)
    if name == "min":
        tg[0] = (0, 0, 0.4, 0.6, 0.5, 0.7)
    if m >= 9:
        a_lo, a_mid, a_hi = (0, 1, 2) if na == 3 else (5, 8, 12)
        # same owner: the later row wins the scalar targets, tcls keeps both labels
        _place(tg, PAIR[0], g, anchors, (3, 4), (0.3, 0.4), a_mid, 1.1, 0.9, label=2)
        _place(tg, PAIR[1], g, anchors, (3, 4), (0.55, 0.35), a_mid, 1.13, 0.88, label=3)
        # same cell, different best anchor
        _place(tg, CELLMATES[0], g, anchors, (7, 2), (0.4, 0.6), a_lo, 1.1, 0.9)
        _place(tg, CELLMATES[1], g, anchors, (7, 2), (0.6, 0.4), a_hi, 0.9, 1.1)
        # class ties: the owner cell's two highest class logits are equal (classes 4 and 7)
        _place(tg, CLASS_TIE[0], g, anchors, (9, 9), (0.5, 0.5), a_mid, 0.9, 1.1, label=4)
        _place(tg, CLASS_TIE[1], g, anchors, (1, 8), (0.5, 0.5), a_mid, 0.9, 1.1, label=7)
        _place(tg, THRESH, g, anchors, (5, 11), (0.3, 0.7), a_lo, 1.1, 0.9)
        # cx = -0.3 / g truncates to cell 0; cy * g an integer (exactly, where g is a power of two)
        _place(tg, NEG, g, anchors, (0, 5), (0.0, 0.0), a_hi, 0.9, 1.1)
        tg[NEG, 2] = -0.3 / g
        # cx = 1 - 2^-24: the last cell
        _place(tg, LAST, g, anchors, (0, 6), (0.0, 0.4), a_mid, 1.1, 0.9)
        tg[LAST, 2] = np.float32(1) - np.float32(2.0 ** -24)
        planted += [("cell", NEG), ("cell", LAST)]
    if name == "wide":
        _place(tg, PAIR2[0], g, anchors, (50, 50), (0.3, 0.4), a_mid, 1.1, 0.9, label=5)
        _place(tg, PAIR2[1], g, anchors, (50, 50), (0.6, 0.3), a_mid, 1.14, 0.87, label=6)
        for i, k in enumerate(TRIPLE):
            _place(tg, k, g, anchors, (33, 60), (0.3 + 0.1 * i, 0.4), a_hi, 1.1 + 0.02 * i, 0.9, label=1 + i)
        # anchors 2 and 9 have the same shape: the first one owns the target; anchor 9's cell is ignored (IoU 0.87) ...
        _place(tg, TIE_HI, g, anchors, (20, 30), (0.5, 0.5), 2, 1.05, 0.92)
        # ... or stays background (a tiny target: IoU 0.16 with the smallest shape)
        _place(tg, TIE_LO, g, anchors, (40, 12), (0.5, 0.5), 2, 0.4, 0.4)
        planted += [("anchor", TIE_HI), ("anchor", TIE_LO)]
    case["raw"] = raw
    if m >= 9:
        for k in CLASS_TIE:
            b, best, gj, gi = _owner_cell(case, k)
            cl = raw[b, gj, gi, best, 5:]
            np.minimum(cl, np.float32(3), out=cl)
            cl[4] = cl[7] = 4.0
            planted.append(("class", k))
        b, best, gj, gi = _owner_cell(case, THRESH)
        raw[b, gj, gi, best, 4] = 0.0   # sigmoid = 0.5 exactly: not above 0.5
        planted.append(("conf", (b, best, gj, gi)))
        back = (n - 1, na - 1, g - 1, g - 2)   # a background cell (the CPU test asserts that it is one)
        raw[back[0], back[2], back[3], back[1], 4] = 0.0
        planted.append(("conf", back))
        case["background"] = back
    if name == "sat":
        # every objectness and class logit saturates: probability exactly 1 or 0 in fp32, 1 or below e^-100 in float64
        pick = rng.randint(0, 2, raw[..., 4:].shape)
        raw[..., 4:] = np.where(pick == 1, 40.0, -104.0).astype(np.float32)
        b, best, gj, gi = _owner_cell(case, THRESH)
        raw[b, gj, gi, best, 2] = 89.0   # exp overflows in fp32: the predicted box is infinitely wide, its IoU 0
        planted = [p for p in planted if p[0] == "cell"] + [("class", "all")]
    case["raw"] = raw.reshape(n, g, g, na * per)
    case["planted"] = tuple(planted)
    return case


@functools.lru_cache(maxsize=None)
def yolo_ref(name, dtype="float64", m=None):
    """The reference of a case (of its first ``m`` rows), computed once and shared: do not write into it."""
    c = yolo_case(name)
    tg = c["targets"] if m is None else np.concatenate([c["targets"]] * (m // max(1, len(c["targets"])) + 1))[:m]
    return yolo_loss_fwd_ref(c["raw"], c["anchors"], c["nc"], tg, 0.5, 1.0, 100.0, np.dtype(dtype))


# ---------------------------------------------------------------------------------------------------------------------
# evaluation tail
# ---------------------------------------------------------------------------------------------------------------------
def batch_statistics_ref(rows, targets, n_images, thr):
    """csrc/evaltail.hip in numpy float32: per image the detections in row order; a detection whose label occurs among the
    image's targets takes the target of maximal IoU (+1 convention, first maximum, any label) and is a true positive iff
    IoU >= thr and that target was not taken before; the scan of an image stops once all its targets are taken.
    ``rows`` [m, cols] (image first, box in columns 1..4, label last), ``targets`` [q, 6] (image, label, x1, y1, x2, y2).
    Returns (tp [m] float32, written [m] bool): rows of an image outside [0, n_images) are not written."""
    f = np.float32
    rows, targets = np.asarray(rows, f), np.asarray(targets, f).reshape(-1, 6)
    m = len(rows)
    tp, written = np.zeros(m, f), np.zeros(m, bool)
    for img in range(n_images):
        ann = targets[targets[:, 0] == f(img)]
        taken = set()
        if len(ann):
            area2 = (ann[:, 4] - ann[:, 2] + f(1)) * (ann[:, 5] - ann[:, 3] + f(1))
        for r in range(m):
            if rows[r, 0] != f(img):
                continue
            written[r] = True
            if len(ann) == 0 or len(taken) == len(ann):
                continue
            x1, y1, x2, y2, label = rows[r, 1], rows[r, 2], rows[r, 3], rows[r, 4], rows[r, -1]
            if not (ann[:, 1] == label).any():
                continue
            area1 = (x2 - x1 + f(1)) * (y2 - y1 + f(1))
            iw = np.maximum(np.minimum(x2, ann[:, 4]) - np.maximum(x1, ann[:, 2]) + f(1), f(0))
            ih = np.maximum(np.minimum(y2, ann[:, 5]) - np.maximum(y1, ann[:, 3]) + f(1), f(0))
            inter = iw * ih
            iou = inter / (area1 + area2 - inter + f(1e-16))
            best = int(np.argmax(iou))
            if iou[best] >= f(thr) and best not in taken:
                tp[r] = 1
                taken.add(best)
    return tp, written


STATS_Q = (1, 63, 64, 65, 130, 8192)
DUP_GROUPS = ((5, 6, 69), (70, 133), (31, 32))   # (5, 6) neighbouring lanes, (5, 69) one lane's two trips, (70, 133) a later lane's
# earlier trip against an earlier lane's later trip, (31, 32) the two sides of a bitmap word
MIRRORS = ((7, 8), (9, 73), (74, 137))           # two different boxes with bit-equal IoU to one detection: the lower index is taken
EARLY = (2, 66, 131)                             # the targets of the image whose scan ends early: three trips, two lanes


@functools.lru_cache(maxsize=None)
def stats_case(q, cols=8):
    """(rows [m, cols], targets [q, 6], n_images, notes).  Images 0 .. n_images - 3 hold the bulk of the targets (so each one's
    targets fall into every lane and, from q = 130 on, into several trips of a lane), image n_images - 2 the EARLY ones,
    image n_images - 1 none; image 1 gets no detections where there are at least five images."""
    rng = np.random.RandomState(7000 + q + cols)
    n_images = (4, 5, 6)[q % 3]
    early_img, bulk = n_images - 2, list(range(n_images - 2))
    nodet = 1 if n_images >= 5 else -1
    tg = np.zeros((q, 6), np.float32)
    tg[:, 0] = [bulk[t % len(bulk)] for t in range(q)]
    tg[:, 1] = rng.randint(0, 3, q)
    tg[:, 2:4] = rng.uniform(0, 900, (q, 2))
    tg[:, 4:6] = tg[:, 2:4] + rng.uniform(20, 120, (q, 2))
    early = [t for t in EARLY if t < q]
    tg[early, 0] = early_img
    groups = [tuple(t for t in grp if t < q) for grp in DUP_GROUPS]
    groups = [grp for grp in groups if len(grp) > 1]
    for grp in groups:
        tg[list(grp)] = tg[grp[0]]
        if tg[grp[0], 0] == nodet:
            tg[list(grp), 0] = 0
    mirrors = [grp for grp in MIRRORS if grp[1] < q]
    for i, (lo, hi) in enumerate(mirrors):   # integer boxes away from the others; hi is lo moved right by 20
        tg[lo, 0] = tg[hi, 0] = 0
        tg[hi, 1] = tg[lo, 1]
        tg[lo, 2:6] = (2000 + 300 * i, 100, 2080 + 300 * i, 180)
        tg[hi, 2:6] = tg[lo, 2:6] + np.float32([20, 0, 20, 0])
    rows, expect = [], {}

    def det(img, box, label):
        r = np.zeros(cols, np.float32)
        r[0], r[1:5], r[5], r[-1] = img, box, rng.uniform(0.05, 0.95), label
        r[6:cols - 1] = rng.uniform(0, 1, cols - 7)
        rows.append(r)
        return len(rows) - 1

    for grp in groups:   # two identical detections on a duplicated target: the first is a true positive, the second is not
        a = det(tg[grp[0], 0], tg[grp[0], 2:6], tg[grp[0], 1])
        b = det(tg[grp[0], 0], tg[grp[0], 2:6], tg[grp[0], 1])
        expect[a], expect[b] = 1.0, 0.0
    for lo, hi in mirrors:   # half-way between the two: the IoUs tie exactly (0.78), the first maximum is taken - seen by the
        # copies that follow: the lower target is no longer free, the higher one is
        expect[det(0, tg[lo, 2:6] + np.float32([10, 0, 10, 0]), tg[lo, 1])] = 1.0
        expect[det(0, tg[lo, 2:6], tg[lo, 1])] = 0.0
        expect[det(0, tg[hi, 2:6], tg[lo, 1])] = 1.0
    for t in early:      # every target of the early image is taken by its first detections; later rows of that image get 0
        expect[det(early_img, tg[t, 2:6], tg[t, 1])] = 1.0
    for t in early * 2:
        expect[det(early_img, tg[t, 2:6] + rng.uniform(-3, 3, 4).astype(np.float32), tg[t, 1])] = 0.0
    if tg[q - 1, 0] != nodet and q - 1 not in early and not any(q - 1 in grp for grp in groups):
        expect[det(tg[q - 1, 0], tg[q - 1, 2:6], tg[q - 1, 1])] = 1.0   # the highest target index (bit 31 of the last word)
    outside = (n_images, -1, n_images + 3, -2)
    for i in range(260):
        t = int(rng.randint(0, q))
        img = tg[t, 0] if tg[t, 0] != nodet and i % 7 else n_images - 1
        box = tg[t, 2:6] + rng.uniform(-12, 12, 4).astype(np.float32) * (i % 4 != 0)
        det(img, box, rng.randint(0, 4))   # label 3 never occurs among the targets
        if i % 50 == 7:
            det(outside[(i // 50) % 4], box, tg[t, 1])
    return np.stack(rows), tg, n_images, dict(expect=expect, nodet=nodet, early_img=early_img)


def stats_threshold_case():
    """One target; row 0 equals it (IoU exactly 1), row 1 is a jittered copy."""
    tg = np.array([[0, 1, 100, 120, 180, 260]], np.float32)
    rows = np.array([[0, 100, 120, 180, 260, 0.9, 0.5, 1], [0, 103.5, 117.25, 176, 262.5, 0.8, 0.5, 1]], np.float32)
    return rows, tg, 1


def stats_threshold_iou():
    """The fp32 IoU of the jittered row with the target, one rounding per operation."""
    f = np.float32
    rows, tg, _ = stats_threshold_case()
    x1, y1, x2, y2 = rows[1, 1:5]
    gx1, gy1, gx2, gy2 = tg[0, 2:6]
    inter = max(min(x2, gx2) - max(x1, gx1) + f(1), f(0)) * max(min(y2, gy2) - max(y1, gy1) + f(1), f(0))
    area1, area2 = (x2 - x1 + f(1)) * (y2 - y1 + f(1)), (gx2 - gx1 + f(1)) * (gy2 - gy1 + f(1))
    iou = inter / (area1 + area2 - inter + f(1e-16))
    assert isinstance(iou, np.float32)
    return iou


# ---------------------------------------------------------------------------------------------------------------------
# Adam / AdamW
# ---------------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, betas, eps, weight_decay, step):
    """The descriptor's scalars: computed in Python doubles and rounded to fp32 once, as millieye_amd/optim.py does."""
    beta1, beta2 = betas
    f = np.float32
    return dict(beta2=f(beta2), eps=f(eps), weight_decay=f(weight_decay), decay=f(1.0 - lr * weight_decay),
                one_minus_beta1=f(1.0 - beta1), one_minus_beta2=f(1.0 - beta2), neg_step_size=f(-(lr / (1.0 - beta1 ** step))),
                bias_correction2_sqrt=f((1.0 - beta2 ** step) ** 0.5))


def adam_step_ref(p, g, m, v, desc_scalars, decoupled):
    """One step in np.float32 arithmetic, every operation rounded on its own, in the order of the header of csrc/optim.hip.
    Returns the new (p, m, v); the inputs are not modified."""
    f = np.float32
    s = {k: f(x) for k, x in desc_scalars.items()}
    p, g, m, v = (np.array(a, f) for a in (p, g, m, v))
    if s["weight_decay"] != 0:
        if decoupled:
            p = p * s["decay"]
        else:
            g = g + s["weight_decay"] * p
    m = m + s["one_minus_beta1"] * (g - m)
    v = v * s["beta2"]
    v = v + (s["one_minus_beta2"] * g) * g
    denom = np.sqrt(v) / s["bias_correction2_sqrt"] + s["eps"]
    p = p + (s["neg_step_size"] * m) / denom
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


ADAM_KINDS = {"adam": (False, dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)),
              "adam_wd": (False, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)),
              "adamw": (True, dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)),
              "adamw_betas": (True, dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1))}
ADAM_COUNTS = (1, 3, 1023, 1024, 1025, 2048, 4097, 0)


@functools.lru_cache(maxsize=None)
def adam_table(tensors=64, seed=11):
    """``tensors`` x (p, g, m, v) with the element counts cycling through ADAM_COUNTS (a 0 in the middle and in the last slot of
    64): gradients of magnitude 1e-6 .. 1e2, one element in sixteen exactly 0 with v = 0 there (the denominator is eps)."""
    rng = np.random.RandomState(seed)
    table = []
    for t in range(tensors):
        k = ADAM_COUNTS[t % len(ADAM_COUNTS)]
        sign = rng.choice([-1.0, 1.0], k)   # p, g and m of one sign: no sum of the step cancels, so a last-bit difference stays one
        p = (sign * (0.1 + np.abs(rng.standard_normal(k)))).astype(np.float32)
        g = (10.0 ** rng.uniform(-6, 2, k) * sign).astype(np.float32)
        m = (0.1 * g * rng.uniform(0.5, 1.5, k)).astype(np.float32)
        v = (0.01 * g.astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, k)).astype(np.float32)
        zero = rng.randint(0, 16, k) == 0
        g[zero], v[zero] = 0.0, 0.0
        table.append((p, g, m, v))
    return table


def sat_expected(c, r):
    """The conf and cls terms of the saturated case by counting, formed in fp32 like the kernel forms them: a saturated
    probability on the wrong side costs exactly 100, one on the right side 0.  (conf with obj_scale = 1 and noobj_scale = 0,
    conf with the scales swapped, cls)."""
    raw5 = c["raw"].reshape(c["n"], c["g"], c["g"], c["na"], c["nc"] + 5).transpose(0, 3, 1, 2, 4)
    obj, noobj = r["obj"] == 1, r["noobj"] == 1
    f = np.float32
    k_obj, k_noobj = int((raw5[..., 4][obj] < 0).sum()), int((raw5[..., 4][noobj] > 0).sum())
    k_cls = int(((raw5[..., 5:][obj] > 0) != (r["tcls"][obj] == 1)).sum())
    assert k_obj and k_noobj and k_cls
    return (float(f(100 * k_obj) / f(r["n_obj"])), float(f(100 * k_noobj) / f(r["n_noobj"])),
            float(f(100 * k_cls) / (f(r["n_obj"]) * f(c["nc"]))))


def ulp_distance(a, b, at=None):
    """Largest distance of two fp32 arrays in units of the spacing of fp32 at ``b`` - or at the larger of |b| and |at| (the
    operand a sum started from, so that a sum that cancels is measured in the units it was rounded in); 0 where the bits agree."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.size == 0:
        return 0.0
    same = a.view(np.int32) == b.view(np.int32)
    ref = np.abs(b) if at is None else np.maximum(np.abs(b), np.abs(np.asarray(at, np.float32)))
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(ref).astype(np.float64)
    return float(np.where(same, 0.0, d).max())
