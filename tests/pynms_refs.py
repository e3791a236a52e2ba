"""numpy restatement of the reference's two Python NMS functions (``utils/utils.py:281-334`` and the vendored
``yolov3/utils/utils.py:231-293``): fp32 in the reference's operation order for every decision and for columns 4-6, float64 for
the merged boxes, a stable sort for ties (the library's rule: lower row first).  A kept box always removes itself (the stated
departure: the reference does not end when the top box fails its own test)."""
import numpy as np

F1 = np.float32(1)
EPS = np.float32(1e-16)


def xywh2xyxy(pred):
    """In-place centre/size -> corners on every row (``c -+ w / 2`` in fp32)."""
    cx, cy, hw, hh = pred[..., 0].copy(), pred[..., 1].copy(), pred[..., 2] / np.float32(2), pred[..., 3] / np.float32(2)
    pred[..., 0], pred[..., 1], pred[..., 2], pred[..., 3] = cx - hw, cy - hh, cx + hw, cy + hh
    return pred


def iou_plus1(box, boxes):
    """``bbox_iou(box[None], boxes)`` of the reference in fp32 (NaN where the reference gives NaN)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x1, y1 = np.maximum(box[0], boxes[:, 0]), np.maximum(box[1], boxes[:, 1])  # np.maximum / minimum hand NaN on like torch
        x2, y2 = np.minimum(box[2], boxes[:, 2]), np.minimum(box[3], boxes[:, 3])
        dw, dh = (x2 - x1) + F1, (y2 - y1) + F1
        dw = np.where(dw < 0, np.float32(0), dw)  # clamp(min=0): NaN stays NaN
        dh = np.where(dh < 0, np.float32(0), dh)
        inter = dw * dh
        a1 = ((box[2] - box[0]) + F1) * ((box[3] - box[1]) + F1)
        a2 = ((boxes[:, 2] - boxes[:, 0]) + F1) * ((boxes[:, 3] - boxes[:, 1]) + F1)
        return inter / (((a1 + a2) - inter) + EPS)


def nms_python_ref(pred, conf_thresh, thr, score_mode=0, inclusive=False, merge=False):
    """``pred`` float32 ``[n, rows, 5 + C]`` is converted to xyxy in place.  Returns per image ``None`` or a dict: ``rows``
    float32 ``[k, 7]`` (boxes un-merged), ``merged`` float64 ``[k, 4]`` (the weighted means; equal to the boxes without
    ``merge``), ``index`` the kept prediction rows, ``cands`` the candidate count."""
    assert pred.dtype == np.float32
    xywh2xyxy(pred)
    conf_thresh, thr = np.float32(conf_thresh), np.float32(thr)
    out = []
    for img in pred:
        with np.errstate(invalid="ignore"):
            cand = np.nonzero(img[:, 4] >= conf_thresh)[0]
        if len(cand) == 0:
            out.append(None)
            continue
        rows = img[cand]
        cls_pred = rows[:, 5:].argmax(1)
        cls_conf = rows[np.arange(len(rows)), 5 + cls_pred]
        score = rows[:, 4] * cls_conf if score_mode else rows[:, 4]
        order = np.argsort(-(score + np.float32(0)), kind="stable")
        det = np.concatenate([rows[order, :5], cls_conf[order, None], cls_pred[order, None].astype(np.float32)], 1)
        index = cand[order]
        alive = np.arange(len(det))
        kept, merged = [], []
        while len(alive):
            cur = det[alive]
            with np.errstate(invalid="ignore"):
                iou = iou_plus1(cur[0, :4], cur[:, :4])
                invalid = ((iou >= thr) if inclusive else (iou > thr)) & (cur[:, 6] == cur[0, 6])
            invalid[0] = True
            kept.append(alive[0])
            if merge:
                wgt = cur[invalid, 4].astype(np.float64)
                merged.append((wgt[:, None] * cur[invalid, :4].astype(np.float64)).sum(0) / wgt.sum())
            else:
                merged.append(cur[0, :4].astype(np.float64))
            alive = alive[~invalid]
        kept = np.asarray(kept)
        out.append({"rows": det[kept], "merged": np.asarray(merged), "index": index[kept], "cands": len(cand)})
    return out


def final_rows(res, merge):
    """The ``[k, 7]`` float32 rows a caller sees: merged boxes rounded to fp32 under ``merge``."""
    rows = res["rows"].copy()
    if merge:
        rows[:, :4] = res["merged"].astype(np.float32)
    return rows
