"""Inputs and plain restatements for the multi-stream output tail (csrc/nms.hip: me_nms_boxes_grouped_f32, me_stream_tail_f32;
demo.MultiStreamFuser(tail=...)): tests/test_stream_tail_cpu.py guards them, tests/test_gpu_stream_tail.py uses them.

The tail of one step, restated: group the network's rows ``(stream, x1, y1, x2, y2, p, cls_score, cls_pred)`` by stream, stably
(each stream keeps the network's order - ``torch.sort(rows[:, 0], stable=True)``), run torchvision's ``batched_nms`` on every
stream's rows alone, and rescale the kept boxes to the stream's frame in float32: ``((v - pad // 2) / unpadded) * original``,
three separately rounded operations (``utils.rescale_boxes``)."""
import numpy as np

from oracle import tv_ops_np

FRAME_SHAPES = ((480, 640), (360, 480), (640, 480), (512, 512), (1080, 1920), (97, 61), (3, 1000))   # (h, w)
SIZES = (416, 608, 96)


def rescale_scalars(current_dim, original_shape):
    """``(pad // 2, current_dim - pad, original)`` for x, then for y: the Python expressions of ``utils.rescale_boxes``."""
    orig = {"y": original_shape[0], "x": original_shape[1]}
    ratio = current_dim / max(original_shape)
    pad = {"x": max(orig["y"] - orig["x"], 0) * ratio, "y": max(orig["x"] - orig["y"], 0) * ratio}
    return [v for axis in ("x", "y") for v in (pad[axis] // 2, current_dim - pad[axis], orig[axis])]


def rescale_f32(boxes, current_dim, original_shape):
    """The rescale as the kernel does it: the six scalars cast to float32, then subtract, divide, multiply - each rounded to
    float32 (numpy float32 arithmetic is exactly that).  ``boxes`` [k,4] float32; returns a new array."""
    c = np.asarray(rescale_scalars(current_dim, original_shape), dtype=np.float64).astype(np.float32)
    b = np.asarray(boxes, dtype=np.float32)
    out = np.empty_like(b)
    with np.errstate(all="ignore"):
        for col, k in ((0, 0), (1, 3), (2, 0), (3, 3)):
            out[:, col] = ((b[:, col] - c[k]) / c[k + 1]) * c[k + 2]
    return out


def tail_ref(rows, streams, frame_hw, img_size, iou, nms=tv_ops_np.batched_nms):
    """The whole tail on the host: ``rows`` [m,8] float32 -> per stream the ``[k,7]`` float32 rows the fuser returns."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 8)
    order = np.argsort(rows[:, 0], kind="stable")
    grouped = rows[order]
    out = []
    for s in range(streams):
        mine = grouped[grouped[:, 0] == s]
        if len(mine) == 0:
            out.append(np.zeros((0, 7), np.float32))
            continue
        keep = np.asarray(nms(mine[:, 1:5], mine[:, 5], mine[:, 7], iou), dtype=np.int64)
        kept = mine[keep][:, 1:].copy()
        kept[:, :4] = rescale_f32(kept[:, :4], img_size, frame_hw[s])
        out.append(kept)
    return out


# ---- the fixture that can tell one maximum per group from a shared one -------------------------------------------------------
def group_a(n, seed):
    """``n`` boxes in [0,1], 0.005 - 0.01 wide, in tight clusters, 4 labels, score ties: (boxes [n,4], scores, labels)."""
    g = np.random.RandomState(seed)
    centres = g.uniform(0.05, 0.95, size=(max(n // 12, 2), 2))
    which = g.randint(0, len(centres), size=n)
    c = centres[which] + g.uniform(-0.002, 0.002, size=(n, 2))
    wh = g.uniform(0.005, 0.01, size=(n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    scores = (g.randint(1, 9, size=n) / 8.0).astype(np.float32)   # eight distinct values: many ties
    labels = g.randint(0, 4, size=n).astype(np.float32)
    return boxes, scores, labels


def group_b(n=40, seed=7):
    """``n`` boxes with coordinates up to 1e5: a maximum that, shared, swamps group A's 0.005-wide boxes in float32."""
    g = np.random.RandomState(seed)
    xy = g.uniform(0, 9.0e4, size=(n, 2))
    wh = g.uniform(100, 1.0e4, size=(n, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    boxes[0] = (9.0e4, 9.0e4, 1.0e5, 1.0e5)
    return boxes, g.uniform(0.1, 1.0, size=n).astype(np.float32), g.randint(0, 4, size=n).astype(np.float32)


def joint_call_kept(a, b, iou, classes=4):
    """What ONE batched_nms call over both groups with the label ``group * classes + class`` keeps of group ``a`` (local
    indices, kept order) - the shortcut the grouped entry point must not be."""
    boxes = np.concatenate([a[0], b[0]], 0)
    scores = np.concatenate([a[1], b[1]], 0)
    labels = np.concatenate([a[2], b[2] + classes], 0)
    keep = tv_ops_np.batched_nms(boxes, scores, labels, iou)
    return keep[keep < len(a[0])]


def synthetic_rows(streams, per_stream, seed, img_size=416, classes=4):
    """Network-like rows ``[m,8]`` for ``per_stream[s]`` detections of stream ``s`` in an interleaved stream order (the mode
    split returns the fusion sub-batch before the camera-only one): clustered boxes in network-input pixels, score ties."""
    g = np.random.RandomState(seed)
    parts = []
    for s in range(streams):
        n = per_stream[s]
        centres = g.uniform(40, img_size - 40, size=(max(n // 6, 1), 2))
        c = centres[g.randint(0, len(centres), size=n)] + g.uniform(-6, 6, size=(n, 2))
        wh = g.uniform(20, 90, size=(n, 2))
        rows = np.zeros((n, 8), np.float32)
        rows[:, 0] = s
        rows[:, 1:3], rows[:, 3:5] = c - wh / 2, c + wh / 2
        rows[:, 5] = g.randint(1, 17, size=n) / 16.0
        rows[:, 6] = g.uniform(0.2, 1.0, size=n)
        rows[:, 7] = g.randint(0, classes, size=n)
        parts.append(rows)
    order = [s for s in range(streams) if s % 3] + [s for s in range(streams) if s % 3 == 0]
    return np.concatenate([parts[s] for s in order], 0)
