"""Stage-2 ExDark evaluation: ``evaluate`` of ``module2_mixed/test_mixed.py:23-97`` ("YOLO trained on COCO / Mixed, tested on
ExDark") with the per-batch work on the device.

Same signature (plus ``root`` / ``num_workers``) and return tuple ``(precision, recall, AP, f1, ap_class, box_stat, pr_curve)``.
Like the reference it builds ``ExDarkDataset(mode, coco_detector=False, augment=False, multiscale=False)`` itself - without
``img_size``, so frames are always produced at the dataset default of 416 and ``img_size`` only scales the targets.

The reference copies the whole raw detector output ``[N, A, 5 + C]`` to the host per batch, counts the rows with
``conf >= conf_thres`` in python, runs NMS on the CPU and ``get_batch_statistics`` as a python loop.  Here one batch is:

* ``StagedRaggedImages.to()``: one upload + one launch of ``me_image_batch_pad_resize_flip_u8_f32``;
* the detector through the engine with the NMS candidate decode inside it (``Darknet._run(x, nms_conf=conf_thres)``), then
  ``hip.nms_batched`` (selection + emit; at most 200 detections per image, as ``non_max_suppression_cpp``);
* ``me_nms_candidate_counts``: the pre-NMS count of every image (``box_stat["before"]``) from the candidate lists;
* ``me_gather_class_boxes_f32``: the kept rows ``output[:, :7]`` as ``(image_i, x1, y1, x2, y2, conf, cls_conf, cls_pred)``;
* ``me_batch_statistics_f32``: the true-positive flags of ``get_batch_statistics``;
* ONE device-to-host copy of rows + flags + counts (a few hundred KB at batch 32; the raw output never leaves the device).

``ap_per_class`` is module 2's (the curve carries the confidences) and runs on the host, as the metric code does everywhere.
"""
import argparse
import os

import numpy as np
import torch

from .. import hip
from ..my_models import _DETECTIONS_PER_IMG, define_yolo, init_yolo
from ..utils.utils import ap_per_class, load_classes, xywh2xyxy
from .datasets import ExDarkDataset

try:
    import tqdm
except Exception:  # pragma: no cover
    tqdm = None

__all__ = ["evaluate", "detect_batch", "build_parser", "main"]

_CHOSEN_CLASSES = list(range(12))  # indices of the ExDark classes among the detector's (test_mixed.py:193)


def detect_batch(model, imgs, conf_thres, nms_thres):
    """Detector + NMS + batch statistics inputs of one batch on the device.  ``imgs`` [n,3,S,S] CUDA float32.

    Returns the device tensors ``(rows, n_rows, before)``: ``rows`` [n * 200, 8] kept detections image-major in NMS order
    (rows at and beyond ``n_rows[0]`` have image index -1), ``before`` int32 [n] the per-image count of rows with
    ``conf >= conf_thres``.  All stream-ordered, nothing is read back."""
    if not hasattr(model, "_run"):
        raise hip.MeError("test_mixed.evaluate needs the library's Darknet (millieye_amd.yolov3.models.Darknet)")
    conf = float(conf_thres)
    plan, yolo_out = model._run(imgs, nms_conf=conf)
    n, n_rows_pred, per = yolo_out.shape
    det, cnt = hip.nms_batched(yolo_out, conf, float(nms_thres), _DETECTIONS_PER_IMG, writeback_xyxy=False,
                               prepped=plan.nms_prepped == conf)
    dev = imgs.device
    lib, stream = hip.lib(), hip.stream_ptr()
    before = torch.empty((n,), device=dev, dtype=torch.int32)
    ws_ptr, _keep = hip.nms_workspace(n, n_rows_pred, dev)
    hip.check(lib.me_nms_candidate_counts(ws_ptr, n, n_rows_pred, before.data_ptr(), None, stream), "me_nms_candidate_counts")
    cap = n * _DETECTIONS_PER_IMG
    rows = torch.full((cap, 8), -1.0, device=dev, dtype=torch.float32)
    n_rows = torch.empty((1,), device=dev, dtype=torch.int32)
    hip.check(lib.me_gather_class_boxes_f32(det.data_ptr(), cnt.data_ptr(), n, _DETECTIONS_PER_IMG, per - 5, -1, 0,
                                            rows.data_ptr(), n_rows.data_ptr(), stream), "me_gather_class_boxes_f32")
    return rows, n_rows, before


def _batch_tail(rows, n_rows, before, targets, n, iou_thres):
    """True-positive flags on the device, then the one copy back: ``(before, after, metrics)`` with ``metrics`` the
    ``[true_positives, pred_scores, pred_labels]`` of every image that has detections (get_batch_statistics)."""
    dev = rows.device
    cap = rows.shape[0]
    tg = targets.to(device=dev, dtype=torch.float32).contiguous()
    tp = torch.zeros((cap,), device=dev, dtype=torch.float32)
    hip.check(hip.lib().me_batch_statistics_f32(rows.data_ptr(), cap, 8, tg.data_ptr() if len(tg) else None, len(tg), n,
                                                float(iou_thres), tp.data_ptr(), hip.stream_ptr()), "me_batch_statistics_f32")
    host = torch.cat((rows.reshape(-1).view(torch.int32), tp.view(torch.int32), n_rows, before)).cpu().numpy()  # as bits
    m = int(host[cap * 9])
    before_h = host[cap * 9 + 1:].tolist()
    kept = host[:cap * 8].view(np.float32).reshape(cap, 8)[:m]
    flags = host[cap * 8:cap * 9].view(np.float32)[:m]
    idx = kept[:, 0].astype(np.int32)
    after = np.bincount(idx, minlength=n)[:n].tolist()
    metrics = []
    for i in range(n):
        sel = idx == i
        if sel.any():
            metrics.append([flags[sel].astype(np.float64), kept[sel, 5], kept[sel, 7]])
    return before_h, after, metrics


def evaluate(model, mode, iou_thres, conf_thres, nms_thres, img_size, batch_size, *, root=None, num_workers=32):
    model.eval()
    dataset = ExDarkDataset(mode, coco_detector=False, augment=False, multiscale=False, root=root)
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers,
                                             collate_fn=dataset.collate_fn)
    device = torch.device("cuda")
    labels = []
    sample_metrics = []
    box_stat = dict(before=[], after=[])
    it = dataloader if tqdm is None else tqdm.tqdm(dataloader, desc="Detecting objects")
    for _, imgs, targets in it:
        labels += targets[:, 1].tolist()
        targets[:, 2:] = xywh2xyxy(targets[:, 2:])
        targets[:, 2:] *= img_size
        with torch.no_grad():
            imgs = imgs.to(device)
            rows, n_rows, before = detect_batch(model, imgs, conf_thres, nms_thres)
            b, a, metrics = _batch_tail(rows, n_rows, before, targets, imgs.shape[0], iou_thres)
        box_stat["before"] += b
        box_stat["after"] += a
        sample_metrics += metrics

    if sample_metrics == []:
        true_positives, pred_scores, pred_labels, labels = np.array([0]), np.array([1]), np.array([1]), np.array([1])
    else:
        true_positives, pred_scores, pred_labels = [np.concatenate(x, 0) for x in list(zip(*sample_metrics))]
    precision, recall, AP, f1, ap_class, pr_curve = ap_per_class(true_positives, pred_scores, pred_labels, labels,
                                                                 with_conf=True)
    return precision, recall, AP, f1, ap_class, box_stat, pr_curve


def build_parser():
    p = argparse.ArgumentParser(description="stage-2 ExDark evaluation (module2_mixed/test_mixed.py)")
    p.add_argument("--batch_size", type=int, default=32, help="size of each image batch")
    p.add_argument("--model_def", type=str, default="config/yolov3-tiny-12.cfg", help="path to model definition file")
    p.add_argument("--weights_path", type=str, default="weights/best_mixed.pt", help="path to weights file")
    p.add_argument("--classes_path", type=str, default="config/exdark.names", help="path to class label file")
    p.add_argument("--iou_thres", type=float, default=0.5, help="iou threshold required to qualify as detected")
    p.add_argument("--conf_thres", type=float, default=0.01, help="object confidence threshold")
    p.add_argument("--nms_thres", type=float, default=0.5, help="iou thresshold for non-maximum suppression")
    p.add_argument("--img_size", type=int, default=416, help="size of each image dimension")
    return p


def _plot_pr_curve(pr_curve, iou_thres, conf_thres):
    try:
        import matplotlib as mpl
        mpl.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("matplotlib is not installed: the P-R curve plot is skipped")
        return
    p, r, _conf = np.array(pr_curve)
    mpl.rcParams["font.size"] = 20
    mpl.rcParams["figure.titlesize"] = "medium"
    plt.figure(figsize=(10, 5))
    plt.subplot(111)
    plt.plot(r, p, lw=3)
    plt.title("P-R Curve")
    plt.xlabel("Recall")
    plt.ylabel("Precision")
    plt.xlim((0, 1))
    plt.ylim((0, 1))
    plt.tight_layout()
    os.makedirs("plot/yolo_mixed", exist_ok=True)
    plt.savefig(f"plot/yolo_mixed/{iou_thres}_{conf_thres}.jpg")
    plt.close()


def main(argv=None):
    opt = build_parser().parse_args(argv)
    print(opt)
    model = define_yolo(opt.model_def).to(torch.device("cuda"))
    init_yolo(model, opt.weights_path)
    print("Compute mAP...")
    precision, recall, ap, f1, ap_class, box_stat, pr_curve = evaluate(
        model, mode="test", iou_thres=opt.iou_thres, conf_thres=opt.conf_thres, nms_thres=opt.nms_thres,
        img_size=opt.img_size, batch_size=opt.batch_size)
    print(f"img_number: {len(box_stat['after'])}, sample_number: {len(np.atleast_1d(pr_curve[0]))}")
    _plot_pr_curve(pr_curve, opt.iou_thres, opt.conf_thres)
    exdark_map = 0
    class_names = load_classes(opt.classes_path)
    for i, c in enumerate(ap_class):
        mark = "+" if c in _CHOSEN_CLASSES else "-"
        print(f"{mark} Class {c} ({class_names[c]})".ljust(30)
              + f"-AP: {ap[i]:.3f} -Precision:{precision[i]:.3f} -Recall:{recall[i]:.3f}")
        if c in _CHOSEN_CLASSES:
            exdark_map += ap[i]
    print(f"mAP_chosen classes:{exdark_map / len(_CHOSEN_CLASSES)}")
    print(f"mAP_all classes: {ap.mean()}")
    return precision, recall, ap, f1, ap_class, box_stat, pr_curve


if __name__ == "__main__":
    main()
