#!/usr/bin/env python
"""Generate tests/golden/exdark_small/ (a small ExDark tree) and tests/golden/exdark_eval_small.npz by running the REAL
module2_mixed reference (``utils/datasets.py`` ExDarkDataset, ``test_mixed.evaluate``) on it.  Build container only:

    python tests/golden/make_golden_exdark.py

The tree has the reference's layout (``data/ExDark/imageclasslist.txt``, ``Img/<Class>/<name>``, ``Label/<Class>/<name>.txt``,
``run/config/coco.names``; the working directory of a run is ``run/``): 12 test frames of 48 - 320 px (landscape, portrait,
square, odd and even size differences, a grayscale and a palette PNG, ``People`` / ``Table`` labels, one frame without a
label file) and two train rows (set_div 1 / 2).  The labels of the test frames are perturbed copies of what the synthetic
detector finds there (``relabel``), so that ``evaluate`` has true positives.

What the fixture pins
  paths/*           self.paths of the reference dataset (train / valid / test, file order)
  items/*           per test item: targets (float32 [k,6] or none), frame size
  b<S>/<i>/*        collate_fn batches (augment off, batch 4) at img_size S: images (uint8 codes, k / 255; at 416 every third
                    row / column, plus a position-weighted checksum), targets
  aug/*             augment=True under torch.manual_seed: flip decision per item, the next torch.rand draw afterwards
  eval<S>/*         test_mixed.evaluate at img_size S: precision / recall / AP / f1 / ap_class / box_stat / pr_curve
"""
import contextlib
import io
import os
import shutil
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from millieye_amd import cfgs, synth  # noqa: E402
from oracle import import_reference  # noqa: E402

TREE = os.path.join(HERE, "exdark_small")
RUN = os.path.join(TREE, "run")
NAME = "exdark_eval_small"
EXDARK = dict(cfg="yolov3-tiny-12", sizes=(160, 416), batch=4, conf=0.01, nms=0.5, iou=0.5, aug_seed=5, tag="exdark_small")

_CLASSES = ["Bicycle", "Boat", "Bottle", "Bus", "Car", "Cat", "Chair", "Cup", "Dog", "Motorbike", "People", "Table"]
_IN_COCO = [0, 1, 2, 3, 5, 8, 15, 16, 39, 41, 56, 60]   # label k of the 12-class detector -> coco.names index

# name, ExDark class folder (1-based index into _CLASSES), (h, w), PIL mode, set_div, labelled
FRAMES = [
    ("e00.png", 11, (120, 200), "RGB", "3", True),    # landscape, even difference
    ("e01.png", 11, (200, 120), "RGB", "3", True),    # portrait, even difference
    ("e02.png", 12, (75, 120), "RGB", "3", True),     # odd difference (pad2 = pad1 + 1)
    ("e03.png", 5, (121, 64), "RGB", "3", True),      # portrait, odd difference
    ("e04.png", 11, (160, 160), "RGB", "3", True),    # square, S == P at img_size 160
    ("e05.png", 1, (96, 96), "L", "3", True),         # grayscale
    ("e06.png", 9, (57, 90), "P", "3", True),         # palette, odd difference
    ("e07.png", 11, (48, 64), "RGB", "3", True),      # smallest
    ("e08.png", 12, (320, 213), "RGB", "3", True),    # largest side, odd difference
    ("e09.png", 7, (150, 260), "RGB", "3", False),    # no label file
    ("e10.png", 4, (233, 177), "RGB", "3", True),
    ("e11.png", 11, (64, 300), "RGB", "3", True),
    ("t00.png", 11, (100, 140), "RGB", "1", True),    # train rows: never in "test"
    ("t01.png", 3, (90, 90), "RGB", "2", True),
]


STORE_STRIDE = {160: 1, 416: 3}   # collated images are stored as uint8 codes, every STORE_STRIDE-th row / column


def weighted_sum(imgs):
    """Position-sensitive float64 checksum of a batch [n,3,S,S] (per frame)."""
    size = imgs.shape[-1]
    return (imgs.double() * torch.arange(size, dtype=torch.float64).view(1, 1, 1, -1)
            * torch.arange(1, size + 1, dtype=torch.float64).view(1, 1, -1, 1)).sum((1, 2, 3)).numpy()


def frame_pixels(name, h, w):
    """Smooth deterministic content (compresses well, gives the detector structure) + a little noise."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = synth.uniform(f"exdark/{name}/phase", (3, 3), 0.0, 6.28)
    img = np.zeros((h, w, 3))
    for c in range(3):
        img[..., c] = 0.5 + 0.25 * np.sin(xx / (7 + 3 * c) + ph[c, 0]) * np.cos(yy / (11 + 2 * c) + ph[c, 1]) \
            + 0.2 * np.sin((xx + yy) / 23.0 + ph[c, 2])
    img += synth.uniform(f"exdark/{name}/noise", (h, w, 3), -0.04, 0.04)
    return np.clip(img * 255.0, 0, 255).astype(np.uint8)


def write_tree():
    from PIL import Image
    if os.path.isdir(TREE):
        shutil.rmtree(TREE)
    os.makedirs(os.path.join(RUN, "config"))
    shutil.copy(os.path.join(import_reference.REFERENCE_ROOT, "module2_mixed", "config", "coco.names"),
                os.path.join(RUN, "config", "coco.names"))
    lines = ["# Name | Class | Light | In/Out | Train/Val/Test"]
    for name, cls, (h, w), mode, set_div, _lab in FRAMES:
        folder = os.path.join(TREE, "data", "ExDark", "Img", _CLASSES[cls - 1])
        os.makedirs(folder, exist_ok=True)
        os.makedirs(os.path.join(TREE, "data", "ExDark", "Label", _CLASSES[cls - 1]), exist_ok=True)
        im = Image.fromarray(frame_pixels(name, h, w))
        if mode == "L":
            im = im.convert("L")
        elif mode == "P":
            im = im.convert("P", palette=Image.ADAPTIVE, colors=64)
        im.save(os.path.join(folder, name))
        lines.append(f"{name} {cls} 1 1 {set_div}")
    lines.append("e99.png 13 1 1 3")    # a class outside the chosen 12: skipped
    with open(os.path.join(TREE, "data", "ExDark", "imageclasslist.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def label_name(k, coco_names):
    """Class label k of the 12-class detector -> the ExDark annotation name (``person`` is ``People``, ``diningtable``
    ``Table``)."""
    coco = coco_names[_IN_COCO[k]]
    return {"person": "People", "diningtable": "Table"}.get(coco, coco.capitalize())


def write_labels(detections):
    """ExDark label files ``% bbGt version=3`` + ``Name left top width height 0 0 0 0 0 0 0``.  ``detections``: name -> list
    of (label k, left, top, width, height) in pixels of the frame, or None (no file)."""
    coco_names = open(os.path.join(RUN, "config", "coco.names")).read().split("\n")[:-1]
    for name, cls, _hw, _mode, _sd, labelled in FRAMES:
        path = os.path.join(TREE, "data", "ExDark", "Label", _CLASSES[cls - 1], name + ".txt")
        if not labelled:
            if os.path.exists(path):
                os.remove(path)
            continue
        rows = detections.get(name) or [(cls_default(cls), 4, 5, 20, 16)]
        body = ["% bbGt version=3"] + [f"{label_name(k, coco_names)} {l} {t} {bw} {bh} 0 0 0 0 0 0 0"
                                        for k, l, t, bw, bh in rows]
        with open(path, "w") as f:
            f.write("\n".join(body) + "\n")


def cls_default(cls):
    """The 12-class label of an ExDark folder class (1-based)."""
    name = _CLASSES[cls - 1]
    coco = {"People": "person", "Table": "diningtable"}.get(name, name.lower())
    coco_names = open(os.path.join(RUN, "config", "coco.names")).read().split("\n")[:-1]
    return _IN_COCO.index(coco_names.index(coco))


def detector(ns, cfg_dir):
    """The reference Darknet with the fixture's deterministic weights (shared with the tests: ``fill_detector_``)."""
    model = ns.models.Darknet(cfgs.write_cfg(EXDARK["cfg"], cfg_dir))
    return fill_detector_(model).eval()


def fill_detector_(model):
    """Synth weights with the objectness of a trained detector: a few hundred rows per frame pass conf 0.01, fewer than 200
    survive NMS (``after`` is not capped by detections_per_img)."""
    synth.fill_darknet_(model, EXDARK["tag"])
    synth.trained_like_(model, tag=EXDARK["tag"] + "/trained", obj_bias=-8.0, cls_bias=-2.0, cls0_bias=0.5)
    return model


def relabel(ns, ds_mod, cfg_dir):
    """Labels of the test frames from the reference's own detections at 416 (two of the best boxes per frame, shifted and
    scaled a little), written as integer ExDark boxes of the original frame."""
    model = detector(ns, cfg_dir)
    ds = ds_mod.ExDarkDataset("test", coco_detector=False, augment=False, multiscale=False)
    dets = {}
    for i in range(len(ds)):
        path = ds.paths["test"]["img"][i]
        name = os.path.basename(path)
        _, img, _ = ds[i]
        P = img.shape[-1]
        h, w = [fr[2] for fr in FRAMES if fr[0] == name][0]
        pad_l, pad_t = (0, (w - h) // 2) if h <= w else ((h - w) // 2, 0)
        x = torch.nn.functional.interpolate(img.unsqueeze(0), size=416, mode="nearest")
        with torch.no_grad():
            _, out = model(x)
        out = ns.utils.non_max_suppression_cpp(out, conf_thresh=0.05, nms_thresh=0.5)[0]
        rows = []
        if out is not None:
            for j in range(min(2, len(out))):
                b = out[j, :4] * (P / 416.0)
                l, t = float(b[0]) - pad_l + 1.5, float(b[1]) - pad_t - 1.0
                bw, bh = float(b[2] - b[0]) * 1.04, float(b[3] - b[1]) * 0.97
                l, t = max(0, int(round(l))), max(0, int(round(t)))
                bw, bh = max(2, min(int(round(bw)), w - l)), max(2, min(int(round(bh)), h - t))
                rows.append((int(out[j, 6]), l, t, bw, bh))
        if [fr[1] for fr in FRAMES if fr[0] == name][0] == 12:   # Table folder: one "Table" box besides the detections
            rows.append((cls_default(12), 3, 4, 30, 20))
        dets[name] = rows
    write_labels(dets)


def run_reference():
    ns = import_reference.import_module2()
    cfg_dir = os.path.join(os.getcwd(), "cfg")
    import importlib
    cwd = os.getcwd()
    os.chdir(RUN)
    try:
        ds_mod = importlib.import_module("utils.datasets")
        write_labels({})                       # placeholder labels so that every labelled frame has a file
        relabel(ns, ds_mod, cfg_dir)
        return collect(ns, ds_mod, cfg_dir)
    finally:
        os.chdir(cwd)


def collect(ns, ds_mod, cfg_dir):
    arrays = {}
    c = EXDARK
    ds = ds_mod.ExDarkDataset("test", coco_detector=False, augment=False, multiscale=False)
    for which in ("train", "valid", "test"):
        arrays[f"paths/{which}/img"] = np.asarray(ds.paths[which]["img"], dtype=str)
        arrays[f"paths/{which}/label"] = np.asarray(ds.paths[which]["label"], dtype=str)
    for i in range(len(ds)):
        _, img, tg = ds[i]
        arrays[f"items/{i}/has_targets"] = np.asarray(tg is not None)
        arrays[f"items/{i}/targets"] = tg.numpy().copy() if tg is not None else np.zeros((0, 6), np.float32)
        arrays[f"items/{i}/padded"] = np.asarray(img.shape)
    coco = ds_mod.ExDarkDataset("test", coco_detector=True, augment=False, multiscale=False)
    for i in range(len(coco)):
        tg = coco[i][2]
        arrays[f"coco/{i}/targets"] = tg.numpy().copy() if tg is not None else np.zeros((0, 6), np.float32)
    # collated batches, augment off
    for size in c["sizes"]:
        ds = ds_mod.ExDarkDataset("test", coco_detector=False, img_size=size, augment=False, multiscale=False)
        for b, start in enumerate(range(0, len(ds), c["batch"])):
            items = [ds[i] for i in range(start, min(start + c["batch"], len(ds)))]
            paths, imgs, targets = ds.collate_fn(items)
            codes = torch.round(imgs * 255).to(torch.uint8)   # every value is k / 255 (ToTensor) or the 0 padding
            assert torch.equal(codes.float() / 255, imgs)
            arrays[f"b{size}/{b}/codes"] = codes.numpy()[:, :, ::STORE_STRIDE[size], ::STORE_STRIDE[size]].copy()
            arrays[f"b{size}/{b}/imgs_wsum"] = weighted_sum(imgs)
            arrays[f"b{size}/{b}/targets"] = targets.numpy().copy()
            arrays[f"b{size}/{b}/paths"] = np.asarray(paths, dtype=str)
    # augmentation: one torch.rand(1) per item; an unlabelled frame that draws a flip fails
    plain = ds_mod.ExDarkDataset("test", coco_detector=False, augment=False, multiscale=False)
    aug = ds_mod.ExDarkDataset("test", coco_detector=False, augment=True, multiscale=False)
    torch.manual_seed(c["aug_seed"])
    flips, fails = [], []
    for i in range(len(aug)):
        try:
            _, img, tg = aug[i]
        except TypeError:
            flips.append(True)
            fails.append(True)
            continue
        fails.append(False)
        flips.append(not torch.equal(img, plain[i][1]))
        arrays[f"aug/{i}/targets"] = tg.numpy().copy() if tg is not None else np.zeros((0, 6), np.float32)
    arrays["aug/flips"], arrays["aug/fails"] = np.asarray(flips), np.asarray(fails)
    arrays["aug/next_rand"] = torch.rand(1).numpy()
    assert any(flips) and not all(flips), flips
    # test_mixed.evaluate, DataLoader without worker processes
    sys.modules.pop("test_mixed", None)
    import test_mixed as ref_tm
    model = detector(ns, cfg_dir)
    real_loader = torch.utils.data.DataLoader

    def loader(dataset, **kw):
        kw.update(num_workers=0)
        return real_loader(dataset, **kw)

    torch.utils.data.DataLoader = loader
    try:
        for size in c["sizes"]:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                precision, recall, AP, f1, ap_class, box_stat, pr_curve = ref_tm.evaluate(
                    model, mode="test", iou_thres=c["iou"], conf_thres=c["conf"], nms_thres=c["nms"], img_size=size,
                    batch_size=c["batch"])
            k = f"eval{size}/"
            arrays[k + "precision"], arrays[k + "recall"] = np.asarray(precision), np.asarray(recall)
            arrays[k + "AP"], arrays[k + "f1"], arrays[k + "ap_class"] = np.asarray(AP), np.asarray(f1), np.asarray(ap_class)
            arrays[k + "before"], arrays[k + "after"] = np.asarray(box_stat["before"]), np.asarray(box_stat["after"])
            for j, part in enumerate(pr_curve):
                arrays[k + f"pr_curve{j}"] = np.asarray(part)
            print(size, "AP", AP, "before", box_stat["before"], "after", box_stat["after"])
    finally:
        torch.utils.data.DataLoader = real_loader
    return arrays


def main():
    write_tree()
    arrays = run_reference()
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
    for dirpath, _, files in os.walk(TREE):
        for f in files:
            assert os.path.getsize(os.path.join(dirpath, f)) < 512 * 1024, f


if __name__ == "__main__":
    main()
