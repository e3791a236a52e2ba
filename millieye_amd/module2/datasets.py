"""Stage-2 input producers: the behaviour of ``ListDataset`` (``module2_mixed/utils/datasets.py:75-166``) with the batch
assembled on the GPU.

What a caller of the reference class can rely on is kept: the constructor arguments, the file convention (a list file of
image paths; the label of ``.../images/x.png`` is ``.../labels/x.txt``), ``(path, image, targets)`` items, a ``collate_fn``
that numbers the targets by sample and draws a new input size every tenth batch when ``multiscale``, and the consumption
of the python / numpy random streams (one ``np.random.random()`` per augmented item, one ``random.choice`` per resize), so
a seeded run sees the same flips, sizes and shuffles (``tests/golden/m2_listdataset.npz``).

The work is split differently.  The host only decodes (``decode_rgb_u8``) and does the label geometry, which is the one
helper shared with the stage-3 producer (``utils.datasets.letterbox_labels``); an item carries the raw uint8 frame and the
flip decision, and ``collate_fn`` hands back a ``StagedImages`` whose ``.to(device)`` uploads the bytes and runs
``me_image_pad_resize_flip_u8_f32`` (ToTensor + pad_to_square + flip + nearest resize in one pass).  There is no CPU
implementation; the restatement the tests compare with is ``oracle/datasets_ref.py``.

``ExDarkDataset`` (``module2_mixed/utils/datasets.py:170-334``, the loader of ``test_mixed.py``) follows the same split; its
frames all have different sizes, so its ``collate_fn`` hands back a ``StagedRaggedImages``: one upload and one launch of
``me_image_batch_pad_resize_flip_u8_f32`` per batch.
"""
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from ..utils.datasets import StagedImages, StagedRaggedImages, _pad_amounts, decode_rgb_u8, letterbox_labels, read_label_rows
from ..utils.utils import load_classes

__all__ = ["ListDataset", "ExDarkDataset", "obtain_bboxs"]

_IMAGE_SUFFIXES = (".png", ".jpg")
_SIZE_STEP, _SIZE_SPAN = 32, 3   # multiscale: img_size +- 3 strides of 32, redrawn every _RESIZE_EVERY batches
_RESIZE_EVERY = 10


def _label_file_of(image_line):
    """``images`` -> ``labels`` and the image suffix -> ``.txt``, on the raw line of the list file (trailing newline
    included, as the reference keeps it: callers strip at use)."""
    out = image_line.replace("images", "labels")
    for suffix in _IMAGE_SUFFIXES:
        out = out.replace(suffix, ".txt")
    return out


class ListDataset(Dataset):
    def __init__(self, list_path, img_size=416, augment=True, multiscale=True, normalized_labels=True):
        with open(list_path, "r") as fh:
            self.img_files = fh.readlines()
        self.label_files = [_label_file_of(line) for line in self.img_files]
        self.img_size = img_size
        self.augment, self.multiscale, self.normalized_labels = augment, multiscale, normalized_labels
        self.min_size = img_size - _SIZE_SPAN * _SIZE_STEP
        self.max_size = img_size + _SIZE_SPAN * _SIZE_STEP
        self.max_objects = 100
        self.batch_count = 0

    def __len__(self):
        return len(self.img_files)

    def _targets_of(self, slot, h, w):
        """``[k,6]`` rows of item ``slot`` relative to the padded square, or ``None`` when it has no label file."""
        label_path = self.label_files[slot].rstrip()
        if not os.path.exists(label_path):
            return None
        side = max(h, w)
        return letterbox_labels(read_label_rows(label_path), (h, w) if self.normalized_labels else (1, 1),
                                _pad_amounts(h, w), (side, side))

    def __getitem__(self, index):
        """-> ``(img_path, (frame_u8 [h,w,3], flip), targets [k,6] | None)``"""
        slot = index % len(self.img_files)
        img_path = self.img_files[slot].rstrip()
        frame = decode_rgb_u8(img_path)
        targets = self._targets_of(slot, frame.shape[0], frame.shape[1])
        flip = bool(self.augment) and np.random.random() < 0.5
        if flip:
            targets[:, 2] = 1 - targets[:, 2]  # (an unlabelled image fails here in the reference too)
        return img_path, (frame, flip), targets

    def collate_fn(self, batch):
        paths = tuple(item[0] for item in batch)
        frames = [item[1][0] for item in batch]
        flips = [item[1][1] for item in batch]
        labelled = [item[2] for item in batch if item[2] is not None]
        for sample, rows in enumerate(labelled):   # numbered among the labelled items, as the reference does
            rows[:, 0] = sample
        targets = torch.cat(labelled, 0)
        if self.multiscale and self.batch_count % _RESIZE_EVERY == 0:
            self.img_size = random.choice(range(self.min_size, self.max_size + 1, _SIZE_STEP))
        self.batch_count += 1
        return paths, StagedImages(frames, self.img_size, flips=flips), targets


# ---- ExDark ------------------------------------------------------------------------------------------------------------
_EXDARK_CLASSES = ["Bicycle", "Boat", "Bottle", "Bus", "Car", "Cat", "Chair", "Cup", "Dog", "Motorbike", "People", "Table"]
_EXDARK_IN_COCO = [0, 1, 2, 3, 5, 8, 15, 16, 39, 41, 56, 60]   # coco.names index of every ExDark class, in ExDark order
_EXDARK_TO_COCO_NAME = {"People": "person", "Table": "diningtable"}


def obtain_bboxs(path):
    """ExDark annotation rows ``[name, left, top, width, height]`` (integers) of a label file; ``%`` starts a comment line
    (``module2_mixed/utils/datasets.py:41-55``: the fields are split on single spaces and parsed with ``int``)."""
    with open(path, "r") as fh:
        lines = [x.strip() for x in fh.read().split("\n") if x and not x.startswith("%")]
    out = []
    for line in lines:
        items = line.split(" ")
        out.append([items[0], int(items[1]), int(items[2]), int(items[3]), int(items[4])])
    return out


class ExDarkDataset(Dataset):
    """ExDark in the layout the reference expects: ``<root>/../data/ExDark/imageclasslist.txt``, ``Img/<Class>/<name>``,
    ``Label/<Class>/<name>.txt`` and ``<root>/config/coco.names``, where ``root`` is the working directory unless given.

    ``__getitem__`` -> ``(img_path, (frame_u8 [h,w,3], flip), targets [k,6] | None)``; ``collate_fn`` -> ``(paths,
    StagedRaggedImages, targets [q,6])``.  set_div 1 and 2 form ``train``, 3 ``test``; ``valid`` is empty."""

    def __init__(self, mode, coco_detector=False, img_size=416, augment=True, multiscale=False, root=None):
        self.mode = mode
        self.img_size = img_size
        self.augment = augment
        self.multiscale = multiscale
        self.coco_detector = coco_detector
        self.root = root
        self.max_objects = 100
        self.min_size = self.img_size - _SIZE_SPAN * _SIZE_STEP
        self.max_size = self.img_size + _SIZE_SPAN * _SIZE_STEP
        self.batch_count = 0
        self.classes = list(_EXDARK_CLASSES)
        self.lighting = ["Low", "Ambient", "Object", "Single", "Weak", "Strong", "Screen", "Window", "Shadow", "Twilight"]
        self.sets = ["Train", "Valid", "Test"]
        self.chosen_classes = list(range(12))
        self._coco_names = None
        self.get_paths()

    def _at(self, rel):
        """A path of the reference's layout, relative to the working directory or to ``root``."""
        return rel if self.root is None else os.path.join(self.root, rel)

    def get_paths(self):
        split = {k: dict(img=[], label=[]) for k in ("train", "valid", "test")}
        with open(self._at("../data/ExDark/imageclasslist.txt"), "r") as fh:
            lines = [x.strip() for x in fh.read().split("\n") if x and not x.startswith("#")]
        for line in lines:
            image_name, image_class, _lighting, _place, set_div = line.split(" ")
            cls = int(image_class) - 1
            if cls not in self.chosen_classes:
                continue
            which = "train" if set_div in ("1", "2") else "test" if set_div == "3" else None
            if which is not None:
                split[which]["img"].append(self._at(os.path.join("../data/ExDark/Img", self.classes[cls], image_name)))
                split[which]["label"].append(
                    self._at(os.path.join("../data/ExDark/Label", self.classes[cls], image_name + ".txt")))
        self.paths = split

    def __len__(self):
        return len(self.paths[self.mode]["img"])

    def class_index(self, name):
        """ExDark label name -> class index of the detector (coco.names order, then the 12 ExDark classes unless
        ``coco_detector``)."""
        if self._coco_names is None:
            self._coco_names = load_classes(self._at("./config/coco.names"))
        idx = self._coco_names.index(_EXDARK_TO_COCO_NAME.get(name, name).lower())
        return idx if self.coco_detector else _EXDARK_IN_COCO.index(idx)

    def _targets_of(self, label_path, h, w):
        """``[k,6]`` float32 rows ``(0, class, cx, cy, w, h)`` relative to the padded square, or ``None`` without a label
        file.  float64 until the store, in the reference's order (:254-279): the left / top corner shifted by the padding
        on its side, the right / bottom corner (``left + width``, ``top + height``) by the padding on the far side -
        ``pad[3]`` is one pixel more than ``pad[2]`` when the size difference is odd."""
        if not os.path.exists(label_path):
            return None
        rows = obtain_bboxs(label_path)
        boxes = np.array([[self.class_index(r[0])] + r[1:] for r in rows], dtype=np.float64)
        pad = _pad_amounts(h, w)
        side = float(max(h, w))
        x1, y1 = boxes[:, 1] + pad[0], boxes[:, 2] + pad[2]
        x2, y2 = (boxes[:, 1] + boxes[:, 3]) + pad[1], (boxes[:, 2] + boxes[:, 4]) + pad[3]
        targets = torch.zeros((len(boxes), 6))
        targets[:, 1] = torch.from_numpy(boxes[:, 0])
        targets[:, 2] = torch.from_numpy(((x1 + x2) / 2) / side)
        targets[:, 3] = torch.from_numpy(((y1 + y2) / 2) / side)
        targets[:, 4] = torch.from_numpy(boxes[:, 3] / side)
        targets[:, 5] = torch.from_numpy(boxes[:, 4] / side)
        return targets

    def __getitem__(self, idx):
        sel = self.paths[self.mode]
        img_path, label_path = sel["img"][idx], sel["label"][idx]
        frame = decode_rgb_u8(img_path)
        targets = self._targets_of(label_path, frame.shape[0], frame.shape[1])
        flip = False
        if self.augment and torch.rand(1) < 0.5:   # one draw of torch's generator per item, as the reference
            flip = True
            targets[:, 2] = 1 - targets[:, 2]  # (an unlabelled image fails here in the reference too)
        return img_path, (frame, flip), targets

    def collate_fn(self, batch):
        paths = tuple(item[0] for item in batch)
        frames = [item[1][0] for item in batch]
        flips = [item[1][1] for item in batch]
        targets = [item[2] for item in batch]
        for sample, rows in enumerate(targets):   # numbered by position in the batch (unlike ListDataset)
            if rows is not None:
                rows[:, 0] = sample
        targets = torch.cat([rows for rows in targets if rows is not None], 0)  # no target at all: raises, as the reference
        if self.multiscale and self.batch_count % _RESIZE_EVERY == 0:
            self.img_size = random.choice(range(self.min_size, self.max_size + 1, _SIZE_STEP))
        self.batch_count += 1
        return paths, StagedRaggedImages(frames, self.img_size, flips=flips), targets
