"""CPU: the host half of ``millieye_amd.module2.datasets.ExDarkDataset`` (module2_mixed/utils/datasets.py:170-334) and the
``test_mixed`` entry point against the REAL reference's outputs on the small ExDark tree (tests/golden/exdark_eval_small.npz,
tests/golden/make_golden_exdark.py): path lists, class mapping, float64 label geometry, the torch.rand draws of the
augmentation, collate_fn numbering, and the module2_mixed drop-in names."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden.make_golden_exdark import EXDARK, NAME, RUN

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, NAME + ".npz"))


def _ds(**kw):
    from millieye_amd.module2.datasets import ExDarkDataset
    kw.setdefault("augment", False)
    return ExDarkDataset("test", root=RUN, **kw)


def test_paths_follow_imageclasslist(g):
    ds = _ds()
    for which in ("train", "valid", "test"):
        for key in ("img", "label"):
            got = [os.path.relpath(p, RUN) for p in ds.paths[which][key]]
            assert got == list(g[f"paths/{which}/{key}"]), (which, key)
    assert len(ds.paths["valid"]["img"]) == 0 and len(ds) == 12
    assert not set(ds.paths["train"]["img"]) & set(ds.paths["test"]["img"])


def test_paths_relative_to_the_working_directory(g, monkeypatch):
    """Without ``root`` the reference's relative paths, resolved against the working directory."""
    from millieye_amd.module2.datasets import ExDarkDataset
    monkeypatch.chdir(RUN)
    ds = ExDarkDataset("test", augment=False)
    assert ds.paths["test"]["img"] == list(g["paths/test/img"])
    assert ds.paths["train"]["label"] == list(g["paths/train/label"])
    assert ds[0][2] is not None


def test_targets_class_mapping_and_geometry(g):
    """Every item's targets bit for bit (float64 geometry narrowed once), both class mappings."""
    plain, coco = _ds(), _ds(coco_detector=True)
    names_seen = set()
    for i in range(len(plain)):
        path, (frame, flip), tg = plain[i]
        assert not flip and frame.dtype == torch.uint8 and frame.shape[2] == 3
        assert max(frame.shape[:2]) == int(g[f"items/{i}/padded"][-1])
        if not bool(g[f"items/{i}/has_targets"]):
            assert tg is None
            continue
        assert tg.dtype == torch.float32
        assert np.array_equal(tg.numpy(), g[f"items/{i}/targets"]), path
        assert np.array_equal(coco[i][2].numpy(), g[f"coco/{i}/targets"]), path
        with open(plain.paths["test"]["label"][i]) as fh:
            names_seen |= {line.split(" ")[0] for line in fh.read().split("\n") if line and not line.startswith("%")}
    assert {"People", "Table"} <= names_seen


def test_odd_padding_shifts_the_far_corner_one_more_pixel():
    """75 x 120 frame: pad (0, 0, 22, 23) - the bottom edge moves by pad2 = 23, the top by 22 (the reference's comment
    ``pad[3] == pad[2]`` does not hold), in float64."""
    from millieye_amd.module2.datasets import obtain_bboxs
    ds = _ds()
    i = [os.path.basename(p) for p in ds.paths["test"]["img"]].index("e02.png")
    _, (frame, _), tg = ds[i]
    assert tuple(frame.shape[:2]) == (75, 120)
    name, left, top, w, h = obtain_bboxs(ds.paths["test"]["label"][i])[0]
    cy = ((np.float64(top) + 22) + (np.float64(top) + np.float64(h) + 23)) / 2 / 120.0
    cx = ((np.float64(left) + 0) + (np.float64(left) + np.float64(w) + 0)) / 2 / 120.0
    assert tg[0, 3].item() == np.float32(cy) and tg[0, 2].item() == np.float32(cx)
    assert tg[0, 5].item() == np.float32(np.float64(h) / 120.0)


def test_augment_draws_one_torch_rand_per_item(g):
    """Same seed -> same flips as the reference, an unlabelled frame that draws a flip fails, and exactly one draw of torch's
    generator per item (the next draw afterwards is the reference's)."""
    ds, aug = _ds(), _ds(augment=True)
    state = np.random.get_state(), random.getstate()
    torch.manual_seed(EXDARK["aug_seed"])
    for i in range(len(aug)):
        if bool(g["aug/fails"][i]):
            with pytest.raises(TypeError):
                aug[i]
            continue
        _, (_, flip), tg = aug[i]
        assert flip == bool(g["aug/flips"][i]), i
        assert np.array_equal(tg.numpy() if tg is not None else np.zeros((0, 6), np.float32), g[f"aug/{i}/targets"]), i
        if flip:
            assert np.array_equal(tg[:, 2].numpy(), (1 - ds[i][2][:, 2]).numpy())
    assert torch.rand(1).numpy()[0] == g["aug/next_rand"][0]
    assert np.random.get_state()[1].tolist() == state[0][1].tolist() and random.getstate() == state[1]


def test_collate_fn_numbers_by_position_and_keeps_size(g):
    from millieye_amd.utils.datasets import StagedRaggedImages
    for size in EXDARK["sizes"]:
        ds = _ds(img_size=size)
        b = 0
        for start in range(0, len(ds), EXDARK["batch"]):
            items = [ds[i] for i in range(start, min(start + EXDARK["batch"], len(ds)))]
            paths, imgs, targets = ds.collate_fn(items)
            assert [os.path.relpath(p, RUN) for p in paths] == list(g[f"b{size}/{b}/paths"])
            assert isinstance(imgs, StagedRaggedImages) and imgs.shape == (len(items), 3, size, size)
            assert np.array_equal(targets.numpy(), g[f"b{size}/{b}/targets"]), (size, b)
            b += 1
        assert ds.batch_count == b


def test_collate_fn_without_targets_raises_and_multiscale_redraws():
    ds = _ds()
    unlabelled = [i for i in range(len(ds)) if ds[i][2] is None]
    with pytest.raises(ValueError):   # torch.cat of an empty list, as in the reference
        ds.collate_fn([ds[unlabelled[0]]])
    ms = _ds(multiscale=True)
    random.seed(3)
    expect = random.Random(3).choice(range(416 - 96, 416 + 96 + 1, 32))
    _, imgs, _ = ms.collate_fn([ms[0], ms[1]])
    assert imgs.size == expect and ms.batch_count == 1
    for _ in range(9):
        _, imgs2, _ = ms.collate_fn([ms[0]])
        assert imgs2.size == expect
    assert ms.batch_count == 10


def test_staged_batch_is_gpu_only():
    from millieye_amd import hip
    ds = _ds()
    _, imgs, _ = ds.collate_fn([ds[0], ds[1]])
    with pytest.raises(hip.MeError):
        imgs.to("cpu")
    with pytest.raises(hip.MeError):
        imgs.type(torch.FloatTensor)
    assert imgs.type() == "torch.cuda.FloatTensor"


def test_cli_flags_and_defaults_of_the_reference():
    from millieye_amd.module2.test_mixed import build_parser
    opt = build_parser().parse_args([])
    assert vars(opt) == dict(batch_size=32, model_def="config/yolov3-tiny-12.cfg", weights_path="weights/best_mixed.pt",
                             classes_path="config/exdark.names", iou_thres=0.5, conf_thres=0.01, nms_thres=0.5, img_size=416)


def test_dropin_m2_exports_exdark_and_test_mixed():
    code = ("from utils.datasets import ExDarkDataset, ListDataset; from test_mixed import evaluate; "
            "print(ExDarkDataset.__module__, evaluate.__module__)")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "millieye_amd", "dropin_m2"), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "millieye_amd.module2.datasets millieye_amd.module2.test_mixed"
