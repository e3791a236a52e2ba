"""CPU (-m "not gpu"): host logic - cfg emitters/parsers, module tree / state-dict surface,
darknet .weights round trip, engine planning (no launches), C-ABI exports, deterministic synth."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from millieye_amd import synth
from tests import parity_helpers as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cfg_emitters_parse_to_expected_graphs():
    from millieye_amd.utils.parse_config import parse_model_config
    tiny = parse_model_config(ph.cfg_path("yolov3-tiny-12"))
    v3 = parse_model_config(ph.cfg_path("yolov3"))
    assert tiny[0]["type"] == "net" and len(tiny) == 25 and len(v3) == 108
    kinds = [b["type"] for b in v3[1:]]
    assert (kinds.count("convolutional"), kinds.count("shortcut"), kinds.count("route"), kinds.count("upsample"),
            kinds.count("yolo")) == (75, 23, 4, 2, 3)
    assert tiny[16]["filters"] == "51" and tiny[16]["batch_normalize"] == 0  # int default, strings otherwise
    assert tiny[1]["batch_normalize"] == "1"


def test_cfg_emitters_equal_reference_cfg_files():
    """Against the reference's config/*.cfg files, parsed into tests/golden/reference_cfgs.json (make_golden.py --cfgs)."""
    import json

    from millieye_amd.utils.parse_config import parse_model_config
    keys = ("type", "batch_normalize", "filters", "size", "stride", "activation", "layers", "from", "mask", "anchors",
            "classes")
    with open(os.path.join(ROOT, "tests", "golden", "reference_cfgs.json")) as fh:
        reference = json.load(fh)

    def norm(defs):
        return [{k: str(v).replace(" ", "") for k, v in d.items() if k in keys} for d in defs[1:]]
    for mine, ref in (("yolov3-tiny-12", "yolov3-tiny-12.cfg"), ("yolov3-tiny-coco", "yolov3-tiny-coco.cfg"),
                      ("yolov3", "yolov3.cfg")):
        a = norm(parse_model_config(ph.cfg_path(mine)))
        b = norm(reference[ref])
        assert len(b) > 0 and a == b, mine


def test_parse_data_config(tmp_path):
    from millieye_amd.utils.parse_config import parse_data_config
    p = tmp_path / "x.data"
    p.write_text("classes= 12\n# c\ntrain=a.txt\nnames=config/exdark.names\n\nlist=a b c\n")
    o = parse_data_config(str(p))
    assert o["gpus"] == "0,1,2,3" and o["num_workers"] == "10" and o["train"] == "a.txt"
    assert o["classes"] == ["", "12"] and o["list"] == ["a", "b", "c"]


def test_darknet_module_tree_and_state_dict_names():
    m = ph.make_darknet("yolov3-tiny-12")
    sd = m.state_dict()
    assert "module_list.0.conv_0.weight" in sd and "module_list.0.batch_norm_0.running_var" in sd
    assert "module_list.15.conv_15.bias" in sd and "module_list.15.batch_norm_15.weight" not in sd
    assert tuple(sd["module_list.12.conv_12.weight"].shape) == (1024, 512, 3, 3)
    assert sum(p.numel() for p in m.parameters()) == 8_695_286  # tiny-12 (same as the reference module tree)
    assert len(m.module_list) == 24 and len(m.yolo_layers) == 2
    assert [n for n, _ in m.module_list[11].named_children()] == ["_debug_padding_11", "maxpool_11"]
    assert m.yolo_layers[0].anchors == [(81, 82), (135, 169), (344, 319)]
    v3 = ph.make_darknet("yolov3")
    assert sum(p.numel() for p in v3.parameters()) == 61_949_149
    assert m.featuremap_module == 8 and v3.featuremap_module == 91


def test_network_state_dict_surface():
    from millieye_amd.my_models import Network, define_yolo
    net = Network(define_yolo(ph.cfg_path("yolov3-tiny-12")), 0.2)
    sd = net.state_dict()
    for key, shape in {
        "img_cnn_layers.net.conv_0.weight": (490, 256, 1, 1), "img_cnn_layers.net.batch_norm_0.running_mean": (490,),
        "radar_cnn_layers.conv1.0.weight": (32, 3, 3, 3), "radar_cnn_layers.conv3.3.weight": (10, 128, 1, 1),
        "refinement_head.net0.0.weight": (256, 490), "refinement_head.net2.0.weight": (13, 256),
        "refinement_head.net3.0.weight": (49, 256), "refinement_head.radar_net.0.weight": (10, 10, 7, 7),
        "refinement_head.fusion_head.0.weight": (1, 98), "ensemble_head.fc1.0.weight": (32, 2),
        "ensemble_head.fc2.0.weight": (2, 64), "base_detector.module_list.0.conv_0.weight": (16, 3, 3, 3),
    }.items():
        assert tuple(sd[key].shape) == shape, key
    heads = sum(v.numel() for k, v in net.named_parameters() if not k.startswith("base_detector."))
    assert heads == 369_820
    assert (net.refine_threshold_img, net.refine_threshold_radar, net.class_num, net.class_idx) == (0, 0, 1, 0)
    assert net.iou_thresh == (0.3, 0.7) and net.loss_lambda == (6, 1) and not net.base_detector.training


def test_darknet_weights_roundtrip(tmp_path):
    a = ph.make_darknet("yolov3-tiny-12", tag="rt")
    a.seen = 1234
    path = str(tmp_path / "w.weights")
    a.save_darknet_weights(path, cutoff=len(a.module_defs))  # default -1 drops the last module like the reference
    b = ph.make_darknet("yolov3-tiny-12", tag="other")
    b.load_darknet_weights(path)
    assert b.seen == 1234
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(va, vb), k


def test_engine_plan_fuses_and_reuses_memory():
    """Planning is pure host logic: no GPU, no library call."""
    from millieye_amd import planner
    from millieye_amd.engine import pick_tap_module
    from millieye_amd.utils.parse_config import parse_model_config
    defs = parse_model_config(ph.cfg_path("yolov3"))[1:]
    tap = pick_tap_module(defs)
    assert tap == 91
    n = 2
    ops, tensors, out, _rows = planner.lower(defs, 3, 96, 96, tap, False, False)
    # every [shortcut] and [upsample] of yolov3.cfg sits right after a conv and rides in its epilogue
    fused = [op for op in ops if op["kind"] == "conv" and op["covers"] == (op["module"], op["module"] + 1)]
    assert sum(op["res"] is not None and op["ups"] == 1 for op in fused) == 23
    assert sum(op["ups"] == 2 and op["res"] is None for op in fused) == 2 and len(fused) == 25
    assert not any(op["kind"] in ("add", "upsample") for op in ops)
    arena_bytes = planner.place(ops, tensors, n, out[tap], False)
    roots = [t for t in tensors if not t.external and t.parent is None]
    assert all(t.offset is not None for t in roots)
    assert 0 < arena_bytes < sum(n * t.h * t.w * t.c * t.esize for t in roots)


def test_synth_is_deterministic_and_sane():
    u = synth.uniform("t", (1000,))
    assert u.dtype == np.float32 and 0 <= u.min() and u.max() < 1
    assert np.array_equal(u, synth.uniform("t", (1000,))) and not np.array_equal(u, synth.uniform("t2", (1000,)))
    assert abs(float(u[0]) - 0.0) >= 0  # values pinned below so a generator change cannot go unnoticed
    assert np.allclose(synth.uniform("a", (4,)), [0.37173092, 0.5254534, 0.5774148, 0.14402205], atol=0)
    z = synth.normal("b", (100000,))
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02


def test_c_abi_exports_every_declared_symbol():
    """The library loads without a GPU and exports exactly what include/millieye_hip.h declares."""
    import __graft_entry__ as g
    from millieye_amd import hip
    g.build()
    header = open(os.path.join(ROOT, "include", "millieye_hip.h")).read()
    declared = set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", header))
    declared -= {"me_last_error"} - {"me_last_error"}
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert declared == set(hip.SIGNATURES), declared ^ set(hip.SIGNATURES)
    loaded = hip.load()
    assert loaded.me_abi_version() == 13
    for which, struct in hip._STRUCTS.items():
        assert loaded.me_sizeof(which) == ctypes.sizeof(struct)
    assert loaded.me_nms_workspace_bytes(2, 2535) > 0


def test_product_path_has_no_cpu_fallback():
    from millieye_amd import hip
    m = ph.make_darknet("yolov3-tiny-12")
    with pytest.raises(hip.MeError):
        m(ph.frames("cpu", 1, 96))  # CPU tensor -> loud error, never the oracle
    from millieye_amd.detector_graph import GraphedDetectorStep
    import torch
    with pytest.raises(hip.MeError):   # the captured training step: the same rule
        GraphedDetectorStep(m.eval())(ph.frames("cpu", 1, 96), torch.tensor([[0, 1, 0.5, 0.5, 0.2, 0.2]]))
    src = ""
    for root, _, files in os.walk(os.path.join(ROOT, "millieye_amd")):
        for f in files:
            if f.endswith(".py"):
                src += open(os.path.join(root, f)).read()
    assert "import oracle" not in src and "from oracle" not in src


def test_dropin_directories_export_the_reference_import_names():
    """``millieye_amd/dropin`` (module3_our_dataset) and ``millieye_amd/dropin_m2`` (module2_mixed) carry the top-level module
    names the reference's scripts import (INTEGRATION.md level 1): in a fresh interpreter started in each directory the names
    resolve to this package's classes."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    checks = {
        "dropin": "from my_models import Network, define_yolo, init_yolo; from test_fusion import evaluate; "
                  "from utils.datasets import MyDataset; from utils.utils import non_max_suppression_cpp, ap_per_class; "
                  "from utils.parse_config import parse_model_config; from yolov3.models import Darknet; "
                  "print(Network.__module__, MyDataset.__module__)",
        "dropin_m2": "from my_models import Network, define_yolo, init_yolo; from test_module2 import evaluate; "
                     "from utils.datasets import ListDataset; from utils.utils import ap_per_class, load_classes; "
                     "from utils.parse_config import parse_data_config; from yolov3.models import Darknet; "
                     "print(Network.__module__, ListDataset.__module__)",
    }
    expect = {"dropin": "millieye_amd.my_models millieye_amd.utils.datasets",
              "dropin_m2": "millieye_amd.module2.my_models millieye_amd.module2.datasets"}
    for d, code in checks.items():
        out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(root, "millieye_amd", d), capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == expect[d], out.stdout


def test_bench_roi_stage_bytes_are_algorithmic():
    """the "RoI pooling + heads" row of bench.py's stage table prices SURVEY 8(d) algorithmic bytes (every
    operand once), not the L2 re-reads of a retired kernel; and any committed stage table is self-consistent
    (frac == algorithmic_bytes / ms / peak)."""
    import glob
    import json

    import bench

    rois, n, fh, fw, wbytes, cols = 6449, 32, 52, 52, 1_300_000, 9
    got = bench.roi_stage_bytes(rois, n, fh, fw, fh, fw, wbytes, cols)
    maps = 4 * n * (fh * fw * 490 + fh * fw * 12)
    per_roi = 2 * 4 * 980 + 4 * cols + 4 * 16 + 1
    assert got == pytest.approx(maps + per_roi * rois + wbytes)
    # marginal bytes per RoI: the pooled features out + back and the rows, no weight re-read (490 * 256 * 4 / 8 per RoI in r04)
    step = bench.roi_stage_bytes(rois + 8, n, fh, fw, fh, fw, wbytes, cols) - got
    assert step == pytest.approx(8 * per_roi) and step < 8 * 8200
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in glob.glob(os.path.join(root, "profiles", "r05_bench_*.json")):
        for line in open(path):
            line = line.strip()
            if not line.startswith("{"):
                continue
            rec = json.loads(line)
            for row in rec.get("stages", []):
                if row.get("bound") == "hbm" and "algorithmic_bytes" in row and row["ms"] > 0:
                    gbs = row["algorithmic_bytes"] / (row["ms"] * 1e-3) / 1e9
                    assert row["frac"] <= gbs / bench.HBM_PEAK_GBS * 1.02 + 1e-4, (path, row)


def test_bench_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 / float64 files, the whole budget respected, an output over its share sampled by rows
    with the same rows on every run (two builds are compared file for file)."""
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 * 1024)
    big = torch.from_numpy(synth.uniform("dump/big", (4, 500, 17)))
    named = {"big": big, "flat": torch.from_numpy(synth.uniform("dump/flat", (40000,))),
             "loss": torch.tensor(1.5, dtype=torch.float64), "count": torch.tensor([3, 2 ** 40]),
             "half": torch.ones(5, 3, dtype=torch.bfloat16)}
    man = bench.dump_outputs(str(tmp_path / "a"), named)
    bench.dump_outputs(str(tmp_path / "b"), named)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "big_sample_rows.npy", "count.npy", "flat.npy", "flat_sample_rows.npy", "half.npy", "loss.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    assert np.load(tmp_path / "a" / "count.npy").tolist() == [3.0, 2.0 ** 40]  # integers exact (float64)
    assert np.load(tmp_path / "a" / "loss.npy").dtype == np.float64 and np.load(tmp_path / "a" / "half.npy").dtype == np.float32
    rows = np.load(tmp_path / "a" / "big_sample_rows.npy").astype(np.int64)
    sample = np.load(tmp_path / "a" / "big.npy")
    assert man["big"]["shape"] == [4, 500, 17] and man["big"]["sample_rows"] == len(rows) == sample.shape[0] > 0
    assert np.all(np.diff(rows) > 0) and np.array_equal(sample, big.reshape(-1, 17).numpy()[rows])
    rows = np.load(tmp_path / "a" / "flat_sample_rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "flat.npy"), named["flat"].numpy()[rows, None])
    assert "sample_rows" not in man["loss"] and np.array_equal(np.load(tmp_path / "a" / "half.npy"), np.ones((5, 3)))


def test_bench_conv_plan_holds_choices_the_tuner_offers(monkeypatch):
    """bench.py's pinned conv plan (profiles/bench_conv_plan_*.json): of the kernel generation the engine's tune file names,
    keyed like the tuner's cache for the default line's layers (416 x 416; batches 32, 8, 1 and the accuracy leg's 2), every
    (tile, split_k) one the tuner offers for a key of that storage type."""
    import json
    import re

    import bench
    from millieye_amd import engine
    monkeypatch.delenv("MILLIEYE_TUNE_CACHE", raising=False)
    version = re.fullmatch(r"conv_tune_(v\d+)\.json", os.path.basename(engine._tune_file())).group(1)
    assert os.path.basename(bench.CONV_PLAN) == f"bench_conv_plan_{version}_gfx950.json", "plan of another kernel generation"
    with open(os.path.join(ROOT, bench.CONV_PLAN)) as fh:
        table = json.load(fh)
    assert len(table) >= 30
    f32_tiles = engine._TUNE_TILES + engine._TUNE_TILES_TAIL + engine._TUNE_TILES_P8_F32 + (50, 60)
    h16_tiles = engine._TUNE_TILES_BF16 + engine._TUNE_TILES_P8 + (50, 60, 40, 41)
    for k, (tile, split) in table.items():
        key = tuple(int(x) for x in k.split(","))
        assert len(key) in (9, 10) and key[0] in (1, 2, 8, 32) and key[3] > 4 and key[1] == key[2], k
        half = len(key) == 10
        assert tile in (h16_tiles if half else f32_tiles), (k, tile)
        assert split in engine._TUNE_SPLITS, (k, split)
        if tile in (50, 60) or tile >= 100 or (half and tile in (40, 41)):
            assert split == 1, (k, tile, split)   # (kernels without a K split)
        if not half and tile in engine._TUNE_TILES_TAIL:
            assert split > 1, (k, tile, split)    # (tail tiles are offered with split_k >= 2 only)


def test_bench_pins_its_conv_plan_in_a_private_copy(monkeypatch):
    """bench.py runs the committed plan through a copy (the tuner writes back what it times; the committed file stays as it
    is); a tune file the caller chose wins."""
    import filecmp

    import bench
    monkeypatch.setenv("MILLIEYE_TUNE_CACHE", "")   # (unset for pin_conv_plan; setenv so that the teardown removes what it sets)
    monkeypatch.setenv("BENCH_CONV_PLAN", "")
    assert bench.pin_conv_plan() == bench.CONV_PLAN
    path = os.environ["MILLIEYE_TUNE_CACHE"]
    assert os.path.abspath(path) != os.path.join(ROOT, bench.CONV_PLAN)
    assert filecmp.cmp(path, os.path.join(ROOT, bench.CONV_PLAN), shallow=False)
    assert bench.pin_conv_plan() == bench.CONV_PLAN and os.environ["MILLIEYE_TUNE_CACHE"] == path   # (a spawned rank)
    monkeypatch.setenv("MILLIEYE_TUNE_CACHE", "/elsewhere/mine.json")
    monkeypatch.delenv("BENCH_CONV_PLAN")
    assert bench.pin_conv_plan() is None and os.environ["MILLIEYE_TUNE_CACHE"] == "/elsewhere/mine.json"


def test_head_caches_follow_replaced_inner_modules():
    """the head weight slots / BatchNorm lists are re-read from the leaf modules on every call - replacing an INNER
    module (``refinement_head.radar_net[1] = BatchNorm2d(..)``, ``net0 = Sequential(..)``) under an unchanged top-level child,
    or a detector block's BatchNorm, must not leave stale tensors behind."""
    from millieye_amd.my_models import Network, _HeadPack, define_yolo
    net = Network(define_yolo(ph.cfg_path("yolov3-tiny-12")), 0.2).eval()
    pack = _HeadPack(net)
    first = pack._slots()
    assert all(dct[key] is t for (dct, key), t in zip(first, pack._sources()))
    assert net._head_bns()[4] is net.refinement_head.radar_net[1] and net._head_bns()[0] is net.img_cnn_layers.net[1]
    net.refinement_head.radar_net[1] = torch.nn.BatchNorm2d(net.refinement_head.radar_net[1].num_features)
    net.refinement_head.net0 = torch.nn.Sequential(torch.nn.Linear(490, 256), torch.nn.LeakyReLU(0.1))
    second = pack._slots()
    assert second is not first
    assert all(dct[key] is t for (dct, key), t in zip(second, pack._sources()))
    assert net._head_bns()[4] is net.refinement_head.radar_net[1] and net._head_bns()[4].training
    with pytest.raises(NotImplementedError):
        net._check_eval()  # the fresh BatchNorm is in train() mode, the others are not
    det = net.base_detector
    assert not det._any_bn_training()
    block = det.module_list[0]
    bn_name = [k for k, m in block._modules.items() if isinstance(m, torch.nn.BatchNorm2d)][0]
    setattr(block, bn_name, torch.nn.BatchNorm2d(block._modules[bn_name].num_features))
    assert det._any_bn_training()
    det.eval()
    assert not det._any_bn_training()
