"""The numpy restatement of the reference's Python NMS (tests/pynms_refs.py) against the goldens recorded from the real
reference (tests/golden/pynms.npz) and, where the reference tree is present, against the live functions on further seeds."""
import importlib.util
import os

import numpy as np
import pytest

from tests import pynms_refs as refs
from tests import pynms_scene_helpers as sh

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = {"m3": (0, False, False), "vend": (1, True, True)}  # score_mode, inclusive, merge


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pynms.npz"))


@pytest.mark.parametrize("name", sh.GOLDEN_SCENES)
def test_scenes_are_defined_and_match_their_checksum(golden, name):
    pred = sh.golden_scene(name)
    for _conf, thr in sh.GOLDEN_SETTINGS:
        sh.assert_defined(pred, thr)
    assert sh.checksum(pred) == str(golden[f"{name}|checksum"])


@pytest.mark.parametrize("fn", sorted(VARIANTS))
@pytest.mark.parametrize("name", sh.GOLDEN_SCENES)
def test_restatement_equals_the_goldens(golden, name, fn):
    merge = VARIANTS[fn][2]
    for conf, thr in sh.GOLDEN_SETTINGS:
        pred = sh.golden_scene(name)
        res = refs.nms_python_ref(pred, conf, thr, *VARIANTS[fn])
        assert sh.checksum(pred[..., :4]) == str(golden[sh.golden_key(name, conf, thr, fn, "all", "xyxy_checksum")])
        for img, r in enumerate(res):
            want = golden[sh.golden_key(name, conf, thr, fn, img)]
            if r is None:
                assert want.shape == (0, 7)
                continue
            if not merge:
                assert np.array_equal(refs.final_rows(r, False), want)  # rows exact
            else:  # count, order and columns 4-6 exact; the reference's fp32 boxes lie within its recorded deviation of float64
                assert r["rows"].shape == want.shape and np.array_equal(r["rows"][:, 4:], want[:, 4:])
                dev = float(golden[sh.golden_key(name, conf, thr, fn, "all", "ref_dev")])
                assert np.abs(want[:, :4].astype(np.float64) - r["merged"]).max() <= dev
    if name == "gap":
        assert res[1] is None and res[0] is not None and res[2] is not None


def test_exact_threshold_pair_analytic():
    """The +1 IoU of the pair is exactly 0.5: ``>`` keeps both, ``>=`` merges them to y2 = 7."""
    a = refs.nms_python_ref(sh.exact_pair_scene(), 0.01, 0.5)[0]
    assert np.array_equal(a["rows"][:, :4], np.array([[0, 0, 9, 9], [0, 0, 9, 4]], np.float32))
    b = refs.nms_python_ref(sh.exact_pair_scene(), 0.01, 0.5, 1, True, True)[0]
    assert np.array_equal(b["merged"], np.array([[0.0, 0.0, 9.0, 7.0]]))


def test_analytic_scenes_have_the_stated_answers():
    g = refs.nms_python_ref(sh.grid_scene(300), 0.01, 0.5)[0]
    assert len(g["rows"]) == 300 and (np.diff(g["rows"][:, 4]) < 0).all()
    p = refs.nms_python_ref(sh.pile_scene(300), 0.01, 0.5, 1, True, True)[0]
    assert len(p["rows"]) == 1
    boxes, obj = sh.chain_rows()
    c = refs.nms_python_ref(sh.rows_from(boxes, np.array(obj, np.float32), [0, 0, 0]), 0.01, 0.5)[0]
    assert list(c["index"]) == [0, 2]


def _live_functions():
    """The reference's two functions, loaded by path in this process: the stand-ins for the third-party modules the reference
    imports (oracle/import_reference.py) are taken out of ``sys.modules`` again, the working directory and ``sys.path`` stay."""
    import sys

    from oracle import import_reference

    if not import_reference.reference_available():
        pytest.skip("the reference tree is not on this machine")
    before, bytecode = set(sys.modules), sys.dont_write_bytecode
    out = {}
    try:
        import_reference.install_stubs()
        for fn, rel in (("m3", ("utils", "utils.py")), ("vend", ("yolov3", "utils", "utils.py"))):
            path = os.path.join(import_reference.REFERENCE_ROOT, "module3_our_dataset", *rel)
            spec = importlib.util.spec_from_file_location("reference_pynms_" + fn, path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            out[fn] = mod.non_max_suppression
    finally:
        for name in set(sys.modules) - before:
            if name.split(".")[0] in ("torchvision", "terminaltables"):
                del sys.modules[name]
        sys.dont_write_bytecode = bytecode
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_equals_the_live_reference(seed):
    import torch

    live = _live_functions()
    pred = sh.scene(f"pynms/live/{seed}", 2, 1500 + 37 * seed, 7 + seed)
    for conf, thr in sh.GOLDEN_SETTINGS + [(0.05, 0.7)]:
        sh.assert_defined(pred, thr)
        for fn, args in VARIANTS.items():
            work = torch.from_numpy(pred.copy())
            got = live[fn](work, conf, thr)
            mine_in = pred.copy()
            mine = refs.nms_python_ref(mine_in, conf, thr, *args)
            assert np.array_equal(work.numpy()[..., :4], mine_in[..., :4])
            for rows, r in zip(got, mine):
                assert (rows is None) == (r is None)
                if rows is None:
                    continue
                rows = rows.numpy()
                assert rows.shape == r["rows"].shape and np.array_equal(rows[:, 4:], r["rows"][:, 4:])
                if args[2]:
                    assert np.abs(rows[:, :4].astype(np.float64) - r["merged"]).max() < 1e-3
                else:
                    assert np.array_equal(rows, r["rows"])


def test_binding_and_dropin_trees_carry_the_python_nms():
    """No GPU needed: the binding declares the two entry points and the descriptor, and in a fresh interpreter started in each
    drop-in directory ``from utils.utils import *`` and ``yolov3.utils.utils`` resolve to this package's functions."""
    import subprocess
    import sys

    from millieye_amd import hip

    assert {"me_nms_python_f32", "me_nms_python_workspace_bytes"} <= set(hip.SIGNATURES)
    assert hip.NmsPythonDesc in hip._STRUCTS.values() and hip.PYNMS_MAX_ROWS == 32768
    import millieye_amd.yolov3.utils.utils as vendored

    assert vendored.__all__ == ["non_max_suppression"]  # the module holds only this function
    root = os.path.dirname(HERE)
    code = ("from utils.utils import *; import yolov3.utils.utils as v; "
            "assert non_max_suppression.__module__ == 'millieye_amd.utils.utils', non_max_suppression.__module__; "
            "assert v.non_max_suppression.__module__ == 'millieye_amd.yolov3.utils.utils'")
    for tree in ("dropin", "dropin_m2"):
        subprocess.run([sys.executable, "-c", code], cwd=os.path.join(root, "millieye_amd", tree), check=True)
