#!/usr/bin/env python
"""Generate tests/golden/pynms.npz by running the REAL reference's two Python NMS functions on the scenes of
tests/pynms_scene_helpers.py.  Build container only (the reference tree is imported through oracle/import_reference.py; the
vendored ``yolov3/utils/utils.py`` is loaded by path: its package name collides with nothing that way):

    python tests/golden/make_golden_pynms.py

Stored per scene: a checksum of the regenerated input; per (conf_thresh, nms_thresh) setting, function and image the kept rows
(``m3``: utils/utils.py:281-334; ``vend``: yolov3/utils/utils.py:231-293; an empty ``[0, 7]`` array stands for ``None``) and the
xyxy columns' checksum after the call; for ``vend`` also the reference's own largest fp32 deviation of its merged boxes from
the float64 restatement (tests/pynms_refs.py) - 16 x that is the bar of the device's merged boxes.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import pynms_refs as refs  # noqa: E402
from tests import pynms_scene_helpers as sh  # noqa: E402
from oracle import import_reference  # noqa: E402


def load_vendored():
    path = os.path.join(import_reference.REFERENCE_ROOT, "module3_our_dataset", "yolov3", "utils", "utils.py")
    spec = importlib.util.spec_from_file_location("reference_vendored_yolov3_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    m3 = import_reference.import_module3().utils.non_max_suppression
    vend = load_vendored().non_max_suppression
    out = {}
    for name in sh.GOLDEN_SCENES:
        pred = sh.golden_scene(name)
        out[f"{name}|checksum"] = np.array(sh.checksum(pred))
        for conf, thr in sh.GOLDEN_SETTINGS:
            sh.assert_defined(pred, thr)
            for fn, func, args in (("m3", m3, (0, False, False)), ("vend", vend, (1, True, True))):
                work = torch.from_numpy(pred.copy())
                got = func(work, conf, thr)
                mine = refs.nms_python_ref(pred.copy(), conf, thr, *args)
                out[sh.golden_key(name, conf, thr, fn, "all", "xyxy_checksum")] = np.array(sh.checksum(work.numpy()[..., :4]))
                dev = 0.0
                for img, (rows, res) in enumerate(zip(got, mine)):
                    rows = np.zeros((0, 7), np.float32) if rows is None else rows.numpy()
                    assert rows.dtype == np.float32
                    out[sh.golden_key(name, conf, thr, fn, img)] = rows
                    if fn == "vend" and len(rows):
                        assert res is not None and len(res["merged"]) == len(rows)
                        dev = max(dev, float(np.abs(rows[:, :4].astype(np.float64) - res["merged"]).max()))
                if fn == "vend":
                    out[sh.golden_key(name, conf, thr, fn, "all", "ref_dev")] = np.array(dev)
                    print(f"{name} conf {conf} thr {thr}: reference fp32 merged boxes deviate {dev:.3e} px from float64")
    path = os.path.join(HERE, "pynms.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
