"""Device time of the reference's Python NMS on the GPU (``hip.nms_python`` -> me_nms_python_f32, csrc/nms_py.hip), and the
error of its merged boxes:
python tools/pynms_latency.py [--repeats 20] [--out profiles/pynms_latency.txt] [--errors-out profiles/pynms_errors.txt]  (GPU box)

Latency: the scenes of tests/pynms_scene_helpers.py at [1,2535,17], [1,10647,85], [32,10647,85] and [16,22743,85], at conf_thresh
0.01 and 0.2 (nms_thresh 0.5), without merging (``utils.utils.non_max_suppression``: rank by objectness, ``>``) and with it
(``yolov3.utils.utils.non_max_suppression``: rank by obj * cls_conf, ``>=``, merged boxes).  Per row: candidates and kept rows per
image (min .. max over the batch), the device time of one call (HIP events around the call on the current stream; the input is
restored before every call, outside the events; 3 warm-up calls, median (min .. max) of the repeats), the same for
``hip.nms_batched`` - the kernels of ``non_max_suppression_cpp``: IoU without +1, at most 200 rows per image - on the same input,
and at the single-frame shapes the host time of the numpy restatement (tests/pynms_refs.py), once.

Errors: per golden scene and setting (tests/golden/pynms.npz) the reference's own fp32 deviation of its merged boxes from the
float64 restatement, the bar of tests/test_gpu_pynms.py (16 x that) and the device's largest deviation from the float64
restatement; the same for a pile of 32 768 near-identical boxes, whose bar is one fp32 unit of the coordinate.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from millieye_amd import hip  # noqa: E402
from tests import pynms_refs as refs  # noqa: E402
from tests import pynms_scene_helpers as sh  # noqa: E402

SHAPES = [(1, 2535, 12), (1, 10647, 80), (32, 10647, 80), (16, 22743, 80)]
VARIANTS = [("no merge", (0, False, False)), ("merge", (1, True, True))]
WARMUP = 3


def _spread(ms):
    return f"{statistics.median(ms):8.3f} ({min(ms):8.3f} .. {max(ms):8.3f})"


def device_ms(call, work, src, repeats):
    out = []
    for i in range(WARMUP + repeats):
        work.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(work)
        b.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            out.append(a.elapsed_time(b))
    return out


def latency(args, say):
    say(f"# {torch.cuda.get_device_name(0)}; device time per call in ms: median (min .. max) of {args.repeats} calls, {WARMUP} warm-up "
        f"calls, HIP events around the call; nms_thresh 0.5")
    say("# python NMS: hip.nms_python (no cap on the kept rows); cpp: hip.nms_batched, the kernels of non_max_suppression_cpp (IoU "
        "without +1, 200 rows per image at most) on the same input; host: tests/pynms_refs.py in numpy on this box's CPU, one run")
    for n, rows, nc in SHAPES:
        pred = sh.scene(f"pynms/latency/{n}x{rows}", n, rows, nc)
        src = torch.from_numpy(pred).cuda()
        work = torch.empty_like(src)
        for conf in (0.01, 0.2):
            cands = (pred[..., 4] >= np.float32(conf)).sum(1)
            cpp = device_ms(lambda w: hip.nms_batched(w, conf, 0.5, 200), work, src, args.repeats)
            for label, variant in VARIANTS:
                ms = device_ms(lambda w: hip.nms_python(w, conf, 0.5, *variant), work, src, args.repeats)
                work.copy_(src)
                kept = hip.nms_python(work, conf, 0.5, *variant)[1].cpu().numpy()
                line = (f"[{n},{rows},{5 + nc}] conf {conf:<4} {label:8s} | candidates {cands.min():5d} .. {cands.max():5d} | kept "
                        f"{kept.min():5d} .. {kept.max():5d} | python NMS {_spread(ms)} | cpp {_spread(cpp)}")
                if n == 1:
                    t0 = time.perf_counter()
                    res = refs.nms_python_ref(pred.copy(), conf, 0.5, *variant)
                    host = (time.perf_counter() - t0) * 1e3
                    assert len(res[0]["rows"]) == int(kept[0])
                    line += f" | host {host:9.1f}"
                say(line)


def errors(say):
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "pynms.npz"))
    say(f"# {torch.cuda.get_device_name(0)}; merged boxes of me_nms_python_f32 (score_mode 1, inclusive, merge) against the float64 "
        "restatement (tests/pynms_refs.py), px")
    say("# scene | conf_thresh nms_thresh | reference fp32 deviation from float64 | bar (16 x) | device deviation from float64")
    variant = (1, True, True)
    for name in sh.GOLDEN_SCENES:
        pred = sh.golden_scene(name)
        for conf, thr in sh.GOLDEN_SETTINGS:
            ref_dev = float(golden[sh.golden_key(name, conf, thr, "vend", "all", "ref_dev")])
            det, cnt = hip.nms_python(torch.from_numpy(pred).cuda(), conf, thr, *variant)
            det, cnt = det.cpu().numpy(), cnt.tolist()
            res = refs.nms_python_ref(pred.copy(), conf, thr, *variant)
            dev = 0.0
            for i, r in enumerate(res):
                if r is not None:
                    assert cnt[i] == len(r["rows"])
                    dev = max(dev, float(np.abs(det[i, :cnt[i], :4].astype(np.float64) - r["merged"]).max()))
            say(f"{name:7s} | {conf:<4} {thr:<3} | {ref_dev:.3e} | {16 * ref_dev:.3e} | {dev:.3e}")
    pred = sh.pile_scene(hip.PYNMS_MAX_ROWS)
    det, cnt = hip.nms_python(torch.from_numpy(pred).cuda(), 0.01, 0.5, *variant)
    xyxy = refs.xywh2xyxy(pred.copy())[0]
    wgt = xyxy[:, 4].astype(np.float64)
    mean = (wgt[:, None] * xyxy[:, :4].astype(np.float64)).sum(0) / wgt.sum()
    dev = np.abs(det[0, 0, :4].cpu().numpy().astype(np.float64) - mean).max()
    bar = float(np.spacing(np.abs(mean).astype(np.float32)).max())
    say(f"pile of {hip.PYNMS_MAX_ROWS} (kept {cnt.tolist()[0]}) | 0.01 0.5 | - | {bar:.3e} (one fp32 unit of the coordinate) | {dev:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default="profiles/pynms_latency.txt")
    ap.add_argument("--errors-out", default="profiles/pynms_errors.txt")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pynms_latency.py measures on the GPU; none is visible")
    for path, job in ((args.errors_out, errors), (args.out, lambda say: latency(args, say))):
        lines = []

        def say(text):
            print(text, flush=True)
            lines.append(text)

        job(say)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
