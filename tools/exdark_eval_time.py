"""Per-batch timing of the stage-2 ExDark evaluation (millieye_amd/module2/test_mixed.py) on synthetic ExDark-like frames.

    python tools/exdark_eval_time.py [--cfg yolov3] [--batch 32] [--conf 0.01] [--batches 4] [--reps 20]

Frames of random sizes (160 - 640 px per side, like ExDark's) are made in memory; the detector has synth weights
(``fill_darknet_`` + ``trained_like_``).  Reported (median over ``reps`` after a warm-up, CUDA events on the current stream):
  producer_batched_ms    StagedRaggedImages.to(): one pinned upload + one me_image_batch_pad_resize_flip_u8_f32 launch
  producer_per_frame_ms  StagedImages.to(): one H2D copy + one me_image_pad_resize_flip_u8_f32 launch per frame
  tail_ms                detector (+ NMS candidate decode) -> NMS -> pre-NMS counts -> rows -> batch statistics -> the one
                         device-to-host copy (detect_batch + _batch_tail), i.e. forward to box_stat
  before_mean, over_matn_rate, fallback_rate
                         pre-NMS candidates per frame; share of frames with more than 1024 candidates (beyond the matrix path
                         of csrc/nms.hip) and share the single-workgroup kernel redid (me_nms_candidate_counts' fallback flags)
One JSON line.  A single-process measurement, not a driver benchmark.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from millieye_amd import cfgs, hip, synth  # noqa: E402
from millieye_amd.module2.test_mixed import _batch_tail, detect_batch  # noqa: E402
from millieye_amd.utils.datasets import StagedImages, StagedRaggedImages  # noqa: E402
from millieye_amd.yolov3.models import Darknet  # noqa: E402

MATN = 1024  # candidates per image the matrix path of csrc/nms.hip looks at


def frames_of(tag, n):
    sides = synth.uniform(tag + "/sides", (n, 2), 160, 641).astype(int)
    return [torch.from_numpy(synth.uniform(f"{tag}/{i}", (int(h), int(w), 3), 0, 256).astype(np.uint8)) for i, (h, w) in
            enumerate(sides)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", default="yolov3")
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--size", type=int, default=416)
    p.add_argument("--conf", type=float, default=0.01)
    p.add_argument("--nms", type=float, default=0.5)
    p.add_argument("--batches", type=int, default=4)
    p.add_argument("--reps", type=int, default=20)
    opt = p.parse_args(argv)
    cfg_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "millieye_exdark_time_cfg")
    model = Darknet(cfgs.write_cfg(opt.cfg, cfg_dir))
    synth.fill_darknet_(model, "exdark_time")
    synth.trained_like_(model, tag="exdark_time/trained")
    model = model.cuda().eval()
    frames = frames_of("exdark_time", opt.batch)
    flips = [bool(i % 2) for i in range(opt.batch)]
    res = dict(cfg=opt.cfg, batch=opt.batch, size=opt.size, conf=opt.conf)
    res["producer_batched_ms"] = timed(lambda: StagedRaggedImages(frames, opt.size, flips).to("cuda"), opt.reps)
    res["producer_per_frame_ms"] = timed(lambda: StagedImages(frames, opt.size, flips).to("cuda"), opt.reps)
    ragged = StagedRaggedImages(frames, opt.size, flips).to("cuda")
    plain = StagedImages(frames, opt.size, flips).to("cuda")
    res["producer_bit_identical"] = bool(torch.equal(ragged, plain))
    targets = torch.tensor([[i, 0, 50.0, 60.0, 200.0, 220.0] for i in range(opt.batch)], dtype=torch.float32)

    def tail():
        with torch.no_grad():
            rows, n_rows, before = detect_batch(model, ragged, opt.conf, opt.nms)
            return _batch_tail(rows, n_rows, before, targets, opt.batch, 0.5)

    res["tail_ms"] = timed(tail, opt.reps)
    before, over, fell = [], 0, 0
    n_frames = 0
    for b in range(opt.batches):
        x = StagedRaggedImages(frames_of(f"exdark_time/b{b}", opt.batch), opt.size, flips).to("cuda")
        with torch.no_grad():
            rows, n_rows, cnt = detect_batch(model, x, opt.conf, opt.nms)
        n, rows_pred = x.shape[0], model.engine_for(model.compute_dtype).plan_for(x, False).rows
        fb = torch.empty((n,), device=x.device, dtype=torch.int32)
        ws_ptr, _keep = hip.nms_workspace(n, rows_pred, x.device)
        hip.check(hip.lib().me_nms_candidate_counts(ws_ptr, n, rows_pred, None, fb.data_ptr(), hip.stream_ptr()),
                  "me_nms_candidate_counts")
        c = cnt.cpu().numpy()
        before += c.tolist()
        over += int((c > MATN).sum())
        fell += int(fb.cpu().numpy().sum())
        n_frames += n
    res["before_mean"] = float(np.mean(before))
    res["over_matn_rate"] = over / n_frames
    res["fallback_rate"] = fell / n_frames
    print(json.dumps(res))


if __name__ == "__main__":
    main()
