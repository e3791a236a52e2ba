"""Step time of the headline path on rectangular frames: python tools/rect_latency.py [--steps 20] [--out profiles/rect_inference.txt]
(GPU box)

``Darknet.forward -> NMS -> Network.forward`` in mode 0 (one ``Network.forward`` call: detector, NMS, score maps, RoI heads, one
host read of the row count), built like ``bench.py``'s ``full`` workload - the same seeded weights, frames cropped from the
benchmark's 416 x 416 frames, its radar inputs - for yolov3.cfg at batch 32 on 416 x 416, 416 x 320 (4:3) and 416 x 256 (16:9),
and for yolov3-tiny-12 on the same sizes, in fp32 and bf16.

One process.  Per (network, dtype) the sizes are timed in blocks of ``--steps`` steps whose order rotates by one every repeat
(``--repeats`` repeats), device synchronised around every block; before the first block every variant runs ``--warmup`` steps
(plans, the autotuner's measurements for the new shapes, the allocator) and the GPU gets a second of sustained load.  Printed:
median (min .. max) of the blocks in ms per step, frames/s, the ratio to 416 x 416 beside the ratio of the derived FLOPs
(``plan.conv_flops``: 2 n ho wo cout k^2 cin per layer, exactly proportional to H * W), and the gap between the two.

The 416 x 416 leg is the square plan - the only way the parent commit has to process such a frame (letterboxed); compare it with
``python bench.py`` / ``python bench.py --dtype bf16`` of the parent on the same box (README: +/- 4 % box to box) before relying
on the other rows."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from millieye_amd import cfgs, synth  # noqa: E402
from millieye_amd.my_models import Network  # noqa: E402
from millieye_amd.yolov3.models import Darknet  # noqa: E402

SIZES = [(416, 416), (416, 320), (416, 256)]
CONF = 0.2


def timed_rotating(fns, steps, repeats):
    """A block of every variant per repeat, the order rotating by one every repeat (tools/multistream_latency.py's protocol).
    Returns per variant the list of its blocks' seconds per step."""
    out = [[] for _ in fns]
    k = len(fns)
    for r in range(repeats):
        for i in [(r + j) % k for j in range(k)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fns[i]()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t0) / steps)
    return out


def build(cfg, batch, dev):
    net = Network(Darknet(cfgs.write_cfg(cfg, os.path.join(tempfile.gettempdir(), f"millieye_rect_lat_{os.getuid()}"))),
                  CONF).eval()
    synth.fill_network_(net, "bench/" + cfg, cls0_bias=3.0, cls_bias=-4.0)   # bench.py's full workload
    net = net.to(dev)
    frames = torch.from_numpy(synth.uniform("bench/frames/0", (batch, 3, 416, 416)))
    maps_np, boxes_np = synth.radar_inputs("bench/radar/0", batch, 416 // 16, boxes_per_image=2)
    variants = []
    for h, w in SIZES:
        x = frames[:, :, :h, :w].contiguous().to(dev)
        maps = torch.from_numpy(maps_np)[:, :, : h // 16, : w // 16].contiguous().to(dev)
        boxes = torch.from_numpy(boxes_np).to(dev)
        variants.append((h, w, x, maps, boxes))
    return net, variants


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--cfgs", nargs="+", default=["yolov3", "yolov3-tiny-12"])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:   # (written as the run goes: a run that is cut short leaves what it measured)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say(f"# {torch.cuda.get_device_name(0)}; Network.forward mode 0 (detector -> NMS -> heads), batch {args.batch}; {args.steps} steps "
        f"per block, {args.repeats} blocks per size in rotating order, median (min .. max) of the blocks; {args.warmup} warm-up steps per "
        f"size first - the autotuner (MILLIEYE_AUTOTUNE, on by default) measures the tiles of every new shape during them - then 1 s "
        f"of untimed load")
    say("# FLOP ratio: derived (plan.conv_flops, proportional to H * W), not measured; gap = measured ratio / FLOP ratio - 1")
    for cfg in args.cfgs:
        net, variants = build(cfg, args.batch, dev)
        for dtype in args.dtypes:
            net.base_detector.compute_dtype = dtype
            fns, flops, rows = [], [], []

            def make(x, maps, boxes):
                def step():
                    with torch.no_grad():
                        return net(x, maps, boxes.clone(), 0)   # forward scales the radar boxes in place
                return step

            for h, w, x, maps, boxes in variants:
                fn = make(x, maps, boxes)
                for _ in range(args.warmup):
                    out = fn()
                torch.cuda.synchronize()
                plan = net.base_detector.engine_for(dtype).plan_for(x)
                fns.append(fn)
                flops.append(plan.conv_flops / args.batch)
                rows.append(int(out.shape[0]))
            t_end = time.perf_counter() + 1.0
            while time.perf_counter() < t_end:   # clocks: sustained load before the first timed block
                fns[0]()
                torch.cuda.synchronize()
            blocks = timed_rotating(fns, args.steps, args.repeats)
            base = statistics.median(blocks[0])
            for (h, w, *_), b, fl, nrows in zip(variants, blocks, flops, rows):
                med = statistics.median(b)
                ratio, fratio = med / base, fl / flops[0]
                say(f"{cfg:15s} {dtype:4s} {h} x {w}: {med * 1e3:8.3f} ({min(b) * 1e3:8.3f} .. {max(b) * 1e3:8.3f}) ms/step | "
                    f"{args.batch / med:8.1f} frames/s | ratio to 416 x 416 {ratio:5.3f} | FLOP ratio {fratio:5.3f} "
                    f"({fl / 1e9:6.2f} GFLOP/frame) | gap {(ratio / fratio - 1) * 100:+5.1f} % | {nrows} output rows")
        net.base_detector.compute_dtype = "f32"
        del net, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
