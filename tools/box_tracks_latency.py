"""What track ids cost (millieye_amd.demo.MultiStreamFuser(tracks=), csrc/box_tracks.hip) against a host tracker:
python tools/box_tracks_latency.py [--steps 200] [--streams 1 8 32] [--out profiles/box_tracks_latency.txt]  (GPU box)

One process, one GPU, the protocol of tools/multistream_latency.py: warm-up first, the device synchronised around every timed
block, variants in blocks whose order alternates (A B, B A, ...), the median of the blocks with their smallest and largest.
Per S:
  (a) the output tail of a fuser step with ``tracks=True`` and with ``tracks=None`` on the same network rows
      (``MultiStreamFuser._tail``: device rows in, per-stream host rows out - the one place where the two steps differ) and
      their difference, the added time of a step; the load is people walking through 480 x 640 frames
      (tests/box_tracks_refs.scene), 4 - 8 detections per stream and step.  Then the same A/B on the whole step of the
      demo network (yolov3-tiny-12, fp32), whose synthetic weights decide the load.
  (b) the tracker launch alone (HIP events around back-to-back launches) at that load and at capacity, 64 tracks x 64
      detections in every stream.
  (c) ``detection_tracks.DetectionTracker`` on the host, one per stream, fed the rows ``hip.stream_tail`` brought to the host.
The acceptance line compares (a) with (c) at the largest S."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from millieye_amd import cfgs, hip, synth  # noqa: E402
from millieye_amd.demo import MultiStreamFuser  # noqa: E402
from millieye_amd.detection_tracks import DetectionTracker, DeviceDetectionTracks  # noqa: E402
from millieye_amd.my_models import Network  # noqa: E402
from millieye_amd.yolov3.models import Darknet  # noqa: E402
from tests import box_tracks_refs as br  # noqa: E402
from tests.golden.make_golden import RADAR_CALIB, radar_points  # noqa: E402

FRAME_HW = (480, 640)
BLOCKS = 4


def blocks_ab(fn_a, fn_b, steps, blocks=BLOCKS):
    """Seconds per step of two variants: ``blocks`` blocks of each in alternating order; returns the two lists."""
    a, b = [], []
    for r in range(blocks):
        for fn, out in (((fn_a, a), (fn_b, b)) if r % 2 == 0 else ((fn_b, b), (fn_a, a))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(steps):
                fn(f)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / steps)
    return a, b


def blocks_one(fn, steps, blocks=BLOCKS):
    return blocks_ab(fn, lambda f: None, steps, blocks)[0]


def ms(values):
    return f"{statistics.median(values) * 1e3:7.3f} ms ({min(values) * 1e3:.3f} - {max(values) * 1e3:.3f})"


def network_rows(S, steps, people=6):
    """Per step the network's rows [m,8] float32 (stream, box in 416-input units, p, cls_score, cls_pred) for S streams of
    walking people (scenes of 40 steps, repeated: at the seam the people of the last step leave and those of the first arrive),
    and the per-stream load."""
    scenes = [br.scene(500 + s, steps=40, people=people) for s in range(S)]
    scale, pad = 416.0 / max(FRAME_HW), (max(FRAME_HW) - min(FRAME_HW)) / 2 * 416.0 / max(FRAME_HW)
    out, load = [], []
    for f in range(steps):
        rows = []
        for s in range(S):
            r = scenes[s][f % 40]
            load.append(len(r))
            net = np.concatenate([np.full((len(r), 1), s, np.float32), r], 1)
            net[:, 1:5] *= scale
            net[:, [2, 4]] += pad
            rows.append(net)
        out.append(torch.from_numpy(np.concatenate(rows, 0).astype(np.float32)))
    return out, load


def device_events(fn, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for f in range(n):
        fn(f)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n * 1e-3


def demo_net():
    net = Network(Darknet(cfgs.write_cfg("yolov3-tiny-12", "/tmp/box_tracks_lat")), 0.2).eval()
    synth.fill_network_(net, "demo/yolov3-tiny-12", cls0_bias=3.0, cls_bias=-4.0)
    return net.to(net.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    hip.load()
    dev = hip.default_device()
    say(f"# python tools/box_tracks_latency.py --steps {args.steps} --streams {' '.join(map(str, args.streams))}")
    say(f"# {torch.cuda.get_device_name(dev)}; {args.steps} steps per block, {BLOCKS} blocks per variant in alternating order, "
        f"median (smallest - largest block); one run, one GPU")
    say("# README: bench numbers move +/- 4 % from GPU box to GPU box; the block ranges below are the spread inside this run")
    net = demo_net()
    verdict = None
    for S in args.streams:
        steps = args.steps
        rows, load = network_rows(S, steps)
        rows_dev = [r.to(dev) for r in rows]
        hws = [FRAME_HW] * S
        plain = MultiStreamFuser(None, RADAR_CALIB, S)
        tracked = MultiStreamFuser(None, RADAR_CALIB, S, tracks=True)
        plain._device = tracked._device = dev
        for f in range(10):   # warm-up
            plain._tail(rows_dev[f], hws)
            tracked._tail(rows_dev[f], hws)
        tracked.tracker.reset()
        a, b = blocks_ab(lambda f: plain._tail(rows_dev[f], hws), lambda f: tracked._tail(rows_dev[f], hws), steps)
        added = [y - x for x, y in zip(a, b)]
        live = int(tracked.tracker.host_counts[:, 2].sum())
        say(f"S={S:2d} (a) tail of a step, {np.mean(load):.1f} detections per stream ({min(load)} - {max(load)}), {live} live tracks "
            f"at the end: tracks=None {ms(a)} | tracks=True {ms(b)} | added {ms(added)}")

        # (c) the host tracker on the rows the tail brought to the host
        scal = plain._scalars[1]
        host_rows = [[r.numpy() for r in hip.stream_tail(rows_dev[f], S, scal, 0.3)[0]] for f in range(steps)]
        trackers = [DetectionTracker() for _ in range(S)]

        def host_step(f):
            for s in range(S):
                trackers[s].step(host_rows[f][s])

        c = blocks_one(host_step, steps)
        say(f"S={S:2d} (c) DetectionTracker on the host, {S} streams in a loop: {ms(c)} per step | (a) added / (c) = "
            f"{statistics.median(added) / statistics.median(c):.3f}")
        if S == max(args.streams):
            verdict = (S, statistics.median(added), statistics.median(c), max(added), min(c))

        # (b) the launch alone, typical load and capacity
        trk = DeviceDetectionTracks(S)
        tails = [torch.from_numpy(br.tail_buffer(host_rows[f])[0]).to(dev) for f in range(steps)]
        ms_of = [sum(len(r) for r in host_rows[f]) for f in range(steps)]
        device_events(lambda f: trk.launch(tails[f], ms_of[f]), 10)
        trk.reset()
        typical = [device_events(lambda f: trk.launch(tails[f], ms_of[f]), steps) for _ in range(BLOCKS)]
        full = [br.grid_rows(64, 900 + k, jitter=2.0) for k in range(8)]
        cap_tails = [torch.from_numpy(br.tail_buffer([full[(k + s) % 8] for s in range(S)])[0]).to(dev) for k in range(8)]
        trk.reset()
        device_events(lambda f: trk.launch(cap_tails[f % 8], 64 * S), 4)
        cap = [device_events(lambda f: trk.launch(cap_tails[f % 8], 64 * S), 40) for _ in range(BLOCKS)]
        counts = trk._counts.cpu().numpy()
        assert (counts[:, 0] == 0).all() and (counts[:, 2] == 64).all(), counts
        say(f"S={S:2d} (b) tracker launch alone (HIP events, back to back): typical load {ms(typical)} | capacity, 64 tracks x 64 "
            f"detections in every stream {ms(cap)}")

        # the whole step of the demo network, with and without tracks
        frames = [(synth.uniform(f"ms/frame{s}", FRAME_HW + (3,)) * 25).astype(np.uint8) for s in range(S)]
        radar = [[[radar_points((f + 7 * s) % 45)] for s in range(S)] for f in range(steps)]
        step_plain = MultiStreamFuser(net, RADAR_CALIB, S, model_mode=0)
        step_tracked = MultiStreamFuser(net, RADAR_CALIB, S, model_mode=0, tracks=True)
        n_step = max(10, steps // 4)
        for f in range(5):
            step_plain(frames, radar[f])
            got = step_tracked(frames, radar[f])
        dets = np.mean([len(r) for r, _i in got])
        a, b = blocks_ab(lambda f: step_plain(frames, radar[f]), lambda f: step_tracked(frames, radar[f]), n_step)
        say(f"S={S:2d}     whole step, yolov3-tiny-12 fp32, {dets:.1f} detections per stream, {n_step} steps per block: tracks=None "
            f"{ms(a)} | tracks=True {ms(b)} | difference of the medians {(statistics.median(b) - statistics.median(a)) * 1e3:+.3f} ms")
    if verdict:
        S, added, host, worst_added, best_host = verdict
        ok = added < host
        say(f"# acceptance at S={S}: (a) added {added * 1e3:.3f} ms {'<' if ok else '>='} (c) host {host * 1e3:.3f} ms: "
            f"{'PASS' if ok else 'FAIL'} (largest added block {worst_added * 1e3:.3f} ms, smallest host block {best_host * 1e3:.3f} ms)")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
