"""What drawing the detections onto the frames costs (millieye_amd.demo.MultiStreamFuser(overlay=), csrc/frame_overlay.hip):
python tools/frame_overlay_latency.py [--steps 200] [--streams 1 8 32] [--out profiles/frame_overlay_latency.txt]  (GPU box)

One process, one GPU, the protocol of tools/box_ranges_latency.py: warm-up first, the device synchronised around every timed
block, variants in blocks whose order alternates (A B, B A, ...), the median of the blocks with their smallest and largest.
The load is that tool's (the radar chain's proposals and walking people, about 8 rows per stream), brought from its 480 x 640
frames to 1080 x 1920 ones: the tail's rescale scalars are those of a 1080 x 1920 frame and the radar points move with the
boxes (u * 3, v * 3 - 180).  The pictures are device-resident surfaces, drawn in place: ``nv12`` as a decoder leaves it (pitch
2048, the chroma plane behind 1088 rows) and packed ``rgb``.
Per S and format:
  (a) the output tail with tracks and ranging, with the overlay (``hip.stream_tail_overlay``) and without
      (``hip.stream_tail_ranges``) on the same network rows, and their difference; beside it what the tracker adds to a tail
      with ranging alone, measured the same way in the same run;
  (b) the overlay launch alone (HIP events around back-to-back launches): on a tail without rows (validation and the item
      phase's fixed cost), boxes without labels, boxes with labels, and 64 boxes with labels in every stream.
No bar was fixed in advance."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from millieye_amd import hip  # noqa: E402
from millieye_amd.demo import MultiStreamFuser  # noqa: E402
from millieye_amd.detection_range import DeviceDetectionRanges  # noqa: E402
from millieye_amd.detection_tracks import DeviceDetectionTracks  # noqa: E402
from millieye_amd.frame_overlay import DeviceFrameOverlay  # noqa: E402
from millieye_amd.utils.datasets import FrameSurface  # noqa: E402
from tests import box_tracks_refs as br  # noqa: E402
from tests.golden.make_golden import RADAR_CALIB  # noqa: E402
from tools.box_ranges_latency import scenes  # noqa: E402
from tools.box_tracks_latency import BLOCKS, blocks_ab, device_events, ms  # noqa: E402

PICTURE_HW = (1080, 1920)


def surfaces(S, fmt, dev):
    h, w = PICTURE_HW
    if fmt == "nv12":
        pitch, rows = 2048, 1088
        size = pitch * rows * 3 // 2
        buffers = [torch.full((size,), 90, dtype=torch.uint8, device=dev) for _ in range(S)]
        return [FrameSurface(b, h, w, "nv12", 0, pitch, pitch * rows, pitch) for b in buffers]
    buffers = [torch.full((h * w * 3,), 90, dtype=torch.uint8, device=dev) for _ in range(S)]
    return [FrameSurface(b, h, w, "rgb") for b in buffers]


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
    say(f"# python tools/frame_overlay_latency.py --steps {args.steps} --streams {' '.join(map(str, args.streams))}")
    say(f"# {torch.cuda.get_device_name(dev)}; {args.steps} steps per block, {BLOCKS} blocks per variant in alternating order, "
        f"median (smallest - largest block); one run, one GPU")
    say("# README: bench numbers move +/- 4 % from GPU box to GPU box; the block ranges below are the spread inside this run")
    for S in args.streams:
        steps = args.steps
        sc = scenes(S, steps, dev)
        for step in sc:   # the radar points follow the boxes into the 1080 x 1920 picture
            step["slots"][:, :, 0] *= 3.0
            step["slots"][:, :, 1] = step["slots"][:, :, 1] * 3.0 - 180.0
        fuser = MultiStreamFuser(None, RADAR_CALIB, S)
        fuser._device = dev
        fuser._tail(sc[0]["rows"], [PICTURE_HW] * S)   # (the rescale scalars of the picture sizes)
        scal = fuser._scalars[1]
        ranger = DeviceDetectionRanges(S, device=dev)
        trackers = [DeviceDetectionTracks(S, device=dev, min_hits=1) for _ in range(3)]

        def ranged(f):
            return hip.stream_tail_ranges(sc[f]["rows"], S, scal, 0.3, ranger, sc[f]["slots"], sc[f]["counts"])

        def tracked(f):
            return hip.stream_tail_ranges(sc[f]["rows"], S, scal, 0.3, ranger, sc[f]["slots"], sc[f]["counts"], tracker=trackers[0])

        for f in range(10):
            ranged(f % steps)
            tracked(f % steps)
        a, b = blocks_ab(ranged, tracked, steps)
        tracker_added = [y - x for x, y in zip(a, b)]
        say(f"S={S:2d}       tail with ranging {ms(a)} | with tracks as well {ms(b)} | the tracker adds {ms(tracker_added)}")
        for fmt in ("nv12", "rgb"):
            pictures = surfaces(S, fmt, dev)
            painter = DeviceFrameOverlay(S, device=dev)

            def plain(f):
                return hip.stream_tail_ranges(sc[f]["rows"], S, scal, 0.3, ranger, sc[f]["slots"], sc[f]["counts"], tracker=trackers[1])

            def drawn(f):
                return hip.stream_tail_overlay(sc[f]["rows"], S, scal, 0.3, painter, pictures, tracker=trackers[2],
                                               ranging=(ranger, sc[f]["slots"], sc[f]["counts"]))

            for f in range(10):
                plain(f % steps)
                drawn(f % steps)
            a, b = blocks_ab(plain, drawn, steps)
            added = [y - x for x, y in zip(a, b)]
            got = [drawn(f) for f in range(min(steps, 40))]
            dets = [len(r) for g in got for r in g[0]]
            ids = sum(int((t[:, 9] >= 0).sum()) for g in got for t in g[2])
            with_range = sum(int((r[:, 2] > 0).sum()) for g in got for r in g[4])
            assert all(st == 0 for g in got for st in g[-1])
            say(f"S={S:2d} {fmt:4s} (a) tail of a step with tracks and ranging, {np.mean(dets):.1f} boxes per stream ({min(dets)} - {max(dets)}), "
                f"{ids / max(sum(dets), 1):.0%} with an id, {with_range / max(sum(dets), 1):.0%} with a range: overlay=None {ms(a)} | "
                f"overlay=True {ms(b)} | added {ms(added)} | added / the tracker's {statistics.median(added) / statistics.median(tracker_added):.2f}")

            # (b) the launch alone
            host_rows = [[r.numpy() for r in g[0]] for g in got]
            n = len(host_rows)
            tails = [torch.from_numpy(br.tail_buffer(host_rows[f])[0]).to(dev) for f in range(n)]
            ms_of = [sum(len(r) for r in host_rows[f]) for f in range(n)]
            empty_tail = torch.from_numpy(br.tail_buffer([np.zeros((0, 7), np.float32)] * S)[0]).to(dev)
            full_rows = br.grid_rows(64, 900, spacing=2.0, size=400.0, origin=(960.0, 540.0))
            full_tail = torch.from_numpy(br.tail_buffer([full_rows] * S)[0]).to(dev)
            boxes_only = DeviceFrameOverlay(S, device=dev, labels=False)
            timings = []
            for name, fn in (("no rows", lambda f: painter.draw(empty_tail, 0, pictures)),
                             ("boxes", lambda f: boxes_only.draw(tails[f % n], ms_of[f % n], pictures)),
                             ("boxes and labels", lambda f: painter.draw(tails[f % n], ms_of[f % n], pictures)),
                             ("64 boxes and labels per stream", lambda f: painter.draw(full_tail, 64 * S, pictures))):
                device_events(fn, 10)
                timings.append(f"{name} {ms([device_events(fn, steps) for _ in range(BLOCKS)])}")
            assert painter.draw(full_tail, 64 * S, pictures).cpu().tolist() == [0] * S
            say(f"S={S:2d} {fmt:4s} (b) overlay launch alone, descriptor upload included (HIP events, back to back): " + " | ".join(timings))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
