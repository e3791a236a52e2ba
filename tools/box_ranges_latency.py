"""What radar ranges cost (millieye_amd.demo.MultiStreamFuser(ranging=), csrc/box_ranges.hip) against the host loop:
python tools/box_ranges_latency.py [--steps 200] [--streams 1 8 32] [--out profiles/box_ranges_latency.txt]  (GPU box)

One process, one GPU, the protocol of tools/box_tracks_latency.py: warm-up first, the device synchronised around every timed
block, variants in blocks whose order alternates (A B, B A, ...), the median of the blocks with their smallest and largest.
The load is that of tools/multistream_latency.py's scenes: every stream's radar frames are ``radar_points((f + 7 * s) % 45)``
through the device radar chain (its kept points stay where ``DeviceRadarProposals`` keeps them), the detections are the
chain's own pixel proposals of the step (boxes that hold returns) and people walking through the 480 x 640 frame
(tests/box_tracks_refs.scene), 4 - 12 rows per stream.
Per S:
  (a) the output tail with ranging (``hip.stream_tail_ranges``) and without (``hip.stream_tail``) on the same network rows -
      device rows in, per-stream host rows out, the one place where the two steps differ - and their difference;
  (b) the ranging launch alone (HIP events around back-to-back launches) at that load and with 64 detections per stream that
      all hold all 256 points of their stream;
  (c) ``detection_range.range_detections`` on the host, one call per stream, on the rows and clouds (a) brought to the host.
Then the A/B of (a) on the whole step of the demo network (yolov3-tiny-12, fp32).  The last line compares (a) added with (c)
at the largest S; no bar was fixed in advance."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from millieye_amd import hip, synth  # noqa: E402
from millieye_amd.demo import MultiStreamFuser  # noqa: E402
from millieye_amd.detection_range import DeviceDetectionRanges, range_detections  # noqa: E402
from millieye_amd.radar_proposals import DeviceRadarProposals  # noqa: E402
from tests import box_tracks_refs as br  # noqa: E402
from tests.golden.make_golden import RADAR_CALIB, radar_points  # noqa: E402
from tools.box_tracks_latency import BLOCKS, FRAME_HW, blocks_ab, blocks_one, demo_net, device_events, ms  # noqa: E402


def scenes(S, steps, dev):
    """Per step: the network rows [m,8] on the device, the cloud slots and counts of the radar chain (clones), and for the
    host loop the clouds as numpy arrays."""
    gen = DeviceRadarProposals(RADAR_CALIB, S, min_hits=1, device=dev)
    walks = [br.scene(500 + s, steps=40, people=4) for s in range(S)]
    scale, pad = 416.0 / max(FRAME_HW), (max(FRAME_HW) - min(FRAME_HW)) / 2 * 416.0 / max(FRAME_HW)
    out = []
    for f in range(steps):
        gen.gen([[radar_points((f + 7 * s) % 45)] for s in range(S)], [FRAME_HW] * S)
        rows = []
        for s in range(S):
            prop = gen.proposals(s).astype(np.float32)
            prop = np.concatenate([prop, np.full((len(prop), 1), 0.9, np.float32), np.full((len(prop), 1), 0.9, np.float32),
                                   np.full((len(prop), 1), 2.0, np.float32)], 1)
            r = np.concatenate([prop, walks[s][f % 40]], 0)
            net = np.concatenate([np.full((len(r), 1), s, np.float32), r], 1)
            net[:, 1:5] *= scale
            net[:, [2, 4]] += pad
            rows.append(net)
        out.append(dict(rows=torch.from_numpy(np.concatenate(rows, 0).astype(np.float32)).to(dev),
                        slots=gen._cloud_slots.clone(), counts=gen._counts.clone(),
                        clouds=[gen.cloud(s) for s in range(S)]))
    return out


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
    say(f"# python tools/box_ranges_latency.py --steps {args.steps} --streams {' '.join(map(str, args.streams))}")
    say(f"# {torch.cuda.get_device_name(dev)}; {args.steps} steps per block, {BLOCKS} blocks per variant in alternating order, "
        f"median (smallest - largest block); one run, one GPU")
    say("# README: bench numbers move +/- 4 % from GPU box to GPU box; the block ranges below are the spread inside this run")
    say("# for comparison: the tracker adds 0.02 - 0.07 ms to the tail (S = 1 .. 32, profiles/box_tracks_latency.txt)")
    net = demo_net()
    verdict = None
    for S in args.streams:
        steps = args.steps
        sc = scenes(S, steps, dev)
        fuser = MultiStreamFuser(None, RADAR_CALIB, S)
        fuser._device = dev
        fuser._tail(sc[0]["rows"], [FRAME_HW] * S)   # (the rescale scalars of the frame sizes)
        scal = fuser._scalars[1]
        ranger = DeviceDetectionRanges(S, device=dev)

        def plain(f):
            return hip.stream_tail(sc[f]["rows"], S, scal, 0.3)

        def ranged(f):
            return hip.stream_tail_ranges(sc[f]["rows"], S, scal, 0.3, ranger, sc[f]["slots"], sc[f]["counts"])

        for f in range(10):   # warm-up
            plain(f % steps)
            ranged(f % steps)
        a, b = blocks_ab(plain, ranged, steps)
        added = [y - x for x, y in zip(a, b)]
        got = [ranged(f) for f in range(steps)]
        dets = [len(r) for g in got for r in g[0]]
        points = [len(c) for f in range(steps) for c in sc[f]["clouds"]]
        with_range = sum(int((r[:, 2] > 0).sum()) for g in got for r in g[2])
        say(f"S={S:2d} (a) tail of a step, {np.mean(dets):.1f} detections ({min(dets)} - {max(dets)}) and {np.mean(points):.1f} points "
            f"({min(points)} - {max(points)}) per stream, {with_range / max(sum(dets), 1):.0%} of the detections get a range: "
            f"ranging=None {ms(a)} | ranging=True {ms(b)} | added {ms(added)}")

        # (c) the host loop on what came to the host; its results are the device's
        host_rows = [[r.numpy() for r in g[0]] for g in got]
        worst = 0.0
        for f in range(steps):
            for s in range(S):
                want = range_detections(host_rows[f][s], sc[f]["clouds"][s])
                if not np.array_equal(want, got[f][2][s], equal_nan=True):
                    worst = float("inf")

        def host_step(f):
            for s in range(S):
                range_detections(host_rows[f][s], sc[f]["clouds"][s])

        c = blocks_one(host_step, steps)
        say(f"S={S:2d} (c) range_detections on the host, {S} streams in a loop: {ms(c)} per step | (a) added / (c) = "
            f"{statistics.median(added) / statistics.median(c):.3f} | device rows {'bit-equal to' if worst == 0.0 else 'DIFFER from'} "
            f"the host's")
        if S == max(args.streams):
            verdict = (S, statistics.median(added), statistics.median(c), max(added), min(c))

        # (b) the launch alone: typical load, and 64 detections x 256 inside points in every stream
        tails = [torch.from_numpy(br.tail_buffer(host_rows[f])[0]).to(dev) for f in range(steps)]
        ms_of = [sum(len(r) for r in host_rows[f]) for f in range(steps)]
        out_r = torch.zeros((max(max(ms_of), 64 * S), 4), dtype=torch.float64, device=dev)
        out_s = torch.zeros((S,), dtype=torch.int32, device=dev)

        def launch(f):
            ranger.launch(tails[f], ms_of[f], sc[f]["slots"], sc[f]["counts"], out_r.data_ptr(), out_s.data_ptr())

        device_events(launch, 10)
        typical = [device_events(launch, steps) for _ in range(BLOCKS)]
        rng = np.random.default_rng(S)
        full_rows = br.grid_rows(64, 900, spacing=2.0, size=400.0, origin=(320.0, 240.0))
        full_tail = torch.from_numpy(br.tail_buffer([full_rows] * S)[0]).to(dev)
        full_cloud = np.stack([rng.uniform(300, 350, (S, 256)), rng.uniform(220, 270, (S, 256)),
                               np.round(rng.uniform(1, 9, (S, 256)), 1), rng.normal(0, 1, (S, 256))], 2)
        full_slots = torch.from_numpy(full_cloud).to(dev)
        full_counts = torch.zeros((S, 8), dtype=torch.int32, device=dev)
        full_counts[:, 1] = 256

        def launch_full(f):
            ranger.launch(full_tail, 64 * S, full_slots, full_counts, out_r.data_ptr(), out_s.data_ptr())

        device_events(launch_full, 4)
        cap = [device_events(launch_full, 40) for _ in range(BLOCKS)]
        inside = out_r[:64 * S, 3].cpu().numpy()
        assert (inside == 256).all() and (out_s.cpu().numpy() == 0).all(), (inside.min(), inside.max())
        say(f"S={S:2d} (b) ranging launch alone (HIP events, back to back): typical load {ms(typical)} | 64 detections per stream, "
            f"256 points inside each {ms(cap)}")

        # the whole step of the demo network, with and without ranging
        frames = [(synth.uniform(f"ms/frame{s}", FRAME_HW + (3,)) * 25).astype(np.uint8) for s in range(S)]
        radar = [[[radar_points((f + 7 * s) % 45)] for s in range(S)] for f in range(steps)]
        step_plain = MultiStreamFuser(net, RADAR_CALIB, S, model_mode=0)
        step_ranged = MultiStreamFuser(net, RADAR_CALIB, S, model_mode=0, ranging=True)
        n_step = max(10, steps // 4)
        for f in range(5):
            step_plain(frames, radar[f])
            res = step_ranged(frames, radar[f])
        n_dets = np.mean([len(r) for r, _i in res])
        a, b = blocks_ab(lambda f: step_plain(frames, radar[f]), lambda f: step_ranged(frames, radar[f]), n_step)
        say(f"S={S:2d}     whole step, yolov3-tiny-12 fp32, {n_dets:.1f} detections per stream, {n_step} steps per block: ranging=None "
            f"{ms(a)} | ranging=True {ms(b)} | difference of the medians {(statistics.median(b) - statistics.median(a)) * 1e3:+.3f} ms")
    if verdict:
        S, added, host, worst_added, best_host = verdict
        say(f"# at S={S}: (a) added {added * 1e3:.3f} ms {'<' if added < host else '>='} (c) host loop {host * 1e3:.3f} ms: the device path "
            f"is {'faster' if added < host else 'NOT faster'} than the host loop (largest added block {worst_added * 1e3:.3f} ms, "
            f"smallest host block {best_host * 1e3:.3f} ms)")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
