"""Latency of the multi-stream step (millieye_amd.demo.MultiStreamFuser) against S sequential FrameFuser calls on the same
inputs: python tools/multistream_latency.py [--steps 100] [--out profiles/multistream_latency.txt]  (GPU box)

Per (network, dtype, S): ms per step and frames/s of both paths (median of the repeats, warm-up first, device synchronised
around every timed region), the radar upload + the two proposal launches (HIP events around ``DeviceRadarProposals.launch``: the
host-side packing of the points and the copy are inside, so it bounds the launches' device time from above), one host
generator call for one stream, and the host time of a step before its first network launch.  The "dark" rows feed 480x640
frames that all select fusion (one ``Network.forward``, no gather); the "mixed" rows feed the tests' frames - two sizes, dark
and bright interleaved - so that every step takes the mode split: two forwards on gathered sub-batches.  The radar streams and
the float64 bar quoted in the first lines are those of tests/test_gpu_multistream.py (tests/multistream_helpers.py).

The output tail (``MultiStreamFuser(tail=...)``), both kinds in the same process, a block of each in every one of four repeats,
the order alternating (host device, device host, ...): "tail
alone" is ``_tail`` on the network's rows of one recorded step - from the device rows to the per-stream host rows, device
synchronised - and "step" the whole step with either tail.  The last lines run the S = max row through
``pipeline.FusionPipeline`` (two processes, every step inferred) against the in-process fuser: steps/s, the first step
(spawn, rendezvous) left out.

``--split frame_modes`` builds every fuser of those rows with ``MultiStreamFuser(split="frame_modes")`` (one forward with per-frame
modes); ``--split compare`` prints only the A/B of the two splits (:func:`compare_splits`; profiles/multistream_frame_modes.txt):
python tools/multistream_latency.py --split compare --streams 8 32 --steps 40 --out profiles/multistream_frame_modes.txt

``--pixel-format rgb nv12 yuyv`` prints only the comparison of the input formats (:func:`compare_formats`;
profiles/multistream_pixel_formats.txt): per network and S the bytes a step packs, the time from the packed payload to the device
batch, the whole in-process step and the two-process pipeline, every format in the same process, in blocks whose order rotates:
python tools/multistream_latency.py --pixel-format rgb nv12 yuyv --streams 8 32 --steps 40 --out profiles/multistream_pixel_formats.txt

``--resize nearest area`` prints only the comparison of the resize modes (:func:`compare_resize`; profiles/multistream_resize.txt):
per network, S, frame size (``--frame-size H W``, repeatable) and pixel format the bytes a step packs, the input launch's own time,
a device-to-device copy of the same packed buffer, the area launch's source-read rate as a fraction of that copy's, and the step:
python tools/multistream_latency.py --resize nearest area --frame-size 480 640 --frame-size 1080 1920 --streams 8 32 --steps 20 --out profiles/multistream_resize.txt

``--img-size H W`` (repeatable) prints only the comparison of network input sizes (:func:`compare_img_sizes`;
profiles/letterbox_inference.txt): per network, S and frame size the input launch alone, the packed payload to the device batch, the
radar-box rebuild with its count copy (rectangular sizes only), ``Network.forward`` alone and the whole step, every size in the same process, in rotating blocks:
python tools/multistream_latency.py --img-size 416 416 --img-size 256 416 --frame-size 1080 1920 --streams 8 --steps 40 --nets yolov3-tiny-12:f32 yolov3:f32 yolov3:bf16 --out profiles/letterbox_inference.txt

``--handover queue pinned`` prints only the comparison of the pipeline's hand-overs (:func:`compare_handover`;
profiles/multistream_handover.txt): per network, S, frame size and pixel format the pipeline's steps/s through the queue and through
the pinned ring, two passes each in opposite order, the in-process fuser's steps/s, the ratios, and where a consumer step goes:
python tools/multistream_latency.py --handover queue pinned --streams 8 32 --out profiles/multistream_handover.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from millieye_amd import cfgs, synth  # noqa: E402
from millieye_amd.demo import FrameFuser, MultiStreamFuser  # noqa: E402
from millieye_amd.my_models import Network  # noqa: E402
from millieye_amd.yolov3.models import Darknet  # noqa: E402
from tests import multistream_helpers as mh  # noqa: E402
from tests.golden.make_golden import RADAR_CALIB, radar_points  # noqa: E402


REPEATS = 3


class DarkSource:
    """Picklable source of the pipeline rows: ``steps`` steps of ``n`` dark 480x640 frames + the radar frames of ``main``."""

    def __init__(self, steps, n):
        self.steps, self.n = steps, n

    def __call__(self):
        frames = [(synth.uniform(f"ms/frame{s}", (480, 640, 3)) * 25).astype(np.uint8) for s in range(self.n)]
        for f in range(self.steps):
            yield frames, [[radar_points((f + 7 * s) % 45)] for s in range(self.n)]


def dark_native_frame(fmt, s, h=480, w=640):
    """Dark ``h x w`` frame of stream ``s`` the way a camera hands it over in ``fmt``: rgb / bgr bytes 0 .. 24 (the frames of the
    "dark" rows), luma 16 .. 40 under near-neutral chroma for nv12 ``[h*3//2, w]`` / yuyv ``[h,w,2]`` - all select fusion."""
    if fmt in ("rgb", "bgr"):
        return (synth.uniform(f"ms/frame{s}", (h, w, 3)) * 25).astype(np.uint8)
    luma = (16 + synth.uniform(f"ms/luma{s}", (h, w)) * 25).astype(np.uint8)
    if fmt == "nv12":
        chroma = (120 + synth.uniform(f"ms/chroma{s}", (h // 2, w)) * 17).astype(np.uint8)
        return np.concatenate([luma, chroma], 0)
    chroma = (120 + synth.uniform(f"ms/chroma{s}", (h, w)) * 17).astype(np.uint8)
    return np.stack([luma, chroma], -1)


class NativeDarkSource:
    """Picklable source of the pipeline rows of :func:`compare_formats`: ``steps`` steps of ``n`` dark frames in ``fmt``."""

    def __init__(self, steps, n, fmt):
        self.steps, self.n, self.fmt = steps, n, fmt

    def __call__(self):
        frames = [dark_native_frame(self.fmt, s) for s in range(self.n)]
        for f in range(self.steps):
            yield frames, [[radar_points((f + 7 * s) % 45)] for s in range(self.n)]


def timed_rotating(fns, steps, repeats):
    """``timed_ab`` for any number of variants: a block of each per repeat, the order rotating by one every repeat.  Returns per
    variant the list of its blocks' seconds per step."""
    out = [[] for _ in fns]
    k = len(fns)
    for r in range(repeats):
        for i in [(r + j) % k for j in range(k)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(steps):
                fns[i](f)
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t0) / steps)
    return out


def _spread(blocks, scale=1e3):
    return f"{statistics.median(blocks) * scale:7.3f} ({min(blocks) * scale:7.3f} .. {max(blocks) * scale:7.3f})"


def compare_formats(args, say):
    """``--pixel-format``: the input formats against the first one named (rgb) in one process.  Per network and S, every
    format's fuser sees frames of the same picture size (480x640, dark: one forward at batch S) and the same radar streams.

    bytes/step: what ``prepare(pack=True)`` packs - what the pipeline queues and the consumer uploads.  "to device": from that
    packed payload to the ``[S,3,416,416]`` batch on the device (``StagedRaggedImages.to``: the upload from pageable memory and the
    launch), device synchronised around every block.  "step": the whole in-process step from the caller's frames (``prepare``
    without packing, then ``infer``: the bytes are packed into pinned memory and uploaded).  "pipeline": ``FusionPipeline``, every
    step inferred, the first step (spawn, rendezvous) left out, one run per format and pass, the passes in opposite order."""
    fmts = args.pixel_format
    from millieye_amd.pipeline import FusionPipeline
    say(f"# {torch.cuda.get_device_name(0)}; 480x640 dark frames; {args.steps} steps per block, {args.repeats} blocks per format in "
        f"rotating order, median (min .. max) of the blocks in ms, 5 warm-up steps; pipeline: {args.steps} steps per run, "
        f"two passes in opposite order, steps/s of each")
    say("# not measured: the cvtColor pass on the host that an integrator with a YUV or BGR camera saves (cv2 is not installed)")
    for cfg, dtype in args.nets:
        net = _demo_net(cfg, dtype)
        for n in args.streams:
            radar = [[[radar_points((f + 7 * s) % 45)] for s in range(n)] for f in range(args.steps)]
            frames = {fmt: [dark_native_frame(fmt, s) for s in range(n)] for fmt in fmts}
            fusers = {fmt: MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, pixel_format=fmt) for fmt in fmts}
            payloads = {fmt: fusers[fmt].prepare(frames[fmt], radar[0], pack=True) for fmt in fmts}
            for f in range(5):
                for fmt in fmts:
                    out = fusers[fmt](frames[fmt], radar[f])
                    payloads[fmt]["img"].to(fusers[fmt].device)
            assert all(info["mode"] == 0 for _r, info in out)
            t_up = timed_rotating([lambda f, fmt=fmt: payloads[fmt]["img"].to(fusers[fmt].device) for fmt in fmts],
                                  args.steps, args.repeats)
            t_step = timed_rotating([lambda f, fmt=fmt: fusers[fmt](frames[fmt], radar[f]) for fmt in fmts],
                                    args.steps, args.repeats)
            pipe = {fmt: [] for fmt in fmts}
            if args.pipeline:
                for order in (fmts, fmts[::-1]):
                    for fmt in order:
                        piped = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, pixel_format=fmt)
                        t0, done = None, 0
                        for _results, _info in FusionPipeline(piped, NativeDarkSource(args.steps + 1, n, fmt), skip_to_newest=False):
                            if t0 is None:
                                torch.cuda.synchronize()
                                t0 = time.perf_counter()
                            else:
                                done += 1
                        pipe[fmt].append(done / (time.perf_counter() - t0))
            for i, fmt in enumerate(fmts):
                nbytes = int(payloads[fmt]["img"].packed.numel())
                base = int(payloads[fmts[0]]["img"].packed.numel())
                med_up, med_step = statistics.median(t_up[i]), statistics.median(t_step[i])
                line = (f"{cfg:16s} {dtype:4s} S={n:2d} {fmt:4s}: {nbytes / 1e6:6.2f} MB/step (x {nbytes / base:4.2f}) | to device "
                        f"{_spread(t_up[i])} ms ({(med_up / statistics.median(t_up[0]) - 1) * 100:+6.1f} %) | step "
                        f"{_spread(t_step[i])} ms ({(med_step / statistics.median(t_step[0]) - 1) * 100:+6.1f} %)")
                if pipe[fmt]:
                    best = max(pipe[fmt])
                    line += (f" | pipeline {', '.join(f'{v:6.1f}' for v in pipe[fmt])} steps/s, ratio to the in-process step "
                             f"{', '.join(f'{v * med_step:4.2f}' for v in pipe[fmt])} (x {best / max(pipe[fmts[0]]):4.2f} of {fmts[0]})")
                say(line)


def handover_frames(fmt, n, hw):
    """``n`` dark ``hw`` frames in ``fmt`` for :func:`compare_handover`: four distinct pictures, repeated over the streams (the
    bytes are copied per stream all the same; generating 32 distinct 1080p frames would take longer than the run)."""
    base = [dark_native_frame(fmt, s, *hw) for s in range(min(n, 4))]
    return [base[s % len(base)] for s in range(n)]


class HandoverSource:
    """Picklable source of :func:`compare_handover`: ``steps`` steps of :func:`handover_frames`."""

    def __init__(self, steps, n, fmt, hw):
        self.steps, self.n, self.fmt, self.hw = steps, n, fmt, tuple(hw)

    def __call__(self):
        frames = handover_frames(self.fmt, self.n, self.hw)
        for f in range(self.steps):
            yield frames, [[radar_points((f + 7 * s) % 45)] for s in range(self.n)]


class _PhasedInfer:
    """``infer=`` of a measured pipeline run: ``fuser.infer`` with three clocks and no added synchronisation.  Per step: the
    time since the previous ``infer`` returned (the slot's return, the caller's loop and the wait for the next payload), the host
    time inside ``payload["img"].to()`` with the device time between two events around it (the upload and the input launch), and
    the rest of ``infer``."""

    def __init__(self, fuser):
        self.fuser, self.rows, self.last = fuser, [], None
        self.events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def __call__(self, payload):
        t0 = time.perf_counter()
        wait = None if self.last is None else t0 - self.last
        img, rec = payload["img"], {}
        e0, e1 = self.events

        def to(device, *a, **k):
            e0.record()
            a0 = time.perf_counter()
            out = type(img).to(img, device, *a, **k)
            rec["host"] = time.perf_counter() - a0
            e1.record()
            return out
        img.to = to
        try:
            results = self.fuser.infer(payload)
        finally:
            del img.to
        t1 = time.perf_counter()
        e1.synchronize()
        if wait is not None:     # (the first step - spawn, rendezvous, plans - is left out)
            self.rows.append((wait, rec["host"], e0.elapsed_time(e1) * 1e-3, t1 - t0 - rec["host"]))
        self.last = time.perf_counter()
        return results

    def medians(self):
        return [statistics.median(col) * 1e3 for col in zip(*self.rows)]


def compare_handover(args, say):
    """``--handover queue pinned``: the two hand-overs of ``FusionPipeline`` - ``queue``: ``handover=None``, every step's bytes
    through the queue's shared memory and up from pageable memory; ``pinned``: ``handover="pinned"``, the bytes packed into a
    registered ``handover.FrameRing`` slot and up from there - against each other and against the in-process fuser.  Per
    network, S, frame size (``--frame-size``, repeatable) and pixel format: dark frames (one forward at batch S), every step
    inferred, two passes per mode in opposite order, steps/s of each from the first step's result (spawn, rendezvous: left out) to
    the last one's - "with the teardown": to the end of the iteration, which adds the producer's exit (a fixed 0.5 - 1 s per run,
    a third of a 100-step run; the two-process rows of the other modes of this tool include it); the
    in-process fuser's steps/s (median of ``REPEATS`` blocks) and every pass's ratio to it; "bar": the gain of ``pinned`` over
    ``queue`` (means of the passes) against the larger pass-to-pass spread of the two modes.  The second line of a row holds
    per mode the medians over the consumer's steps of both passes of the phases of :class:`_PhasedInfer`."""
    from millieye_amd.handover import FrameRing
    from millieye_amd.pipeline import FusionPipeline
    modes = args.handover
    sizes = [tuple(v) for v in (args.frame_size or [(480, 640), (1080, 1920)])]
    fmts = args.pixel_format or ["rgb", "nv12"]
    say(f"# {torch.cuda.get_device_name(0)}; dark frames; pipeline: {args.steps} steps per run, every step inferred, timed from the "
        f"first step's result to the last one's, two passes per hand-over in opposite order; in-process: {args.steps} steps per block, median of {REPEATS} blocks, "
        f"5 warm-up steps")
    probe = FrameRing(2, 1 << 20)
    status = probe.register()
    say(f"# hipHostRegister of a 2 x 1 MiB ring: status {status}; torch reports slot.is_pinned() = {probe.slot(1).is_pinned()}")
    probe.close()
    for cfg, dtype in args.nets:
        net = _demo_net(cfg, dtype)
        for n in args.streams:
            for hw in sizes:
                for fmt in fmts:
                    radar = [[[radar_points((f + 7 * s) % 45)] for s in range(n)] for f in range(args.steps)]
                    frames = handover_frames(fmt, n, hw)
                    pixfmt = None if fmt == "rgb" else fmt      # (rgb: the default path, the one the earlier pipeline rows ran)
                    local = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, pixel_format=pixfmt)
                    for f in range(5):
                        out = local(frames, radar[f])
                    assert all(info["mode"] == 0 for _r, info in out)
                    t_local = timed(lambda f: local(frames, radar[f]), args.steps)
                    nbytes = int(local.prepare(frames, radar[0], pack=True)["img"].packed.numel())
                    rate, whole, phases, stats = {m: [] for m in modes}, {m: [] for m in modes}, {}, {}
                    for order in (modes, modes[::-1]):
                        for mode in order:
                            piped = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, pixel_format=pixfmt)
                            infer = phases.setdefault(mode, _PhasedInfer(piped))
                            infer.fuser, infer.last = piped, None
                            pipe = FusionPipeline(piped, HandoverSource(args.steps + 1, n, fmt, hw), infer=infer,
                                                  skip_to_newest=False, handover=None if mode == "queue" else mode)
                            t0, done = None, 0
                            for _results, _info in pipe:
                                if t0 is None:
                                    torch.cuda.synchronize()
                                    t0 = time.perf_counter()
                                else:
                                    done += 1
                                    t_last = time.perf_counter()
                            rate[mode].append(done / (t_last - t0))
                            whole[mode].append(done / (time.perf_counter() - t0))
                            stats[mode] = pipe.stats
                    head = f"{cfg:16s} {dtype:4s} S={n:2d} {hw[0]:4d}x{hw[1]:<4d} {fmt:4s}"
                    line = f"{head}: {nbytes / 1e6:7.2f} MB/step | in-process {1 / t_local:6.1f} steps/s"
                    for mode in modes:
                        line += (f" | {mode} {', '.join(f'{v:6.1f}' for v in rate[mode])} steps/s (x "
                                 f"{', '.join(f'{v * t_local:4.2f}' for v in rate[mode])} of in-process; with the teardown "
                                 f"{', '.join(f'{v:5.1f}' for v in whole[mode])})")
                    if "queue" in rate and "pinned" in rate:
                        mean = {m: statistics.mean(rate[m]) for m in modes}
                        spread = max(max(rate[m]) - min(rate[m]) for m in modes)
                        gain = mean["pinned"] - mean["queue"]
                        line += (f" | pinned / queue x {mean['pinned'] / mean['queue']:4.2f}; bar: gain {gain:+6.1f} steps/s against "
                                 f"a spread of {spread:5.1f}: {'cleared' if gain > spread else 'NOT cleared'}")
                        fallback = stats["pinned"].get("handover_fallback")
                        if fallback:
                            line += f" ({fallback} steps fell back to the queue)"
                    say(line)
                    say(f"{head}: per consumer step, median ms: " + " | ".join(
                        "{} wait {:6.2f}, to() host {:6.2f} / device {:6.2f}, rest of infer {:6.2f}".format(m, *phases[m].medians())
                        for m in modes))


def compare_resize(args, say):
    """``--resize``: the resize modes of ``MultiStreamFuser(resize=)`` against the first one named (nearest) in one process, in
    rotating blocks like :func:`compare_formats`.  Per network, S, frame size (``--frame-size``, repeatable) and pixel format
    (``--pixel-format``, default rgb nv12), every mode's fuser sees the same dark frames and radar streams.

    bytes/step: what ``prepare(pack=True)`` packs.  "launch": the input launch alone on buffers that are already on the device -
    HIP events around a block of back-to-back launches, divided by their number; the sources rotate over a ring of copies of the
    packed buffer of about 1 GB (at most 16), so that a launch does not find its source in the Infinity Cache where the ring is
    larger than it.  "copy": ``copy_`` of the same packed buffers device to device over the same ring, the same way; "of copy" is
    copy time / launch time of the area mode = its source-read rate as a fraction of the copy's rate (the copy also writes what
    it reads; the area launch writes ``S x 3 x 416 x 416`` floats).  "step": the whole in-process step from the caller's frames."""
    from millieye_amd import hip
    modes = args.resize
    fmts = args.pixel_format or ["rgb", "nv12"]
    sizes = [tuple(v) for v in (args.frame_size or [[480, 640]])]
    say(f"# {torch.cuda.get_device_name(0)}; dark frames; {args.steps} steps (launches, copies) per block, {args.repeats} blocks per "
        f"mode in rotating order, median (min .. max) of the blocks, 5 warm-up steps")
    entry = {"nearest": "me_image_batch_formats_u8_f32", "area": "me_image_batch_area_u8_f32"}
    for cfg, dtype in args.nets:
        net = _demo_net(cfg, dtype)
        for n in args.streams:
            radar = [[[radar_points((f + 7 * s) % 45)] for s in range(n)] for f in range(args.steps)]
            for h, w in sizes:
                for fmt in fmts:
                    distinct = [dark_native_frame(fmt, s, h, w) for s in range(min(n, 4))]   # (four pictures, in turn)
                    frames = [distinct[s % len(distinct)] for s in range(n)]
                    fusers = {m: MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, pixel_format=fmt, resize=m)
                              for m in modes}
                    payload = fusers[modes[0]].prepare(frames, radar[0], pack=True)
                    packed, desc = payload["img"].packed, payload["img"].desc
                    nbytes = int(packed.numel())
                    dev = fusers[modes[0]].device
                    ring = [packed.to(dev) for _ in range(max(1, min(16, -(-(1 << 30) // nbytes))))]
                    spare = torch.empty_like(ring[0])
                    d_desc = desc.to(dev)
                    out = torch.empty((n, 3, 416, 416), device=dev, dtype=torch.float32)
                    lib, stream = hip.lib(), hip.stream_ptr()

                    def launches(mode):
                        fn = getattr(lib, entry[mode])
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        a.record()
                        for f in range(args.steps):
                            hip.check(fn(ring[f % len(ring)].data_ptr(), nbytes, d_desc.data_ptr(), n, out.data_ptr(), 416, stream),
                                      entry[mode])
                        b.record()
                        torch.cuda.synchronize()
                        return a.elapsed_time(b) * 1e-3 / args.steps

                    def copies(_mode):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        a.record()
                        for f in range(args.steps):
                            spare.copy_(ring[f % len(ring)])
                        b.record()
                        torch.cuda.synchronize()
                        return a.elapsed_time(b) * 1e-3 / args.steps

                    for f in range(5):
                        for m in modes:
                            res = fusers[m](frames, radar[f])
                    assert all(info["mode"] == 0 for _r, info in res)
                    variants = [("launch", m) for m in modes] + [("copy", None)]
                    for kind, m in variants:
                        (launches if kind == "launch" else copies)(m)
                    t_dev = [[] for _ in variants]
                    for r in range(args.repeats):
                        for i in [(r + j) % len(variants) for j in range(len(variants))]:
                            kind, m = variants[i]
                            t_dev[i].append((launches if kind == "launch" else copies)(m))
                    t_step = timed_rotating([lambda f, m=m: fusers[m](frames, radar[f]) for m in modes], args.steps, args.repeats)
                    t_copy = statistics.median(t_dev[-1])
                    for i, m in enumerate(modes):
                        t_launch = statistics.median(t_dev[i])
                        line = (f"{cfg:16s} {dtype:4s} S={n:2d} {h}x{w} {fmt:4s} {m:7s}: {nbytes / 1e6:7.2f} MB/step, ring of {len(ring):2d} | "
                                f"launch {_spread(t_dev[i], 1e6)} us | copy {_spread(t_dev[-1], 1e6)} us")
                        if m == "area":
                            line += f" | source read {nbytes / t_launch / 1e9:7.1f} GB/s = {t_copy / t_launch:4.2f} of copy"
                        line += (f" | step {_spread(t_step[i])} ms "
                                 f"({(statistics.median(t_step[i]) / statistics.median(t_step[0]) - 1) * 100:+6.1f} %)")
                        say(line)
                    del ring, spare, out


def compare_img_sizes(args, say):
    """``--img-size``: ``MultiStreamFuser(img_size=)`` for every size named, the first one (the square path) as the yardstick,
    in one process and rotating blocks.  Every fuser sees the same dark RGB frames (``--frame-size``, default 1080 1920: one
    fusion forward at batch S) and radar streams.

    "launch": the input launch alone on buffers already on the device (HIP events around a block of back-to-back launches over a
    ring of copies of the packed buffer, as in :func:`compare_resize`) - ``me_image_batch_pad_resize_flip_u8_f32`` for a square
    size, ``me_image_batch_letterbox_u8_f32`` for a rectangular one.  "boxes": ``DeviceRadarProposals.letterbox_boxes`` - two
    launches and the copy of S + 1 counts, the call a rectangular step adds (host time, it synchronises).  "to device": from the
    packed payload to the batch on the device (the upload of the frames' bytes from pageable memory and the launch, device
    synchronised around every block).  "forward": ``Network.forward`` in the fusion mode on the step's own inputs, HIP events.
    "step": the whole in-process step from the caller's frames (packing into pinned memory, upload, radar chain, maps, boxes,
    mode rule, forward, tail)."""
    from millieye_amd import hip
    sizes = [h if h == w else (h, w) for h, w in args.img_size]
    frame_sizes = [tuple(v) for v in (args.frame_size or [[1080, 1920]])]
    say(f"# {torch.cuda.get_device_name(0)}; dark rgb frames; {args.steps} steps (launches) per block, {args.repeats} blocks per size "
        f"in rotating order, median (min .. max) of the blocks, 5 warm-up steps")
    for cfg, dtype in args.nets:
        net = _demo_net(cfg, dtype)
        for n in args.streams:
            radar = [[[radar_points((f + 7 * s) % 45)] for s in range(n)] for f in range(args.steps)]
            for h, w in frame_sizes:
                distinct = [dark_native_frame("rgb", s, h, w) for s in range(min(n, 4))]
                frames = [distinct[s % len(distinct)] for s in range(n)]
                fusers = [MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, img_size=size) for size in sizes]
                dev = fusers[0].device
                lib, stream = hip.lib(), hip.stream_ptr()
                staged = [fuser.prepare(frames, radar[0], pack=True)["img"] for fuser in fusers]
                nbytes = int(staged[0].packed.numel())
                ring = [staged[0].packed.to(dev) for _ in range(max(1, min(16, -(-(1 << 30) // nbytes))))]
                descs = [st.desc.to(dev) for st in staged]
                outs = [torch.empty(tuple(st.shape), device=dev, dtype=torch.float32) for st in staged]

                def launches(i):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for f in range(args.steps):
                        src = ring[f % len(ring)].data_ptr()
                        if fusers[i].rect:
                            H, W = sizes[i]
                            hip.check(lib.me_image_batch_letterbox_u8_f32(src, nbytes, descs[i].data_ptr(), n, outs[i].data_ptr(),
                                                                          H, W, stream), "me_image_batch_letterbox_u8_f32")
                        else:
                            hip.check(lib.me_image_batch_pad_resize_flip_u8_f32(src, nbytes, descs[i].data_ptr(), n,
                                                                                outs[i].data_ptr(), sizes[i], stream),
                                      "me_image_batch_pad_resize_flip_u8_f32")
                    b.record()
                    torch.cuda.synchronize()
                    return a.elapsed_time(b) * 1e-3 / args.steps

                inputs = []
                for i, fuser in enumerate(fusers):
                    for f in range(5):
                        res = fuser(frames, radar[f])
                    assert all(info["mode"] == 0 for _r, info in res)
                    gen = fuser.generator
                    if fuser.rect:
                        inputs.append((staged[i].to(dev), gen.heatmaps((sizes[i][0] // 16, sizes[i][1] // 16)),
                                       gen.letterbox_boxes(sizes[i])[0]))
                    else:
                        step = gen.gen(radar[5], [(h, w)] * n)
                        inputs.append((staged[i].to(dev), gen.heatmaps(32), step.radar_box))
                    launches(i)

                def forwards(i):
                    img, radar_map, radar_box = inputs[i]
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    with torch.no_grad():
                        for f in range(args.steps):
                            net(img, radar_map, radar_box.clone(), 0)
                    b.record()
                    torch.cuda.synchronize()
                    return a.elapsed_time(b) * 1e-3 / args.steps

                t_launch, t_fwd = [[] for _ in sizes], [[] for _ in sizes]
                for r in range(args.repeats):
                    for i in [(r + j) % len(sizes) for j in range(len(sizes))]:
                        t_launch[i].append(launches(i))
                        t_fwd[i].append(forwards(i))
                t_step = timed_rotating([lambda f, i=i: fusers[i](frames, radar[f]) for i in range(len(sizes))], args.steps,
                                        args.repeats)
                t_up = timed_rotating([lambda f, i=i: staged[i].to(dev) for i in range(len(sizes))], args.steps, args.repeats)
                for i, size in enumerate(sizes):
                    name = f"{size[0]}x{size[1]}" if fusers[i].rect else f"{size}x{size}"
                    line = (f"{cfg:16s} {dtype:4s} S={n:2d} {h}x{w} -> {name:9s}: {nbytes / 1e6:6.2f} MB/step | launch "
                            f"{_spread(t_launch[i], 1e6)} us | to device {_spread(t_up[i])} ms | forward {_spread(t_fwd[i])} ms "
                            f"(x {statistics.median(t_fwd[i]) / statistics.median(t_fwd[0]):5.3f}) | step {_spread(t_step[i])} ms "
                            f"(x {statistics.median(t_step[i]) / statistics.median(t_step[0]):5.3f})")
                    if fusers[i].rect:
                        gen = fusers[i].generator
                        t_box = timed_rotating([lambda f: gen.letterbox_boxes(sizes[i])], args.steps, args.repeats)[0]
                        line += f" | boxes + count copy {_spread(t_box, 1e6)} us"
                    say(line)
                del ring, outs, inputs


def timed_ab(fn_a, fn_b, steps, repeats=4):
    """``timed`` for two variants, a block of each per repeat in alternating order (A B, B A, ...), so that both see the same
    machine state and neither always runs first."""
    a, b = [], []
    for r in range(repeats):
        for fn, out in (((fn_a, a), (fn_b, b)) if r % 2 == 0 else ((fn_b, b), (fn_a, a))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(steps):
                fn(f)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / steps)
    return statistics.median(a), statistics.median(b)


def timed(fn, steps, repeats=REPEATS):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(steps):
            fn(f)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps)
    return statistics.median(out)


def _demo_net(cfg, dtype):
    net = Network(Darknet(cfgs.write_cfg(cfg, f"/tmp/ms_lat_{cfg}")), 0.2).eval()
    synth.fill_network_(net, "demo/" + cfg, cls0_bias=3.0, cls_bias=-4.0)
    net = net.to(net.device)
    net.base_detector.compute_dtype = dtype
    return net


def compare_splits(args, say):
    """``--split compare``: ``MultiStreamFuser(split="frame_modes")`` against ``split="forwards"`` (the yardstick) in one process.

    "mixed" rows: the tests' frames (two sizes, dark and bright interleaved, the dark count fixed), a block of each split in
    every one of four repeats, the order alternating.  "varying" rows: the number of dark streams changes every step, cycling
    over nine counts, from cold plan tables (the engines' plans are dropped first; the autotuner's per-layer choices made during
    the run stay cached, as in a long-running process); the time of every step counts, plan builds included, and the plans built
    are counted at ``DarknetEngine._build``.  Both fusers of a row see the same frames and radar streams."""
    say(f"# {torch.cuda.get_device_name(0)}; mixed: {args.steps} steps per block, median of 4 alternating blocks per split, "
        f"5 warm-up steps; varying: {args.vary_steps} steps per split, every step timed, device synchronised around the run")
    for cfg in args.cfgs:
        for dtype in ("f32", "bf16"):
            net = _demo_net(cfg, dtype)
            eng = net.base_detector.engine_for(dtype)
            for n in args.streams:
                frames = [mh.stream_frame(s) for s in range(n)]
                dark = sum(s % 3 != 0 for s in range(n))   # (tests.multistream_helpers.stream_frame)
                radar = [[[radar_points((f + 7 * s) % 45)] for s in range(n)] for f in range(max(args.steps, args.vary_steps))]
                fusers = {split: MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, split=split)
                          for split in ("forwards", "frame_modes")}
                for f in range(5):
                    for fuser in fusers.values():
                        fuser(frames, radar[f])
                t_fw, t_fm = timed_ab(lambda f: fusers["forwards"](frames, radar[f]),
                                      lambda f: fusers["frame_modes"](frames, radar[f]), args.steps)
                say(f"{cfg:16s} {dtype:4s} S={n:2d} mixed ({dark:2d} dark): forwards {t_fw * 1e3:7.2f} ms/step | frame_modes "
                    f"{t_fm * 1e3:7.2f} ms/step ({(t_fm / t_fw - 1) * 100:+5.1f} %)")
            # the dark count changes every step: nine counts spread over 1 .. S - 1
            n = max(args.streams)
            if n < 10 or args.vary_steps <= 0:
                continue
            counts = sorted({1 + round(i * (n - 2) / 8) for i in range(9)})
            assert len(counts) == 9
            bright = [mh.stream_frame(s, dark=False) for s in range(n)]
            darkf = [mh.stream_frame(s, dark=True) for s in range(n)]
            built = [0]
            build = eng._build

            def counting_build(*a, **k):
                built[0] += 1
                return build(*a, **k)
            eng._build = counting_build
            res = {}
            for split in ("forwards", "frame_modes", "forwards", "frame_modes"):   # (two runs each: the spread)
                fuser = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, split=split)
                eng._plans.clear()
                built[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for f in range(args.vary_steps):
                    a = counts[f % 9]
                    fuser([darkf[s] if s < a else bright[s] for s in range(n)], radar[f])
                torch.cuda.synchronize()
                res.setdefault(split, []).append(((time.perf_counter() - t0) / args.vary_steps, built[0]))
            eng._build = build
            say(f"{cfg:16s} {dtype:4s} S={n:2d} varying (dark counts {counts}, {args.vary_steps} steps): " + " | ".join(
                f"{split} " + ", ".join(f"{t * 1e3:7.2f} ms/step with {b} plans built" for t, b in res[split]) for split in res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--cfgs", nargs="*", default=["yolov3-tiny-12", "yolov3"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pipeline", dest="pipeline", action="store_false", help="skip the two-process rows")
    ap.add_argument("--split", choices=["forwards", "frame_modes", "compare"], default="forwards",
                    help="MultiStreamFuser(split=...) of every fuser; 'compare': only the A/B of the two splits (compare_splits)")
    ap.add_argument("--vary-steps", type=int, default=36, help="--split compare: steps of the run with a changing dark count")
    ap.add_argument("--pixel-format", nargs="+", default=None, choices=["rgb", "bgr", "nv12", "yuyv"],
                    help="only the comparison of these input formats against the first one (compare_formats)")
    ap.add_argument("--repeats", type=int, default=4, help="--pixel-format / --resize: blocks per variant")
    ap.add_argument("--nets", nargs="*", default=["yolov3-tiny-12:f32", "yolov3:bf16"],
                    help="--pixel-format / --resize: the cfg:dtype pairs to measure")
    ap.add_argument("--resize", nargs="+", default=None, choices=["nearest", "area"],
                    help="only the comparison of these resize modes against the first one (compare_resize), for the formats of "
                         "--pixel-format (default rgb nv12)")
    ap.add_argument("--frame-size", nargs=2, type=int, action="append", metavar=("H", "W"), default=None,
                    help="--resize / --img-size: the frames' size (default 480 640 / 1080 1920); may be given several times")
    ap.add_argument("--img-size", nargs=2, type=int, action="append", metavar=("H", "W"), default=None,
                    help="only the comparison of these network input sizes against the first one (compare_img_sizes); sides "
                         "multiples of 32; may be given several times")
    ap.add_argument("--handover", nargs="+", default=None, choices=["queue", "pinned"],
                    help="only the comparison of these FusionPipeline hand-overs (compare_handover), for the sizes of --frame-size "
                         "(default 480 640 and 1080 1920) and the formats of --pixel-format (default rgb nv12)")
    args = ap.parse_args()
    args.nets = [tuple(v.split(":")) for v in args.nets]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# python tools/multistream_latency.py {' '.join(sys.argv[1:])}".rstrip())
    if args.handover:
        compare_handover(args, say)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    if args.img_size:
        compare_img_sizes(args, say)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    if args.resize:
        compare_resize(args, say)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    if args.pixel_format:
        compare_formats(args, say)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    if args.split == "compare":
        compare_splits(args, say)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    say(f"# {torch.cuda.get_device_name(0)}; {args.steps} steps per repeat, median of {REPEATS} repeats, 5 warm-up steps")
    dev = mh.kalman_deviation()
    say(f"# float64 bar of tests/test_gpu_multistream.py: host tracker inv vs solve deviation {dev:.3e}, bar (16 x) {16 * dev:.3e}")
    for cfg in args.cfgs:
        for dtype in ("f32", "bf16"):
            net = _demo_net(cfg, dtype)
            for n, mixed in [(n, False) for n in args.streams] + [(max(args.streams), True)]:
                if mixed:   # two frame sizes, dark and bright interleaved: both sub-batches every step
                    frames = [mh.stream_frame(s) for s in range(n)]
                else:       # dark: every frame selects fusion
                    frames = [(synth.uniform(f"ms/frame{s}", (480, 640, 3)) * 25).astype(np.uint8) for s in range(n)]
                # the seeds wrap every 45 steps: the synthetic reflectors drift out of the filter's depth range after that, and
                # seed 46 holds a point on the camera plane (tests/multistream_helpers.py)
                radar = [[[radar_points((f + 7 * s) % 45)] for s in range(n)] for f in range(args.steps)]
                multi = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, split=args.split)   # the default tail
                other = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, split=args.split,
                                         tail="device" if multi.tail == "host" else "host")
                multi_host, multi_dev = (multi, other) if multi.tail == "host" else (other, multi)
                singles = [FrameFuser(net, RADAR_CALIB, model_mode=3, min_hits=2) for _ in range(n)]
                for f in range(5):   # warm-up: plans, autotuner, allocator
                    multi(frames, radar[f])
                    other(frames, radar[f])
                    for s in range(n):
                        singles[s](frames[s], radar[f][s])
                t_multi = timed(lambda f: multi(frames, radar[f]), args.steps)
                t_seq = timed(lambda f: [singles[s](frames[s], radar[f][s]) for s in range(n)], args.steps)
                # radar upload + chain + pack, HIP events (the host packs the points between the two records)
                gen = multi.generator
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev = []
                for f in range(args.steps):
                    torch.cuda.synchronize()
                    a.record()
                    gen.launch(radar[f])
                    b.record()
                    torch.cuda.synchronize()
                    ev.append(a.elapsed_time(b))
                t_launch = statistics.median(ev)
                t_host_gen = timed(lambda f: singles[0].generator(radar[f][0]), args.steps)
                # host time of a step before the first network launch: prepare + radar chain + staging + maps + mode rule

                def front(f):
                    p = multi.prepare(frames, radar[f])
                    img = p["img"].to(multi.device)
                    gen.gen(p["radar_frames"], p["hw"])
                    gen.heatmaps(32)
                    multi._modes(img)
                t_front = timed(front, args.steps)
                say(f"{cfg:16s} {dtype:4s} S={n:2d} {'mixed' if mixed else 'dark '}: multi ({multi.tail} tail) {t_multi * 1e3:7.2f} ms/step "
                    f"({n / t_multi:7.1f} frames/s) | {n} x FrameFuser {t_seq * 1e3:7.2f} ms ({n / t_seq:7.1f} frames/s) | "
                    f"ratio {t_seq / t_multi:5.2f} | radar upload + proposal launches {t_launch:6.3f} ms | host generator, 1 stream "
                    f"{t_host_gen * 1e3:6.3f} ms | front before the network {t_front * 1e3:6.2f} ms")
                # the output tail: both kinds on the rows of one recorded step, then the whole step with either
                recorded = []
                tail_fn = multi_dev._tail
                multi_dev._tail = lambda rows, hws: recorded.append((rows.clone(), hws)) or tail_fn(rows, hws)
                multi_dev(frames, radar[5])
                multi_dev._tail = tail_fn
                rows, hws = recorded[0]
                t_tail_host, t_tail_dev = timed_ab(lambda f: multi_host._tail(rows, hws), lambda f: multi_dev._tail(rows, hws),
                                                   args.steps)
                t_step_host, t_step_dev = timed_ab(lambda f: multi_host(frames, radar[f]), lambda f: multi_dev(frames, radar[f]),
                                                   args.steps)
                say(f"{cfg:16s} {dtype:4s} S={n:2d} {'mixed' if mixed else 'dark '}: tail alone on {rows.shape[0]:5d} rows: host "
                    f"{t_tail_host * 1e3:6.3f} ms, device {t_tail_dev * 1e3:6.3f} ms (x {t_tail_host / t_tail_dev:4.2f}) | step: "
                    f"host tail {t_step_host * 1e3:7.2f} ms, device tail {t_step_dev * 1e3:7.2f} ms "
                    f"({(t_step_dev / t_step_host - 1) * 100:+5.1f} %)")
                if n == max(args.streams) and not mixed and args.pipeline:
                    from millieye_amd.pipeline import FusionPipeline
                    piped = MultiStreamFuser(net, RADAR_CALIB, n, model_mode=3, min_hits=2, tail="device", split=args.split)
                    t0, done = None, 0
                    for _results, _info in FusionPipeline(piped, DarkSource(args.steps + 1, n), skip_to_newest=False):
                        if t0 is None:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        else:
                            done += 1
                    t_pipe = (time.perf_counter() - t0) / done
                    say(f"{cfg:16s} {dtype:4s} S={n:2d} dark : two-process pipeline {1 / t_pipe:7.1f} steps/s ({t_pipe * 1e3:6.2f} ms/step) "
                        f"| in-process fuser {1 / t_step_dev:7.1f} steps/s ({t_step_dev * 1e3:6.2f} ms/step) | ratio "
                        f"{t_step_dev / t_pipe:4.2f}")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
