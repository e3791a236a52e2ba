"""What reading frames where they lie costs and saves: ``StagedSurfaces.to()`` (``me_image_batch_surfaces_u8_f32``) against
``StagedRaggedImages.to()`` on dense tensors, the input step of a ``MultiStreamFuser``.

Per streams S, frame size, pixel format and resize, the median time of one ``to()`` - on the host (until the call returns: the
gather, the uploads and the launch are queued) and on the device (events around the call) - for three inputs:

* ``dense``:   dense frame tensors through ``StagedRaggedImages`` - today's path: every frame is packed into one pinned buffer
               on the host, uploaded, and read by the dense kernel;
* ``pinned``:  one pitched pinned CPU surface per stream (pitch aligned to ``--align`` bytes, the NV12 chroma plane behind a
               height aligned to 16 rows) - uploaded as it lies, one copy per stream, no gather;
* ``cuda``:    the same surfaces resident on the device - nothing is uploaded but the descriptor.

Then the kernels alone, device events around ``--launches`` back-to-back launches over data that lies on the device: the dense
kernel against the surface kernel on dense-equivalent surfaces (``pitch == row``) and on the pitched ones, alternating, the
median of ``--repeats`` rounds.  Needs a GPU; there is no fallback.

python tools/surface_input_latency.py --out profiles/multistream_surfaces.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from millieye_amd import hip  # noqa: E402
from millieye_amd.utils.datasets import FrameSurface, StagedRaggedImages, StagedSurfaces  # noqa: E402

ROW_BYTES = {"rgb": 3, "nv12": 1}


def _align(v, a):
    return -(-v // a) * a


def dense_frame(fmt, h, w, seed):
    shape = (h, w, 3) if fmt == "rgb" else (h * 3 // 2, w)
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8))


def pitched_surface(frame, fmt, h, w, align, place):
    """``frame`` copied into a buffer with rows ``align``-aligned (``align = 1``: dense-equivalent), moved by ``place``."""
    row = ROW_BYTES[fmt] * w
    pitch = _align(row, align)
    rows_y = h if fmt == "rgb" else _align(h, 16 if align > 1 else 1)
    rows = rows_y + (h // 2 if fmt == "nv12" else 0)
    buf = torch.zeros((rows, pitch), dtype=torch.uint8)
    buf[:h, :row] = frame.reshape(-1, row)[:h]
    if fmt == "nv12":
        buf[rows_y:rows_y + h // 2, :w] = frame[h:]
    return FrameSurface(place(buf.reshape(-1)), h, w, fmt, 0, pitch, rows_y * pitch if fmt == "nv12" else None,
                        pitch if fmt == "nv12" else None)


def time_to(make, steps, warmup):
    """Median host / device milliseconds of ``make().to("cuda")``; ``make`` builds the staged object of one step."""
    host, dev = [], []
    for i in range(warmup + steps):
        staged = make()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        out = staged.to("cuda")
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if i >= warmup:
            host.append((t1 - t0) * 1e3), dev.append(a.elapsed_time(b))
        del out
    return statistics.median(host), statistics.median(dev)


def time_kernels(calls, launches, repeats):
    """Median device milliseconds per launch of each of ``calls`` (functions that queue one launch), alternating."""
    per = [[] for _ in calls]
    for call in calls:   # warm-up: code objects, caches
        call()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, call in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                call()
            b.record()
            torch.cuda.synchronize()
            per[k].append(a.elapsed_time(b) / launches)
    return [statistics.median(p) for p in per]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--frame-size", nargs=2, type=int, action="append", metavar=("H", "W"), default=None)
    ap.add_argument("--formats", nargs="*", default=["rgb", "nv12"], choices=sorted(ROW_BYTES))
    ap.add_argument("--resize", nargs="*", default=["nearest", "area"], choices=["nearest", "area"])
    ap.add_argument("--img-size", type=int, default=416)
    ap.add_argument("--align", type=int, default=256, help="pitch alignment of the pitched surfaces, bytes")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_input_latency: needs a GPU")
    sizes = [tuple(s) for s in (args.frame_size or [[480, 640], [1080, 1920]])]
    lib, size = hip.lib(), args.img_size
    lines = [f"# python tools/surface_input_latency.py {' '.join(sys.argv[1:])}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}; img_size {size}; to(): median of {args.steps} steps after {args.warmup} warm-up "
             f"steps, host = until to() returns, device = events around to(); kernels: device events around {args.launches} "
             f"launches, median of {args.repeats} rounds, the variants alternating; pitch alignment {args.align} bytes"]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for n in args.streams:
        for h, w in sizes:
            for fmt in args.formats:
                frames = [dense_frame(fmt, h, w, 7 + s) for s in range(n)]
                pinned = [pitched_surface(f, fmt, h, w, args.align, lambda b: b.pin_memory()) for f in frames]
                resident = [pitched_surface(f, fmt, h, w, args.align, lambda b: b.cuda()) for f in frames]
                equivalent = [pitched_surface(f, fmt, h, w, 1, lambda b: b.cuda()) for f in frames]
                for resize in args.resize:
                    head = f"S={n:2d} {h:4d}x{w:<4d} {fmt:4s} {resize:7s}"
                    want = StagedRaggedImages(frames, size, formats=fmt, resize=resize).to("cuda")
                    for surfaces in (pinned, resident, equivalent):   # faster and different is not faster
                        assert torch.equal(StagedSurfaces(surfaces, size, resize=resize).to("cuda"), want)
                    dense = time_to(lambda: StagedRaggedImages(frames, size, formats=fmt, resize=resize), args.steps, args.warmup)
                    pin = time_to(lambda: StagedSurfaces(pinned, size, resize=resize), args.steps, args.warmup)
                    res = time_to(lambda: StagedSurfaces(resident, size, resize=resize), args.steps, args.warmup)
                    mb = sum(f.numel() for f in frames) / 1e6
                    emit(f"{head}: {mb:7.2f} MB/step | to() median ms host / device: dense {dense[0]:6.2f} / {dense[1]:6.2f} | "
                         f"pinned surfaces {pin[0]:6.2f} / {pin[1]:6.2f} | cuda surfaces {res[0]:6.2f} / {res[1]:6.2f}")
                    # the kernels alone, everything on the device
                    packed = StagedRaggedImages(frames, size, formats=fmt, resize=resize).pack()
                    d_src, d_desc = packed.packed.cuda(), packed.desc.cuda()
                    out, stream = torch.empty_like(want), hip.stream_ptr()
                    d_eq = StagedSurfaces(equivalent, size, resize=resize).descriptor([]).cuda()
                    d_pitched = StagedSurfaces(resident, size, resize=resize).descriptor([]).cuda()
                    area = int(resize == "area")

                    def dense_call():
                        if area:
                            lib.me_image_batch_area_u8_f32(d_src.data_ptr(), d_src.numel(), d_desc.data_ptr(), n, out.data_ptr(), size, stream)
                        else:
                            lib.me_image_batch_letterbox_u8_f32(d_src.data_ptr(), d_src.numel(), d_desc.data_ptr(), n,
                                                                out.data_ptr(), size, size, stream)

                    def surface_call(desc):
                        return lambda: lib.me_image_batch_surfaces_u8_f32(desc.data_ptr(), n, out.data_ptr(), size, size, area, stream)

                    k = time_kernels([dense_call, surface_call(d_eq), surface_call(d_pitched)], args.launches, args.repeats)
                    emit(f"{head}: kernel alone, median ms per launch: dense {k[0]:7.4f} | surfaces, pitch == row {k[1]:7.4f} "
                         f"(x {k[1] / k[0]:.3f}) | surfaces, pitched {k[2]:7.4f} (x {k[2] / k[0]:.3f})")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
