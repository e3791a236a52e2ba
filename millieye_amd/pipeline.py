"""The live demo's two-stage pipeline (``module3_our_dataset/run_mp.py:42-160,289-338``):

    producer process  (run_mp ``pre_process``)   frame + radar frames -> radar tracking / box proposals / staged inputs
         |  mp.Queue(maxsize=3), newest kept: when more than two items wait, the producer drops the oldest (:148-149)
         |  mp.Event: after the first frame the producer waits until the consumer finished its first - slow - inference (:146-147)
    consumer (this process, owns the GPU)         input kernels -> mode selection -> Network.forward -> NMS 0.3 -> rescale

Host work (~0.65 ms per frame: Kalman tracks, DBSCAN, proposal arithmetic) and device work overlap exactly like in the
reference; the device half is :meth:`millieye_amd.demo.FrameFuser.infer`, the host half :meth:`FrameFuser.prepare`.
Video decoding, the serial-port capture and the OpenCV window are not part of the path: frames come from a caller-supplied
*source factory* - a picklable callable returning an iterator of ``(frame_uint8_hwc, radar_frames)`` - which is called
inside the producer process (like the reference opens ``cv2.VideoCapture`` there).

With a :class:`millieye_amd.demo.MultiStreamFuser` the same two processes carry S streams per step: the source yields
``(frames, radar_frames)`` with S entries each; the producer runs the model-free host half (``demo.prepare_streams``: the
checks and the packing of every frame's bytes into one buffer + descriptor - most of the host time of a step at S = 32) and
never touches the HIP library or the GPU.  A fuser built with ``pixel_format=`` has the producer pack the cameras' native bytes
(NV12: half of the RGB bytes, YUYV: two thirds), which is what crosses the process boundary and the PCIe link; its ``resize=``
travels with the packed frames.  The trackers live on the device, in the consumer, so the producer never drops a
step (a dropped step would lose its radar frames and break the tracks): it blocks on the full queue, and the consumer skips
instead - it takes everything that waits, runs ``advance`` (the radar chain alone) on all but the newest step, in order, and
``infer`` on the newest.
"""
import multiprocessing as mp
import pickle
import queue as _queue
import time
import traceback

__all__ = ["FusionPipeline", "ProducerError", "QUEUE_SIZE"]


class ProducerError(RuntimeError):
    """The producer process failed (source iterator, radar tracking, staging); carries its traceback text."""

QUEUE_SIZE = 3      # run_mp.py:289
_END = "__end__"


def _producer(q, first_done, all_done, source_factory, prepare_factory, drop_oldest):
    """run_mp.py:42-160.  ``prepare_factory()`` builds the host half inside this process (tracker state lives here)."""
    dropped = 0
    error = None
    try:
        prepare = prepare_factory()
        for idx, (frame, radar_frames) in enumerate(source_factory()):
            payload = prepare(frame, radar_frames)
            payload["frame_idx"] = idx
            q.put(payload)
            if idx == 0:
                first_done.wait()          # inference of the first frame on the GPU is very slow (:146-147)
            if drop_oldest:
                try:
                    if q.qsize() > QUEUE_SIZE - 1:   # avoid blocking on a full queue: discard the oldest (:148-149)
                        q.get_nowait()
                        dropped += 1
                except (NotImplementedError, _queue.Empty):
                    pass
    except BaseException as exc:  # reported through the END payload: a crash must not look like the end of the stream
        error = f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"
    finally:
        q.put({"frame_idx": _END, "dropped": dropped, "error": error})
        # tensors travel as shared-memory handles served by THIS process: stay until the consumer has taken everything
        all_done.wait(timeout=120)


def _producer_multi(q, first_done, all_done, source_factory, prepare_factory):
    """The producer of a multi-stream pipeline: every step is queued (blocking ``put``), skipping is the consumer's business."""
    error = None
    try:
        prepare = prepare_factory()
        for idx, (frames, radar_frames) in enumerate(source_factory()):
            payload = prepare(frames, radar_frames)
            payload["frame_idx"] = idx
            q.put(payload)
            if idx == 0:
                first_done.wait()
    except BaseException as exc:
        error = f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"
    finally:
        q.put({"frame_idx": _END, "dropped": 0, "error": error})
        all_done.wait(timeout=120)


class _MultiPrepareFactory:
    """Picklable recipe of the multi-stream host half: ``demo.prepare_streams`` with the frames packed - no model, no
    generator, no HIP library."""

    def __init__(self, streams, img_size, pixel_format=None, resize=None):
        self.streams, self.img_size, self.pixel_format, self.resize = int(streams), img_size, pixel_format, resize

    def __call__(self):
        import functools
        from .demo import prepare_streams
        return functools.partial(prepare_streams, streams=self.streams, img_size=self.img_size, pack=True,
                                 pixel_format=self.pixel_format, resize=self.resize)


class _PrepareFactory:
    """Picklable recipe of the host half: builds a fresh ``FrameFuser`` (without a model) in the producer."""

    def __init__(self, calib_param, img_size, generator_kwargs, generator=None, pixel_format=None, resize=None):
        self.calib_param, self.img_size, self.generator_kwargs = calib_param, img_size, generator_kwargs
        self.generator = generator   # a caller-supplied generator instance travels by pickle (checked by FusionPipeline)
        self.pixel_format, self.resize = pixel_format, resize

    def __call__(self):
        from .demo import FrameFuser
        if self.generator is not None:
            return FrameFuser(None, self.calib_param, img_size=self.img_size, generator=self.generator,
                              pixel_format=self.pixel_format, resize=self.resize).prepare
        return FrameFuser(None, self.calib_param, img_size=self.img_size, pixel_format=self.pixel_format, resize=self.resize,
                          **self.generator_kwargs).prepare


class FusionPipeline:
    """``for rows, info in FusionPipeline(fuser, source_factory): ...`` - detections per frame, in frame order, frames the
    producer dropped are skipped (``info["frame_idx"]`` says which one this is).

    ``fuser``: a :class:`millieye_amd.demo.FrameFuser` (its model stays in this process).  A default
    ``RadarProposalGenerator`` is re-created from its parameters inside the producer; a generator the caller passed to
    ``FrameFuser(generator=...)`` is sent there by pickle as it is now, and refused (``TypeError``) when it cannot be
    pickled - never silently replaced.  ``infer``: override of the device half (tests).  ``drop_oldest=False`` turns the
    reference's newest-wins policy into back-pressure (every frame is processed).  A failure in the producer (source,
    tracking, staging) ends the iteration with :class:`ProducerError` carrying the producer's traceback.

    ``fuser``: a :class:`millieye_amd.demo.MultiStreamFuser` - ``for results, info in FusionPipeline(fuser, source_factory)``
    yields per step the list of S ``(rows, info)`` its ``infer`` returns and ``info = dict(frame_idx=..., skipped=[...])``,
    the steps that were only advanced since the previous yield.  The source yields ``(frames, radar_frames)`` with S entries
    each.  ``skip_to_newest=True`` (default): of the steps that wait, all but the newest only run ``advance`` (the radar
    chain, so the trackers see every step in order); ``False``: every step is inferred.  ``stats["dropped"]`` counts the
    skipped steps.  ``drop_oldest`` does not apply: the producer never drops.  ``advance``: override (tests)."""

    def __init__(self, fuser, source_factory, infer=None, drop_oldest=True, prepare_factory=None, start_method="spawn",
                 skip_to_newest=True, advance=None):
        self.fuser, self.source_factory, self.drop_oldest = fuser, source_factory, drop_oldest
        self.infer = infer or fuser.infer
        self.multi = hasattr(fuser, "streams") and hasattr(fuser, "advance")
        self.skip_to_newest = skip_to_newest
        self.advance = advance or getattr(fuser, "advance", None)
        if prepare_factory is None and self.multi:
            prepare_factory = _MultiPrepareFactory(fuser.streams, fuser.img_size, getattr(fuser, "pixel_format", None),
                                                   getattr(fuser, "resize", None))
        if prepare_factory is None:
            g = fuser.generator
            if getattr(fuser, "generator_is_default", False):
                prepare_factory = _PrepareFactory(g.calib_param, fuser.img_size, g.kwargs,
                                                  pixel_format=getattr(fuser, "pixel_format", None),
                                                  resize=getattr(fuser, "resize", None))
            else:
                try:
                    pickle.dumps(g)
                except Exception as exc:
                    raise TypeError("FusionPipeline: the FrameFuser was built with a custom generator= that cannot be "
                                    f"pickled into the producer process ({exc}); pass prepare_factory= instead") from exc
                prepare_factory = _PrepareFactory(getattr(g, "calib_param", None), fuser.img_size, {}, generator=g,
                                                  pixel_format=getattr(fuser, "pixel_format", None),
                                                  resize=getattr(fuser, "resize", None))
        self.prepare_factory = prepare_factory
        self.ctx = mp.get_context(start_method)      # run_mp.py:287: spawn
        self.stats = {}

    @staticmethod
    def _next_payload(q, proc, poll_s=0.5):
        """``q.get()`` that notices a producer killed hard (OOM killer, a segfault in the decode / radar code): such a
        process never posts its END payload, and a crash must not look like an endless wait."""
        import queue as _queue
        while True:
            try:
                return q.get(timeout=poll_s)
            except _queue.Empty:
                if not proc.is_alive():
                    try:   # whatever it managed to queue before dying (END included) still counts
                        return q.get(timeout=poll_s)
                    except _queue.Empty:
                        raise ProducerError(f"the producer process died without ending the stream (exit code "
                                            f"{proc.exitcode})") from None

    def _iter_multi(self):
        ctx = self.ctx
        q = ctx.Queue(maxsize=QUEUE_SIZE)
        first_done = ctx.Event()
        all_done = ctx.Event()
        proc = ctx.Process(target=_producer_multi, args=(q, first_done, all_done, self.source_factory, self.prepare_factory),
                           daemon=True)
        proc.start()
        t0, frames, dropped = time.perf_counter(), 0, 0
        end = None
        try:
            while end is None:
                waiting = [self._next_payload(q, proc)]
                while self.skip_to_newest and waiting[-1]["frame_idx"] != _END:   # everything else that waits, in order
                    try:
                        waiting.append(q.get_nowait())
                    except _queue.Empty:
                        break
                if waiting[-1]["frame_idx"] == _END:
                    end = waiting.pop()
                skipped = []
                for payload in waiting[:-1]:
                    self.advance(payload)
                    skipped.append(payload["frame_idx"])
                dropped += len(skipped)
                if waiting:
                    results = self.infer(waiting[-1])
                    first_done.set()
                    frames += 1
                    yield results, dict(frame_idx=waiting[-1]["frame_idx"], skipped=skipped)
            if end.get("error"):
                raise ProducerError("the producer process failed:\n" + end["error"])
        finally:
            first_done.set()
            all_done.set()
            if end is None:
                proc.terminate()   # left early (break, an exception in infer): the producer may be blocked on the full queue
            proc.join(timeout=10)
            if proc.is_alive():
                proc.terminate()
            self.stats = dict(dropped=dropped, frames=frames, seconds=time.perf_counter() - t0)

    def __iter__(self):
        if self.multi:
            return self._iter_multi()
        return self._iter_single()

    def _iter_single(self):
        ctx = self.ctx
        q = ctx.Queue(maxsize=QUEUE_SIZE)
        first_done = ctx.Event()
        all_done = ctx.Event()
        proc = ctx.Process(target=_producer, args=(q, first_done, all_done, self.source_factory, self.prepare_factory,
                                                   self.drop_oldest), daemon=True)
        proc.start()
        t0, frames, dropped = time.perf_counter(), 0, None
        try:
            while True:
                payload = self._next_payload(q, proc)
                if payload["frame_idx"] == _END:
                    dropped = payload["dropped"]
                    if payload.get("error"):
                        raise ProducerError("the producer process failed:\n" + payload["error"])
                    break
                rows, info = self.infer(payload)
                first_done.set()               # run_mp.py:316
                info = dict(info, frame_idx=payload["frame_idx"])
                frames += 1
                yield rows, info
        finally:
            first_done.set()
            all_done.set()
            proc.join(timeout=10)
            if proc.is_alive():
                proc.terminate()               # run_mp.py:336
            self.stats = dict(dropped=dropped, frames=frames, seconds=time.perf_counter() - t0)
