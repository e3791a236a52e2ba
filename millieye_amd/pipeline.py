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

``handover="pinned"`` (opt-in, multi-stream only): the frames' bytes do not travel through the queue but through a
``handover.FrameRing`` - one shared-memory segment this process creates, registers with the HIP runtime once and unlinks; the
producer packs into a free slot and queues the slot's index, the consumer uploads out of the registered pages and gives the
index back (:class:`FusionPipeline`).
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
HANDOVERS = ("pinned",)
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


class _ConsumerLeft(Exception):
    """The producer's polls found ``all_done`` set: nobody will take another step."""


def _poll(source_q, all_done, poll_s=0.2):
    """``source_q.get()`` that gives up once the consumer has left (a blocked ``get`` would outlive it)."""
    while True:
        try:
            return source_q.get(timeout=poll_s)
        except _queue.Empty:
            if all_done.is_set():
                raise _ConsumerLeft() from None


def _producer_multi(q, first_done, all_done, source_factory, prepare_factory, handover=None):
    """The producer of a multi-stream pipeline: every step is queued (blocking ``put``), skipping is the consumer's business.

    ``handover``: ``None`` or ``(ring, free, ctrl)`` - the consumer's ``handover.FrameRing`` (attached here by unpickling; ``None``:
    it arrives over ``ctrl`` behind the first-frame rendezvous, sized from step 0), the queue of free slot indices and the
    control queue.  With a ring, a step takes a free slot before it packs (polling, so that a consumer that left is noticed),
    packs into it and queues the payload without the bytes; a step that does not fit gives the slot back unused and travels
    through the queue like any step without a ring."""
    error = None
    ring = None
    try:
        prepare = prepare_factory()
        if handover is not None:
            from .utils.datasets import PackBufferTooSmall
            ring, free, ctrl = handover
        for idx, (frames, radar_frames) in enumerate(source_factory()):
            payload = None
            if ring is not None:
                slot = _poll(free, all_done)
                try:
                    payload = prepare(frames, radar_frames, out=ring.slot(slot))
                    payload["img"].lend_to_ring(slot)
                except PackBufferTooSmall:
                    free.put(slot)
                    payload = prepare(frames, radar_frames)
                    payload["handover_fallback"] = True
            if payload is None:
                payload = prepare(frames, radar_frames)
            payload["frame_idx"] = idx
            q.put(payload)
            if idx == 0:
                first_done.wait()
                if handover is not None and ring is None:
                    ring = _poll(ctrl, all_done)
    except _ConsumerLeft:
        pass
    except BaseException as exc:
        error = f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"
    finally:
        q.put({"frame_idx": _END, "dropped": 0, "error": error})
        all_done.wait(timeout=120)
        if ring is not None:
            payload = None   # (its img may still view a slot)
            ring.close()


class _Handover:
    """The consumer's side of ``handover="pinned"``: the ring (owned and registered here), the queue of free slot indices, the
    control queue that carries the ring's handle when step 0 sizes it, and the staged objects currently bound to a slot."""

    def __init__(self, ctx, ring_slots):
        self.ring, self.ring_slots, self.fallback = None, ring_slots, 0
        self.free, self.ctrl = ctx.Queue(), ctx.Queue()
        self.bound = []

    @property
    def slot_bytes(self):
        return None if self.ring is None else self.ring.slot_bytes

    def open(self, slot_bytes):
        from .handover import FrameRing
        self.ring = FrameRing(self.ring_slots, slot_bytes)
        self.ring.register()
        for i in range(self.ring_slots):
            self.free.put(i)

    def open_for(self, payload):
        """Size the ring from a step that came through the queue - its byte total plus one quarter - and send the producer
        the handle."""
        packed = getattr(payload.get("img"), "packed", None)
        if packed is None:
            raise ValueError("FusionPipeline(handover='pinned', slot_bytes=None): step 0 carries no packed frames to size the "
                             "ring from; pass slot_bytes=")
        total = max(int(packed.numel()), 1)
        self.open(total + total // 4)
        self.ctrl.put(self.ring)     # (pickles to the handle)

    def take(self, payload):
        """A payload fresh from the queue: bind its frames to this process's mapping of the ring, or count the fallback."""
        if payload.get("handover_fallback"):
            self.fallback += 1
            return
        img = payload.get("img")
        if getattr(img, "ring_slot", None) is not None:
            img.bind(self.ring)
            self.bound.append(img)

    def give_back(self, payload, synchronize=False):
        img = payload.get("img")
        if not any(img is b for b in self.bound):
            return
        if synchronize:   # the upload out of the slot was queued on the current stream; infer= overrides need not end in a read
            import torch
            if torch.cuda.is_available() and torch.cuda.is_initialized():
                torch.cuda.current_stream().synchronize()
        self.bound = [b for b in self.bound if b is not img]
        img.unbind()
        self.free.put(img.ring_slot)

    def close(self):
        for img in self.bound:
            img.unbind()
        self.bound = []
        if self.ring is not None:
            self.ring.close()
        for chan in (self.free, self.ctrl):
            chan.cancel_join_thread()
            chan.close()


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
    skipped steps.  ``drop_oldest`` does not apply: the producer never drops.  ``advance``: override (tests).

    ``handover="pinned"`` (multi-stream fusers only; default ``None``: every step's bytes travel through the queue): the frames'
    bytes cross the process boundary in a :class:`millieye_amd.handover.FrameRing` - ``ring_slots`` (default ``QUEUE_SIZE + 2``,
    at least 2) slots of ``slot_bytes`` in one shared-memory segment that this process creates, registers with the HIP runtime
    once and unlinks when the iteration ends, however it ends.  The producer takes a free slot index from a queue before it
    packs, packs straight into the slot and queues the payload without the bytes; the consumer uploads out of the registered
    pages and gives the index back - for a step that was only advanced right after ``advance``, for the inferred step once
    ``infer`` has returned and the current stream is synchronised.  The free-slot queue is the back-pressure; the producer
    still never drops a step.  ``slot_bytes=None``: step 0 travels through the queue, the ring is sized from its byte total
    plus one quarter and its handle reaches the producer at the first-frame rendezvous.  A later step that does not fit a slot
    travels through the queue (``stats["handover_fallback"]`` counts them).  ``stats`` also holds ``handover``,
    ``ring_slots`` and ``slot_bytes`` (``None`` when no ring was ever opened)."""

    def __init__(self, fuser, source_factory, infer=None, drop_oldest=True, prepare_factory=None, start_method="spawn",
                 skip_to_newest=True, advance=None, handover=None, ring_slots=None, slot_bytes=None):
        self.fuser, self.source_factory, self.drop_oldest = fuser, source_factory, drop_oldest
        self.infer = infer or fuser.infer
        self.multi = hasattr(fuser, "streams") and hasattr(fuser, "advance")
        if handover is not None:
            if handover not in HANDOVERS:
                raise ValueError(f"FusionPipeline: unknown handover {handover!r} (None or one of {', '.join(HANDOVERS)})")
            if not self.multi:
                raise ValueError("FusionPipeline: handover= is for multi-stream fusers (a FrameFuser's frame is queued as it is)")
            ring_slots = QUEUE_SIZE + 2 if ring_slots is None else int(ring_slots)
            if ring_slots < 2:
                raise ValueError(f"FusionPipeline: ring_slots must be at least 2 (got {ring_slots}): one slot is packed while "
                                 f"another is read")
            if slot_bytes is not None and int(slot_bytes) <= 0:
                raise ValueError(f"FusionPipeline: slot_bytes must be positive (got {slot_bytes})")
        elif ring_slots is not None or slot_bytes is not None:
            raise ValueError("FusionPipeline: ring_slots= / slot_bytes= need handover='pinned'")
        self.handover, self.ring_slots = handover, ring_slots
        self.slot_bytes = None if slot_bytes is None else int(slot_bytes)
        self.ring_name = None
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
        args = (q, first_done, all_done, self.source_factory, self.prepare_factory)
        hand = None
        if self.handover is not None:
            hand = _Handover(ctx, self.ring_slots)
            if self.slot_bytes is not None:
                hand.open(self.slot_bytes)       # the ring exists before the producer starts
            args += ((hand.ring, hand.free, hand.ctrl),)
        t0, frames, dropped = time.perf_counter(), 0, 0
        end = proc = None
        try:
            proc = ctx.Process(target=_producer_multi, args=args, daemon=True)
            proc.start()
            while end is None:
                waiting = [self._next_payload(q, proc)]
                while self.skip_to_newest and waiting[-1]["frame_idx"] != _END:   # everything else that waits, in order
                    try:
                        waiting.append(q.get_nowait())
                    except _queue.Empty:
                        break
                if waiting[-1]["frame_idx"] == _END:
                    end = waiting.pop()
                if hand is not None:
                    for payload in waiting:
                        hand.take(payload)
                skipped = []
                for payload in waiting[:-1]:
                    self.advance(payload)
                    if hand is not None:
                        hand.give_back(payload)          # the radar chain does not read frames
                    skipped.append(payload["frame_idx"])
                dropped += len(skipped)
                if waiting:
                    results = self.infer(waiting[-1])
                    if hand is not None:
                        hand.give_back(waiting[-1], synchronize=True)
                        if hand.ring is None:            # slot_bytes=None: step 0 came through the queue and sizes the ring
                            hand.open_for(waiting[-1])
                    first_done.set()
                    frames += 1
                    yield results, dict(frame_idx=waiting[-1]["frame_idx"], skipped=skipped)
            if end.get("error"):
                raise ProducerError("the producer process failed:\n" + end["error"])
        finally:
            first_done.set()
            all_done.set()
            if proc is not None:
                if end is None:
                    proc.terminate()   # left early (break, an exception in infer): the producer may be blocked on the full queue
                proc.join(timeout=10)
                if proc.is_alive():
                    proc.terminate()
            self.stats = dict(dropped=dropped, frames=frames, seconds=time.perf_counter() - t0)
            if hand is not None:
                self.stats.update(handover=self.handover, ring_slots=self.ring_slots, slot_bytes=hand.slot_bytes,
                                  handover_fallback=hand.fallback)
                self.ring_name = None if hand.ring is None else hand.ring.name   # (of the last run; gone by now)
                waiting = payload = None
                hand.close()          # after the producer is gone: unregister, unmap, unlink

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
