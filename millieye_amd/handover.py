"""The pinned hand-over buffer of the two-process multi-stream pipeline (``pipeline.FusionPipeline(handover="pinned")``).

:class:`FrameRing` is ``slots`` x ``slot_bytes`` uint8 in ONE ``multiprocessing.shared_memory`` segment that lives as long as
the pipeline.  The consumer - the process that owns the GPU - creates it, registers the whole mapping with the HIP runtime once
(``hipHostRegister`` through ``torch.cuda.cudart()``: page-locked, so ``tensor.to(device, non_blocking=True)`` of a slot is one
DMA out of the very pages the producer wrote) and unlinks it.  The producer attaches by name, packs every step's frame bytes
straight into a free slot (``StagedRaggedImages.pack(out=ring.slot(i))``) and queues only the slot index: no fresh tensor, no
shared-memory file per step, no page faults on a new mapping, no bounce buffer.  The producer never registers anything, never
loads the HIP library and never initialises the GPU.

Which slot is free is the pipeline's business (a queue of free indices); the ring itself is storage."""
import os
from multiprocessing import shared_memory

import torch

from . import hip

__all__ = ["FrameRing", "PAGE"]

PAGE = 4096   # slot_bytes is rounded up to this: every slot starts on a page


def _attach(name, slots, slot_bytes):
    return FrameRing(slots, slot_bytes, name=name)


class FrameRing:
    """``FrameRing(slots, slot_bytes)`` creates and owns the segment; pickling carries the handle ``(name, slots,
    slot_bytes)`` - never bytes - and unpickling (or ``FrameRing(slots, slot_bytes, name=...)``) attaches to it.

    ``slot(i)``: a 1-D uint8 torch view of slot ``i`` (no copy; every call returns the same tensor).  ``register()`` /
    ``unregister()``: owner only, idempotent; without a CUDA device ``register()`` does nothing and ``registered`` stays
    ``False``.  ``close()``: synchronise the device (if initialised), unregister, drop the views, close the mapping and - the
    owner - unlink the name; callable twice, and whatever became of the other process."""

    _shm = _base = None
    registered = False

    def __init__(self, slots, slot_bytes, name=None):
        slots, slot_bytes = int(slots), int(slot_bytes)
        if slots <= 0 or slot_bytes <= 0:
            raise ValueError(f"FrameRing: slots and slot_bytes must be positive (got {slots} x {slot_bytes})")
        self.slots = slots
        self.slot_bytes = -(-slot_bytes // PAGE) * PAGE
        self.owner = name is None
        self.registered = False
        self.register_status = None     # what cudaHostRegister returned (0: success), None: never called
        self._views = {}
        size = self.slots * self.slot_bytes
        if self.owner:
            self._shm = shared_memory.SharedMemory(create=True, size=size)
            try:   # reserve the pages now: a full /dev/shm is an OSError here, not a SIGBUS at the producer's first write
                if getattr(self._shm, "_fd", -1) >= 0 and hasattr(os, "posix_fallocate"):
                    os.posix_fallocate(self._shm._fd, 0, size)
            except OSError as exc:
                self._shm.close()
                self._shm.unlink()
                self._shm = None
                raise hip.MeError(f"FrameRing: cannot reserve {slots} x {self.slot_bytes} bytes of shared memory "
                                  f"({exc})") from exc
        else:
            try:
                self._shm = shared_memory.SharedMemory(name=name, track=False)   # (Python >= 3.13)
            except TypeError:
                self._shm = shared_memory.SharedMemory(name=name)
            if self._shm.size < size:
                got = self._shm.size
                self._shm.close()
                self._shm = None
                raise hip.MeError(f"FrameRing: segment {name} holds {got} bytes, the handle says {size}")
        self.name = self._shm.name
        self._base = torch.frombuffer(self._shm.buf, dtype=torch.uint8, count=size)

    @property
    def handle(self):
        return (self.name, self.slots, self.slot_bytes)

    @property
    def closed(self):
        return self._shm is None

    def __reduce__(self):
        return (_attach, self.handle)

    def slot(self, i):
        if self._shm is None:
            raise hip.MeError("FrameRing: the ring is closed")
        i = int(i)
        if not 0 <= i < self.slots:
            raise hip.MeError(f"FrameRing: slot {i} of {self.slots}")
        if i not in self._views:
            self._views[i] = self._base[i * self.slot_bytes:(i + 1) * self.slot_bytes]
        return self._views[i]

    def register(self):
        """One ``hipHostRegister`` of the whole mapping.  Returns the runtime's status (0: success), ``None`` when there is
        no CUDA device or the ring is registered already."""
        if self._shm is None:
            raise hip.MeError("FrameRing: the ring is closed")
        if not self.owner:
            raise hip.MeError("FrameRing.register(): only the process that created the ring registers it")
        if self.registered or not torch.cuda.is_available():
            return None
        status = int(torch.cuda.cudart().cudaHostRegister(self._base.data_ptr(), self._base.numel(), 0))
        self.register_status = status
        self.registered = status == 0
        if status != 0:
            raise hip.MeError(f"FrameRing.register(): hipHostRegister of {self._base.numel()} bytes failed (status {status})")
        return status

    def unregister(self):
        if not self.registered:
            return None
        self.registered = False
        return int(torch.cuda.cudart().cudaHostUnregister(self._base.data_ptr()))

    def close(self):
        if self._shm is None:
            return
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()          # no copy out of a slot may be in flight when its pages are unpinned
        self.unregister()
        shm, self._shm = self._shm, None
        self._views.clear()
        self._base = None
        try:
            shm.close()
        except BufferError:
            # a caller still holds a view of a slot: the mapping stays until that view dies, the name goes all the same
            pass
        if self.owner:
            try:
                shm.unlink()
            except FileNotFoundError:
                pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
