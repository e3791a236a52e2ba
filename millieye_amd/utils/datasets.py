"""Input producer: ``MyDataset`` with the batch assembled on the GPU.

Mirror of ``module3_our_dataset/utils/datasets.py:109-326``: same constructor, file layout
(``dataset.txt``, ``image/*.jpg``, ``label/*.txt``, ``radar_box/*.pkl``, ``radar_point/*.pkl``), scene split, label /
radar-box arithmetic and ``collate_fn`` return tuple ``(paths, imgs, targets, radar_boxes, radar_maps)``.

What moved to the device (``csrc/input.hip``):

* ``ToTensor`` + ``pad_to_square`` + nearest ``resize`` of every frame  -> ``me_image_pad_resize_u8_f32``
* ``plot_radar_heatmap`` (3 x ``np.histogram2d``) + ``ToTensor().float()`` + ``pad_to_square`` + bilinear
  ``F.interpolate(align_corners=True)`` of every radar map             -> ``me_radar_heatmap_f32`` (one launch per batch)

``__getitem__`` therefore only decodes (PIL, like the reference) and parses the small text / pickle files - it stays
picklable CPU data, so ``DataLoader(num_workers>0)`` still works - and ``collate_fn`` returns *staged* batches for
``imgs`` / ``radar_maps``: objects whose ``.to(device)`` (the call ``train.py:181-182`` / ``test_fusion.py:66-67`` make on
them anyway) uploads the raw bytes / points and launches the kernels in the consumer process.  ``targets`` and
``radar_boxes`` are the same CPU tensors as in the reference.  There is no CPU implementation here:
``.to("cpu")`` raises (the CPU restatement used by the tests lives in ``oracle/datasets_ref.py``).
"""
import os
import pickle
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import hip
from .utils import canvas_hw, canvas_size

__all__ = ["MyDataset", "StagedImages", "StagedRaggedImages", "StagedRadarMaps", "obtain_bboxs", "PIXEL_FORMATS",
           "picture_hw", "RESIZE_MODES", "resize_mode", "FrameSurface", "StagedSurfaces"]

_SCENES = ["0", "1", "2", "3", "4"]


def obtain_bboxs(path):
    """Annotation lines ``label x y w h`` of a text file (datasets.py:41-56); ``%`` starts a comment line."""
    out = []
    with open(path, "r") as fh:
        for line in fh.read().split("\n"):
            if not line or line.startswith("%"):
                continue
            items = line.strip().split(" ")
            out.append([items[0]] + [float(v) for v in items[1:5]])
    return out


def _pad_amounts(h, w):
    """(left, right, top, bottom) of ``pad_to_square`` (datasets.py:16-27)."""
    diff = abs(h - w)
    pad1, pad2 = diff // 2, diff - diff // 2
    return (0, 0, pad1, pad2) if h <= w else (pad1, pad2, 0, 0)


def read_label_rows(label_path):
    """A YOLO label file as a float64 ``[k,5]`` tensor ``(class, cx, cy, w, h)`` (``np.loadtxt``, like the reference)."""
    return torch.from_numpy(np.loadtxt(label_path).reshape(-1, 5))


def letterbox_labels(lab, scale_hw, pad, padded_hw):
    """Label geometry shared by both producers (stage 3 ``MyDataset``, stage 2 ``module2.ListDataset``).

    ``lab``: float64 ``[k,5]`` rows ``(class, cx, cy, w, h)``; ``scale_hw = (sy, sx)`` turns its coordinates into pixels of
    the *unpadded* frame (the frame's height / width for normalised labels, ``(1, 1)`` for pixel labels); ``pad`` is
    ``_pad_amounts`` of that frame, ``padded_hw`` the padded size.  Returns float32 ``[k,6]`` rows ``(0, class, cx, cy, w, h)``
    relative to the padded square.  float64 arithmetic in the reference's order (module3 ``datasets.py:224-245``, module2
    ``utils/datasets.py:111-135``): corners in pixels, each shifted by the padding on its side, centre back to [0,1];
    extents scaled by one python-float ratio."""
    sy, sx = scale_hw
    padded_h, padded_w = padded_hw
    half_w, half_h = lab[:, 3] / 2, lab[:, 4] / 2
    left = (lab[:, 1] - half_w) * sx + pad[0]
    right = (lab[:, 1] + half_w) * sx + pad[1]
    top = (lab[:, 2] - half_h) * sy + pad[2]
    bottom = (lab[:, 2] + half_h) * sy + pad[3]
    out = torch.zeros((len(lab), 6))
    out[:, 1] = lab[:, 0]
    out[:, 2] = ((left + right) / 2) / padded_w
    out[:, 3] = ((top + bottom) / 2) / padded_h
    out[:, 4] = lab[:, 3] * (sx / padded_w)
    out[:, 5] = lab[:, 4] * (sy / padded_h)
    return out


def decode_rgb_u8(img_path):
    """PIL decode -> uint8 ``[h,w,3]`` tensor (the only image work left on the host)."""
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(img_path).convert("RGB"), dtype=np.uint8))


class StagedImages:
    """A batch of decoded frames waiting for ``.to(device)``: uint8 HWC tensors + the target side."""

    def __init__(self, frames, size, flips=None):
        self.frames, self.size = list(frames), int(size)
        # stage-2 augmentation (module2_mixed/utils/datasets.py:143-146): mirror the padded square before the resize
        self.flips = [bool(f) for f in flips] if flips is not None else [False] * len(self.frames)
        self.shape = torch.Size((len(self.frames), 3, self.size, self.size))
        self.dtype = torch.float32

    def __len__(self):
        return len(self.frames)

    def size_(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def to(self, device, *_, **__):
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.MeError("StagedImages.to(): the batch is assembled by the HIP library - CUDA device required")
        lib = hip.lib()
        out = torch.empty(tuple(self.shape), device=device, dtype=torch.float32)
        stream = hip.stream_ptr()
        for i, frame in enumerate(self.frames):
            h, w, c = frame.shape
            if c != 3 or frame.dtype != torch.uint8:
                raise hip.MeError(f"frame {i}: expected uint8 [h,w,3], got {frame.dtype} {tuple(frame.shape)}")
            d = frame.contiguous().to(device, non_blocking=True)
            hip.check(lib.me_image_pad_resize_flip_u8_f32(d.data_ptr(), h, w, out[i].data_ptr(), self.size,
                                                          int(self.flips[i]), stream), "me_image_pad_resize_flip_u8_f32")
        return out


PIXEL_FORMATS = {"rgb": 0, "bgr": 1, "nv12": 2, "yuyv": 3}   # name -> ME_PIXFMT_* (include/millieye_hip.h)


def pixel_format_names(pixel_format, n, what="frame"):
    """One pixel format name, or one per frame, as a list of ``n`` checked names (:data:`PIXEL_FORMATS`)."""
    names = list(pixel_format) if isinstance(pixel_format, (list, tuple)) else [pixel_format] * n
    if len(names) != n:
        raise hip.MeError(f"{len(names)} pixel formats for {n} {what}s")
    for i, name in enumerate(names):
        if not isinstance(name, str) or name not in PIXEL_FORMATS:
            raise hip.MeError(f"{what} {i}: unknown pixel format {name!r} (one of {', '.join(PIXEL_FORMATS)})")
    return names


def picture_hw(frame, pixel_format="rgb", what="frame"):
    """Height and width in pixels of the picture a uint8 frame tensor holds in ``pixel_format``: ``"rgb"`` / ``"bgr"``
    ``[h,w,3]``, ``"yuyv"`` ``[h,w,2]`` (w even), ``"nv12"`` ``[h*3//2, w]`` (h and w even; the Y plane over the interleaved UV
    plane, the way cv2 and video decoders hand it over).  Raises :class:`hip.MeError` for anything else."""
    if not isinstance(pixel_format, str) or pixel_format not in PIXEL_FORMATS:
        raise hip.MeError(f"{what}: unknown pixel format {pixel_format!r} (one of {', '.join(PIXEL_FORMATS)})")
    shape, dtype = tuple(frame.shape), frame.dtype
    if pixel_format == "nv12":
        expected = "uint8 [h*3//2, w] with h and w even"
        # 3h/2 rows: a row count divisible by 3 is an even h
        ok = len(shape) == 2 and shape[0] > 0 and shape[0] % 3 == 0 and shape[1] > 0 and shape[1] % 2 == 0
        hw = (shape[0] // 3 * 2, shape[1]) if ok else None
    elif pixel_format == "yuyv":
        expected = "uint8 [h,w,2] with w even"
        ok = len(shape) == 3 and shape[2] == 2 and shape[0] > 0 and shape[1] > 0 and shape[1] % 2 == 0
        hw = shape[:2] if ok else None
    else:
        expected = "uint8 [h,w,3]"
        ok = len(shape) == 3 and shape[2] == 3 and shape[0] > 0 and shape[1] > 0
        hw = shape[:2] if ok else None
    if not ok or str(dtype) not in ("torch.uint8", "uint8"):   # (a tensor or a numpy array)
        raise hip.MeError(f"{what}: {pixel_format} expects {expected}, got {dtype} {shape}")
    return int(hw[0]), int(hw[1])


RESIZE_MODES = ("nearest", "area")


def resize_mode(resize, what="resize"):
    """``None`` or one checked name of :data:`RESIZE_MODES`."""
    if resize is not None and (not isinstance(resize, str) or resize not in RESIZE_MODES):
        raise hip.MeError(f"{what}: unknown resize mode {resize!r} (one of {', '.join(RESIZE_MODES)})")
    return resize


class PackBufferTooSmall(hip.MeError):
    """``StagedRaggedImages.pack(out=)``: the frames' bytes do not fit ``out`` (the message names both counts)."""


class StagedRaggedImages(StagedImages):
    """A ``StagedImages`` whose ``.to(device)`` builds the whole batch in one launch: every frame's bytes are packed into one
    pinned uint8 buffer and uploaded once, with a ``[n,4]`` int64 descriptor ``(byte offset, h, w, flip)`` per frame, and
    ``me_image_batch_pad_resize_flip_u8_f32`` writes ``[n,3,size,size]`` (bit-identical to the per-frame kernel).  ``.type()``
    accepts the CUDA float tensor types, for callers that write ``imgs.type(torch.cuda.FloatTensor)``.

    ``formats``: one name of :data:`PIXEL_FORMATS` or one per frame - the frames are what a camera or a decoder hands over
    (shapes: :func:`picture_hw`), their native bytes are packed, the descriptor is ``[n,5]`` ``(byte offset, h, w, flip,
    format id)`` with the picture's ``h, w``, and ``me_image_batch_formats_u8_f32`` converts on the device: a frame gives the
    bits its RGB conversion gives on the default path.  ``formats=None`` is the default path.

    ``resize``: a name of :data:`RESIZE_MODES`.  ``None`` / ``"nearest"``: the reference's ``F.interpolate(mode="nearest")``,
    everything above as it is.  ``"area"``: ``F.interpolate(padded_square, size, mode="area")`` - every source pixel is
    averaged into the output instead of one in ``(P / size)^2`` being kept - by ``me_image_batch_area_u8_f32``, always with the
    ``[n,5]`` descriptor (``formats=None``: all RGB).  The reference's scripts have no such option; the result is pinned to
    torch's float64 ``area`` interpolation of the padded ``u8 / 255`` square rounded to float32, which the kernel's integer
    arithmetic gives exactly (include/millieye_hip.h).  It needs ``max(h, w) <= 255 * size`` per frame (``pack()`` raises
    otherwise); with ``max(h, w) == size`` it gives the bits of the nearest path, and the geometry is the same, so box
    rescaling does not change.

    ``size=(H, W)``: the batch is ``[n,3,H,W]`` - every frame letterboxed by ``utils.utils.letterbox_geometry`` (padded with
    zeros to the smallest rectangle of the canvas's aspect ratio that holds it, both axes may be padded, mirrored if asked) and
    resized with one nearest ``F.interpolate(size=(H, W))`` by ``me_image_batch_letterbox_u8_f32``, always with the ``[n,5]``
    descriptor (``formats=None``: all RGB).  The reference has no rectangular input; the result is torch's own
    ``F.interpolate(F.pad(u8 / 255), size=(H, W), mode="nearest")`` bit for bit.  ``(S, S)`` is ``S``.  ``resize="area"`` with a
    rectangular size raises :class:`hip.MeError` here: there is no rectangular area kernel."""

    packed = desc = None   # set by pack(): the frames' bytes in one uint8 buffer and the [n,4] ([n,5]) int64 descriptor
    formats = None         # None: packed RGB and the [n,4] descriptor; else one checked name per frame
    resize = None          # None / "nearest": the nearest kernels; "area": me_image_batch_area_u8_f32
    rect = None            # (H, W) of a rectangular canvas: me_image_batch_letterbox_u8_f32
    ring_slot = None       # set by lend_to_ring(): ``packed`` lies in this slot of a handover.FrameRing and does not pickle
    ring_total = 0         # ... and holds this many bytes
    uploaded = None        # set by to(): (the packed bytes on the device, the CPU descriptor) of the last upload

    def __init__(self, frames, size, flips=None, formats=None, resize=None):
        size = canvas_size(size, "StagedRaggedImages size")
        self.rect = size if isinstance(size, tuple) else None   # (H, W) of a rectangular canvas
        super().__init__(frames, size[0] if self.rect else size, flips)
        self.resize = resize_mode(resize, "StagedRaggedImages")
        if self.rect:
            if self.resize == "area":
                raise hip.MeError(f"StagedRaggedImages: resize='area' has no rectangular form (size {self.rect[0]} x "
                                  f"{self.rect[1]})")
            self.size = self.rect
            self.shape = torch.Size((len(self.frames), 3) + self.rect)
        if formats is not None:
            self.formats = pixel_format_names(formats, len(self.frames))
        if formats is not None or self.resize == "area" or self.rect:
            self.frames = [torch.as_tensor(f) for f in self.frames]

    def _format_descriptor(self):
        """The ``[n,5]`` descriptor of the native frames and their byte total; checks every frame (:func:`picture_hw`)."""
        desc = torch.empty((len(self.frames), 5), dtype=torch.int64)
        total = 0
        for i, (frame, name) in enumerate(zip(self.frames, self.formats or ["rgb"] * len(self.frames))):
            h, w = picture_hw(frame, name, f"frame {i}")
            if self.resize == "area" and max(h, w) > 255 * self.size:
                raise hip.MeError(f"frame {i}: {h} x {w} is beyond the area resize's range max(h, w) <= 255 * size = "
                                  f"{255 * self.size}")
            desc[i] = torch.tensor([total, h, w, int(self.flips[i]), PIXEL_FORMATS[name]])
            total += frame.numel()
        return desc, total

    def pack(self, pin=False, keep_frames=True, out=None):
        """The host half of :meth:`to`, callable ahead of time and without a GPU (``pin=False``): checks the frames and copies
        their bytes into one buffer.  The object then carries ``packed`` / ``desc`` (through pickle too) and :meth:`to` only
        uploads them; ``keep_frames=False`` drops the per-frame tensors so that the bytes travel once.

        ``out``: a 1-D contiguous uint8 CPU tensor the bytes go straight into - a slot of a ``handover.FrameRing`` - instead of a
        fresh buffer; ``packed`` is ``out[:total]`` and the bytes behind ``total`` are not touched.  A too-small ``out`` raises
        :class:`PackBufferTooSmall` (a :class:`hip.MeError`) after all the checks and before a byte is written."""
        n = len(self.frames)
        if self.formats is not None or self.resize == "area" or self.rect:
            desc, total = self._format_descriptor()
        else:
            desc = torch.empty((n, 4), dtype=torch.int64)
            total = 0
            for i, frame in enumerate(self.frames):
                h, w, c = frame.shape
                if c != 3 or frame.dtype != torch.uint8 or h <= 0 or w <= 0:
                    raise hip.MeError(f"frame {i}: expected uint8 [h,w,3], got {frame.dtype} {tuple(frame.shape)}")
                desc[i, 0], desc[i, 1], desc[i, 2], desc[i, 3] = total, h, w, int(self.flips[i])
                total += h * w * 3
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 1 or out.device.type != "cpu" \
                    or not out.is_contiguous():
                raise hip.MeError("StagedRaggedImages.pack(out=): a 1-D contiguous uint8 CPU tensor is expected (got "
                                  f"{getattr(out, 'dtype', type(out).__name__)} {tuple(getattr(out, 'shape', ()))})")
            if int(out.numel()) < total:
                raise PackBufferTooSmall(f"StagedRaggedImages.pack(out=): the frames hold {total} bytes, out holds "
                                         f"{int(out.numel())}")
            packed = out[:total]
        else:
            packed = torch.empty((total,), dtype=torch.uint8, pin_memory=pin)
        for i, frame in enumerate(self.frames):
            start = int(desc[i, 0])
            packed[start:start + frame.numel()].copy_(frame.reshape(-1))
        self.packed, self.desc = packed, desc
        if not keep_frames:
            self.frames = []
        return self

    # A packed object whose bytes lie in slot ``ring_slot`` of a ``handover.FrameRing`` (``lend_to_ring``, after
    # ``pack(out=ring.slot(i))``) pickles without them: the slot index and the byte total travel, and the receiver binds the
    # object to its own mapping of the same ring (``bind``) before ``to()``.  Any other object pickles as it always did.
    def lend_to_ring(self, slot):
        if self.packed is None:
            raise hip.MeError("StagedRaggedImages.lend_to_ring(): pack(out=ring.slot(i)) first")
        self.ring_slot, self.ring_total = int(slot), int(self.packed.numel())
        return self

    def bind(self, ring):
        if self.ring_slot is None:
            raise hip.MeError("StagedRaggedImages.bind(): the object's bytes do not lie in a ring")
        slot = ring.slot(self.ring_slot)
        if self.ring_total > int(slot.numel()):
            raise hip.MeError(f"StagedRaggedImages.bind(): {self.ring_total} bytes in a slot of {int(slot.numel())}")
        self.packed = slot[:self.ring_total]
        return self

    def unbind(self):
        """Forget the slot's bytes (the slot is about to be given back); ``to()`` then raises until the next ``bind``."""
        if self.ring_slot is not None:
            self.packed = None
        return self

    def __getstate__(self):
        if self.ring_slot is None:
            return self.__dict__
        state = dict(self.__dict__)
        state["packed"] = None
        return state

    def __len__(self):
        return int(self.shape[0])

    def to(self, device, *_, **__):
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.MeError("StagedRaggedImages.to(): the batch is assembled by the HIP library - CUDA device required")
        if self.packed is None and self.ring_slot is not None:
            raise hip.MeError(f"StagedRaggedImages.to(): the bytes lie in slot {self.ring_slot} of a FrameRing - bind(ring) first")
        n = int(self.shape[0])
        out = torch.empty(tuple(self.shape), device=device, dtype=torch.float32)
        if n == 0:
            return out
        src = self if self.packed is not None else StagedRaggedImages(self.frames, self.size, self.flips, self.formats,
                                                                      self.resize).pack(pin=True)
        packed, desc = src.packed, src.desc
        total = int(packed.numel())
        d_src = packed.to(device, non_blocking=True)
        d_desc = desc.pin_memory().to(device, non_blocking=True)
        self.uploaded = (d_src, desc)   # the bytes the launch reads, kept for whoever draws into them (frame_overlay)
        if self.rect:
            hip.check(hip.lib().me_image_batch_letterbox_u8_f32(d_src.data_ptr(), total, d_desc.data_ptr(), n, out.data_ptr(),
                                                                self.rect[0], self.rect[1], hip.stream_ptr()),
                      "me_image_batch_letterbox_u8_f32")
            return out
        if self.resize == "area":
            hip.check(hip.lib().me_image_batch_area_u8_f32(d_src.data_ptr(), total, d_desc.data_ptr(), n, out.data_ptr(),
                                                           self.size, hip.stream_ptr()), "me_image_batch_area_u8_f32")
            return out
        if self.formats is not None:
            hip.check(hip.lib().me_image_batch_formats_u8_f32(d_src.data_ptr(), total, d_desc.data_ptr(), n, out.data_ptr(),
                                                              self.size, hip.stream_ptr()), "me_image_batch_formats_u8_f32")
            return out
        hip.check(hip.lib().me_image_batch_pad_resize_flip_u8_f32(d_src.data_ptr(), total, d_desc.data_ptr(), n,
                                                                   out.data_ptr(), self.size, hip.stream_ptr()),
                  "me_image_batch_pad_resize_flip_u8_f32")
        return out

    def device_surfaces(self):
        """After :meth:`to`: every frame as a dense :class:`FrameSurface` on the uploaded bytes the input launch read."""
        if self.uploaded is None:
            raise hip.MeError("StagedRaggedImages.device_surfaces(): to(device) first")
        d_src, desc = self.uploaded
        names = self.formats or ["rgb"] * int(desc.shape[0])
        return [FrameSurface(d_src, int(desc[i, 1]), int(desc[i, 2]), names[i], int(desc[i, 0])) for i in range(int(desc.shape[0]))]

    def type(self, dtype=None, non_blocking=False, **__):
        if dtype is None:
            return "torch.cuda.FloatTensor"
        name = dtype if isinstance(dtype, str) else f"{getattr(dtype, '__module__', '')}.{getattr(dtype, '__name__', '')}"
        if name != "torch.cuda.FloatTensor":
            raise hip.MeError(f"StagedRaggedImages.type({dtype!r}): the batch is built on the GPU as torch.cuda.FloatTensor")
        return self.to("cuda")


_ROW_BYTES_PER_PIXEL = {"rgb": 3, "bgr": 3, "yuyv": 2, "nv12": 1}   # bytes of plane 0 per pixel of a row


class FrameSurface:
    """A picture where it lies: ``h x w`` pixels in ``pixel_format`` inside ``buffer`` (a 1-D contiguous uint8 torch tensor on
    the CPU or on a CUDA device), its first byte at ``offset``, consecutive rows ``pitch`` bytes apart (``None``: dense rows).
    NV12 has its interleaved UV plane at ``uv_offset`` (``None``: ``offset + h * pitch``, right behind the Y plane) with rows
    ``uv_pitch`` bytes apart (``None``: ``pitch``).  This is what a V4L2 buffer (``bytesperline``), a hardware decoder (aligned
    pitch, UV plane behind an aligned height, in device memory) or a slice of a larger frame looks like;
    :class:`StagedSurfaces` reads it without a gather into a dense tensor.

    The constructor applies the validity rules of ``me_image_batch_surfaces_u8_f32`` (include/millieye_hip.h) on the host and
    raises :class:`hip.MeError` naming the rule and the numbers.  ``origin`` is ``(x0, y0)`` of this picture in the picture the
    surface was first built on: ``(0, 0)`` at construction, accumulated by :meth:`crop`.

    A surface on a CUDA buffer does not pickle (a device buffer does not cross a process boundary)."""

    origin = (0, 0)

    def __init__(self, buffer, h, w, pixel_format="rgb", offset=0, pitch=None, uv_offset=None, uv_pitch=None):
        if not isinstance(pixel_format, str) or pixel_format not in PIXEL_FORMATS:
            raise hip.MeError(f"FrameSurface: unknown pixel format {pixel_format!r} (one of {', '.join(PIXEL_FORMATS)})")
        if not isinstance(buffer, torch.Tensor) or buffer.dtype != torch.uint8 or buffer.dim() != 1 \
                or not buffer.is_contiguous() or buffer.device.type not in ("cpu", "cuda"):
            raise hip.MeError("FrameSurface: buffer must be a 1-D contiguous uint8 torch tensor on the CPU or a CUDA device (got "
                              f"{getattr(buffer, 'dtype', type(buffer).__name__)} {tuple(getattr(buffer, 'shape', ()))})")
        self.buffer, self.pixel_format = buffer, pixel_format
        self.h, self.w, self.offset = int(h), int(w), int(offset)
        nv12 = pixel_format == "nv12"
        row = _ROW_BYTES_PER_PIXEL[pixel_format] * self.w
        self.pitch = row if pitch is None else int(pitch)
        self.uv_offset = (self.offset + self.h * self.pitch if uv_offset is None else int(uv_offset)) if nv12 else 0
        self.uv_pitch = (self.pitch if uv_pitch is None else int(uv_pitch)) if nv12 else 0
        self._check(row)

    def _check(self, row):
        h, w, off, pitch, nbytes = self.h, self.w, self.offset, self.pitch, int(self.buffer.numel())
        what = f"FrameSurface ({self.pixel_format} {h} x {w})"
        if nbytes <= 0 or self.buffer.data_ptr() == 0:
            raise hip.MeError(f"{what}: the buffer is empty (bytes > 0 and base != 0 are required)")
        if not (1 <= h <= 1 << 30 and 1 <= w <= 1 << 30):
            raise hip.MeError(f"{what}: 1 <= h, w <= 2^30 is required")
        if self.pixel_format == "nv12" and (h % 2 or w % 2):
            raise hip.MeError(f"{what}: nv12 needs h and w even")
        if self.pixel_format == "yuyv" and w % 2:
            raise hip.MeError(f"{what}: yuyv needs w even")
        if pitch < row:
            raise hip.MeError(f"{what}: pitch {pitch} is below the row's {row} bytes (pitch >= row; no negative pitches)")
        if not 0 <= off <= nbytes - row:
            raise hip.MeError(f"{what}: offset {off} is outside [0, bytes - row] = [0, {nbytes} - {row}]")
        if h - 1 > (nbytes - row - off) // pitch:
            raise hip.MeError(f"{what}: the last row ends at byte {off + (h - 1) * pitch + row} of a buffer of {nbytes} "
                              f"(offset {off}, pitch {pitch})")
        if self.pixel_format == "nv12":
            uv_off, uv_pitch = self.uv_offset, self.uv_pitch
            if uv_pitch < w:
                raise hip.MeError(f"{what}: uv_pitch {uv_pitch} is below the chroma row's {w} bytes (uv_pitch >= w)")
            if not 0 <= uv_off <= nbytes - w:
                raise hip.MeError(f"{what}: uv_offset {uv_off} is outside [0, bytes - w] = [0, {nbytes} - {w}]")
            if h // 2 - 1 > (nbytes - w - uv_off) // uv_pitch:
                raise hip.MeError(f"{what}: the last chroma row ends at byte {uv_off + (h // 2 - 1) * uv_pitch + w} of a buffer "
                                  f"of {nbytes} (uv_offset {uv_off}, uv_pitch {uv_pitch})")

    @property
    def row_bytes(self):
        return _ROW_BYTES_PER_PIXEL[self.pixel_format] * self.w

    def span(self):
        """``(lo, hi)``: the byte range of the buffer the picture's rows touch (both planes of NV12)."""
        lo, hi = self.offset, self.offset + (self.h - 1) * self.pitch + self.row_bytes
        if self.pixel_format == "nv12":
            lo = min(lo, self.uv_offset)
            hi = max(hi, self.uv_offset + (self.h // 2 - 1) * self.uv_pitch + self.w)
        return lo, hi

    def row(self, base, nbytes, rebase=0, flip=False):
        """The surface's row of the ``[n,10]`` descriptor when ``nbytes`` of its buffer, from byte ``rebase`` on, lie at the
        device address ``base``."""
        return [int(base), int(nbytes), self.offset - rebase, self.h, self.w, int(bool(flip)), PIXEL_FORMATS[self.pixel_format],
                self.pitch, self.uv_offset - rebase if self.pixel_format == "nv12" else 0, self.uv_pitch]

    def crop(self, x0, y0, cw, ch):
        """The ``ch x cw`` region at column ``x0``, row ``y0`` as a new surface on the same buffer: offset arithmetic, no copy.
        YUYV needs ``x0`` and ``cw`` even, NV12 all four (whole chroma samples)."""
        x0, y0, cw, ch = int(x0), int(y0), int(cw), int(ch)
        what = f"FrameSurface.crop({x0}, {y0}, {cw}, {ch}) of {self.pixel_format} {self.h} x {self.w}"
        if x0 < 0 or y0 < 0 or cw < 1 or ch < 1 or x0 + cw > self.w or y0 + ch > self.h:
            raise hip.MeError(f"{what}: the region does not lie inside the picture")
        if self.pixel_format == "yuyv" and (x0 % 2 or cw % 2):
            raise hip.MeError(f"{what}: yuyv needs x0 and the width even")
        if self.pixel_format == "nv12" and (x0 % 2 or y0 % 2 or cw % 2 or ch % 2):
            raise hip.MeError(f"{what}: nv12 needs x0, y0, the width and the height even")
        nv12 = self.pixel_format == "nv12"
        out = FrameSurface(self.buffer, ch, cw, self.pixel_format,
                           self.offset + y0 * self.pitch + _ROW_BYTES_PER_PIXEL[self.pixel_format] * x0, self.pitch,
                           self.uv_offset + (y0 // 2) * self.uv_pitch + x0 if nv12 else None, self.uv_pitch if nv12 else None)
        out.origin = (self.origin[0] + x0, self.origin[1] + y0)
        return out

    @classmethod
    def from_view(cls, tensor, pixel_format="rgb"):
        """The surface of a uint8 ``[h,w,3]`` (``"rgb"`` / ``"bgr"``) or ``[h,w,2]`` (``"yuyv"``) torch tensor or numpy array
        whose innermost two dimensions are dense and whose row stride is at least the row's bytes - a slice
        ``full[y0:y1, x0:x1]``, a V4L2 buffer viewed with its ``bytesperline`` - built on the tensor's storage without a copy.
        Any other stride pattern raises and names the strides; so does ``"nv12"`` (two planes are not one view)."""
        if pixel_format == "nv12":
            raise hip.MeError("FrameSurface.from_view: nv12 has two planes, which one view cannot describe - build the "
                              "FrameSurface with uv_offset / uv_pitch")
        h, w = picture_hw(tensor, pixel_format, "FrameSurface.from_view")
        t = torch.as_tensor(tensor)
        c, strides = int(t.shape[2]), tuple(int(s) for s in t.stride())
        if strides[2] != 1 or strides[1] != c or (h > 1 and strides[0] < w * c):
            raise hip.MeError(f"FrameSurface.from_view: strides {strides} of a {tuple(t.shape)} view are not (pitch >= {w * c}, "
                              f"{c}, 1)")
        storage = t.untyped_storage()
        buffer = torch.empty(0, dtype=torch.uint8, device=t.device).set_(storage, 0, (storage.nbytes(),), (1,))
        return cls(buffer, h, w, pixel_format, int(t.storage_offset()), strides[0] if h > 1 else w * c)

    def __getstate__(self):
        if self.buffer.device.type != "cpu":
            raise hip.MeError(f"FrameSurface: a surface on a {self.buffer.device} buffer does not pickle (a device buffer does "
                              "not cross a process boundary)")
        return self.__dict__


class StagedSurfaces:
    """A batch of :class:`FrameSurface` waiting for ``.to(device)``: the sibling of :class:`StagedRaggedImages` that reads the
    frames where they lie.  ``to("cuda")`` uploads, per distinct CPU buffer and in one ``non_blocking`` copy, the byte span from
    the lowest to the highest byte any of its surfaces touches (a pitched V4L2 buffer goes up as it is, a region of interest
    takes only its rows along), uploads nothing for CUDA buffers, and makes one ``me_image_batch_surfaces_u8_f32`` launch with a
    ``[n,10]`` descriptor per frame: ``[n,3,size,size]`` (``[n,3,H,W]`` for ``size=(H, W)``), every frame bit-identical to what
    :class:`StagedRaggedImages` gives on its pixels copied into a dense frame.  ``flips``, ``resize`` and ``size`` mean what they
    mean there; ``resize="area"`` with a rectangular size raises here as well.

    The surfaces' buffers must stay alive until the launch has run; tensors used on the current stream do (torch's allocator
    is stream-ordered)."""

    def __init__(self, surfaces, size, flips=None, resize=None):
        self.surfaces = list(surfaces)
        size = canvas_size(size, "StagedSurfaces size")
        self.size = size
        self.resize = resize_mode(resize, "StagedSurfaces")
        if isinstance(size, tuple) and self.resize == "area":
            raise hip.MeError(f"StagedSurfaces: resize='area' has no rectangular form (size {size[0]} x {size[1]})")
        self.flips = [bool(f) for f in flips] if flips is not None else [False] * len(self.surfaces)
        if len(self.flips) != len(self.surfaces):
            raise hip.MeError(f"StagedSurfaces: {len(self.flips)} flips for {len(self.surfaces)} surfaces")
        for i, s in enumerate(self.surfaces):
            if not isinstance(s, FrameSurface):
                raise hip.MeError(f"StagedSurfaces: surface {i} is a {type(s).__name__}, not a FrameSurface")
            if self.resize == "area" and max(s.h, s.w) > 255 * size:
                raise hip.MeError(f"surface {i}: {s.h} x {s.w} is beyond the area resize's range max(h, w) <= 255 * size = "
                                  f"{255 * size}")
        self.shape = torch.Size((len(self.surfaces), 3) + canvas_hw(size))
        self.dtype = torch.float32
        self.uploaded = None   # set by to(): the device copies of the CPU spans of the last upload

    def __len__(self):
        return len(self.surfaces)

    def plan(self):
        """The host half of :meth:`to`, without a GPU: ``(spans, where)`` - ``spans`` lists ``[buffer, lo, hi]`` per distinct CPU
        buffer, the byte range its surfaces touch; ``where[i]`` is the span surface ``i`` reads from, ``None`` for a surface on
        a CUDA buffer."""
        spans, where, index = [], [], {}
        for s in self.surfaces:
            if s.buffer.device.type != "cpu":
                where.append(None)
                continue
            key, (lo, hi) = (s.buffer.data_ptr(), int(s.buffer.numel())), s.span()
            if key not in index:
                index[key] = len(spans)
                spans.append([s.buffer, lo, hi])
            else:
                span = spans[index[key]]
                span[1], span[2] = min(span[1], lo), max(span[2], hi)
            where.append(index[key])
        return spans, where

    def descriptor(self, addresses):
        """The ``[n,10]`` int64 descriptor when span ``k`` of :meth:`plan` lies at the device address ``addresses[k]``: the
        surfaces of a CPU buffer are rebased onto its span, a CUDA buffer is named as it is."""
        spans, where = self.plan()
        rows = []
        for s, k, flip in zip(self.surfaces, where, self.flips):
            if k is None:
                rows.append(s.row(s.buffer.data_ptr(), s.buffer.numel(), 0, flip))
            else:
                rows.append(s.row(addresses[k], spans[k][2] - spans[k][1], spans[k][1], flip))
        return torch.tensor(rows, dtype=torch.int64).reshape(-1, 10)

    def to(self, device, *_, **__):
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.MeError("StagedSurfaces.to(): the batch is assembled by the HIP library - CUDA device required")
        n = len(self.surfaces)
        out = torch.empty(tuple(self.shape), device=device, dtype=torch.float32)
        if n == 0:
            return out
        for i, s in enumerate(self.surfaces):
            if s.buffer.device.type == "cuda" and s.buffer.device != out.device:
                raise hip.MeError(f"StagedSurfaces.to({out.device}): surface {i} lies on {s.buffer.device}")
        spans, _ = self.plan()
        uploads = [buffer[lo:hi].to(device, non_blocking=True) for buffer, lo, hi in spans]
        self.uploaded = uploads   # the spans the launch reads, kept for whoever draws into them (device_surfaces)
        d_desc = self.descriptor([u.data_ptr() for u in uploads]).pin_memory().to(device, non_blocking=True)
        height, width = canvas_hw(self.size)
        hip.check(hip.lib().me_image_batch_surfaces_u8_f32(d_desc.data_ptr(), n, out.data_ptr(), height, width,
                                                           int(self.resize == "area"), hip.stream_ptr()),
                  "me_image_batch_surfaces_u8_f32")
        return out

    def device_surfaces(self):
        """After :meth:`to`: every picture as a :class:`FrameSurface` in device memory - a surface on a CUDA buffer as it is, a
        surface on a CPU buffer rebased onto the upload of its span (the bytes the input launch read)."""
        if self.uploaded is None:
            raise hip.MeError("StagedSurfaces.device_surfaces(): to(device) first")
        spans, where = self.plan()
        out = []
        for s, k in zip(self.surfaces, where):
            if k is None:
                out.append(s)
                continue
            lo, nv12 = spans[k][1], s.pixel_format == "nv12"
            out.append(FrameSurface(self.uploaded[k], s.h, s.w, s.pixel_format, s.offset - lo, s.pitch,
                                    s.uv_offset - lo if nv12 else None, s.uv_pitch if nv12 else None))
        return out

    def type(self, dtype=None, non_blocking=False, **__):
        if dtype is None:
            return "torch.cuda.FloatTensor"
        name = dtype if isinstance(dtype, str) else f"{getattr(dtype, '__module__', '')}.{getattr(dtype, '__name__', '')}"
        if name != "torch.cuda.FloatTensor":
            raise hip.MeError(f"StagedSurfaces.type({dtype!r}): the batch is built on the GPU as torch.cuda.FloatTensor")
        return self.to("cuda")


class StagedRadarMaps:
    """Radar points of a batch waiting for ``.to(device)``: per frame ``[n_i,4]`` float64 (u, v, depth, velocity) and
    the original image size ``(w, h)``.

    ``map_size=(mh, mw)``: ``[n,3,mh,mw]`` maps for a rectangular network input (``me_radar_heatmap_rect_f32``): the same bins,
    padded by ``utils.utils.letterbox_geometry`` to the aspect ratio of ``mh x mw`` and resized with bilinear
    ``align_corners=True``.  This is the dataset's resized map, ``map_size = img_size / 16`` per side; the demos' raw 32 x 32
    map (quirk q15) has no rectangular form.  ``(m, m)`` is ``m``."""

    def __init__(self, points, sizes, map_size, radar_maps_size=32):
        self.points, self.sizes = list(points), list(sizes)
        self.map_size, self.radar_maps_size = canvas_size(map_size, "StagedRadarMaps map_size"), int(radar_maps_size)
        self.shape = torch.Size((len(self.points), 3) + canvas_hw(self.map_size))
        self.dtype = torch.float32

    def __len__(self):
        return len(self.points)

    def to(self, device, *_, **__):
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.MeError("StagedRadarMaps.to(): the maps are computed by the HIP library - CUDA device required")
        n = len(self.points)
        out = torch.empty(tuple(self.shape), device=device, dtype=torch.float32)
        if n == 0:
            return out
        rows = [np.asarray(p, dtype=np.float64).reshape(-1, 4) for p in self.points]
        offsets = np.zeros(n + 1, dtype=np.int32)
        offsets[1:] = np.cumsum([len(r) for r in rows])
        flat = np.concatenate(rows, 0) if offsets[-1] else np.zeros((1, 4), np.float64)
        d_pts = torch.from_numpy(np.ascontiguousarray(flat)).to(device)
        d_off = torch.from_numpy(offsets).to(device)
        d_sz = torch.tensor(self.sizes, dtype=torch.int32).reshape(n, 2).to(device)
        if isinstance(self.map_size, tuple):
            hip.check(hip.lib().me_radar_heatmap_rect_f32(d_pts.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), n,
                                                          self.radar_maps_size, out.data_ptr(), self.map_size[0],
                                                          self.map_size[1], hip.stream_ptr()), "me_radar_heatmap_rect_f32")
            return out
        hip.check(hip.lib().me_radar_heatmap_f32(d_pts.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), n,
                                                 self.radar_maps_size, out.data_ptr(), self.map_size, hip.stream_ptr()),
                  "me_radar_heatmap_f32")
        return out


class MyDataset(Dataset):
    """``__getitem__`` -> ``(img_path, frame_u8 [h,w,3], targets [k,6] | None, radar_box [r,5] | None, (points [n,4]
    float64, (w, h)))``; ``collate_fn`` -> ``(paths, StagedImages, targets [q,6], radar_boxes [r,5], StagedRadarMaps)``."""

    def __init__(self, mode, illumination, img_size=416, augment=False, multiscale=True, test_list=0,
                 dataset_folder="../data/our_dataset"):
        self.mode = mode
        self.illumination = illumination
        self.img_size = img_size
        self.map_size = int(self.img_size / 16)
        self.augment = augment
        self.multiscale = multiscale
        self.test_list = _SCENES[test_list:test_list + 1]
        self.train_list = _SCENES[:test_list] + _SCENES[test_list + 1:]
        self.max_objects = 100
        self.min_size = self.img_size - 3 * 32
        self.max_size = self.img_size + 3 * 32
        self.batch_count = 0
        self.chosen_classes = list(range(12))
        self.get_paths(dataset_folder)

    def get_paths(self, dataset_folder):
        """``dataset.txt`` lines look like ``<light><scene>-<...>-<appendix>``; the scene digit decides train / test
        (5-fold by ``test_list``), the light letter must be in ``illumination`` (datasets.py:156-194)."""
        split = {"train": dict(img=[], label=[], box=[], point=[]), "test": dict(img=[], label=[], box=[], point=[])}
        with open(f"{dataset_folder}/dataset.txt", "r") as fh:
            lines = [x.strip() for x in fh.read().split("\n") if x and not x.startswith("#")]
        for line in lines:
            head = line.split("-")[0]
            light, scene = head[0], head[1]
            _appendix = line.split("-")[2]  # the reference indexes it too: malformed lines must fail the same way
            if light not in self.illumination:
                continue
            for which, scenes in (("train", self.train_list), ("test", self.test_list)):
                if scene in scenes:
                    split[which]["img"].append(os.path.join(f"{dataset_folder}/image", line + ".jpg"))
                    split[which]["label"].append(os.path.join(f"{dataset_folder}/label", line + ".txt"))
                    split[which]["box"].append(os.path.join(f"{dataset_folder}/radar_box", line + ".pkl"))
                    split[which]["point"].append(os.path.join(f"{dataset_folder}/radar_point", line + ".pkl"))
        self.paths = split

    def __len__(self):
        return len(self.paths[self.mode]["img"])

    def __getitem__(self, idx):
        from PIL import Image

        sel = self.paths[self.mode]
        img_path, label_path, box_path, point_path = (sel[k][idx] for k in ("img", "label", "box", "point"))
        frame = torch.from_numpy(np.array(Image.open(img_path).convert("RGB"), dtype=np.uint8))  # [h,w,3]
        h, w = frame.shape[0], frame.shape[1]
        pad = _pad_amounts(h, w)
        padded_h, padded_w = h + pad[2] + pad[3], w + pad[0] + pad[1]

        targets = self._load_targets(label_path, (h, w), pad, (padded_h, padded_w))
        radar_box_output = self._load_radar_boxes(box_path, pad, padded_h)

        with open(point_path, "rb") as handle:
            points = np.asarray(pickle.load(handle), dtype=np.float64).reshape(-1, 4)  # (u, v, depth, velocity) rows
        return img_path, frame, targets, radar_box_output, (points, (w, h))

    @staticmethod
    def _load_targets(label_path, hw, pad, padded_hw):
        """``[k,6]`` target rows of one frame (``letterbox_labels``), or ``None`` without a label file."""
        if not os.path.exists(label_path):
            return None
        return letterbox_labels(read_label_rows(label_path), hw, pad, padded_hw)

    @staticmethod
    def _load_radar_boxes(box_path, pad, padded_side):
        """Radar proposals: pickled ``[r,4]`` xyxy pixels of the unpadded frame -> ``[r',5]`` rows ``(0, x1,y1,x2,y2)`` in
        [0,1] of the padded square (clamped, empty boxes dropped), or ``None`` (datasets.py:250-264)."""
        with open(box_path, "rb") as handle:
            rb = torch.from_numpy(pickle.load(handle))
        if len(rb) == 0:
            return None
        shift = torch.tensor([pad[0], pad[2], pad[1], pad[3]], dtype=rb.dtype)
        rb += shift  # in place on the unpickled array, like the reference's column-wise +=
        rb = torch.clamp(rb / padded_side, 0, 1)
        rb = rb[(rb[:, 0] < rb[:, 2]) & (rb[:, 1] < rb[:, 3])]
        if len(rb) == 0:
            return None
        out = torch.zeros((len(rb), 5))
        out[:, 1:] = rb
        return out

    def collate_fn(self, batch):
        paths, frames, targets, radar_boxes, radar_points = list(zip(*batch))
        for i, boxes in enumerate(targets):
            if boxes is not None:
                boxes[:, 0] = i
        for i, boxes in enumerate(radar_boxes):
            if boxes is not None:
                boxes[:, 0] = i
        targets = [b for b in targets if b is not None]
        targets = torch.cat(targets, 0) if len(targets) > 0 else torch.empty(0, 6)
        radar_boxes = [b for b in radar_boxes if b is not None]
        radar_boxes = torch.cat(radar_boxes, 0) if len(radar_boxes) > 0 else torch.empty(0, 5)
        if self.multiscale and self.batch_count % 10 == 0:  # a new input size every tenth batch (datasets.py:312-314)
            self.img_size = random.choice(range(self.min_size, self.max_size + 1, 32))
            self.map_size = int(self.img_size / 16)
        imgs = StagedImages(frames, self.img_size)
        radar_maps = StagedRadarMaps([p for p, _ in radar_points], [s for _, s in radar_points], self.map_size)
        self.batch_count += 1
        return paths, imgs, targets, radar_boxes, radar_maps
