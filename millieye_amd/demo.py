"""One camera frame + its radar frames through the whole fusion path, the way the live demos do it
(``module3_our_dataset/run_mp.py:65-160,296-330`` / ``run_sp.py:117-241``) - without the demos' I/O (video decoding,
serial-port capture, OpenCV window).  ``millieye_amd/pipeline.py`` runs the two halves of
:class:`FrameFuser` in two processes with run_mp's ``mp.Queue(maxsize=3)`` / ``mp.Event`` hand-over:

    radar frames --RadarProposalGenerator--> box proposals (pixels) + point cloud
    frame uint8 [h,w,3] --ToTensor / pad_to_square / resize(416)--> img [1,3,416,416]     (me_image_pad_resize_u8_f32)
    point cloud --plot_radar_heatmap / pad_to_square--> radar_map [1,3,32,32]              (me_radar_heatmap_f32, no resize:
                                                                                            the demos feed the raw map, quirk q15)
    proposals --+pad, /padded side, clamp, drop empty--> radar_box [k,5]                   (run_mp.py:120-135)
    mode: auto = fusion iff img.mean() < 0.08, else camera only                            (run_mp.py:204-212)
    Network.forward(img, radar_map, radar_box, mode)[:, 1:] -> batched_nms(.., 0.3) -> rescale_boxes to the frame

:class:`MultiStreamFuser` is the same step for S camera + radar nodes behind one card: the radar chain of every stream on the
device (``radar_proposals.DeviceRadarProposals``), one ragged-batch launch for the frames, one heat-map launch from the device
cloud, per-frame means for the mode rule, at most two ``Network.forward`` calls (the fusion frames, the camera-only frames) and
one pass over the network's rows for the output tail (``me_stream_tail_f32``: the second NMS of every stream and the rescale to
its frame, one copy back).  ``pipeline.FusionPipeline`` runs its host half (:func:`prepare_streams`) in the producer process.

``img_size=(H, W)`` on either fuser (and :func:`prepare_streams`) feeds the rectangular network: every frame, radar map and radar
box is letterboxed by ``utils.utils.letterbox_geometry`` and the rows come back through the per-axis ``rescale_boxes``.  The
reference has no counterpart (its ``YOLOLayer`` has one ``grid_size``); tests/letterbox_refs.py restates the step with stock torch.

Parity: every numeric stage is one of the pinned pieces (input kernels: tests/golden/dataset_small; Network.forward:
network_*.npz; NMS: nms_synth; radar proposals: radar_proposals_synth + the unpinned Kalman part); the glue in this file
restates run_mp's inline code and has no fixture of its own.
"""
import numpy as np
import torch

from . import hip
from .detection_range import range_detections, ranging_params
from .frame_overlay import dense_frame, draw_detections, overlay_params
from .radar_proposals import DeviceRadarProposals, RadarProposalGenerator
from .utils.datasets import (FrameSurface, StagedImages, StagedRadarMaps, StagedRaggedImages, StagedSurfaces, _pad_amounts,
                             picture_hw, pixel_format_names, resize_mode)
from .utils.utils import box_ops, canvas_size, letterbox_geometry, rescale_boxes, rescale_scalars

__all__ = ["mode_selection", "radar_boxes_for_network", "prepare_streams", "FrameFuser", "MultiStreamFuser"]


def mode_selection(mode, img, dark_threshold=0.08):
    """0 milliEye fusion, 1 camera only, 2 radar only, 3 auto: fusion when the frame is dark (run_mp.py:204-212; the offline
    evaluation uses 0.1, test_fusion.py:24-32)."""
    if mode in (0, 1, 2):
        return mode
    if mode == 3:
        return 0 if float(img.mean()) < dark_threshold else 1
    return None  # the reference falls off the end for other values


def _network_input_size(img_size, what):
    """``img_size`` of a fuser: an ``int`` is taken as it is (the square path, unchanged); ``(H, W)`` must have sides that are
    positive multiples of 32 (``Network.forward``'s rule) and ``(S, S)`` becomes ``S``."""
    return canvas_size(img_size, f"{what}: img_size", multiple=32) if isinstance(img_size, (tuple, list)) else img_size


def _rect_map_size(img_size):
    """The radar map of a rectangular input ``(H, W)``: the dataset's ``map_size = img_size / 16`` per side.  (The demos' raw
    32 x 32 map, quirk q15, which the square fusers feed, has no rectangular form.)"""
    return (img_size[0] // 16, img_size[1] // 16)


def radar_boxes_for_network(xyxy_pixels, frame_hw, canvas=None):
    """Pixel boxes of the un-padded frame -> ``[k,5]`` rows ``(0, x1, y1, x2, y2)`` in units of the padded square side,
    clamped to [0,1], empty boxes dropped (run_mp.py:119-135).

    ``canvas=(H, W)``: the frame is letterboxed into a rectangular network input (``utils.utils.letterbox_geometry``): the
    padding is split per axis, x is in units of the padded width ``Pw`` and y of the padded height ``Ph``.  ``(S, S)`` gives
    what ``None`` gives."""
    h, w = frame_hw
    boxes = torch.as_tensor(np.asarray(xyxy_pixels, dtype=np.float32).reshape(-1, 4))
    if len(boxes) == 0:
        return torch.zeros((0, 5))
    if canvas is not None:
        Ph, Pw, top, left = letterbox_geometry((h, w), canvas)
        boxes = boxes + torch.tensor([left, top, Pw - w - left, Ph - h - top], dtype=torch.float32)
        boxes = torch.clamp(boxes / torch.tensor([Pw, Ph, Pw, Ph], dtype=torch.float32), 0, 1)
    else:
        left, right, top, bottom = _pad_amounts(h, w)
        side = float(max(h, w))
        boxes = boxes + torch.tensor([left, top, right, bottom], dtype=torch.float32)
        boxes = torch.clamp(boxes / side, 0, 1)
    boxes = boxes[(boxes[:, 0] < boxes[:, 2]) & (boxes[:, 1] < boxes[:, 3])]
    out = torch.zeros((len(boxes), 5))
    out[:, 1:] = boxes
    return out


def _fuser_surface(frame, pixel_format, what):
    """A frame of a step that reads surfaces (``utils.datasets.FrameSurface``) as the surface a fuser may take: a surface is
    checked - its format is the stream's, and it is a whole picture: the radar chain projects into the full frame, so a
    cropped camera picture would no longer line up with the radar boxes and maps - and a frame tensor in ``pixel_format``
    (``None``: RGB) is wrapped, as a view where its strides allow it."""
    if isinstance(frame, FrameSurface):
        if pixel_format is not None and frame.pixel_format != pixel_format:
            raise hip.MeError(f"{what}: the surface holds {frame.pixel_format}, the stream's pixel_format is {pixel_format}")
        if tuple(frame.origin) != (0, 0):
            raise hip.MeError(f"{what}: a cropped surface (origin {tuple(frame.origin)}) would not line up with the radar "
                              "geometry - the fusers take whole pictures")
        return frame
    name = pixel_format or "rgb"
    frame = torch.as_tensor(frame)
    h, w = picture_hw(frame, name, what)
    if name == "nv12":   # the Y plane over the UV plane in one dense tensor
        return FrameSurface(frame.contiguous().reshape(-1), h, w, "nv12")
    c = int(frame.shape[2])
    if frame.stride(2) != 1 or frame.stride(1) != c or (h > 1 and frame.stride(0) < w * c):
        frame = frame.contiguous()
    return FrameSurface.from_view(frame, name)


class FrameFuser:
    """``fuser(frame_uint8_hwc, radar_frames)`` -> ``(detections [m,7], info)``; detections are rows
    ``(x1, y1, x2, y2, conf, cls_conf, cls_pred)`` in pixels of the original frame, like the demos draw them.

    ``pixel_format``: a name of ``utils.datasets.PIXEL_FORMATS`` - the camera's native frame.  ``resize``: ``None`` /
    ``"nearest"`` (the reference's resize) or ``"area"`` (``F.interpolate(mode="area")``, an option the reference does not have;
    semantics and range: ``StagedRaggedImages``).  Either one stages the frame through the ragged-batch kernels.

    ``img_size=(H, W)`` (sides multiples of 32): the frame is letterboxed to the rectangular network input
    (``utils.utils.letterbox_geometry``, ``me_image_batch_letterbox_u8_f32``), the radar boxes are normalised per axis, the radar
    map is the dataset's resized ``(H / 16, W / 16)`` map (the raw 32 x 32 map of the square path has no rectangular form) and
    the rows come back through the per-axis ``rescale_boxes``.  ``(S, S)`` is ``S``; ``resize="area"`` is refused.

    ``frame`` may be a ``utils.datasets.FrameSurface`` (a pitched or device-resident picture, read where it lies by
    ``StagedSurfaces``); its format must be ``pixel_format`` where that is given, and a cropped surface is refused.

    ``ranging``: ``None`` (default), ``True`` or a dict of ``shrink``, ``gate``, ``min_points`` - ``info`` gains ``"ranges"``,
    the ``[k,4]`` float64 rows ``(range_m, velocity_mps, points_used, points_inside)`` of
    ``detection_range.range_detections`` on the returned detections and the cloud of the host generator, and
    ``"range_status"`` (always 0 here), like :class:`MultiStreamFuser`'s.

    ``overlay``: ``None`` (default), ``True`` or a dict of ``frame_overlay.draw_detections`` style parameters - ``info`` gains
    ``"overlay"``, a numpy copy of the frame in its native layout with the returned detections (and their ranges, with
    ``ranging=``) drawn by ``draw_detections`` on the host, and ``"overlay_status"``.  The input frame is not touched."""

    def __init__(self, model, calib_param, model_mode=3, img_size=416, nms_iou=0.3, dark_threshold=0.08, generator=None,
                 pixel_format=None, resize=None, ranging=None, overlay=None, **generator_kwargs):
        self.model, self.model_mode, self.img_size = model, model_mode, _network_input_size(img_size, "FrameFuser")
        self.rect = isinstance(self.img_size, tuple)
        self.nms_iou, self.dark_threshold = nms_iou, dark_threshold
        # None: uint8 [h,w,3] RGB through the per-frame kernel; a name of utils.datasets.PIXEL_FORMATS: the camera's native
        # frame, staged through the ragged-batch kernel (bit-identical to the per-frame one on the converted frame)
        self.pixel_format = None if pixel_format is None else pixel_format_names(pixel_format, 1)[0]
        self.resize = resize_mode(resize, "FrameFuser")
        if self.rect and self.resize == "area":
            raise hip.MeError(f"FrameFuser: resize='area' has no rectangular form (img_size {self.img_size[0]} x "
                              f"{self.img_size[1]})")
        self.range_params = ranging_params(ranging, "FrameFuser")
        self.overlay_params = overlay_params(overlay, "FrameFuser")
        self.generator_is_default = generator is None   # pipeline.py: re-created in the producer vs sent by pickle
        self.generator = generator or RadarProposalGenerator(calib_param, **generator_kwargs)

    def __call__(self, frame, radar_frames):
        return self.infer(self.prepare(frame, radar_frames))

    # The two halves run_mp.py puts in two processes (millieye_amd/pipeline.py does the same): everything that needs only
    # the host - radar tracking, proposal arithmetic, staging of the raw frame bytes / point cloud - and everything that
    # needs the device.  ``prepare`` keeps the tracker state, so it must see the frames in order.
    def prepare(self, frame, radar_frames):
        """Host half (run_mp.py:65-152 ``pre_process``): a picklable payload for :meth:`infer`."""
        if isinstance(frame, FrameSurface):
            frame = _fuser_surface(frame, self.pixel_format, "FrameFuser")
            h, w = frame.h, frame.w
            img = StagedSurfaces([frame], self.img_size, resize=self.resize)
        elif self.pixel_format is not None or self.resize == "area" or self.rect:
            frame = torch.as_tensor(frame)
            h, w = picture_hw(frame, self.pixel_format or "rgb")
            img = StagedRaggedImages([frame], self.img_size, formats=self.pixel_format, resize=self.resize).pack()
        else:
            frame = torch.as_tensor(frame)
            if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
                raise hip.MeError(f"frame must be uint8 [h,w,3] (got {frame.dtype} {tuple(frame.shape)})")
            h, w = int(frame.shape[0]), int(frame.shape[1])
            img = StagedImages([frame], self.img_size)
        proposals, cloud = self.generator(radar_frames)
        canvas = {}
        if self.overlay_params is not None:   # a copy of the picture in its native layout for infer() to draw on
            if isinstance(frame, FrameSurface):
                canvas = dict(canvas=(dense_frame(frame), frame.pixel_format))
            else:
                canvas = dict(canvas=(frame.numpy().copy(), self.pixel_format or "rgb"))
        return dict(hw=(h, w), proposals=proposals, points=int(len(cloud)), **canvas,
                    cloud=np.array(cloud, dtype=np.float64).reshape(-1, 4),   # for ranging=: whichever fuser infers decides
                    radar_box=radar_boxes_for_network(proposals, (h, w), self.img_size if self.rect else None),
                    img=img, radar_map=StagedRadarMaps([cloud], [(w, h)],
                                                       map_size=_rect_map_size(self.img_size) if self.rect else 32))

    def infer(self, payload):
        """Device half (run_mp.py:296-330): input kernels, mode selection, ``Network.forward``, second NMS, rescale."""
        dev = getattr(self.model, "device", None) or hip.default_device()
        h, w = payload["hw"]
        radar_box = payload["radar_box"].to(dev)
        img = payload["img"].to(dev)
        radar_map = payload["radar_map"].to(dev)
        mode = mode_selection(self.model_mode, img, self.dark_threshold)
        with torch.no_grad():
            rows = self.model(img, radar_map, radar_box, mode)[:, 1:].cpu()
        keep = box_ops.batched_nms(rows[:, :4], rows[:, 4], rows[:, 6], self.nms_iou)
        rows = rows[keep]
        if len(rows):
            rescale_boxes(rows, self.img_size, (h, w))
        info = dict(mode=mode, proposals=payload["proposals"], radar_boxes=int(radar_box.shape[0]), points=payload["points"])
        if self.range_params is not None:
            info.update(ranges=range_detections(rows.numpy(), payload["cloud"], **self.range_params), range_status=0)
        if self.overlay_params is not None:
            canvas, name = payload["canvas"]
            status = draw_detections(canvas, name, rows.numpy(), ranges=info.get("ranges"), **self.overlay_params)
            info.update(overlay=canvas, overlay_status=status)
        return rows, info


def prepare_streams(frames, radar_frames, streams, img_size=416, pack=False, pixel_format=None, resize=None, out=None):
    """Host half of a :class:`MultiStreamFuser` step: checks and stages the raw frame bytes and radar frames (picklable; the
    trackers live on the device, so the radar chain itself belongs to ``infer``).  Needs neither a model nor the HIP library:
    ``pipeline.FusionPipeline`` calls it in the producer process with ``pack=True``, which also does the host loop of
    ``StagedRaggedImages.to`` - every frame's bytes into one buffer + the descriptor - so the consumer only uploads.

    ``pixel_format``: one name of ``utils.datasets.PIXEL_FORMATS`` or one per stream - the frames are the cameras' native ones
    (``"bgr"`` ``[h,w,3]``, ``"yuyv"`` ``[h,w,2]``, ``"nv12"`` ``[h*3//2, w]``), their bytes are staged as they are and converted
    on the device; ``payload["hw"]`` is the picture's size.  ``None``: uint8 ``[h,w,3]`` RGB.

    ``resize``: ``None`` / ``"nearest"`` or ``"area"`` (``StagedRaggedImages``); an unknown name raises here.

    ``img_size=(H, W)``: the frames are staged for the letterbox kernel (``StagedRaggedImages(size=(H, W))``).

    ``out`` (with ``pack=True``): the 1-D uint8 tensor the bytes are packed into (``StagedRaggedImages.pack(out=)``) - a slot of
    the pipeline's ``handover.FrameRing``.

    Any frame may be a ``utils.datasets.FrameSurface`` - a pitched host buffer, a picture a decoder left in device memory - in
    place of a tensor.  A step with at least one surface stages ALL its frames through ``StagedSurfaces`` (tensors are wrapped,
    as views where their strides allow) and one ``me_image_batch_surfaces_u8_f32`` launch; a step of tensors goes the way it
    always went.  ``payload["hw"]`` is the surface's ``(h, w)``; a surface whose format is not the stream's ``pixel_format``,
    a cropped surface (``origin != (0, 0)``: the radar chain projects into the full frame) and ``pack=True`` raise."""
    resize = resize_mode(resize, "prepare_streams")
    img_size = _network_input_size(img_size, "prepare_streams")
    if len(frames) != streams or len(radar_frames) != streams:
        raise hip.MeError(f"MultiStreamFuser: {len(frames)} frames / {len(radar_frames)} radar lists for {streams} streams")
    if any(isinstance(f, FrameSurface) for f in frames):
        if pack or out is not None:
            raise hip.MeError("prepare_streams: pack=True packs dense frames - surfaces are not packed, and a device buffer "
                              "does not cross a process boundary")
        names = [None] * streams if pixel_format is None else pixel_format_names(pixel_format, streams, "stream")
        surfaces = [_fuser_surface(f, name, f"stream {i}") for i, (f, name) in enumerate(zip(frames, names))]
        return dict(hw=[(s.h, s.w) for s in surfaces], img=StagedSurfaces(surfaces, img_size, resize=resize),
                    radar_frames=[list(r) for r in radar_frames])
    frames = [torch.as_tensor(f) for f in frames]
    if pixel_format is not None:
        names = pixel_format_names(pixel_format, streams, "stream")
        hws = [picture_hw(f, name, f"stream {i}") for i, (f, name) in enumerate(zip(frames, names))]
        img = StagedRaggedImages(frames, img_size, formats=names, resize=resize)
    else:
        for i, frame in enumerate(frames):
            if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
                raise hip.MeError(f"stream {i}: frame must be uint8 [h,w,3] (got {frame.dtype} {tuple(frame.shape)})")
        hws = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
        img = StagedRaggedImages(frames, img_size, resize=resize)
    if out is not None and not pack:
        raise hip.MeError("prepare_streams: out= needs pack=True")
    if pack:
        img.pack(keep_frames=False, out=out)
    return dict(hw=hws, img=img, radar_frames=[list(r) for r in radar_frames])


class MultiStreamFuser:
    """:class:`FrameFuser` for ``streams`` camera + radar nodes in one step: ``fuser(frames, radar_frames)`` takes S uint8
    ``[h,w,3]`` frames (sizes may differ per stream) and S lists of radar frames and returns a list of S ``(rows [m,7], info)``
    with the meaning :class:`FrameFuser` gives them.  Stream ``s`` sees what its own ``FrameFuser`` would see; every stream
    keeps its own tracker state on the device (``generator.reset(stream)`` forgets one).

    Per step: one upload + two launches for the radar chain, one ragged-batch launch for the frames, one heat-map launch, one
    launch for the per-frame means (auto mode), ``Network.forward`` once for the frames that select fusion and once for the
    camera-only ones, then the output tail.

    ``tail="device"`` (default): ``hip.stream_tail`` - the network's rows are listed per stream on the device, one segmented
    NMS handles every stream (seven launches in all), the kept rows come back rescaled to each stream's frame in one copy.
    ``tail="host"``: the rows are sorted by stream with torch and copied, one ``me_nms_boxes_f32`` call per stream is queued
    (the same seven launches each) and ``rescale_boxes`` runs per stream on the host rows.  Both give ``torch.equal`` rows;
    on an MI355X the tail alone takes 0.05 - 0.17 ms on the device against 0.15 - 2.5 ms on the host (S = 1 .. 32) and the whole
    step is 10 - 42 % shorter in every row of ``profiles/multistream_latency.txt``.

    ``split="forwards"`` (default): a step whose streams pick different modes reads the S means back, gathers the fusion and the
    camera-only sub-batch and runs ``Network.forward`` on each - the detector runs at batch ``a`` and ``S - a`` for ``a`` dark
    streams, a plan per size.  ``split="frame_modes"``: ``hip.frame_modes`` decides on the device (fixed modes 0 / 1: a constant
    vector; a fixed mode 2 keeps the scalar call) and ONE ``Network.forward(..., frame_modes=)`` takes all S streams at the
    fixed batch S - no read-back in front of the network, no gather, one detector plan whatever the light does; every stream's
    rows are ``torch.equal`` to what the whole batch gives at that stream's mode.  The modes reach ``info["mode"]`` in one small
    copy behind the tail.  Measured against ``"forwards"`` in ``profiles/multistream_frame_modes.txt``.

    The device tail lists every stream in a ``[streams][m]`` workspace (``m`` = the rows of the step, the one bound of a
    stream's rows the host holds without a read-back): it raises :class:`hip.MeError` for more than 32768 rows in a step, where
    the host tail only needs every stream's own rows to stay under that, and its workspace grows as ``streams * m``.

    A joint ``me_nms_boxes_f32`` call with the label ``stream * num_classes + class`` would NOT: that entry point separates
    labels with torchvision's offset trick (``boxes + label * (max + 1)`` in float32), not by equality, so one maximum shared
    by all streams rounds the boxes of the later streams differently from the per-frame call of the demos.  The segmented call
    keeps one maximum per stream - the NMS kernels are batched over lists that each have their own - and so reproduces the
    per-stream calls bit for bit.

    The device generator (``DeviceRadarProposals``) is built on first use of :attr:`generator` - by the first :meth:`infer` or
    :meth:`advance` - not by the constructor: the host half (:meth:`prepare`, :func:`prepare_streams`) and
    ``pipeline.FusionPipeline``'s consumer set-up need no GPU.  Bad calibration or generator arguments and a missing GPU therefore
    raise at that first use; touch ``fuser.generator`` after construction to have them raise early.

    ``pixel_format``: one name or one per stream from ``"rgb"``, ``"bgr"``, ``"nv12"``, ``"yuyv"`` - the frames are taken the way
    the camera or the decoder hands them over (:func:`prepare_streams`) and converted by the input kernel
    (``me_image_batch_formats_u8_f32``): no conversion pass on the host, half (NV12) or two thirds (YUYV) of the bytes packed and
    uploaded, and every stream's rows are ``torch.equal`` to those of its frame converted to RGB.  Default ``None``: RGB.

    ``resize``: ``None`` / ``"nearest"`` - the reference's ``F.interpolate(mode="nearest")``, which keeps one source pixel in
    ``(P / img_size)^2`` (one in 21 of a 1080p frame at 416) - or ``"area"``: ``F.interpolate(padded_square, img_size,
    mode="area")``, every source pixel averaged into its output (``me_image_batch_area_u8_f32``, any ``pixel_format``).  The
    reference's scripts have no such option: ``"area"`` is pinned to torch's float64 ``area`` interpolation rounded to float32,
    not to the reference.  It needs ``max(h, w) <= 255 * img_size`` per frame, gives the nearest path's bits for ``max(h, w) ==
    img_size``, and leaves the geometry alone: box rescaling, the radar boxes and the tail do not change, and the auto mode's
    mean is taken over the area-resized image.  Checked here, when the fuser is built.

    ``img_size=(H, W)`` (sides positive multiples of 32; ``(S, S)`` is ``S``): the rectangular network input.  Every frame is
    letterboxed by one rule (``utils.utils.letterbox_geometry``) in the input launch (``me_image_batch_letterbox_u8_f32``), the
    radar maps are the dataset's resized ``(H / 16, W / 16)`` maps (``me_radar_heatmap_rect_f32``; the raw 32 x 32 map of the
    square path has no rectangular form), the network's radar boxes are rebuilt per axis from the device proposals
    (``DeviceRadarProposals.letterbox_boxes``: two launches and one more small copy per step, for the counts the sub-batch
    gather and ``info["radar_boxes"]`` use) and both tails rescale per axis - the tail kernel is unchanged, only its six
    scalars per stream differ.  ``split="frame_modes"`` and ``resize="area"`` are refused with a rectangular size.

    Any stream's frame may be a ``utils.datasets.FrameSurface`` - a pitched host buffer, a picture a decoder left in device
    memory - in place of a tensor: the step's frames are then read where they lie (``StagedSurfaces``, one
    ``me_image_batch_surfaces_u8_f32`` launch) and every stream's rows are ``torch.equal`` to those of the dense copies
    (:func:`prepare_streams`).  Everything behind the input launch is the same.

    ``tracks``: ``None`` (default) - nothing below happens.  ``True`` or a dict of ``detection_tracks.DetectionTracker``
    parameters (``max_age``, ``min_hits``, ``iou_min``, ``birth_conf``): every stream's detections get track ids from a tracker
    of its own on the device (``detection_tracks.DeviceDetectionTracks``, one launch behind the tail's, reading the tail's
    output buffer where it lies; ``hip.stream_tail_tracks``).  Every stream's ``info`` gains ``"tracks"``, a ``[k,10]`` float64
    numpy array ``(id, x1, y1, x2, y2, conf, cls, hit_streak, age, det)`` - ``det`` is the row of the stream's returned
    detections behind the track - and ``"track_status"`` (0, or a ``hip.TRACKS_E_*`` word: that stream's tracker refused the
    step, kept its state and has no rows).  The detection rows are ``torch.equal`` to those without tracking and the step has no
    more device-to-host copies; its tail takes 0.02 - 0.07 ms longer (S = 1 .. 32, ``profiles/box_tracks_latency.txt``), where
    S host trackers take 0.2 - 7.3 ms.  It needs ``tail="device"``.  :attr:`tracker` is the device tracker
    (``tracker.reset(stream)`` forgets one stream's tracks).  :meth:`advance` does not touch it: a step that ``pipeline.FusionPipeline`` skips has no
    detections, so it does not age the tracks - ``max_age`` counts the steps that were inferred, not the frames that
    arrived.

    ``ranging``: ``None`` (default) - nothing below happens.  ``True`` or a dict of ``detection_range.range_detections``
    parameters (``shrink``, ``gate``, ``min_points``): every detection gets the range and the radial speed of the radar returns
    inside its box, from the kept points the radar chain left on the device (``detection_range.DeviceDetectionRanges``, one
    launch behind the tail's and the tracker's, ``me_box_ranges_f64``; ``hip.stream_tail_ranges``) - in every mode, the radar
    chain runs in camera-only steps too, and with square and rectangular ``img_size``, the tail's rows are frame pixels either
    way.  Every stream's ``info`` gains ``"ranges"``, a ``[k,4]`` float64 numpy array ``(range_m, velocity_mps, points_used,
    points_inside)`` with one row per returned detection - ``(NaN, NaN, 0, n)`` where no group of ``min_points`` returns was
    found - and ``"range_status"`` (0 or a ``hip.RANGES_E_*`` word); with ``tracks=`` as well also ``"track_ranges"``
    ``[t,4]``: ``ranges[det]`` per track row, ``(NaN, NaN, 0, 0)`` where ``det < 0``.  The rows are bit-equal to
    ``range_detections(rows, generator.cloud(s))``; the detection rows, the tracks and the device-to-host copies of a step
    are unchanged.  It needs ``tail="device"``.  Cost: ``profiles/box_ranges_latency.txt``.

    ``overlay``: ``None`` (default) - nothing below happens.  ``True`` or a dict of ``frame_overlay.draw_detections`` style
    parameters (``thickness``, ``font_scale``, ``labels``, ``color_by``, ``classes``, ``palette``): every stream's boxes and
    labels (``#id`` with ``tracks=``, the confidence, the range with ``ranging=``) are painted into its picture on the device
    (``frame_overlay.DeviceFrameOverlay``, one launch behind the tail's, the tracker's and the ranger's, ``me_frame_overlay_u8``;
    ``hip.stream_tail_overlay``), bit-equal to ``draw_detections`` on the frame with that step's ``info``.  A stream whose
    frame is a ``FrameSurface`` on a CUDA buffer is drawn IN PLACE, after the input launch has read it on the same stream; for a
    frame that came from the host, the uploaded bytes the input launch read are kept and drawn into.  Every stream's ``info``
    gains ``"overlay"``, a ``FrameSurface`` in device memory (the stream's own surface for an in-place stream), and
    ``"overlay_status"`` (0 or a ``hip.OVERLAY_E_*`` word: more than 64 drawn rows leave the picture untouched).  The pictures
    of different streams must not share bytes.  The detection rows, the tracks, the ranges and the device-to-host copies of a
    step are unchanged (the status words travel in the tail's copy).  It needs ``tail="device"``.  Cost:
    ``profiles/frame_overlay_latency.txt``."""

    def __init__(self, model, calib_params, streams, model_mode=3, img_size=416, nms_iou=0.3, dark_threshold=0.08,
                 tail="device", split="forwards", pixel_format=None, resize=None, tracks=None, ranging=None, overlay=None,
                 **generator_kwargs):
        self.model, self.model_mode, self.streams = model, model_mode, int(streams)
        self.img_size = _network_input_size(img_size, "MultiStreamFuser")
        self.rect = isinstance(self.img_size, tuple)
        self.nms_iou, self.dark_threshold = nms_iou, dark_threshold
        if tail not in ("device", "host"):
            raise hip.MeError(f"MultiStreamFuser: tail must be 'device' or 'host' (got {tail!r})")
        if split not in ("forwards", "frame_modes"):
            raise hip.MeError(f"MultiStreamFuser: split must be 'forwards' or 'frame_modes' (got {split!r})")
        self.split = split
        if self.rect and split == "frame_modes":
            raise hip.MeError(f"MultiStreamFuser: split='frame_modes' needs a square img_size (Network.forward refuses "
                              f"frame_modes on {self.img_size[0]} x {self.img_size[1]} frames)")
        if self.streams <= 0:
            raise hip.MeError(f"MultiStreamFuser: streams must be positive (got {streams})")
        # None, one name or one per stream (prepare_streams checks the frames against it)
        self.pixel_format = None if pixel_format is None else pixel_format_names(pixel_format, self.streams, "stream")
        self.resize = resize_mode(resize, "MultiStreamFuser")
        if self.rect and self.resize == "area":
            raise hip.MeError(f"MultiStreamFuser: resize='area' has no rectangular form (img_size {self.img_size[0]} x "
                              f"{self.img_size[1]})")
        self.tail = tail
        if tracks is not None and tracks is not False:
            if tail != "device":
                raise hip.MeError("MultiStreamFuser: tracks need tail='device' (the tracker reads the device tail's output buffer)")
            if tracks is not True and not isinstance(tracks, dict):
                raise hip.MeError(f"MultiStreamFuser: tracks must be None, True or a dict of tracker parameters (got {tracks!r})")
            self.track_params = {} if tracks is True else dict(tracks)
        else:
            self.track_params = None
        self.range_params = ranging_params(ranging, "MultiStreamFuser")
        if self.range_params is not None and tail != "device":
            raise hip.MeError("MultiStreamFuser: ranging needs tail='device' (the kernel reads the device tail's output buffer)")
        self.overlay_params = overlay_params(overlay, "MultiStreamFuser")
        if self.overlay_params is not None and tail != "device":
            raise hip.MeError("MultiStreamFuser: overlay needs tail='device' (the kernel reads the device tail's output buffer)")
        self._painter = None
        self._step_surfaces = self._step_overlay = None   # the pictures of the step being inferred / their status words
        self._tracker = self._ranger = None
        self._step_tracks = None       # (rows per stream, status per stream) of the step being inferred
        self._step_ranges = None       # the same for the ranges
        self.calib_params, self.generator_kwargs = calib_params, generator_kwargs
        self._device = getattr(model, "device", None)
        self._generator = None
        self._scalars = (None, None)   # (frame sizes, their rescale scalars on the device)
        self._fixed_modes = {}         # split="frame_modes" with a fixed mode 0 / 1: the constant vector on the device

    @property
    def device(self):
        if self._device is None:
            self._device = hip.default_device()
        return self._device

    @property
    def generator(self):
        if self._generator is None:
            self._generator = DeviceRadarProposals(self.calib_params, self.streams, device=self.device, **self.generator_kwargs)
        return self._generator

    @property
    def tracker(self):
        """The device tracker of ``tracks=`` (built on first use, like :attr:`generator`); ``None`` without tracking."""
        if self._tracker is None and self.track_params is not None:
            from .detection_tracks import DeviceDetectionTracks
            self._tracker = DeviceDetectionTracks(self.streams, device=self.device, **self.track_params)
        return self._tracker

    @property
    def ranger(self):
        """The ``DeviceDetectionRanges`` of ``ranging=`` (built on first use); ``None`` without ranging."""
        if self._ranger is None and self.range_params is not None:
            from .detection_range import DeviceDetectionRanges
            self._ranger = DeviceDetectionRanges(self.streams, device=self.device, **self.range_params)
        return self._ranger

    @property
    def painter(self):
        """The ``DeviceFrameOverlay`` of ``overlay=`` (built on first use); ``None`` without overlay."""
        if self._painter is None and self.overlay_params is not None:
            from .frame_overlay import DeviceFrameOverlay
            self._painter = DeviceFrameOverlay(self.streams, device=self.device, **self.overlay_params)
        return self._painter

    def __call__(self, frames, radar_frames):
        return self.infer(self.prepare(frames, radar_frames))

    def prepare(self, frames, radar_frames, pack=False):
        """Host half (:func:`prepare_streams`): a picklable payload for :meth:`infer` / :meth:`advance`."""
        return prepare_streams(frames, radar_frames, self.streams, self.img_size, pack=pack, pixel_format=self.pixel_format,
                               resize=self.resize)

    def advance(self, payload):
        """The radar chain of one step and nothing else - what :meth:`infer` does first: a step whose detections nobody
        will look at (``FusionPipeline`` skipping to the newest frames) still reaches the trackers."""
        return self.generator.gen(payload["radar_frames"], payload["hw"])

    def _modes(self, img):
        if self.model_mode != 3:
            return [mode_selection(self.model_mode, None)] * self.streams
        means = hip.frame_means(img).cpu()   # one launch, one copy of S floats
        return [0 if float(m) < self.dark_threshold else 1 for m in means]

    def _infer_frame_modes(self, img, radar_map, step, hws):
        """``split="frame_modes"``: the modes are decided on the device (auto) or are a constant vector (fixed 0 / 1), one
        ``Network.forward(..., frame_modes=)`` takes all S streams - no sub-batches, no read-back in front of the network - and
        the modes come to the host in one small copy behind the tail, for ``info["mode"]`` alone."""
        n = self.streams
        if self.model_mode == 3:
            modes_dev = hip.frame_modes(img, self.dark_threshold)[0]
        else:
            modes_dev = self._fixed_modes.get(self.model_mode)
            if modes_dev is None:
                modes_dev = self._fixed_modes[self.model_mode] = torch.full((n,), int(self.model_mode), dtype=torch.int32).to(self.device)
        with torch.no_grad():
            rows = self.model(img, radar_map, step.radar_box, frame_modes=modes_dev)
            per_stream = self._tail(rows, hws)
        return per_stream, modes_dev.cpu().tolist()

    def infer(self, payload):
        """Device half: radar chain, input kernels, mode selection, ``Network.forward`` per mode, second NMS, rescale."""
        dev, n = self.device, self.streams
        hws = payload["hw"]
        img = payload["img"].to(dev)
        if self.overlay_params is not None:   # the pictures in device memory: in place, or the bytes just uploaded
            self._step_surfaces = payload["img"].device_surfaces()
        step = self.generator.gen(payload["radar_frames"], hws)
        counts = step.host_counts
        if self.rect:   # the resized maps and the per-axis boxes; column 4 becomes the rectangular canvas's count
            radar_map = self.generator.heatmaps(_rect_map_size(self.img_size))
            radar_box, box_counts = self.generator.letterbox_boxes(self.img_size)
            counts = counts.copy()
            counts[:, 4] = box_counts
        else:
            radar_map = self.generator.heatmaps(32)   # the raw 32 x 32 maps, like FrameFuser (quirk q15)
            radar_box = step.radar_box
        if self.split == "frame_modes" and self.model_mode in (0, 1, 3):   # (a fixed mode 2 has no per-frame form: scalar call)
            per_stream, modes = self._infer_frame_modes(img, radar_map, step, hws)
            return self._results(per_stream, modes, counts)
        modes = self._modes(img)
        box_start = np.concatenate([[0], np.cumsum(counts[:, 4])])
        outs = []
        with torch.no_grad():
            for mode in sorted(set(modes), key=lambda m: (m is None, m)):
                idx = [s for s in range(n) if modes[s] == mode]
                if len(idx) == n:
                    rows = self.model(img, radar_map, radar_box, mode)
                else:   # gather the sub-batch; the frame index column goes local and comes back as the stream number
                    where = torch.tensor(idx, dtype=torch.int64).to(dev)
                    box_rows = [r for s in idx for r in range(int(box_start[s]), int(box_start[s + 1]))]
                    local = [float(k) for k, s in enumerate(idx) for _ in range(int(counts[s, 4]))]
                    rb = radar_box[torch.tensor(box_rows, dtype=torch.int64).to(dev)]
                    if len(local):
                        rb[:, 0] = torch.tensor(local, dtype=torch.float32).to(dev)
                    rows = self.model(img[where], radar_map[where], rb, mode)
                    rows = torch.cat([where[rows[:, 0].long()].to(rows.dtype)[:, None], rows[:, 1:]], 1)
                outs.append(rows)
            rows = torch.cat(outs, 0) if len(outs) > 1 else outs[0]
            per_stream = self._tail(rows, hws)
        return self._results(per_stream, modes, counts)

    def _results(self, per_stream, modes, counts):
        n = self.streams
        proposals = self.generator._proposals.cpu().numpy()
        result = []
        for s in range(n):
            r = per_stream[s]
            result.append((r, dict(mode=modes[s], proposals=proposals[s, :int(counts[s, 7])].copy(),
                                   radar_boxes=int(counts[s, 4]), points=int(counts[s, 1]))))
            if self._step_tracks is not None:
                result[-1][1].update(tracks=self._step_tracks[0][s], track_status=int(self._step_tracks[1][s]))
            if self._step_ranges is not None:
                ranges = self._step_ranges[0][s]
                result[-1][1].update(ranges=ranges, range_status=int(self._step_ranges[1][s]))
                if self._step_tracks is not None:   # host indexing of what already came back
                    det = self._step_tracks[0][s][:, 9].astype(np.int64)
                    track_ranges = np.tile(np.array([np.nan, np.nan, 0.0, 0.0]), (len(det), 1))
                    track_ranges[det >= 0] = ranges[det[det >= 0]]
                    result[-1][1]["track_ranges"] = track_ranges
            if self._step_overlay is not None:
                result[-1][1].update(overlay=self._step_surfaces[s], overlay_status=int(self._step_overlay[s]))
        self._step_tracks = self._step_ranges = self._step_surfaces = self._step_overlay = None
        return result

    def _tail(self, rows, hws):
        """Network rows ``[m,8]`` (stream in column 0) -> per stream the ``[k,7]`` CPU rows after the second NMS, in pixels of
        the stream's frame."""
        if self.tail == "device":
            key = tuple(hws)
            if self._scalars[0] != key:   # the frame sizes rarely change: their scalars stay on the device
                self._scalars = (key, rescale_scalars(self.img_size, hws).to(rows.device))
            if self.overlay_params is not None:
                gen = self.generator
                ranging = None if self.range_params is None else (self.ranger, gen._cloud_slots, gen._counts)
                got = hip.stream_tail_overlay(rows.to(torch.float32).contiguous(), self.streams, self._scalars[1], self.nms_iou,
                                              self.painter, self._step_surfaces, tracker=self.tracker, ranging=ranging)
                if self.track_params is not None:
                    self._step_tracks = got[2:4]
                if ranging is not None:
                    self._step_ranges = got[-3:-1]
                self._step_overlay = got[-1]
                return got[0]
            if self.range_params is not None:
                gen = self.generator
                got = hip.stream_tail_ranges(rows.to(torch.float32).contiguous(), self.streams, self._scalars[1], self.nms_iou,
                                             self.ranger, gen._cloud_slots, gen._counts, tracker=self.tracker)
                if self.track_params is not None:
                    self._step_tracks = got[2:4]
                self._step_ranges = got[-2:]
                return got[0]
            if self.track_params is not None:
                per_stream, _counts, tracks, status = hip.stream_tail_tracks(
                    rows.to(torch.float32).contiguous(), self.streams, self._scalars[1], self.nms_iou, self.tracker)
                self._step_tracks = (tracks, status)
                return per_stream
            return hip.stream_tail(rows.to(torch.float32).contiguous(), self.streams, self._scalars[1], self.nms_iou)[0]
        per_stream = self._second_nms(rows)
        for s, r in enumerate(per_stream):
            if len(r):
                rescale_boxes(r, self.img_size, hws[s])
        return per_stream

    def _second_nms(self, rows):
        """``box_ops.batched_nms(rows[:, :4], rows[:, 4], rows[:, 6], nms_iou)`` of every stream's rows (stream = column 0 of
        ``rows`` [m,8]): the rows are grouped by stream on the device (stable: each stream keeps the network's order), copied
        once, the S calls are queued back to back on the grouped rows and their kept indices come back in one copy."""
        n, dev = self.streams, rows.device
        empty = torch.zeros((0, 7))
        if rows.shape[0] == 0:
            return [empty.clone() for _ in range(n)]
        order = torch.sort(rows[:, 0], stable=True).indices
        grouped = rows[order].to(torch.float32)
        boxes, scores, labels = grouped[:, 1:5].contiguous(), grouped[:, 5].contiguous(), grouped[:, 7].contiguous()
        host = grouped.cpu()
        per = torch.bincount(host[:, 0].long(), minlength=n).tolist()
        kept = hip.nms_indices_grouped(boxes, scores, labels, per, self.nms_iou)
        return [host[k][:, 1:].clone() if per[s] else empty.clone() for s, k in enumerate(kept)]
