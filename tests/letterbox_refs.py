"""Plain torch CPU references of the rectangular input path (include/millieye_hip.h, "letterbox to a rectangular canvas"):
tests/test_letterbox_cpu.py guards them and the host code, tests/test_gpu_letterbox.py compares the kernels and the fusers with
them.  The reference's YOLOLayer has one grid_size, so its scripts have no rectangular input: the pins are stock torch ops.

* geometry, restated from the definition (the smallest rectangle of the canvas's aspect ratio that holds the picture);
* frames: ``F.pad`` + ``F.interpolate(mode="nearest")`` of ``u8 / 255`` (formats through tests/pixel_format_refs.py first);
* heat maps: the oracle's bins, padded, + ``F.interpolate(mode="bilinear", align_corners=True)``;
* the per-axis radar box arithmetic in float32;
* the per-axis box rescale and the host composition of one fuser step."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import pixel_format_refs as pf

# picture (h, w) -> canvas (H, W) of the kernel tests; the last one is the issue's 1080p case
SHAPES = (((7, 5), (32, 64)), ((5, 7), (64, 32)), ((1, 1), (32, 96)), ((33, 97), (32, 96)), ((97, 33), (96, 30)),
          ((64, 96), (64, 96)), ((10, 300), (32, 32)), ((1080, 1920), (256, 416)))


def geometry(picture_hw, canvas_hw):
    """``(Ph, Pw, top, bottom, left, right)``: the padded rectangle and the four pads."""
    (h, w), (H, W) = picture_hw, canvas_hw
    g = math.gcd(H, W)
    a, b = H // g, W // g
    k = 1
    while a * k < h or b * k < w:   # the definition: the first multiple of (a, b) that holds the picture
        k += 1
    Ph, Pw = a * k, b * k
    top, left = (Ph - h) // 2, (Pw - w) // 2
    return Ph, Pw, top, Ph - h - top, left, Pw - w - left


def geometry_fast(picture_hw, canvas_hw):
    """:func:`geometry` without the loop (for 1080p and the random sweeps); the CPU test pins one to the other."""
    (h, w), (H, W) = picture_hw, canvas_hw
    g = math.gcd(H, W)
    a, b = H // g, W // g
    k = max((h + a - 1) // a, (w + b - 1) // b)
    Ph, Pw = a * k, b * k
    top, left = (Ph - h) // 2, (Pw - w) // 2
    return Ph, Pw, top, Ph - h - top, left, Pw - w - left


def letterbox_nearest(frame, canvas_hw, fmt="rgb", flip=False):
    """uint8 frame in ``fmt`` -> float32 ``[3,H,W]``: ToTensor, zero pad, optional mirror of the padded rectangle, one nearest
    ``F.interpolate`` to the canvas."""
    rgb = torch.from_numpy(pf.to_rgb_u8(np.asarray(frame), fmt))
    img = rgb.permute(2, 0, 1).float().div(255)
    _Ph, _Pw, top, bottom, left, right = geometry_fast(tuple(img.shape[1:]), canvas_hw)
    img = F.pad(img, (left, right, top, bottom), "constant", value=0)
    if flip:
        img = torch.flip(img, [-1])
    return F.interpolate(img.unsqueeze(0), size=tuple(canvas_hw), mode="nearest").squeeze(0)


def kernel_index_rule(picture_hw, canvas_hw, flip=False):
    """The kernel's index rule restated in numpy float32: per output row / column the picture row / column it reads, -1 for
    padding.  ``py = (Ph == H) ? y : min((int)floorf((float)y * ((float)Ph / (float)H)), Ph - 1)``, likewise x; the mirror is
    ``px = Pw - 1 - px``; then ``- top`` / ``- left``."""
    (h, w), (H, W) = picture_hw, canvas_hw
    Ph, Pw, top, _b, left, _r = geometry_fast(picture_hw, canvas_hw)

    def axis(n_out, P):
        i = np.arange(n_out)
        if P == n_out:
            return i
        scale = np.float32(P) / np.float32(n_out)
        return np.minimum(np.floor(i.astype(np.float32) * scale).astype(np.int64), P - 1)

    py, px = axis(H, Ph), axis(W, Pw)
    if flip:
        px = Pw - 1 - px
    sy, sx = py - top, px - left
    return np.where((sy >= 0) & (sy < h), sy, -1), np.where((sx >= 0) & (sx < w), sx, -1)


def gather_by_rule(rgb_u8, canvas_hw, flip=False):
    """``[3,H,W]`` float32 from :func:`kernel_index_rule`: ``(float)c / 255.f`` of the picked pixel, 0 for padding."""
    rgb_u8 = np.asarray(rgb_u8)
    sy, sx = kernel_index_rule(rgb_u8.shape[:2], canvas_hw, flip)
    vals = rgb_u8[np.maximum(sy, 0)][:, np.maximum(sx, 0)].astype(np.float32) / np.float32(255)
    vals[(sy < 0)[:, None] | (sx < 0)[None, :]] = 0
    return torch.from_numpy(np.ascontiguousarray(vals.transpose(2, 0, 1)))


def heatmap_rect(points, image_wh, map_hw, radar_maps_size=32):
    """``[3,mh,mw]`` float32 radar map of one frame: the oracle's ``plot_radar_heatmap`` bins of the original image, padded by
    the geometry rule for the aspect ratio of ``map_hw``, + bilinear ``align_corners=True``."""
    from oracle import datasets_ref
    m = datasets_ref.to_tensor(datasets_ref.plot_radar_heatmap(np.asarray(points, dtype=np.float64).reshape(-1, 4).transpose(),
                                                               tuple(image_wh), radar_maps_size)).float()
    _Ph, _Pw, top, bottom, left, right = geometry(tuple(m.shape[1:]), map_hw)
    m = F.pad(m, (left, right, top, bottom), "constant", value=0)
    return F.interpolate(m.unsqueeze(0), size=tuple(map_hw), mode="bilinear", align_corners=True).squeeze(0)


def radar_boxes(proposals, frame_hw, canvas_hw, stream=0):
    """Pixel proposals ``[k,4]`` float64 -> the kept ``[k',5]`` float32 rows ``(stream, x1, y1, x2, y2)``: each value rounded to
    float32, + its side's pad, / the padded width (x) or height (y), clamp to [0, 1] (NaN stays), empty boxes dropped."""
    h, w = frame_hw
    Ph, Pw, top, bottom, left, right = geometry_fast(frame_hw, canvas_hw)
    b = torch.from_numpy(np.asarray(proposals, dtype=np.float64).reshape(-1, 4)).to(torch.float32)
    b = b + torch.tensor([left, top, right, bottom], dtype=torch.float32)
    b = torch.clamp(b / torch.tensor([Pw, Ph, Pw, Ph], dtype=torch.float32), 0, 1)
    b = b[(b[:, 0] < b[:, 2]) & (b[:, 1] < b[:, 3])]
    return torch.cat([torch.full((len(b), 1), float(stream)), b], 1)


def rescale_terms(canvas_hw, frame_hw):
    """``(pad // 2, canvas - pad, original)`` for x, then for y, as python floats: ``pad_x = (Pw - w) * (W / Pw)``,
    ``pad_y = (Ph - h) * (H / Ph)``."""
    (H, W), (h, w) = canvas_hw, frame_hw
    Ph, Pw = geometry_fast(frame_hw, canvas_hw)[:2]
    pad_x, pad_y = (Pw - w) * (W / Pw), (Ph - h) * (H / Ph)
    return [pad_x // 2, W - pad_x, w, pad_y // 2, H - pad_y, h]


def rescale(boxes, canvas_hw, frame_hw):
    """``((v - pad // 2) / unpadded) * original`` per axis on a float32 ``[k,4]`` tensor (a copy)."""
    c = rescale_terms(canvas_hw, frame_hw)
    out = boxes.clone()
    for col, k in ((0, 0), (1, 3), (2, 0), (3, 3)):
        out[:, col] = ((boxes[:, col] - c[k]) / c[k + 1]) * c[k + 2]
    return out


def fuser_step(net_cpu, frame, cloud, proposals, canvas_hw, conf, nms_iou=0.3, dark_threshold=0.08, fmt="rgb"):
    """One ``FrameFuser(img_size=canvas_hw, model_mode=3)`` step composed on the host from the references above and
    tests/rect_refs.py's network: ``(rows [m,7] in frame pixels, mode, radar boxes)``."""
    from oracle import tv_ops_np
    from tests import rect_refs
    H, W = canvas_hw
    h, w = pf.picture_hw(frame, fmt)
    img = letterbox_nearest(frame, canvas_hw, fmt).unsqueeze(0)
    radar_map = heatmap_rect(cloud, (w, h), (H // 16, W // 16)).unsqueeze(0)
    rbox = radar_boxes(proposals, (h, w), canvas_hw)
    mode = 0 if float(img.mean()) < dark_threshold else 1
    rows = rect_refs.network_forward_rect(net_cpu, img, radar_map, rbox, mode, conf_thresh=conf)[0][:, 1:].float()
    if len(rows):
        keep = np.asarray(tv_ops_np.batched_nms(rows[:, :4].numpy(), rows[:, 4].numpy(), rows[:, 6].numpy(), nms_iou), np.int64)
        rows = rows[torch.from_numpy(keep)]
        rows[:, :4] = rescale(rows[:, :4], canvas_hw, (h, w))
    return rows, mode, len(rbox)
