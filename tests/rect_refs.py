"""Float64 restatements for rectangular inputs [n,3,H,W] (test infrastructure; tests/test_rect_refs_cpu.py pins both to the oracle
at square shapes).

The oracle's ``darknet_forward`` decodes with one ``grid_size`` like the reference and cannot serve here.  ``darknet_forward_rect``
walks the ``Darknet`` object's own torch modules by ``module_defs`` - conv / BN / leaky, maxpool with the 2 x 2 / stride-1 zero
extension, upsample, route, shortcut - in float64 and puts Darknet's rectangular decode on top:

    stride = H / gh = W / gw          row r = row_offset + a * gh * gw + gy * gw + gx
    x = (sigmoid(tx) + gx) * stride   y = (sigmoid(ty) + gy) * stride   w, h = exp(t) * (anchor / stride) * stride

``network_forward_rect`` is ``oracle.network_ref.network_forward`` with that detector in front and the radar boxes scaled per
axis, composed from the oracle's own pieces."""
import copy
import functools

import torch
import torch.nn.functional as F

from millieye_amd import synth
from oracle import network_ref, tv_ops
from tests import parity_helpers as ph


def frames(tag, n, h, w):
    return torch.from_numpy(synth.uniform(tag, (n, 3, h, w), 0.0, 1.0))


@functools.lru_cache(maxsize=None)
def detector_case(name, n, h, w):
    """``(CPU model, frames, featuremap, rows, fractions)`` of one seeded detector case, computed once per session.  The model
    and the tensors are shared: copy the model before moving it, and leave the tensors as they are."""
    from millieye_amd.engine import pick_tap_module
    model = ph.make_darknet(name)
    x = frames(f"rect/{name}/{n}/{h}x{w}", n, h, w)
    fm, rows, frac = darknet_forward_rect(model, x, pick_tap_module(model.module_defs), return_frac=True)
    return model, x, fm, rows, frac


def edge_rows(frac):
    """Rows whose sigmoid(tx) or sigmoid(ty) is so close to 0 or 1 that float32 may round the cell offset onto a cell border
    (2^-20: sixteen float32 steps at 1, and below half a step of the largest cell index + 1 used in the tests)."""
    eps = 2.0 ** -20
    return ((frac < eps) | (frac > 1 - eps)).any(-1)


def yolo_decode_rect(x, anchors, num_classes, img_hw):
    """x NCHW [n, A*(5+C), gh, gw] -> [n, A*gh*gw, 5+C]; also returns the fraction bits (sigmoid of tx, ty) per row."""
    n, _, gh, gw = x.shape
    na = len(anchors)
    stride = img_hw[0] / gh
    assert stride == img_hw[1] / gw, (img_hw, gh, gw)
    pred = x.view(n, na, num_classes + 5, gh, gw).permute(0, 1, 3, 4, 2)
    gx = torch.arange(gw, dtype=x.dtype).view(1, 1, 1, gw)
    gy = torch.arange(gh, dtype=x.dtype).view(1, 1, gh, 1)
    # anchors / stride is rounded to float32 like the device's table (the reference's scaled_anchors tensor)
    scaled = torch.tensor([(aw / stride, ah / stride) for aw, ah in anchors], dtype=torch.float32).to(x.dtype)
    sx, sy = torch.sigmoid(pred[..., 0]), torch.sigmoid(pred[..., 1])
    out = torch.empty(pred.shape, dtype=x.dtype)
    out[..., 0] = (sx + gx) * stride
    out[..., 1] = (sy + gy) * stride
    out[..., 2] = torch.exp(pred[..., 2]) * scaled[:, 0].view(1, na, 1, 1) * stride
    out[..., 3] = torch.exp(pred[..., 3]) * scaled[:, 1].view(1, na, 1, 1) * stride
    out[..., 4:] = torch.sigmoid(pred[..., 4:])
    frac = torch.stack((sx, sy), -1)
    return out.reshape(n, na * gh * gw, num_classes + 5), frac.reshape(n, na * gh * gw, 2)


def darknet_forward_rect(model, x, tap_module, return_frac=False):
    """``(featuremap, yolo_outputs)`` in float64 from a CPU ``Darknet`` object (its parameters, its ``module_defs``)."""
    m = copy.deepcopy(model).cpu().double().eval()
    img_hw = (x.shape[2], x.shape[3])
    x = x.double()
    outs, rows, fracs, feat = [], [], [], None
    with torch.no_grad():
        for i, (d, mod) in enumerate(zip(m.module_defs, m.module_list)):
            kind = d["type"]
            if kind in ("convolutional", "maxpool"):
                for child in mod:           # Conv2d, BatchNorm2d, LeakyReLU / ZeroPad2d, MaxPool2d: stock torch modules
                    x = child(x)
                if i == tap_module:
                    feat = x
            elif kind == "upsample":        # (the product's Upsample module launches a kernel: restated here)
                x = F.interpolate(x, scale_factor=int(d["stride"]), mode="nearest")
            elif kind == "route":
                x = torch.cat([outs[int(l)] for l in d["layers"].split(",")], 1)
            elif kind == "shortcut":
                x = outs[-1] + outs[int(d["from"])]
            elif kind == "yolo":
                x, fr = yolo_decode_rect(x, mod[0].anchors, mod[0].num_classes, img_hw)
                rows.append(x)
                fracs.append(fr)
            else:
                raise ValueError(kind)
            outs.append(x)
    res = (feat, torch.cat(rows, 1))
    return res + (torch.cat(fracs, 1),) if return_frac else res


def row_cells(model, h, w):
    """``(stride, gx, gy)`` per row of ``yolo_outputs`` for an ``h x w`` input, from the row order alone."""
    strides, gxs, gys = [], [], []
    factor = _yolo_strides(model.module_defs)
    for layer, s in zip(model.yolo_layers, factor):
        gh, gw = h // s, w // s
        for _a in range(layer.num_anchors):
            gy, gx = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
            gxs.append(gx.reshape(-1))
            gys.append(gy.reshape(-1))
            strides.append(torch.full((gh * gw,), s))
    return torch.cat(strides), torch.cat(gxs), torch.cat(gys)


def _yolo_strides(defs):
    """Downsampling factor in front of every [yolo] block, in cfg order."""
    factor, found = [], []
    for i, d in enumerate(defs):
        kind = d["type"]
        f = factor[i - 1] if i else 1
        if kind in ("convolutional", "maxpool"):
            f = f * int(d["stride"])
        elif kind == "upsample":
            f = f // int(d["stride"])
        elif kind == "route":
            first = int(d["layers"].split(",")[0])
            f = factor[i + first if first < 0 else first]
        elif kind == "yolo":
            found.append(f)
        factor.append(f)
    return found


def network_forward_rect(net, images, maps, radar_boxes, model_mode=0, conf_thresh=0.2, thr_img=0.0, thr_radar=0.0,
                         class_idx=0, class_num=1, tap_module=8):
    """``network_ref.network_forward`` for ``images`` [n,3,H,W]: the detector above (rounded to float32 where the oracle's
    detector hands over float32), ``radar_boxes[:, 1:]`` scaled by ``(W, H, W, H)``; everything else is the oracle's code.
    ``net``: a CPU ``Network``.  Returns ``(output, scaled radar boxes)``."""
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    H, W = images.shape[2], images.shape[3]
    with torch.no_grad():
        feature_map, output_tensor = darknet_forward_rect(net.base_detector, images, tap_module)
        feature_map, output_tensor = feature_map.float(), output_tensor.float()
        detections = network_ref.nms_cpp(output_tensor, conf_thresh)
        img_boxes = []
        for image_i, det in enumerate(detections):
            if det is not None:
                det = det[det[:, 6] == class_idx]
                if len(det) > 0:
                    b = torch.zeros((len(det), 8 + class_num))
                    b[:, 0] = image_i
                    b[:, 1:] = det[:, :7 + class_num]
                    img_boxes.append(b)
        img_boxes = torch.cat(img_boxes, 0) if img_boxes else torch.empty((0, 8 + class_num))
        num_img = len(img_boxes)
        radar_boxes = radar_boxes.clone()
        if len(radar_boxes) > 0:
            radar_boxes[:, 1:] *= torch.tensor([W, H, W, H], dtype=radar_boxes.dtype)
        if model_mode == 1:
            return img_boxes[:, :8], radar_boxes
        if model_mode == 2:
            thr_img = 1
        roi_score_map = network_ref.img_cnn(sd, feature_map)
        radar_score_map = network_ref.radar_cnn(sd, maps)
        box_locations = torch.cat((img_boxes[:, :5], radar_boxes), 0)
        crop_img = tv_ops.ps_roi_align(roi_score_map, box_locations, (7, 7), spatial_scale=1. / 16)
        crop_radar = tv_ops.roi_align(radar_score_map, box_locations, (7, 7), spatial_scale=1. / 16)
        regress_param, refinement_vector = network_ref.refinement(sd, crop_radar, crop_img)
        radar_rows = torch.cat((radar_boxes, refinement_vector[num_img:], torch.zeros((len(radar_boxes), 1)),
                                refinement_vector[num_img:, 1:]), -1)
        boxes = torch.cat((img_boxes, radar_rows), 0)
        yolo_vector = torch.cat((img_boxes[:, 5:6], img_boxes[:, 8:]), 1)
        masks_img = network_ref.ensemble(sd, refinement_vector[:num_img], yolo_vector)
        masks = torch.cat((masks_img[:, :1], refinement_vector[num_img:, :1]), 0)
        masks = torch.cat((1 - masks, masks), -1)
        positive = torch.cat((masks[:num_img, 1] > thr_img, masks[num_img:, 1] > thr_radar), 0)
        if model_mode != 2:
            located = network_ref.box_regress(regress_param[positive], boxes[positive, 1:5])
        else:
            located = boxes[positive, 1:5]
        output = torch.cat((boxes[positive, :1], located, masks[positive, 1:], boxes[positive, 6:8]), -1)
        masks_tmp = masks.clone()
        masks_tmp[num_img:, 1] /= 5
        order = torch.sort(masks_tmp[positive, 1], descending=True, stable=True).indices
        return output[order], radar_boxes
