"""Plain references of the RoI-head and stage-2 kernels (csrc/heads.hip, csrc/m2_train.hip): one small function per operation,
numpy / torch only, no project kernel, in the kernels' layouts (matrices [rows, channels], maps NHWC, weights as the state dict
holds them: ``w0`` [256,490], ``w1`` [4,256], ``w2`` [c,256], ``rw`` [10,490], ``e1w`` [32,2], ``e2w`` [2,32*slots]).
``tests/test_heads_refs_cpu.py`` pins every function to the oracle's restatement of the reference (oracle/network_ref.py,
oracle/network_m2_ref.py) and to torch float64 autograd through it; ``tests/test_gpu_heads_blocks.py`` compares the kernels with them.

Every function computes in ``dtype`` - float64 is the reference; float32 is the same restatement in stock torch single precision on
the CPU, the yardstick of the kernels' error bar (as ``train_block_refs.yolo_loss_grad(dtype=)``).

The LeakyReLU slope is the float32 value of 0.1 and a pre-activation of exactly 0 takes the slope, as in train_block_refs."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.train_block_refs import SLOPE

U = 2.0 ** -24
P, PP, C_OUT, FEAT, HID = 7, 49, 10, 490, 256


def _t(a, dtype=torch.float64):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype)


def _w(W, dtype):
    return {k: _t(v, dtype) for k, v in W.items()}


def leaky(v):
    return torch.where(v > 0, v, SLOPE * v)


def near_zero(value, abs_terms):
    """The rounding distance of a sign / threshold decision: |value| < 8 * 2^-24 * sum |terms|."""
    return np.abs(np.asarray(value, np.float64)) < 8 * U * np.asarray(abs_terms, np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# proposal assembly
# ---------------------------------------------------------------------------------------------------------------------
def gather_class_boxes(det, count, class_idx, class_num):
    """det [n, max_det, 7 + num_classes] (x1,y1,x2,y2, obj, cls_conf, cls_pred, scores), count [n] -> rows [total, 8 + class_num]
    = (image_i, det[:7 + class_num]) of the first min(count, max_det) detections of every image whose cls_pred == class_idx
    (class_idx < 0: all of them), image-major, detection order kept; the same dtype as det (values are copied, not computed)."""
    det, count = np.asarray(det), np.asarray(count)
    n, max_det = det.shape[:2]
    slot = np.arange(max_det)[None, :] < np.minimum(count, max_det)[:, None]
    if class_idx >= 0:
        slot &= det[:, :, 6] == np.float32(class_idx)
    img, k = np.nonzero(slot)          # row-major: image-major, then detection order
    rows = np.empty((len(img), 8 + class_num), det.dtype)
    rows[:, 0] = img
    rows[:, 1:] = det[img, k, :7 + class_num]
    return rows, len(img)


# ---------------------------------------------------------------------------------------------------------------------
# RoI pooling (torchvision 0.6 semantics, float64): for the EXACT inputs, where the pooled values do not depend on the precision
# ---------------------------------------------------------------------------------------------------------------------
def _bilinear(img, y, x):
    h, w = img.shape[:2]
    if y < -1.0 or y > h or x < -1.0 or x > w:
        return 0.0
    y, x = max(y, 0.0), max(x, 0.0)
    yl, xl = int(y), int(x)
    if yl >= h - 1:
        yh = yl = h - 1
        y = float(yl)
    else:
        yh = yl + 1
    if xl >= w - 1:
        xh = xl = w - 1
        x = float(xl)
    else:
        xh = xl + 1
    ly, lx = y - yl, x - xl
    hy, hx = 1.0 - ly, 1.0 - lx
    return hy * hx * img[yl, xl] + hy * lx * img[yl, xh] + ly * hx * img[yh, xl] + ly * lx * img[yh, xh]


def _pool(map_nhwc, rois, scale, ps):
    m = np.asarray(map_nhwc, np.float64)
    rois = np.asarray(rois, np.float64)
    out = np.zeros((len(rois), C_OUT, P, P))
    off = 0.5 if ps else 0.0
    for r, roi in enumerate(rois):
        img = m[int(roi[0])]
        sw, sh, ew, eh = (roi[1:5] * scale - off).tolist()
        rw_, rh_ = ew - sw, eh - sh
        if not ps:
            rw_, rh_ = max(rw_, 1.0), max(rh_, 1.0)
        bh, bw = rh_ / P, rw_ / P
        gh, gw = int(np.ceil(rh_ / P)), int(np.ceil(rw_ / P))
        cnt = gh * gw if ps else max(gh * gw, 1)
        for ph in range(P):
            for pw in range(P):
                ch = np.arange(C_OUT) * PP + ph * P + pw if ps else np.arange(C_OUT)
                acc = np.zeros(C_OUT)
                for iy in range(gh):
                    y = sh + ph * bh + (iy + 0.5) * bh / gh
                    for ix in range(gw):
                        x = sw + pw * bw + (ix + 0.5) * bw / gw
                        acc = acc + _bilinear(img[:, :, ch], y, x)
                with np.errstate(invalid="ignore", divide="ignore"):   # (a zero-area PS-RoI: 0 / 0, as torchvision)
                    out[r, :, ph, pw] = acc / cnt
    return out.reshape(len(rois), FEAT)


def ps_roi_align(map_nhwc, rois, scale):
    """map [n,h,w,490] in the reference's channel order (c*7+ph)*7+pw -> [k,490], feature f = c*49 + ph*7 + pw."""
    return _pool(map_nhwc, rois, scale, True)


def roi_align(map_nhwc, rois, scale):
    """roi_align(aligned=False, sampling_ratio=-1): map [n,h,w,10] -> [k,490], feature f = c*49 + ph*7 + pw."""
    return _pool(map_nhwc, rois, scale, False)


# ---------------------------------------------------------------------------------------------------------------------
# stage 3
# ---------------------------------------------------------------------------------------------------------------------
def frontend(feat_img, feat_rad, W, rb=None, dtype=torch.float64):
    """net0 (490 -> 256, LeakyReLU), net1, net2 rows 0 and 1, the radar 7x7 conv (10 x 490) from the pooled features [k,490] each.
    ``hidden`` [k,256] is what save_hidden holds (after the LeakyReLU), ``small`` [k,16] = (reg0..3, z2_0, z2_1, rconv0..9) what
    save_small holds: biases added (``rb``: radar_net.0.bias; None = the inference kernels' small, which leave it to rshift),
    pre-activation.  ``hidden_pre`` is net0's pre-activation."""
    w = _w(W, dtype)
    fi, fr = _t(feat_img, dtype), _t(feat_rad, dtype)
    pre = fi @ w["w0"].T + w["b0"]
    hidden = leaky(pre)
    small = torch.cat((hidden @ w["w1"].T + w["b1"], hidden @ w["w2"][:2].T + w["b2"][:2], fr @ w["rw"].T), 1)
    if rb is not None:
        small = small + torch.cat((torch.zeros(6, dtype=dtype), _t(rb, dtype)))
    return dict(hidden=hidden, hidden_pre=pre, small=small)


def box_regress(reg, xyxy):
    x1, y1, x2, y2 = xyxy.unbind(1)
    cx, cy, bw, bh = (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1
    nx, ny = reg[:, 0] * bw + cx, reg[:, 1] * bh + cy
    nw, nh = torch.exp(reg[:, 2]) * bw, torch.exp(reg[:, 3]) * bh
    return torch.stack((nx - nw / 2, ny - nh / 2, nx + nw / 2, ny + nh / 2), 1)


def _radar_net(small, w):
    rpre = small[:, 6:16] * w["rscale"] + w["rshift"]
    rl = leaky(rpre)
    rlogit = rl @ w["rw2"].reshape(10) + w["rb2"].reshape(())
    return rpre, rl, rlogit


def _fc1(refine2, boxes, w):
    """x [n,2,2] = ((conf, yolo0), (cls1, yolo1)) with yolo = columns 5 and 8 of the proposal rows -> fc1 pre-activation [n,2,32]."""
    x = torch.stack((refine2, torch.stack((boxes[:, 5], boxes[:, 8]), 1)), -1)
    return x, x @ w["e1w"].T + w["e1b"]


def tail(small, rois, img_boxes, n_img, W, thr_img, thr_radar, regress, dtype=torch.float64):
    """tail_one for every RoI: rois [k,5] (the first n_img are image proposals: rows of img_boxes [>= n_img, cols]).
    conf = sigmoid(sigmoid(radar logit) + sigmoid(z2_0)) (quirk q2); image rows: p = softmax(ensemble)[:, 0], c6 / c7 from the
    proposal; radar rows: p = conf, c6 = cls1, c7 = 0; keep = p > thr_img / thr_radar; sort_key = p or p / 5; out_rows [k,8]."""
    w = _w(W, dtype)
    sm, roi = _t(small, dtype), _t(rois, dtype)
    k = sm.shape[0]
    bx = _t(img_boxes, dtype)[:n_img]
    cls = torch.sigmoid(sm[:, 4:6])
    rpre, _rl, rlogit = _radar_net(sm, w)
    conf = torch.sigmoid(torch.sigmoid(rlogit) + cls[:, 0])
    refine = torch.stack((conf, cls[:, 1]), 1)
    _x, pre = _fc1(refine[:n_img], bx, w)
    o = leaky(pre).reshape(n_img, 64) @ w["e2w"].T + w["e2b"]
    is_img = torch.arange(k) < n_img
    p = torch.cat((torch.softmax(o, 1)[:, 0], conf[n_img:]))
    thr = torch.where(is_img, torch.tensor(thr_img, dtype=dtype), torch.tensor(thr_radar, dtype=dtype))
    c6 = torch.cat((bx[:, 6], cls[n_img:, 1]))
    c7 = torch.cat((bx[:, 7], torch.zeros(k - n_img, dtype=dtype)))
    xyxy = box_regress(sm[:, :4], roi[:, 1:5]) if regress else roi[:, 1:5]
    out_rows = torch.cat((roi[:, :1], xyxy, p[:, None], c6[:, None], c7[:, None]), 1)
    return dict(regress=sm[:, :4], refine=refine, mask1=p, keep=(p > thr), sort_key=torch.where(is_img, p, p / 5), out_rows=out_rows,
                o=o, keep_margin=p - thr, keep_terms=p.abs() + thr.abs())


def heads_loss(mask1, conf, label_pos, in_focal, in_conf, alpha, lam, dtype=torch.float64):
    """terms [k,2] = (focal(alpha, gamma 2) on [1-p, p] against the one-hot label, BCE(conf, label) / lam, logs clamped at -100)
    for the rows with in_focal / in_conf, and the seeds dL/dp, dL/dconf (denominator clamped at 1e-12, as torch's BCE backward)."""
    p, x = _t(mask1, dtype), _t(conf, dtype)
    pos, foc, cnf = (torch.as_tensor(np.asarray(v)).bool() for v in (label_pos, in_focal, in_conf))
    pt = torch.where(pos, p, 1 - p)
    a = torch.where(pos, torch.tensor(alpha, dtype=dtype), torch.tensor(1 - alpha, dtype=dtype))
    lg = torch.log(pt)
    zero = torch.zeros((), dtype=dtype)
    focal = torch.where(foc, -a * (1 - pt) ** 2 * lg, zero)
    dpt = a * (2 * (1 - pt) * lg - (1 - pt) ** 2 / pt)
    seed_p = torch.where(foc, torch.where(pos, dpt, -dpt), zero)
    y = pos.to(dtype)
    bce = -(y * torch.log(x).clamp(min=-100) + (1 - y) * torch.log(1 - x).clamp(min=-100)) / lam
    seed_c = (x - y) / ((1 - x) * x).clamp(min=1e-12) / lam
    return dict(terms=torch.stack((focal, torch.where(cnf, bce, zero)), 1), seed_p=seed_p, seed_conf=torch.where(cnf, seed_c, zero))


def tail_bwd(small, refine, mask1, seed_p, seed_conf, img_boxes, n_img, W, dtype=torch.float64):
    """Backward of the tail from the seeds dL/dp (image rows only: the objective's focal term is taken over image proposals, so
    seed_p of a radar row is not read) and dL/dconf: the eight outputs of me_heads_tail_bwd_f32, plus the fc1 pre-activations
    ``pre`` [n_img,64] with the sum of their |terms| (``pre_terms``) for the sign decisions of the LeakyReLU derivative."""
    w = _w(W, dtype)
    sm, rf, p = _t(small, dtype), _t(refine, dtype), _t(mask1, dtype)
    sp, sc = _t(seed_p, dtype), _t(seed_conf, dtype)
    k = sm.shape[0]
    bx = _t(img_boxes, dtype)[:n_img]
    conf, cls1 = rf[:, 0], rf[:, 1]
    cls0 = torch.sigmoid(sm[:, 4])
    _rpre, rl, rlogit = _radar_net(sm, w)
    rconf = torch.sigmoid(rlogit)
    x, pre = _fc1(rf[:n_img], bx, w)
    go0 = sp[:n_img] * p[:n_img] * (1 - p[:n_img])
    g_o = torch.zeros((k, 2), dtype=dtype)
    g_o[:n_img] = torch.stack((go0, -go0), 1)
    dh = (g_o[:n_img] @ w["e2w"]).reshape(n_img, 2, 32)
    dpre = dh * torch.where(pre > 0, torch.ones((), dtype=dtype), torch.tensor(SLOPE, dtype=dtype))
    d_r = (dpre * w["e1w"][:, 0]).sum(-1)
    pad = lambda t, cols: torch.cat((t.reshape(n_img, cols), torch.zeros((k - n_img, cols), dtype=dtype)))  # noqa: E731
    d_conf = sc + pad(d_r[:, 0], 1)[:, 0]
    d_cls1 = pad(d_r[:, 1], 1)[:, 0]
    d_s = d_conf * conf * (1 - conf)
    g_rlogit = d_s * rconf * (1 - rconf)
    e1 = w["e1w"].abs()
    pre_terms = x[..., :1].abs() * e1[:, 0] + x[..., 1:].abs() * e1[:, 1] + w["e1b"].abs()
    return dict(g_o=g_o, g_hpre=pad(dpre, 64), h_act=pad(leaky(pre), 64), xin=pad(x, 4),
                g_z2=torch.stack((d_s * cls0 * (1 - cls0), d_cls1 * cls1 * (1 - cls1)), 1),
                g_rl=g_rlogit[:, None] * w["rw2"].reshape(1, 10), rl=rl, g_rlogit=g_rlogit,
                pre=pre.reshape(n_img, 64), pre_terms=pre_terms.reshape(n_img, 64))


# ---------------------------------------------------------------------------------------------------------------------
# stage 2
# ---------------------------------------------------------------------------------------------------------------------
def m2_pairs(refine, boxes):
    """x2 [k * c1, 2] = (refinement_vector, yolo_vector) pairs, yolo_vector = columns 5, 8 .. 8 + c1 - 2 of the proposal rows;
    the dtype of refine (values are copied)."""
    refine, boxes = np.asarray(refine), np.asarray(boxes)
    c1 = refine.shape[1]
    yolo = np.concatenate((boxes[:, 5:6], boxes[:, 8:8 + c1 - 1]), 1)
    return np.stack((refine, yolo.astype(refine.dtype)), -1).reshape(-1, 2)


def m2_rows(o, regress, boxes, thr, dtype=torch.float64):
    """masks = softmax(o) [k,2]; rows [k,8] = (image_i, box_regress(x1,y1,x2,y2), masks[:,1], cls_score, cls_pred); keep; key."""
    o, reg, bx = _t(o, dtype), _t(regress, dtype), _t(boxes, dtype)
    masks = torch.softmax(o, 1)
    p = masks[:, 1]
    rows = torch.cat((bx[:, :1], box_regress(reg, bx[:, 1:5]), p[:, None], bx[:, 6:8]), 1)
    return dict(masks=masks, rows=rows, keep=p > thr, key=p, keep_margin=p - thr, keep_terms=p.abs() + abs(thr))


def m2_heads(feat, boxes, class_num, W, thr, dtype=torch.float64):
    """Stage-2 heads from the pooled features [k,490] and the proposal rows [k, >= 8 + class_num]: net0 + LeakyReLU, net1 ->
    regress, net2 + sigmoid -> refine [k, class_num + 1], ensemble fc1 (2 -> 32, LeakyReLU) per class slot, fc2 (-> 2, LeakyReLU),
    softmax; p = column 1; rows as m2_rows."""
    w = _w(W, dtype)
    f, bx = _t(feat, dtype), _t(boxes, dtype)
    k, c1 = f.shape[0], class_num + 1
    hidden = leaky(f @ w["w0"].T + w["b0"])
    regress = hidden @ w["w1"].T + w["b1"]
    refine = torch.sigmoid(hidden @ w["w2"][:c1].T + w["b2"][:c1])
    x = torch.from_numpy(m2_pairs(refine.numpy(), bx.numpy())).reshape(k, c1, 2)
    h = leaky(x @ w["e1w"].T + w["e1b"])
    o = leaky(h.reshape(k, 32 * c1) @ w["e2w"].T + w["e2b"])
    out = m2_rows(o, regress, bx, thr, dtype)
    return dict(regress=regress, refine=refine, mask=out["key"], out_rows=out["rows"], keep=out["keep"], sort_key=out["key"], o=o,
                keep_margin=out["keep_margin"], keep_terms=out["keep_terms"])


def m2_regress_targets(boxes, tloc):
    """regression_loss's targets of the proposals [k, >= 5] against target_location [k,4] (xyxy)."""
    x, y, w, h = (boxes[:, 1] + boxes[:, 3]) / 2, (boxes[:, 2] + boxes[:, 4]) / 2, boxes[:, 3] - boxes[:, 1], boxes[:, 4] - boxes[:, 2]
    xt, yt, wt, ht = (tloc[:, 0] + tloc[:, 2]) / 2, (tloc[:, 1] + tloc[:, 3]) / 2, tloc[:, 2] - tloc[:, 0], tloc[:, 3] - tloc[:, 1]
    return torch.stack(((xt - x) / (w + 1e-16), (yt - y) / (h + 1e-16), torch.log(wt / w + 1e-16), torch.log(ht / h + 1e-16)), 1)


def m2_loss(o, refine, regress, boxes, tloc, clabel, pos, sample, alpha, lambda0, lambda1, grad_scale, dtype=torch.float64):
    """terms [k,5] = (focal on softmax(o) for the sampled rows - component 1 for a positive, 0 for a negative -, confidence BCE of
    refine[:,0] for the sampled rows, category BCE of refine[:,1:] against clabel, SmoothL1 xy, SmoothL1 wh for the positive
    rows), per RoI and unscaled, and d_o, d_refine, d_regress = the gradients of
    grad_scale * (focal + (conf + category) / lambda0 + (xy + wh) / lambda1) by autograd through those terms."""
    o, rf, reg = (_t(v, dtype).clone().requires_grad_(True) for v in (o, refine, regress))
    bx, tl, cl = _t(boxes, dtype), _t(tloc, dtype), _t(clabel, dtype)
    pos, smp = torch.as_tensor(np.asarray(pos)).bool(), torch.as_tensor(np.asarray(sample)).bool()
    k = o.shape[0]
    terms = torch.zeros((k, 5), dtype=dtype)
    si, pi = smp.nonzero().flatten(), pos.nonzero().flatten()
    sm = torch.softmax(o[si], 1)
    ps_ = pos[si]
    p = torch.where(ps_, sm[:, 1], sm[:, 0])
    a = torch.where(ps_, torch.tensor(alpha, dtype=dtype), torch.tensor(1 - alpha, dtype=dtype))
    cols = lambda c, n: (torch.full((n,), c, dtype=torch.long),)  # noqa: E731
    terms = terms.index_put((si,) + cols(0, len(si)), -a * (1 - p) ** 2 * torch.log(p))
    terms = terms.index_put((si,) + cols(1, len(si)), F.binary_cross_entropy(rf[si, 0], ps_.to(dtype), reduction="none"))
    terms = terms.index_put((pi,) + cols(2, len(pi)), F.binary_cross_entropy(rf[pi, 1:], cl[pi], reduction="none").sum(1))
    sl1 = F.smooth_l1_loss(m2_regress_targets(bx[pi], tl[pi]), reg[pi], reduction="none")
    terms = terms.index_put((pi,) + cols(3, len(pi)), sl1[:, :2].sum(1))
    terms = terms.index_put((pi,) + cols(4, len(pi)), sl1[:, 2:].sum(1))
    t = terms.sum(0)
    ((t[0] + (t[1] + t[2]) / lambda0 + (t[3] + t[4]) / lambda1) * grad_scale).backward()
    zg = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)  # noqa: E731
    return dict(terms=terms.detach(), d_o=zg(o), d_refine=zg(rf), d_regress=zg(reg))


def mask_scale(x, mask, scale):
    """y = mask ? x * scale : 0 in float64."""
    return np.where(np.asarray(mask) != 0, np.asarray(x, np.float64) * float(scale), 0.0)
