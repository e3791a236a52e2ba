"""Seeded inputs of tests/test_gpu_heads_blocks.py (numpy only, no kernel, no GPU): the GPU tests run them through the kernels,
tests/test_heads_refs_cpu.py asserts - from the references alone - the conditions the GPU tests rely on (exactness of the EXACT
inputs, the share of sign / threshold decisions within rounding distance of 0)."""
import numpy as np

from millieye_amd import synth

SCALE = 1.0 / 16


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------
def real_weights(tag, c2=13, slots=2):
    """fp32 weights with the state dict's shapes; ``c2`` rows of net2, ``slots`` class slots of the ensemble head's fc2."""
    n, u = synth.normal, synth.uniform
    t = "hb/" + tag
    rscale = u(t + "rs", (10,), 0.5, 1.5) * np.where(np.arange(10) % 3 == 1, -1, 1).astype(np.float32)
    return dict(w0=n(t + "w0", (256, 490), 0, 0.05), b0=n(t + "b0", (256,), 0, 0.1), w1=n(t + "w1", (4, 256), 0, 0.05),
                b1=n(t + "b1", (4,), 0, 0.1), w2=n(t + "w2", (c2, 256), 0, 0.1), b2=n(t + "b2", (c2,), 0, 0.1),
                rw=n(t + "rw", (10, 490), 0, 0.05), rb=n(t + "rb", (10,), 0, 0.1), rscale=rscale, rshift=n(t + "rh", (10,), 0, 0.3),
                rw2=n(t + "rw2", (10,), 0, 0.5), rb2=n(t + "rb2", (1,), 0, 0.1), e1w=n(t + "e1w", (32, 2), 0, 0.7),
                e1b=n(t + "e1b", (32,), 0, 0.3), e2w=n(t + "e2w", (2, 32 * slots), 0, 0.3), e2b=n(t + "e2b", (2,), 0, 0.1))


def exact_weights(seed, positive):
    """Small integers.  ``positive``: b0 = 8192 + (-4 .. 4) lifts every hidden pre-activation above 0 (|sum| <= 490 * 8 * 2), so
    that the hidden vector - and with it net1 / net2 - stays integer; otherwise b0 = -4 .. 4 and both LeakyReLU branches occur."""
    r = np.random.RandomState(seed)
    i = lambda shape, lo=-2, hi=2: r.randint(lo, hi + 1, shape).astype(np.float32)  # noqa: E731
    w = real_weights("exact")   # (the tail's weights: not used by the training-mode front end, but the pointers must be valid)
    w.update(w0=i((256, 490)), b0=i((256,), -4, 4) + (8192.0 if positive else 0.0), w1=i((4, 256)), b1=i((4,), -4, 4),
             w2=i((13, 256)), b2=i((13,), -4, 4), rw=i((10, 490)), rb=i((10,), -4, 4))
    return {k: np.asarray(v, np.float32) for k, v in w.items()}


# ---------------------------------------------------------------------------------------------------------------------
# stage-3 inputs
# ---------------------------------------------------------------------------------------------------------------------
def proposal_rows(tag, rois, cols):
    """[k, cols] proposal rows (image_i, x1,y1,x2,y2, obj, cls_conf, cls_pred, scores) around rois [k,5]; cls_pred is a class id
    1 .. 12, never 0: the kernels copy it into column 7 of out_rows, where radar rows carry a constant 0."""
    k = len(rois)
    rows = np.zeros((k, cols), np.float32)
    rows[:, :5] = rois
    rows[:, 5:] = synth.uniform("hb/" + tag + "conf", (k, cols - 5), 0.05, 0.95)
    rows[:, 7] = 1 + np.floor(synth.uniform("hb/" + tag + "cls", (k,)) * 12)
    return rows


def real_rois(tag, k, n, size):
    """k RoIs over n frames of size x size pixels, sorted by frame; from eight RoIs on the first six are a zero-area box, an inverted
    one, one outside the map, one far in the negative, one over the whole map and beyond, and a one-pixel sliver."""
    u = synth.uniform("hb/" + tag, (k, 5)).astype(np.float64)
    cx, cy = u[:, 1] * size, u[:, 2] * size
    w, h = 8 + u[:, 3] * size * 0.6, 8 + u[:, 4] * size * 0.6
    rois = np.stack((np.floor(u[:, 0] * n), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), 1)
    if k >= 8:
        rois[0, 1:] = (40.0, 52.0, 40.0, 52.0)
        rois[1, 1:] = (120.0, 100.0, 60.0, 30.0)
        rois[2, 1:] = (size + 50, size + 60, size + 90, size + 130)
        rois[3, 1:] = (-300.0, -280.0, -200.0, -150.0)
        rois[4, 1:] = (-size, -size, 2 * size, 2 * size)
        rois[5, 1:] = (33.3, 10.0, 34.1, 150.0)
    return rois[np.argsort(rois[:, 0], kind="stable")].astype(np.float32)


def real_case(tag, k_img, cap_img, k_rad, n, fh, fw, rh, rw, cols):
    """Score maps in the reference's layout (NCHW, channel (c*7+ph)*7+pw), proposals and radar boxes for the REAL runs."""
    size = 16.0 * max(fh, fw)
    m490 = synth.uniform("hb/" + tag + "m490", (n, 490, fh, fw), -1, 1)
    m10 = synth.uniform("hb/" + tag + "m10", (n, 10, rh, rw), 0, 1)
    boxes = np.zeros((cap_img, cols), np.float32)
    boxes[:k_img] = proposal_rows(tag, real_rois(tag + "img", k_img, n, size), cols)
    rad = real_rois(tag + "rad", k_rad, n, size) if k_rad else np.zeros((0, 5), np.float32)
    return dict(tag=tag, m490=m490, m10=m10, img_boxes=boxes, k_img=k_img, cap_img=cap_img, radar=rad, n=n, fh=fh, fw=fw, rh=rh,
                rw=rw, cols=cols)


# (tag, k_img, cap_img, k_rad, n, fh, fw, rh, rw, cols), then bin_major, radar_pitch, regress
REAL_CASES = {
    "a": (("a", 37, 45, 5, 2, 13, 13, 13, 13, 9), 1, 12, 1),
    "b": (("b", 66, 70, 9, 3, 10, 14, 13, 13, 12), 0, 10, 0),
}
BIG_CASE = (("big", 4000, 4090, 14, 2, 13, 13, 13, 13, 9), 1, 10, 1)   # 4104 slots = 513 workgroups of 8


def exact_case(seed, k_img, cap_img, k_rad, n, fh, fw, rh, rw, cols):
    """EXACT inputs of the front end: maps of small multiples of 4, boxes 112 px wide and high whose bilinear samples fall on
    half-pixel centres (image proposals at 8 + 16 a for PS-RoIAlign, radar boxes at 16 a for RoIAlign; spatial_scale 1/16)."""
    r = np.random.RandomState(seed)
    m490 = (4 * r.randint(-2, 3, (n, 490, fh, fw))).astype(np.float32)
    m10 = (4 * r.randint(0, 3, (n, 10, rh, rw))).astype(np.float32)

    def boxes(k, h, w, off):
        b = np.sort(r.randint(0, n, k))
        x1 = off + 16.0 * r.randint(0, w - 7, k)
        y1 = off + 16.0 * r.randint(0, h - 7, k)
        return np.stack((b, x1, y1, x1 + 112, y1 + 112), 1).astype(np.float32)

    rows = np.zeros((cap_img, cols), np.float32)
    rows[:k_img] = proposal_rows(f"exact{seed}", boxes(k_img, fh, fw, 8.0), cols)
    return dict(tag=f"exact{seed}", m490=m490, m10=m10, img_boxes=rows, k_img=k_img, cap_img=cap_img, radar=boxes(k_rad, rh, rw, 0.0),
                n=n, fh=fh, fw=fw, rh=rh, rw=rw, cols=cols)


# k = k_img + k_rad over {1, 7, 8, 9, 31, 32, 33, 65}: (k_img, cap_img, k_rad, n, fh, fw, rh, rw, cols, bin_major, radar_pitch)
EXACT_CASES = [
    (1, 3, 0, 1, 13, 13, 13, 13, 9, 1, 10),
    (6, 9, 1, 2, 13, 13, 10, 14, 9, 0, 12),
    (3, 4, 5, 2, 10, 14, 13, 13, 12, 1, 12),
    (9, 12, 0, 3, 13, 13, 13, 13, 9, 0, 10),
    (30, 40, 1, 2, 10, 14, 10, 14, 9, 1, 10),
    (27, 28, 5, 3, 13, 13, 10, 14, 12, 0, 12),
    (33, 34, 0, 2, 13, 13, 13, 13, 9, 1, 12),
    (60, 64, 5, 3, 10, 14, 13, 13, 9, 0, 10),
]


def all_rois(case):
    return np.concatenate((case["img_boxes"][:case["k_img"], :5], case["radar"]), 0).astype(np.float32)


def tv_pooled(case):
    """The oracle's fp32 RoI pooling (oracle/tv_ops: the torchvision restatement) of every RoI of a case: ([k,490], [k,490])."""
    import torch

    from oracle import tv_ops
    rois = torch.from_numpy(all_rois(case))
    fi = tv_ops.ps_roi_align(torch.from_numpy(case["m490"]), rois, (7, 7), spatial_scale=SCALE)
    fr = tv_ops.roi_align(torch.from_numpy(case["m10"]), rois, (7, 7), spatial_scale=SCALE)
    return fi.reshape(len(rois), 490).numpy(), fr.reshape(len(rois), 490).numpy()


def stage3_reference(case, W, feat_img, feat_rad, regress, dtype=None):
    """Front end + tail of tests/heads_refs.py on a case's pooled features, thresholds by pick_threshold from the float64 p."""
    import torch

    from tests import heads_refs as R
    k_img = case["k_img"]
    f = R.frontend(feat_img, feat_rad, W)
    t = R.tail(f["small"], all_rois(case), case["img_boxes"], k_img, W, 0.0, 0.0, regress)
    p = t["mask1"].numpy()
    thr_img, thr_rad = pick_threshold(p[:k_img]), pick_threshold(p[k_img:])
    if thr_img == thr_rad:
        thr_rad = float(np.float32(thr_rad * 0.75))
    dtype = dtype or torch.float64
    f = R.frontend(feat_img, feat_rad, W, dtype=dtype)
    t = R.tail(f["small"], all_rois(case), case["img_boxes"], k_img, W, thr_img, thr_rad, regress, dtype=dtype)
    return dict(t, small=f["small"], hidden=f["hidden"], thr_img=thr_img, thr_radar=thr_rad)


def pick_threshold(p):
    """A threshold inside the range of the reference's p (float64, NaN rows left out): the middle of the widest gap between
    neighbours in the middle half of the sorted values, as the fp32 number the kernel is handed.  A condition on the inputs,
    computed from the reference alone - it keeps the rows at rounding distance from the threshold rare."""
    v = np.sort(np.asarray(p, np.float64)[np.isfinite(p)])
    if len(v) < 4:
        return float(np.float32(v.mean() + 1e-3)) if len(v) else 0.5
    mid = v[len(v) // 4: len(v) - len(v) // 4]
    i = int(np.argmax(np.diff(mid)))
    return float(np.float32((mid[i] + mid[i + 1]) / 2))


# ---------------------------------------------------------------------------------------------------------------------
# tail / loss / backward inputs
# ---------------------------------------------------------------------------------------------------------------------
def tail_case(k, n_img, cols=9):
    """A ``small`` block as the front end would leave it, the RoIs and the proposal rows, for me_heads_tail_f32 and its backward."""
    t = f"tail{k}"
    small = synth.normal("hb/" + t + "s", (k, 16), 0, 1.0)
    small[:, 2:4] *= 0.3   # (exp of the size regressions)
    rois = real_rois(t + "r", k, 2, 208.0)
    return dict(small=small, rois=rois, img_boxes=proposal_rows(t, rois[:n_img], cols), n_img=n_img, cols=cols,
                radar=np.ascontiguousarray(rois[n_img:]))


BWD_CASE = (300, 211)   # (k, n_img) of the tail-backward test
M2_ROWS_CASES = [(1, 2), (255, 13), (257, 16), (700, 2)]   # (k, c1)


def m2_rows_case(k, c1):
    """Inputs of me_m2_pairs_f32 / me_m2_rows_f32: proposal rows with two columns more than the kernels read."""
    cols = 8 + c1 - 1 + 2
    t = f"m2pr{k}"
    return dict(cols=cols, boxes=proposal_rows(t, real_rois(t, k, 2, 208.0), cols), refine=synth.uniform("hb/" + t + "r", (k, c1), 0, 1),
                o=synth.normal("hb/" + t + "o", (k, 2), 0, 2.0), regress=synth.normal("hb/" + t + "g", (k, 4), 0, 0.4))


TAIL_KS = (1, 255, 256, 257)


def tail_real_case(k):
    """The case whose save_small block me_heads_tail_f32 is run on: three quarters image proposals, conv bias 0."""
    case = real_case("tail", k - k // 4, k - k // 4 + 2, k // 4, 2, 13, 13, 13, 13, 9)
    return case, dict(real_weights("tail"), rb=np.zeros(10, np.float32))


def loss_case():
    """All eight (label_pos, in_focal, in_conf) combinations, p and x swept over [1e-6, 1 - 1e-6] (log-spaced towards both ends),
    in one call; returns also the row count."""
    g = np.concatenate((10.0 ** np.linspace(-6, -0.31, 20), 1 - 10.0 ** np.linspace(-0.31, -6, 20)))
    p, x = np.meshgrid(g, g[::-1])
    p, x = np.tile(p.ravel(), 8).astype(np.float32), np.tile(x.ravel(), 8).astype(np.float32)
    combo = np.repeat(np.arange(8), g.size ** 2)
    return dict(mask1=p, conf=x, label_pos=(combo & 1).astype(np.uint8), in_focal=((combo >> 1) & 1).astype(np.uint8),
                in_conf=((combo >> 2) & 1).astype(np.uint8), k=p.size, alpha=0.6, lam=4.5)


def bce_endpoints():
    """x in {0, 1} against both labels (the -100 log clamp and the 1e-12 denominator clamp), and two ordinary values."""
    x = np.array([0, 0, 1, 1, 0.25, 0.75], np.float32)
    y = np.array([0, 1, 0, 1, 1, 0], np.uint8)
    return x, y


def m2_case(tag, k, class_num, cols, n=2, fh=13, fw=13):
    size = 16.0 * fh
    rois = real_rois("m2" + tag, k, n, size)
    last = np.flatnonzero(rois[:, 0] == rois[0, 0])[-1]   # the first frame's last RoI is an ordinary box: it goes in front, so
    rois[[0, last]] = rois[[last, 0]]                     # that a run of one row has a finite row to compare (asserted on the CPU)
    rows = proposal_rows("m2" + tag, rois, cols)
    rows[:, 7] = np.floor(synth.uniform("hb/m2" + tag + "cls", (k,)) * class_num)
    return dict(m490=synth.uniform("hb/m2" + tag + "map", (n, 490, fh, fw), -1, 1), boxes=rows, n=n, fh=fh, fw=fw)


def m2_loss_case(c1, k=96):
    """pos x sample in all four combinations; SmoothL1 residuals on both sides of 1 and none within 1e-3 of it (asserted by the CPU
    test); the last eight rows carry the BCE endpoints (refine 0 / 1 against both labels) and are compared apart."""
    t = f"m2l{c1}"
    o = synth.normal("hb/" + t + "o", (k, 2), 0, 2.0)
    refine = synth.uniform("hb/" + t + "r", (k, c1), 0.02, 0.98)
    boxes = proposal_rows(t, real_rois(t + "b", k, 2, 208.0)[:, :5], 8 + c1 - 1)
    boxes[:, 1:5] = np.stack((20 + 4.0 * np.arange(k) % 90, 30 + 3.0 * np.arange(k) % 70, 0 * np.arange(k), 0 * np.arange(k)), 1)
    boxes[:, 3] = boxes[:, 1] + 24 + np.arange(k) % 40
    boxes[:, 4] = boxes[:, 2] + 16 + np.arange(k) % 50
    jit = synth.uniform("hb/" + t + "j", (k, 4), -0.45, 0.45).astype(np.float64)
    w, h = (boxes[:, 3] - boxes[:, 1]).astype(np.float64), (boxes[:, 4] - boxes[:, 2]).astype(np.float64)
    cx, cy = boxes[:, 1] + w / 2 + jit[:, 0] * w, boxes[:, 2] + h / 2 + jit[:, 1] * h
    wt, ht = w * np.exp(jit[:, 2]), h * np.exp(jit[:, 3])
    tloc = np.stack((cx - wt / 2, cy - ht / 2, cx + wt / 2, cy + ht / 2), 1).astype(np.float32)
    regress = synth.normal("hb/" + t + "g", (k, 4), 0, 0.4)
    regress[::3] += np.where(np.arange(len(regress[::3]))[:, None] % 2 == 0, 2.0, -2.0).astype(np.float32)   # the linear side
    clabel = (synth.uniform("hb/" + t + "c", (k, c1 - 1)) < 0.2).astype(np.float32)
    pos, sample = (np.arange(k) % 2).astype(np.uint8), ((np.arange(k) // 2) % 2).astype(np.uint8)
    ends = np.arange(k - 8, k)
    refine[ends] = np.where(np.arange(8)[:, None] % 2 == 0, 0.0, 1.0).astype(np.float32)
    pos[ends] = (np.arange(8) // 2) % 2
    sample[ends] = 1
    clabel[ends] = ((np.arange(8) // 4) % 2)[:, None]
    return dict(o=o, refine=refine, regress=regress, boxes=boxes, tloc=tloc, clabel=clabel, pos=pos, sample=sample, k=k, c1=c1,
                ends=ends, alpha=0.6, lambda0=11.0, lambda1=3.0, grad_scale=0.37)
