"""The references of tests/heads_refs.py against something independent of them - the oracle's restatement of the reference
(oracle/network_ref.py: refinement, ensemble, box_regress, focal_loss on float64 state dicts; oracle/network_m2_ref.py; oracle/tv_ops),
torch float64 autograd through that code, the per-image Python loop of the proposal assembly - so that the yardstick of
tests/test_gpu_heads_blocks.py is itself checked without a GPU.  Tolerance 1e-12 of each tensor's largest magnitude where both
sides are float64, 1e-5 against the oracle's fp32-only whole-network functions (a structural pin: a wrong column is an error of 1).

The second half asserts, from the references alone, the conditions on the inputs of tests/heads_cases.py that the GPU tests rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from millieye_amd import cfgs, synth
from oracle import network_m2_ref
from oracle import network_ref as nr
from oracle import tv_ops
from tests import heads_cases as HC
from tests import heads_refs as R

f64 = torch.float64


def _close(got, ref, tol=1e-12, what=""):
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    assert err <= tol * max(1.0, float(np.abs(ref).max()) if ref.size else 1.0), (what, err)


def _sd(W):
    """A float64 state dict of the heads with the reference's names whose eval-mode radar BatchNorm is the affine (rscale, rshift):
    running_mean 0, running_var 1 - eps, weight rscale, bias rshift; the 7x7 conv carries its bias rb."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    p, e = "refinement_head.", "ensemble_head."
    return {p + "net0.0.weight": t(W["w0"]), p + "net0.0.bias": t(W["b0"]), p + "net1.0.weight": t(W["w1"]), p + "net1.0.bias": t(W["b1"]),
            p + "net2.0.weight": t(W["w2"]), p + "net2.0.bias": t(W["b2"]),
            p + "radar_net.0.weight": t(W["rw"]).reshape(10, 10, 7, 7), p + "radar_net.0.bias": t(W["rb"]),
            p + "radar_net.1.weight": t(W["rscale"]), p + "radar_net.1.bias": t(W["rshift"]),
            p + "radar_net.1.running_mean": torch.zeros(10, dtype=f64), p + "radar_net.1.running_var": torch.full((10,), 1 - 1e-5, dtype=f64),
            p + "radar_net.3.weight": t(W["rw2"]).reshape(1, 10, 1, 1), p + "radar_net.3.bias": t(W["rb2"]),
            e + "fc1.0.weight": t(W["e1w"]), e + "fc1.0.bias": t(W["e1b"]), e + "fc2.0.weight": t(W["e2w"]), e + "fc2.0.bias": t(W["e2b"])}


class _Recorder:
    """Stands in for ``torch.nn.functional`` inside oracle/network_ref: every call is passed on, its result keeps its gradient
    (retain_grad) and is remembered in call order.  The oracle writes the LeakyReLU slope as the literal 0.1, which in float64
    is not the float32 value the reference network and the kernels multiply with: leaky_relu gets R.SLOPE."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(F, name)

        def wrapped(*a, **kw):
            out = fn(a[0], R.SLOPE) if name == "leaky_relu" else fn(*a, **kw)
            if isinstance(out, torch.Tensor) and out.requires_grad:
                out.retain_grad()
            self.calls.append((name, out))
            return out
        return wrapped


# ---------------------------------------------------------------------------------------------------------------------
# the references against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("class_idx,class_num,num_classes", [(-1, 12, 12), (0, 1, 12), (5, 0, 80), (7, 12, 80)])
def test_gather_class_boxes_ref_is_the_per_image_loop(class_idx, class_num, num_classes):
    r = np.random.RandomState(3)
    n, max_det = 4, 9
    det = r.rand(n, max_det, 7 + num_classes).astype(np.float32)
    det[:, :, 6] = r.randint(0, 7, (n, max_det))
    count = np.array([0, 9, 4, 13], np.int32)   # (13 > max_det: the kernels clamp)
    want = []
    for i in range(n):   # my_models.py:459-473 as oracle/network_ref.network_forward restates it
        d = torch.from_numpy(det[i, :min(count[i], max_det)])
        if class_idx >= 0:
            d = d[d[:, 6] == class_idx]
        if len(d) > 0:
            b = torch.zeros((len(d), 8 + class_num))
            b[:, 0] = i
            b[:, 1:] = d[:, :7 + class_num]
            want.append(b)
    want = torch.cat(want, 0).numpy() if want else np.zeros((0, 8 + class_num), np.float32)
    rows, total = R.gather_class_boxes(det, count, class_idx, class_num)
    assert total == len(want) and rows.dtype == np.float32 and np.array_equal(rows, want)
    assert total > 0 or class_idx == 7


def test_pooling_refs_against_tv_ops():
    """Bit-equal on the EXACT inputs (where every sample is exact), 1e-5 on real boxes (float64 against the oracle's fp32)."""
    args = HC.EXACT_CASES[2]
    case = HC.exact_case(2, *args[:9])
    fi, fr = HC.tv_pooled(case)
    nhwc = lambda m: m.transpose(0, 2, 3, 1)  # noqa: E731
    assert np.array_equal(R.ps_roi_align(nhwc(case["m490"]), HC.all_rois(case), HC.SCALE), fi)
    assert np.array_equal(R.roi_align(nhwc(case["m10"]), HC.all_rois(case), HC.SCALE), fr)
    case = HC.real_case("pin", 10, 10, 4, 2, 10, 14, 13, 13, 9)
    fi, fr = HC.tv_pooled(case)
    rois = HC.all_rois(case)
    ok = np.isfinite(fi).all(1)
    assert ok.sum() >= len(rois) - 2   # (the zero-area and the inverted PS-RoI are NaN)
    _close(R.ps_roi_align(nhwc(case["m490"]), rois, HC.SCALE)[ok], fi[ok], 1e-5)
    _close(R.roi_align(nhwc(case["m10"]), rois, HC.SCALE), fr, 1e-5)


def _oracle_stage3(W, fi, fr, boxes, k_img, rois, thr_img, thr_rad, regress):
    """network_ref.network_forward's lines behind the pooling, on float64 tensors."""
    sd = _sd(W)
    k = len(rois)
    ci = torch.from_numpy(fi.astype(np.float64)).reshape(k, 10, 7, 7)
    cr = torch.from_numpy(fr.astype(np.float64)).reshape(k, 10, 7, 7)
    bx, rb = torch.from_numpy(boxes[:k_img].astype(np.float64)), torch.from_numpy(rois[k_img:].astype(np.float64))
    reg, rv = nr.refinement(sd, cr, ci)
    radar_rows = torch.cat((rb, rv[k_img:], torch.zeros((k - k_img, 1), dtype=f64), rv[k_img:, 1:]), -1)
    allb = torch.cat((bx[:, :8], radar_rows[:, :8]), 0)
    masks_img = nr.ensemble(sd, rv[:k_img], torch.cat((bx[:, 5:6], bx[:, 8:9]), 1))
    p = torch.cat((masks_img[:, 0], rv[k_img:, 0]))
    positive = torch.cat((p[:k_img] > thr_img, p[k_img:] > thr_rad))
    located = nr.box_regress(reg, allb[:, 1:5]) if regress else allb[:, 1:5]
    rows = torch.cat((allb[:, :1], located, p[:, None], allb[:, 6:8]), -1)
    key = p.clone()
    key[k_img:] /= 5
    return dict(regress=reg, refine=rv, mask1=p, keep=positive, out_rows=rows, sort_key=key)


@pytest.mark.parametrize("name", ["a", "b"])
def test_frontend_and_tail_refs_against_the_oracle(name, monkeypatch):
    monkeypatch.setattr(nr, "F", _Recorder())
    args, _bm, _pitch, regress = HC.REAL_CASES[name]
    case = HC.real_case(*args)
    W = HC.real_weights(name)
    fi, fr = HC.tv_pooled(case)
    ok = np.isfinite(fi).all(1)
    rois = HC.all_rois(case)
    k_img = case["k_img"]
    f = R.frontend(fi, fr, W, rb=W["rb"])
    t = R.tail(f["small"], rois, case["img_boxes"], k_img, W, 0.41, 0.57, regress)
    want = _oracle_stage3(W, fi, fr, case["img_boxes"], k_img, rois, 0.41, 0.57, regress)
    for key in ("regress", "refine", "mask1", "out_rows", "sort_key"):
        _close(t[key][ok], want[key][ok], 1e-12, key)
    assert torch.equal(t["keep"], want["keep"]) and 0 < int(t["keep"].sum()) < len(rois)
    # the inference kernels' small leaves the conv bias to rshift
    W2 = dict(W, rshift=(W["rshift"].astype(np.float64) + W["rb"].astype(np.float64) * W["rscale"].astype(np.float64)))
    t2 = R.tail(R.frontend(fi, fr, W)["small"], rois, case["img_boxes"], k_img, W2, 0.41, 0.57, regress)
    _close(t2["mask1"][ok], want["mask1"][ok], 1e-12)


def test_loss_and_tail_backward_refs_against_autograd_through_the_oracle(monkeypatch):
    """The seeds against autograd through focal_loss / binary_cross_entropy on leaves p and conf; then every output of the tail
    backward against the gradients that autograd leaves on the intermediate tensors of refinement() and ensemble()."""
    args, _bm, _pitch, _regress = HC.REAL_CASES["a"]
    case = HC.real_case(*args)
    W = HC.real_weights("a")
    fi, fr = HC.tv_pooled(case)
    ok = np.isfinite(fi).all(1)
    fi, fr = fi[ok], fr[ok]
    boxes = case["img_boxes"][:case["k_img"]][ok[:case["k_img"]]]
    k, k_img = len(fi), len(boxes)
    alpha, lam = 0.75, 6.0   # (alpha exactly representable: focal_loss builds it as a float32 tensor)
    r = np.random.RandomState(9)
    pos, sampled = r.rand(k) < 0.4, r.rand(k) < 0.7
    in_focal = sampled & (np.arange(k) < k_img)

    rec = _Recorder()
    monkeypatch.setattr(nr, "F", rec)
    sd = _sd(W)
    ci = torch.from_numpy(fi.astype(np.float64)).reshape(k, 10, 7, 7).requires_grad_(True)
    cr = torch.from_numpy(fr.astype(np.float64)).reshape(k, 10, 7, 7).requires_grad_(True)
    reg, rv = nr.refinement(sd, cr, ci)
    rv.retain_grad()
    bx = torch.from_numpy(boxes.astype(np.float64))
    masks_img = nr.ensemble(sd, rv[:k_img], torch.cat((bx[:, 5:6], bx[:, 8:9]), 1))
    masks_img.retain_grad()
    names = [c[0] for c in rec.calls]
    assert names == ["linear", "leaky_relu", "linear", "linear", "conv2d", "batch_norm", "leaky_relu", "conv2d", "linear", "leaky_relu",
                     "linear"], names
    t_ = {i: c[1] for i, c in enumerate(rec.calls)}
    hidden, reg_t, z2, rconv, rl, rlogit, fc1_pre, h_act, o = t_[1], t_[2], t_[3], t_[4], t_[6], t_[7], t_[8], t_[9], t_[10]
    masks = torch.cat((masks_img[:, :1], rv[k_img:, :1]), 0)
    masks = torch.cat((1 - masks, masks), -1)
    onehot = torch.tensor([1.0, 0.0], dtype=f64).repeat(k, 1)
    onehot[torch.from_numpy(pos)] = torch.tensor([0.0, 1.0], dtype=f64)
    sel = torch.from_numpy(in_focal)
    masks_loss = nr.focal_loss(masks[sel], onehot[sel], alpha)
    cl = torch.from_numpy(pos.astype(np.float64))
    ss = torch.from_numpy(sampled)
    conf_loss = F.binary_cross_entropy(rv[ss, 0], cl[ss], reduction="sum")
    (masks_loss + conf_loss / lam).backward()

    # the front end and the tail (once more, now from the recorded tensors)
    f = R.frontend(fi, fr, W, rb=W["rb"])
    _close(f["hidden"], hidden, 1e-12)
    small = torch.cat((reg_t, z2[:, :2], rconv.reshape(k, 10)), 1).detach()
    _close(f["small"], small, 1e-12)
    rois = HC.all_rois(case)[ok]
    tl = R.tail(small, rois, boxes, k_img, W, 0.0, 0.0, 1)
    _close(tl["o"], o, 1e-12)
    p = torch.cat((masks_img[:, 0], rv[k_img:, 0])).detach()
    _close(tl["mask1"], p, 1e-12)

    # the seeds: autograd on leaves
    pl, xl = p.clone().requires_grad_(True), rv[:, 0].detach().clone().requires_grad_(True)
    m2 = torch.stack((1 - pl, pl), 1)
    l_f, l_c = nr.focal_loss(m2[sel], onehot[sel], alpha), F.binary_cross_entropy(xl[ss], cl[ss], reduction="sum") / lam
    (l_f + l_c).backward()
    ls = R.heads_loss(p, rv[:, 0].detach(), pos, in_focal, sampled, alpha, lam)
    _close(ls["seed_p"], pl.grad, 1e-12, "seed_p")
    _close(ls["seed_conf"], xl.grad, 1e-12, "seed_conf")
    _close(ls["terms"].sum(0), torch.stack((l_f, l_c)).detach(), 1e-12, "terms")
    assert bool((ls["terms"][~sel, 0] == 0).all()) and bool((ls["terms"][~ss, 1] == 0).all())

    # the tail backward against what autograd left on the oracle's intermediates
    b = R.tail_bwd(small, rv.detach(), p, ls["seed_p"], ls["seed_conf"], boxes, k_img, W)
    zpad = lambda t, cols: torch.cat((t.reshape(k_img, cols), torch.zeros((k - k_img, cols), dtype=f64)))  # noqa: E731
    _close(b["g_o"], zpad(o.grad, 2), 1e-12, "g_o")
    _close(b["g_hpre"], zpad(fc1_pre.grad, 64), 1e-12, "g_hpre")
    _close(b["h_act"], zpad(h_act.detach(), 64), 1e-12, "h_act")
    x_in = torch.stack((rv[:k_img].detach(), torch.stack((bx[:, 5], bx[:, 8]), 1)), -1)
    _close(b["xin"], zpad(x_in, 4), 1e-12, "xin")
    _close(b["g_z2"], z2.grad[:, :2], 1e-12, "g_z2")
    _close(b["g_rl"], rl.grad.reshape(k, 10), 1e-12, "g_rl")
    _close(b["rl"], rl.detach().reshape(k, 10), 1e-12, "rl")
    _close(b["g_rlogit"], rlogit.grad.reshape(k), 1e-12, "g_rlogit")
    assert float(b["g_hpre"].abs().max()) > 0 and float(b["g_rl"][k_img:].abs().max()) > 0
    # seed_p of a radar row is not read (the objective's focal term runs over image proposals)
    sp2 = ls["seed_p"].clone()
    sp2[k_img:] = 123.0
    b2 = R.tail_bwd(small, rv.detach(), p, sp2, ls["seed_conf"], boxes, k_img, W)
    assert all(torch.equal(b[key], b2[key]) for key in b)


def test_m2_refs_against_the_oracle_forward():
    """network_m2_ref.network_m2_forward (fp32, whole network) on the golden stage-2 case: its pooled features and proposal rows
    through m2_heads / m2_pairs / m2_rows give its regress, refine and masks."""
    from millieye_amd.module2.my_models import Network, define_yolo
    from tests.golden.make_golden import M2_CASES, m2_fill_
    from tests.parity_helpers import cfg_path
    name, cfg, n, s, conf = M2_CASES[0]
    net = m2_fill_(Network(define_yolo(cfg_path(cfg)), conf), name)
    x = torch.from_numpy(synth.uniform(name + "/x", (n, 3, s, s)))
    sd = net.state_dict()
    _o, it = network_m2_ref.network_m2_forward(cfgs.KNOWN[cfg](), sd, x, conf_thresh=conf, return_internals=True)
    thr = HC.pick_threshold(it["masks"][:, 1].double().numpy())
    out, it = network_m2_ref.network_m2_forward(cfgs.KNOWN[cfg](), sd, x, conf_thresh=conf, refine_threshold=thr, return_internals=True)
    k = len(it["boxes"])
    assert k > 8
    g = lambda key: sd[key].numpy()  # noqa: E731
    W = dict(w0=g("refinement_head.net0.0.weight"), b0=g("refinement_head.net0.0.bias"), w1=g("refinement_head.net1.0.weight"),
             b1=g("refinement_head.net1.0.bias"), w2=g("refinement_head.net2.0.weight"), b2=g("refinement_head.net2.0.bias"),
             e1w=g("ensemble_head.fc1.0.weight"), e1b=g("ensemble_head.fc1.0.bias"), e2w=g("ensemble_head.fc2.0.weight"),
             e2b=g("ensemble_head.fc2.0.bias"))
    m = R.m2_heads(it["crop"].reshape(k, 490), it["boxes"], 12, W, thr)
    _close(m["regress"], it["regress"], 1e-5)
    _close(m["refine"], it["refine"], 1e-5)
    _close(m["mask"], it["masks"][:, 1], 1e-5)
    kept = m["keep"].numpy()
    rows = m["out_rows"][torch.from_numpy(kept)]
    rows = rows[torch.sort(rows[:, 5], descending=True, stable=True).indices]
    assert 0 < kept.sum() < k and rows.shape == out.shape
    _close(rows, out, 1e-5)
    pairs = R.m2_pairs(it["refine"].numpy(), it["boxes"].numpy())
    yolo = torch.cat((it["boxes"][:, 5:6], it["boxes"][:, 8:]), 1)
    assert np.array_equal(pairs, torch.stack((it["refine"], yolo), -1).reshape(-1, 2).numpy())
    r2 = R.m2_rows(m["o"], m["regress"], it["boxes"], thr)
    assert torch.equal(r2["rows"], m["out_rows"]) and torch.equal(r2["keep"], m["keep"])
    _close(r2["masks"].sum(1), torch.ones(k, dtype=f64), 1e-12)


@pytest.mark.parametrize("c1", [2, 13])
def test_m2_loss_ref_against_autograd_through_the_oracles_statements(c1):
    """network_m2_ref.network_m2_train_step's loss lines (:118-138: selections by filter, sums over the selection) in float64."""
    from oracle.network_ref import xyxy2xywh
    c = HC.m2_loss_case(c1)
    alpha, l0, l1, gs = c["alpha"], c["lambda0"], c["lambda1"], c["grad_scale"]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    o, rv, rp_all = t(c["o"]).requires_grad_(True), t(c["refine"]).requires_grad_(True), t(c["regress"]).requires_grad_(True)
    boxes, tloc, clabel = t(c["boxes"]), t(c["tloc"]), t(c["clabel"])
    pos_filter, sample_filter = torch.from_numpy(c["pos"]).bool(), torch.from_numpy(c["sample"]).bool()
    masks = torch.softmax(o, dim=1)
    label_onehot = torch.tensor([1.0, 0.0], dtype=f64).repeat(c["k"], 1)
    label_onehot[pos_filter] = torch.tensor([0.0, 1.0], dtype=f64)
    lab, m = label_onehot[sample_filter], masks[sample_filter]
    a = torch.where(lab[:, 1:2] == 1, torch.full((len(lab), 1), alpha, dtype=f64), torch.full((len(lab), 1), 1 - alpha, dtype=f64))
    probs = (m * lab).sum(1).view(-1, 1)
    masks_loss = (-a * torch.pow(1 - probs, 2) * probs.log()).sum()
    conf_loss = F.binary_cross_entropy(rv[sample_filter, 0], pos_filter.to(f64)[sample_filter], reduction="sum")
    xr, yr, wr, hr = xyxy2xywh(boxes[pos_filter, 1:5]).t()
    xt, yt, wt, ht = xyxy2xywh(tloc[pos_filter]).t()
    p01 = torch.stack(((xt - xr) / (wr + 1e-16), (yt - yr) / (hr + 1e-16)), -1)
    p23 = torch.stack((torch.log(wt / wr + 1e-16), torch.log(ht / hr + 1e-16)), -1)
    rp = rp_all[pos_filter]
    loss_xy = F.smooth_l1_loss(p01, rp[:, :2], reduction="sum")
    loss_wh = F.smooth_l1_loss(p23, rp[:, 2:], reduction="sum")
    category_loss = F.binary_cross_entropy(rv[pos_filter, 1:], clabel[pos_filter], reduction="sum")
    loss = masks_loss + (conf_loss + category_loss) / l0 + (loss_xy + loss_wh) / l1
    (loss * gs).backward()
    got = R.m2_loss(c["o"], c["refine"], c["regress"], c["boxes"], c["tloc"], c["clabel"], c["pos"], c["sample"], alpha, l0, l1, gs)
    _close(got["terms"].sum(0), torch.stack((masks_loss, conf_loss, category_loss, loss_xy, loss_wh)).detach(), 1e-12, "terms")
    _close(got["d_o"], o.grad, 1e-12)
    _close(got["d_refine"], rv.grad, 1e-12)
    _close(got["d_regress"], rp_all.grad, 1e-12)
    neither = ~(pos_filter | sample_filter)
    assert bool(neither.any()) and bool((got["terms"][neither] == 0).all()) and bool((got["d_refine"][neither] == 0).all())
    assert np.array_equal(R.mask_scale([1.5, -2.0, 3.0], [1, 0, 7], 2.0), [3.0, 0.0, 6.0])


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(HC.EXACT_CASES)))
def test_exact_inputs_are_exact(idx):
    """Every pooled value, weight and partial sum of the EXACT front-end inputs is an integer below 2^24: the fp32 result cannot
    depend on the order of summation.  Bound on the partial sums: sum |w| |f| + |b|.  With the lifted b0 the hidden vector is
    positive, so net1 / net2 are exact too; without it both LeakyReLU branches occur."""
    args = HC.EXACT_CASES[idx]
    case = HC.exact_case(idx, *args[:9])
    nhwc = lambda m: m.transpose(0, 2, 3, 1)  # noqa: E731
    rois = HC.all_rois(case)
    assert len(rois) == (1, 7, 8, 9, 31, 32, 33, 65)[idx] and case["cap_img"] > case["k_img"]
    fi, fr = R.ps_roi_align(nhwc(case["m490"]), rois, HC.SCALE), R.roi_align(nhwc(case["m10"]), rois, HC.SCALE)
    tvi, tvr = HC.tv_pooled(case)
    assert np.array_equal(fi, tvi) and np.array_equal(fr, tvr)
    assert np.array_equal(fi, np.round(fi)) and np.array_equal(fr, np.round(fr)) and np.abs(fi).max() > 0
    k_img = case["k_img"]
    assert len(np.unique(fi[:k_img] % 4)) > 1 or k_img == 0, "the four bilinear weights of 1/4 must show in the image branch"
    for positive in (True, False):
        W = HC.exact_weights(100 + idx, positive)
        for key in ("w0", "b0", "w1", "b1", "w2", "b2", "rw", "rb"):
            assert np.array_equal(W[key], np.round(W[key]))
        a = lambda v: np.abs(np.asarray(v, np.float64))  # noqa: E731
        assert (a(fi) @ a(W["w0"]).T + a(W["b0"])).max() < 2 ** 24
        assert (a(fr) @ a(W["rw"]).T + a(W["rb"])).max() < 2 ** 24
        f = R.frontend(fi, fr, W, rb=W["rb"])
        pre = f["hidden_pre"].numpy()
        if positive:
            assert pre.min() > 0
            assert (a(f["hidden"]) @ a(np.concatenate((W["w1"], W["w2"][:2]))).T + 4).max() < 2 ** 24
            assert np.array_equal(f["small"].numpy(), np.round(f["small"].numpy()))
        else:
            assert (pre > 0).any() and (pre < 0).any()


def test_real_inputs_keep_their_decisions_away_from_rounding():
    """keep = p > thr: the rows whose float64 p - thr lies within 8 * 2^-24 * (|p| + |thr|) of 0 are left out of the GPU
    comparison; at most 1 % of any case (in fact none: pick_threshold puts the thresholds into gaps).  The thresholds differ and
    lie inside the range of p."""
    for name, (args, _bm, _pitch, regress) in list(HC.REAL_CASES.items()) + [("big", HC.BIG_CASE)]:
        case = HC.real_case(*args)
        fi, fr = HC.tv_pooled(case)
        ref = HC.stage3_reference(case, HC.real_weights(name), fi, fr, regress)
        p, k_img = ref["mask1"].numpy(), case["k_img"]
        ok = np.isfinite(p)
        assert ok.sum() >= len(p) - 4   # (zero-area and inverted PS-RoIs, among the proposals and the radar boxes)
        assert ref["thr_img"] != ref["thr_radar"]
        assert np.nanmin(p[:k_img]) < ref["thr_img"] < np.nanmax(p[:k_img]) and np.nanmin(p[k_img:]) < ref["thr_radar"] < np.nanmax(p[k_img:])
        near = R.near_zero(ref["keep_margin"].numpy()[ok], ref["keep_terms"].numpy()[ok])
        assert near.mean() <= 0.01, (name, near.mean())
        keep = ref["keep"].numpy()[ok]
        assert 0.2 < keep.mean() < 0.8


def test_tail_kernel_inputs_keep_their_decisions_away_from_rounding():
    for k in HC.TAIL_KS:
        case, W = HC.tail_real_case(k)
        ref = HC.stage3_reference(case, W, *HC.tv_pooled(case), 1)
        ok = np.isfinite(ref["mask1"].numpy())
        assert R.near_zero(ref["keep_margin"].numpy()[ok], ref["keep_terms"].numpy()[ok]).mean() <= 0.01, k


@pytest.mark.parametrize("k,n_img", [(1, 1), (255, 192), (256, 192), (257, 193), HC.BWD_CASE])
def test_tail_inputs_keep_their_decisions_away_from_rounding(k, n_img):
    """The tail's keep and the LeakyReLU branches of the tail backward (fc1 pre-activation within 8 * 2^-24 * sum |terms| of 0)."""
    c = HC.tail_case(k, n_img)
    W = HC.real_weights("tail")
    t = R.tail(c["small"], c["rois"], c["img_boxes"], n_img, W, 0.0, 0.0, 1)
    thr = HC.pick_threshold(t["mask1"].numpy())
    t = R.tail(c["small"], c["rois"], c["img_boxes"], n_img, W, thr, thr * 0.75, 1)
    assert R.near_zero(t["keep_margin"].numpy(), t["keep_terms"].numpy()).mean() <= 0.01
    b = R.tail_bwd(c["small"], t["refine"], t["mask1"], np.ones(k), np.ones(k), c["img_boxes"], n_img, W)
    assert R.near_zero(b["pre"].numpy(), b["pre_terms"].numpy()).mean() <= 0.01
    assert (b["pre"].numpy() > 0).any() and (b["pre"].numpy() < 0).any()


@pytest.mark.parametrize("c1", [2, 13])
def test_m2_loss_inputs_cover_both_sides_of_smooth_l1(c1):
    c = HC.m2_loss_case(c1)
    pos = c["pos"].astype(bool)
    d = (R.m2_regress_targets(torch.from_numpy(c["boxes"].astype(np.float64)), torch.from_numpy(c["tloc"].astype(np.float64)))
         - torch.from_numpy(c["regress"].astype(np.float64))).numpy()[pos]
    assert (np.abs(d) < 1).any() and (np.abs(d) > 1).any() and (np.abs(np.abs(d) - 1) > 1e-3).all()
    combos = {(int(p), int(s)) for p, s in zip(c["pos"][:-8], c["sample"][:-8])}
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    lc = HC.loss_case()
    assert {(a, b, d_) for a, b, d_ in zip(lc["label_pos"], lc["in_focal"], lc["in_conf"])} == {(a, b, d_) for a in (0, 1) for b in (0, 1) for d_ in (0, 1)}
    assert lc["mask1"].min() <= 1.0001e-6 and lc["mask1"].max() >= 1 - 1.2e-6


def test_m2_inputs_keep_their_decisions_away_from_rounding():
    """keep = masks[:, 1] > threshold of me_m2_heads_f32 and me_m2_rows_f32 on the GPU tests' cases and thresholds."""
    for class_num in (1, 12, 15):
        c1, cols = class_num + 1, 8 + class_num + 3
        W = HC.real_weights(f"m2h{class_num}", c2=c1, slots=c1)
        for cap in (9, 24):
            c = HC.m2_case(f"{class_num}_{cap}", cap, class_num, cols)
            feat = tv_ops.ps_roi_align(torch.from_numpy(c["m490"]), torch.from_numpy(c["boxes"][:, :5].copy()), (7, 7),
                                       spatial_scale=HC.SCALE).reshape(cap, 490).numpy()
            thr = HC.pick_threshold(R.m2_heads(feat, c["boxes"], class_num, W, 0.0)["mask"].numpy())
            ref = R.m2_heads(feat, c["boxes"], class_num, W, thr)
            ok = np.isfinite(ref["mask"].numpy())
            assert ok.sum() >= cap - 2 and 0 < ref["keep"].numpy()[ok].sum() < ok.sum()
            assert ok[0]   # (the run with *n_boxes = 1 compares this row)
            assert not R.near_zero(ref["keep_margin"].numpy()[ok], ref["keep_terms"].numpy()[ok]).any()
    for k, c1 in HC.M2_ROWS_CASES:
        c = HC.m2_rows_case(k, c1)
        thr = HC.pick_threshold(R.m2_rows(c["o"], c["regress"], c["boxes"], 0.0)["key"].numpy())
        ref = R.m2_rows(c["o"], c["regress"], c["boxes"], thr)
        assert R.near_zero(ref["keep_margin"].numpy(), ref["keep_terms"].numpy()).mean() <= 0.01
