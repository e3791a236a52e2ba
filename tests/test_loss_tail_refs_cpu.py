"""The references of tests/loss_tail_refs.py pinned on the CPU: the float32 form of ``yolo_loss_fwd_ref`` to the oracle's torch
restatement, ``batch_statistics_ref`` to the host ``get_batch_statistics``, ``adam_step_ref`` to ``torch.optim.Adam`` / ``AdamW``;
and the conditions on the inputs of tests/test_gpu_loss_tail.py (every decision clear of its threshold, the planted ties and
duplicates where the cases say they are), computed from the float64 reference alone."""
import numpy as np
import pytest
import torch

from tests import loss_tail_refs as R

NEW_NA3 = ("base", "base16", "base64", "mid", "empty", "sat")
ALL_NEW = ("min",) + NEW_NA3 + ("wide",)
DISCRETE = ("obj", "noobj", "tcls", "tconf", "class_mask")


def _same(a, b, rel):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rel * abs(b)


def _pin_to_oracle(case, anchors_arg, img_dim):
    from oracle import darknet_ref
    mine = R.yolo_loss_fwd_ref(case["raw"], case["anchors"], case["nc"], case["targets"], 0.5, 1.0, 100.0, np.float32)
    total, metrics, dense = darknet_ref.yolo_loss_terms(torch.from_numpy(case["raw"]), anchors_arg, case["nc"], img_dim,
                                                        torch.from_numpy(case["targets"].copy()))
    for k in R.DENSE:
        a, b = np.asarray(mine[k], np.float64), dense[k].numpy().astype(np.float64)
        assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-6, k
    assert mine["n_obj"] == dense["n_obj"] and mine["n_noobj"] == dense["n_noobj"]
    for i, k in enumerate(R.SCALARS):
        assert _same(float(mine["scalars"][i]), float(metrics[k]), 1e-6), (k, mine["scalars"][i], metrics[k])
    assert _same(float(mine["scalars"][0]), float(total), 1e-6)


@pytest.mark.parametrize("n,g,nc,m", R.LEGACY)
def test_yolo_float32_form_equals_the_oracle_on_the_existing_cases(n, g, nc, m):
    """The four cases of test_yolo_loss_kernel_vs_the_torch_restatement: dense tensors to 1e-6, scalars to 1e-6 relative."""
    _pin_to_oracle(R.legacy_yolo_case(n, g, nc, m), [(10, 13), (33, 23), (62, 45)], 32 * g)


@pytest.mark.parametrize("name", NEW_NA3)
def test_yolo_float32_form_equals_the_oracle_on_the_new_cases(name):
    """The new three-anchor cases (saturated logits and the overflowing width included); the anchors are handed over scaled
    (image size = grid size: stride 1)."""
    case = R.yolo_case(name)
    _pin_to_oracle(case, [(float(w), float(h)) for w, h in case["anchors"]], case["g"])


@pytest.mark.parametrize("name", ALL_NEW)
def test_yolo_cases_meet_the_condition_on_their_inputs(name):
    """No target and no cell has to be left out: every decision clears its threshold by 1e-4 relative (the planted exact ties
    apart), so the float32 form takes every decision as float64 does."""
    c = R.yolo_case(name)
    assert R.yolo_input_violations(c["raw"], c["anchors"], c["nc"], c["targets"], 0.5, c["planted"]) == []
    r64, r32 = R.yolo_ref(name), R.yolo_ref(name, "float32")
    assert r64["bad"] == 0 and (r64["winner"] >= 0).all()
    for k in DISCRETE + ("tx", "ty"):
        assert np.array_equal(np.asarray(r64[k], np.float64), np.asarray(r32[k], np.float64)), k
    assert r64["counts"] == r32["counts"] and r64["n_obj"] == r32["n_obj"] and r64["n_noobj"] == r32["n_noobj"]


@pytest.mark.parametrize("name", ("base", "base16", "base64", "wide"))
def test_yolo_cases_hold_what_they_plant(name):
    c, r = R.yolo_case(name), R.yolo_ref(name)
    g, tg, own, win = c["g"], c["targets"], r["owner"], r["winner"]
    tb = (tg[:, 2:6] * np.float32(g)).astype(np.float64)
    groups = [R.PAIR] + ([R.PAIR2, R.TRIPLE] if name == "wide" else [])
    for grp in groups:   # one owner; the last row wins the scalar targets, tcls holds every label
        at = tuple(own[grp[0]])
        last = grp[-1]
        assert all(tuple(own[k]) == at for k in grp) and all(win[k] == last for k in grp)
        assert r["tx"][at] == tb[last, 0] - np.floor(tb[last, 0]) and r["tx"][at] != tb[grp[0], 0] - np.floor(tb[grp[0], 0])
        assert r["tw"][at] == np.log(tb[last, 2] / np.float64(c["anchors"][at[1], 0]) + 1e-16)
        assert [int(i) for i in np.flatnonzero(r["tcls"][at])] == sorted(int(tg[k, 1]) for k in grp)
        assert len({int(tg[k, 1]) for k in grp}) == len(grp)
    a, b = (tuple(own[k]) for k in R.CELLMATES)
    assert a[0] == b[0] and a[2:] == b[2:] and a[1] != b[1] and r["obj"][a] == 1 and r["obj"][b] == 1
    assert win[R.CELLMATES[0]] == R.CELLMATES[0] and win[R.CELLMATES[1]] == R.CELLMATES[1]
    per = c["nc"] + 5
    for k, want in zip(R.CLASS_TIE, (1, 0)):   # logits 4 and 7 tie at the top: the first index is the argmax
        at = tuple(own[k])
        cl = c["raw"].reshape(c["n"], g, g, c["na"], per)[at[0], at[2], at[3], at[1], 5:]
        assert cl[4] == cl[7] == cl.max() and (np.delete(cl, [4, 7]) < cl[4]).all()
        assert int(tg[k, 1]) == (4, 7)[1 - want] and r["class_mask"][at] == want and win[k] == k
    assert own[R.NEG][3] == 0 and tb[R.NEG, 0] < 0 and abs(r["tx"][tuple(own[R.NEG])] - 0.7) < 1e-6
    assert own[R.LAST][3] == g - 1 and tg[R.LAST, 2] < 1
    if name in ("base16", "base64"):
        assert tb[R.NEG, 1] == 5.0 and r["ty"][tuple(own[R.NEG])] == 0.0   # cy * g is an integer, exactly
    raw5 = c["raw"].reshape(c["n"], g, g, c["na"], per)
    at, back = tuple(own[R.THRESH]), c["background"]
    assert raw5[at[0], at[2], at[3], at[1], 4] == 0 and r["obj"][at] == 1
    assert raw5[back[0], back[2], back[3], back[1], 4] == 0 and r["noobj"][back] == 1 and r["obj"][back] == 0
    if name == "wide":
        assert c["n"] * c["na"] * g * g > 256 * 256 and c["n"] * c["na"] * g * g * c["nc"] > 4096 * 256 and len(tg) > 256
        assert own[R.PAIR2[0]][0] == 0 and R.PAIR2[0] // 256 != R.PAIR2[1] // 256
        assert len({k // 256 for k in R.TRIPLE}) == 2
        assert np.array_equal(c["anchors"][2], c["anchors"][9])
        for k, ignored in ((R.TIE_HI, True), (R.TIE_LO, False)):
            at = tuple(own[k])
            twin = (at[0], 9, at[2], at[3])
            assert at[1] == 2 and win[k] == k and r["obj"][twin] == 0 and r["noobj"][twin] == (0 if ignored else 1)


def test_yolo_empty_and_saturated_cases():
    """No target: n_noobj = cells, every per-object mean NaN like the reference, precision and recall 0.  Saturated logits: the
    probabilities are exactly 1 or 0 in fp32, every clamped element contributes exactly 100, the overflowing width gives IoU 0."""
    e = R.yolo_ref("empty")
    c = R.yolo_case("empty")
    assert e["n_obj"] == 0 and e["n_noobj"] == c["n"] * c["na"] * c["g"] ** 2
    s = dict(zip(R.SCALARS, e["scalars"]))
    assert all(np.isnan(s[k]) for k in ("loss", "x", "y", "w", "h", "conf", "cls", "cls_acc", "conf_obj"))
    assert s["precision"] == 0 and s["recall50"] == 0 and s["recall75"] == 0 and np.isfinite(s["conf_noobj"])
    c = R.yolo_case("sat")
    r64, r32 = R.yolo_ref("sat"), R.yolo_ref("sat", "float32")
    assert np.isfinite(r64["scalars"]).all() and np.isfinite(r32["scalars"]).all()
    at = tuple(r64["owner"][R.THRESH])
    assert r64["winner"][R.THRESH] == R.THRESH and r32["iou_scores"][at] == 0 and 0 <= r64["iou_scores"][at] < 1e-30
    raw5 = c["raw"].reshape(c["n"], c["g"], c["g"], c["na"], c["nc"] + 5).transpose(0, 3, 1, 2, 4)
    assert set(np.unique(raw5[..., 4:])) == {np.float32(-104), np.float32(40)}
    want = R.sat_expected(c, r64)
    for D, rel in ((np.float32, 0.0), (np.float64, 1e-7)):
        for k, (obj_scale, noobj_scale) in enumerate(((1.0, 0.0), (0.0, 1.0))):
            got = R.yolo_loss_fwd_ref(c["raw"], c["anchors"], c["nc"], c["targets"], 0.5, obj_scale, noobj_scale, D)
            assert abs(got["scalars"][5] - want[k]) <= rel * want[k] and abs(got["scalars"][6] - want[2]) <= rel * want[2]


# ---------------------------------------------------------------------------------------------------------------------
def _host_tp(rows, targets, n_images, thr):
    from millieye_amd.test_fusion import regroup_outputs
    from millieye_amd.utils.utils import get_batch_statistics
    out = torch.from_numpy(rows)
    host = get_batch_statistics(regroup_outputs(out, n_images), torch.from_numpy(targets), iou_threshold=thr)
    tp = np.full(len(rows), np.nan)
    present = [i for i in range(n_images) if (rows[:, 0] == i).any()]
    assert len(host) == len(present)
    for i, (tp_i, _scores, labels) in zip(present, host):
        sel = rows[:, 0] == i
        assert np.array_equal(np.asarray(labels), rows[sel, -1])
        tp[sel] = tp_i
    return tp


@pytest.mark.parametrize("q,cols", [(q, 8) for q in R.STATS_Q] + [(130, 11), (65, 11)])
def test_batch_statistics_ref_equals_the_host_code(q, cols):
    """Every case of the GPU test: the reference equals get_batch_statistics(regroup_outputs(...)) row for row, writes exactly the
    rows of images inside the batch, and the case holds what it plants (first of two identical detections on a duplicated target
    is the true positive, the early image's later rows are 0, the highest target index is matched)."""
    rows, tg, n_images, notes = R.stats_case(q, cols)
    assert rows.shape[1] == cols and 4 <= n_images <= 6 and 200 <= len(rows) <= 400
    for thr in (0.5,) if q != 130 else (0.5, 0.3, 0.9):
        tp, written = R.batch_statistics_ref(rows, tg, n_images, thr)
        inside = (rows[:, 0] >= 0) & (rows[:, 0] < n_images)
        assert np.array_equal(written, inside) and 0 < (~inside).sum()
        host = _host_tp(rows, tg, n_images, thr)
        assert np.array_equal(tp[inside], host[inside]) and np.isnan(host[~inside]).all()
        for r, want in notes["expect"].items() if thr == 0.5 else ():
            assert tp[r] == want, (q, r, want)
        assert tp.sum() > len([w for w in notes["expect"].values() if w]) or q == 1
    assert (tg[:, 0] == n_images - 1).sum() == 0 and (rows[:, 0] == n_images - 1).any()      # an image without targets
    if notes["nodet"] >= 0 and q > 1:
        assert (tg[:, 0] == notes["nodet"]).any() and not (rows[:, 0] == notes["nodet"]).any()   # ... and one without detections
    if q >= 130:   # one image's targets sit in different lanes and in second / third trips of one lane
        mine = np.flatnonzero(tg[:, 0] == 0)
        assert len({t % 64 for t in mine}) > 8 and any((t + 64) in mine for t in mine) and mine.max() >= 128
    if q == 8192:
        assert (q - 1) >> 5 == 255 and (q - 1) & 31 == 31


def test_batch_statistics_exact_threshold():
    """IoU >= thr: a detection equal to its target is a true positive at thr = 1.0; a jittered one is at thr = its IoU and is
    not one fp32 step above."""
    rows, tg, n_images = R.stats_threshold_case()
    assert R.batch_statistics_ref(rows[:1], tg, n_images, 1.0)[0][0] == 1
    iou = R.stats_threshold_iou()
    assert 0.5 < iou < 1
    for thr, want in ((iou, 1), (np.nextafter(np.float32(iou), np.float32(2)), 0)):
        tp, _ = R.batch_statistics_ref(rows[1:], tg, n_images, thr)
        assert tp[0] == want and _host_tp(rows[1:], tg, n_images, float(thr))[0] == want


# ---------------------------------------------------------------------------------------------------------------------
TORCH_ULP = {"p": 12.0, "m": 3.0, "v": 7.0}   # measured, see the docstring below


@pytest.mark.parametrize("kind", sorted(R.ADAM_KINDS))
@pytest.mark.parametrize("t0", (0, 997))
def test_adam_ref_equals_torch_optim(kind, t0):
    """Three steps (t = 1..3 and 998..1000) from non-zero moments on the 64-tensor table against torch.optim.Adam / AdamW
    (foreach=False) on CPU tensors.  They are NOT bit-equal: torch's vectorised CPU kernels of ``lerp_``, ``addcmul_`` and
    ``add(alpha=)`` use a fused multiply-add, so after ONE step 21 % of exp_avg, 5 % of exp_avg_sq (25 % with L2 weight decay)
    and 0.2 % of the parameters differ from the one-rounding-per-operation form by one unit in the last place (3 / 5 units with
    weight decay, where g + wd * p feeds both moments).  Largest distances after the three steps, in fp32 units in the last
    place (the parameter's in units of the larger of the parameter before and after the step, since the step can cancel it):
        adam         p 10  m 2  v 2      adam_wd      p 12  m 3  v 7
        adamw        p 12  m 2  v 2      adamw_betas  p  2  m 2  v 3
    The pin is the largest of each column and nothing more.  The bar of the GPU test is not loosened by this: the kernel has
    contraction off and must equal ``adam_step_ref`` bit for bit."""
    decoupled, kw = R.ADAM_KINDS[kind]
    table = [t for t in R.adam_table() if len(t[0])]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p, _g, _m, _v in table]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(params, foreach=False, **kw)
    for prm, (_p, _g, m, v) in zip(params, table):
        opt.state[prm] = dict(step=torch.tensor(float(t0)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    mine = [(p.copy(), m.copy(), v.copy()) for p, _g, m, v in table]
    worst = dict(p=0.0, m=0.0, v=0.0)
    for s in range(3):
        sc = R.adam_scalars(kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"], t0 + s + 1)
        for i, (prm, (_p, g, _m, _v)) in enumerate(zip(params, table)):
            gs = g * np.float32(0.5 ** s)
            prm.grad = torch.from_numpy(gs.copy())
            mine[i] = R.adam_step_ref(mine[i][0], gs, mine[i][1], mine[i][2], sc, decoupled)
        before = [prm.detach().numpy().copy() for prm in params]
        opt.step()
        for prm, p0, (p, m, v) in zip(params, before, mine):
            st = opt.state[prm]
            for key, a, b, at in (("p", p, prm.detach().numpy(), p0), ("m", m, st["exp_avg"].numpy(), None),
                                  ("v", v, st["exp_avg_sq"].numpy(), None)):
                worst[key] = max(worst[key], R.ulp_distance(a, b, at))
    print(kind, t0, worst)
    for key in worst:
        assert worst[key] <= TORCH_ULP[key], (key, worst)
