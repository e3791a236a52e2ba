"""-m gpu: the RoI-head and stage-2 kernels (csrc/heads.hip, csrc/m2_train.hip) one by one through the C ABI against the plain
float64 references of tests/heads_refs.py (pinned to the oracle and to torch float64 autograd by tests/test_heads_refs_cpu.py), on
the seeded inputs of tests/heads_cases.py (whose conditions the same CPU test asserts).  Conventions of tests/test_gpu_train_blocks.py:

* EXACT inputs: every pooled value, weight and partial sum is an fp32 integer - the kernel must equal float64 BIT FOR BIT.
  One necessary exception: with integer weights whose hidden vector takes both LeakyReLU branches, slope * negative integer is
  no integer, so net1 / net2 of save_small (columns 0..5) cannot be bit-exact there and are held to the dot-product bound
  256 * 2^-24 * sum |w| |h|; a second weight set whose lifted b0 keeps the hidden vector positive checks them bit for bit.
* REAL inputs: the kernel's largest error against float64, relative to the output's largest magnitude, must be at most
  max(16 x the same error of stock torch fp32 on the CPU computing the same operation, 4 * 2^-24) (``_bar``).  Both errors of
  every such case go to profiles/heads_blocks_errors.txt.
* Two generations of a kernel on the same inputs: 2e-6 relative (the bar of test_two_launch_heads_equal_the_fused_launch), and
  whether they were in fact bit-identical is printed.
* A sign or threshold decision (keep = p > thr, the LeakyReLU derivative in the tail backward) whose float64 operand lies within
  8 * 2^-24 * sum |terms| of 0 is left out of the comparison; the left-out share must stay <= 1 %.
* Outputs are poisoned, buffers carry rows / columns of sentinel behind what the kernel may write."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (the children below run this file as a script)
    sys.path.insert(0, ROOT)

from tests import heads_cases as HC  # noqa: E402
from tests import heads_refs as R  # noqa: E402
from tests.test_gpu_train_blocks import SENT, U, _bar, _bits_equal, _rel  # noqa: E402

pytestmark = pytest.mark.gpu
ERRORS_FILE = os.path.join(ROOT, "profiles", "heads_blocks_errors.txt")
_LOG = {}
F32 = torch.float32
PAD_ROWS = 3
KEEP_POISON = 7


def _log(section, line):
    _LOG.setdefault(section, []).append(line)
    print(f"[{section}] {line}")


@pytest.fixture(scope="module", autouse=True)
def _write_errors_file():
    """Sections of profiles/heads_blocks_errors.txt are replaced by the tests that ran; the others stay."""
    yield
    if not _LOG:
        return
    sections, cur = {}, None
    if os.path.exists(ERRORS_FILE):
        for line in open(ERRORS_FILE).read().splitlines():
            if line.startswith("## "):
                cur = line[3:].strip()
                sections[cur] = []
            elif cur is not None and line.strip():
                sections[cur].append(line)
    sections.update(_LOG)
    head = ("# Measured by tests/test_gpu_heads_blocks.py on an MI355X: per case and output the kernel's and stock torch fp32 CPU's largest\n"
            "# error against the float64 reference, relative to the output's largest magnitude (kernel / torch).\n"
            "# Bar: kernel <= max(16 x torch, 4 * 2^-24 = 2.4e-07).\n")
    try:
        with open(ERRORS_FILE, "w") as f:
            f.write(head)
            for name in sorted(sections):
                f.write(f"\n## {name}\n" + "\n".join(sections[name]) + "\n")
    except OSError:   # (a read-only checkout: the numbers are in the test output)
        pass


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _poison(*shape, dtype=F32):
    return torch.full(shape, KEEP_POISON if dtype == torch.uint8 else SENT, dtype=dtype, device="cuda")


def _host(t):
    return t.detach().cpu().numpy()


def _n64(v):
    return v.detach().numpy().astype(np.float64) if isinstance(v, torch.Tensor) else np.asarray(v, np.float64)


def _report(section, name, pairs):
    """pairs {output: (kernel array, float64 reference, torch fp32 array)}: logs kernel / torch errors, returns the outputs above the bar."""
    bad, parts = [], []
    for key, (got, ref, ref32) in pairs.items():
        ek, et = _rel(got, _n64(ref)), _rel(_n64(ref32), _n64(ref))
        parts.append(f"{key} {ek:.1e} / {et:.1e}")
        if not _bar(ek, et):
            bad.append(key)
    _log(section, f"{name}: " + ", ".join(parts) + ("  ABOVE THE BAR: " + " ".join(bad) if bad else ""))
    return bad


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def _generations_agree(name, a, b, keys, rows):
    """Two generations on the same inputs: 2e-6 relative on the finite rows; prints whether the bits were the same."""
    ident = True
    for key in keys:
        x, y = a[key][:len(rows)][rows], b[key][:len(rows)][rows]
        ident = ident and _same_bits(x, y)
        if x.dtype == np.float32:
            np.testing.assert_allclose(x, y, rtol=2e-6, atol=2e-6, err_msg=f"{name}: {key}")
        else:
            assert np.array_equal(x, y), f"{name}: {key}"
    print(f"{name}: bit-identical = {ident}")
    return ident


# ---------------------------------------------------------------------------------------------------------------------
# me_gather_class_boxes_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 300])
def test_gather_class_boxes_bit_for_bit(hip_lib, n):
    """Rows, order and total against the per-image loop's restatement: image counts of 0, max_det, in between and above max_det
    (clamped), 256-slot rounds on both sides of 256, more than 256 images (the strided count of the all-classes path), one class,
    every class and a class no row has; rows behind *total keep their poison."""
    from millieye_amd import hip
    lib = hip.lib()
    combos = [(0, 12), (1, 12), (12, 12), (12, 80), (1, 80), (0, 80)]   # (class_num, num_classes)
    i = 0
    for max_det in (1, 200, 256, 257, 600):
        r = np.random.RandomState(1000 * n + max_det)
        dets = {}
        for nc in (12, 80):
            det = r.randint(0, 1 << 20, (n, max_det, 7 + nc)).astype(np.float32)
            det[:, :, 6] = r.randint(0, 8, (n, max_det))   # classes 0 .. 7: class 11 is on no row
            dets[nc] = (det, _cu(det))
        kinds = r.randint(0, 4, n)
        kinds[:min(n, 4)] = [3, 1, 2, 0][:min(n, 4)]
        count = np.where(kinds == 0, 0, np.where(kinds == 1, max_det, np.where(kinds == 2, r.randint(0, max_det + 1, n), max_det + 5)))
        count_d = _cu(count.astype(np.int32))
        for class_idx in (-1, 0, 5, 11):
            class_num, nc = combos[i % len(combos)]
            i += 1
            det, det_d = dets[nc]
            want, total = R.gather_class_boxes(det, count, class_idx, class_num)
            cols = 8 + class_num
            boxes = _poison(n * max_det + 2, cols)
            tot_d = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            hip.check(lib.me_gather_class_boxes_f32(det_d.data_ptr(), count_d.data_ptr(), n, max_det, nc, class_idx, class_num,
                                                    boxes.data_ptr(), tot_d.data_ptr(), hip.stream_ptr()), "me_gather_class_boxes_f32")
            what = f"n {n} max_det {max_det} class_idx {class_idx} class_num {class_num} num_classes {nc}"
            assert int(tot_d.item()) == total, what
            got = _host(boxes)
            _bits_equal(got[:total], want, what)
            assert (got[total:] == SENT).all(), what + ": rows behind *total were written"
            assert class_idx != 11 or total == 0


# ---------------------------------------------------------------------------------------------------------------------
# stage-3 heads: one object per launch configuration
# ---------------------------------------------------------------------------------------------------------------------
class Stage3:
    """The device side of one case: maps, boxes, weights, poisoned outputs with PAD_ROWS rows behind the capacity, the descriptor."""

    def __init__(self, case, W, bin_major, radar_pitch, regress, thr_img=0.0, thr_radar=0.0, pool=True, train=False, save_feat=False):
        from millieye_amd import hip
        self.hip, self.case, self.train, self.pool, self.save_feat = hip, case, train, pool, save_feat
        n, fh, fw, rh, rw = (case[k] for k in ("n", "fh", "fw", "rh", "rw"))
        m490 = case["m490"].transpose(0, 2, 3, 1)
        if bin_major:
            q = np.arange(490)
            m490 = m490[..., (q % 10) * 49 + q // 10]
        img_pitch = 490 if bin_major else 496
        img = np.full((n, fh, fw, img_pitch), SENT, np.float32)
        img[..., :490] = m490
        rad = np.full((n, rh, rw, radar_pitch), SENT, np.float32)
        rad[..., :10] = case["m10"].transpose(0, 2, 3, 1)
        boxes = case["img_boxes"].copy()
        boxes[case["k_img"]:] = np.nan   # (rows behind *n_img are not to be read)
        self.k_img, self.k_rad, self.cap_img = case["k_img"], len(case["radar"]), case["cap_img"]
        self.k, self.cap = self.k_img + self.k_rad, self.cap_img + self.k_rad
        self.t = dict(img=_cu(img), rad=_cu(rad), boxes=_cu(boxes), n_img=_cu(np.array([self.k_img], np.int32)),
                      radar=_cu(case["radar"]) if self.k_rad else None)
        self.w = {k: _cu(np.asarray(v, np.float32)) for k, v in W.items()}
        self.w["w0t"] = _cu(np.asarray(W["w0"], np.float32).T.copy())
        d = hip.HeadsDesc()
        d.img_map, d.radar_map, d.img_pitch, d.radar_pitch, d.img_bin_major = self.t["img"].data_ptr(), self.t["rad"].data_ptr(), img_pitch, radar_pitch, bin_major
        d.n, d.fh, d.fw, d.rh, d.rw, d.spatial_scale = n, fh, fw, rh, rw, HC.SCALE
        d.img_boxes, d.n_img, d.n_img_cap, d.box_cols = self.t["boxes"].data_ptr(), self.t["n_img"].data_ptr(), self.cap_img, case["cols"]
        d.radar_boxes, d.n_radar = (self.t["radar"].data_ptr() if self.k_rad else None), self.k_rad
        d.thr_img, d.thr_radar, d.regress = thr_img, thr_radar, regress
        for nm in ("w0t", "b0", "w1", "b1", "w2", "b2", "rw", "rscale", "rshift", "rw2", "rb2", "e1w", "e1b", "e2w", "e2b"):
            setattr(d.wts, nm, self.w[nm].data_ptr())
        if train:
            d.wts.rb = self.w["rb"].data_ptr()
        self.d = d
        self.fresh_outputs()

    def fresh_outputs(self):
        rows, d = self.cap + PAD_ROWS, self.d
        o = dict(regress=_poison(rows, 4), refine=_poison(rows, 2), mask1=_poison(rows), out_rows=_poison(rows, 8), sort_key=_poison(rows),
                 keep=_poison(rows, dtype=torch.uint8))
        d.regress_out, d.refine_out, d.mask1_out = o["regress"].data_ptr(), o["refine"].data_ptr(), o["mask1"].data_ptr()
        d.out_rows, d.keep, d.sort_key = o["out_rows"].data_ptr(), o["keep"].data_ptr(), o["sort_key"].data_ptr()
        if self.pool:
            o["pooled"] = _poison(rows, 980)
            d.pool_scratch = o["pooled"].data_ptr()
        if self.train:
            o["small"], o["hidden"] = _poison(rows, 16), _poison(rows, 256)
            d.save_small, d.save_hidden = o["small"].data_ptr(), o["hidden"].data_ptr()
        if self.save_feat:
            o["feat_img"], o["feat_rad"] = _poison(rows, 490), _poison(rows, 490)
            d.save_feat_img, d.save_feat_rad = o["feat_img"].data_ptr(), o["feat_rad"].data_ptr()
        self.o = o
        return o

    def launch(self):
        self.hip.check(self.hip.lib().me_roi_heads_f32(C.byref(self.d), self.hip.stream_ptr()), "me_roi_heads_f32")
        torch.cuda.synchronize()
        return {k: _host(v) for k, v in self.o.items()}

    def tail(self, small, k):
        self.hip.check(self.hip.lib().me_heads_tail_f32(C.byref(self.d), small.data_ptr(), k, self.hip.stream_ptr()), "me_heads_tail_f32")
        torch.cuda.synchronize()
        return {k_: _host(v) for k_, v in self.o.items()}


TAIL_KEYS = ("regress", "refine", "mask1", "out_rows", "sort_key")


def _slots_behind_untouched(out, k, cap, keys=TAIL_KEYS, what=""):
    """Behind the last RoI: keep == 0 up to the capacity (the launch clears it), everything else still poisoned."""
    assert (out["keep"][k:cap] == 0).all(), what + ": keep behind the last RoI"
    assert (out["keep"][cap:] == KEEP_POISON).all(), what + ": keep behind the capacity"
    for key in keys:
        assert (out[key][k:] == SENT).all(), f"{what}: {key} was written behind the last RoI"


def _check_inference(out, ref, ref32, k, cap, section, name):
    """regress, refine, mask1, out_rows, sort_key against float64 under the bar (rows that are finite in the reference: a zero-area
    or inverted PS-RoI is NaN on both sides); keep == (p > thr) outside rounding distance; the slots behind the last RoI."""
    ok = np.isfinite(_n64(ref["mask1"])) & np.isfinite(_n64(ref["out_rows"])).all(1)
    assert ok.sum() >= k - 4
    pairs = {key: (out[key][:k][ok], _n64(ref[key])[ok], _n64(ref32[key])[ok]) for key in ("regress", "refine", "mask1", "sort_key")}
    rows, rr, r32 = out["out_rows"][:k][ok], _n64(ref["out_rows"])[ok], _n64(ref32["out_rows"])[ok]
    assert np.array_equal(rows[:, 0], rr[:, 0]), name + ": image index"
    assert np.array_equal(rows[:, 7], rr[:, 7]), name + ": c7 (the proposal's class id, never 0, on image rows; 0 on radar rows)"
    pairs["box"] = (rows[:, 1:5], rr[:, 1:5], r32[:, 1:5])
    pairs["p,c6"] = (rows[:, 5:7], rr[:, 5:7], r32[:, 5:7])
    bad = _report(section, name, pairs)
    near = R.near_zero(_n64(ref["keep_margin"]), _n64(ref["keep_terms"])) & ok
    assert near.sum() <= 0.01 * k, name + ": too many rows at rounding distance from the threshold"
    sure = ok & ~near
    assert np.array_equal(out["keep"][:k][sure], _n64(ref["keep"])[sure].astype(np.uint8)), name + ": keep"
    assert (out["keep"][:k][~ok] == 0).all(), name + ": a NaN row was kept"
    _slots_behind_untouched(out, k, cap, what=name)
    return bad, ok


def _real_setup(name, spec=None):
    args, bin_major, pitch, regress = spec or HC.REAL_CASES[name]
    case = HC.real_case(*args)
    W = HC.real_weights(name)
    fi, fr = HC.tv_pooled(case)
    ref = HC.stage3_reference(case, W, fi, fr, regress)
    ref32 = HC.stage3_reference(case, W, fi, fr, regress, dtype=torch.float32)
    return case, W, bin_major, pitch, regress, fi, fr, ref, ref32


def _pooled_is_tv_ops(out, fi, fr, k, what):
    got_i, got_r = (out["pooled"][:k, :490], out["pooled"][:k, 490:]) if "pooled" in out else (out["feat_img"][:k], out["feat_rad"][:k])
    assert _same_bits(got_i, fi), what + ": image-branch pooled features differ from tv_ops.ps_roi_align"
    assert _same_bits(got_r, fr), what + ": radar-branch pooled features differ from tv_ops.roi_align"


_REAL_CACHE = {}


def _real(name):
    if name not in _REAL_CACHE:
        _REAL_CACHE[name] = _real_setup(name)
    return _REAL_CACHE[name]


@pytest.mark.parametrize("name", ["a", "b"])
def test_stage3_heads_real_inputs_two_launch_and_fused(hip_lib, name):
    """The default path (roi_pool10_kernel + roi_heads_mfma_kernel) and the single fused launch at a small capacity
    (roi_heads_kernel<32>): each against float64, against each other, pooled features bit-identical with oracle/tv_ops (the fused
    launch's through its training-mode feature saves).  Case a: bin-major map, radar pitch 12, regress on, 9 box columns; case b:
    reference channel order on a pitched map, radar map of another size at pitch 10, regress off, 12 box columns."""
    case, W, bin_major, pitch, regress, fi, fr, ref, ref32 = _real(name)
    common = dict(thr_img=ref["thr_img"], thr_radar=ref["thr_radar"])
    outs, bad = {}, []
    for gen, pool in (("two-launch", True), ("fused<32>", False)):
        s = Stage3(case, W, bin_major, pitch, regress, pool=pool, **common)
        outs[gen] = s.launch()
        b, ok = _check_inference(outs[gen], ref, ref32, s.k, s.cap, "stage-3 heads, real inputs", f"case {name} {gen}")
        bad += [f"{gen}: {v}" for v in b]
        if pool:
            _pooled_is_tv_ops(outs[gen], fi, fr, s.k, gen)
            assert (outs[gen]["pooled"][s.k:] == SENT).all(), "pool_scratch behind the last RoI"
    _generations_agree(f"case {name}: two-launch vs fused<32>", outs["two-launch"], outs["fused<32>"], TAIL_KEYS + ("keep",), ok)
    s = Stage3(case, W, bin_major, pitch, regress, pool=False, train=True, save_feat=True)
    _pooled_is_tv_ops(s.launch(), fi, fr, s.k, "fused<32> feature saves")
    assert not bad, bad


def test_stage3_heads_real_inputs_513_workgroups(hip_lib):
    """pool_scratch = NULL with 4104 RoI slots = 513 workgroups: the launcher's switch to roi_heads_kernel<4> (above 512).  Against
    float64, against the default path on the same inputs; the pooled features through the feature saves."""
    case, W, bin_major, pitch, regress, fi, fr, ref, ref32 = _real_setup("big", HC.BIG_CASE)
    common = dict(thr_img=ref["thr_img"], thr_radar=ref["thr_radar"])
    s = Stage3(case, W, bin_major, pitch, regress, pool=False, **common)
    assert (s.cap + 7) // 8 == 513
    fused = s.launch()
    bad, ok = _check_inference(fused, ref, ref32, s.k, s.cap, "stage-3 heads, real inputs", "4104 slots fused<4>")
    s2 = Stage3(case, W, bin_major, pitch, regress, pool=True, **common)
    split = s2.launch()
    bad2, _ = _check_inference(split, ref, ref32, s2.k, s2.cap, "stage-3 heads, real inputs", "4104 slots two-launch")
    _pooled_is_tv_ops(split, fi, fr, s2.k, "two-launch")
    _generations_agree("4104 slots: two-launch vs fused<4>", split, fused, TAIL_KEYS + ("keep",), ok)
    s3 = Stage3(case, W, bin_major, pitch, regress, pool=False, train=True, save_feat=True)
    _pooled_is_tv_ops(s3.launch(), fi, fr, s3.k, "fused<4> feature saves")
    assert not bad + bad2, bad + bad2


CHILD_ENVS = {"pool": {"MILLIEYE_POOL10": "0"}, "valu": {"MILLIEYE_HEADS_MFMA": "0"}}


def _child(which, out_path):
    """Runs in a fresh process whose environment selects a kernel generation (the variables are read once per process): the two
    REAL cases through me_roi_heads_f32 with pool_scratch, outputs to an .npz."""
    for key, val in CHILD_ENVS[which].items():
        assert os.environ.get(key) == val
    from millieye_amd import hip
    hip.load()
    res = {}
    for name in ("a", "b"):
        case, W, bin_major, pitch, regress, _fi, _fr, ref, _ref32 = _real_setup(name)
        s = Stage3(case, W, bin_major, pitch, regress, pool=True, thr_img=ref["thr_img"], thr_radar=ref["thr_radar"])
        for key, v in s.launch().items():
            res[f"{name}/{key}"] = v
    np.savez(out_path, **res)


@pytest.mark.parametrize("which", ["pool", "valu"])
def test_stage3_generations_behind_environment_switches(hip_lib, tmp_path, which):
    """MILLIEYE_POOL10=0 (roi_pool_kernel: a thread per pooled value) and MILLIEYE_HEADS_MFMA=0 (the VALU heads behind the pooling
    launch), each in a fresh child process: against float64 under the bar, pooled features bit-identical with oracle/tv_ops, and
    against the default path of this process."""
    path = str(tmp_path / f"{which}.npz")
    env = dict(os.environ, **CHILD_ENVS[which])
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), which, path], cwd=ROOT, env=env, timeout=240,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert proc.returncode == 0, proc.stdout.decode(errors="replace")[-4000:]
    got = np.load(path)
    bad = []
    for name in ("a", "b"):
        case, W, bin_major, pitch, regress, fi, fr, ref, ref32 = _real(name)
        out = {key.split("/")[1]: got[key] for key in got.files if key.startswith(name + "/")}
        k, cap = case["k_img"] + len(case["radar"]), case["cap_img"] + len(case["radar"])
        b, ok = _check_inference(out, ref, ref32, k, cap, "stage-3 heads, real inputs", f"case {name} {' '.join(f'{a}={v}' for a, v in CHILD_ENVS[which].items())}")
        bad += b
        _pooled_is_tv_ops(out, fi, fr, k, which)
        mine = Stage3(case, W, bin_major, pitch, regress, pool=True, thr_img=ref["thr_img"], thr_radar=ref["thr_radar"]).launch()
        _generations_agree(f"case {name}: default vs {which}", mine, out, TAIL_KEYS + ("keep", "pooled"), ok)
    assert not bad, bad


@pytest.mark.parametrize("idx", range(len(HC.EXACT_CASES)))
def test_stage3_front_end_exact_inputs_bit_for_bit(hip_lib, idx):
    """Training mode (the launch stops before any transcendental) on EXACT inputs, k = 1, 7, 8, 9, 31, 32, 33, 65 RoIs split between
    image proposals and 0 / 1 / 5 radar boxes, n_img_cap > *n_img, both channel orders, radar pitch 10 / 12, radar maps of another
    size: the pooling launch + roi_heads_mfma_kernel and the fused roi_heads_kernel<32> with its feature saves.
    pooled features, save_small and the non-negative part of save_hidden equal float64 bit for bit, the negative part of save_hidden
    equals the reference rounded once to fp32.  With the lifted b0 (hidden vector positive) that is all of save_small; with both
    LeakyReLU branches live, net1 / net2 sum fp32-rounded slope products: those six columns are held to the dot-product bound
    256 * 2^-24 * sum |w| |h| against float64 of the rounded hidden vector (the radar columns stay bit-exact)."""
    args = HC.EXACT_CASES[idx]
    case = HC.exact_case(idx, *args[:9])
    bin_major, pitch = args[9], args[10]
    nhwc = lambda m: m.transpose(0, 2, 3, 1)  # noqa: E731
    rois = HC.all_rois(case)
    fi, fr = R.ps_roi_align(nhwc(case["m490"]), rois, HC.SCALE), R.roi_align(nhwc(case["m10"]), rois, HC.SCALE)
    for positive in (True, False):
        W = HC.exact_weights(100 + idx, positive)
        f = R.frontend(fi, fr, W, rb=W["rb"])
        hid, small = f["hidden"].numpy(), f["small"].numpy()
        for form, pool in (("mfma", True), ("fused", False)):
            s = Stage3(case, W, bin_major, pitch, 1, pool=pool, train=True, save_feat=not pool)
            out = s.launch()
            k, what = s.k, f"exact case {idx} {form} positive {positive}"
            got_i, got_r = (out["pooled"][:k, :490], out["pooled"][:k, 490:]) if pool else (out["feat_img"][:k], out["feat_rad"][:k])
            _bits_equal(got_i, fi, what + " image features")
            _bits_equal(got_r, fr, what + " radar features")
            _bits_equal(out["hidden"][:k], hid.astype(np.float32), what + " save_hidden (the negative part rounded once)")
            _bits_equal(out["hidden"][:k][hid >= 0], hid[hid >= 0], what + " save_hidden, non-negative part")
            _bits_equal(out["small"][:k, 6:], small[:, 6:], what + " save_small radar conv")
            if positive:
                _bits_equal(out["small"][:k], small, what + " save_small")
            else:
                h32 = hid.astype(np.float32).astype(np.float64)
                w12 = np.concatenate((W["w1"], W["w2"][:2])).astype(np.float64)
                want = h32 @ w12.T + np.concatenate((W["b1"], W["b2"][:2]))
                bound = 256 * U * (np.abs(h32) @ np.abs(w12).T + 4)
                assert (np.abs(out["small"][:k, :6] - want) <= bound).all(), what + " save_small net1 / net2"
            _slots_behind_untouched(out, k, s.cap, keys=("small", "hidden") + (("pooled",) if pool else ("feat_img", "feat_rad")), what=what)
            for key in TAIL_KEYS:   # (the tail runs separately in training mode)
                assert (out[key] == SENT).all(), what + f": {key} written in training mode"


@pytest.mark.parametrize("k", HC.TAIL_KS)
def test_heads_tail_equals_the_fused_tail_and_float64(hip_lib, k):
    """me_heads_tail_f32 on the save_small block of a training-mode launch (conv bias 0, so that it is the inference launch's own
    small): the same bits as the outputs of both inference launches, whose kernels end in the same tail_one - the default pooling
    launch + roi_heads_mfma_kernel, and the fused roi_heads_kernel<32> (pool_scratch = NULL), whose own training-mode save_small is
    run through the tail as well - and, from that fp32 block, float64 under the bar."""
    case, W = HC.tail_real_case(k)
    fi, fr = HC.tv_pooled(case)
    ref0 = HC.stage3_reference(case, W, fi, fr, 1)
    thr = dict(thr_img=ref0["thr_img"], thr_radar=ref0["thr_radar"])
    for form, pool in (("roi_heads_kernel<32>", False), ("roi_pool10_kernel + roi_heads_mfma_kernel", True)):
        inf = Stage3(case, W, 1, 10, 1, pool=pool, **thr).launch()
        tr = Stage3(case, W, 1, 10, 1, pool=pool, train=True, save_feat=not pool)
        small = tr.launch()["small"][:k]
        s = Stage3(case, W, 1, 10, 1, pool=False, **thr)
        out = s.tail(_cu(small), k)
        for key in TAIL_KEYS + ("keep",):
            assert _same_bits(out[key][:k], inf[key][:k]), f"k {k}: {key} differs from the tail of {form}"
    rois = HC.all_rois(case)
    ref = R.tail(small, rois, case["img_boxes"], case["k_img"], W, thr["thr_img"], thr["thr_radar"], 1)
    ref32 = R.tail(small, rois, case["img_boxes"], case["k_img"], W, thr["thr_img"], thr["thr_radar"], 1, dtype=torch.float32)
    assert (out["keep"][k:] == KEEP_POISON).all(), "me_heads_tail_f32 writes k rows only"
    out["keep"][k:s.cap] = 0   # (what _check_inference expects of a launch that clears the slots)
    bad, _ok = _check_inference(out, ref, ref32, k, s.cap, "heads_tail", f"k {k}")
    assert not bad, bad


def test_heads_loss_vs_float64_and_the_bce_clamps(hip_lib):
    """All eight (label_pos, in_focal, in_conf) combinations over a 40 x 40 sweep of p and x in [1e-6, 1 - 1e-6] in one call, alpha and
    conf_lambda off their defaults: terms and seeds under the bar; exactly 0 where a row is in neither sum.  Then x in {0, 1} against
    torch fp32 BCELoss forward and backward on the CPU: the -100 log clamp and the 1e-12 denominator clamp, bit for bit."""
    from millieye_amd import hip
    lib = hip.lib()
    c = HC.loss_case()
    k = c["k"]
    alpha, lam = float(np.float32(c["alpha"])), float(np.float32(c["lam"]))

    def call(mask1, conf, pos, foc, cnf, n):
        terms, sp, sc = _poison(n + PAD_ROWS, 2), _poison(n + PAD_ROWS), _poison(n + PAD_ROWS)
        ins = [_cu(v) for v in (mask1, np.stack((conf, 0 * conf), 1), pos, foc, cnf)]   # (kept alive over the call)
        hip.check(lib.me_heads_loss_f32(*[v.data_ptr() for v in ins], n, alpha, lam, terms.data_ptr(), sp.data_ptr(), sc.data_ptr(),
                                        hip.stream_ptr()), "me_heads_loss_f32")
        got = dict(terms=_host(terms), seed_p=_host(sp), seed_conf=_host(sc))
        assert all((v[n:] == SENT).all() for v in got.values()), "written behind k"
        return {key: v[:n] for key, v in got.items()}

    got = call(c["mask1"], c["conf"], c["label_pos"], c["in_focal"], c["in_conf"], k)
    a = (c["mask1"], c["conf"], c["label_pos"], c["in_focal"], c["in_conf"], alpha, lam)
    ref, ref32 = R.heads_loss(*a), R.heads_loss(*a, dtype=torch.float32)
    pairs = {"focal": (got["terms"][:, 0], ref["terms"][:, 0], ref32["terms"][:, 0]), "bce": (got["terms"][:, 1], ref["terms"][:, 1], ref32["terms"][:, 1]),
             "seed_p": (got["seed_p"], ref["seed_p"], ref32["seed_p"]), "seed_conf": (got["seed_conf"], ref["seed_conf"], ref32["seed_conf"])}
    bad = _report("heads_loss", f"sweep, k {k}", pairs)
    # the sweep's largest seeds (1 / p at p = 1e-6) hide the middle of the range: the same bar on the rows with p, x in [0.01, 0.99]
    mid = (c["mask1"] > 0.01) & (c["mask1"] < 0.99) & (c["conf"] > 0.01) & (c["conf"] < 0.99)
    bad += _report("heads_loss", "sweep, p and x in [0.01, 0.99]", {key: tuple(_n64(v)[mid] for v in trip) for key, trip in pairs.items()})
    foc, cnf = c["in_focal"] == 0, c["in_conf"] == 0
    assert (got["terms"][foc, 0] == 0).all() and (got["seed_p"][foc] == 0).all() and (got["terms"][cnf, 1] == 0).all() and (got["seed_conf"][cnf] == 0).all()
    assert not bad, bad
    # the clamps
    x, y = HC.bce_endpoints()
    one = np.ones(len(x), np.uint8)
    got = call(np.full(len(x), 0.5, np.float32), x, y, 0 * one, one, len(x))
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    loss = F.binary_cross_entropy(xt, torch.from_numpy(y.astype(np.float32)), reduction="none")
    loss.sum().backward()
    want_l = loss.detach().numpy() / np.float32(lam)
    want_g = xt.grad.numpy() / np.float32(lam)
    ends = (x == 0) | (x == 1)
    assert np.array_equal(got["terms"][ends, 1], want_l[ends]), (got["terms"][ends, 1], want_l[ends])
    assert np.array_equal(got["seed_conf"][ends], want_g[ends]), (got["seed_conf"][ends], want_g[ends])
    assert np.abs(got["seed_conf"][ends]).max() > 1e11 and got["terms"][ends, 1].max() == np.float32(100) / np.float32(lam)
    # the two ordinary rows of that call: float64 under the bar, like the sweep
    a = (np.full(len(x), 0.5, np.float32)[~ends], x[~ends], y[~ends], 0 * one[~ends], one[~ends], alpha, lam)
    ref, ref32 = R.heads_loss(*a), R.heads_loss(*a, dtype=torch.float32)
    bad = _report("heads_loss", "the ordinary rows beside the BCE endpoints", {
        "bce": (got["terms"][~ends, 1], ref["terms"][:, 1], ref32["terms"][:, 1]), "seed_conf": (got["seed_conf"][~ends], ref["seed_conf"], ref32["seed_conf"])})
    assert not bad, bad


BWD_KEYS = (("g_o", 2), ("g_hpre", 64), ("h_act", 64), ("xin", 4), ("g_z2", 2), ("g_rl", 10), ("rl", 10), ("g_rlogit", 1))


def test_heads_tail_bwd_vs_float64_and_the_device_row_count(hip_lib):
    """me_heads_tail_bwd_f32: all eight outputs under the bar, zeros for the radar rows of g_hpre / h_act / xin; the elements whose fc1
    pre-activation lies at rounding distance from 0 (and, for the outputs behind the ensemble head's input gradient, their rows)
    are left out.  me_heads_tail_bwd_dev_f32 with *k_dev in {0, 1, k - 1, k}: the plain call's bits in front of *k_dev, zeros behind,
    the sentinel behind the capacity."""
    from millieye_amd import hip
    lib = hip.lib()
    k, n_img = HC.BWD_CASE
    c = HC.tail_case(k, n_img)
    W = HC.real_weights("tail")
    t = R.tail(c["small"], c["rois"], c["img_boxes"], n_img, W, 0.0, 0.0, 1)
    refine, mask1 = t["refine"].numpy().astype(np.float32), t["mask1"].numpy().astype(np.float32)
    seed_p, seed_c = (HC.synth.normal(f"hb/bwd{j}", (k,), 0, 2.0) for j in (0, 1))
    s = Stage3(dict(HC.real_case("bwd", n_img, n_img, k - n_img, 2, 13, 13, 13, 13, 9), img_boxes=c["img_boxes"], radar=c["radar"]), W, 1, 10, 1)
    ins = [_cu(v) for v in (c["small"], refine, mask1, seed_p, seed_c)]

    def call(k_dev=None):
        outs = {key: _poison(k + PAD_ROWS, cols) for key, cols in BWD_KEYS}
        ptrs = [outs[key].data_ptr() for key, _ in BWD_KEYS]
        if k_dev is None:
            hip.check(lib.me_heads_tail_bwd_f32(C.byref(s.d), *[v.data_ptr() for v in ins], k, *ptrs, hip.stream_ptr()), "me_heads_tail_bwd_f32")
        else:
            kd = _cu(np.array([k_dev], np.int32))
            hip.check(lib.me_heads_tail_bwd_dev_f32(C.byref(s.d), *[v.data_ptr() for v in ins], k, kd.data_ptr(), *ptrs, hip.stream_ptr()),
                      "me_heads_tail_bwd_dev_f32")
        got = {key: _host(v) for key, v in outs.items()}
        assert all((v[k:] == SENT).all() for v in got.values()), "written behind the capacity"
        return {key: v[:k] for key, v in got.items()}

    got = call()
    a = (c["small"], refine, mask1, seed_p, seed_c, c["img_boxes"], n_img, W)
    ref, ref32 = R.tail_bwd(*a), R.tail_bwd(*a, dtype=torch.float32)
    near = np.zeros((k, 64), bool)
    near[:n_img] = R.near_zero(ref["pre"].numpy(), ref["pre_terms"].numpy())
    assert near.mean() <= 0.01
    row_ok = ~near.any(1)
    pairs = {}
    for key, cols in BWD_KEYS:
        g, r64, r32 = got[key].reshape(k, cols), _n64(ref[key]).reshape(k, cols), _n64(ref32[key]).reshape(k, cols)
        sel = ~near if key == "g_hpre" else (row_ok if key in ("g_z2", "g_rl", "g_rlogit") else np.ones(k, bool))
        pairs[key] = (g[sel], r64[sel], r32[sel])
    bad = _report("heads_tail_bwd", f"k {k}, {n_img} image rows", pairs)
    for key in ("g_hpre", "h_act", "xin", "g_o"):
        assert (got[key][n_img:] == 0).all(), f"{key}: radar rows must be zero"
    assert np.abs(got["g_rl"][n_img:]).max() > 0
    assert not bad, bad
    for k_dev in (0, 1, k - 1, k):
        dev = call(k_dev)
        for key, _cols in BWD_KEYS:
            assert _same_bits(dev[key][:k_dev], got[key][:k_dev]), f"*k_dev {k_dev}: {key} differs from the plain call"
            assert (dev[key][k_dev:] == 0).all(), f"*k_dev {k_dev}: {key} is not zero behind the live rows"


# ---------------------------------------------------------------------------------------------------------------------
# stage 2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("class_num", [1, 12, 15])
def test_m2_heads_vs_float64(hip_lib, class_num):
    """me_m2_heads_f32 for 1, 12 and 15 classes (16 is refused: class_num + 1 <= 16), boxes_cap 9 / 24 with *n_boxes in
    {0, 1, 8, 9, boxes_cap}, three more box columns than 8 + class_num, with pool_scratch and with NULL (the same bits).  The live
    rows of every run with *n_boxes >= 1 are compared with float64 under the bar (the first row is finite in every case, so the
    one-row run compares it), and are the bits of the same rows of the *n_boxes = boxes_cap run.
    CONTRACT: the kernels write the rows in front of *n_boxes only - every output row behind it, keep included, keeps what the
    caller put there (unlike me_roi_heads_f32, which clears keep up to its capacity)."""
    from millieye_amd import hip
    from oracle import tv_ops
    lib = hip.lib()
    c1, cols = class_num + 1, 8 + class_num + 3
    W = HC.real_weights(f"m2h{class_num}", c2=c1, slots=c1)
    wd = {k: _cu(np.asarray(v, np.float32)) for k, v in W.items()}
    wd["w0t"] = _cu(W["w0"].T.copy())
    hw = hip.HeadsWeights()
    for nm in ("w0t", "b0", "w1", "b1", "w2", "b2", "e1w", "e1b", "e2w", "e2b"):
        setattr(hw, nm, wd[nm].data_ptr())
    keys = (("regress", 4), ("refine", c1), ("mask", 1), ("out_rows", 8), ("sort_key", 1))
    bad = []
    for cap in (9, 24):
        c = HC.m2_case(f"{class_num}_{cap}", cap, class_num, cols)   # (tests/test_heads_refs_cpu.py builds the same cases)
        pitch = 493
        img = np.full((c["n"], c["fh"], c["fw"], pitch), SENT, np.float32)
        img[..., :490] = c["m490"].transpose(0, 2, 3, 1)
        img_d, boxes_d = _cu(img), _cu(c["boxes"])
        feat = tv_ops.ps_roi_align(torch.from_numpy(c["m490"]), torch.from_numpy(c["boxes"][:, :5].copy()), (7, 7),
                                   spatial_scale=HC.SCALE).reshape(cap, 490).numpy()
        ref0 = R.m2_heads(feat, c["boxes"], class_num, W, 0.0)
        thr = HC.pick_threshold(ref0["mask"].numpy())
        ref, ref32 = R.m2_heads(feat, c["boxes"], class_num, W, thr), R.m2_heads(feat, c["boxes"], class_num, W, thr, dtype=torch.float32)
        ok_all = np.isfinite(_n64(ref["mask"]))
        assert ok_all.sum() >= cap - 2 and thr > 0
        full = None
        for nb in sorted({0, 1, 8, 9, cap}, reverse=True):   # (boxes_cap first: the shorter runs are compared with its rows)
            nb_d = _cu(np.array([nb], np.int32))
            res = {}
            for pool in (True, False):
                o = {key: _poison(cap + PAD_ROWS, w) for key, w in keys}
                o["keep"] = _poison(cap + PAD_ROWS, dtype=torch.uint8)
                scratch = _poison(cap + PAD_ROWS, 490) if pool else None
                hip.check(lib.me_m2_heads_f32(img_d.data_ptr(), pitch, c["n"], c["fh"], c["fw"], HC.SCALE, boxes_d.data_ptr(), nb_d.data_ptr(), cap,
                                              cols, class_num, C.byref(hw), thr, o["regress"].data_ptr(), o["refine"].data_ptr(), o["mask"].data_ptr(),
                                              o["out_rows"].data_ptr(), o["keep"].data_ptr(), o["sort_key"].data_ptr(),
                                              scratch.data_ptr() if pool else None, hip.stream_ptr()), "me_m2_heads_f32")
                res[pool] = {key: _host(v) for key, v in o.items()}
                if pool:
                    got_pool = _host(scratch)
                    assert _same_bits(got_pool[:nb], feat[:nb]) and (got_pool[nb:] == SENT).all(), "pool_scratch"
            for key in res[True]:
                assert _same_bits(res[True][key], res[False][key]), f"class_num {class_num} cap {cap} n_boxes {nb}: {key} with / without pool_scratch"
            out, ok = res[True], ok_all[:nb]
            for key, _w in keys:
                assert (out[key][nb:] == SENT).all(), f"{key}: a row behind *n_boxes was written"
            assert (out["keep"][nb:] == KEEP_POISON).all(), "keep: a row behind *n_boxes was written"
            full = full or out
            for key in out:   # (a row depends on no other row, and the inputs are the same)
                assert _same_bits(out[key][:nb], full[key][:nb]), f"class_num {class_num} cap {cap} n_boxes {nb}: {key} differs from the n_boxes = {cap} run"
            if nb == 0:
                continue
            assert ok[0], "the first row is compared in every run"
            pairs = {key: (out[key][:nb].reshape(nb, -1)[ok], _n64(ref[key])[:nb].reshape(nb, -1)[ok], _n64(ref32[key])[:nb].reshape(nb, -1)[ok])
                     for key in ("regress", "refine", "mask", "sort_key")}
            rows, rr, r32 = out["out_rows"][:nb][ok], _n64(ref["out_rows"])[:nb][ok], _n64(ref32["out_rows"])[:nb][ok]
            assert np.array_equal(rows[:, 0], rr[:, 0]) and np.array_equal(rows[:, 6:8], rr[:, 6:8])
            pairs["box"] = (rows[:, 1:5], rr[:, 1:5], r32[:, 1:5])
            pairs["p"] = (rows[:, 5], rr[:, 5], r32[:, 5])
            bad += _report("m2_heads", f"class_num {class_num} boxes_cap {cap} n_boxes {nb}", pairs)
            near = R.near_zero(_n64(ref["keep_margin"])[:nb], _n64(ref["keep_terms"])[:nb]) & ok
            assert near.sum() <= 0.01 * nb
            sure = ok & ~near
            assert np.array_equal(out["keep"][:nb][sure], _n64(ref["keep"])[:nb][sure].astype(np.uint8)), "keep"
            assert nb < cap or 0 < out["keep"][:nb][sure].sum() < sure.sum()
    rc = lib.me_m2_heads_f32(img_d.data_ptr(), pitch, c["n"], c["fh"], c["fw"], HC.SCALE, boxes_d.data_ptr(), nb_d.data_ptr(), cap, 8 + 16, 16,
                             C.byref(hw), thr, *[o[key].data_ptr() for key in ("regress", "refine", "mask", "out_rows", "keep", "sort_key")], None,
                             hip.stream_ptr())
    assert rc == -1, "class_num = 16 must return ME_E_BADARG"
    assert not bad, bad


@pytest.mark.parametrize("k,c1", HC.M2_ROWS_CASES)
def test_m2_pairs_bit_for_bit_and_rows_vs_float64(hip_lib, k, c1):
    from millieye_amd import hip
    lib = hip.lib()
    c = HC.m2_rows_case(k, c1)
    cols, boxes, refine, o, reg = c["cols"], c["boxes"], c["refine"], c["o"], c["regress"]
    x2 = _poison(k * c1 + PAD_ROWS, 2)
    boxes_d, refine_d = _cu(boxes), _cu(refine)
    hip.check(lib.me_m2_pairs_f32(refine_d.data_ptr(), boxes_d.data_ptr(), cols, k, c1, x2.data_ptr(), hip.stream_ptr()), "me_m2_pairs_f32")
    got = _host(x2)
    _bits_equal(got[:k * c1], R.m2_pairs(refine, boxes), "pairs")
    assert (got[k * c1:] == SENT).all()
    thr = HC.pick_threshold(R.m2_rows(o, reg, boxes, 0.0)["key"].numpy())
    ref, ref32 = R.m2_rows(o, reg, boxes, thr), R.m2_rows(o, reg, boxes, thr, dtype=torch.float32)
    masks, rows, key, keep = _poison(k + PAD_ROWS, 2), _poison(k + PAD_ROWS, 8), _poison(k + PAD_ROWS), _poison(k + PAD_ROWS, dtype=torch.uint8)
    o_d, reg_d = _cu(o), _cu(reg)
    hip.check(lib.me_m2_rows_f32(o_d.data_ptr(), reg_d.data_ptr(), boxes_d.data_ptr(), cols, k, thr, masks.data_ptr(), rows.data_ptr(),
                                 keep.data_ptr(), key.data_ptr(), hip.stream_ptr()), "me_m2_rows_f32")
    gm, gr, gk, gp = _host(masks), _host(rows), _host(key), _host(keep)
    assert (gm[k:] == SENT).all() and (gr[k:] == SENT).all() and (gk[k:] == SENT).all() and (gp[k:] == KEEP_POISON).all()
    rr, r32 = _n64(ref["rows"]), _n64(ref32["rows"])
    assert np.array_equal(gr[:k, 0], rr[:, 0]) and np.array_equal(gr[:k, 6:8], rr[:, 6:8])
    bad = _report("m2_rows", f"k {k}", {"masks": (gm[:k], ref["masks"], ref32["masks"]), "box": (gr[:k, 1:5], rr[:, 1:5], r32[:, 1:5]),
                                        "p": (gr[:k, 5], rr[:, 5], r32[:, 5]), "key": (gk[:k], ref["key"], ref32["key"])})
    near = R.near_zero(_n64(ref["keep_margin"]), _n64(ref["keep_terms"]))
    assert near.sum() <= 0.01 * k
    assert np.array_equal(gp[:k][~near], _n64(ref["keep"])[~near].astype(np.uint8))
    assert not bad, bad


@pytest.mark.parametrize("c1", [2, 13])
def test_m2_loss_vs_float64_and_the_bce_clamps(hip_lib, c1):
    """One call: pos x sample in all four combinations, SmoothL1 residuals on both sides of 1, grad_scale, lambda0, lambda1 and alpha
    off their defaults - terms and the three gradients under the bar over the ordinary rows; the last eight rows hold refine in
    {0, 1} against both labels and are asserted against torch fp32 BCELoss forward and backward on the CPU, bit for bit."""
    from millieye_amd import hip
    lib = hip.lib()
    c = HC.m2_loss_case(c1)
    k, ends = c["k"], c["ends"]
    alpha, l0, l1, gs = (float(np.float32(c[key])) for key in ("alpha", "lambda0", "lambda1", "grad_scale"))
    cols = c["boxes"].shape[1]
    terms, d_o, d_r, d_g = _poison(k + PAD_ROWS, 5), _poison(k + PAD_ROWS, 2), _poison(k + PAD_ROWS, c1), _poison(k + PAD_ROWS, 4)
    dv = {key: _cu(c[key]) for key in ("o", "refine", "regress", "boxes", "tloc", "clabel", "pos", "sample")}   # (kept alive over the call)
    hip.check(lib.me_m2_loss_f32(dv["o"].data_ptr(), dv["refine"].data_ptr(), c1, dv["regress"].data_ptr(), dv["boxes"].data_ptr(), cols,
                                 *[dv[key].data_ptr() for key in ("tloc", "clabel", "pos", "sample")], k, alpha, l0, l1, gs, terms.data_ptr(),
                                 d_o.data_ptr(), d_r.data_ptr(), d_g.data_ptr(), hip.stream_ptr()), "me_m2_loss_f32")
    got = dict(terms=_host(terms), d_o=_host(d_o), d_refine=_host(d_r), d_regress=_host(d_g))
    assert all((v[k:] == SENT).all() for v in got.values()), "written behind k"
    a = (c["o"], c["refine"], c["regress"], c["boxes"], c["tloc"], c["clabel"], c["pos"], c["sample"], alpha, l0, l1, gs)
    ref, ref32 = R.m2_loss(*a), R.m2_loss(*a, dtype=torch.float32)
    body = np.ones(k, bool)
    body[ends] = False
    pairs = {f"terms[{j}]": (got["terms"][:k][body, j], _n64(ref["terms"])[body, j], _n64(ref32["terms"])[body, j]) for j in range(5)}
    pairs.update({key: (got[key][:k][body], _n64(ref[key])[body], _n64(ref32[key])[body]) for key in ("d_o", "d_refine", "d_regress")})
    bad = _report("m2_loss", f"c1 {c1}, k {k}", pairs)
    neither = (c["pos"] == 0) & (c["sample"] == 0)
    assert neither.any() and all((got[key][:k][neither] == 0).all() for key in got)
    # the clamps: refine in {0, 1}
    x = torch.from_numpy(c["refine"][ends].copy()).requires_grad_(True)
    y = np.concatenate((c["pos"][ends, None].astype(np.float32), c["clabel"][ends]), 1)
    loss = F.binary_cross_entropy(x, torch.from_numpy(y), reduction="none")
    loss.sum().backward()
    is_pos = c["pos"][ends].astype(bool)
    assert np.array_equal(got["terms"][ends, 1], loss.detach().numpy()[:, 0])                      # (every end row is sampled)
    assert np.array_equal(got["terms"][ends, 2], np.where(is_pos, loss.detach().numpy()[:, 1:].sum(1), 0))   # (sums of 0 and 100: exact)
    want_g = np.float32(gs) * x.grad.numpy() / np.float32(l0)
    want_g[~is_pos, 1:] = 0
    assert np.array_equal(got["d_refine"][ends], want_g), (got["d_refine"][ends], want_g)
    assert np.abs(want_g).max() > 1e10 and got["terms"][ends, 1].max() == 100
    assert not bad, bad


@pytest.mark.parametrize("count", [1, 255, 257, 65535 * 256 + 3])
def test_mask_scale_bit_for_bit(hip_lib, count):
    """y = mask ? x * scale : 0 is one fp32 rounding of the float64 product; 65535 * 256 + 3 elements is one element more than a
    single pass of the largest grid covers.  Elements behind count keep their poison."""
    from millieye_amd import hip
    r = np.random.RandomState(count % 1000)
    x = r.standard_normal(count).astype(np.float32)
    mask = (r.randint(0, 3, count) * 100).astype(np.uint8)   # 0, 100, 200: any non-zero byte keeps
    scale = float(np.float32(1.7))
    y = _poison(count + 5)
    x_d, mask_d = _cu(x), _cu(mask)
    hip.check(hip.lib().me_mask_scale_f32(x_d.data_ptr(), mask_d.data_ptr(), scale, count, y.data_ptr(), hip.stream_ptr()), "me_mask_scale_f32")
    got = _host(y)
    want = R.mask_scale(x, mask, scale).astype(np.float32)
    assert np.array_equal(got[:count], want), f"{int((got[:count] != want).sum())} elements differ"
    assert (got[count:] == SENT).all()
    assert count == 1 or ((want != 0).any() and (want == 0).any())


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
