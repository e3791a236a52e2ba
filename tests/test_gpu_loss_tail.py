"""-m gpu: csrc/yolo_loss.hip (me_yolo_loss_fwd_f32, me_yolo_loss_fwd_counted_f32), csrc/evaltail.hip (me_batch_statistics_f32)
and csrc/optim.hip (me_adam_step_f32) one by one through the C ABI against the plain references of tests/loss_tail_refs.py
(pinned on the CPU by tests/test_loss_tail_refs_cpu.py, which also asserts the conditions on the inputs used here).

The test owns every buffer: every output sits in an allocation of its own between NaN (floats) or 0xA5 (bytes) guard bands and
starts out as that poison, the raw map is a channel slice of a wider pitched buffer whose neighbour channels are NaN (and, for
the same bits, a dense copy), the Adam tensors lie between sentinel gaps of one banded arena per buffer kind; guards, gaps and
inputs must survive every call.

Bars of the YOLO loss (float64 reference; the float32 form of the same reference is the yardstick of rounding):
* obj, noobj, tcls, tconf, class_mask, tx, ty, n_obj, n_noobj: exact.
* tw, th, iou_scores: error relative to the tensor's largest magnitude <= max(16 x the float32 form's, 4 * 2^-24).
* cls_acc, recall50, recall75, precision: within 2 fp32 units of the same ratio formed from the reference's integer counts.
* the loss terms, conf_obj, conf_noobj: relative error <= max(16 x the float32 form's, 4 * 2^-24).
Both errors of every case and term go to profiles/loss_tail_errors.txt.
Evaluation tail: every tp flag equal to the float32 reference.  Adam: parameters and both moments equal to the one-rounding-per-
operation float32 reference bit for bit (the kernel has contraction off, the build no fast-math flag, fp32 divide and square
root are correctly rounded).

Each test was run once against a deliberately broken build of its kernel and failed: the scatter's later-target scan starting at
t + 2 (wide and the counted table: tx of the cell rows 255 and 256 share), the reduce loop without its stride (wide: tconf of
the cells past 65 536, n_noobj), the cross-lane tie rule with ot > best_t (the mirrored pairs of every q >= 63; the duplicated
boxes alone do not see it), the Adam kernel without its i >= numel break (991 sentinel words behind the tensors)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import loss_tail_refs as R
from tests.conv_refs import banded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS_FILE = os.path.join(ROOT, "profiles", "loss_tail_errors.txt")
SENT = 12345.0
TP_SENT = 7.0
U = 2.0 ** -24
FLOOR = 4 * U
NAN = float("nan")
_LOG = {}
FLOAT_DENSE = ("tx", "ty", "tw", "th", "tcls", "tconf", "class_mask", "iou_scores")
EXACT = ("obj", "noobj", "tcls", "tconf", "class_mask", "tx", "ty")
TERMS = {"loss": 0, "x": 1, "y": 2, "w": 3, "h": 4, "conf": 5, "cls": 6, "conf_obj": 11, "conf_noobj": 12}
RATIOS = {"cls_acc": 7, "recall50": 8, "recall75": 9, "precision": 10}


def _log(section, line):
    _LOG.setdefault(section, []).append(line)
    print(line)


@pytest.fixture(scope="module", autouse=True)
def _write_errors_file():
    """Sections of profiles/loss_tail_errors.txt are replaced by the tests that ran; the others stay."""
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
    head = ("# Measured by tests/test_gpu_loss_tail.py on an MI355X.\n"
            "# yolo_loss: per case and term the kernel's and the float32 form's (tests/loss_tail_refs.py) error against the float64\n"
            "# reference (kernel / float32 form): scalars relative to the reference, tensors relative to their largest magnitude.\n"
            "# Bar: kernel <= max(16 x float32 form, 4 * 2^-24 = 2.4e-07).  adam: distance to the one-rounding-per-operation float32\n"
            "# reference in fp32 units in the last place (bar: 0).\n")
    try:
        with open(ERRORS_FILE, "w") as f:
            f.write(head)
            for name in sorted(sections):
                f.write(f"\n## {name}\n" + "\n".join(sections[name]) + "\n")
    except OSError:   # (a read-only checkout: the numbers are in the test output)
        pass


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _input(a, dtype=torch.float32):
    """A read-only operand in a banded allocation; returns (tensor, function asserting bands and content are unchanged)."""
    a = np.ascontiguousarray(a)
    t, bands = banded(a.shape, dtype, 64, 67, NAN if dtype == torch.float32 else 0x5A, "cuda")
    t.copy_(torch.from_numpy(a))

    def check(what):
        bands(what)
        assert _same_bits(t.cpu().numpy(), a), f"{what}: an input was written"

    return t, check


# ---------------------------------------------------------------------------------------------------------------------
# YOLO loss forward
# ---------------------------------------------------------------------------------------------------------------------
class _Outputs:
    """Every output of the loss kernel in its own poisoned allocation between guard bands."""

    def __init__(self, n, na, g, nc):
        cells = (n, na, g, g)
        self.t, self.bands = {}, []
        for k in ("obj", "noobj"):
            self.t[k], chk = banded(cells, torch.uint8, 256, 67, 0xA5, "cuda")
            self.bands.append(chk)
        for k in FLOAT_DENSE + ("result",):
            shape = (16,) if k == "result" else cells + ((nc,) if k == "tcls" else ())
            self.t[k], chk = banded(shape, torch.float32, 64, 67, NAN, "cuda")
            self.bands.append(chk)

    def ptrs(self):
        return [self.t[k].data_ptr() for k in ("obj", "noobj", "tx", "ty", "tw", "th", "tcls", "tconf", "class_mask", "iou_scores")]

    def host(self, what):
        for chk in self.bands:
            chk(what)
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def _workspace(lib):
    return torch.zeros(int(lib.me_yolo_loss_workspace_bytes()), dtype=torch.uint8, device="cuda")


def _yolo_run(lib, hip, c, targets, pitched=True, ws=None, count=None, scales=(1.0, 100.0), what=""):
    """One call on fresh poisoned outputs.  ``count`` (an int) selects the counted entry: ``targets`` is then the capacity table.
    Returns the outputs on the host (``result`` [16] among them) after the guards and the inputs were checked."""
    n, g, na, nc = c["n"], c["g"], c["na"], c["nc"]
    ch = na * (nc + 5)
    raw2 = c["raw"].reshape(n * g * g, ch)
    if pitched:
        frame = np.full((n * g * g, ch + 10), np.nan, np.float32)
        frame[:, 3:3 + ch] = raw2
        rbuf, rcheck = _input(frame)
        rptr, pitch = rbuf.data_ptr() + 3 * 4, ch + 10
    else:
        rbuf, rcheck = _input(raw2)
        rptr, pitch = rbuf.data_ptr(), ch
    m = len(targets)
    tbuf, tcheck = _input(np.asarray(targets, np.float32).reshape(m, 6)) if m else (None, None)
    out = _Outputs(n, na, g, nc)
    ws = _workspace(lib) if ws is None else ws
    anchors = (C.c_float * (2 * na))(*[float(v) for v in c["anchors"].ravel()])
    tail = out.ptrs() + [ws.data_ptr(), out.t["result"].data_ptr(), hip.stream_ptr()]
    tptr = tbuf.data_ptr() if m else None
    if count is None:
        rc = lib.me_yolo_loss_fwd_f32(rptr, pitch, n, g, na, nc, anchors, tptr, m, 0.5, scales[0], scales[1], *tail)
    else:
        cnt, ccheck = _input(np.array([count], np.int32), torch.int32)
        rc = lib.me_yolo_loss_fwd_counted_f32(rptr, pitch, n, g, na, nc, anchors, tptr, m, cnt.data_ptr(), 0.5, scales[0], scales[1],
                                              *tail)
    hip.check(rc, f"yolo loss {what}")
    torch.cuda.synchronize()
    host = out.host(what)
    rcheck(what + " raw")
    if m:
        tcheck(what + " targets")
    if count is not None:
        ccheck(what + " count")
    return host


def _assert_same_run(a, b, what):
    for k in a:
        assert _same_bits(a[k], b[k]), f"{what}: {k} differs"


def _rel_scalar(got, ref):
    return abs(float(got) - ref) / abs(ref) if ref != 0 else abs(float(got))


def _rel_tensor(got, ref):
    top = float(np.abs(ref).max()) if ref.size else 0.0
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / (top if top > 0 else 1.0) if ref.size else 0.0


def _check_against_ref(name, got, r64, r32, section="yolo_loss"):
    res = got["result"]
    assert res[15] == 0.0, f"{name}: the bad-target flag is set"
    for k in EXACT:
        bad = np.asarray(got[k], np.float64) != np.asarray(r64[k], np.float64)
        assert not bad.any(), f"{name} {k}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}"
    assert res[13] == r64["n_obj"] and res[14] == r64["n_noobj"], (name, res[13], res[14], r64["n_obj"], r64["n_noobj"])
    failures = []
    for k in ("tw", "th", "iou_scores"):
        assert not np.isnan(got[k]).any(), f"{name} {k}: NaN"
        ek, ef = _rel_tensor(got[k], r64[k]), _rel_tensor(r32[k], r64[k])
        _log(section, f"{name} {k}: {ek:.2e} / {ef:.2e}")
        if not ek <= max(16 * ef, FLOOR):
            failures.append((k, ek, ef))
    for k, want in zip(RATIOS, R.ratio_metrics32(r64)):
        g32 = np.float32(res[RATIOS[k]])
        if np.isnan(want):
            assert np.isnan(g32), (name, k, g32)
        else:
            assert abs(float(g32) - float(want)) <= 2 * float(np.spacing(np.abs(want))), (name, k, g32, want)
    for k, i in TERMS.items():
        ref = float(r64["scalars"][i])
        if np.isnan(ref):
            assert np.isnan(res[i]), (name, k, res[i])
            _log(section, f"{name} {k}: nan like the reference")
            continue
        ek, ef = _rel_scalar(res[i], ref), _rel_scalar(r32["scalars"][i], ref)
        _log(section, f"{name} {k}: {ek:.2e} / {ef:.2e}")
        if not ek <= max(16 * ef, FLOOR):
            failures.append((k, ek, ef))
    assert not failures, (name, failures)


@pytest.mark.parametrize("name", ("min", "base", "base16", "base64", "mid", "wide", "empty"))
def test_yolo_loss_fwd_vs_float64(hip_lib, name):
    """Every case on a pitched NaN-neighboured slice and on a dense copy: the same bits in all 16 result words and in every dense
    tensor, and the bars of the module docstring against the float64 reference.  ``wide`` (67 600 cells, 1 081 600 tcls elements,
    300 targets, 16 anchors) takes the grid-stride loops of the init and the reduce kernel and two scatter workgroups; base /
    base16 / base64 / wide carry the planted duplicates, ties, borders and the exact 0.5 objectness (asserted to be where the
    case says by tests/test_loss_tail_refs_cpu.py) - the exact tensors are what checks them."""
    from millieye_amd import hip
    lib = hip.lib()
    c = R.yolo_case(name)
    pitched = _yolo_run(lib, hip, c, c["targets"], True, what=name + " pitched")
    dense = _yolo_run(lib, hip, c, c["targets"], False, what=name + " dense")
    _assert_same_run(pitched, dense, name + ": pitched against dense")
    _check_against_ref(name, pitched, R.yolo_ref(name), R.yolo_ref(name, "float32"))


def test_yolo_loss_fwd_target_outside_the_grid(hip_lib):
    """cx = 1.0 is cell g: result[15] is set (the reference raises IndexError); the next call on the same workspace is clean
    again and gives the bits of a run on a fresh one."""
    from millieye_amd import hip
    lib = hip.lib()
    c = R.yolo_case("base")
    ws = _workspace(lib)
    bad = c["targets"].copy()
    bad[R.CELLMATES[0], 2] = 1.0
    assert _yolo_run(lib, hip, c, bad, ws=ws, what="outside")["result"][15] == 1.0
    again = _yolo_run(lib, hip, c, c["targets"], ws=ws, what="after outside")
    assert again["result"][15] == 0.0
    _assert_same_run(again, _yolo_run(lib, hip, c, c["targets"], what="fresh"), "after a flagged call")


def test_yolo_loss_fwd_saturated_logits(hip_lib):
    """Objectness and class logits of +40 / -104 in every cell (fp32 and float64 agree: probability exactly 1 or 0, the log clamp
    at -100 applies) and a raw width logit of 89 in one owner cell (exp overflows in fp32): every result word finite, iou_scores
    0 and not NaN in that cell, the bars against float64 - and every clamped element contributes exactly 100: with one of the
    two scales 0 the conf term, and the cls term, equal the count of wrong-side probabilities x 100 over the cell count formed
    in fp32, bit for bit."""
    from millieye_amd import hip
    lib = hip.lib()
    c = R.yolo_case("sat")
    r64, r32 = R.yolo_ref("sat"), R.yolo_ref("sat", "float32")
    got = _yolo_run(lib, hip, c, c["targets"], what="sat")
    _assert_same_run(got, _yolo_run(lib, hip, c, c["targets"], False, what="sat dense"), "sat: pitched against dense")
    assert np.isfinite(got["result"]).all(), got["result"]
    at = tuple(r64["owner"][R.THRESH])
    assert got["iou_scores"][at] == 0.0 and got["obj"][at] == 1
    _check_against_ref("sat", got, r64, r32)
    want = R.sat_expected(c, r64)
    for k, scales in enumerate(((1.0, 0.0), (0.0, 1.0))):
        res = _yolo_run(lib, hip, c, c["targets"], scales=scales, what=f"sat scales {scales}")["result"]
        assert float(res[5]) == want[k] and float(res[6]) == want[2], (scales, res[5], res[6], want)


def test_yolo_loss_fwd_counted_entry(hip_lib):
    """me_yolo_loss_fwd_counted_f32 over a table of 600 rows: live counts 257 (crosses a scatter workgroup, the duplicate pair
    (255, 256) straddles it; the rows behind hold NaN, 123.0 and out-of-grid values), 0, -5 (clamps to 0) and 10 000 (clamps to
    the capacity; the table then holds 600 valid rows) - each equal, bit for bit in result (result[15] = 0 included) and dense
    tensors, to the plain entry on the live rows alone."""
    from millieye_amd import hip
    lib = hip.lib()
    c = R.yolo_case("wide")
    tg = c["targets"]
    table = np.empty((600, 6), np.float32)
    table[:257] = tg[:257]
    junk = np.array([[np.nan] * 6, [123.0] * 6, [0, 1, 7.5, -3.0, 0.2, 0.2], [99, 99, 0.5, 0.5, 0.1, 0.1]], np.float32)
    table[257:] = junk[np.arange(600 - 257) % 4]
    full = np.concatenate([tg, tg])
    for count, tab, live in ((257, table, tg[:257]), (0, table, tg[:0]), (-5, table, tg[:0]), (10000, full, full)):
        counted = _yolo_run(lib, hip, c, tab, count=count, what=f"counted {count}")
        plain = _yolo_run(lib, hip, c, live, what=f"plain {len(live)}")
        assert counted["result"][15] == 0.0 and counted["result"][13] == R.yolo_ref("wide", m=len(live))["n_obj"]
        _assert_same_run(counted, plain, f"live count {count}")
        if count == 257:   # ... and the live rows against float64: row 256 wins the cell it shares with row 255
            ref = R.yolo_ref("wide", m=257)
            assert tuple(ref["owner"][256]) == tuple(ref["owner"][255]) and ref["winner"][255] == 256
            _check_against_ref("wide[:257] counted", counted, ref, R.yolo_ref("wide", "float32", m=257), section="yolo_loss_counted")


def test_yolo_loss_fwd_workspace_reuse(hip_lib):
    """``wide`` (256 reduce blocks) and then ``min`` (1 block) on one workspace: the bits of ``min`` on a fresh zeroed workspace
    (no partial sum of the larger launch is read).  ``wide`` twice: the same bits (fixed-order sums)."""
    from millieye_amd import hip
    lib = hip.lib()
    wide, small = R.yolo_case("wide"), R.yolo_case("min")
    ws = _workspace(lib)
    first = _yolo_run(lib, hip, wide, wide["targets"], ws=ws, what="wide")
    after = _yolo_run(lib, hip, small, small["targets"], ws=ws, what="min after wide")
    _assert_same_run(after, _yolo_run(lib, hip, small, small["targets"], what="min fresh"), "min after wide")
    _assert_same_run(first, _yolo_run(lib, hip, wide, wide["targets"], ws=ws, what="wide again"), "wide twice")


# ---------------------------------------------------------------------------------------------------------------------
# evaluation tail
# ---------------------------------------------------------------------------------------------------------------------
def _stats_run(lib, hip, rows, tg, n_images, thr, what=""):
    m, q = len(rows), len(tg)
    rbuf, rcheck = _input(rows)
    tbuf, tcheck = _input(tg) if q else (None, None)
    tp, bands = banded((m,), torch.float32, 64, 67, TP_SENT, "cuda")
    rc = lib.me_batch_statistics_f32(rbuf.data_ptr(), m, rows.shape[1], tbuf.data_ptr() if q else None, q, n_images, float(thr),
                                     tp.data_ptr(), hip.stream_ptr())
    torch.cuda.synchronize()
    bands(what)
    rcheck(what + " rows")
    if q:
        tcheck(what + " targets")
    return rc, tp.cpu().numpy()


@pytest.mark.parametrize("q,cols", [(q, 8) for q in R.STATS_Q] + [(130, 11), (65, 11)])
def test_batch_statistics_vs_float32_reference(hip_lib, q, cols):
    """q targets on 4 to 6 images (each bulk image's targets in every lane and, from q = 130, in second and third trips of a
    lane; duplicated target boxes on neighbouring lanes, in two trips of one lane, across lanes and trips, across a bitmap word;
    pairs of different boxes whose IoUs with one detection tie exactly, in the same three positions - the lower index must be
    the one taken, which the copies of the two boxes that follow show; the highest target index matched; an image whose targets are all taken early; images without targets / without detections;
    rows outside the batch): every tp equal to the reference, the sentinel kept in rows outside the batch, the same bits twice."""
    from millieye_amd import hip
    lib = hip.lib()
    rows, tg, n_images, notes = R.stats_case(q, cols)
    for thr in (0.5,) if q != 130 else (0.5, 0.3, 0.9):
        ref, written = R.batch_statistics_ref(rows, tg, n_images, thr)
        rc, tp = _stats_run(lib, hip, rows, tg, n_images, thr, f"q {q}")
        hip.check(rc, "me_batch_statistics_f32")
        assert (tp[~written] == TP_SENT).all() and (~written).sum() > 0, "a row outside the batch was written"
        bad = np.flatnonzero(tp[written] != ref[written])
        assert bad.size == 0, (q, cols, thr, np.flatnonzero(written)[bad][:8].tolist())
        for r, want in notes["expect"].items() if thr == 0.5 else ():
            assert tp[r] == want, (q, r, want)
        rc, again = _stats_run(lib, hip, rows, tg, n_images, thr, f"q {q} again")
        assert rc == 0 and _same_bits(tp, again)
    _log("batch_statistics", f"q {q} cols {cols}: {len(rows)} rows on {n_images} images, {int(ref[written].sum())} true positives at thr {thr} - equal")


def test_batch_statistics_limits_and_thresholds(hip_lib):
    """8193 targets are refused with an error naming the limit and tp untouched; no rows: 0 without a launch; no targets: every
    row of the batch 0; IoU >= thr: an exact copy is a true positive at thr = 1.0, a jittered box at thr = its fp32 IoU and not
    one fp32 step above."""
    from millieye_amd import hip
    lib = hip.lib()
    rows, tg, n_images, _ = R.stats_case(8192)
    more = np.concatenate([tg, tg[:1]])
    rc, tp = _stats_run(lib, hip, rows, more, n_images, 0.5, "8193")
    assert rc < 0 and b"8192" in lib.me_last_error() and (tp == TP_SENT).all()
    assert lib.me_batch_statistics_f32(None, 0, 8, None, 0, n_images, 0.5, None, hip.stream_ptr()) == 0
    rc, tp = _stats_run(lib, hip, rows, tg[:0], n_images, 0.5, "no targets")
    inside = (rows[:, 0] >= 0) & (rows[:, 0] < n_images)
    assert rc == 0 and (tp[inside] == 0).all() and (tp[~inside] == TP_SENT).all()
    rows, tg, n_images = R.stats_threshold_case()
    rc, tp = _stats_run(lib, hip, rows[:1], tg, n_images, 1.0, "thr 1")
    assert rc == 0 and tp[0] == 1.0
    iou = R.stats_threshold_iou()
    for thr, want in ((iou, 1.0), (np.nextafter(iou, np.float32(2)), 0.0)):
        rc, tp = _stats_run(lib, hip, rows[1:], tg, n_images, thr, "thr at the IoU")
        assert rc == 0 and tp[0] == want, (thr, tp)


# ---------------------------------------------------------------------------------------------------------------------
# Adam / AdamW
# ---------------------------------------------------------------------------------------------------------------------
GAP = 16


class _Arena:
    """The tensors of one buffer kind in one banded allocation, a sentinel gap in front of, between and behind them."""

    def __init__(self, arrays):
        total = sum(len(a) + GAP for a in arrays) + GAP
        self.image = np.full(total, SENT, np.float32)
        self.offsets, o = [], GAP
        for a in arrays:
            self.image[o:o + len(a)] = a
            self.offsets.append(o)
            o += len(a) + GAP
        self.dev, self.bands = banded((total,), torch.float32, 64, 1091, SENT, "cuda")   # (a chunk that ran past numel stays inside)
        self.dev.copy_(torch.from_numpy(self.image))

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.offsets[i]

    def expect(self, arrays, what):
        """The arena holds ``arrays`` and, everywhere else, the sentinel - bit for bit."""
        self.bands(what)
        want = self.image.copy()
        for o, a in zip(self.offsets, arrays):
            want[o:o + len(a)] = a
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, f"{what}: {bad.size} words differ, first at {int(bad[0])}: {got[bad[0]]!r} vs {want[bad[0]]!r}"


def _adam_setup(hip, table, scalars, decoupled, null_empty=False):
    chunk = int(hip.lib().me_adam_chunk())
    arenas = [_Arena([t[k] for t in table]) for k in range(4)]
    d = hip.AdamDesc()
    chunks = 0
    for i, t in enumerate(table):
        n = len(t[0])
        for field, arena in zip((d.param, d.grad, d.exp_avg, d.exp_avg_sq), arenas):
            field[i] = None if (null_empty and n == 0) else arena.ptr(i)
        d.numel[i] = n
        d.first_chunk[i] = chunks
        chunks += (n + chunk - 1) // chunk
    d.count, d.decoupled = len(table), 1 if decoupled else 0
    for k, v in scalars.items():
        setattr(d, k, float(v))
    return d, arenas


def _adam_unchanged(arenas, table, what):
    for k, arena in enumerate(arenas):
        arena.expect([t[k] for t in table], what)


@pytest.mark.parametrize("kind", sorted(R.ADAM_KINDS))
@pytest.mark.parametrize("step", (1, 1000))
def test_adam_step_bit_for_bit(hip_lib, kind, step):
    """One step from non-zero moments over a table of 64 tensors (element counts cycling through 1, 3, 1023, 1024, 1025, 2048,
    4097 and 0 - a 0 in the middle and in the last slot, null pointers for the empty ones at step 1000; gradients of 1e-6 .. 1e2,
    some exactly 0 with v = 0: the denominator is eps): parameters and both moments equal adam_step_ref bit for bit, nothing
    past numel and no gradient changes."""
    from millieye_amd import hip
    lib = hip.lib()
    decoupled, kw = R.ADAM_KINDS[kind]
    table = R.adam_table()
    assert len(table) == 64 and len(table[31][0]) == 0 and len(table[63][0]) == 0
    sc = R.adam_scalars(kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"], step)
    d, arenas = _adam_setup(hip, table, sc, decoupled, null_empty=step == 1000)
    hip.check(lib.me_adam_step_f32(C.byref(d), hip.stream_ptr()), "me_adam_step_f32")
    torch.cuda.synchronize()
    want = [R.adam_step_ref(p, g, m, v, sc, decoupled) for p, g, m, v in table]
    got = [a.dev.cpu().numpy() for a in arenas]
    worst = {}
    for name, k, j in (("p", 0, 0), ("m", 2, 1), ("v", 3, 2)):
        worst[name] = max(R.ulp_distance(got[k][o:o + len(w[j])], w[j]) for o, w in zip(arenas[k].offsets, want))
    _log("adam", f"{kind} step {step}: p {worst['p']:.0f} ulp, exp_avg {worst['m']:.0f} ulp, exp_avg_sq {worst['v']:.0f} ulp")
    arenas[1].expect([t[1] for t in table], "gradients")
    arenas[0].expect([w[0] for w in want], "parameters")
    arenas[2].expect([w[1] for w in want], "exp_avg")
    arenas[3].expect([w[2] for w in want], "exp_avg_sq")


def test_adam_step_refusals_and_trivial_counts(hip_lib):
    """Refused before any launch, with an error code and every buffer untouched: 65 tensors, a first_chunk that is not the
    prefix sum, a null pointer with numel > 0, 1 - beta1 = 0.5.  0 tensors and a table of empty tensors return 0."""
    from millieye_amd import hip
    lib = hip.lib()
    decoupled, kw = R.ADAM_KINDS["adamw"]
    table = R.adam_table()[:16]
    sc = R.adam_scalars(kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"], 1)

    def spoil_count(d):
        d.count = 65

    def spoil_chunk(d):
        d.first_chunk[3] += 1

    def spoil_ptr(d):
        d.grad[2] = None

    def spoil_beta(d):
        d.one_minus_beta1 = 0.5

    for spoil in (spoil_count, spoil_chunk, spoil_ptr, spoil_beta):
        d, arenas = _adam_setup(hip, table, sc, decoupled)
        spoil(d)
        assert lib.me_adam_step_f32(C.byref(d), hip.stream_ptr()) < 0 and lib.me_last_error(), spoil.__name__
        torch.cuda.synchronize()
        _adam_unchanged(arenas, table, spoil.__name__)
    d, arenas = _adam_setup(hip, table, sc, decoupled)
    d.count = 0
    assert lib.me_adam_step_f32(C.byref(d), hip.stream_ptr()) == 0
    empty = [tuple(a[:0] for a in t) for t in table[:5]]
    d2, arenas2 = _adam_setup(hip, empty, sc, decoupled, null_empty=True)
    assert lib.me_adam_step_f32(C.byref(d2), hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    _adam_unchanged(arenas, table, "count 0")
    _adam_unchanged(arenas2, empty, "empty tensors")
