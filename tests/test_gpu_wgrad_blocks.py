"""-m gpu: the fp32 weight-gradient kernels (csrc/train.hip, csrc/wgrad9.hip) form by form through the C ABI, on buffers the test
owns, against the float64 reference tests/train_block_refs.conv_wgrad (pinned to torch float64 autograd by
tests/test_train_block_refs_cpu.py).  The cases live in tests/wgrad_cases.py; every one first asserts, through
``me_conv_wgrad_form`` on its real pointers, that the launcher runs the kernel form it is there for (the same is asserted
without a GPU by tests/test_wgrad_form_cpu.py).

EXACT inputs are integers |v| <= 4: every product and partial sum is exact in fp32 for fewer than 2^20 pixels, so the result
must equal float64 BIT FOR BIT in the OHWI and the OIHW layout, whatever the order of summation.

A. Every default form (and the plain kernel me_conv_wgrad_f32) on exact inputs, and one real-input case per form: the largest
   error against float64 relative to the output's largest magnitude at most max(16 x the same figure of stock torch fp32 CPU
   autograd, 4 * 2^-24), every element within T * 2^-24 * sum|dy||x| over its T terms, a second run bit-identical.  Both errors
   of every real case go to profiles/wgrad_errors.txt.
B. Poison.  EVERY run of this file (A - D) has x and dy inside NaN allocations (guard bands, and NaN channels beside the slice
   where the case has any), dw inside a NaN allocation and a NaN workspace of exactly the size passed: dw must be finite and
   exact, every band untouched.  B adds one case per kernel form and per reduction form, the direct-write path without any
   workspace, me_conv_wgrad_h16 (it shares the slab reductions), and locality: one NaN in x[img, y, x, ci] may change only
   dW[:, ci], one NaN in dy[p, co] only dW[co], each at least where the reference turns NaN.
C. The workspace contract: full, one float short of what the form needs, exactly one slab, none - all exact, each on the form
   the query predicts; OIHW with k > 1 and less than one slab is refused and leaves dw alone; the documented refusals.
D. The forms only a process switch reaches (MILLIEYE_WGRAD_TILE / _DEPTH, MILLIEYE_WGRAD9 / _NG), each in one fresh child process.

NOT covered: the MILLIEYE_ABLATION forms of conv_wgrad_mfma_kernel (they compute wrong results on purpose), the transposing
branch (kk > 0) of conv_wgrad_reduce_kernel (ME_WGRAD_REDUCE_OIHW_FLAT: cout >= 65536), and the P >= 2^31 guard (operands of
8 GiB)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (the children of part D run this file as a script)
    sys.path.insert(0, ROOT)

from millieye_amd import synth  # noqa: E402
from tests import conv_refs  # noqa: E402
from tests import train_block_refs as R  # noqa: E402
from tests import wgrad_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
U = 2.0 ** -24
FLOOR = 4 * U
SENT = 12345.0
ERRORS_FILE = os.path.join(ROOT, "profiles", "wgrad_errors.txt")
_LOG = {}
_REFS = {}


def _log(section, line):
    _LOG.setdefault(section, []).append(line)
    print(line)


@pytest.fixture(scope="module", autouse=True)
def _write_errors_file():
    """Sections of profiles/wgrad_errors.txt are replaced by the tests that ran; the others stay."""
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
    head = ("# Measured by tests/test_gpu_wgrad_blocks.py on an MI355X: per real-input case the kernel's and stock torch fp32 CPU's\n"
            "# largest error against the float64 reference, relative to the output's largest magnitude (kernel / torch), and the\n"
            "# kernel's worst element against the dot-product bound T * 2^-24 * sum|dy||x|.\n"
            "# Bar: kernel <= max(16 x torch, 4 * 2^-24 = 2.4e-07) and worst error / bound <= 1.\n")
    try:
        with open(ERRORS_FILE, "w") as f:
            f.write(head)
            for name in sorted(sections):
                f.write(f"\n## {name}\n" + "\n".join(sections[name]) + "\n")
    except OSError:   # (a read-only checkout: the numbers are in the test output)
        pass


# ---------------------------------------------------------------------------------------------------------------------
# operands, references, one launch
# ---------------------------------------------------------------------------------------------------------------------
def _exact_operands(c):
    rng = np.random.RandomState(sum(map(ord, c["name"])) + c["cin"] * 7 + c["cout"])
    ho, wo = W.out_hw(c)
    return W.ints(rng, (c["n"], c["h"], c["w"], c["cin"])), W.ints(rng, (c["n"], ho, wo, c["cout"]))


def _real_operands(c):
    ho, wo = W.out_hw(c)
    x = synth.normal("wg/x" + c["name"], (c["n"], c["h"], c["w"], c["cin"]))
    dy = (synth.normal("wg/d" + c["name"], (c["n"], ho, wo, c["cout"])) / np.float32(W.pixels(c))).astype(np.float32)
    return x, dy


def _ref(c, x, dy, key):
    """float64 dW [cout, cin, k, k], computed once per (case shape, operands) and never modified."""
    key = (key, c["k"], c["s"], c["pad"], x.shape, dy.shape, hashlib.sha1(x.tobytes()).digest(), hashlib.sha1(dy.tobytes()).digest())
    if key not in _REFS:
        ref = R.conv_wgrad(x, dy, c["k"], c["s"], c["pad"])
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def _sliced(a, left, right):
    """numpy [..., c] -> (GPU view [rows, c] inside a NaN allocation of [rows, left + c + right] between NaN bands, band check)."""
    c = a.shape[-1]
    rows = a.size // c
    buf, check = conv_refs.banded((rows, left + c + right), torch.float32, 256, 256, NAN, "cuda")
    view = buf[:, left:left + c]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(rows, c)))
    return view, check


def _bits_equal(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements are not finite, first at " \
                                   f"{np.argwhere(~np.isfinite(got))[0].tolist()}"
    bad = got != ref
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[bad][0]!r} vs {ref[bad][0]!r}"


def _launch(hip, c, x, dy, expect=True):
    """One call of me_conv_wgrad_mfma_f32 / _oihw_f32 on the case, every buffer poisoned as the module docstring says.
    Returns dW as float64 [cout, cin, k, k] (``expect`` = a return code: the code must come back and dw stay untouched)."""
    lib = hip.lib()
    xv, xcheck = _sliced(x, c["xl"], c["xr"])
    yv, ycheck = _sliced(dy, c["yl"], c["yr"])
    k, cin, cout = c["k"], c["cin"], c["cout"]
    dw, dwcheck = conv_refs.banded((cout, cin, k, k) if c["oihw"] else (cout, k, k, cin), torch.float32, 256, 256, NAN, "cuda")
    nbytes = W.workspace_bytes(lib, c)
    ws, wscheck = (None, None)
    if nbytes > 0:
        assert nbytes % 4 == 0
        ws, wscheck = conv_refs.banded((nbytes // 4,), torch.float32, 64, 1024, NAN, "cuda")
    ptrs = dict(x_ptr=xv.data_ptr(), dy_ptr=yv.data_ptr(), dw_ptr=dw.data_ptr(), ws_ptr=ws.data_ptr() if ws is not None else None,
                ws_bytes=nbytes)
    if expect is True:
        W.assert_form(hip, c, **ptrs)
    else:
        assert W.query(hip, c, **ptrs)[0] == expect, c["name"]
    fn = lib.me_conv_wgrad_mfma_oihw_f32 if c["oihw"] else lib.me_conv_wgrad_mfma_f32
    rc = fn(xv.data_ptr(), c["xl"] + cin + c["xr"], yv.data_ptr(), c["yl"] + cout + c["yr"], dw.data_ptr(), c["n"], c["h"], c["w"],
            cin, cout, k, c["s"], c["pad"], ws.data_ptr() if ws is not None else None, nbytes, hip.stream_ptr())
    torch.cuda.synchronize()
    for what, chk in (("x", xcheck), ("dy", ycheck), ("dw", dwcheck), ("workspace", wscheck)):
        if chk is not None:
            chk(f"{c['name']}: {what}")
    if expect is not True:
        assert rc == expect, (c["name"], rc)
        assert bool(torch.isnan(dw).all()), f"{c['name']}: a refused call wrote dw"
        return None
    hip.check(rc, c["name"])
    got = dw.cpu().numpy().astype(np.float64)
    return got if c["oihw"] else got.transpose(0, 3, 1, 2)


def _exact_case(hip, c, layouts=(False, True)):
    x, dy = _exact_operands(c)
    ref = _ref(c, x, dy, "exact")
    for oihw in layouts:
        cc = dict(c, oihw=oihw, reduce=c["reduce"] if oihw == c["oihw"] else None)
        _bits_equal(_launch(hip, cc, x, dy), ref, f"{c['name']} {'OIHW' if oihw else 'OHWI'}")


def _torch_fp32(x, dy, c):
    xt = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)
    wt = torch.zeros((c["cout"], c["cin"], c["k"], c["k"]), requires_grad=True)
    F.conv2d(xt, wt, None, c["s"], c["pad"]).backward(torch.from_numpy(np.ascontiguousarray(dy)).permute(0, 3, 1, 2))
    return wt.grad.numpy().astype(np.float64)


def _rel(got, ref):
    m = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / (m if m > 0 else 1.0)


def _real_figures(c, x, dy, got, section):
    """Logs and returns (ok, line) for one real-input result ``got`` [cout, cin, k, k]."""
    ref = _ref(c, x, dy, "real")
    bound = W.pixels(c) * U * _ref(c, np.abs(x), np.abs(dy), "abs")
    assert np.isfinite(got).all(), c["name"]
    ek, et = _rel(got, ref), _rel(_torch_fp32(x, dy, c), ref)
    worst = float((np.abs(got - ref) / bound).max())
    ok = ek <= max(16.0 * et, FLOOR) and worst <= 1.0
    line = f"{c['name']} ({c['form']}, {W.pixels(c)} pixels, cin {c['cin']} cout {c['cout']} k {c['k']} s {c['s']}): " \
           f"{ek:.2e} / {et:.2e}, worst error / bound {worst:.2e}" + ("" if ok else "  ABOVE THE BAR")
    _log(section, line)
    return ok, line


# ---------------------------------------------------------------------------------------------------------------------
# A. every default form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in W.PART_A])
def test_default_form_exact_vs_float64(hip_lib, name):
    from millieye_amd import hip
    _exact_case(hip, next(c for c in W.PART_A if c["name"] == name))


@pytest.mark.parametrize("name", W.PART_A_REAL)
def test_default_form_real_inputs_vs_float64(hip_lib, name):
    from millieye_amd import hip
    c = dict(next(c for c in W.PART_A if c["name"] == name), oihw=True)
    x, dy = _real_operands(c)
    got = _launch(hip, c, x, dy)
    ok, line = _real_figures(c, x, dy, got, "default forms")
    again = _launch(hip, c, x, dy)
    assert np.array_equal(got, again), f"{name}: a second run differs"
    assert ok, line


def _plain_launch(hip, x, dy, k, s, pad, xp, yp):
    n, h, w, cin = x.shape
    cout = dy.shape[-1]
    xv, xcheck = _sliced(x, 0, xp)
    yv, ycheck = _sliced(dy, 0, yp)
    dw, dwcheck = conv_refs.banded((cout, k, k, cin), torch.float32, 256, 256, NAN, "cuda")
    hip.check(hip.lib().me_conv_wgrad_f32(xv.data_ptr(), cin + xp, yv.data_ptr(), cout + yp, dw.data_ptr(), n, h, w, cin, cout, k, s,
                                          pad, hip.stream_ptr()), "me_conv_wgrad_f32")
    torch.cuda.synchronize()
    for chk in (xcheck, ycheck, dwcheck):
        chk("me_conv_wgrad_f32")
    return dw.cpu().numpy().astype(np.float64).transpose(0, 3, 1, 2)


@pytest.mark.parametrize("shape", W.PLAIN)
def test_plain_kernel_vs_float64(hip_lib, shape):
    """me_conv_wgrad_f32 (conv_wgrad_kernel, no matrix pipe): ragged channel blocks, k = 1 / 3 / 7, stride 2, pitched operands."""
    from millieye_amd import hip
    n, h, w, cin, cout, k, s, pad, xp, yp = shape
    c = W.case(f"plain_{cin}_{cout}_k{k}_s{s}", "plain", n, h, w, cin, cout, k, s=s, pad=pad)
    x, dy = _exact_operands(c)
    _bits_equal(_plain_launch(hip, x, dy, k, s, pad, xp, yp), _ref(c, x, dy, "exact"), c["name"])
    if shape == W.PLAIN_REAL:
        x, dy = _real_operands(c)
        got = _plain_launch(hip, x, dy, k, s, pad, xp, yp)
        ok, line = _real_figures(c, x, dy, got, "plain kernel")
        assert np.array_equal(got, _plain_launch(hip, x, dy, k, s, pad, xp, yp)), "a second run differs"
        assert ok, line


# ---------------------------------------------------------------------------------------------------------------------
# B. poison, bands, locality
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in W.PART_B])
def test_poisoned_neighbours_and_workspace(hip_lib, name):
    from millieye_amd import hip
    c = next(c for c in W.PART_B if c["name"] == name)
    assert c["xl"] + c["xr"] > 0 and c["yl"] + c["yr"] > 0
    _exact_case(hip, c, layouts=(c["oihw"],))


def _tap_pixels(c):
    ho, wo = W.out_hw(c)
    return [(0, c["h"] // 2, c["w"] // 2), (c["n"] - 1, c["h"] - 1, c["w"] - 1)], [(0, 0, 0), (c["n"] - 1, ho - 1, wo - 1)]


@pytest.mark.parametrize("name", W.LOCALITY)
def test_one_nan_stays_in_its_channel(hip_lib, name):
    from millieye_amd import hip
    c = next(c for c in W.PART_B if c["name"] == name)
    x, dy = _exact_operands(c)
    clean = _launch(hip, c, x, dy)
    xpix, ypix = _tap_pixels(c)
    for i, (img, yy, xx) in enumerate(xpix):
        ci = (c["cin"] - 1, 0)[i % 2] if c["cin"] > 1 else 0
        xn = x.copy()
        xn[img, yy, xx, ci] = np.nan
        got = _launch(hip, c, xn, dy)
        want_nan = np.isnan(R.conv_wgrad(xn, dy, c["k"], c["s"], c["pad"]))
        assert want_nan.any() and not np.delete(want_nan, ci, axis=1).any()
        nan = np.isnan(got)
        assert not np.delete(nan, ci, axis=1).any(), f"{name}: a NaN in x channel {ci} reached another input channel"
        assert (nan | ~want_nan).all(), f"{name}: {int((want_nan & ~nan).sum())} elements missed the NaN in x{(img, yy, xx, ci)}"
        assert np.array_equal(got[~nan], clean[~nan]), f"{name}: x{(img, yy, xx, ci)} changed elements it does not feed"
    for i, (img, yy, xx) in enumerate(ypix):
        co = (0, c["cout"] - 1)[i % 2]
        dn = dy.copy()
        dn[img, yy, xx, co] = np.nan
        got = _launch(hip, c, x, dn)
        want_nan = np.isnan(R.conv_wgrad(x, dn, c["k"], c["s"], c["pad"]))
        assert want_nan.any() and not np.delete(want_nan, co, axis=0).any()
        nan = np.isnan(got)
        assert not np.delete(nan, co, axis=0).any(), f"{name}: a NaN in dy channel {co} reached another output channel"
        assert (nan | ~want_nan).all(), f"{name}: {int((want_nan & ~nan).sum())} elements missed the NaN in dy{(img, yy, xx, co)}"
        assert np.array_equal(got[~nan], clean[~nan]), f"{name}: dy{(img, yy, xx, co)} changed elements it does not feed"


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("shape", W.H16)
def test_h16_slab_reductions_with_a_poisoned_workspace(hip_lib, half, shape):
    """me_conv_wgrad_h16 (64 x 64 and 128 x 128 tiles): 16-bit channel slices between NaN channels, a NaN workspace of exactly
    the size asked for, dw between NaN bands; small integers are exact in both storage types."""
    from millieye_amd import hip
    lib = hip.lib()
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[half]
    n, h, w, cin, cout, k, s, oihw = shape
    c = W.case(f"h16_{cin}_{cout}_k{k}_s{s}", "h16", n, h, w, cin, cout, k, s=s, oihw=oihw)
    x, dy = _exact_operands(c)
    ho, wo = W.out_hw(c)

    def sliced16(a, left, right):
        ch = a.shape[-1]
        buf, check = conv_refs.banded((a.size // ch, left + ch + right), dt, 256, 256, NAN, "cuda")
        view = buf[:, left:left + ch]
        view.copy_(torch.from_numpy(a.reshape(-1, ch)).to(dt))
        return view, check

    xv, xcheck = sliced16(x, 8, 16)
    yv, ycheck = sliced16(dy, 16, 8)
    dw, dwcheck = conv_refs.banded((cout, cin, k, k) if oihw else (cout, k, k, cin), torch.float32, 256, 256, NAN, "cuda")
    nbytes = W.full_workspace_bytes(lib, c)
    ws, wscheck = conv_refs.banded((max(nbytes // 4, 1),), torch.float32, 64, 1024, NAN, "cuda")
    hip.check(lib.me_conv_wgrad_h16(xv.data_ptr(), cin + 24, yv.data_ptr(), cout + 24, dw.data_ptr(), n, h, w, cin, cout, k, s,
                                    c["pad"], ws.data_ptr() if nbytes else None, nbytes, 1 if oihw else 0, hip.HALF_TYPES[dt],
                                    hip.stream_ptr()), "me_conv_wgrad_h16")
    torch.cuda.synchronize()
    for chk in (xcheck, ycheck, dwcheck) + ((wscheck,) if nbytes else ()):
        chk(c["name"])
    got = dw.cpu().numpy().astype(np.float64)
    _bits_equal(got if oihw else got.transpose(0, 3, 1, 2), _ref(c, x, dy, "exact"), c["name"])


# ---------------------------------------------------------------------------------------------------------------------
# C. the workspace contract
# ---------------------------------------------------------------------------------------------------------------------
def _form_need(hip, c):
    """Bytes the case's own form needs: its slabs (the stem: its 768 partial sums per weight)."""
    form, splits, _reduce = W.query(hip, c)
    assert form == c["form"]
    return splits * W.count(c) * 4


@pytest.mark.parametrize("oihw", [False, True], ids=["ohwi", "oihw"])
@pytest.mark.parametrize("name", [c["name"] for c in W.PART_C])
def test_workspace_contract(hip_lib, name, oihw):
    """Whatever workspace the caller has, an OHWI call computes the same exact result: on the form's own kernel with the full
    workspace, on the per-tap kernels in one pass otherwise (the stem: on the generic scalar kernel).  OIHW with k > 1 needs one
    slab to transpose from."""
    from millieye_amd import hip
    base = dict(next(c for c in W.PART_C if c["name"] == name), oihw=oihw)
    need, slab = _form_need(hip, base), 4 * W.count(base)
    fallback = "mfma_scalar" if base["form"] == "stem" else "mfma_vec"
    x, dy = _exact_operands(base)
    ref = _ref(base, x, dy, "exact")
    assert need > slab
    for ws, form, splits in (("full", base["form"], base["splits"]), (need - 4, fallback, 1), (slab, fallback, 1),
                             (slab - 4, fallback, 1), (None, fallback, 1)):
        c = dict(base, ws=ws, form=form, splits=splits, name=f"{name} ws {ws}")
        if oihw and (ws is None or ws == slab - 4):
            _launch(hip, c, x, dy, expect=W.BADARG)
            continue
        if ws != "full":
            c["reduce"] = "none" if not oihw else ("oihw_v4" if c["cin"] % 4 == 0 else "oihw")
        _bits_equal(_launch(hip, c, x, dy), ref, c["name"])


def test_documented_refusals(hip_lib):
    """Null operands, ksize = 8, n = 0, a filter larger than the padded map: the negative code, before any launch (the query
    returns the same code: it IS the launcher's decision), dw untouched."""
    from millieye_amd import hip
    lib = hip.lib()
    c = W.case("refusals", "mfma_vec", 2, 13, 11, 36, 100, 3)
    x, dy = _exact_operands(c)
    xv, _ = _sliced(x, 0, 0)
    yv, _ = _sliced(dy, 0, 0)
    dw = torch.full((100, 3, 3, 36), SENT, device="cuda")
    ws = torch.full((W.full_workspace_bytes(lib, c) // 4,), SENT, device="cuda")

    def call(fn, xp=xv.data_ptr(), yp=yv.data_ptr(), dp=dw.data_ptr(), n=2, h=13, w=11, k=3, pad=1):
        return fn(xp, 36, yp, 100, dp, n, h, w, 36, 100, k, 1, pad, ws.data_ptr(), ws.numel() * 4, hip.stream_ptr())

    for fn in (lib.me_conv_wgrad_mfma_f32, lib.me_conv_wgrad_mfma_oihw_f32):
        assert call(fn, xp=None) == W.NULLPTR and call(fn, yp=None) == W.NULLPTR and call(fn, dp=None) == W.NULLPTR
        assert call(fn, k=8) == W.BADARG and call(fn, n=0) == W.BADARG
        assert call(fn, h=3, w=3, k=7, pad=0) == W.BADARG
        assert b"filter is larger" in lib.me_last_error()
    plain = lambda **kw: lib.me_conv_wgrad_f32(kw.get("xp", xv.data_ptr()), 36, yv.data_ptr(), 100, dw.data_ptr(), kw.get("n", 2),  # noqa: E731
                                               kw.get("h", 13), kw.get("w", 11), 36, 100, kw.get("k", 3), 1, kw.get("pad", 1),
                                               hip.stream_ptr())
    assert plain(xp=None) == W.NULLPTR and plain(k=8) == W.BADARG and plain(n=0) == W.BADARG
    assert plain(h=3, w=3, k=7, pad=0) == W.BADARG
    torch.cuda.synchronize()
    assert bool((dw == SENT).all()) and bool((ws == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# D. the switch-only forms, each in one fresh child process
# ---------------------------------------------------------------------------------------------------------------------
_CHILD_LOST = []


def _child(name):
    """Runs with the child's switches in the environment (they are read once, at the first weight gradient of a process):
    every case asserts its form through the query and must be exact in its layout; the first mismatch raises."""
    from millieye_amd import hip
    env, cases = W.CHILDREN[name]
    assert all(os.environ.get(k) == v for k, v in env.items())
    hip.load()
    for c in cases:
        _exact_case(hip, c, layouts=(c["oihw"],))
        print("ok", c["name"], c["form"], flush=True)


@pytest.mark.parametrize("name", sorted(W.CHILDREN))
def test_switch_only_forms_in_a_child_process(hip_lib, name):
    assert not _CHILD_LOST, f"not started: child {_CHILD_LOST[0]} ended by a signal or at its time limit"
    env, cases = W.CHILDREN[name]
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), name], cwd=ROOT, env=dict(os.environ, **env), timeout=240,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    except subprocess.TimeoutExpired as exc:
        _CHILD_LOST.append(name)
        raise AssertionError(f"child {name} ran into its time limit:\n" + (exc.stdout or b"").decode(errors="replace")[-4000:])
    out = proc.stdout.decode(errors="replace")
    if proc.returncode < 0 or proc.returncode in (134, 139):
        _CHILD_LOST.append(name)
    assert proc.returncode == 0, out[-4000:]
    assert sum(line.startswith("ok ") for line in out.splitlines()) == len(cases), out[-4000:]


if __name__ == "__main__":
    _child(sys.argv[1])
