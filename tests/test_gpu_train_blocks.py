"""-m gpu: the training building blocks (csrc/train.hip, csrc/train_h16.hip) one by one through the C ABI against the plain
float64 references of tests/train_block_refs.py (pinned to torch float64 autograd by tests/test_train_block_refs_cpu.py).

Two kinds of input:
* EXACT inputs - small integers (|v| <= 4) or multiples of 1/8, so that every product and partial sum is exactly representable
  in fp32 (and in bf16 / f16 storage): the result does not depend on the order of summation and the kernel must equal the
  float64 reference BIT FOR BIT.  This is what sees a dropped, doubled or misplaced term.
* REAL inputs (synth.uniform / synth.normal) for the rounding behaviour, with bars that come from the number format (the
  length-k dot-product bound k * 2^-24 * sum|a||b|, ulps of the float64 value rounded to fp32) or from stock torch fp32 on the
  CPU: 16 x its error against float64 relative to the output's largest magnitude, floor 4 * 2^-24 (different summation trees of
  the same length scatter by about the square root of the term count in units of 2^-24).  Both errors of every such case are
  written to profiles/train_blocks_errors.txt by the GPU run.

Where LeakyReLU decides by a sign, an element whose float64 pre-activation lies within rounding distance of 0 gets dy = 0 (a
condition on the inputs, computed from the reference alone): a flipped branch there is not a kernel error.
Every pitched buffer carries a sentinel in its padding columns, which must survive the call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (the rows-kernel child below runs this file as a script)
    sys.path.insert(0, ROOT)

from millieye_amd import synth  # noqa: E402
from tests import train_block_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 12345.0
U = 2.0 ** -24
FLOOR = 4 * U
ERRORS_FILE = os.path.join(ROOT, "profiles", "train_blocks_errors.txt")
_LOG = {}


def _p(t):
    return t.data_ptr() if t is not None else None


def _dev(a, pad=0, off=0, dtype=torch.float32):
    """numpy [rows, c] -> (buffer [rows, off + c + pad] filled with the sentinel, view [rows, c] into it) on the GPU."""
    a = np.asarray(a)
    rows, c = a.shape
    buf = torch.full((rows, off + c + pad), SENT, dtype=dtype, device="cuda")
    view = buf[:, off:off + c]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))
    return buf, view


def _pads_intact(buf, c, off=0):
    ok = bool((buf[:, :off] == SENT).all()) and bool((buf[:, off + c:] == SENT).all())
    assert ok, "a padding column was written"


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64) if t.dtype != torch.float64 else t.detach().cpu().numpy()


def _ints(rng, shape, lo=-4, hi=4):
    return rng.randint(lo, hi + 1, shape).astype(np.float32)


def _bits_equal(got, ref, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got != ref
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[bad][0]!r} vs {ref[bad][0]!r}"


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    m = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / (m if m > 0 else 1.0)


def _ulps(got32, ref64):
    """|got - fp32(ref)| in units of the spacing of fp32 at the reference."""
    ref32 = np.asarray(ref64, np.float64).astype(np.float32)
    sp = np.spacing(np.abs(ref32)).astype(np.float64)
    return float((np.abs(np.asarray(got32, np.float64) - ref32.astype(np.float64)) / sp).max()) if ref32.size else 0.0


def _bar(kernel_err, torch_err):
    return kernel_err <= max(16.0 * torch_err, FLOOR)


def _log(section, line):
    _LOG.setdefault(section, []).append(line)


@pytest.fixture(scope="module", autouse=True)
def _write_errors_file():
    """Sections of profiles/train_blocks_errors.txt are replaced by the tests that ran; the others stay."""
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
    head = ("# Measured by tests/test_gpu_train_blocks.py on an MI355X: per case the kernel's and stock torch fp32 CPU's largest\n"
            "# error against the float64 reference, relative to the output's largest magnitude (kernel / torch).\n"
            "# Bar: kernel <= max(16 x torch, 4 * 2^-24 = 2.4e-07).  Lines marked 'recorded' are not asserted.\n")
    try:
        with open(ERRORS_FILE, "w") as f:
            f.write(head)
            for name in sorted(sections):
                f.write(f"\n## {name}\n" + "\n".join(sections[name]) + "\n")
    except OSError:   # (a read-only checkout: the numbers are in the test output)
        pass


# ---------------------------------------------------------------------------------------------------------------------
# gemm / colsum
# ---------------------------------------------------------------------------------------------------------------------
DIMS = (1, 2, 10, 15, 16, 17, 63, 64, 65, 130, 490)


def _gemm_call(lib, hip, ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc):
    hip.check(lib.me_gemm_f32(ta, tb, m, n, k, alpha, _p(a), lda, _p(b), ldb, beta, _p(c), ldc, hip.stream_ptr()), "me_gemm_f32")


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm_vs_float64(hip_lib, ta, tb):
    """12 seeded (m, n, k) per transpose combination (48 in all, the corners 1 / 490 forced in), every operand pitched.
    Exact inputs with alpha = 2, beta = -1: bit-equal.  Real inputs with beta = 0 over a C full of NaN (C is not read): every
    element within k * 2^-24 * sum|a||b|.  k = 0 with beta != 0: C = beta * C."""
    from millieye_amd import hip
    lib = hip.lib()
    rng = np.random.RandomState(1000 + 2 * ta + tb)
    cases = [(1, 1, 1), (490, 490, 490), (1, 490, 65), (130, 1, 17)] + [tuple(int(v) for v in rng.choice(DIMS, 3)) for _ in range(8)]
    for i, (m, n, k) in enumerate(cases):
        pa, pb, pc = 1 + i % 3, 2 + i % 5, 1 + i % 4
        sa, sb = ((k, m) if ta else (m, k)), ((n, k) if tb else (k, n))
        a, b, c0 = _ints(rng, sa), _ints(rng, sb), _ints(rng, (m, n))
        abuf, av = _dev(a, pa)
        bbuf, bv = _dev(b, pb)
        cbuf, cv = _dev(c0, pc)
        _gemm_call(lib, hip, ta, tb, m, n, k, 2.0, av, sa[1] + pa, bv, sb[1] + pb, -1.0, cv, n + pc)
        _bits_equal(_np(cv), R.gemm(ta, tb, 2.0, a, b, -1.0, c0), f"gemm exact {ta}{tb} {m}x{n}x{k}")
        _pads_intact(cbuf, n)
        ar = synth.uniform(f"tb/ga{i}{ta}{tb}", sa, -1, 1)
        br = synth.normal(f"tb/gb{i}{ta}{tb}", sb)
        abuf, av = _dev(ar, pa)
        bbuf, bv = _dev(br, pb)
        cbuf, cv = _dev(np.full((m, n), np.nan, np.float32), pc)
        _gemm_call(lib, hip, ta, tb, m, n, k, 1.0, av, sa[1] + pa, bv, sb[1] + pb, 0.0, cv, n + pc)
        err = np.abs(_np(cv) - R.gemm(ta, tb, 1.0, ar, br))
        bound = k * U * R.gemm_abs(ta, tb, ar, br)
        assert (err <= bound).all(), f"gemm real {ta}{tb} {m}x{n}x{k}: worst err / bound {float((err / bound).max()):.3f}"
        _pads_intact(cbuf, n)
    c0 = _ints(rng, (17, 65))
    cbuf, cv = _dev(c0, 3)
    _gemm_call(lib, hip, ta, tb, 17, 65, 0, 1.0, None, 1, None, 1, 0.5, cv, 68)
    _bits_equal(_np(cv), 0.5 * c0.astype(np.float64), "k = 0")
    _pads_intact(cbuf, 65)


def test_colsum_vs_float64(hip_lib):
    """Every column-group width the launcher picks (64 down to 8) and fewer rows than row lanes, pitched."""
    from millieye_amd import hip
    lib = hip.lib()
    rng = np.random.RandomState(77)
    for cols in (1, 2, 10, 32, 64, 65, 130, 490):
        for rows in (0, 1, 7, 15, 16, 17, 1600, 5408, 21632):
            x = _ints(rng, (rows, cols))
            xbuf, xv = _dev(x, 3)
            obuf, ov = _dev(np.full((1, cols), 7.0, np.float32), 2)
            hip.check(lib.me_colsum_f32(_p(xv) if rows else None, cols + 3, rows, cols, _p(ov), hip.stream_ptr()), "me_colsum_f32")
            _bits_equal(_np(ov)[0], R.colsum(x), f"colsum exact {rows}x{cols}")
            _pads_intact(obuf, cols)
            if rows in (17, 5408, 21632):
                xr = synth.normal(f"tb/cs{rows}x{cols}", (rows, cols))
                xbuf, xv = _dev(xr, 3)
                hip.check(lib.me_colsum_f32(_p(xv), cols + 3, rows, cols, _p(ov), hip.stream_ptr()), "me_colsum_f32")
                err = np.abs(_np(ov)[0] - R.colsum(xr))
                assert (err <= rows * U * np.abs(xr.astype(np.float64)).sum(0)).all(), (rows, cols)


@pytest.mark.parametrize("m,n,pad_b", [(2, 64, 0), (32, 2, 0), (1, 10, 0), (10, 490, 6), (2, 256, 0)])
def test_train_path_gemm_on_both_sides_of_the_matrix_pipe_switch(hip_lib, m, n, pad_b):
    """train_path._gemm(A^T B) at the stage-3 backward's shapes: k < 64 runs me_gemm_f32, k >= 64 me_conv_wgrad_mfma_f32 - the
    same float64 product for both: bit-equal on exact inputs, the dot-product bound on real ones."""
    from millieye_amd import train_path as tp
    rng = np.random.RandomState(m * 1000 + n)
    for k in (63, 64, 65, 300, 2500):
        for real in (False, True):
            a = synth.uniform(f"tb/pa{m}{n}{k}", (k, m), -1, 1) if real else _ints(rng, (k, m))
            b = synth.normal(f"tb/pb{m}{n}{k}", (k, n)) if real else _ints(rng, (k, n))
            abuf, av = _dev(a)
            bbuf, bv = _dev(b, pad_b)
            c = torch.full((m, n), float("nan"), device="cuda")
            tp._gemm(1, 0, m, n, k, av, m, bv, n + pad_b, c, n)
            ref = R.gemm(1, 0, 1.0, a, b)
            if real:
                err, bound = np.abs(_np(c) - ref), k * U * R.gemm_abs(1, 0, a, b)
                assert (err <= bound).all(), f"{m}x{n}x{k}: worst err / bound {float((err / bound).max()):.3f}"
            else:
                _bits_equal(_np(c), ref, f"_gemm exact {m}x{n}x{k}")
            _pads_intact(bbuf, n)


# ---------------------------------------------------------------------------------------------------------------------
# activation / upsample / max-pool backward
# ---------------------------------------------------------------------------------------------------------------------
MAPS = [(2, 5, 7, 1), (2, 5, 7, 3), (3, 3, 5, 10), (2, 7, 5, 12), (2, 5, 3, 256)]
BIG_MAP = (4, 47, 49, 256)   # 2.36 M elements: more than the 8192 x 256 threads of the largest grid


@pytest.mark.parametrize("n,h,w,c", MAPS + [BIG_MAP])
def test_act_bwd_vs_float64(hip_lib, n, h, w, c):
    from millieye_amd import hip
    lib = hip.lib()
    rng = np.random.RandomState(c)
    rows = n * h * w
    for act in (hip.ACT_LINEAR, hip.ACT_LEAKY, hip.ACT_SIGMOID):
        if act == hip.ACT_SIGMOID:
            y = (1.0 / (1.0 + np.exp(-synth.normal(f"tb/ay{c}", (rows, c), 0, 3).astype(np.float64)))).astype(np.float32)
            dy = synth.uniform(f"tb/ad{c}", (rows, c), -1, 1)
        else:
            y, dy = _ints(rng, (rows, c)), _ints(rng, (rows, c))   # (y == 0 exactly under leaky: the slope, like torch)
        ybuf, yv = _dev(y, 1)
        gbuf, gv = _dev(dy, 5)
        xbuf, xv = _dev(np.full((rows, c), SENT, np.float32), 2)
        hip.check(lib.me_act_bwd_f32(_p(yv), c + 1, _p(gv), c + 5, _p(xv), c + 2, rows, c, act, hip.stream_ptr()), "me_act_bwd_f32")
        got = _np(xv)
        if act == hip.ACT_LINEAR:
            _bits_equal(got, R.act_bwd(y, dy, R.LINEAR), "linear")
        elif act == hip.ACT_LEAKY:   # one fp32 rounding of 0.1f * g
            want = np.where(y > 0, dy, np.float32(0.1) * dy).astype(np.float32)
            _bits_equal(got, want, "leaky")
            assert _ulps(got, R.act_bwd(y, dy, R.LEAKY)) == 0
        else:
            assert _ulps(got, R.act_bwd(y, dy, R.SIGMOID)) <= 2.0
        _pads_intact(xbuf, c)
    xbuf, xv = _dev(np.full((4, c), SENT, np.float32))
    hip.check(lib.me_act_bwd_f32(_p(xv), c, _p(xv), c, _p(xv), c, 0, c, hip.ACT_LEAKY, hip.stream_ptr()), "rows = 0")
    assert bool((xbuf == SENT).all())


@pytest.mark.parametrize("n,h,w,c", MAPS + [BIG_MAP])
def test_upsample2_bwd_vs_float64(hip_lib, n, h, w, c):
    from millieye_amd import hip
    rng = np.random.RandomState(c + 1)
    dy, dx0 = _ints(rng, (n, 2 * h, 2 * w, c)), _ints(rng, (n, h, w, c))
    gbuf, gv = _dev(dy.reshape(-1, c), 3)
    xbuf, xv = _dev(dx0.reshape(-1, c), 1)
    hip.check(hip.lib().me_upsample2_bwd_f32(_p(gv), c + 3, _p(xv), c + 1, n, h, w, c, hip.stream_ptr()), "me_upsample2_bwd_f32")
    _bits_equal(_np(xv).reshape(n, h, w, c), dx0 + R.upsample2_bwd(dy), "upsample2 bwd accumulates into dx")
    _pads_intact(xbuf, c)


POOLS = [(2, 2, 0, 0), (2, 1, 0, 1), (3, 1, 1, 0), (5, 1, 2, 0)]


@pytest.mark.parametrize("size,stride,pad,zero_ext", POOLS)
@pytest.mark.parametrize("data", ["ties", "negative"])
def test_maxpool_bwd_vs_float64(hip_lib, size, stride, pad, zero_ext, data):
    """Every (size, stride, pad, zero_ext) detector_train.py issues, on even and odd maps, data full of ties (integers from
    -2 .. 2 and constant patches) and all-negative data (under the zero extension the border zeros win and get nothing)."""
    from millieye_amd import hip
    maps = [(2, 6, 8, 1), (2, 5, 7, 3), (3, 7, 5, 10), (2, 6, 6, 12), (1, 5, 9, 256)]
    if (size, data) == (2, "ties") and stride == 2:
        maps.append(BIG_MAP)
    for n, h, w, c in maps:
        rng = np.random.RandomState(h * 100 + c + size)
        if data == "ties":
            x = _ints(rng, (n, h, w, c), -2, 2)
            x[0, : h // 2, : w // 2] = 1.0
        else:
            x = -_ints(rng, (n, h, w, c), 1, 3)
        ho, wo = R.maxpool_out_size(h, size, stride, pad, zero_ext), R.maxpool_out_size(w, size, stride, pad, zero_ext)
        dy, dx0 = _ints(rng, (n, ho, wo, c)), _ints(rng, (n, h, w, c))
        ibuf, iv = _dev(x.reshape(-1, c), 2)
        gbuf, gv = _dev(dy.reshape(-1, c), 1)
        xbuf, xv = _dev(dx0.reshape(-1, c), 5)
        hip.check(hip.lib().me_maxpool_bwd_f32(_p(iv), c + 2, _p(gv), c + 1, _p(xv), c + 5, n, h, w, c, size, stride, pad, zero_ext,
                                               hip.stream_ptr()), "me_maxpool_bwd_f32")
        _bits_equal(_np(xv).reshape(n, h, w, c), dx0 + R.maxpool_bwd(x, dy, size, stride, pad, zero_ext),
                    f"maxpool bwd {(size, stride, pad, zero_ext)} on {(n, h, w, c)} {data}")
        _pads_intact(xbuf, c)


# ---------------------------------------------------------------------------------------------------------------------
# eval-mode affine + activation backward, fp32
# ---------------------------------------------------------------------------------------------------------------------
def _affine_call(lib, hip, yv, ldy, gv, ldg, rows, c, scale, gamma, beta, act, dcv, lddc, ds, dg, ws):
    hip.check(lib.me_affine_act_bwd_f32(_p(yv), ldy, _p(gv), ldg, rows, c, _p(scale), _p(gamma), _p(beta), act, _p(dcv), lddc,
                                        _p(ds), _p(dg), ws.data_ptr(), hip.stream_ptr()), "me_affine_act_bwd_f32")


def _affine_case(rows, c, pad, off, bn, seed):
    """One shape through me_affine_act_bwd_f32: exact inputs (linear: dc, dshift, dgamma bit-equal; leaky: dc bit-equal to the
    fp32 product), fused form == split form == second run, then real inputs.  Returns the real-input figures.
    (pad, off): padding columns and a column offset of the views (off = 1: pointers 4 bytes off 16-byte alignment)."""
    from millieye_amd import hip
    lib = hip.lib()
    rng = np.random.RandomState(seed)
    ld = off + c + pad
    vec4 = int(c % 4 == 0 and ld % 4 == 0 and off % 4 == 0)
    cu = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()  # noqa: E731
    ws = torch.empty(max(int(lib.me_affine_bwd_workspace_bytes(rows, c)), 256), dtype=torch.uint8, device="cuda")
    new_out = lambda: (_dev(np.full((rows, c), SENT, np.float32), pad, off), torch.full((c,), SENT, device="cuda"),  # noqa: E731
                       torch.full((c,), SENT, device="cuda") if bn else None)
    # ---- exact inputs
    scale = (2.0 ** rng.randint(-2, 3, c)).astype(np.float32) * np.where(rng.rand(c) < 0.3, -1, 1).astype(np.float32)
    gamma = (2.0 ** rng.randint(-2, 3, c)).astype(np.float32) * np.where(rng.rand(c) < 0.3, -1, 1).astype(np.float32)
    beta = _ints(rng, (c,))
    z, dy = _ints(rng, (rows, c)), _ints(rng, (rows, c))
    dsc, dga, dbe = (cu(scale), cu(gamma), cu(beta)) if bn else (None, None, None)
    gbuf, gv = _dev(dy, pad, off)
    for act in (hip.ACT_LINEAR, hip.ACT_LEAKY):
        y = z if act == hip.ACT_LINEAR else np.where(z > 0, z, np.float32(0.1) * z).astype(np.float32)
        ybuf, yv = _dev(y, pad, off)
        (dcbuf, dcv), ds, dg = new_out()
        _affine_call(lib, hip, yv, ld, gv, ld, rows, c, dsc, dga, dbe, act, dcv, ld, ds, dg, ws)
        _pads_intact(dcbuf, c, off)
        g32 = dy if act == hip.ACT_LINEAR else np.where(y > 0, dy, np.float32(0.1) * dy).astype(np.float32)
        _bits_equal(_np(dcv), (g32 * scale if bn else g32).astype(np.float64), f"dc exact act {act}")
        if act == hip.ACT_LINEAR:
            # the pre-activation as the kernel sees it: y itself (c = (y - shift) / scale for any shift)
            ref = R.affine_act_bwd(z, dy, None, None, gamma if bn else None, beta if bn else None, R.LINEAR)
            assert max(np.abs(ref["dshift"]).max(), np.abs(ref["dgamma"]).max() if bn else 0) < 2 ** 24   # (exact in fp32)
            _bits_equal(_np(ds), ref["dshift"], "dshift exact")
            if bn:
                _bits_equal(_np(dg), ref["dgamma"], "dgamma exact")
        # the split form and a second run: the same bits
        (dcbuf2, dcv2), ds2, dg2 = new_out()
        _affine_call(lib, hip, yv, ld, gv, ld, rows, c, dsc, dga, dbe, act, dcv2, ld, None, None, ws)
        hip.check(lib.me_affine_bwd_sums_f32(ws.data_ptr(), rows, c, vec4, _p(ds2), _p(dg2), hip.stream_ptr()), "me_affine_bwd_sums_f32")
        assert torch.equal(dcbuf2, dcbuf) and torch.equal(ds2, ds) and (not bn or torch.equal(dg2, dg)), "split form"
        (dcbuf3, dcv3), ds3, dg3 = new_out()
        _affine_call(lib, hip, yv, ld, gv, ld, rows, c, dsc, dga, dbe, act, dcv3, ld, ds3, dg3, ws)
        assert torch.equal(dcbuf3, dcbuf) and torch.equal(ds3, ds) and (not bn or torch.equal(dg3, dg)), "second run"
    # ---- real inputs, leaky: F.batch_norm(training=False) + leaky_relu under autograd
    tag = f"tb/af{rows}x{c}"
    cv = synth.normal(tag + "c", (rows, c))
    dy = synth.uniform(tag + "d", (rows, c), -1, 1)
    if bn:
        gamma = synth.uniform(tag + "g", (c,), 0.5, 1.5) * np.where(np.arange(c) % 3 == 1, -1, 1).astype(np.float32)
        beta = synth.uniform(tag + "b", (c,), -0.5, 0.5)
        rm, rv = synth.uniform(tag + "m", (c,), -1, 1), synth.uniform(tag + "v", (c,), 0.5, 1.5)
        scale64 = gamma.astype(np.float64) / np.sqrt(rv.astype(np.float64) + 1e-5)
        shift64 = beta.astype(np.float64) - rm.astype(np.float64) * scale64
    else:
        gamma = beta = None
        scale64, shift64 = np.ones(c), synth.uniform(tag + "b", (c,), -0.5, 0.5).astype(np.float64)
    scale32, shift32 = scale64.astype(np.float32), shift64.astype(np.float32)   # what the forward folded (engine / _BnEval)
    z64 = cv.astype(np.float64) * scale32 + shift32
    dy = np.where(np.abs(z64) < 64 * U * (np.abs(cv * scale32) + np.abs(shift32)), np.float32(0), dy).astype(np.float32)
    y = np.where(z64 > 0, z64, R.SLOPE * z64).astype(np.float32)   # the stored output, rounded once
    ybuf, yv = _dev(y, pad, off)
    gbuf, gv = _dev(dy, pad, off)
    (dcbuf, dcv), ds, dg = new_out()
    _affine_call(lib, hip, yv, ld, gv, ld, rows, c, cu(scale32) if bn else None, cu(gamma) if bn else None,
                 cu(beta) if bn else None, hip.ACT_LEAKY, dcv, ld, ds, dg, ws)
    _pads_intact(dcbuf, c, off)
    ref_dc = R.affine_act_bwd(cv, dy, scale32 if bn else None, shift32, None, None, R.LEAKY)["dc"]   # the kernel's own operands
    ref = R.affine_act_bwd(cv, dy, scale64, shift64, gamma, beta, R.LEAKY)                         # autograd's semantics
    ct = torch.from_numpy(np.ascontiguousarray(cv.T)).reshape(1, c, rows, 1).requires_grad_(True)
    if bn:
        gt, bt = torch.from_numpy(gamma.copy()).requires_grad_(True), torch.from_numpy(beta.copy()).requires_grad_(True)
        zt = F.batch_norm(ct, torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy()), gt, bt, False, 0.1, 1e-5)
    else:
        gt, bt = None, torch.from_numpy(shift32.copy()).requires_grad_(True)
        zt = ct + bt.view(1, c, 1, 1)
    F.leaky_relu(zt, 0.1).backward(torch.from_numpy(np.ascontiguousarray(dy.T)).reshape(1, c, rows, 1))
    out = dict(dc_ulps=_ulps(_np(dcv), ref_dc), dshift=(_rel(_np(ds), ref["dshift"]), _rel(bt.grad.numpy(), ref["dshift"])))
    if bn:
        out["dgamma"] = (_rel(_np(dg), ref["dgamma"]), _rel(gt.grad.numpy(), ref["dgamma"]))
    return out


def _affine_report(section, name, res):
    line = f"{name}: dc {res['dc_ulps']:.2f} ulp"
    ok = res["dc_ulps"] <= 2.0
    for k in ("dshift", "dgamma"):
        if k in res:
            line += f", {k} {res[k][0]:.2e} / {res[k][1]:.2e}"
            ok = ok and _bar(*res[k])
    _log(section, line + ("" if ok else "  ABOVE THE BAR"))
    print(line)
    return ok


AFFINE_CASES = [  # rows, channels, pad, off, bn   (scalar kernel: channels 70, an odd pitch or a 4-byte pointer offset)
    (1, 70, 0, 0, True), (1, 64, 0, 0, True), (3, 32, 1, 0, True), (3, 128, 4, 0, False), (255, 70, 2, 0, False),
    (255, 64, 0, 0, True), (256, 32, 3, 1, True), (256, 128, 0, 0, True), (257, 64, 4, 0, True), (257, 8, 2, 1, False),
    (5408, 70, 0, 0, True), (5408, 128, 8, 0, True), (21632, 64, 0, 0, False), (21632, 32, 1, 0, True),
    (86528, 32, 0, 0, True), (86528, 70, 1, 0, True), (300000, 8, 0, 0, True), (300000, 8, 1, 0, True)]


@pytest.mark.parametrize("rows,c,pad,off,bn", AFFINE_CASES)
def test_affine_act_bwd_f32_vs_float64(hip_lib, rows, c, pad, off, bn):
    res = _affine_case(rows, c, pad, off, bn, seed=rows + c)
    assert _affine_report("affine_act_bwd_f32", f"rows {rows} channels {c} pad {pad} off {off} bn {int(bn)}", res)


def test_affine_act_bwd_f32_gamma_of_zero_gives_dgamma_zero(hip_lib):
    """xhat = (act^-1(y) - beta) / gamma cannot be recovered from the stored output when gamma == 0: the kernels write
    dgamma = 0 for that channel (include/millieye_hip.h says so); dc and dshift are unaffected."""
    from millieye_amd import hip
    lib = hip.lib()
    rng = np.random.RandomState(5)
    for rows, c, pad in ((300, 64, 0), (300, 70, 1)):
        y, dy = _ints(rng, (rows, c)), _ints(rng, (rows, c))
        gamma, beta = np.ones(c, np.float32), _ints(rng, (c,))
        gamma[[0, c - 1]] = 0.0
        ybuf, yv = _dev(y, pad)
        gbuf, gv = _dev(dy, pad)
        dcbuf, dcv = _dev(np.full((rows, c), SENT, np.float32), pad)
        ds, dg = torch.full((c,), SENT, device="cuda"), torch.full((c,), SENT, device="cuda")
        ws = torch.empty(max(int(lib.me_affine_bwd_workspace_bytes(rows, c)), 256), dtype=torch.uint8, device="cuda")
        cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        _affine_call(lib, hip, yv, c + pad, gv, c + pad, rows, c, cu(np.ones(c, np.float32)), cu(gamma), cu(beta), hip.ACT_LINEAR, dcv,
                     c + pad, ds, dg, ws)
        ref = R.affine_act_bwd(y, dy, None, None, np.where(gamma == 0, 1, gamma), beta, R.LINEAR)
        want = np.where(gamma == 0, 0.0, ref["dgamma"])
        _bits_equal(_np(dg), want, "dgamma")
        _bits_equal(_np(ds), ref["dshift"], "dshift")
        _bits_equal(_np(dcv), dy.astype(np.float64), "dc")


ROWS_KERNEL_CASES = [(1000, 32), (5408, 64), (777, 128), (1000, 256), (600, 512), (300, 1024), (300, 1280)]


def _rows_kernel_child(out_path):
    """Runs in a fresh process with MILLIEYE_AFFINE_ROWS=1 (read once, when the library first plans an affine backward)."""
    from millieye_amd import hip
    assert os.environ.get("MILLIEYE_AFFINE_ROWS") == "1"
    hip.load()
    table = []
    for rows, c in ROWS_KERNEL_CASES:
        res = _affine_case(rows, c, 0, 0, True, seed=rows + c)   # (raises on any exact-input mismatch)
        table.append([rows, c, res["dc_ulps"], res["dshift"][0], res["dshift"][1], res["dgamma"][0], res["dgamma"][1]])
    np.save(out_path, np.asarray(table, np.float64))


def test_affine_rows_kernel_in_a_child_process(hip_lib, tmp_path):
    """affine_bwd_rows_kernel<Q>, Q = 8 ... 256 (channels 32 ... 1280), is selected by MILLIEYE_AFFINE_ROWS=1 at the library's
    first use: one fresh child process runs the same case function (exact inputs bit-equal, split form, second run) and hands
    the real-input figures back."""
    out = str(tmp_path / "rows_kernel.npy")
    env = dict(os.environ, MILLIEYE_AFFINE_ROWS="1")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=ROOT, env=env, timeout=240,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert proc.returncode == 0, proc.stdout.decode(errors="replace")[-4000:]
    table = np.load(out)
    assert table.shape == (len(ROWS_KERNEL_CASES), 7)
    ok = True
    for rows, c, ulps, ds_k, ds_t, dg_k, dg_t in table.tolist():
        ok = _affine_report("affine_bwd_rows_kernel", f"rows {int(rows)} channels {int(c)}",
                            dict(dc_ulps=ulps, dshift=(ds_k, ds_t), dgamma=(dg_k, dg_t))) and ok
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit storage: affine backward and weight gradient
# ---------------------------------------------------------------------------------------------------------------------
HALVES = {"bf16": torch.bfloat16, "f16": torch.float16}


def _round_to(v64, dt):
    return torch.from_numpy(np.asarray(v64, np.float64)).to(torch.float32).to(dt)


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("rows,c,bn", [(2 * 52 * 52, 128, True), (3 * 13 * 13, 1024, True), (1000, 64, False), (77, 32, True)])
def test_affine_act_bwd_h16_vs_float64(hip_lib, half, rows, c, bn):
    """Inputs exactly representable in the storage type.  dc must be the float64 value rounded once (RNE) to the storage type;
    where the float64 value lies within 2^-22 (relative) of a rounding boundary of the storage type the neighbour is allowed
    (the kernel rounds 0.1f * g and * scale in fp32 first).  Such elements are at most 1e-5 of the inputs: the test moves dy to
    its neighbouring storage value where the reference lands in that zone, and asserts the remaining share."""
    from millieye_amd import hip
    lib = hip.lib()
    dt = HALVES[half]
    tag = f"tb/h{rows}x{c}"
    y16 = torch.from_numpy(synth.uniform(tag + "y", (rows, c), -2, 2)).to(dt)
    y16[0, :] = 0   # y == 0 exactly: the slope
    g16 = torch.from_numpy(synth.uniform(tag + "g", (rows, c), -1, 1)).to(dt)
    scale = synth.uniform(tag + "s", (c,), 0.5, 1.5) if bn else None
    gamma = synth.uniform(tag + "ga", (c,), 0.5, 1.5) * np.where(np.arange(c) % 3 == 1, -1, 1).astype(np.float32) if bn else None
    beta = synth.uniform(tag + "be", (c,), -0.5, 0.5) if bn else None
    y = y16.float().numpy()

    def reference(g16_):
        r = R.affine_act_bwd(y, g16_.float().numpy(), scale, None, None, None, R.LEAKY)   # (z = scale * c has the sign of y)
        lo, hi = _round_to(r["dc"] * (1 - 2.0 ** -22), dt), _round_to(r["dc"] * (1 + 2.0 ** -22), dt)
        return r, lo, hi

    assert scale is None or (scale > 0).all()   # (so that sign(z) == sign(y) in the reference call above)
    for _ in range(3):   # move dy off the zones
        r, lo, hi = reference(g16)
        near = lo != hi
        if not bool(near.any()):
            break
        bits = g16.view(torch.int16)
        bits[near] += 1
    r, lo, hi = reference(g16)
    near = (lo != hi).numpy()
    assert near.mean() <= 1e-5, f"{near.mean():.2e} of the elements lie in a double-rounding zone"
    # sums: from the pre-activation of the 16-bit y (leaky inverted in float64), fp32 parameters
    z = np.where(y > 0, y.astype(np.float64), y.astype(np.float64) / R.SLOPE)
    g = g16.float().numpy().astype(np.float64) * np.where(y > 0, 1.0, R.SLOPE)
    ref_ds = g.sum(0)
    ref_dg = (g * (z - beta) / gamma).sum(0) if bn else None
    cu = lambda a: torch.from_numpy(a).cuda() if a is not None else None  # noqa: E731
    yd, gd = y16.cuda(), g16.cuda()
    dc = torch.full((rows, c), 7.0, device="cuda", dtype=dt)
    ds, dg = torch.full((c,), SENT, device="cuda"), (torch.full((c,), SENT, device="cuda") if bn else None)
    ws = torch.empty(max(int(lib.me_affine_bwd_h16_workspace_bytes(rows, c)), 256), dtype=torch.uint8, device="cuda")
    dsc, dga, dbe = cu(scale), cu(gamma), cu(beta)
    hip.check(lib.me_affine_act_bwd_h16(_p(yd), c, _p(gd), c, rows, c, _p(dsc), _p(dga), _p(dbe), hip.ACT_LEAKY,
                                        _p(dc), c, _p(ds), _p(dg), ws.data_ptr(), hip.HALF_TYPES[dt], hip.stream_ptr()), "h16")
    got = dc.cpu()
    bad = ((got != lo) & (got != hi)).numpy()
    assert not bad.any(), f"dc: {int(bad.sum())} elements are not the float64 value rounded once, first {np.argwhere(bad)[0].tolist()}"
    # The sums accumulate fp32 terms in double, leave as float chunk partials and end in one float: per term one rounding of
    # 0.1f * g (dshift: <= 2^-24 |g| each, plus the partials' and the result's rounding <= 2 * 2^-24 sum|g|), and for dgamma five
    # more in xhat = (y * 10.f - beta) * (1.f / gamma), 10 * fp32(0.1) - 1 = 1.5e-8 included: 3 resp. 8 units of 2^-24 * sum|term|.
    for name, got_s, ref_s, bound in (("dshift", ds, ref_ds, 3 * U * np.abs(g).sum(0)),
                                      ("dgamma", dg, ref_dg, 8 * U * (np.abs(g) * (np.abs(z) + np.abs(beta)) / np.abs(gamma)).sum(0) if bn else None)):
        if ref_s is None:
            continue
        err = np.abs(_np(got_s) - ref_s)
        _log("affine_act_bwd_h16", f"{half} rows {rows} channels {c} {name}: {_rel(_np(got_s), ref_s):.2e}, worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (name, float((err / bound).max()))
    # linear, no scale: dc == dy, the sums of the 16-bit integers exactly
    rng = np.random.RandomState(rows)
    yi, gi = _ints(rng, (rows, c)), _ints(rng, (rows, c))
    yd, gd = torch.from_numpy(yi).to(dt).cuda(), torch.from_numpy(gi).to(dt).cuda()
    bi = _ints(rng, (c,)) if bn else None
    gai = (2.0 ** rng.randint(-2, 3, c)).astype(np.float32) if bn else None
    dga, dbe = cu(gai), cu(bi)
    hip.check(lib.me_affine_act_bwd_h16(_p(yd), c, _p(gd), c, rows, c, None, _p(dga), _p(dbe), hip.ACT_LINEAR,
                                        _p(dc), c, _p(ds), _p(dg), ws.data_ptr(), hip.HALF_TYPES[dt], hip.stream_ptr()), "h16 linear")
    ref = R.affine_act_bwd(yi, gi, None, None, gai, bi, R.LINEAR)
    _bits_equal(_np(dc), ref["dc"], "dc linear")
    _bits_equal(_np(ds), ref["dshift"], "dshift linear")
    if bn:
        _bits_equal(_np(dg), ref["dgamma"], "dgamma linear")


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,cin,cout,k,s", [(2, 26, 64, 128, 3, 1), (2, 26, 128, 256, 3, 2), (3, 13, 256, 128, 1, 1), (1, 20, 32, 64, 3, 1),
                                              (2, 13, 512, 256, 1, 1), (1, 52, 128, 128, 3, 1),
                                              (6, 13, 64, 64, 3, 1),     # several images per pixel slice
                                              (2, 13, 64, 8, 1, 1)])     # 1 x 1 with cout = 8
def test_conv_wgrad_h16_exact_vs_float64(hip_lib, half, n, h, cin, cout, k, s):
    from millieye_amd import hip
    dt = HALVES[half]
    pad = (k - 1) // 2
    ho = (h + 2 * pad - k) // s + 1
    rng = np.random.RandomState(h * cin + cout)
    x, dy = _ints(rng, (n, h, h, cin)), _ints(rng, (n, ho, ho, cout))
    got = hip.conv_wgrad_h16(torch.from_numpy(x).to(dt).cuda(), torch.from_numpy(dy).to(dt).cuda(), k, s, pad, oihw=True)
    _bits_equal(_np(got), R.conv_wgrad(x, dy, k, s, pad), "dW")


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm, training mode
# ---------------------------------------------------------------------------------------------------------------------
EPS = 1e-5


def _bn_ws(lib, c):
    ws_t = torch.empty(int(lib.me_bn_workspace_bytes(c)) + 256, dtype=torch.uint8, device="cuda")
    return ws_t, ws_t.data_ptr() + (-ws_t.data_ptr()) % 256


def _bn_case(rows, c, act, pads, running, momentum, null_out, mean, std, tag):
    """me_bn_train_fwd_f32 + me_bn_train_bwd_f32 on one shape: {output: (kernel error, torch fp32 CPU error)} against float64."""
    from millieye_amd import hip
    lib = hip.lib()
    x = (synth.normal(tag + "x", (rows, c)).astype(np.float64) * std + mean).astype(np.float32)
    gamma = synth.uniform(tag + "g", (c,), 0.5, 1.5) * np.where(np.arange(c) % 3 == 1, -1, 1).astype(np.float32)
    beta = synth.uniform(tag + "b", (c,), -0.5, 0.5)
    rm0, rv0 = synth.uniform(tag + "m", (c,), -1, 1), synth.uniform(tag + "v", (c,), 0.5, 1.5)
    dy = synth.uniform(tag + "d", (rows, c), -1, 1)
    f = R.bn_train_fwd(x, gamma, beta, EPS, momentum, rm0 if running else None, rv0 if running else None, act)
    if act == R.LEAKY:   # the branch of an element at rounding distance from 0 is not a kernel property
        big = np.abs(gamma) * (np.abs(x) + np.abs(f["mean"])) * f["rstd"] + np.abs(beta)
        dy = np.where(np.abs(f["z"]) < 64 * U * big, np.float32(0), dy).astype(np.float32)
    b = R.bn_train_bwd(x, dy, gamma, beta, EPS, act)
    # stock torch, fp32, CPU
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).reshape(1, c, rows, 1).requires_grad_(True)
    gt, bt = torch.from_numpy(gamma.copy()).requires_grad_(True), torch.from_numpy(beta.copy()).requires_grad_(True)
    rmt, rvt = (torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy())) if running else (None, None)
    zt = F.batch_norm(xt, rmt, rvt, gt, bt, True, momentum, EPS)
    yt = F.leaky_relu(zt, 0.1) if act == R.LEAKY else zt
    yt.backward(torch.from_numpy(np.ascontiguousarray(dy.T)).reshape(1, c, rows, 1))
    tvar, tmean = torch.var_mean(xt.detach(), dim=(0, 2, 3), unbiased=False)
    unrow = lambda t: t.detach().reshape(c, rows).t().numpy()  # noqa: E731
    torch_out = dict(y=unrow(yt), mean=tmean.numpy(), var=tvar.numpy(), dx=unrow(xt.grad), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy())
    if running:
        torch_out.update(running_mean=rmt.numpy(), running_var=rvt.numpy())
    # the kernels
    cu = lambda a: torch.from_numpy(np.asarray(a, np.float32).copy()).cuda()  # noqa: E731
    px, py, pdy, pdx = pads
    xbuf, xv = _dev(x, px)
    ybuf, yv = _dev(np.full((rows, c), SENT, np.float32), py)
    gbuf, gv = _dev(dy, pdy)
    dxbuf, dxv = _dev(np.full((rows, c), SENT, np.float32), pdx)
    dga, dbe, drm, drv = cu(gamma), cu(beta), (cu(rm0) if running else None), (cu(rv0) if running else None)
    sm, sv, sr = (torch.full((c,), SENT, device="cuda") for _ in range(3))
    dg, db = torch.full((c,), SENT, device="cuda"), torch.full((c,), SENT, device="cuda")
    ws_t, ws = _bn_ws(lib, c)
    hip.check(lib.me_bn_train_fwd_f32(_p(xv), c + px, rows, c, _p(dga), _p(dbe), EPS, momentum, _p(drm), _p(drv), act, _p(yv), c + py,
                                      _p(sm), _p(sv), _p(sr), ws, hip.stream_ptr()), "me_bn_train_fwd_f32")
    hip.check(lib.me_bn_train_bwd_f32(_p(xv), c + px, _p(gv), c + pdy, rows, c, _p(dga), _p(dbe), _p(sm), _p(sr), act,
                                      None if null_out == "dx" else _p(dxv), c + pdx, None if null_out == "dgamma" else _p(dg),
                                      None if null_out == "dbeta" else _p(db), ws, hip.stream_ptr()), "me_bn_train_bwd_f32")
    _pads_intact(ybuf, c)
    _pads_intact(dxbuf, c)
    _pads_intact(xbuf, c)
    got = dict(y=_np(yv), mean=_np(sm), var=_np(sv), dx=_np(dxv), dgamma=_np(dg), dbeta=_np(db))
    if running:
        got.update(running_mean=_np(drm), running_var=_np(drv))
    refs = dict(y=f["y"], mean=f["mean"], var=f["var"], dx=b["dx"], dgamma=b["dgamma"], dbeta=b["dbeta"],
                running_mean=f["running_mean"], running_var=f["running_var"])
    if null_out:
        untouched = dict(dx=dxbuf, dgamma=dg, dbeta=db)[null_out]
        assert bool((untouched == SENT).all())
        got.pop(null_out)
    return {k: (_rel(got[k], refs[k]), _rel(torch_out[k], refs[k])) for k in got}


def _bn_report(section, name, res, asserted=True):
    bad = [k for k, (ek, et) in res.items() if not _bar(ek, et)]
    line = f"{name}: " + ", ".join(f"{k} {ek:.1e} / {et:.1e}" for k, (ek, et) in res.items())
    line += "  (recorded)" if not asserted else ("  ABOVE THE BAR: " + " ".join(bad) if bad else "")
    _log(section, line)
    print(line)
    return not bad


BN_CHANNELS = (1, 10, 64, 65, 70, 128, 1024)
BN_ROWS = (2, 3, 63, 64, 65, 257, 5408, 21632)
BN_PADS = [(0, 0, 0, 0), (1, 2, 3, 5), (6, 0, 1, 2)]


@pytest.mark.parametrize("c", BN_CHANNELS)
def test_bn_train_fwd_bwd_vs_float64(hip_lib, c):
    """Every row count per channel count; pitches, activation, running statistics (NULL / momentum 0.1 / 0.03) and the NULL
    output cycle through the cases."""
    failed = []
    for i, rows in enumerate(BN_ROWS):
        j = i + BN_CHANNELS.index(c)
        act = (R.LEAKY, R.LINEAR)[j % 2]
        running, momentum = [(True, 0.1), (True, 0.03), (False, 0.1)][j % 3]
        null_out = (None, "dx", "dgamma", "dbeta")[j % 4]
        res = _bn_case(rows, c, act, BN_PADS[j % 3], running, momentum, null_out, 0.3, 1.0, f"tb/bn{rows}x{c}")
        name = f"rows {rows} channels {c} act {act} pads {BN_PADS[j % 3]} running {int(running)} momentum {momentum} null {null_out}"
        if not _bn_report("bn_train shapes", name, res):
            failed.append(name)
    assert not failed, failed


@pytest.mark.parametrize("std", [1.0, 1e-2])
@pytest.mark.parametrize("ratio", [0, 1, 3, 5, 10, 100, 1000])
def test_bn_train_with_a_mean_far_from_zero(hip_lib, ratio, std):
    """mean / std from 0 to 100 (asserted) and 1000 (recorded): the variance E[x^2] - mean^2 loses (mean / std)^2 * 2^-24
    wherever a partial sum is kept in float.  3 and 5 lie on the two sides of the kernel's per-channel switch (|mean| > 4 std)
    from the float-rounded chunk partials to the double ones."""
    failed = []
    for rows, c in ((5408, 10), (21632, 64), (86528, 10)):
        res = _bn_case(rows, c, R.LEAKY, BN_PADS[1], True, 0.1, None, ratio * std, std, f"tb/bm{rows}x{c}r{ratio}s{std}")
        name = f"mean/std {ratio} std {std} rows {rows} channels {c}"
        if not _bn_report("bn_train mean over std", name, res, asserted=ratio < 1000) and ratio < 1000:
            failed.append(name)
    assert not failed, failed


@pytest.mark.parametrize("c,act", [(10, R.LEAKY), (70, R.LINEAR), (128, R.LEAKY)])
def test_bn_train_bwd_dev_vs_the_plain_call(hip_lib, c, act):
    """Capacity 512, live rows from a device word: bit-equal to me_bn_train_bwd_f32 over the live rows, dx == 0 exactly behind
    them; live rows 0: dx, dgamma and dbeta are all written, and are 0."""
    from millieye_amd import hip
    lib = hip.lib()
    cap = 512
    x, dy = synth.normal(f"tb/dv{c}x", (cap, c)), synth.uniform(f"tb/dv{c}d", (cap, c), -1, 1)
    gamma, beta = synth.uniform(f"tb/dv{c}g", (c,), 0.5, 1.5), synth.uniform(f"tb/dv{c}b", (c,), -0.5, 0.5)
    cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dga, dbe = cu(gamma), cu(beta)
    xbuf, xv = _dev(x, 3)
    gbuf, gv = _dev(dy, 1)
    ws_t, ws = _bn_ws(lib, c)
    for live in (512, 511, 65, 2, 0):
        sm, sr = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        want_dx = torch.zeros((cap, c), device="cuda")
        want_dg, want_db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        if live:
            sv = torch.empty(c, device="cuda")
            y = torch.empty((live, c), device="cuda")
            hip.check(lib.me_bn_train_fwd_f32(_p(xv), c + 3, live, c, _p(dga), _p(dbe), EPS, 0.1, None, None, act, _p(y), c, _p(sm), _p(sv),
                                              _p(sr), ws, hip.stream_ptr()), "fwd")
            hip.check(lib.me_bn_train_bwd_f32(_p(xv), c + 3, _p(gv), c + 1, live, c, _p(dga), _p(dbe), _p(sm), _p(sr), act, _p(want_dx), c,
                                              _p(want_dg), _p(want_db), ws, hip.stream_ptr()), "plain bwd")
        dxbuf, dxv = _dev(np.full((cap, c), SENT, np.float32), 2)
        dg, db = torch.full((c,), SENT, device="cuda"), torch.full((c,), SENT, device="cuda")
        rows_dev = torch.tensor([live], dtype=torch.int32, device="cuda")
        hip.check(lib.me_bn_train_bwd_dev_f32(_p(xv), c + 3, _p(gv), c + 1, cap, _p(rows_dev), c, _p(dga), _p(dbe), _p(sm), _p(sr), act,
                                              _p(dxv), c + 2, _p(dg), _p(db), ws, hip.stream_ptr()), "dev bwd")
        assert torch.equal(dxv, want_dx), f"dx, live {live}"
        assert bool((dxv[live:] == 0).all())
        assert torch.equal(dg, want_dg) and torch.equal(db, want_db), f"dgamma / dbeta, live {live}"
        _pads_intact(dxbuf, c)


# ---------------------------------------------------------------------------------------------------------------------
# YOLO-loss gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,g,nc,m", [(2, 13, 12, 9), (3, 26, 80, 40), (1, 7, 3, 1), (2, 10, 12, 0)])
def test_yolo_loss_bwd_vs_float64_autograd(hip_lib, n, g, nc, m):
    """me_yolo_loss_bwd_f32 and me_yolo_loss_bwd_dev_f32 on the cases of test_yolo_loss_kernel_vs_the_torch_restatement, pitched
    raw and draw, from the dense tensors the forward kernel wrote: against float64 autograd through the same terms (bar: 16 x
    the fp32 CPU restatement's error), bit-equal to each other, exactly 0 in cells of neither mask."""
    import ctypes as C
    from millieye_amd import hip
    lib = hip.lib()
    rng = np.random.RandomState(100 * g + m)
    anchors = [(10, 13), (33, 23), (62, 45)]
    na, per = 3, 5 + nc
    raw = rng.normal(0, 1.5, (n, g, g, na * per)).astype(np.float32)
    tg = np.zeros((m, 6), np.float32)
    if m:
        tg[:, 0], tg[:, 1] = rng.randint(0, n, m), rng.randint(0, nc, m)
        tg[:, 2:4], tg[:, 4:6] = rng.uniform(0.02, 0.98, (m, 2)), rng.uniform(0.03, 0.5, (m, 2))
    if m >= 9:
        tg[3] = tg[1]
        tg[3, 1] = (tg[1, 1] + 1) % nc
        tg[3, 2] += 0.2 / g
        tg[5, 2:4] = np.floor(tg[5, 2:4] * g) / g
    rbuf, rv = _dev(raw.reshape(-1, na * per), 7, 3)
    pitch = na * per + 10
    stride = 32.0
    scaled = [float(np.float32(v)) for aw, ah in anchors for v in (aw / stride, ah / stride)]
    cells = (n, na, g, g)
    f32 = dict(device="cuda", dtype=torch.float32)
    obj, noobj = torch.empty(cells, device="cuda", dtype=torch.uint8), torch.empty(cells, device="cuda", dtype=torch.uint8)
    tx, ty, tw, th, tconf, cmask, ious = (torch.empty(cells, **f32) for _ in range(7))
    tcls = torch.empty(cells + (nc,), **f32)
    result = torch.zeros(16, **f32)
    ws = torch.zeros(int(lib.me_yolo_loss_workspace_bytes()), dtype=torch.uint8, device="cuda")
    tgd = torch.from_numpy(tg).cuda()
    hip.check(lib.me_yolo_loss_fwd_f32(_p(rv), pitch, n, g, na, nc, (C.c_float * 6)(*scaled), _p(tgd) if m else None, m, 0.5, 1.0, 100.0,
                                       _p(obj), _p(noobj), _p(tx), _p(ty), _p(tw), _p(th), _p(tcls), _p(tconf), _p(cmask), _p(ious),
                                       ws.data_ptr(), _p(result), hip.stream_ptr()), "me_yolo_loss_fwd_f32")
    res = result.tolist()
    assert res[15] == 0.0
    n_obj, n_noobj = res[13], res[14]
    dense = {k: v.cpu().numpy() for k, v in dict(obj=obj, noobj=noobj, tx=tx, ty=ty, tw=tw, th=th, tconf=tconf, tcls=tcls).items()}
    assert n_obj == dense["obj"].sum() and n_noobj == dense["noobj"].sum()
    args = (_p(obj), _p(noobj), _p(tx), _p(ty), _p(tw), _p(th), _p(tcls), _p(tconf))
    neither = ~((dense["obj"] != 0) | (dense["noobj"] != 0))
    for gs in (1.0, 0.37):
        ref = R.yolo_loss_grad(raw, dense, na, nc, 1.0, 100.0, gs)
        ref32 = R.yolo_loss_grad(raw, dense, na, nc, 1.0, 100.0, gs, dtype=torch.float32)
        d1buf, d1 = _dev(np.full((n * g * g, na * per), SENT, np.float32), 2, 1)
        hip.check(lib.me_yolo_loss_bwd_f32(_p(rv), pitch, n, g, na, nc, *args, n_obj, n_noobj, 1.0, 100.0, gs, _p(d1), na * per + 3,
                                           hip.stream_ptr()), "me_yolo_loss_bwd_f32")
        d2buf, d2 = _dev(np.full((n * g * g, na * per), SENT, np.float32), 2, 1)
        gsd = None if gs == 1.0 else torch.tensor([gs], **f32)
        hip.check(lib.me_yolo_loss_bwd_dev_f32(_p(rv), pitch, n, g, na, nc, *args, _p(result), 1.0, 100.0, _p(gsd), _p(d2), na * per + 3,
                                               hip.stream_ptr()), "me_yolo_loss_bwd_dev_f32")
        assert torch.equal(d1buf, d2buf), "the two entry points differ"
        _pads_intact(d1buf, na * per, 1)
        got = _np(d1).reshape(n, g, g, na * per)
        ek, et = _rel(got, ref), _rel(ref32, ref)
        line = f"n {n} g {g} classes {nc} targets {m} grad_scale {gs}: {ek:.2e} / {et:.2e}"
        _log("yolo_loss_bwd", line)
        print(line)
        assert _bar(ek, et), line
        assert np.all(got.reshape(n, g, g, na, per).transpose(0, 3, 1, 2, 4)[neither] == 0)
    _pads_intact(rbuf, na * per, 3)


if __name__ == "__main__":
    _rows_kernel_child(sys.argv[1])
