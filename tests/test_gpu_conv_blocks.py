"""-m gpu: the fused inference convolutions (``me_conv2d_f32``, ``me_conv2d_h16``, ``me_bneck_h16``) tile id by tile id through
the C ABI against the plain float64 reference of tests/conv_refs.py (pinned to torch float64 by tests/test_conv_refs_cpu.py,
which also checks the arithmetic facts the shapes below rest on).

A. fp32 precision bar.  Real inputs, weights N(0, 2/K), two input sets (centred / like post-leaky activations).  Per case
   e = max |got - ref64| / abs_sum64, and e(kernel) <= min(16 x e(stock torch fp32 CPU), K * 2^-24).  Both numbers of every case
   go to profiles/conv_errors.txt.  The 16-bit path joins with its fp32-output form on operands rounded first.
B. Poison and sentinels.  The test owns every buffer (descriptors, not the wrappers): everything a launch may address but must
   not use - channels beside the x / residual slices, guard bands around every operand, the whole split-K workspace, the output
   and its neighbours - holds NaN before the launch.  The outputs must be finite and equal, bit for bit, the same tile id on
   clean dense buffers; every other byte of y's allocation and the workspace's bands must be untouched.  Locality: one NaN
   pixel (or weight row) changes exactly its receptive field (its output channel), compared with the run that has zeros there.
C. The 2^31 guards from both sides and operands past 2^32 bytes.  Integer-valued inputs make every fp32 partial sum exact, so
   the kernel must EQUAL the float64 reference on sampled row bands and, on the whole tensor, the same tile id run band by
   band (small offsets) - just below a guard on the forced tile, just above it through tile 0, and the forced ids whose
   launcher checks the guard must refuse."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import conv_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS_FILE = os.path.join(ROOT, "profiles", "conv_errors.txt")
NAN = float("nan")
F32 = torch.float32
HALVES = {"bf16": torch.bfloat16, "f16": torch.float16}
YL, YR = 8, 24    # poisoned channels to the left / right of the y and residual slices
_LOG = {}


def _p(t):
    return t.data_ptr() if t is not None else None


def _dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _pitch(t):
    return t.shape[-1] if t.is_contiguous() else t.stride(-2)


# --------------------------------------------------------------------------------------
# descriptor-level launches: every buffer is the caller's
# --------------------------------------------------------------------------------------
def _desc_common(d, x, wgt, scale, shift, res, y, k, s, pad, act, ups, tile, split, nchw=False):
    if nchw:
        n, cin, h, w = x.shape
    else:
        n, h, w, cin = x.shape
    d.x, d.wgt, d.scale, d.shift, d.res, d.y = _p(x), _p(wgt), _p(scale), _p(shift), _p(res), _p(y)
    d.x_pitch = cin if nchw else _pitch(x)
    d.res_pitch = _pitch(res) if res is not None else 0
    d.y_pitch = _pitch(y)
    d.n, d.h, d.w, d.cin, d.cout = n, h, w, cin, wgt.shape[0]
    d.ksize, d.stride, d.pad = k, s, pad
    d.ho, d.wo = R.out_size(h, k, s, pad), R.out_size(w, k, s, pad)
    d.act, d.upsample, d.x_nchw, d.tile, d.split_k = act, ups, 1 if nchw else 0, tile, split
    return d


def _launch_f32(hip, x, wgt, scale, shift, k, s, pad, act, y, res=None, ups=1, tile=0, split=1, nchw=False, wgt_tiled=None,
                counters=None, tap_masks=None):
    """me_conv2d_f32 on the caller's buffers, with a NaN workspace of exactly the size the library asks for between guard bands.
    Returns the workspace's guard check (None when the launch needs no workspace)."""
    d = _desc_common(hip.ConvDesc(), x, wgt, scale, shift, res, y, k, s, pad, act, ups, tile, split, nchw)
    d.wgt_tiled = _p(wgt_tiled)
    if tap_masks is not None:
        d.tap_mask_cols = int(tap_masks[0])
        for i, m in enumerate(tap_masks[1]):
            d.tap_mask[i] = int(m)
    check = None
    need = int(hip.lib().me_conv2d_workspace_bytes(C.byref(d))) if tap_masks is None else 0
    if need > 0:
        assert need % 4 == 0
        buf, check = R.banded((need // 4,), F32, 64, 1024, NAN, "cuda")
        d.workspace, d.workspace_bytes = buf.data_ptr(), need
        if counters is not None:
            d.tile_counters, d.tile_counters_len = counters.data_ptr(), counters.numel()
    hip.check(hip.lib().me_conv2d_f32(C.byref(d), hip.stream_ptr()), "me_conv2d_f32")
    torch.cuda.synchronize()
    return check


def _launch_h16(hip, x, wgt, scale, shift, k, s, pad, act, y, res=None, ups=1, tile=0, split=1, wgt_tiled=None, tap_masks=None):
    d = _desc_common(hip.Conv16Desc(), x, wgt, scale, shift, res, y, k, s, pad, act, ups, tile, split)
    d.y_f32 = 1 if y.dtype == F32 else 0
    d.half_type = hip.HALF_TYPES[x.dtype]
    d.wgt_tiled = _p(wgt_tiled)
    if tap_masks is not None:
        d.tap_mask_cols = int(tap_masks[0])
        for i, m in enumerate(tap_masks[1]):
            d.tap_mask[i] = int(m)
    check = None
    need = int(hip.lib().me_conv2d_h16_workspace_bytes(C.byref(d))) if tap_masks is None else 0
    if need > 0:
        buf, check = R.banded(((need + 3) // 4,), F32, 64, 1024, NAN, "cuda")
        d.workspace, d.workspace_bytes = buf.data_ptr(), need
    hip.check(hip.lib().me_conv2d_h16(C.byref(d), hip.stream_ptr()), "me_conv2d_h16")
    torch.cuda.synchronize()
    return check


def _sliced(t, left, right, fill=NAN):
    """A copy of the NHWC tensor ``t`` as the channel slice [left, left + c) of a wider buffer inside one banded allocation:
    (view, guard check).  Neighbour channels and bands hold ``fill``."""
    c = t.shape[-1]
    buf, check = R.banded(tuple(t.shape[:-1]) + (left + c + right,), t.dtype, 256, 256, fill, "cuda")
    view = buf[..., left:left + c]
    view.copy_(t)
    return view, check


def _band_copy(t, lead=256, tail=256):
    buf, check = R.banded(tuple(t.shape), t.dtype, lead, tail, NAN, "cuda")
    buf.copy_(t)
    return buf, check


def _poisoned_y(shape, cout, dtype):
    """(view [.., cout] into a NaN allocation with NaN neighbours and bands, the allocation's flat tensor)."""
    buf, check = R.banded(tuple(shape[:-1]) + (YL + cout + YR,), dtype, 256, 256, NAN, "cuda")
    return buf[..., YL:YL + cout], check.raw


def _assert_y(view, raw, clean, what):
    """The slice is finite and equals ``clean`` bit for bit; every other element of the allocation still holds its NaN."""
    assert bool(torch.isfinite(view.float()).all()), f"{what}: non-finite outputs ({int((~torch.isfinite(view.float())).sum())})"
    assert _same_bits(view, clean), f"{what}: {int((_bits(view) != _bits(clean)).sum())} outputs differ from the clean dense run"
    cout = view.shape[-1]
    expect, chk = R.banded(tuple(view.shape[:-1]) + (YL + cout + YR,), view.dtype, 256, 256, NAN, "cuda")
    expect[..., YL:YL + cout].copy_(clean)
    assert bool(torch.equal(_bits(raw), _bits(chk.raw))), f"{what}: bytes outside the output slice were written"


# --------------------------------------------------------------------------------------
# part A
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _part_a_reference(family, name):
    cases = R.H16_F32OUT if family == "h16_f32out" else R.FAMILIES[family][1]
    case = next(c for c in cases if c["name"] == name)
    return case, R.real_inputs(f"A/{family}/{name}/", case, case["inputs"])


@functools.lru_cache(maxsize=None)
def _part_a_yardstick(family, name, half=None):
    """(ref64, abs_sum64, e(torch fp32)) - computed once per case, shared by every tile id, never modified."""
    case, (x, wg, scale, shift, res) = _part_a_reference(family, name)
    if half is not None:
        x, wg = R.round_to(x, half).float().numpy(), R.round_to(wg, half).float().numpy()
    k, s, pad, act, ups = case["k"], case["s"], case["pad"], case["act"], case["ups"]
    ref = R.fused_conv64(x, wg, scale, shift, k, s, pad, act, res, ups)
    den = R.abs_sum64(x, wg, scale, shift, k, s, pad, res, ups)
    e_t = R.rel_err(R.torch_fp32(x, wg, scale, shift, k, s, pad, act, res, ups), ref, den)
    ref.setflags(write=False)
    den.setflags(write=False)
    return ref, den, e_t


def _record(section, label, e_k, e_t, kk):
    line = f"{label:<44s} kernel {e_k:.3e}  torch {e_t:.3e}  ratio {e_k / e_t:7.2f}  K*2^-24 {kk * R.U24:.3e}"
    print(line)
    _LOG.setdefault(section, []).append(line)
    return e_k <= R.bar(e_t, kk)


@pytest.fixture(scope="module", autouse=True)
def _write_errors_file():
    """Sections of profiles/conv_errors.txt are replaced by the tests that ran; the others stay."""
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
    head = ("# Measured by tests/test_gpu_conv_blocks.py on an MI355X: per kernel family, tile id and case the largest error of the\n"
            "# kernel and of stock torch fp32 on the CPU against the float64 reference, relative to abs_sum64 (conv(|x|, |w|) |scale| +\n"
            "# |shift| + |res|), their ratio and the format bound K * 2^-24.  Bar: kernel <= min(16 x torch, K * 2^-24).\n")
    try:
        with open(ERRORS_FILE, "w") as f:
            f.write(head)
            for name in sorted(sections):
                f.write(f"\n## {name}\n" + "\n".join(sections[name]) + "\n")
    except OSError:
        pass


_A_PARAMS = [(fam, tile) for fam, (tiles, _cases) in R.FAMILIES.items() for tile in tiles]


@pytest.mark.parametrize("family,tile", _A_PARAMS, ids=[f"{f}-{t}" for f, t in _A_PARAMS])
def test_fp32_precision_bar(hip_lib, family, tile):
    """Part A: every forced fp32 tile id on its family's cases; a split launch meets the bar of the whole one."""
    from millieye_amd import hip
    missed = []
    for case in R.FAMILIES[family][1]:
        _case, (x, wg, scale, shift, res) = _part_a_reference(family, case["name"])
        ref, den, e_t = _part_a_yardstick(family, case["name"])
        k, s, pad, act, ups = case["k"], case["s"], case["pad"], case["act"], case["ups"]
        xd = _dev(x.transpose(0, 3, 1, 2)) if case["nchw"] else _dev(x)
        got = hip.conv2d(xd, _dev(wg), _dev(scale), _dev(shift), k, s, pad, act, residual=_dev(res) if res is not None else None,
                         upsample=ups, x_nchw=case["nchw"], tile=tile, split_k=case["split"])
        torch.cuda.synchronize()
        e_k = R.rel_err(got.cpu().numpy(), ref, den)
        if not _record(f"fp32 {family}", f"tile {tile:>3d} {case['name']} split {case['split']}", e_k, e_t, k * k * case["cin"]):
            missed.append((case["name"], e_k, e_t))
    assert not missed, f"{family} tile {tile}: (case, e(kernel), e(torch fp32)) over the bar: {missed}"


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_h16_fp32_output_precision_bar(hip_lib, half):
    """Part A for the fp32-output form of me_conv2d_h16: operands rounded to the storage type first, then the fp32 bar."""
    from millieye_amd import hip
    dt = HALVES[half]
    missed = []
    for case in R.H16_F32OUT:
        _case, (x, wg, scale, shift, res) = _part_a_reference("h16_f32out", case["name"])
        ref, den, e_t = _part_a_yardstick("h16_f32out", case["name"], dt)
        k, s, pad, act = case["k"], case["s"], case["pad"], case["act"]
        for tile in (0, 1, 3):
            got = hip.conv2d_h16(R.round_to(x, dt).cuda(), R.round_to(wg, dt).cuda(), _dev(scale), _dev(shift), k, s, pad, act,
                                 residual=_dev(res) if res is not None else None, y_f32=True, tile=tile, split_k=1 if tile else 0)
            torch.cuda.synchronize()
            e_k = R.rel_err(got.cpu().numpy(), ref, den)
            if not _record(f"{half} operands, fp32 output", f"tile {tile:>3d} {case['name']}", e_k, e_t, k * k * case["cin"]):
                missed.append((case["name"], tile, e_k, e_t))
    assert not missed, f"(case, tile, e(kernel), e(torch fp32)) over the bar: {missed}"


# --------------------------------------------------------------------------------------
# part B: poison
# --------------------------------------------------------------------------------------
def _operands(case, seed, dtype=F32):
    """Part B operands: any finite values do (the comparison is with the same kernel on clean buffers)."""
    x, wg, scale, shift, res = R.real_inputs(f"B/{case['name']}/{seed}/", case, "centred")
    return (_dev(x, dtype), _dev(wg, dtype), _dev(scale), _dev(shift), _dev(res, dtype) if res is not None else None)


def _poison_f32(hip, case, tile, counters=False, tap_masks=None, operands=None, wgt_poisoned=None):
    """One case on one fp32 tile id: clean dense run through the wrapper, then the same descriptor on poisoned buffers."""
    x, wg, scale, shift, res = operands if operands is not None else _operands(case, 0)
    k, s, pad, act, ups, split = case["k"], case["s"], case["pad"], case["act"], case["ups"], case["split"]
    what = f"tile {tile} {case['name']}"
    clean = hip.conv2d(x, wg, scale, shift, k, s, pad, act, residual=res, upsample=ups, tile=tile, split_k=split,
                       in_launch_reduce=counters, tap_masks=tap_masks)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(clean).all()), what
    checks = []
    xs, c = _sliced(x, case.get("xl", 0), case.get("xr", 0)); checks.append(("x", c))   # noqa: E702
    wsrc = wg if wgt_poisoned is None else wgt_poisoned
    wb, c = _band_copy(wsrc); checks.append(("wgt", c))   # noqa: E702
    wt = None
    if tile >= 100:
        wt, c = _band_copy(hip.tile_weights_f32(wg)); checks.append(("wgt_tiled", c))   # noqa: E702
    sb, c = _band_copy(scale, 64, 64); checks.append(("scale", c))   # noqa: E702
    hb, c = _band_copy(shift, 64, 64); checks.append(("shift", c))   # noqa: E702
    rs = None
    if res is not None:
        rs, c = _sliced(res, YL, YR); checks.append(("res", c))   # noqa: E702
    y, raw = _poisoned_y(tuple(clean.shape), clean.shape[-1], F32)
    cnt = torch.zeros(1 << 16, dtype=torch.int32, device="cuda") if counters else None
    ws_check = _launch_f32(hip, xs, wb, sb, hb, k, s, pad, act, y, res=rs, ups=ups, tile=tile, split=split, wgt_tiled=wt,
                           counters=cnt, tap_masks=tap_masks)
    _assert_y(y, raw, clean, what)
    for name, c in checks:
        c(f"{what}: {name}")
    if ws_check is not None:
        ws_check(f"{what}: workspace")
    if cnt is not None:
        assert int(cnt.abs().sum()) == 0, f"{what}: arrival counters must be back at zero"
    return ws_check is not None


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 7, 21, 22, 23, 24, 25, 6, 51, 52, 53, 54, 55, 31])
def test_poison_f32_per_tap_tiles(hip_lib, tile):
    """Buffer-addressed, DMA and register-staged tiles: ragged channel chunks (cin 24 / 40; 48 on the buffer kernel, which needs
    cin % 16), a 16-channel slice with NaN on each side, ragged cout (72 / 255), ragged last tile (M = 286), a map smaller than a
    tile, stride 2, 5x5 / pad 2, split-K 3 with residual and upsampling through the reduce pass (NaN workspace)."""
    from millieye_amd import hip
    cases = R.POISON_BUFFER if tile <= 7 and tile != 6 else R.POISON_GENERAL
    used_ws = 0
    for case in cases:
        used_ws += _poison_f32(hip, case, tile)
    assert used_ws >= 1, "the split-K case must have gone through a workspace"
    if tile <= 7 and tile != 6:   # slabs summed inside the launch: same bits, counters back at zero
        assert _poison_f32(hip, cases[-1], tile, counters=True)


@pytest.mark.parametrize("tile", [41, 42, 43, 44, 45, 47])
def test_poison_f32_tail_split(hip_lib, tile):
    """The tail split with fewer than 256 tiles (everything is tail) and with more (whole tiles and tail pieces in one launch),
    two-pass and in-launch reduction, compact slabs in a NaN workspace of exactly the size the library asks for."""
    from millieye_amd import hip
    assert _poison_f32(hip, R.POISON_TAIL_SMALL, tile)
    assert _poison_f32(hip, R.POISON_TAIL_SMALL, tile, counters=True)
    n, cout = R.POISON_TAIL_LARGE[tile]
    large = R._b(f"tail_large{tile}", n, 52, 52, 32, cout, 3, 1, R.LEAKY, res=True, split=3, xl=32)
    assert _poison_f32(hip, large, tile)


def test_poison_f32_weight_stationary(hip_lib):
    """Tiles 50 / 60: rows behind the last pixel and ragged cout rows come from the DMA range check; every persistent workgroup
    walks more tiles than its LDS ring has slots (on this device's CU count), so slots are refilled while others are read."""
    from millieye_amd import hip
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for case in R.POISON_WS1 + R.POISON_WS3:
        turns, nslot = R.ws_ring_turns(case, cus)
        assert turns > nslot, f"{case['name']}: {turns} tiles per workgroup do not wrap a ring of {nslot} slots on {cus} CUs"
    for case in R.POISON_WS1:
        _poison_f32(hip, case, 50)
    for case in R.POISON_WS3:
        _poison_f32(hip, case, 60)


@pytest.mark.parametrize("tile", R.P8_128 + R.P8_256)
def test_poison_f32_patch_resident(hip_lib, tile):
    """The patch-resident tiles on 5 x 13 x 13 (two images per tile: pad rows between them must be zeros, not the neighbour
    image or NaN) and on one tiny image, with the tiled weight copy between NaN bands."""
    from millieye_amd import hip
    for case in R.POISON_P8:
        _poison_f32(hip, case, tile)


def _parity_operands(cin, cout, n, h, w, dtype=F32):
    from millieye_amd import synth
    from millieye_amd.detector_train import _PARITY_TAP_MASKS, _parity_weights
    wf = torch.from_numpy(synth.uniform(f"B/par/w{cin}", (cout, 3, 3, cin), -1, 1)).cuda() / (9 * cin) ** 0.5
    dc = torch.from_numpy(synth.uniform(f"B/par/dc{cin}", (n, h, w, cout), -1, 1)).cuda()
    pw = _parity_weights(wf)                              # [4 * cin, 2, 2, cout]: four classes of cin output channels
    bad = pw.clone().reshape(4, cin, 4, cout)
    for cls, mask in enumerate(_PARITY_TAP_MASKS):
        for t in range(4):
            if not (mask >> t) & 1:
                assert bool((bad[cls, :, t] == 0).all())
                bad[cls, :, t] = NAN                      # a skipped tap: the kernel must never multiply it
    return dc.to(dtype), pw.to(dtype), bad.reshape(pw.shape).to(dtype), _PARITY_TAP_MASKS


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
def test_poison_f32_skipped_taps(hip_lib, tile):
    """The 2x2 / pad 1 convolution with the parity tap masks: the (class, tap) pairs the masks skip hold NaN weights instead of
    their structural zeros (and x sits between NaN channels) - a skipped tap that is loaded and multiplied shows at once."""
    from millieye_amd import hip
    cin, cout = 128, 48          # classes of 128 output channels: every tile width divides them
    dc, pw, bad, masks = _parity_operands(cin, cout, 2, 7, 9)
    case = R._b("parity2x2", 2, 7, 9, cout, 4 * cin, 2, 1, R.LINEAR, pad=1, xl=16, xr=16)
    ones, zeros = torch.ones(4 * cin, device="cuda"), torch.zeros(4 * cin, device="cuda")
    _poison_f32(hip, case, tile, tap_masks=(cin, masks), operands=(dc, pw, ones, zeros, None), wgt_poisoned=bad)


def _poison_h16(hip, case, tile, dt, p8=False):
    x, wg, scale, shift, res = _operands(case, 1, dt)
    k, s, pad, act, ups, split = case["k"], case["s"], case["pad"], case["act"], case["ups"], case["split"]
    what = f"{dt} tile {tile} {case['name']}"
    clean = hip.conv2d_h16(x, wg, scale, shift, k, s, pad, act, residual=res, upsample=ups, tile=tile, split_k=split)
    torch.cuda.synchronize()
    checks = []
    xs, c = _sliced(x, case.get("xl", 0), case.get("xr", 0)); checks.append(("x", c))   # noqa: E702
    wb, c = _band_copy(wg); checks.append(("wgt", c))   # noqa: E702
    wt = None
    if tile >= 100:
        wt, c = _band_copy(hip.tile_weights_h16(wg)); checks.append(("wgt_tiled", c))   # noqa: E702
    sb, c = _band_copy(scale, 64, 64); checks.append(("scale", c))   # noqa: E702
    hb, c = _band_copy(shift, 64, 64); checks.append(("shift", c))   # noqa: E702
    rs = None
    if res is not None:
        rs, c = _sliced(res, YL, YR); checks.append(("res", c))   # noqa: E702
    y, raw = _poisoned_y(tuple(clean.shape), clean.shape[-1], dt)
    ws_check = _launch_h16(hip, xs, wb, sb, hb, k, s, pad, act, y, res=rs, ups=ups, tile=tile, split=split, wgt_tiled=wt)
    _assert_y(y, raw, clean, what)
    for name, c in checks:
        c(f"{what}: {name}")
    if ws_check is not None:
        ws_check(f"{what}: workspace")
    return ws_check is not None


H16_POISON = [
    R._b("h_cin32_cout72", 2, 13, 11, 32, 72, 3, 1, R.LEAKY, xl=8, xr=24),
    R._b("h_cin96_cout255_k1", 2, 13, 11, 96, 255, 1, 1, R.LINEAR, res=True, xl=32),
    R._b("h_tiny_slices", 1, 5, 7, 64, 72, 3, 1, R.LEAKY, xl=32, xr=32),
    R._b("h_stride2", 2, 13, 11, 64, 72, 3, 2, R.LEAKY, xl=32),
    R._b("h_k5_pad2", 1, 9, 7, 32, 40, 5, 1, R.LEAKY, xr=16),
    R._b("h_split3_res_ups", 2, 13, 11, 64, 72, 3, 1, R.LEAKY, res=True, ups=2, split=3, xl=16),
]
H16_POISON_P8 = [R._b("hp8_two_per_tile", 5, 13, 13, 64, 256, 3, 1, R.LEAKY, res=True, xl=32, xr=32),
                 R._b("hp8_tiny", 1, 5, 7, 32, 256, 3, 1, R.LINEAR),
                 R._b("hp8_split2", 3, 13, 13, 96, 256, 3, 1, R.LEAKY, res=True, split=2, xl=32)]


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 11, 12, 13, 14])
def test_poison_h16_per_tap_tiles(hip_lib, tile, half):
    from millieye_amd import hip
    used_ws = 0
    for case in H16_POISON:
        used_ws += _poison_h16(hip, case, tile, HALVES[half])
    assert used_ws >= 1


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("tile", [121, 131, 221, 100, 200, 431, 621, 731, 821])
def test_poison_h16_patch_resident(hip_lib, tile, half):
    from millieye_amd import hip
    splits = tile in (121, 131, 221, 100, 431, 621, 731)    # the ids the K split of the patch tiles is tested on
    used_ws = sum(_poison_h16(hip, case, tile, HALVES[half]) for case in H16_POISON_P8 if splits or case["split"] == 1)
    assert used_ws >= (1 if splits else 0)   # (the split case: NaN slabs)


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_poison_h16_streaming_and_wave_split_tiles(hip_lib, half):
    """Tile 50 (1x1, weights in registers), tile 60 (3x3, cin 32 / 64) and the small-batch tiles 40 / 41 (K split over the waves)."""
    from millieye_amd import hip
    dt = HALVES[half]
    _poison_h16(hip, R._b("h50_ragged", 9, 13, 11, 128, 128, 1, 1, R.LEAKY, xl=32, xr=32), 50, dt)
    _poison_h16(hip, R._b("h50_small", 1, 5, 5, 64, 32, 1, 1, R.LINEAR, xl=8), 50, dt)
    _poison_h16(hip, R._b("h60_s1", 3, 37, 29, 32, 64, 3, 1, R.LEAKY, res=True, xl=32), 60, dt)
    _poison_h16(hip, R._b("h60_s2", 2, 13, 11, 64, 128, 3, 2, R.LINEAR, xr=16), 60, dt)
    for tile in (40, 41):
        _poison_h16(hip, R._b("hkw_deep", 1, 13, 13, 512, 320, 3, 1, R.LEAKY, res=True, xl=32), tile, dt)
        _poison_h16(hip, R._b("hkw_k1_255", 1, 13, 11, 256, 255, 1, 1, R.LINEAR, xr=32), tile, dt)


BNECK_POISON = {1: (3, 13, 11, 64, 128, 256), 3: (2, 20, 31, 32, 64, 128), 4: (2, 20, 31, 32, 64, 128)}   # tile: n, h, w, cin, cmid, cout


def _bneck_operands(tile, dt):
    from millieye_amd import synth
    n, h, w, cin, cmid, cout = BNECK_POISON[tile]
    tag = f"B/bneck{tile}/"
    x = _dev(synth.uniform(tag + "x", (n, h, w, cin), -1, 1), dt)
    w1 = _dev(synth.normal(tag + "w1", (cmid, 1, 1, cin), 0, (2.0 / cin) ** 0.5), dt)
    w2 = _dev(synth.normal(tag + "w2", (cout, 3, 3, cmid), 0, (2.0 / (9 * cmid)) ** 0.5), dt)
    f = [_dev(synth.uniform(tag + c, (m,), lo, hi)) for c, m, lo, hi in (("s1", cmid, 0.5, 1.5), ("t1", cmid, 0.2, 1.2),
                                                                          ("s2", cout, 0.5, 1.5), ("t2", cout, -0.5, 0.5))]
    res = _dev(synth.uniform(tag + "r", (n, h, w, cout), -1, 1), dt)
    return x, w1, w2, f, res


def _launch_bneck(hip, x, w1t, w2t, f, res, y, tile):
    d = hip.Bneck16Desc()
    n, h, w, cin = x.shape
    d.x, d.x_pitch = x.data_ptr(), _pitch(x)
    d.w1_tiled, d.scale1, d.shift1 = w1t.data_ptr(), f[0].data_ptr(), f[1].data_ptr()
    d.w2_tiled, d.scale2, d.shift2 = w2t.data_ptr(), f[2].data_ptr(), f[3].data_ptr()
    d.res, d.res_pitch = _p(res), _pitch(res) if res is not None else 0
    d.y, d.y_pitch = y.data_ptr(), _pitch(y)
    d.n, d.h, d.w, d.cin, d.cmid, d.cout = n, h, w, cin, w1t.shape[2], w2t.shape[2]
    d.act1, d.act2, d.half_type, d.tile = 1, 1, hip.HALF_TYPES[x.dtype], tile
    hip.check(hip.lib().me_bneck_h16(C.byref(d), hip.stream_ptr()), "me_bneck_h16")
    torch.cuda.synchronize()


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("tile", [1, 3, 4])
def test_poison_bneck_h16(hip_lib, tile, half):
    """me_bneck_h16 (1x1 -> 3x3 + shortcut in one launch): NaN beside the x / residual slices and around both tiled weight
    copies, both scale / shift pairs, the output; ragged rows (13 x 11, 20 x 31), several images per tile."""
    from millieye_amd import hip
    assert tuple(hip.BNECK_TILES) == (1, 3, 4)
    dt = HALVES[half]
    x, w1, w2, f, res = _bneck_operands(tile, dt)
    what = f"bneck {half} tile {tile}"
    clean = hip.bneck_h16(x, w1, f[0], f[1], w2, f[2], f[3], residual=res, tile=tile)
    torch.cuda.synchronize()
    checks = []
    xs, c = _sliced(x, 32, 32); checks.append(("x", c))   # noqa: E702
    w1t, c = _band_copy(hip.tile_weights_h16(w1)); checks.append(("w1", c))   # noqa: E702
    w2t, c = _band_copy(hip.tile_weights_h16(w2)); checks.append(("w2", c))   # noqa: E702
    fb = []
    for i, t in enumerate(f):
        b, c = _band_copy(t, 64, 64); fb.append(b); checks.append((f"affine{i}", c))   # noqa: E702
    rs, c = _sliced(res, YL, YR); checks.append(("res", c))   # noqa: E702
    y, raw = _poisoned_y(tuple(clean.shape), clean.shape[-1], dt)
    _launch_bneck(hip, xs, w1t, w2t, fb, rs, y, tile)
    _assert_y(y, raw, clean, what)
    for name, c in checks:
        c(f"{what}: {name}")


# --------------------------------------------------------------------------------------
# part B: locality
# --------------------------------------------------------------------------------------
def _assert_locality(y_nan, y_zero, n, img, mask, what):
    """Outside the receptive field (other images included) the bits of the zeroed run; inside NaN."""
    inside = torch.zeros(y_nan.shape[:3], dtype=torch.bool, device=y_nan.device)
    inside[img] = torch.from_numpy(mask).to(y_nan.device)
    assert bool(torch.isnan(y_nan[inside].float()).all()), f"{what}: an output inside the receptive field is not NaN"
    out = ~inside
    assert bool(torch.isfinite(y_zero.float()).all()), what
    assert bool(torch.equal(_bits(y_nan[out]), _bits(y_zero[out]))), \
        f"{what}: {int((_bits(y_nan[out]) != _bits(y_zero[out])).sum())} outputs outside the receptive field changed"


def _assert_weight_row_locality(run, wg, what, row=None, all_nan=False):
    """``run(weights)``: a NaN weight row gives a NaN output channel ``row`` and leaves every other channel's bits as the run
    with that row zeroed has them (``all_nan``: the row feeds every output, which must all be NaN)."""
    r = wg.shape[0] // 2
    wz, wn = wg.clone(), wg.clone()
    wz[r] = 0.0
    wn[r] = NAN
    yz, yn = run(wz), run(wn)
    assert bool(torch.isfinite(yz.float()).all()), what
    if all_nan:
        assert bool(torch.isnan(yn.float()).all()), f"{what}: a NaN row of the first filter must reach every output"
        return
    row = r if row is None else row
    others = [c for c in range(yn.shape[-1]) if c != row]
    assert bool(torch.isnan(yn[..., row].float()).all()), f"{what}: the NaN weight row must give a NaN channel"
    assert _same_bits(yn[..., others], yz[..., others]), f"{what}: a NaN weight row changed another channel"


def _locality_tiles_f32(name):
    tiles = [(3, 1), (5, 1), (23, 1), (53, 1), (43, 3), (2, 3)]
    if name in ("k3", "k3s2"):
        tiles.append((60, 1))
    if name == "k1":
        tiles.append((50, 1))
    return tiles


@pytest.mark.parametrize("loc", R.LOCALITY, ids=[c[0] for c in R.LOCALITY])
def test_locality_f32(hip_lib, loc):
    """One NaN input pixel (interior, corner, last pixel of the last image) and one NaN weight row, on a tile id of every family
    that takes the shape (whole and split launches)."""
    from millieye_amd import hip
    name, n, h, w, cin, cout, k, s, pad = loc
    case = R._b(name, n, h, w, cin, cout, k, s, R.LEAKY, pad=pad)
    x, wg, scale, shift, _res = _operands(case, 2)
    run = lambda xx, ww, tile, split: hip.conv2d(xx, ww, scale, shift, k, s, pad, R.LEAKY, tile=tile, split_k=split)  # noqa: E731
    for tile, split in _locality_tiles_f32(name):
        for img, py, px in R.locality_pixels(n, h, w):
            xz, xn = x.clone(), x.clone()
            xz[img, py, px] = 0.0
            xn[img, py, px] = NAN
            _assert_locality(run(xn, wg, tile, split), run(xz, wg, tile, split), n, img, R.receptive_mask(h, w, k, s, pad, py, px),
                             f"{name} tile {tile} split {split} pixel {(img, py, px)}")
        _assert_weight_row_locality(lambda ww: run(x, ww, tile, split), wg, f"{name} tile {tile} split {split}")


@pytest.mark.parametrize("tile", [221, 131, 100])
def test_locality_f32_patch_resident(hip_lib, tile):
    from millieye_amd import hip
    n, h, w, cin, cout = 3, 13, 11, 32, 256
    case = R._b("loc_p8", n, h, w, cin, cout, 3, 1, R.LEAKY)
    x, wg, scale, shift, _res = _operands(case, 3)
    run = lambda xx: hip.conv2d(xx, wg, scale, shift, 3, 1, 1, R.LEAKY, tile=tile, split_k=1)  # noqa: E731
    for img, py, px in R.locality_pixels(n, h, w):
        xz, xn = x.clone(), x.clone()
        xz[img, py, px] = 0.0
        xn[img, py, px] = NAN
        _assert_locality(run(xn), run(xz), n, img, R.receptive_mask(h, w, 3, 1, 1, py, px), f"p8 tile {tile} pixel {(img, py, px)}")
    _assert_weight_row_locality(lambda ww: hip.conv2d(x, ww, scale, shift, 3, 1, 1, R.LEAKY, tile=tile, split_k=1), wg, f"p8 tile {tile}")


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_locality_h16_and_bneck(hip_lib, half):
    from millieye_amd import hip
    dt = HALVES[half]
    n, h, w, cin, cout = 3, 13, 11, 64, 256
    case = R._b("loc_h16", n, h, w, cin, cout, 3, 1, R.LEAKY)
    x, wg, scale, shift, _res = _operands(case, 4, dt)
    for tile, split in ((3, 1), (4, 1), (13, 3), (221, 1), (41, 1)):
        run = lambda xx: hip.conv2d_h16(xx, wg, scale, shift, 3, 1, 1, R.LEAKY, tile=tile, split_k=split)  # noqa: E731
        for img, py, px in R.locality_pixels(n, h, w):
            xz, xn = x.clone(), x.clone()
            xz[img, py, px] = 0.0
            xn[img, py, px] = NAN
            _assert_locality(run(xn), run(xz), n, img, R.receptive_mask(h, w, 3, 1, 1, py, px),
                             f"{half} tile {tile} split {split} pixel {(img, py, px)}")
        _assert_weight_row_locality(lambda ww: hip.conv2d_h16(x, ww, scale, shift, 3, 1, 1, R.LEAKY, tile=tile, split_k=split), wg,
                                    f"{half} tile {tile} split {split}")
    for tile in hip.BNECK_TILES:     # 1x1 then 3x3: the receptive field of the pair is the 3x3's
        x, w1, w2, f, res = _bneck_operands(tile, dt)
        n, h, w = x.shape[:3]
        run = lambda xx: hip.bneck_h16(xx, w1, f[0], f[1], w2, f[2], f[3], residual=res, tile=tile)  # noqa: E731
        for img, py, px in R.locality_pixels(n, h, w):
            xz, xn = x.clone(), x.clone()
            xz[img, py, px] = 0.0
            xn[img, py, px] = NAN
            _assert_locality(run(xn), run(xz), n, img, R.receptive_mask(h, w, 3, 1, 1, py, px), f"bneck {half} tile {tile} pixel {(img, py, px)}")
        # a mid channel feeds every output (the centre tap is always inside the map); a row of the 3x3 one output channel
        _assert_weight_row_locality(lambda ww: hip.bneck_h16(x, ww, f[0], f[1], w2, f[2], f[3], residual=res, tile=tile), w1,
                                    f"bneck {half} tile {tile} w1", all_nan=True)
        _assert_weight_row_locality(lambda ww: hip.bneck_h16(x, w1, f[0], f[1], ww, f[2], f[3], residual=res, tile=tile), w2,
                                    f"bneck {half} tile {tile} w2")


# --------------------------------------------------------------------------------------
# part C
# --------------------------------------------------------------------------------------
GIB = 1 << 30


def _room(need_bytes):
    free, _total = torch.cuda.mem_get_info()
    if free < 2 * need_bytes:
        pytest.skip(f"needs {need_bytes / GIB:.1f} GiB, twice that must be free ({free / GIB:.1f} GiB are)")


def _rand_ints(shape, lo, hi, seed, dtype=F32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == F32:
        return torch.randint(lo, hi + 1, shape, generator=g, device="cuda", dtype=dtype)
    return torch.randint(lo, hi + 1, shape, generator=g, device="cuda", dtype=torch.int16).to(dtype)


def _rows_view(x, a, b):
    """Rows [a, b) of a one-image NHWC tensor (or channel slice) as a tensor the descriptors accept."""
    sub = x[:, a:b]
    pitch = x.stride(2)
    return torch.as_strided(sub, sub.shape, ((b - a) * x.shape[2] * pitch, x.shape[2] * pitch, pitch, 1), sub.storage_offset())


def _check_bands_one_image(y, x, wg, scale, shift, k, pad, act, seed, what):
    """Stride 1, one image: bands of 8 output rows against fused_conv64 of the input rows they read (zero rows beyond the map)."""
    h, ho = x.shape[1], y.shape[1]
    wc, sc, hc = wg.cpu(), scale.cpu(), shift.cpu()
    row_bytes = max(y.shape[2] * y.shape[3] * y.element_size(), x.shape[2] * x.stride(2) * x.element_size())
    for r0 in R.sample_bands(ho, row_bytes, seed=seed):
        r1 = min(r0 + 8, ho)
        a, b = r0 - pad, r1 - 1 - pad + k
        xb = x[:, max(a, 0):min(b, h)].cpu()
        ref = R.fused_conv64(xb, wc, sc, hc, k, 1, (max(-a, 0), max(b - h, 0), pad, pad), act)
        got = y[:, r0:r1].cpu()
        want = R.round_to(ref, y.dtype)
        assert tuple(got.shape) == tuple(want.shape)
        assert bool(torch.equal(got, want)), f"{what}: rows {r0}..{r1} differ from the float64 reference in " \
                                             f"{int((got != want).sum())} elements"


def _check_stitched_one_image(hip, y, launch, x, k, pad, rows, what):
    """The whole tensor against the same tile id run on bands of ``rows`` output rows with their halo (small offsets)."""
    h, ho = x.shape[1], y.shape[1]
    for r0 in range(0, ho, rows):
        r1 = min(r0 + rows, ho)
        a0, b0 = max(r0 - pad, 0), min(r1 - 1 - pad + k, h)
        part = launch(_rows_view(x, a0, b0))
        # output row j of the sub-launch reads sub rows j - pad .. j - pad + k - 1 = global rows a0 + j - pad ..; global output row
        # r reads global rows r - pad ..: j = r - a0
        lo = r0 - a0
        assert bool(torch.equal(y[:, r0:r1], part[:, lo:lo + (r1 - r0)])), f"{what}: rows {r0}..{r1} differ from the band-wise run"
        del part


def _one_image_case(hip, h, w, cin, x_pitch, cout, act, tile, seed, what, half=None, band_rows=512, y16=False):
    """3x3 / stride 1 / pad 1 on one h x w image: forced ``tile`` (or 0) must equal the reference and the band-wise run.  16-bit
    operands give fp32 outputs, or - ``y16``, for the tiles that have no fp32-output form - 16-bit ones rounded once."""
    dt = half or F32
    es = 2 if half else 4
    ydt = dt if y16 else F32
    _room(h * w * (x_pitch + 2 * cout) * es)
    xfull = _rand_ints((1, h, w, x_pitch), -R.INT_X, R.INT_X, seed, dt)
    x = xfull if x_pitch == cin else xfull[..., :cin]
    wg = _rand_ints((cout, 3, 3, cin), -R.INT_W, R.INT_W, seed + 1, dt)
    scale = torch.full((cout,), 2.0, device="cuda")
    shift = _rand_ints((cout,), -3, 3, seed + 2)
    assert R.exact_sum_bound(9 * cin, 2.0, 3.0) < 2 ** 24
    wt = None
    if tile >= 100:
        wt = (hip.tile_weights_h16 if half else hip.tile_weights_f32)(wg)

    def launch(xx, t=tile):
        y = torch.empty((1, xx.shape[1], w, cout), device="cuda", dtype=ydt)
        if half:
            _launch_h16(hip, xx, wg, scale, shift, 3, 1, 1, act, y, tile=t, split=1, wgt_tiled=wt)
        else:
            _launch_f32(hip, xx, wg, scale, shift, 3, 1, 1, act, y, tile=t, split=1, wgt_tiled=wt)
        return y

    y = launch(x)
    _check_bands_one_image(y, x, wg, scale, shift, 3, 1, act, seed, what)
    _check_stitched_one_image(hip, y, launch, x, 3, 1, band_rows, what)
    return x, wg, scale, shift


def _refused(hip, x, wg, scale, shift, tile, split=1, half=None):
    cout, w = wg.shape[0], x.shape[2]
    y = torch.empty((1, x.shape[1], w, cout), device="cuda", dtype=F32 if not half else half)
    wt = None
    if tile >= 100:
        wt = (hip.tile_weights_h16 if half else hip.tile_weights_f32)(wg)
    with pytest.raises(hip.MeError):
        if half:
            _launch_h16(hip, x, wg, scale, shift, 3, 1, 1, R.LINEAR, y, tile=tile, split=split, wgt_tiled=wt)
        else:
            _launch_f32(hip, x, wg, scale, shift, 3, 1, 1, R.LINEAR, y, tile=tile, split=split, wgt_tiled=wt)


def test_guard_f32_buffer_window(hip_lib):
    """buf_addressable<BM> (csrc/conv.hip) at cin = pitch = 16 on a 4096-wide image: the largest h it accepts on the 64-row buffer
    tile; one more row through tile 0 (falls back to the DMA kernel, 64-bit pointers), where the tail split (checks the guard
    itself) must refuse."""
    from millieye_amd import hip
    w, cin, cout = 4096, 16, 16
    ok = lambda h: R.buf_addressable(64, h, w, cin, cin, 3, h, w)  # noqa: E731
    h = R.largest_h(ok)
    assert ok(h) and not ok(h + 1)
    _one_image_case(hip, h, w, cin, cin, cout, R.LEAKY, 3, 11, f"buffer tile 3 at h {h} (accepted)")
    torch.cuda.empty_cache()
    x, wg, scale, shift = _one_image_case(hip, h + 1, w, cin, cin, cout, R.LEAKY, 0, 12, f"tile 0 at h {h + 1} (beyond the guard)")
    _refused(hip, x, wg, scale, shift, 43, split=3)
    del x
    torch.cuda.empty_cache()


def test_guard_f32_weight_stationary_3x3(hip_lib):
    """ws3x3_f32_eligible (csrc/conv_ws_f32.hip): one image below 2^31 bytes - 2048 x 4095 pixels at a pitch of 64 channels are
    accepted on tile 60, 2049 rows refused; tile 0 takes the larger image."""
    from millieye_amd import hip
    w, cin, pitch, cout = 4095, 32, 64, 32
    ok = lambda h: R.ws3x3_f32_window(h, w, pitch)  # noqa: E731
    h = R.largest_h(ok)
    assert h == 2048
    _one_image_case(hip, h, w, cin, pitch, cout, R.LEAKY, 60, 21, f"tile 60 at h {h} (accepted)", band_rows=256)
    torch.cuda.empty_cache()
    x, wg, scale, shift = _one_image_case(hip, h + 1, w, cin, pitch, cout, R.LINEAR, 0, 22, f"tile 0 at h {h + 1}", band_rows=256)
    _refused(hip, x, wg, scale, shift, 60)
    del x
    torch.cuda.empty_cache()


def test_guard_f32_patch_resident(hip_lib):
    """p8_eligible (csrc/conv_p8_f32.hip): two images of the window's span below 2^31 bytes - 69905 x 60 pixels at a pitch of 64
    channels accepted on tile 221, one more row refused and taken by tile 0.  (60 wide: the patch of a 256-row tile, 256 + 2 * 62
    rows, still fits the 80 KB of LDS that tile 221 may use; 64 wide does not.)"""
    from millieye_amd import hip
    w, cin, pitch, cout = R.P8_GUARD_W, 16, 64, 128
    assert R.p8_f32_lds_bytes(256, 128, 8, w) <= 80 * 1024
    ok = lambda h: R.p8_window(1, h, w, pitch)  # noqa: E731
    h = R.largest_h(ok)
    assert h == 69905
    _one_image_case(hip, h, w, cin, pitch, cout, R.LEAKY, 221, 31, f"tile 221 at h {h} (accepted)", band_rows=8192)
    torch.cuda.empty_cache()
    x, wg, scale, shift = _one_image_case(hip, h + 1, w, cin, pitch, cout, R.LINEAR, 0, 32, f"tile 0 at h {h + 1}", band_rows=8192)
    _refused(hip, x, wg, scale, shift, 221)
    del x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_guard_h16_buffer_window(hip_lib, half):
    """addressable16 (csrc/conv_h16.hip), fp32 output of integer operands: the largest accepted h on the 64-row tile equals the
    reference; one more row is refused (the 16-bit path has no kernel with 64-bit addressing to fall back to)."""
    from millieye_amd import hip
    dt = HALVES[half]
    w, cin, cout = 4096, 32, 16
    ok = lambda h: R.buf_addressable(64, h, w, cin, cin, 3, h, w, 2)  # noqa: E731
    h = R.largest_h(ok)
    x, wg, scale, shift = _one_image_case(hip, h, w, cin, cin, cout, R.LEAKY, 3, 41, f"{half} tile 3 at h {h} (accepted)", half=dt)
    del x
    torch.cuda.empty_cache()
    _room((h + 1) * w * cin * 2)
    x = torch.zeros((1, h + 1, w, cin), device="cuda", dtype=dt)
    for tile in (0, 3):
        _refused(hip, x, wg, scale, shift, tile, half=dt)
    del x
    torch.cuda.empty_cache()


def _refused_h16_one_more_row(hip, h, w, cin, pitch, wg, scale, shift, dt, tiles):
    _room((h + 1) * w * pitch * 2)
    xfull = torch.zeros((1, h + 1, w, pitch), device="cuda", dtype=dt)
    for tile in tiles:
        _refused(hip, xfull[..., :cin], wg, scale, shift, tile, half=dt)
    del xfull
    torch.cuda.empty_cache()


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_guard_h16_patch_resident(hip_lib, half):
    """p8_eligible (csrc/conv_p8_h16.hip): the fp32 formula at two bytes per element - 69905 x 60 pixels at a pitch of 128
    channels accepted on tile 221 (16-bit output, rounded once), one more row refused by it and by tile 0."""
    from millieye_amd import hip
    dt = HALVES[half]
    w, cin, pitch, cout = R.P8_GUARD_W, 32, 128, 128
    ok = lambda h: R.p8_window(1, h, w, pitch, 2)  # noqa: E731
    h = R.largest_h(ok)
    assert h == 69905
    x, wg, scale, shift = _one_image_case(hip, h, w, cin, pitch, cout, R.LEAKY, 221, 33, f"{half} tile 221 at h {h} (accepted)",
                                          half=dt, band_rows=8192, y16=True)
    del x
    torch.cuda.empty_cache()
    _refused_h16_one_more_row(hip, h, w, cin, pitch, wg, scale, shift, dt, (221, 0))


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_guard_h16_weight_stationary_3x3(hip_lib, half):
    """ws3x3_eligible (csrc/conv3x3_ws_h16.hip): 2048 x 4095 pixels at a pitch of 128 16-bit channels accepted on tile 60, 2049 rows
    refused by it and by tile 0."""
    from millieye_amd import hip
    dt = HALVES[half]
    w, cin, pitch, cout = 4095, 32, 128, 64
    ok = lambda h: R.ws3x3_f32_window(h, w, pitch, 2)  # noqa: E731
    h = R.largest_h(ok)
    assert h == 2048
    x, wg, scale, shift = _one_image_case(hip, h, w, cin, pitch, cout, R.LEAKY, 60, 23, f"{half} tile 60 at h {h} (accepted)",
                                          half=dt, band_rows=256, y16=True)
    del x
    torch.cuda.empty_cache()
    _refused_h16_one_more_row(hip, h, w, cin, pitch, wg, scale, shift, dt, (60, 0))


@pytest.mark.parametrize("half", [None, "bf16", "f16"], ids=["f32", "bf16", "f16"])
def test_guard_weight_stationary_1x1_pitch(hip_lib, half):
    """ws1x1_f32_eligible (csrc/conv_ws_f32.hip) and ws1x1_eligible (csrc/conv1x1_ws_h16.hip) bound the PITCH, not h: the 128 rows
    of the tallest tile (cin 64 -> cout 32) must lie inside 2^31 bytes.  132 pixels (a whole tile and a ragged one) as channel
    slices of one NaN buffer at the largest accepted pitch equal float64; at the next pitch tile 50 refuses, and the fp32 tile 0
    still gives the right answer."""
    from millieye_amd import hip
    dt = HALVES[half] if half else F32
    es = 2 if half else 4
    n, h, w, cin, cout = 1, 12, 11, 64, 32
    p_ok, p_no = R.ws1x1_guard_pitches(es)
    assert R.ws1x1_window(p_ok, es) and not R.ws1x1_window(p_no, es) and h * w > 128
    _room(h * w * p_no * es)
    raw = torch.empty((h * w * p_no,), device="cuda", dtype=dt)
    xs = _rand_ints((n, h, w, cin), -R.INT_X, R.INT_X, 91, dt)
    wg = _rand_ints((cout, 1, 1, cin), -R.INT_W, R.INT_W, 92, dt)
    scale, shift = torch.full((cout,), 2.0, device="cuda"), _rand_ints((cout,), -3, 3, 93)
    assert R.exact_sum_bound(cin, 2.0, 3.0) < 2 ** 24
    want = R.round_to(R.fused_conv64(xs.cpu(), wg.cpu(), scale.cpu(), shift.cpu(), 1, 1, 0, R.LEAKY), dt)

    def run(pitch, tile):
        raw.fill_(NAN)
        x = torch.as_strided(raw, (n, h, w, cin), (h * w * pitch, w * pitch, pitch, 1))
        x.copy_(xs)
        y = torch.empty((n, h, w, cout), device="cuda", dtype=dt)
        (_launch_h16 if half else _launch_f32)(hip, x, wg, scale, shift, 1, 1, 0, R.LEAKY, y, tile=tile, split=1)
        return y.cpu()

    got = run(p_ok, 50)
    assert bool(torch.equal(got, want)), f"tile 50 at pitch {p_ok}: {int((got != want).sum())} elements differ from float64"
    with pytest.raises(hip.MeError):
        run(p_no, 50)
    if not half:
        got = run(p_no, 0)
        assert bool(torch.equal(got, want)), f"tile 0 at pitch {p_no}: {int((got != want).sum())} elements differ from float64"
    del raw
    torch.cuda.empty_cache()


def test_guard_bneck_h16_supported(hip_lib):
    """me_bneck_h16_supported restates the patch window: 1 at the largest h the formula accepts (and the launch then equals the
    two launches it replaces), 0 one row further, where me_bneck_h16 must refuse."""
    from millieye_amd import hip
    dt = torch.bfloat16
    w, cin, pitch, cmid, cout = 60, 32, 1024, 128, 256
    ok = lambda h: R.p8_window(1, h, w, pitch, 2)  # noqa: E731
    h = R.largest_h(ok)
    _room((h + 1) * w * (pitch + 3 * cout) * 2)
    xfull = _rand_ints((1, h + 1, w, pitch), -1, 1, 51, dt)
    w1 = _rand_ints((cmid, 1, 1, cin), -1, 1, 52, dt)
    w2 = _rand_ints((cout, 3, 3, cmid), -1, 1, 53, dt)
    f = [torch.ones(cmid, device="cuda"), _rand_ints((cmid,), -2, 2, 54), torch.full((cout,), 0.5, device="cuda"), _rand_ints((cout,), -2, 2, 55)]
    d = hip.Bneck16Desc()
    d.n, d.w, d.cin, d.cmid, d.cout, d.x_pitch, d.tile = 1, w, cin, cmid, cout, pitch, 1
    d.h = h
    assert hip.lib().me_bneck_h16_supported(C.byref(d)) == 1
    d.h = h + 1
    assert hip.lib().me_bneck_h16_supported(C.byref(d)) == 0
    x_ok = _rows_view(xfull[..., :cin], 0, h)
    assert (cin + 2) <= 256 and R.exact_sum_bound(9 * cmid) * (cin + 2) / (R.INT_X * R.INT_W) < 2 ** 24   # mid exact in 8 bits
    one = hip.bneck_h16(x_ok, w1, f[0], f[1], w2, f[2], f[3], tile=1, act1=R.LINEAR, act2=R.LINEAR)
    # the two launches it replaces, band by band with a halo row (the per-tap 1x1 tile spans two images of its window: the
    # whole map at this pitch is beyond ITS guard)
    rows = 1024
    for r0 in range(0, h, rows):
        r1 = min(r0 + rows, h)
        a0, b0 = max(r0 - 1, 0), min(r1 + 1, h)
        mid = hip.conv2d_h16(_rows_view(x_ok, a0, b0), w1, f[0], f[1], 1, 1, 0, R.LINEAR, tile=1, split_k=1)
        two = hip.conv2d_h16(mid, w2, f[2], f[3], 3, 1, 1, R.LINEAR, tile=131, split_k=1)[:, r0 - a0:r0 - a0 + (r1 - r0)]
        assert bool(torch.equal(one[:, r0:r1], two)), f"rows {r0}..{r1}: {int((one[:, r0:r1] != two).sum())} elements differ from the two launches"
    # sampled bands (both ends, seeded random ones) against float64: integers, so the mid tensor is exact in 16 bits and the
    # output rounds once
    for r0 in R.sample_bands(h, w * pitch * 2, seed=56):
        r1 = r0 + 8
        a, b = max(r0 - 1, 0), min(r1 + 1, h)
        xb = x_ok[:, a:b].cpu()
        m64 = R.fused_conv64(xb, w1.cpu(), f[0].cpu(), f[1].cpu(), 1, 1, 0, R.LINEAR)
        m64 = R.round_to(m64, dt).double().numpy()
        ref = R.fused_conv64(m64, w2.cpu(), f[2].cpu(), f[3].cpu(), 3, 1, (1 if a == 0 else 0, 1 if b == h else 0, 1, 1), R.LINEAR)
        want = R.round_to(ref, dt)
        assert want.shape[1] == r1 - r0
        assert bool(torch.equal(one[:, r0:r1].cpu(), want)), f"rows {r0}..{r1} differ from the float64 reference"
    with pytest.raises(hip.MeError):
        hip.bneck_h16(xfull[..., :cin], w1, f[0], f[1], w2, f[2], f[3], tile=1, act1=R.LINEAR, act2=R.LINEAR)
    del xfull, x_ok, one, two, mid
    torch.cuda.empty_cache()


def _many_images_case(hip, n, hw, cin, cout, tile, split, with_res, ups, seed, what, chunk=6, half=None):
    """1x1 convolution over n images of hw x hw pixels: bands against float64, and image chunks against the whole launch.
    ``half``: 16-bit operands, residual and output (rounded once from the exact fp32 value); the slabs stay fp32."""
    dt = half or F32
    es = 2 if half else 4
    m = n * hw * hw
    need = m * (cin + cout * ups * ups + (cout if with_res else 0)) * es + (m * split * cout * 4 if split > 1 else 0)
    _room(need)
    x = _rand_ints((n, hw, hw, cin), -R.INT_X, R.INT_X, seed, dt)
    wg = _rand_ints((cout, 1, 1, cin), -R.INT_W, R.INT_W, seed + 1, dt)
    scale = torch.full((cout,), 0.5, device="cuda")
    shift = _rand_ints((cout,), -3, 3, seed + 2)
    res = _rand_ints((n, hw, hw, cout), -3, 3, seed + 3, dt) if with_res else None
    act = R.LINEAR if with_res else R.LEAKY          # (leaky + residual rounds twice: not exact)
    assert R.exact_sum_bound(cin, 0.5, 3.0, 3.0) < 2 ** 24

    def launch(xx, rr, sp):
        y = torch.empty((xx.shape[0], hw * ups, hw * ups, cout), device="cuda", dtype=dt)
        ws_check = (_launch_h16 if half else _launch_f32)(hip, xx, wg, scale, shift, 1, 1, 0, act, y, res=rr, ups=ups, tile=tile, split=sp)
        assert (ws_check is not None) == (sp > 1), "a forced split goes through a workspace"
        if ws_check is not None:
            ws_check(f"{what}: workspace")
        return y

    y = launch(x, res, split)
    rows_per_img = hw * ups
    big_row_bytes = max(hw * cin, rows_per_img * cout) * es
    wc, sc, hc = wg.cpu(), scale.cpu(), shift.cpu()
    for r in R.sample_bands(n * rows_per_img, big_row_bytes, seed=seed):
        r -= r % 8
        img, r0 = divmod(r, rows_per_img)
        q0, q1 = r0 // ups, -(-(r0 + 8) // ups)
        ref = R.fused_conv64(x[img:img + 1, q0:q1].cpu(), wc, sc, hc, 1, 1, 0, act,
                             res[img:img + 1, q0:q1].cpu() if with_res else None, ups)
        want = R.round_to(ref, dt)[:, r0 - q0 * ups:r0 - q0 * ups + 8]
        got = y[img:img + 1, r0:r0 + 8].cpu()
        assert bool(torch.equal(got, want)), f"{what}: image {img} rows {r0}..{r0 + 8} differ from the float64 reference in " \
                                             f"{int((got != want).sum())} elements"
    for i in range(0, n, chunk):
        part = launch(x[i:i + chunk], res[i:i + chunk] if with_res else None, 1)
        assert bool(torch.equal(y[i:i + chunk], part)), f"{what}: images {i}..{i + chunk} differ from the chunk-wise run"
        del part
    del x, y, res
    torch.cuda.empty_cache()


_MANY = [(None, 0), (None, 3), ("bf16", 0), ("bf16", 3), ("f16", 3)]
_MANY_IDS = [f"{h or 'f32'}-{t}" for h, t in _MANY]


@pytest.mark.parametrize("half,tile", _MANY, ids=_MANY_IDS)
def test_many_images_x_past_4gib(hip_lib, half, tile):
    """x of 66 x 128 x 128 x 1024: 4.4 GB in fp32 and, the same element count, 2.2 GB in 16 bits - the image rebasing of the
    input must be 64-bit (fp32) and must not wrap at 2^31 bytes (16-bit)."""
    from millieye_amd import hip
    _many_images_case(hip, 66, 128, 1024, 16 if not half else 32, tile, 1, False, 1, 61, f"{half or 'f32'} x past 2^31 / 2^32 bytes, tile {tile}",
                      half=HALVES.get(half))


@pytest.mark.parametrize("half,tile", _MANY, ids=_MANY_IDS)
def test_many_images_y_and_residual_past_4gib(hip_lib, half, tile):
    """y and the residual of 66 x 128 x 128 x 1024 (4.4 GB each in fp32, 2.2 GB in 16 bits); and the upsampled form
    (66 x 256 x 256 x 256)."""
    from millieye_amd import hip
    cin, name = (16, "f32") if not half else (32, half)
    _many_images_case(hip, 66, 128, cin, 1024, tile, 1, True, 1, 71, f"{name} y / res past 2^31 / 2^32 bytes, tile {tile}", half=HALVES.get(half))
    _many_images_case(hip, 66, 128, cin, 256, tile, 1, True, 2, 72, f"{name} upsampled y past 2^31 / 2^32 bytes, tile {tile}", half=HALVES.get(half))


@pytest.mark.parametrize("half,tile", _MANY[:4], ids=_MANY_IDS[:4])
def test_many_images_split_k_slabs_past_4gib(hip_lib, half, tile):
    """split_k = 4 with fp32 slabs of 66 x 128 x 128 x 256 = 1.1 GB each: slab offsets beyond 2^32 bytes, NaN workspace; fp32 and
    16-bit operands."""
    from millieye_amd import hip
    cin = 256 if half else 64      # (the 16-bit kernels split whole 64-channel stages: four of them)
    _many_images_case(hip, 66, 128, cin, 256, tile, 4, False, 1, 81, f"{half or 'f32'} slabs past 2^32 bytes, tile {tile}", half=HALVES.get(half))
