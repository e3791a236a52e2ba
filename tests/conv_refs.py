"""Plain float64 references of the fused inference convolution (``me_conv2d_f32`` / ``me_conv2d_h16`` / ``me_bneck_h16``), the
error measure of the fp32 precision bar, guard-banded buffers, and the shape tables of ``tests/test_gpu_conv_blocks.py``.
numpy / torch float64 only, no project kernel and no ``F.conv2d``.  Layouts are the kernels': maps are NHWC, weights OHWI
``[cout, k, k, cin]``.  ``tests/test_conv_refs_cpu.py`` pins the references to stock torch float64 and checks, for every
table below, the arithmetic facts the GPU tests rest on.

Order of the fused operation (csrc/conv32_common.h, ``epilogue``): convolution, ``* scale + shift`` per output channel,
activation, ``+ residual``, nearest x2 upsampling.  The LeakyReLU slope is the float32 value of 0.1."""
import numpy as np
import torch

from millieye_amd import synth

LINEAR, LEAKY, SIGMOID = 0, 1, 2
SLOPE = float(np.float32(0.1))
U24 = 2.0 ** -24


def _f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu()
        a = (a.float() if a.dtype in (torch.bfloat16, torch.float16) else a).numpy()
    return np.asarray(a, dtype=np.float64)


def _pads(pad):
    """pad: one number (all four sides) or (top, bottom, left, right)."""
    return (pad,) * 4 if isinstance(pad, int) else tuple(int(v) for v in pad)


def out_size(h, k, stride, pad_lo, pad_hi=None):
    return (h + pad_lo + (pad_lo if pad_hi is None else pad_hi) - k) // stride + 1


def im2col(x, k, stride, pad):
    """x [n, h, w, c] -> [n, ho, wo, k * k * c], columns ordered (ky, kx, channel) like a flattened OHWI filter; zero padding."""
    x = _f64(x)
    n, h, w, c = x.shape
    top, bottom, left, right = _pads(pad)
    xp = np.zeros((n, h + top + bottom, w + left + right, c))
    xp[:, top:top + h, left:left + w, :] = x
    ho, wo = out_size(h, k, stride, top, bottom), out_size(w, k, stride, left, right)
    cols = np.empty((n, ho, wo, k * k * c))
    for ky in range(k):
        for kx in range(k):
            t = ky * k + kx
            cols[..., t * c:(t + 1) * c] = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride, :]
    return cols


def _upsample2(y):
    return y.repeat(2, axis=1).repeat(2, axis=2)


def fused_conv64(x, w, scale, shift, k, stride, pad, act, res=None, ups=1):
    """act(conv(x, w) * scale + shift) + res, then nearest x2 upsampling, all in float64: explicit im2col and one matmul."""
    w = _f64(w)
    cout = w.shape[0]
    assert w.shape[1] == k and w.shape[2] == k
    y = im2col(x, k, stride, pad) @ w.reshape(cout, -1).T
    y = y * _f64(scale) + _f64(shift)
    if act == LEAKY:
        y = np.where(y > 0, y, SLOPE * y)
    elif act == SIGMOID:
        y = 1.0 / (1.0 + np.exp(-y))
    elif act != LINEAR:
        raise ValueError(act)
    if res is not None:
        y = y + _f64(res)
    return _upsample2(y) if ups == 2 else y


def abs_sum64(x, w, scale, shift, k, stride, pad, res=None, ups=1):
    """conv(|x|, |w|) * |scale| + |shift| + |res|: the magnitude every rounding of the fused operation is relative to, so an
    error divided by it does not grow where the terms cancel."""
    w = np.abs(_f64(w))
    y = im2col(np.abs(_f64(x)), k, stride, pad) @ w.reshape(w.shape[0], -1).T
    y = y * np.abs(_f64(scale)) + np.abs(_f64(shift))
    if res is not None:
        y = y + np.abs(_f64(res))
    return _upsample2(y) if ups == 2 else y


def rel_err(got, ref64, denom64):
    """e = max |got - ref64| / abs_sum64."""
    got = _f64(got)
    assert got.shape == ref64.shape == denom64.shape, (got.shape, ref64.shape, denom64.shape)
    assert np.isfinite(got).all(), "non-finite output"
    return float((np.abs(got - ref64) / denom64).max())


def round_to(t64, dtype):
    """float64 -> float32 -> ``dtype`` (torch tensor): the rounding points of the 16-bit kernels (fp32 accumulator, 16-bit store)."""
    t = torch.from_numpy(np.ascontiguousarray(_f64(t64))).to(torch.float32)
    return t if dtype == torch.float32 else t.to(dtype)


_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def banded(shape, dtype, lead, tail, fill, device="cpu"):
    """One allocation of ``lead`` + prod(shape) + ``tail`` elements filled with ``fill`` (NaN allowed).  Returns the inner view
    of ``shape`` and a function that asserts every guard element still holds ``fill``, bit for bit.  ``lead`` is kept a
    multiple of 256 bytes so the inner view is as aligned as the allocation."""
    count = int(np.prod(shape))
    raw = torch.full((lead + count + tail,), fill, dtype=dtype, device=device)
    assert (lead * raw.element_size()) % 256 == 0, "lead band must keep the 256-byte alignment"
    bits = raw.view(_INT_VIEW[raw.element_size()])
    pattern = bits[0].clone() if lead + tail + count else None
    inner = raw[lead:lead + count].view(shape)

    def check(what=""):
        front, back = bits[:lead], bits[lead + count:]
        bad = int((front != pattern).sum()) + int((back != pattern).sum())
        assert bad == 0, f"{what}: {bad} guard elements were overwritten"

    check.raw = raw
    return inner, check


# --------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------
INPUT_SETS = ("centred", "postleaky")


def real_inputs(tag, case, input_set):
    """Real-valued operands of ``case`` (a dict with n, h, w, cin, cout, k and optionally res): x NHWC from the input set -
    ``centred``: U(-1, 1); ``postleaky``: leaky(U(-0.8, 1.3)), mean about +0.4 like the activations between two layers -
    weights N(0, 2 / K) OHWI, scale U(0.5, 1.5), shift U(-0.5, 0.5), residual U(-1, 1)."""
    n, h, w, cin, cout, k = (case[key] for key in ("n", "h", "w", "cin", "cout", "k"))
    if input_set == "centred":
        x = synth.uniform(tag + "x", (n, h, w, cin), -1.0, 1.0)
    elif input_set == "postleaky":
        x = synth.uniform(tag + "x", (n, h, w, cin), -0.8, 1.3)
        x = np.where(x > 0, x, np.float32(0.1) * x).astype(np.float32)
    else:
        raise ValueError(input_set)
    kk = k * k * cin
    wgt = synth.normal(tag + "w", (cout, k, k, cin), 0.0, (2.0 / kk) ** 0.5)
    scale = synth.uniform(tag + "s", (cout,), 0.5, 1.5)
    shift = synth.uniform(tag + "b", (cout,), -0.5, 0.5)
    res = None
    if case.get("res"):
        s, pad = case.get("s", 1), case.get("pad", (k - 1) // 2)
        res = synth.uniform(tag + "r", (n, out_size(h, k, s, pad), out_size(w, k, s, pad), cout), -1.0, 1.0)
    return x, wgt, scale, shift, res


def torch_fp32(x, w, scale, shift, k, stride, pad, act, res=None, ups=1):
    """The yardstick of the precision bar: the same fused operation with stock torch float32 ops on the CPU (NHWC in / out)."""
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()  # noqa: E731
    y = F.conv2d(t(x).permute(0, 3, 1, 2), t(w).permute(0, 3, 1, 2), None, stride, pad)
    y = y * t(scale).view(1, -1, 1, 1) + t(shift).view(1, -1, 1, 1)
    if act == LEAKY:
        y = F.leaky_relu(y, 0.1)
    elif act == SIGMOID:
        y = torch.sigmoid(y)
    if res is not None:
        y = y + t(res).permute(0, 3, 1, 2)
    if ups == 2:
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# --------------------------------------------------------------------------------------
# part A: the fp32 precision bar - one small set of shapes per kernel family
# --------------------------------------------------------------------------------------
def _c(name, n, h, w, cin, cout, k, s, act, inputs, res=False, ups=1, split=1, nchw=False, pad=None):
    return dict(name=name, n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, pad=(k - 1) // 2 if pad is None else pad, act=act,
                inputs=inputs, res=res, ups=ups, split=split, nchw=nchw)


def _general(shallow_cin, split):
    """Deep K (two couts), shallow ragged, stride 2, 1x1, residual + split-K 3, upsample, sigmoid."""
    return [
        _c("deep256", 2, 13, 13, 512, 256, 3, 1, LEAKY, "centred", split=split),
        _c("deep255", 2, 13, 13, 512, 255, 3, 1, LEAKY, "postleaky", split=split),
        _c("ragged", 2, 13, 11, shallow_cin, 72, 3, 1, LEAKY, "postleaky", split=split),
        _c("stride2", 2, 16, 16, 32, 64, 3, 2, LEAKY, "centred", split=split),
        _c("k1", 1, 13, 13, 128, 255, 1, 1, LINEAR, "postleaky", split=split),
        _c("res_split3", 2, 13, 13, 64, 96, 3, 1, LEAKY, "centred", res=True, split=3),
        _c("ups", 1, 13, 13, 64, 48, 1, 1, LEAKY, "postleaky", ups=2, split=split),
        _c("sigmoid", 1, 10, 12, 32, 40, 3, 1, SIGMOID, "centred", split=split),
    ]


P8_128 = (121, 131, 201, 221, 311, 321)
P8_256 = (100, 110, 200)
FAMILIES = {
    # name: (tile ids, cases)
    "buffer": ((1, 2, 3, 4, 5, 7), _general(48, 1)),
    "dma": ((21, 22, 23, 24, 25, 6), _general(24, 1)),
    "register": ((51, 52, 53, 54, 55, 31), _general(24, 1)),
    "tail": ((41, 42, 43, 44, 45, 47), _general(48, 3)),
    "ws1x1": ((50,), [_c("k1_512_255", 3, 13, 11, 512, 255, 1, 1, LINEAR, "centred"),
                      _c("k1_64_72", 3, 13, 11, 64, 72, 1, 1, LEAKY, "postleaky")]),
    "ws3x3": ((60,), [_c("c64_res", 2, 13, 11, 64, 72, 3, 1, LEAKY, "postleaky", res=True),
                      _c("c32_s2", 2, 16, 16, 32, 64, 3, 2, LEAKY, "centred")]),
    "patch128": (P8_128, [_c("deep256", 2, 13, 13, 512, 256, 3, 1, LEAKY, "centred"),
                          _c("shallow_res", 2, 13, 11, 48, 128, 3, 1, LEAKY, "postleaky", res=True)]),
    "patch256": (P8_256, [_c("deep256", 2, 13, 13, 512, 256, 3, 1, LEAKY, "centred"),
                          _c("shallow_res", 2, 13, 11, 48, 256, 3, 1, LINEAR, "postleaky", res=True)]),
    "stem": ((0, 92, 91), [_c("nchw32", 3, 13, 21, 3, 32, 3, 1, LEAKY, "centred", nchw=True),
                           _c("nhwc64_sig", 2, 17, 9, 3, 64, 3, 1, SIGMOID, "postleaky")]),
    "smallcin4": ((0,), [_c("cin4", 1, 9, 9, 4, 20, 3, 1, LEAKY, "postleaky"),
                         _c("cin4_lin", 2, 7, 5, 4, 8, 3, 1, LINEAR, "centred")]),
}
# the fp32-output form of the 16-bit path: operands rounded to the storage type first
H16_F32OUT = [_c("deep255", 2, 13, 13, 512, 255, 3, 1, LEAKY, "postleaky"),
              _c("k1_res", 1, 13, 13, 128, 255, 1, 1, LINEAR, "centred", res=True),
              _c("ragged96", 2, 13, 11, 96, 72, 3, 1, LEAKY, "centred")]


def part_a_cases():
    """Every distinct (case, K) of part A: [(family, case)]."""
    out = [(fam, case) for fam, (_tiles, cases) in FAMILIES.items() for case in cases]
    return out + [("h16_f32out", case) for case in H16_F32OUT]


def bar(e_torch, kk):
    """Part A: 16 x the error of stock torch fp32, never more than the format bound K * 2^-24."""
    return min(16.0 * e_torch, kk * U24)


# --------------------------------------------------------------------------------------
# part B: shapes that make every mask do work
# --------------------------------------------------------------------------------------
TILE_SHAPE = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (128, 32), 5: (256, 128), 7: (64, 64), 6: (256, 128)}
for _t in (1, 2, 3, 4, 5):
    TILE_SHAPE[20 + _t] = TILE_SHAPE[40 + _t] = TILE_SHAPE[_t]
TILE_SHAPE[47] = (64, 64)
for _t, _s in ((51, (128, 128)), (52, (128, 64)), (53, (64, 64)), (54, (128, 32)), (55, (128, 128)), (31, (128, 128))):
    TILE_SHAPE[_t] = _s


def _b(name, n, h, w, cin, cout, k, s, act, res=False, ups=1, split=1, pad=None, xl=0, xr=0):
    d = _c(name, n, h, w, cin, cout, k, s, act, "centred", res=res, ups=ups, split=split, pad=pad)
    d.update(xl=xl, xr=xr)
    return d


# (x channel slice: xl / xr poisoned channels to the left / right of the slice; y and res always get 8 / 24 around theirs)
POISON_GENERAL = [
    _b("cin24_cout72", 2, 13, 11, 24, 72, 3, 1, LEAKY, xr=8),                  # ragged channel chunk, ragged M, ragged cout
    _b("cin40_cout255_k1", 2, 13, 11, 40, 255, 1, 1, LINEAR, res=True, xl=8),  # ragged chunk, 1x1, ragged rows of 255
    _b("cin16_slices", 1, 5, 7, 16, 72, 3, 1, LEAKY, xl=16, xr=16),            # a map smaller than one tile, slice on each side
    _b("stride2", 2, 13, 11, 32, 72, 3, 2, LEAKY, xl=32),
    _b("k5_pad2", 1, 9, 7, 16, 40, 5, 1, LEAKY, xr=16),
    _b("split3_res_ups", 2, 13, 11, 48, 72, 3, 1, LEAKY, res=True, ups=2, split=3, xl=16),
]
POISON_BUFFER = [dict(c, cin=48) if c["cin"] in (24, 40) else c for c in POISON_GENERAL]  # cin % 16: stay on the buffer kernel
POISON_TAIL_SMALL = _b("tail_small", 2, 13, 11, 48, 72, 3, 1, LEAKY, res=True, split=3, xl=16)   # fewer than 256 tiles
POISON_TAIL_LARGE = {41: (4, 500), 42: (2, 500), 43: (2, 250), 44: (2, 250), 45: (8, 500), 47: (2, 250)}  # tile: (n, cout) at 52x52
# tiles 50 / 60 keep a ring of LDS slots per persistent workgroup, which walks tiles b, b + grid_m, b + 2 grid_m, ...: a slot is
# refilled only from the (NSLOT + 1)-th tile of one workgroup on, so the batches are sized by ws_ring_turns below
POISON_WS1 = [_b("ws1_ragged", 300, 13, 11, 64, 255, 1, 1, LINEAR, xl=32, xr=32), _b("ws1_c128", 480, 13, 11, 128, 72, 1, 1, LEAKY)]
POISON_WS3 = [_b("ws3_s1", 56, 37, 29, 32, 72, 3, 1, LEAKY, res=True, xl=32), _b("ws3_s2", 260, 13, 11, 64, 255, 3, 2, LINEAR, xr=16)]
POISON_P8 = [_b("p8_two_per_tile", 5, 13, 13, 32, 256, 3, 1, LEAKY, res=True, xl=16, xr=16),
             _b("p8_tiny", 1, 5, 7, 16, 256, 3, 1, LINEAR)]
MI355X_CUS = 256


def _ws_grid_m(tiles, tiles_n, lds, minw, nw, cus):
    """csrc/conv_ws_f32.hip launch_w1 / launch_w3r: workgroups along M = min(tiles, resident workgroups per column tile)."""
    per_cu = max(min(160 * 1024 // lds, minw * 4 // nw), 1)
    per_n = max(cus * per_cu // tiles_n // 8 * 8, 8)
    return min(tiles, per_n)


def ws_ring_turns(case, cus=MI355X_CUS):
    """(tiles a workgroup of fp32 tile 50 / 60 walks at the most, ring slots NSLOT) for a POISON_WS1 / POISON_WS3 case: the
    instance table of launch_ws1x1_f32 / launch_ws3x3_f32 and the launchers' grid, restated."""
    cin, cout, k, s = case["cin"], case["cout"], case["k"], case["s"]
    if k == 1:      # (cin, widest cout): WN, WM, NSLOT, MINW
        wn, wm, nslot, minw = {64: ((1, 4, 4, 2) if cout <= 32 else (2, 2, 3, 2) if cout <= 64 else (4, 1, 4, 2)),
                               128: ((2, 2, 2, 2) if cout <= 64 else (4, 1, 3, 2))}[cin]
        tiles = -(-case["n"] * case["h"] * case["w"] // (32 * wm))
        lds = nslot * 32 * wm * cin * 4
    else:           # (cin, stride): WN, WM, tile height, tile width, NSLOT, MINW
        wn, wm, th, tw, nslot, minw = {(32, 1): (2, 2, 4, 16, 3, 2), (32, 2): (2, 2, 4, 16, 2, 2),
                                       (64, 1): (4, 1, 4, 8, 3, 1), (64, 2): (4, 1, 4, 8, 3, 1)}[(cin, s)]
        ho, wo = out_size(case["h"], 3, s, 1), out_size(case["w"], 3, s, 1)
        tiles = case["n"] * -(-ho // th) * -(-wo // tw)
        pieces = -(-((th - 1) * s + 3) * ((tw - 1) * s + 3) * cin * 4 // 1024)
        lds = nslot * -(-pieces // (wn * wm)) * wn * wm * 1024
    grid_m = _ws_grid_m(tiles, -(-cout // (32 * wn)), lds, minw, wn * wm, cus)
    return -(-tiles // grid_m), nslot


def tiles_of(case, bm, bn):
    m = case["n"] * out_size(case["h"], case["k"], case["s"], case["pad"]) * out_size(case["w"], case["k"], case["s"], case["pad"])
    return -(-m // bm) * -(-case["cout"] // bn), m


def receptive_mask(h, w, k, stride, pad, py, px):
    """[ho, wo] bool: outputs whose window contains input pixel (py, px)."""
    ho, wo = out_size(h, k, stride, pad), out_size(w, k, stride, pad)
    oy, ox = np.arange(ho)[:, None] * stride - pad, np.arange(wo)[None, :] * stride - pad
    return (oy <= py) & (py < oy + k) & (ox <= px) & (px < ox + k)


LOCALITY = [  # name, n, h, w, cin, cout, k, stride, pad
    ("k3", 2, 13, 11, 32, 72, 3, 1, 1),
    ("k3s2", 2, 13, 11, 32, 72, 3, 2, 1),
    ("k5", 2, 9, 7, 16, 40, 5, 1, 2),
    ("k1", 2, 13, 11, 64, 72, 1, 1, 0),
]


def locality_pixels(n, h, w):
    """(image, y, x): an interior pixel, a corner, the last pixel of the last image."""
    return [(0, h // 2, w // 2), (0, 0, 0), (n - 1, h - 1, w - 1)]


# --------------------------------------------------------------------------------------
# part C: the 2^31 guards, restated
# --------------------------------------------------------------------------------------
LIMIT = 1 << 31


def buf_addressable(bm, h, w, x_pitch, cin, k, ho, wo, esize=4):
    """csrc/conv.hip buf_addressable<BM> (esize 4) and csrc/conv_h16.hip addressable16 (esize 2), weights of a small cout."""
    span_imgs = (bm - 1) // (ho * wo) + 2
    img_bytes = h * w * x_pitch * esize
    tap_bytes = (k * w + k) * x_pitch * esize + cin * esize
    ktot = k * k * cin
    return span_imgs * img_bytes + 2 * tap_bytes < LIMIT and 256 * ktot * esize + ktot * esize < LIMIT


def ws3x3_f32_window(h, w, x_pitch, esize=4):
    """csrc/conv_ws_f32.hip ws3x3_f32_eligible (esize 4) and csrc/conv3x3_ws_h16.hip ws3x3_eligible (esize 2): one image inside the
    window, coordinates in 12 bits."""
    return h * w * x_pitch * esize < LIMIT and h < 4096 and w < 4096


def ws1x1_window(x_pitch, esize=4):
    """csrc/conv_ws_f32.hip ws1x1_f32_eligible (esize 4) and csrc/conv1x1_ws_h16.hip ws1x1_eligible (esize 2): the 128 rows of the
    tallest tile inside the window.  It depends on the pitch alone."""
    return x_pitch * esize * 128 < LIMIT


def ws1x1_guard_pitches(esize):
    """(largest pitch tile 50 accepts, smallest it refuses) among the pitches the kernels take (16-byte rows)."""
    step = 16 // esize
    refused = LIMIT // (128 * esize)
    return refused - step, refused


def p8_window(n, h, w, x_pitch, esize=4):
    """csrc/conv_p8_f32.hip / conv_p8_h16.hip p8_eligible and me_bneck_h16_supported: padded positions and the images a tile spans."""
    span = 1024 // ((h + 1) * (w + 1)) + 2
    return n * (h + 1) * (w + 1) < LIMIT and span * h * w * x_pitch * esize < LIMIT


P8_GUARD_W = 60   # map width of the patch-resident guard case


def p8_f32_lds_bytes(bm, bn, nwaves, w):
    """csrc/conv_p8_f32.hip launch_p8: three weight stages and two copies of a patch of bm + 2 * (w + 2) rows of 64 bytes, in
    16-row units shared out among the waves."""
    rows = bm + 2 * (w + 2)
    lpa = -(-(-(-rows // 16)) // nwaves)
    return 3 * bn * 64 + 2 * lpa * nwaves * 1024


def largest_h(accepts, lo=1, hi=1 << 24):
    """Largest h with accepts(h), for a predicate that is true up to some h and false beyond."""
    assert accepts(lo) and not accepts(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepts(mid) else (lo, mid)
    return lo


INT_X, INT_W = 3, 2   # part C operands: x in {-3..3}, w in {-2..2}


def exact_sum_bound(kk, scale=1.0, shift=0.0, res=0.0):
    """Largest magnitude any partial sum / epilogue value of a part C case can take: all integers (or power-of-two multiples)
    below 2^24 are exact in fp32, whatever the order of summation."""
    return (INT_X * INT_W * kk) * max(scale, 1.0) + abs(shift) + abs(res)


def sample_bands(rows, row_bytes, band=8, seed=0, extra=4):
    """Start rows of the sampled bands of a tensor of ``rows`` rows of ``row_bytes`` bytes: the first and the last ``band`` rows,
    the ``band`` rows around every multiple of 2^31 bytes, and ``extra`` seeded random ones."""
    starts = {0, max(rows - band, 0)}
    total = rows * row_bytes
    for cut in range(LIMIT, total, LIMIT):
        starts.add(min(max(cut // row_bytes - band // 2, 0), max(rows - band, 0)))
    rng = np.random.RandomState(seed)
    for _ in range(extra):
        starts.add(int(rng.randint(0, max(rows - band, 0) + 1)))
    return sorted(starts)
