"""Case tables of tests/test_gpu_wgrad_blocks.py (the fp32 weight-gradient kernels behind ``me_conv_wgrad_mfma_f32`` /
``me_conv_wgrad_mfma_oihw_f32``), and the one place that turns a case into the arguments of a call.  Every case NAMES the kernel
form (and, in part B, the reduction form) it is there for; tests/test_wgrad_form_cpu.py asserts through ``me_conv_wgrad_form``,
without a GPU, that the launcher really sends it there, and the GPU tests assert it again on the real pointers before they run.

A case: n, h, w, cin, cout, k, s (stride), pad, and how the operands sit in memory - ``xl`` / ``xr`` (``yl`` / ``yr``): channels
to the left / right of the x (dy) slice inside a wider buffer, so pitch = xl + cin + xr and the pointer is 4 * xl bytes off the
256-byte-aligned buffer - ``oihw``, and ``ws``: 'full' (what me_conv_wgrad_workspace_bytes asks for, at least one slab for OIHW
with k > 1), None (no workspace), or a number of bytes."""
import numpy as np

NULL_CODE, BADARG, NULLPTR, TOOBIG = 0, -1, -2, -4
X_BASE, DY_BASE, DW_BASE, WS_BASE = 0x100000, 0x200000, 0x300000, 0x400000   # stand-in addresses for the query on the CPU
SW_BLOCKS = 768   # partial sums per weight of the stem kernel (csrc/train.hip)


def case(name, form, n, h, w, cin, cout, k, s=1, pad=None, xl=0, xr=0, yl=0, yr=0, oihw=False, ws="full", reduce=None, splits=None):
    return dict(name=name, form=form, n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, pad=(k - 1) // 2 if pad is None else pad,
                xl=xl, xr=xr, yl=yl, yr=yr, oihw=oihw, ws=ws, reduce=reduce, splits=splits)


def out_hw(c):
    return (c["h"] + 2 * c["pad"] - c["k"]) // c["s"] + 1, (c["w"] + 2 * c["pad"] - c["k"]) // c["s"] + 1


def pixels(c):
    ho, wo = out_hw(c)
    return c["n"] * ho * wo


def count(c):
    return c["cout"] * c["k"] * c["k"] * c["cin"]


def full_workspace_bytes(lib, c):
    ho, wo = out_hw(c)
    need = int(lib.me_conv_wgrad_workspace_bytes(c["n"], ho, wo, c["cin"], c["cout"], c["k"]))
    if c["oihw"] and c["k"] > 1:
        need = max(need, 4 * count(c))
    return need


def workspace_bytes(lib, c):
    if c["ws"] is None:
        return 0
    return full_workspace_bytes(lib, c) if c["ws"] == "full" else int(c["ws"])


def query(hip, c, x_ptr=None, dy_ptr=None, dw_ptr=DW_BASE, ws_ptr=WS_BASE, ws_bytes=None):
    """me_conv_wgrad_form on the case: (form name, slices, reduction name) or (negative code, None, None).  Without pointers the
    stand-in addresses carry the case's own alignment."""
    lib = hip.lib()
    nbytes = workspace_bytes(lib, c) if ws_bytes is None else ws_bytes
    x_ptr = X_BASE + 4 * c["xl"] if x_ptr is None else x_ptr
    dy_ptr = DY_BASE + 4 * c["yl"] if dy_ptr is None else dy_ptr
    return hip.wgrad_form(x_ptr, c["xl"] + c["cin"] + c["xr"], dy_ptr, c["yl"] + c["cout"] + c["yr"], dw_ptr, c["n"], c["h"],
                          c["w"], c["cin"], c["cout"], c["k"], c["s"], c["pad"], ws_ptr if nbytes > 0 else None, nbytes, c["oihw"])


def assert_form(hip, c, **ptrs):
    got = query(hip, c, **ptrs)
    assert got[0] == c["form"], f"{c['name']}: the launcher runs {got}, the case is there for {c['form']}"
    if c["reduce"] is not None:
        assert got[2] == c["reduce"], f"{c['name']}: reduction {got[2]}, the case is there for {c['reduce']}"
    if c["splits"] is not None:
        assert got[1] == c["splits"], f"{c['name']}: {got[1]} slices, the case is there for {c['splits']}"
    return got


# ---------------------------------------------------------------------------------------------------------------------
# A. every default form (exact inputs; the case marked real=... also runs real inputs)
# ---------------------------------------------------------------------------------------------------------------------
NINE = "nine_tap"
PART_A = [
    # stem_wgrad_kernel: cin 3, cout 32 (one block of 32) and 36 (a ragged second block), stride 1 / 2, rectangular maps
    case("stem_c32", "stem", 2, 9, 13, 3, 32, 3),
    case("stem_c36_s2", "stem", 2, 10, 7, 3, 36, 3, s=2),
    case("stem_c36_pitched", "stem", 3, 7, 12, 3, 36, 3, xr=2, yr=4),
    # conv_wgrad_pipe_kernel<64,32,4>: cin <= 32
    case("pipe_c4_k3", "pipe_64_32", 2, 9, 11, 4, 64, 3),
    case("pipe_c20_k1", "pipe_64_32", 3, 13, 11, 20, 68, 1),
    case("pipe_c32_s2", "pipe_64_32", 2, 13, 11, 32, 68, 3, s=2),
    case("pipe_c32_k1_sliced", "pipe_64_32", 5, 13, 11, 32, 64, 1, xr=4, yl=4),
    # conv_wgrad_mfma_kernel<true>
    case("mfma_k1_p429", "mfma_vec", 3, 13, 11, 36, 100, 1, splits=2),        # 429 pixels: slices of 224 and 205
    case("mfma_s2_p660", "mfma_vec", 5, 23, 21, 48, 100, 3, s=2, splits=3),   # 660 pixels: 224, 224, 212
    case("mfma_k7_pad0", "mfma_vec", 2, 12, 10, 36, 100, 7, pad=0),
    case("mfma_s2_one_slice", "mfma_vec", 2, 13, 11, 48, 100, 3, s=2, splits=1),
    # conv_wgrad_mfma_kernel<false>: ragged channels; a vector-eligible shape on an odd pitch; on a pointer one float off
    case("scalar_c10_c255", "mfma_scalar", 2, 13, 11, 10, 255, 3),
    case("scalar_pitch", "mfma_scalar", 2, 9, 11, 36, 100, 3, xr=1),
    case("scalar_dy_pitch", "mfma_scalar", 2, 9, 11, 36, 100, 3, yr=2),
    case("scalar_pointer", "mfma_scalar", 2, 9, 11, 36, 100, 3, xl=1, xr=3),
    # conv_wgrad_tile_kernel<128,128>: exactly 16384 pixels, a ragged second tile on either side, stride 2
    case("tile_co132", "tile_128_128", 4, 64, 64, 128, 132, 3),
    case("tile_ci132", "tile_128_128", 4, 64, 64, 132, 128, 3),
    case("tile_s2", "tile_128_128", 16, 64, 64, 128, 128, 3, s=2),
    # conv_wgrad9_kernel<2,2,2>: halo rounds 1 / 2 (W = 14 / 15) and 2 / 3 (30 / 31), the full LDS ring, the smallest image,
    # several images inside one 16-position stage, 13 x 13, 2 x 3 tiles
    case("nine_w14", NINE, 2, 3, 14, 64, 64, 3),
    case("nine_w15", NINE, 2, 3, 15, 64, 64, 3),
    case("nine_w30", NINE, 2, 3, 30, 64, 64, 3),
    case("nine_w31", NINE, 2, 3, 31, 64, 64, 3),
    case("nine_w238", NINE, 1, 2, 238, 64, 64, 3),
    case("nine_1x16", NINE, 1, 1, 16, 64, 64, 3),
    case("nine_9x3x4", NINE, 9, 3, 4, 64, 64, 3),
    case("nine_13x13", NINE, 2, 13, 13, 64, 64, 3),
    case("nine_2x3_tiles", NINE, 2, 13, 13, 128, 192, 3),
    case("nine_sliced_operands", NINE, 2, 13, 13, 64, 64, 3, xl=4, xr=8, yr=4),
    # their neighbours on the per-tap kernels
    case("nine_w239_falls_back", "mfma_vec", 1, 2, 239, 64, 64, 3),
    case("nine_1x15_falls_back", "mfma_vec", 1, 1, 15, 64, 64, 3),
]
# one real-input case per form
PART_A_REAL = ["stem_c36_s2", "pipe_c32_s2", "mfma_s2_p660", "scalar_c10_c255", "tile_co132", "nine_13x13", "nine_w31"]

# me_conv_wgrad_f32, the plain kernel (no query: one form): n, h, w, cin, cout, k, s, pad, x pad columns, dy pad columns
PLAIN = [(2, 7, 5, 3, 255, 1, 1, 0, 1, 2), (2, 7, 5, 3, 255, 3, 1, 1, 0, 0), (2, 9, 8, 70, 10, 3, 2, 1, 3, 1),
         (1, 9, 10, 70, 10, 7, 1, 3, 0, 5), (2, 11, 9, 3, 255, 7, 2, 0, 2, 0)]
PLAIN_REAL = (2, 9, 8, 70, 10, 3, 2, 1, 3, 1)

# ---------------------------------------------------------------------------------------------------------------------
# B. poison: one case per form and per reduction form (x / dy always channel slices: 4 or 8 NaN channels on either side)
# ---------------------------------------------------------------------------------------------------------------------
SL = dict(xl=4, xr=8, yl=8, yr=4)
PART_B = [
    case("flat_scalar", "mfma_scalar", 2, 13, 11, 10, 255, 3, xl=3, xr=2, yl=1, yr=4, reduce="flat", splits=2),
    case("flat_v4", "mfma_vec", 3, 13, 11, 36, 100, 1, reduce="flat_v4", splits=2, **SL),
    case("oihw_scalar_c10", "mfma_scalar", 2, 13, 11, 10, 255, 3, xl=3, xr=2, yl=1, yr=4, oihw=True, reduce="oihw"),
    case("oihw_v4", "mfma_vec", 5, 23, 21, 48, 100, 3, s=2, oihw=True, reduce="oihw_v4", splits=3, **SL),
    case("oihw_c100_ragged_block", "mfma_vec", 2, 13, 11, 100, 68, 3, oihw=True, reduce="oihw_v4", **SL),
    case("oihw_one_slice", "mfma_vec", 2, 13, 11, 48, 100, 3, s=2, oihw=True, reduce="oihw_v4", splits=1, **SL),
    case("stem_ohwi", "stem", 2, 10, 7, 3, 36, 3, s=2, xl=1, xr=4, yl=8, yr=4, reduce="stem"),
    case("stem_oihw", "stem", 2, 9, 13, 3, 32, 3, xl=2, xr=1, yl=4, yr=4, oihw=True, reduce="stem"),
    case("pipe_flat_v4", "pipe_64_32", 5, 13, 11, 32, 64, 1, reduce="flat_v4", **SL),
    case("pipe_oihw", "pipe_64_32", 2, 13, 11, 20, 68, 3, s=2, oihw=True, reduce="oihw_v4", **SL),
    case("tile_oihw", "tile_128_128", 4, 64, 64, 128, 132, 3, oihw=True, reduce="oihw_v4", **SL),
    case("tile_flat_v4", "tile_128_128", 4, 64, 64, 132, 128, 3, reduce="flat_v4", **SL),
    case("nine_oihw", NINE, 2, 13, 13, 64, 64, 3, oihw=True, reduce="oihw_v4", **SL),
    case("nine_flat_v4", NINE, 2, 3, 31, 128, 64, 3, reduce="flat_v4", **SL),
    # direct write (one slice, OHWI or 1 x 1): no workspace at all
    case("direct_ohwi", "mfma_vec", 2, 13, 11, 48, 100, 3, s=2, ws=None, reduce="none", splits=1, **SL),
    case("direct_oihw_k1", "pipe_64_32", 1, 13, 11, 20, 68, 1, oihw=True, ws=None, reduce="none", splits=1, **SL),
    case("direct_scalar", "mfma_scalar", 1, 9, 11, 10, 255, 3, xl=3, xr=2, yl=1, yr=4, ws=None, reduce="none", splits=1),
]
LOCALITY = ["flat_scalar", "oihw_v4", "stem_oihw", "pipe_oihw", "tile_oihw", "nine_oihw", "nine_flat_v4", "direct_ohwi"]
# me_conv_wgrad_h16 shares the slab reductions: tile 64 and 128, both layouts: n, h, w, cin, cout, k, s, oihw
H16 = [(2, 13, 11, 64, 72, 3, 1, True), (3, 13, 11, 64, 72, 1, 1, False), (2, 13, 13, 128, 128, 3, 1, True),
       (2, 26, 26, 128, 128, 3, 2, False)]

# ---------------------------------------------------------------------------------------------------------------------
# C. the workspace contract: (shape, form with the full workspace)
# ---------------------------------------------------------------------------------------------------------------------
PART_C = [case("ws_nine", NINE, 2, 13, 13, 64, 128, 3), case("ws_sliced", "mfma_vec", 5, 23, 21, 48, 100, 3, s=2, splits=3),
          case("ws_stem", "stem", 2, 9, 13, 3, 32, 3)]

# ---------------------------------------------------------------------------------------------------------------------
# D. the forms only a process switch reaches: child name -> (environment, cases)
# ---------------------------------------------------------------------------------------------------------------------
_NINE_SHAPES = [c for c in PART_A if c["form"] == NINE]
CHILDREN = {
    "tile128": (dict(MILLIEYE_WGRAD_TILE="128"), [
        case("t128x64_k3", "tile_128_64", 2, 13, 11, 64, 132, 3, oihw=True),
        case("t128x64_c36_k1", "tile_128_64", 3, 13, 11, 36, 128, 1),
        case("t128x64_s2", "tile_128_64", 2, 13, 11, 100, 192, 3, s=2),
        case("t64x128_k3", "tile_64_128", 2, 13, 11, 132, 64, 3, oihw=True),
        case("t64x128_k1", "tile_64_128", 3, 13, 11, 128, 100, 1),
        case("t64x128_s2", "tile_64_128", 2, 13, 11, 192, 68, 3, s=2),
    ]),
    "depth5": (dict(MILLIEYE_WGRAD_DEPTH="5", MILLIEYE_WGRAD_TILE="128"), [
        case("p128x128", "pipe_128_128", 2, 13, 11, 132, 128, 3, oihw=True),
        case("p128x128_k1", "pipe_128_128", 3, 13, 11, 128, 132, 1),
        case("p128x128_s2", "pipe_128_128", 2, 13, 11, 128, 128, 3, s=2),
        case("p128x64", "pipe_128_64", 2, 13, 11, 64, 132, 3, oihw=True),
        case("p128x64_k1", "pipe_128_64", 3, 13, 11, 36, 128, 1),
        case("p64x128", "pipe_64_128", 2, 13, 11, 132, 64, 3, oihw=True),
        case("p64x128_s2", "pipe_64_128", 2, 13, 11, 192, 68, 3, s=2),
        case("p64x64", "pipe_64_64", 2, 13, 11, 36, 100, 3, oihw=True),
        case("p64x64_k1", "pipe_64_64", 3, 13, 11, 48, 68, 1),
        case("p64x64_k7", "pipe_64_64", 2, 12, 10, 36, 100, 7, pad=0),
        case("p64x32_stays", "pipe_64_32", 2, 13, 11, 32, 68, 3, s=2),
    ]),
    "per_tap": (dict(MILLIEYE_WGRAD9="0", MILLIEYE_WGRAD_DEPTH="1"),
                [dict(c, form="mfma_vec", name=c["name"] + "_per_tap") for c in _NINE_SHAPES] + [
        case("c4_on_mfma", "mfma_vec", 2, 9, 11, 4, 64, 3),
        case("c20_k1_on_mfma", "mfma_vec", 3, 13, 11, 20, 68, 1),
        case("c32_s2_on_mfma", "mfma_vec", 2, 13, 11, 32, 68, 3, s=2, oihw=True),
        case("tile_per_tap", "tile_128_128", 4, 64, 64, 128, 128, 3),
    ]),
    "nine4w": (dict(MILLIEYE_WGRAD9_NG="1"),
               [dict(c, form="nine_tap_4w", name=c["name"] + "_4w") for c in _NINE_SHAPES]
               + [dict(c, form="nine_tap_4w", name=c["name"] + "_4w_oihw", oihw=True) for c in _NINE_SHAPES[-3:]]),
}


def ints(rng, shape, lo=-4, hi=4):
    return rng.randint(lo, hi + 1, shape).astype(np.float32)
