"""No GPU: pins the float64 references of tests/conv_refs.py to stock torch float64 and to a naive five-loop convolution, and
checks - for every table tests/test_gpu_conv_blocks.py draws its inputs from - the facts that make those tests sound: the
yardstick error of part A is neither zero nor the format bound, the part B shapes are as ragged as they claim, the
receptive-field masks cover some but not all outputs, the part C sums are exact in fp32 and its shapes sit on both sides of
the guards."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_refs as R


def _torch64(x, w, scale, shift, k, stride, pad, act, res=None, ups=1):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    y = F.conv2d(t(x).permute(0, 3, 1, 2), t(w).permute(0, 3, 1, 2), None, stride, pad)
    y = y * t(scale).view(1, -1, 1, 1) + t(shift).view(1, -1, 1, 1)
    if act == R.LEAKY:
        y = F.leaky_relu(y, R.SLOPE)
    elif act == R.SIGMOID:
        y = torch.sigmoid(y)
    if res is not None:
        y = y + t(res).permute(0, 3, 1, 2)
    if ups == 2:
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_fused_conv64_is_torch_float64(k):
    rng = np.random.RandomState(100 + k)
    seen = 0
    for stride in (1, 2, 3):
        for pad in (0, 1, 2):
            n, h, w, cin, cout = 2, 7 + stride, 6 + k, 5, 4
            if h + 2 * pad < k or w + 2 * pad < k:
                continue
            x, wg = rng.randn(n, h, w, cin), rng.randn(cout, k, k, cin)
            scale, shift = rng.rand(cout) + 0.5, rng.randn(cout)
            ho, wo = R.out_size(h, k, stride, pad), R.out_size(w, k, stride, pad)
            for act, with_res, ups in ((R.LINEAR, False, 1), (R.LEAKY, True, 1), (R.SIGMOID, False, 2), (R.LEAKY, True, 2)):
                res = rng.randn(n, ho, wo, cout) if with_res else None
                got = R.fused_conv64(x, wg, scale, shift, k, stride, pad, act, res, ups)
                want = _torch64(x, wg, scale, shift, k, stride, pad, act, res, ups)
                assert got.shape == want.shape == (n, ho * ups, wo * ups, cout)
                np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)
                den = R.abs_sum64(x, wg, scale, shift, k, stride, pad, res, ups)
                ref_den = _torch64(np.abs(x), np.abs(wg), np.abs(scale), np.abs(shift), k, stride, pad, R.LINEAR,
                                   None if res is None else np.abs(res), ups)
                np.testing.assert_allclose(den, ref_den, rtol=1e-13, atol=1e-13)
                assert (den >= np.abs(got) - 1e-12).all() or act == R.SIGMOID
                seen += 1
    assert seen >= 24


def test_fused_conv64_is_the_five_loop_convolution():
    rng = np.random.RandomState(7)
    n, h, w, cin, cout, k, stride, pad = 2, 5, 4, 3, 2, 3, 2, 1
    x, wg = rng.randn(n, h, w, cin), rng.randn(cout, k, k, cin)
    scale, shift = rng.rand(cout) + 0.5, rng.randn(cout)
    ho, wo = R.out_size(h, k, stride, pad), R.out_size(w, k, stride, pad)
    res = rng.randn(n, ho, wo, cout)
    want = np.zeros((n, ho, wo, cout))
    for i in range(n):
        for oy in range(ho):
            for ox in range(wo):
                for o in range(cout):
                    acc = 0.0
                    for ky in range(k):
                        for kx in range(k):
                            iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
                            if 0 <= iy < h and 0 <= ix < w:
                                for c in range(cin):
                                    acc += x[i, iy, ix, c] * wg[o, ky, kx, c]
                    v = acc * scale[o] + shift[o]
                    want[i, oy, ox, o] = (v if v > 0 else R.SLOPE * v) + res[i, oy, ox, o]
    got = R.fused_conv64(x, wg, scale, shift, k, stride, pad, R.LEAKY, res)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)
    # unequal padding (the halo bands of part C): a band of rows with explicit zero rows equals the rows of the whole map
    whole = R.fused_conv64(x, wg, scale, shift, k, 1, 1, R.LINEAR)
    band = R.fused_conv64(x[:, 1:4], wg, scale, shift, k, 1, (0, 0, 1, 1), R.LINEAR)
    assert np.array_equal(band, whole[:, 2:3])


def test_round_to_and_banded():
    v = np.array([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -12, -3.0, 0.1])
    assert R.round_to(v, torch.bfloat16).dtype == torch.bfloat16
    assert R.round_to(v, torch.bfloat16).tolist() == torch.tensor(v).float().bfloat16().tolist()
    assert R.round_to(v, torch.float16).tolist() == [1.001953125, 1.0, -3.0, float(np.float16(np.float32(0.1)))]
    assert R.round_to(v, torch.float32).tolist() == [float(np.float32(t)) for t in v]
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        inner, check = R.banded((3, 5), dtype, 128, 7, float("nan"))
        assert inner.shape == (3, 5) and bool(torch.isnan(inner).all())
        inner.fill_(1.0)
        check("untouched")
        check.raw[127] = 1.0
        with pytest.raises(AssertionError):
            check("front")
        check.raw[127] = float("nan")
        check("restored")
        check.raw[-1] = float("inf")
        with pytest.raises(AssertionError):
            check("back")
    inner, check = R.banded((4,), torch.int32, 64, 64, 0)
    inner += 1
    check("ints")


# every input set the GPU file uses: the fp32 families as they are, the fp32-output form of the 16-bit path rounded to each type
_YARDSTICKS = [(f, c, None) for f, c in R.part_a_cases() if f != "h16_f32out"] + \
              [(f, c, half) for f, c in R.part_a_cases() if f == "h16_f32out" for half in (torch.bfloat16, torch.float16)]


@pytest.mark.parametrize("family,case,half", _YARDSTICKS,
                         ids=[f"{f}-{c['name']}" + (f"-{str(h).split('.')[-1]}" if h else "") for f, c, h in _YARDSTICKS])
def test_part_a_yardstick_is_neither_empty_nor_the_format_bound(family, case, half):
    """e(torch fp32) > 0 and < K * 2^-24 for every input set of part A; the input sets are what they claim to be."""
    x, wg, scale, shift, res = R.real_inputs(f"A/{family}/{case['name']}/", case, case["inputs"])
    if half is not None:
        x, wg = R.round_to(x, half).float().numpy(), R.round_to(wg, half).float().numpy()
    k, s, pad, act, ups = case["k"], case["s"], case["pad"], case["act"], case["ups"]
    kk = k * k * case["cin"]
    assert abs(float(wg.std()) - (2.0 / kk) ** 0.5) < 0.1 * (2.0 / kk) ** 0.5
    if case["inputs"] == "centred":
        assert abs(float(x.mean())) < 0.05 and x.min() >= -1 and x.max() <= 1
    else:
        assert 0.3 < float(x.mean()) < 0.5
    ref = R.fused_conv64(x, wg, scale, shift, k, s, pad, act, res, ups)
    den = R.abs_sum64(x, wg, scale, shift, k, s, pad, res, ups)
    e = R.rel_err(R.torch_fp32(x, wg, scale, shift, k, s, pad, act, res, ups), ref, den)
    assert 0.0 < e < kk * R.U24, (e, kk * R.U24)
    assert 0.0 < R.bar(e, kk) <= kk * R.U24


def test_part_a_families_reach_their_code_paths():
    for fam in ("buffer", "dma", "register", "tail"):
        tiles, cases = R.FAMILIES[fam]
        names = {c["name"]: c for c in cases}
        assert names["deep256"]["cin"] * 9 == 4608 and names["deep255"]["cout"] == 255
        assert names["ragged"]["cout"] == 72 and (names["ragged"]["n"] * 13 * 11) % 64
        assert names["stride2"]["s"] == 2 and names["k1"]["k"] == 1 and names["ups"]["ups"] == 2
        assert names["res_split3"]["res"] and names["res_split3"]["split"] == 3 and names["sigmoid"]["act"] == R.SIGMOID
        for t in tiles:
            assert t in R.TILE_SHAPE
    assert R.FAMILIES["buffer"][1][2]["cin"] % 16 == 0 and R.FAMILIES["tail"][1][2]["cin"] % 16 == 0   # stay on the buffer kernel
    assert R.FAMILIES["dma"][1][2]["cin"] % 16 and R.FAMILIES["register"][1][2]["cin"] % 16           # a ragged channel chunk
    assert all(c["split"] == 3 for c in R.FAMILIES["tail"][1])
    for c in R.FAMILIES["ws1x1"][1]:
        assert c["k"] == 1 and c["cin"] in (64, 128, 256, 384, 512) and not c["res"] and c["act"] != R.SIGMOID
    for c in R.FAMILIES["ws3x3"][1]:
        assert c["k"] == 3 and c["cin"] in (32, 64)
    for fam, width in (("patch128", 128), ("patch256", 256)):
        for c in R.FAMILIES[fam][1]:
            assert c["k"] == 3 and c["s"] == 1 and c["cin"] % 16 == 0 and c["cout"] % width == 0 and c["act"] != R.SIGMOID
    assert all(c["cin"] == 3 and c["cout"] % 32 == 0 for c in R.FAMILIES["stem"][1])
    assert all(c["cin"] == 4 for c in R.FAMILIES["smallcin4"][1])


def test_part_b_shapes_are_as_ragged_as_they_claim():
    for cases in (R.POISON_GENERAL, R.POISON_BUFFER):
        assert {c["name"] for c in cases} == {"cin24_cout72", "cin40_cout255_k1", "cin16_slices", "stride2", "k5_pad2", "split3_res_ups"}
    assert sorted(c["cin"] for c in R.POISON_GENERAL if c["cin"] % 16) == [24, 40]
    assert all(c["cin"] % 16 == 0 for c in R.POISON_BUFFER)
    slices = next(c for c in R.POISON_GENERAL if c["name"] == "cin16_slices")
    assert slices["cin"] == 16 and slices["xl"] > 0 and slices["xr"] > 0
    for tile, (bm, bn) in R.TILE_SHAPE.items():
        for c in R.POISON_GENERAL:
            tiles, m = R.tiles_of(c, bm, bn)
            if c["name"] in ("cin24_cout72", "cin40_cout255_k1"):
                assert m == 2 * 13 * 11 and m % bm and c["cout"] % bn, (tile, c["name"])   # ragged last tile, ragged columns
            if c["name"] == "cin16_slices":
                assert m == 35 and m < bm                                                     # a map smaller than one tile
        tiles, m = R.tiles_of(R.POISON_TAIL_SMALL, bm, bn)
        assert 0 < tiles < 256
    for tile, (n, cout) in R.POISON_TAIL_LARGE.items():
        bm, bn = R.TILE_SHAPE[tile]
        tiles = -(-n * 52 * 52 // bm) * -(-cout // bn)
        assert 256 < tiles < 512 and tiles % 256, (tile, tiles)                               # whole tiles and tail pieces
    # tiles 50 / 60: every persistent workgroup walks more tiles than its ring has slots (ceil(tiles / grid_m) > NSLOT with the
    # launchers' own grid on the 256 CUs of an MI355X), ragged last tiles and cout rows included
    for c in R.POISON_WS1 + R.POISON_WS3:
        turns, nslot = R.ws_ring_turns(c)
        assert turns > nslot, (c["name"], turns, nslot)
    assert R._ws_grid_m(1341, 2, 4 * 32 * 64 * 4, 2, 4, 256) == 256 and R.ws_ring_turns(R.POISON_WS1[0]) == (6, 4)
    assert R.ws_ring_turns(dict(R.POISON_WS1[0], n=9)) == (1, 4)      # a small batch: one tile per workgroup, nothing refilled
    assert (R.POISON_WS1[0]["n"] * 13 * 11) % 32 and R.POISON_WS1[0]["cout"] % 128 and R.POISON_WS3[0]["cout"] % 64
    two = R.POISON_P8[0]
    assert (two["n"], two["h"], two["w"]) == (5, 13, 13) and 2 * 14 * 14 > 128 and 14 * 14 < 256     # two images in a 256-row tile
    assert R.POISON_P8[1]["h"] * R.POISON_P8[1]["w"] < 128


def test_receptive_field_masks_cover_some_and_not_all_outputs():
    for name, n, h, w, cin, cout, k, s, pad in R.LOCALITY:
        ho, wo = R.out_size(h, k, s, pad), R.out_size(w, k, s, pad)
        for img, py, px in R.locality_pixels(n, h, w):
            m = R.receptive_mask(h, w, k, s, pad, py, px)
            assert m.shape == (ho, wo) and 0 < int(m.sum()) < m.size, (name, py, px)
            # against the definition: output (oy, ox) reads (oy * s - pad + ky, ox * s - pad + kx)
            brute = np.zeros((ho, wo), bool)
            for oy in range(ho):
                for ox in range(wo):
                    brute[oy, ox] = any(oy * s - pad + ky == py and ox * s - pad + kx == px for ky in range(k) for kx in range(k))
            assert np.array_equal(m, brute)
        # a NaN pixel gives NaN exactly inside the mask (float64 reference)
        rng = np.random.RandomState(3)
        x, wg = rng.randn(1, h, w, 2), rng.randn(3, k, k, 2) + 3.0
        x[0, h // 2, w // 2] = np.nan
        y = R.fused_conv64(x, wg, np.ones(3), np.zeros(3), k, s, pad, R.LEAKY)
        assert np.array_equal(np.isnan(y[0]).all(-1), R.receptive_mask(h, w, k, s, pad, h // 2, w // 2))
        assert np.array_equal(np.isnan(y[0]).any(-1), np.isnan(y[0]).all(-1))


def test_part_c_sums_are_exact_and_the_shapes_sit_on_both_sides_of_the_guards():
    # every partial sum is an integer below 2^24 (scale a power of two, integer shift / residual)
    for kk, scale, shift, res in ((9 * 16, 2.0, 3.0, 0.0), (9 * 32, 0.5, -2.0, 3.0), (1024, 0.5, 1.0, 0.0), (16, 2.0, 1.0, 3.0),
                                  (64, 2.0, -1.0, 0.0)):
        assert R.exact_sum_bound(kk, scale, shift, res) < 2 ** 24
    rng = np.random.RandomState(5)
    x = rng.randint(-R.INT_X, R.INT_X + 1, (1, 6, 9, 16)).astype(np.float32)
    wg = rng.randint(-R.INT_W, R.INT_W + 1, (8, 3, 3, 16)).astype(np.float32)
    ref = R.fused_conv64(x, wg, np.full(8, 2.0), np.full(8, 3.0), 3, 1, 1, R.LEAKY)
    got = R.torch_fp32(x, wg, np.full(8, 2.0, np.float32), np.full(8, 3.0, np.float32), 3, 1, 1, R.LEAKY)
    assert np.array_equal(got, ref.astype(np.float32))        # exact inputs: fp32 equals the rounded float64 result, any order
    # the fp32 buffer kernel: cin = pitch = 16, 4096 wide, 64-row tiles
    ok = lambda h: R.buf_addressable(64, h, 4096, 16, 16, 3, h, 4096)  # noqa: E731
    h = R.largest_h(ok)
    assert ok(h) and not ok(h + 1) and 2 * h * 4096 * 64 < R.LIMIT <= 2 * (h + 1) * 4096 * 64 + 2 * ((3 * 4096 + 3) * 64 + 64)
    assert R.buf_addressable(256, h, 4096, 16, 16, 3, h, 4096) == ok(h)            # the span factor is 2 for every tile height here
    ok60 = lambda h: R.ws3x3_f32_window(h, 4095, 64)  # noqa: E731
    assert R.largest_h(ok60) == 2048
    okp8 = lambda h: R.p8_window(1, h, R.P8_GUARD_W, 64)  # noqa: E731
    assert R.largest_h(okp8) == 69905
    # tile 221 (256 x 128, 8 waves, two workgroups per CU: 80 KB each) takes the 60-wide map, not a 64-wide one
    assert R.p8_f32_lds_bytes(256, 128, 8, R.P8_GUARD_W) == 24576 + 49152 <= 80 * 1024 < R.p8_f32_lds_bytes(256, 128, 8, 64) == 90112
    # the 16-bit twins: the same formulas at two bytes per element
    assert R.largest_h(lambda h: R.p8_window(1, h, R.P8_GUARD_W, 128, 2)) == 69905
    assert R.largest_h(lambda h: R.ws3x3_f32_window(h, 4095, 128, 2)) == 2048
    # tile 50: the pitch alone; (accepted, refused) are neighbours among the pitches with 16-byte rows, ~2.2 GB for 132 pixels
    for es, pair in ((4, (4194300, 4194304)), (2, (8388600, 8388608))):
        assert R.ws1x1_guard_pitches(es) == pair and R.ws1x1_window(pair[0], es) and not R.ws1x1_window(pair[1], es)
        assert pair[0] * es % 16 == 0 and 132 * pair[1] * es < 12 * 2 ** 30 // 4
    okb = lambda h: R.p8_window(1, h, 60, 1024, 2)  # noqa: E731  (me_bneck_h16_supported, 16-bit)
    hb = R.largest_h(okb)
    assert 2 * hb * 60 * 2048 < R.LIMIT <= 2 * (hb + 1) * 60 * 2048
    # sampled bands: both ends, every 2 GiB boundary, inside the tensor
    rows, row_bytes = 66 * 128, 128 * 1024 * 4
    starts = R.sample_bands(rows, row_bytes, seed=1)
    assert starts[0] == 0 and starts[-1] == rows - 8 and all(0 <= s <= rows - 8 for s in starts)
    cuts = [c for c in range(R.LIMIT, rows * row_bytes, R.LIMIT)]
    assert len(cuts) == 2 and all(any(s * row_bytes <= c < (s + 8) * row_bytes for s in starts) for c in cuts)
