"""-m gpu: the 16-byte epilogue of ``conv_igemm_buf_f32`` (whole tiles go through an LDS transpose and store a float4 per lane)
against the 4-byte epilogue it replaces, through the C ABI.

The switch ``MILLIEYE_EPILOGUE16`` (like ``MILLIEYE_STORE_MODE``) is read once per process, so every (switch, store mode) pair
runs in a fresh child process: this file, run as a script, computes every case below and saves the outputs; the six children run
side by side, once per module.  The tests then compare what they saved.

* Bit identity: ``=1`` and ``=0`` give the same bytes - whole output buffers, including the poisoned columns beside a slice.
* Mixed eligibility: launches with whole and ragged tiles, an unaligned ``y`` and 255 channels meet the fp32 precision bar of
  tests/test_gpu_conv_blocks.py against the float64 reference of tests/conv_refs.py.
* Race screen for the LDS reuse: one launch with several workgroups per CU, 20 times, always the same bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (the children below run this file as a script)
    sys.path.insert(0, ROOT)

from tests import conv_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = -7.5
Y_EXTRA, RES_EXTRA = 64, 32   # y_pitch = cout + 64, res_pitch = cout + 32
N, HW = 2, 16                 # M = 512
TILES = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (43, 2), (43, 3)]   # (tile id, split)
# name: (k, cin, cout).  cin 32 walks K tap-major, cin 64 (four 16-channel chunks per tap) chunk-major (choose_order in conv.hip)
SHAPES = {"c3_32_64": (3, 32, 64), "c3_32_128": (3, 32, 128), "k1_64_64": (1, 64, 64), "c3_64_64": (3, 64, 64)}
ACTS = (R.LEAKY, R.LINEAR)
MODES = (0, 1, 2)
MODE_TILES = {0: TILES, 1: [(1, 1), (3, 1), (43, 2)], 2: [(1, 1), (3, 1), (43, 2)]}   # the store modes 1 / 2 run a subset
RACE = dict(name="race", n=8, h=52, w=52, cin=32, cout=64, k=3, s=1, pad=1, act=R.LEAKY, res=True)   # 338 tiles of 64 x 64
RACE_RUNS = 20
MIXED = {   # n = 2, 13 x 13: M = 338 = five whole 64-row tiles and a ragged one (tile 3)
    "cout96": dict(name="cout96", n=2, h=13, w=13, cin=32, cout=96, k=3, s=1, pad=1, act=R.LEAKY, res=True),    # ragged column tile
    "y_off1": dict(name="y_off1", n=2, h=13, w=13, cin=32, cout=64, k=3, s=1, pad=1, act=R.LEAKY, res=True),    # y unaligned
    "cout255": dict(name="cout255", n=2, h=13, w=13, cin=32, cout=255, k=3, s=1, pad=1, act=R.LEAKY, res=False),
}


def _case(shape, act, res):
    k, cin, cout = SHAPES[shape]
    return dict(name=shape, n=N, h=HW, w=HW, cin=cin, cout=cout, k=k, s=1, pad=(k - 1) // 2, act=act, res=res)


def _key(tile, split, shape, act, res, form):
    return f"t{tile}s{split}/{shape}/act{act}/res{int(res)}/{form}"


# --------------------------------------------------------------------------------------
# the child: every case on this process's (MILLIEYE_EPILOGUE16, MILLIEYE_STORE_MODE)
# --------------------------------------------------------------------------------------
def _child(out_path, mode):
    from millieye_amd import hip
    hip.load()
    dev = "cuda"
    inputs = {}

    def operands(case):
        if case["name"] not in inputs:
            x, wg, scale, shift, res = R.real_inputs(f"ep16/{case['name']}/", dict(case, res=True), "centred")
            inputs[case["name"]] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, wg, scale, shift, res))
        return inputs[case["name"]]

    def run(case, tile, split, form, counters=False):
        """form: "wide" = y and the residual are channel slices of wider buffers (different pitches), "dense", or "off1" = a dense
        y that starts one float past a 16-byte boundary.  Returns the whole y allocation."""
        x, wg, scale, shift, res = operands(case)
        n, ho, wo, cout = res.shape
        if form == "wide":
            buf = torch.full((n, ho, wo, cout + Y_EXTRA), POISON, device=dev)
            y = buf[..., :cout]
            rbuf = torch.full((n, ho, wo, cout + RES_EXTRA), POISON, device=dev)
            rbuf[..., :cout] = res
            r = rbuf[..., :cout]
        elif form == "off1":
            buf = torch.full((res.numel() + 4,), POISON, device=dev)
            y = buf[1:1 + res.numel()].view(n, ho, wo, cout)
            r = res
        else:
            buf = torch.full((n, ho, wo, cout), POISON, device=dev)
            y, r = buf, res
        hip.conv2d(x, wg, scale, shift, case["k"], case["s"], case["pad"], case["act"], residual=r if case["res"] else None,
                   out=y, tile=tile, split_k=split, in_launch_reduce=counters)
        torch.cuda.synchronize()
        return buf

    got = {}
    for tile, split in MODE_TILES[mode]:
        for shape in SHAPES:
            for act in ACTS:
                for res in (False, True):
                    got[_key(tile, split, shape, act, res, "wide")] = run(_case(shape, act, res), tile, split, "wide").cpu()
            # the in-launch reduction: the last workgroup of a tile reads the slabs back and goes on to the fused epilogue
            s2 = max(split, 2)
            got[_key(tile, s2, shape, R.LEAKY, True, "counters")] = run(_case(shape, R.LEAKY, True), tile, s2, "wide", True).cpu()
        got[_key(tile, split, "c3_32_64", R.LEAKY, True, "dense")] = run(_case("c3_32_64", R.LEAKY, True), tile, split, "dense").cpu()
    if mode == 0:
        for name, case in MIXED.items():
            got["mixed/" + name] = run(case, 3, 1, "off1" if name == "y_off1" else "dense").cpu()
        # 338 tiles on tile 43: 256 whole tiles with the fused epilogue and 82 cut into slab pieces, in one launch
        got["coexist/reduce_pass"] = run(RACE, 43, 2, "dense").cpu()
        got["coexist/counters"] = run(RACE, 43, 2, "dense", True).cpu()
    first = run(RACE, 3, 1, "dense")
    differ = sum(0 if torch.equal(run(RACE, 3, 1, "dense").view(torch.int32), first.view(torch.int32)) else 1
                 for _ in range(RACE_RUNS - 1))
    got["race/first"] = first.cpu()
    got["race/runs_that_differ"] = torch.tensor(differ)
    torch.save(got, out_path)


@pytest.fixture(scope="module")
def runs(hip_lib, tmp_path_factory):
    """{(epilogue16, store mode): {case key: saved tensor}} from six children running side by side."""
    tmp = tmp_path_factory.mktemp("epilogue16")
    procs = {}
    for ep in (0, 1):
        for mode in MODES:
            out = str(tmp / f"ep{ep}_mode{mode}.pt")
            env = dict(os.environ, MILLIEYE_EPILOGUE16=str(ep), MILLIEYE_STORE_MODE=str(mode))
            procs[(ep, mode)] = (out, subprocess.Popen([sys.executable, os.path.abspath(__file__), out, str(mode)], cwd=ROOT, env=env,
                                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = {key: (out, p.communicate(timeout=600)[0], p.returncode) for key, (out, p) in procs.items()}
    for key, (out, log, rc) in logs.items():
        assert rc == 0, f"child {key}: exit {rc}\n{log.decode(errors='replace')[-4000:]}"
    return {key: torch.load(out) for key, (out, _log, _rc) in logs.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(runs, mode, key):
    new, old = runs[(1, mode)][key], runs[(0, mode)][key]
    assert new.shape == old.shape
    bad = int((_bits(new) != _bits(old)).sum())
    assert bad == 0, f"store mode {mode} {key}: {bad} of {new.numel()} elements differ between the two epilogues"
    return new


def _assert_slice(buf, cout, what):
    """Columns beside the output slice keep their poison; the slice itself is finite and written."""
    assert bool((buf[..., cout:] == POISON).all()), f"{what}: columns beside the output slice were written"
    assert bool(torch.isfinite(buf[..., :cout]).all()) and not bool((buf[..., :cout] == POISON).any()), f"{what}: outputs missing"


_IDENTITY = [(mode, tile, split) for mode in MODES for tile, split in MODE_TILES[mode]]


@pytest.mark.parametrize("mode,tile,split", _IDENTITY, ids=[f"mode{m}-tile{t}-split{s}" for m, t, s in _IDENTITY])
def test_bit_identity(runs, mode, tile, split):
    """3x3 cin 32 -> 64 / 128, 3x3 cin 64 -> 64, 1x1 cin 64 -> 64 at M = 512; leaky and linear; with and without a residual whose
    pitch differs from y's; y a slice of a tensor 64 channels wider (poisoned), and once dense."""
    for shape, (_k, _cin, cout) in SHAPES.items():
        for act in ACTS:
            for res in (False, True):
                key = _key(tile, split, shape, act, res, "wide")
                _assert_slice(_assert_same(runs, mode, key), cout, key)
    key = _key(tile, split, "c3_32_64", R.LEAKY, True, "dense")
    assert bool(torch.isfinite(_assert_same(runs, mode, key)).all()), key


@pytest.mark.parametrize("mode", MODES)
def test_bit_identity_in_launch_reduction(runs, mode):
    """tile_counters set, split 2 (3 for the second tile-43 entry): the epilogue behind the slab read-back."""
    for tile, split in MODE_TILES[mode]:
        for shape, (_k, _cin, cout) in SHAPES.items():
            key = _key(tile, max(split, 2), shape, R.LEAKY, True, "counters")
            _assert_slice(_assert_same(runs, mode, key), cout, key)


def test_whole_tiles_and_slab_pieces_in_one_launch(runs):
    """Tile 43 on 338 tiles: 256 whole tiles take the fused epilogue, 82 are cut in two - summed by the reduce pass, or in the
    launch with arrival counters.  Both forms agree between the epilogues, and with each other (same fixed order of the sum)."""
    a = _assert_same(runs, 0, "coexist/reduce_pass")
    b = _assert_same(runs, 0, "coexist/counters")
    assert bool(torch.isfinite(a).all())
    assert bool(torch.equal(_bits(a), _bits(b)))


@pytest.mark.parametrize("name", list(MIXED))
def test_mixed_eligibility_meets_the_fp32_bar(runs, name):
    """One launch with whole tiles on the 16-byte path and ragged ones (rows past M, cout 96 on 64-wide tiles, cout 255) on the
    4-byte path; an unaligned y makes the whole launch fall back.  Bar of test_gpu_conv_blocks.py part A:
    max |got - ref64| / abs_sum64 <= min(16 x the same figure of stock torch fp32 on the CPU, K * 2^-24)."""
    case = MIXED[name]
    x, wg, scale, shift, res = R.real_inputs(f"ep16/{name}/", dict(case, res=True), "centred")
    res = res if case["res"] else None
    k, s, pad, act = case["k"], case["s"], case["pad"], case["act"]
    ref = R.fused_conv64(x, wg, scale, shift, k, s, pad, act, res)
    den = R.abs_sum64(x, wg, scale, shift, k, s, pad, res)
    e_t = R.rel_err(R.torch_fp32(x, wg, scale, shift, k, s, pad, act, res), ref, den)
    kk = k * k * case["cin"]
    for ep in (1, 0):
        buf = runs[(ep, 0)]["mixed/" + name]
        if name == "y_off1":
            assert bool((buf[:1] == POISON).all()) and bool((buf[1 + ref.size:] == POISON).all()), "bytes beside y were written"
            buf = buf[1:1 + ref.size].view(ref.shape)
        e_k = R.rel_err(buf.numpy(), ref, den)
        print(f"{name} epilogue16={ep}: kernel {e_k:.3e}  torch {e_t:.3e}  K*2^-24 {kk * R.U24:.3e}")
        assert e_k <= R.bar(e_t, kk), (name, ep, e_k, e_t)
    _assert_same(runs, 0, "mixed/" + name)


@pytest.mark.parametrize("mode", MODES)
def test_lds_reuse_race_screen(runs, mode):
    """64 x 64 tiles with residual at n = 8, 52 x 52, cin 32 -> 64: 338 workgroups, several per CU, so one workgroup's transpose
    runs beside the K loops of others.  20 runs in one process give the same bytes, and they are those of the 4-byte epilogue."""
    for ep in (0, 1):
        assert int(runs[(ep, mode)]["race/runs_that_differ"]) == 0, f"epilogue16={ep}: runs differ from the first"
    assert bool(torch.isfinite(_assert_same(runs, mode, "race/first")).all())


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]))
