"""-m gpu: ``me_image_batch_surfaces_u8_f32`` and what is built on it.  The governing property: a frame read through its
surface - pitch, offset, NV12 chroma plane of its own, a buffer of its own - gives the bits the dense entry point
(``me_image_batch_letterbox_u8_f32`` for the nearest resize, ``me_image_batch_area_u8_f32`` for the area resize) gives on its
pixels copied into a dense frame, whatever the bytes around the picture are.  The stock torch CPU references of
tests/letterbox_refs.py and tests/area_resize_refs.py are compared as well, so that not only HIP is compared with HIP.

Every descriptor of this file, the invalid ones included, points into a live allocation large enough for the picture it
claims: a wrong kernel shows as a wrong answer."""
import functools
import pickle

import numpy as np
import pytest
import torch

from millieye_amd import synth
from tests import area_resize_refs as ar, letterbox_refs as lr, multistream_helpers as mh, pixel_format_refs as pf
from tests import surface_helpers as sfh
from tests.golden.make_golden import RADAR_CALIB

pytestmark = pytest.mark.gpu

E_BADARG, E_NULLPTR, E_ALIGN, E_TOOBIG = -1, -2, -3, -4      # include/millieye_hip.h
GUARD, SENTINEL = 64, 12345.0                                # floats in front of and behind dst (64: dst stays 16-byte aligned)
NEAREST, AREA = 0, 1


def _launch(rows, H, W, resize):
    """One ``me_image_batch_surfaces_u8_f32`` call on ``[n][10]`` descriptor rows: ``[n,3,H,W]`` on the host.  dst is NaN between
    two sentinel blocks; the sentinels must survive and every element must come back finite."""
    from millieye_amd import hip
    n = len(rows)
    d_desc = torch.tensor(rows, dtype=torch.int64).reshape(n, 10).cuda()
    buf = torch.full((2 * GUARD + n * 3 * H * W,), float("nan"), device="cuda", dtype=torch.float32)
    buf[:GUARD] = SENTINEL
    buf[-GUARD:] = SENTINEL
    dst = buf[GUARD:-GUARD]
    hip.check(hip.lib().me_image_batch_surfaces_u8_f32(d_desc.data_ptr(), n, dst.data_ptr(), H, W, resize, hip.stream_ptr()),
              "me_image_batch_surfaces_u8_f32")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[-GUARD:] == SENTINEL).all()), "a sentinel was overwritten"
    out = host[GUARD:-GUARD].reshape(n, 3, H, W)
    assert bool(torch.isfinite(out).all()), "elements left unwritten"
    return out


def _dense(frames, fmts, flips, H, W, resize):
    """The dense entry point of the mode on dense frames (numpy, native layout): ``[n,3,H,W]`` on the host."""
    from millieye_amd import hip
    from millieye_amd.utils.datasets import StagedRaggedImages
    n = len(frames)
    staged = StagedRaggedImages([torch.from_numpy(np.ascontiguousarray(f)) for f in frames], (H, W), flips, formats=list(fmts)).pack()
    assert tuple(staged.desc.shape) == (n, 5)
    d_src, d_desc = staged.packed.cuda(), staged.desc.cuda()
    out = torch.full((n, 3, H, W), float("nan"), device="cuda")
    if resize == AREA:
        assert H == W
        hip.check(hip.lib().me_image_batch_area_u8_f32(d_src.data_ptr(), int(d_src.numel()), d_desc.data_ptr(), n, out.data_ptr(),
                                                       H, hip.stream_ptr()), "me_image_batch_area_u8_f32")
    else:
        hip.check(hip.lib().me_image_batch_letterbox_u8_f32(d_src.data_ptr(), int(d_src.numel()), d_desc.data_ptr(), n,
                                                            out.data_ptr(), H, W, hip.stream_ptr()), "me_image_batch_letterbox_u8_f32")
    return out.cpu()


def _torch_ref(frame, fmt, flip, H, W, resize):
    if resize == AREA:
        return torch.from_numpy(ar.area_resize_native(frame, fmt, H, bool(flip)))
    return lr.letterbox_nearest(frame, (H, W), fmt, bool(flip))


def _equal(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: {got[i].item()!r} vs "
                             f"{want[i].item()!r}")


class Batch:
    """Pictures embedded back to back in ``nbuf`` buffers (frame ``i`` in buffer ``i % nbuf``): a frame's neighbours in memory
    are other frames' bytes and fill.  ``specs``: ``(fmt, h, w, seed, flip, where)`` with ``where`` for
    ``surface_helpers.layout``; every non-picture byte comes from ``fill_seed``."""

    def __init__(self, specs, fill_seed, nbuf=3):
        from millieye_amd.utils.datasets import FrameSurface
        chunks, placed = [[] for _ in range(nbuf)], []
        self.frames, self.fmts, self.flips = [], [], []
        for i, (fmt, h, w, seed, flip, where) in enumerate(specs):
            dense = pf.native_frame(fmt, h, w, seed=seed)
            start = sum(len(c) for c in chunks[i % nbuf])
            chunks[i % nbuf].append(sfh.embed_bytes(dense, fmt, h, w, fill_seed + i, **where))
            placed.append((start, sfh.layout(fmt, h, w, **where)))
            self.frames.append(dense), self.fmts.append(fmt), self.flips.append(int(flip))
        self.cpu = [torch.from_numpy(np.concatenate(c)) for c in chunks]
        self.cuda = [b.cuda() for b in self.cpu]
        self.surfaces, self.rows = [], []
        for i, ((fmt, h, w, _seed, flip, where), (start, (pitch, uv_off, uv_pitch, _n))) in enumerate(zip(specs, placed)):
            k = i % nbuf
            s = FrameSurface(self.cpu[k], h, w, fmt, start + where.get("offset", 0), pitch,
                             None if uv_off is None else start + uv_off, uv_pitch)
            assert np.array_equal(sfh.extract(s), self.frames[i])
            self.surfaces.append(s)
            self.rows.append(s.row(self.cuda[k].data_ptr(), self.cuda[k].numel(), 0, flip))


# ---- 1, 2: formats x modes x pitches through the C ABI, and the independence of every non-picture byte ----------------------
PICTURES = (("rgb", 10, 14), ("bgr", 14, 10), ("rgb", 9, 33), ("bgr", 10, 14), ("rgb", 14, 10), ("bgr", 9, 33),
            ("nv12", 8, 12), ("nv12", 12, 8), ("yuyv", 9, 12))
PITCH_EXTRA = (0, 1, 5, 64)
# (H, W, resize): nearest to a square, a rectangle and a width that is no multiple of 4 (one store per pixel); area likewise
MODES = ((16, 16, NEAREST), (12, 20, NEAREST), (6, 7, NEAREST), (16, 16, AREA), (7, 7, AREA))


def _format_specs():
    specs = []
    for p, (fmt, h, w) in enumerate(PICTURES):
        for q, extra in enumerate(PITCH_EXTRA):
            i = len(specs)
            # odd offsets; the UV plane behind a gap, its pitch never the Y plane's; both flips for every picture
            where = dict(offset=1 + 2 * (i % 7), pitch_extra=extra, uv_gap=3 + p, uv_pitch_extra=extra + 3, tail=i % 3)
            specs.append((fmt, h, w, 100 + p, (p + q) & 1, where))
    return specs


@functools.lru_cache(maxsize=None)
def _format_run(H, W, resize, fill_seed):
    batch = Batch(_format_specs(), fill_seed)
    return batch, _launch(batch.rows, H, W, resize)


@functools.lru_cache(maxsize=None)
def _format_want(H, W, resize):
    batch, _ = _format_run(H, W, resize, 1000)
    return _dense(batch.frames, batch.fmts, batch.flips, H, W, resize)


@pytest.mark.parametrize("H,W,resize", MODES, ids=lambda v: str(v))
def test_formats_modes_pitches(hip_lib, H, W, resize):
    batch, got = _format_run(H, W, resize, 1000)
    want = _format_want(H, W, resize)
    assert len({r[0] for r in batch.rows}) == 3 and len(set(batch.fmts)) == 4
    for i, (fmt, h, w, _seed, flip, where) in enumerate(_format_specs()):
        what = f"{H} x {W} resize {resize}: frame {i} ({fmt} {h} x {w}, flip {flip}, {where})"
        _equal(got[i], want[i], what)
        if where["pitch_extra"] == 5:   # one pitch per picture against stock torch on the CPU
            _equal(got[i], _torch_ref(batch.frames[i], fmt, flip, H, W, resize), what + " vs torch")
    assert float(want.abs().sum()) > 0


@pytest.mark.parametrize("H,W,resize", MODES, ids=lambda v: str(v))
def test_padding_independence(hip_lib, H, W, resize):
    """The same pictures with every other byte of the buffers drawn anew: not one output bit may move."""
    first, got_a = _format_run(H, W, resize, 1000)
    second, got_b = _format_run(H, W, resize, 2000)
    assert all(np.array_equal(a, b) for a, b in zip(first.frames, second.frames))
    assert any(not torch.equal(a, b) for a, b in zip(first.cpu, second.cpu))
    _equal(got_b, got_a, f"{H} x {W} resize {resize}: another fill")


# ---- 3: the area kernel walking a row in segments, with a pitch ---------------------------------------------------------------
def test_area_segments_with_a_pitch(hip_lib):
    """4 x 1500 RGB (4500-byte rows: wider than one 4096-byte segment) with pitch = row + 3, and 2 x 2100 NV12 (wider than one
    2048-pixel segment) with uv_pitch = w + 2; to size 16, plain and mirrored."""
    specs = []
    for flip in (0, 1):
        specs.append(("rgb", 4, 1500, 31, flip, dict(offset=5, pitch_extra=3, tail=1)))
        specs.append(("nv12", 2, 2100, 32, flip, dict(offset=3, pitch_extra=6, uv_gap=9, uv_pitch_extra=2, tail=2)))
    batch = Batch(specs, 3000, nbuf=2)
    got = _launch(batch.rows, 16, 16, AREA)
    want = _dense(batch.frames, batch.fmts, batch.flips, 16, 16, AREA)
    for i, (fmt, h, w, _seed, flip, _where) in enumerate(specs):
        _equal(got[i], want[i], f"{fmt} {h} x {w} flip {flip}")
        _equal(got[i], _torch_ref(batch.frames[i], fmt, flip, 16, 16, AREA), f"{fmt} {h} x {w} flip {flip} vs torch")


# ---- 4: the buffer's last bytes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resize", (NEAREST, AREA))
def test_buffer_ends_with_the_picture(hip_lib, resize):
    """The last row of every surface ends exactly at ``bytes``; the buffer is the front of a larger allocation.  A 16-byte load
    of the area kernel that would end behind ``bytes`` has to fall back to guarded byte loads: the bytes behind the buffer
    (inside the allocation, so nothing is out of range either way) may not show in the output."""
    specs = (("rgb", 5, 7, 41, 0, dict(offset=3, pitch_extra=2)), ("yuyv", 3, 6, 42, 1, dict(offset=1, pitch_extra=1)),
             ("nv12", 4, 6, 43, 0, dict(offset=1, pitch_extra=3, uv_gap=5, uv_pitch_extra=1)),
             ("bgr", 6, 5, 44, 1, dict(pitch_extra=0)))
    size, runs = 8, []
    for behind in (5, 6):
        rows, keep = [], []
        for i, (fmt, h, w, seed, flip, where) in enumerate(specs):
            surface, dense, _ = sfh.embedded(fmt, h, w, seed, fill_seed=50 + i, **where)
            nbytes = surface.buffer.numel()
            assert surface.span()[1] == nbytes
            tail = torch.from_numpy(np.random.RandomState(behind * 10 + i).randint(0, 256, 64).astype(np.uint8))
            alloc = torch.cat([surface.buffer, tail]).cuda()
            keep.append(alloc)
            rows.append(surface.row(alloc.data_ptr(), nbytes, 0, flip))
        runs.append(_launch(rows, size, size, resize))
    frames = [pf.native_frame(fmt, h, w, seed=seed) for fmt, h, w, seed, _f, _w in specs]
    want = _dense(frames, [s[0] for s in specs], [s[4] for s in specs], size, size, resize)
    _equal(runs[0], want, "the surfaces that end with their buffers")
    _equal(runs[1], runs[0], "other bytes behind the buffers")


# ---- 5: 64-bit addressing -----------------------------------------------------------------------------------------------------
def test_addresses_beyond_2_31(hip_lib):
    """An RGB surface 4 x 5 with pitch 2^30 in a buffer of 3 GiB + 15 bytes (its last row ends with the buffer), and one whose
    first byte lies at 2^31 + 5.  Only the rows' bytes are written."""
    nbytes = 3 * (1 << 30) + 15
    try:
        big = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    except RuntimeError as exc:   # (torch.cuda.OutOfMemoryError is one)
        pytest.skip(f"the device refuses a {nbytes}-byte allocation: {str(exc).splitlines()[0]}")
    rng = np.random.RandomState(61)
    fill = [rng.randint(0, 256, 15 if y == 3 else 128).astype(np.uint8) for y in range(4)]
    for y in range(4):
        big[y << 30:(y << 30) + len(fill[y])] = torch.from_numpy(fill[y]).cuda()
    tall = np.stack([f[:15] for f in fill]).reshape(4, 5, 3)
    far = np.stack([fill[2][5 + 20 * y:][:15] for y in range(3)]).reshape(3, 5, 3)    # off = 2^31 + 5, pitch 20
    rows = [[big.data_ptr(), nbytes, 0, 4, 5, 0, 0, 1 << 30, 0, 0], [big.data_ptr(), nbytes, (1 << 31) + 5, 3, 5, 1, 1, 20, 0, 0]]
    for resize in (NEAREST, AREA):
        got = _launch(rows, 4, 4, resize)
        _equal(got, _dense([tall, far], ["rgb", "bgr"], [0, 1], 4, 4, resize), f"resize {resize}")
        _equal(got[0], _torch_ref(tall, "rgb", 0, 4, 4, resize), f"resize {resize} vs torch")


# ---- 6: crops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb", "bgr", "yuyv", "nv12"])
def test_crops(hip_lib, fmt):
    """A 6 x 8 crop at row 2, column 4 of a pitched 16 x 20 picture against the dense kernels on the copied-out crop."""
    surface, dense, _ = sfh.embedded(fmt, 16, 20, seed=71, fill_seed=72, offset=3, pitch_extra=9, uv_gap=7, uv_pitch_extra=4)
    crop = surface.crop(4, 2, 8, 6)
    copied = sfh.extract(crop)
    assert np.array_equal(pf.to_rgb_u8(copied, fmt), pf.to_rgb_u8(dense, fmt)[2:8, 4:12])   # NV12: its chroma rows 1 .. 3
    buffer = surface.buffer.cuda()
    rows = [crop.row(buffer.data_ptr(), buffer.numel(), 0, flip) for flip in (0, 1)]
    for H, W, resize in ((12, 20, NEAREST), (7, 7, AREA)):
        got = _launch(rows, H, W, resize)
        _equal(got, _dense([copied, copied], [fmt, fmt], [0, 1], H, W, resize), f"{fmt} crop, {H} x {W} resize {resize}")
        _equal(got[1], _torch_ref(copied, fmt, 1, H, W, resize), f"{fmt} crop, {H} x {W} resize {resize} vs torch")


# ---- 7: invalid rows, one rule at a time, between valid frames ------------------------------------------------------------------
BASE, BYTES, OFF, HH, WW, FLIP, FMT, PITCH, UV_OFF, UV_PITCH = range(10)


def _invalid_rows():
    """``[(rule, row)]``: valid rows of live buffers with one field changed.  The picture an invalid row claims still lies inside
    the allocation its base points into."""
    keep, out = [], []

    def valid(fmt, h, w, seed, **where):
        surface, _, _ = sfh.embedded(fmt, h, w, seed, fill_seed=seed + 1, **where)
        buffer = surface.buffer.cuda()
        keep.append(buffer)
        return surface.row(buffer.data_ptr(), buffer.numel(), 0, 0)

    row = valid("rgb", 6, 8, 81, offset=3, pitch_extra=5)
    row[PITCH] = 24 - 1
    out.append(("pitch = row - 1", row))
    row = valid("rgb", 6, 8, 82, offset=3, pitch_extra=5)
    row[BYTES] -= 1
    out.append(("the extent one byte short", row))
    row = valid("nv12", 2, 8, 83, offset=1, pitch_extra=2, uv_gap=3, uv_pitch_extra=1, tail=8)
    row[BYTES] = row[UV_OFF] + 8 - 1     # uv_off = bytes - w + 1: the one chroma row ends a byte behind the buffer
    out.append(("uv_off one byte short", row))
    row = valid("nv12", 8, 12, 84, pitch_extra=2, uv_gap=3, uv_pitch_extra=1)
    row[HH] = 7
    out.append(("odd h for NV12", row))
    row = valid("yuyv", 6, 12, 85, pitch_extra=2)
    row[WW] = 11
    out.append(("odd w for YUYV", row))
    row = valid("rgb", 6, 8, 86)
    row[FMT] = 7
    out.append(("format id 7", row))
    row = valid("rgb", 6, 8, 87, offset=32)
    row[BASE], row[BYTES], row[OFF] = row[BASE] + 16, row[BYTES] - 16, -1    # the byte in front of the named buffer is the allocation's
    out.append(("negative off", row))
    return keep, out


def test_invalid_rows_between_valid_frames(hip_lib):
    keep, invalid = _invalid_rows()
    a = Batch([("bgr", 10, 14, 91, 1, dict(offset=1, pitch_extra=5)),
               ("nv12", 8, 12, 92, 0, dict(offset=3, pitch_extra=1, uv_gap=5, uv_pitch_extra=2))], 4000, nbuf=2)
    for H, W, resize in ((12, 20, NEAREST), (16, 16, AREA)):
        want = _dense(a.frames, a.fmts, a.flips, H, W, resize)
        rows = [a.rows[0]]
        for k, (_rule, row) in enumerate(invalid):
            rows += [row, a.rows[(k + 1) % 2]]
        got = _launch(rows, H, W, resize)
        for k, (rule, _row) in enumerate(invalid):
            assert torch.equal(got[1 + 2 * k], torch.zeros(3, H, W)), f"{rule}: the frame is not all zero (resize {resize})"
            _equal(got[2 * k], want[k % 2], f"the frame in front of '{rule}' (resize {resize})")
            _equal(got[2 * k + 2], want[(k + 1) % 2], f"the frame behind '{rule}' (resize {resize})")
    # the area resize's range: max(h, w) = 256 at size 1 is invalid, 255 is the last valid size
    wide = [sfh.embedded("rgb", 1, w, 95 + w, fill_seed=7, pitch_extra=3) for w in (255, 256)]
    buffers = [s.buffer.cuda() for s, _d, _r in wide]
    rows = [s.row(b.data_ptr(), b.numel(), 0, 0) for (s, _d, _r), b in zip(wide, buffers)]
    got = _launch([rows[0], rows[1], rows[0]], 1, 1, AREA)
    want = _dense([wide[0][1]], ["rgb"], [0], 1, 1, AREA)
    assert torch.equal(got[1], torch.zeros(3, 1, 1)) and float(want.abs().sum()) > 0
    _equal(got[0], want[0], "1 x 255 in front of 1 x 256")
    _equal(got[2], want[0], "1 x 255 behind 1 x 256")
    _equal(_launch([rows[1]], 1, 1, NEAREST), _dense([wide[1][1]], ["rgb"], [0], 1, 1, NEAREST), "1 x 256 is valid for the nearest resize")
    del keep


# ---- 8: argument checks ---------------------------------------------------------------------------------------------------------
def test_argument_checks(hip_lib):
    from millieye_amd import hip
    lib = hip.lib()
    surface, _, _ = sfh.embedded("rgb", 6, 8, 97, pitch_extra=5)
    buffer = surface.buffer.cuda()
    desc = torch.tensor([surface.row(buffer.data_ptr(), buffer.numel())], dtype=torch.int64).cuda()
    dst = torch.full((4 + 3 * 16 * 16,), float("nan"), device="cuda")
    stream = hip.stream_ptr()

    def call(desc_ptr, n, dst_ptr, H, W, resize):
        return lib.me_image_batch_surfaces_u8_f32(desc_ptr, n, dst_ptr, H, W, resize, stream)

    assert call(desc.data_ptr(), 1, dst.data_ptr(), 12, 16, AREA) == E_BADARG       # no rectangular area form
    assert b"rectangular" in lib.me_last_error()
    assert call(desc.data_ptr(), 1, dst.data_ptr(), 16, 16, 2) == E_BADARG
    assert call(desc.data_ptr(), 1, dst.data_ptr(), 16, 16, -1) == E_BADARG
    assert call(desc.data_ptr(), 65536, dst.data_ptr(), 16, 16, NEAREST) == E_BADARG
    assert call(desc.data_ptr(), 1, dst.data_ptr(), 0, 16, NEAREST) == E_BADARG
    assert call(None, 1, dst.data_ptr(), 16, 16, NEAREST) == E_NULLPTR
    assert call(desc.data_ptr(), 1, None, 16, 16, NEAREST) == E_NULLPTR
    assert call(desc.data_ptr(), 1, dst.data_ptr(), 1 << 15, 1 << 15, NEAREST) == E_TOOBIG
    for resize in (NEAREST, AREA):   # dst 4 bytes off: refused for width % 4 == 0 alone
        assert call(desc.data_ptr(), 1, dst.data_ptr() + 4, 16, 16, resize) == E_ALIGN
    assert call(desc.data_ptr(), 0, dst.data_ptr(), 16, 16, NEAREST) == 0 and call(None, 0, None, 16, 16, AREA) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()), "a refused call or n == 0 wrote to dst"
    assert call(desc.data_ptr(), 1, dst.data_ptr() + 4, 15, 15, NEAREST) == 0       # width % 4 != 0: scalar stores, any alignment
    torch.cuda.synchronize()
    host = dst.cpu()
    assert bool(torch.isnan(host[:1]).all()) and bool(torch.isfinite(host[1:1 + 3 * 225]).all()) and bool(torch.isnan(host[1 + 3 * 225:]).all())


# ---- 9: StagedSurfaces ----------------------------------------------------------------------------------------------------------
def _staged_inputs():
    """Pitched surfaces of all four formats (256-byte pitch alignment, the NV12 chroma plane behind an aligned height) and a
    crop, two of them in one buffer; with their dense copies."""
    specs = (("rgb", 40, 36), ("bgr", 30, 52), ("nv12", 32, 48), ("yuyv", 24, 40))
    surfaces, frames = [], []
    for i, (fmt, h, w) in enumerate(specs):
        row = sfh.ROW_BYTES[fmt] * w
        where = dict(offset=256 * (i % 2), pitch_extra=-row % 256, uv_gap=256 * 8, uv_pitch_extra=-w % 256, tail=i)
        s, dense, _ = sfh.embedded(fmt, h, w, seed=110 + i, fill_seed=120 + i, **where)
        surfaces.append(s), frames.append(dense)
    crop = surfaces[0].crop(6, 10, 20, 24)     # a second surface of the first buffer
    return surfaces + [crop], frames + [sfh.extract(crop)], [s[0] for s in specs] + ["rgb"], [0, 1, 1, 0, 1]


def _placed(surfaces, how):
    """The surfaces with their buffers moved: ``how[i]`` of ``"pageable"``, ``"pinned"``, ``"cuda"``.  Surfaces that shared a
    buffer and go the same way still share one."""
    from millieye_amd.utils.datasets import FrameSurface
    move = {"pageable": lambda b: b.clone(), "pinned": lambda b: b.pin_memory(), "cuda": lambda b: b.cuda()}
    moved, out = {}, []
    for s, h in zip(surfaces, how):
        key = (s.buffer.data_ptr(), h)
        if key not in moved:
            moved[key] = move[h](s.buffer)
        nv12 = s.pixel_format == "nv12"
        out.append(FrameSurface(moved[key], s.h, s.w, s.pixel_format, s.offset, s.pitch, s.uv_offset if nv12 else None,
                                s.uv_pitch if nv12 else None))
    return out


@pytest.mark.parametrize("size,resize", ((64, None), (64, "area"), ((64, 96), "nearest")), ids=("64", "64-area", "64x96"))
def test_staged_surfaces(hip_lib, size, resize):
    from millieye_amd import hip
    from millieye_amd.utils.datasets import StagedRaggedImages, StagedSurfaces
    surfaces, frames, fmts, flips = _staged_inputs()
    want = StagedRaggedImages([torch.from_numpy(np.ascontiguousarray(f)) for f in frames], size, flips, formats=fmts,
                              resize=resize).to("cuda").cpu()
    assert float(want.abs().sum()) > 0
    n = len(surfaces)
    for how in (["pageable"] * n, ["pinned"] * n, ["cuda"] * n, ["cuda", "pageable", "pinned", "cuda", "pageable"]):
        batch = _placed(surfaces, how)
        assert [s.buffer.is_pinned() for s in batch] == [h == "pinned" for h in how]
        staged = StagedSurfaces(batch, size, flips, resize=resize)
        assert tuple(staged.shape) == tuple(want.shape)
        got = staged.to("cuda")
        assert got.is_cuda and got.dtype == torch.float32
        _equal(got.cpu(), want, f"StagedSurfaces {how} size {size} resize {resize}")
        spans, where = staged.plan()
        assert [w is None for w in where] == [h == "cuda" for h in how]
        assert len(spans) == len({s.buffer.data_ptr() for s, h in zip(batch, how) if h != "cuda"})   # one upload per buffer
        # a CUDA buffer is not copied: the descriptor names the buffer itself
        desc = staged.descriptor([0] * len(spans))
        for i, (s, h) in enumerate(zip(batch, how)):
            if h == "cuda":
                assert int(desc[i, 0]) == s.buffer.data_ptr() and int(desc[i, 1]) == s.buffer.numel() and int(desc[i, 2]) == s.offset
    _equal(staged.type(torch.cuda.FloatTensor).cpu(), want, "type()")
    assert tuple(StagedSurfaces([], size, resize=resize).to("cuda").shape) == (0, 3) + tuple(want.shape[2:])
    with pytest.raises(hip.MeError, match="does not pickle"):
        pickle.dumps(staged)


# ---- 10: the fusers -------------------------------------------------------------------------------------------------------------
STREAMS, FORMATS = 3, ["rgb", "rgb", "nv12"]


@functools.lru_cache(maxsize=None)
def _net():
    from tests.test_gpu_network import _build
    net = _build("demo", "yolov3-tiny-12", 0.1).eval()
    synth.fill_network_(net, "demo", cls0_bias=3.0, cls_bias=-4.0)
    return net.to(net.device)


@functools.lru_cache(maxsize=None)
def _fuser_frames():
    """Per stream the dense camera frame (numpy) and its pitched surface: the scenes of tests/multistream_helpers.py, stream 1
    resident on the device, stream 2 an NV12 decoder surface (pitch aligned to 256, the UV plane behind an aligned height)."""
    from millieye_amd.utils.datasets import FrameSurface
    dense, surfaces = [], []
    for s, fmt in enumerate(FORMATS):
        h, w = mh.FRAME_SIZES[s % 2]
        frame = mh.stream_frame(s) if fmt == "rgb" else pf.native_frame(fmt, h, w, seed=130 + s, dark=True)
        row = sfh.ROW_BYTES[fmt] * w
        where = dict(offset=64 * s, pitch_extra=-row % 256 + 256 * (s == 0), uv_gap=16 * (w + (-w % 256)), uv_pitch_extra=-w % 256)
        pitch, uv_off, uv_pitch, _ = sfh.layout(fmt, h, w, **where)
        buffer = torch.from_numpy(sfh.embed_bytes(frame, fmt, h, w, 140 + s, **where))
        surface = FrameSurface(buffer.cuda() if s == 1 else buffer, h, w, fmt, where["offset"], pitch, uv_off, uv_pitch)
        dense.append(frame), surfaces.append(surface)
    return dense, surfaces


def _same_results(got, want, what):
    assert len(got) == len(want)
    for s, ((rows_a, info_a), (rows_b, info_b)) in enumerate(zip(got, want)):
        _equal(rows_a, rows_b, f"{what}: rows of stream {s}")
        assert info_a.keys() == info_b.keys()
        for key in info_a:
            assert np.array_equal(np.asarray(info_a[key]), np.asarray(info_b[key])), f"{what}: info[{key!r}] of stream {s}"


@pytest.mark.parametrize("img_size,resize", ((64, None), (64, "area"), ((64, 96), None)), ids=("64", "64-area", "64x96"))
def test_multistream_fuser_on_surfaces(hip_lib, img_size, resize):
    from millieye_amd.demo import MultiStreamFuser
    from millieye_amd.utils.datasets import StagedRaggedImages, StagedSurfaces
    net = _net()
    dense, surfaces = _fuser_frames()
    kw = dict(model_mode=3, min_hits=mh.MIN_HITS, img_size=img_size, pixel_format=FORMATS, resize=resize)
    on_dense, on_surfaces, mixed = (MultiStreamFuser(net, RADAR_CALIB, STREAMS, **kw) for _ in range(3))
    rows_total = 0
    for f in range(3):
        radar = [mh.stream_radar(s, f) for s in range(STREAMS)]
        payload = on_dense.prepare(dense, radar)
        assert isinstance(payload["img"], StagedRaggedImages)            # tensors only: the dense path, as before
        want = on_dense.infer(payload)
        payload = on_surfaces.prepare(surfaces, radar)
        assert isinstance(payload["img"], StagedSurfaces) and payload["hw"] == [(s.h, s.w) for s in surfaces]
        _same_results(on_surfaces.infer(payload), want, f"step {f}, surfaces")
        _same_results(mixed([dense[0], surfaces[1], dense[2]], radar), want, f"step {f}, a surface among tensors")
        rows_total += sum(len(r) for r, _i in want)
    assert rows_total > 0


def test_frame_fuser_on_a_surface(hip_lib):
    from millieye_amd.demo import FrameFuser
    net = _net()
    dense, surfaces = _fuser_frames()
    rows_total = 0
    for s, kw in ((2, dict(img_size=(64, 96))), (1, dict(img_size=64, resize="area")), (0, dict(img_size=64))):
        kw.update(model_mode=3, min_hits=mh.MIN_HITS)
        # (stream 0 without a pixel_format: the dense frame goes through the per-frame kernel, the parent's default path)
        fmt = None if s == 0 else FORMATS[s]
        a, b = FrameFuser(net, RADAR_CALIB, pixel_format=fmt, **kw), FrameFuser(net, RADAR_CALIB, pixel_format=fmt, **kw)
        for f in range(3):
            radar = mh.stream_radar(s, f)
            want, got = a(dense[s], radar), b(surfaces[s], radar)
            _same_results([got], [want], f"FrameFuser stream {s} step {f}")
            rows_total += len(want[0])
    assert rows_total > 0
