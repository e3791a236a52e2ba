"""CPU: the yardsticks of the multi-stream output tail (tests/stream_tail_refs.py) - the float32 rescale recipe against
``utils.rescale_boxes`` bit for bit, the restated tail against the torch code of ``MultiStreamFuser(tail="host")`` with the
oracle's NMS in place of the device call, and the guard that keeps the A / B fixture able to catch a shared maximum."""
import numpy as np
import torch

from millieye_amd.utils.utils import rescale_boxes, rescale_scalars
from oracle import tv_ops_np
from tests import stream_tail_refs as refs


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    """Bit for bit, NaNs in the same places (any payload)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(an, bn) and np.array_equal(_bits(a)[~an], _bits(b)[~bn])


def test_rescale_recipe_equals_rescale_boxes_bit_for_bit():
    g = np.random.RandomState(3)
    total = differ = 0
    for hw in refs.FRAME_SHAPES:
        for size in refs.SIZES:
            v = g.uniform(-50, size + 50, size=(4096, 4)).astype(np.float32)
            v[:8] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, size, 1e-42, 3.0e38], np.float32)[:, None]
            want = rescale_boxes(torch.from_numpy(v.copy()), size, hw).numpy()
            got = refs.rescale_f32(v, size, hw)
            total += v.size
            differ += int(v.size - np.count_nonzero((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))
            # the scalars the device path uploads are the restatement's
            assert np.array_equal(rescale_scalars(size, [hw]).numpy()[0],
                                  np.asarray(refs.rescale_scalars(size, hw), np.float64).astype(np.float32))
    print(f"{total} values, {differ} differ in bits")
    assert total == 344064 and differ == 0


def test_tail_restatement_equals_the_host_path_arithmetic():
    """tail_ref against what ``MultiStreamFuser._second_nms`` + ``rescale_boxes`` do, with the oracle's batched_nms per stream
    in place of ``me_nms_boxes_f32``: stable torch sort, bincount, per-stream rows, in-place rescale."""
    streams, hws = 6, [(480, 640), (360, 480), (640, 480), (480, 640), (360, 480), (640, 480)]
    per = [37, 0, 12, 65, 1, 20]
    rows = refs.synthetic_rows(streams, per, seed=11)
    assert len(rows) == sum(per) and not np.all(np.diff(rows[:, 0]) >= 0), "the stream order must be interleaved"
    got = refs.tail_ref(rows, streams, hws, 416, 0.3)
    t = torch.from_numpy(rows)
    order = torch.sort(t[:, 0], stable=True).indices
    grouped = t[order]
    counts = torch.bincount(grouped[:, 0].long(), minlength=streams).tolist()
    assert counts == per
    start = 0
    for s in range(streams):
        mine = grouped[start:start + counts[s]]
        start += counts[s]
        keep = torch.from_numpy(tv_ops_np.batched_nms(mine[:, 1:5].numpy(), mine[:, 5].numpy(), mine[:, 7].numpy(), 0.3))
        want = mine[keep][:, 1:].clone()
        if len(want):
            rescale_boxes(want, 416, hws[s])
        assert got[s].shape == tuple(want.shape) and _same(got[s], want.numpy()), f"stream {s}"
        assert 0 < len(want) < counts[s] or counts[s] <= 1, f"stream {s}: the NMS must suppress something"


def test_fixture_catches_a_shared_maximum():
    """A joint call over groups A and B with the label ``group * 4 + class`` shares B's maximum (1e5): A's 0.005-wide boxes are
    rounded to the float32 grid at 1e5 - 4e5 and its kept set changes.  The grouped entry point must equal the per-group call,
    so the fixture has to keep telling the two apart."""
    b = refs.group_b()
    assert float(b[0].max()) == 1.0e5
    for n, seed in ((65, 1), (300, 2)):
        a = refs.group_a(n, seed)
        assert a[0].min() >= 0 and a[0].max() <= 1 and len(np.unique(a[1])) < n // 4 and set(a[2]) == {0.0, 1.0, 2.0, 3.0}
        w = a[0][:, 2:] - a[0][:, :2]
        assert w.min() >= 0.00499 and w.max() <= 0.01001
        alone = tv_ops_np.batched_nms(*a, 0.3)
        joint = refs.joint_call_kept(a, b, 0.3)
        differ = len(set(alone.tolist()) ^ set(joint.tolist()))
        print(f"group A with {n} boxes: {len(alone)} kept alone, {len(joint)} in the joint call, {differ} rows differ")
        assert 0 < len(alone) < n, "clusters must suppress"
        assert differ >= 1
