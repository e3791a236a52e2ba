"""No GPU: tests/frame_modes_refs.py against the torch ops and the host rule it restates."""
import numpy as np
import pytest
import torch

from tests import frame_modes_refs as refs


def _torch_order(keep, key):
    keep, key = torch.as_tensor(keep), torch.as_tensor(key)
    ranked = torch.nonzero((keep != 0) & (keep != 2)).flatten()
    ranked = ranked[torch.sort(key[ranked], descending=True, stable=True).indices]
    passed = torch.nonzero(keep == 2).flatten()
    return torch.cat([ranked, passed]).numpy(), (len(ranked), len(passed))


@pytest.mark.parametrize("values", [(0, 1, 2), (0, 2), (0, 1), (0,), (1,), (2,), (1, 2)])
@pytest.mark.parametrize("cap", [0, 1, 37, 300])
def test_two_segment_order_is_stable_sort_plus_concatenation(values, cap):
    g = torch.Generator().manual_seed(11 + cap + 7 * len(values))
    keep = torch.tensor(values, dtype=torch.uint8)[torch.randint(0, len(values), (cap,), generator=g)].numpy()
    key = (torch.randint(0, 6, (cap,), generator=g).float() / 8).numpy()   # six distinct keys: ties everywhere
    order, counts = refs.two_segment_order(keep, key)
    want, want_counts = _torch_order(keep, key)
    assert counts == want_counts
    assert np.array_equal(order, want)
    assert counts[0] == int(((keep != 0) & (keep != 2)).sum()) and counts[1] == int((keep == 2).sum())
    if cap >= 37 and 1 in values:
        assert len(np.unique(key[order[:counts[0]]])) < counts[0], "the case must hold ties"


def test_two_segment_order_small_example():
    keep = np.array([2, 1, 0, 1, 2, 1, 1], dtype=np.uint8)
    key = np.array([9.0, 0.5, 7.0, 0.75, 0.1, 0.5, 0.75], dtype=np.float32)
    order, counts = refs.two_segment_order(keep, key)
    assert order.tolist() == [3, 6, 1, 5, 0, 4] and counts == (4, 2)


def test_mode_rule_compares_in_double():
    edge = np.float32(0.08)
    up, down = np.nextafter(edge, np.float32(1)), np.nextafter(edge, np.float32(0))
    assert float(edge) < 0.08 < float(up)   # the float32 nearest to 0.08 lies below the double 0.08
    means = np.array([edge, up, down, 0.0, 1.0], dtype=np.float32)
    assert refs.mode_rule(means, 0.08).tolist() == [0, 1, 0, 0, 1]
    # the host rule of MultiStreamFuser._modes / demo.mode_selection
    assert refs.mode_rule(means, 0.08).tolist() == [0 if float(m) < 0.08 else 1 for m in torch.from_numpy(means)]
    # a float32 comparison would call the edge itself bright
    assert not (edge < np.float32(0.08))
