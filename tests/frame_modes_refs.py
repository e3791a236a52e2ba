"""numpy restatements of the per-frame-mode pieces (tests/test_frame_modes_cpu.py pins them to torch; tests/test_gpu_frame_modes.py
compares the device with them):

* the two-segment order of ``me_compact_sort_rows_modes_f32``: the ranked rows (``keep`` neither 0 nor 2) by descending key, equal
  keys in ascending row order, then the passed-through rows (``keep == 2``) in ascending row order;
* the mode rule of ``me_frame_modes_f32`` / ``MultiStreamFuser._modes``: ``float(mean) < threshold`` in double -> 0, else 1.
"""
import numpy as np


def two_segment_order(keep, key):
    """Row indices in output order and ``(ranked, passed through)``."""
    keep = np.asarray(keep)
    key = np.asarray(key, dtype=np.float32)
    ranked = np.flatnonzero((keep != 0) & (keep != 2))
    # a stable ascending sort of the negated keys = a stable descending sort of the keys (negation is exact and keeps ties)
    ranked = ranked[np.argsort(-key[ranked], kind="stable")]
    passed = np.flatnonzero(keep == 2)
    return np.concatenate([ranked, passed]).astype(np.int64), (int(len(ranked)), int(len(passed)))


def mode_rule(means, threshold):
    """int32 modes of float32 means: the comparison is made in double, like Python's ``float(m) < threshold``."""
    means = np.asarray(means)
    assert means.dtype == np.float32
    return np.where(means.astype(np.float64) < np.float64(threshold), 0, 1).astype(np.int32)
