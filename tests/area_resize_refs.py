"""numpy restatement of the area-averaging resize of ``me_image_batch_area_u8_f32`` (include/millieye_hip.h), written from
the definition and independent of the kernel, in int64:

    padded square of side P = max(h, w), zeros outside the picture (``diff // 2`` in front), mirrored left-right for ``flip``;
    output index i covers [floor(i P / S), ceil((i + 1) P / S)) on each axis;
    per channel  np.float32(window sum) / np.float32(255 * window area)   - one IEEE division of two exact operands.

The window sums come from an integral image.  tests/test_area_resize_cpu.py pins it to torch's float64 ``area`` interpolation;
tests/test_gpu_area_resize.py compares the kernel with it, bit for bit.  The other pixel formats go through
``tests.pixel_format_refs.to_rgb_u8`` first."""
import numpy as np

from tests import pixel_format_refs as pf


def windows(P, S):
    """``(a, b)``: int64 ``[S]`` window bounds ``[a_i, b_i)`` of the padded axis of length ``P`` (python-int products)."""
    a = np.array([(i * P) // S for i in range(S)], dtype=np.int64)
    b = np.array([-((-(i + 1) * P) // S) for i in range(S)], dtype=np.int64)
    return a, b


def padded_square(rgb, flip=False):
    """uint8 ``[h,w,3]`` -> uint8 ``[P,P,3]``: ``pad_to_square(img, 0)``, then the mirror of the padded square."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    P = max(h, w)
    top, left = ((abs(h - w) // 2, 0) if h <= w else (0, abs(h - w) // 2))
    square = np.zeros((P, P, 3), np.uint8)
    square[top:top + h, left:left + w] = rgb
    return square[:, ::-1] if flip else square


def area_resize(rgb, S, flip=False):
    """RGB uint8 ``[h,w,3]`` -> float32 ``[3,S,S]``."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    P = max(h, w)
    top, left = ((abs(h - w) // 2, 0) if h <= w else (0, abs(h - w) // 2))
    if flip:                       # the mirrored square holds the mirrored picture behind the padding of the other side
        rgb, left = rgb[:, ::-1], P - left - w
    # the padded square is zero outside the picture: its window sums are those of the picture's part of the window, taken
    # from the picture's integral image (a 4099-pixel row is not padded out to 4099 x 4099)
    integral = np.zeros((h + 1, w + 1, 3), np.int64)
    integral[1:, 1:] = rgb.astype(np.int64).cumsum(0).cumsum(1)
    a, b = windows(P, S)
    ya, yb, xa, xb = a[:, None], b[:, None], a[None, :], b[None, :]
    cnt = (yb - ya) * (xb - xa)                                                            # [S,S]: padding counts
    ya, yb = np.clip(ya - top, 0, h), np.clip(yb - top, 0, h)
    xa, xb = np.clip(xa - left, 0, w), np.clip(xb - left, 0, w)
    total = integral[yb, xb] - integral[ya, xb] - integral[yb, xa] + integral[ya, xa]      # [S,S,3]
    assert total.max(initial=0) < 2 ** 31
    out = total.astype(np.float32) / (255 * cnt).astype(np.float32)[:, :, None]
    assert out.dtype == np.float32
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def area_resize_native(frame, fmt, S, flip=False):
    """A frame in pixel format ``fmt`` (tests/pixel_format_refs.py) -> float32 ``[3,S,S]``."""
    return area_resize(pf.to_rgb_u8(frame, fmt), S, flip)


class StreamSource:
    """Picklable pipeline source: ``n`` steps of the RGB frames ``multistream_helpers.stream_frame(s)`` (480 x 640 and
    360 x 480, the same every step) + the radar streams of tests/multistream_helpers."""

    def __init__(self, n, streams):
        self.n, self.streams = n, streams

    def step(self, f):
        from tests import multistream_helpers as mh
        return [mh.stream_frame(s) for s in range(self.streams)], [mh.stream_radar(s, f) for s in range(self.streams)]

    def __call__(self):
        for f in range(self.n):
            yield self.step(f)
