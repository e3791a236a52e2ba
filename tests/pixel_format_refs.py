"""numpy restatement of the pixel formats of ``me_image_batch_formats_u8_f32`` (include/millieye_hip.h), written from the
definition and independent of the kernel: chroma addressing of NV12 / YUYV, and the integer limited-range BT.601 conversion
that OpenCV's ``cvtColor`` uses for ``COLOR_YUV2RGB_NV12`` / ``COLOR_YUV2RGB_YUY2``, in int64:

    y = max(0, Y - 16) * 1220542;   u = U - 128;   v = V - 128
    R = clamp((y + (1 << 19) + 1673527 * v)               >> 20, 0, 255)
    G = clamp((y + (1 << 19) -  852492 * v - 409993 * u)  >> 20, 0, 255)
    B = clamp((y + (1 << 19) + 2116026 * u)               >> 20, 0, 255)

tests/test_pixel_formats_cpu.py pins it (known answers, the float formula, hand-written addressing tables, cv2 where
installed); tests/test_gpu_pixel_formats.py compares the kernel with it.  Also the seeded native frames and the picklable
pipeline source those tests share."""
import numpy as np

FORMATS = ("rgb", "bgr", "nv12", "yuyv")


def yuv_to_rgb(yuv):
    """int ``[..., 3]`` (Y, U, V) -> uint8 ``[..., 3]`` (R, G, B)."""
    yuv = np.asarray(yuv).astype(np.int64)
    y = np.maximum(0, yuv[..., 0] - 16) * 1220542
    u, v = yuv[..., 1] - 128, yuv[..., 2] - 128
    half = 1 << 19
    r = (y + half + 1673527 * v) >> 20          # numpy's >> on int64 is arithmetic
    g = (y + half - 852492 * v - 409993 * u) >> 20
    b = (y + half + 2116026 * u) >> 20
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def picture_hw(frame, fmt):
    frame = np.asarray(frame)
    if fmt == "nv12":
        assert frame.ndim == 2 and frame.shape[0] % 3 == 0 and frame.shape[1] % 2 == 0, frame.shape
        return frame.shape[0] // 3 * 2, frame.shape[1]
    assert frame.ndim == 3 and frame.shape[2] == (2 if fmt == "yuyv" else 3), frame.shape
    return frame.shape[0], frame.shape[1]


def yuv444(frame, fmt):
    """The (Y, U, V) every pixel of an NV12 ``[h*3//2, w]`` / YUYV ``[h,w,2]`` frame uses: uint8 ``[h,w,3]``.  Chroma is not
    interpolated: a 2x2 block (NV12) / a pixel pair (YUYV) shares one (U, V)."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8
    h, w = picture_hw(frame, fmt)
    if fmt == "nv12":
        luma = frame[:h]
        uv = frame[h:].reshape(h // 2, w // 2, 2)
        uv = np.repeat(np.repeat(uv, 2, axis=0), 2, axis=1)
    else:
        assert fmt == "yuyv" and w % 2 == 0
        luma = frame[:, :, 0]
        uv = np.stack([frame[:, 0::2, 1], frame[:, 1::2, 1]], -1)   # [h, w/2, (U, V)]
        uv = np.repeat(uv, 2, axis=1)
    return np.concatenate([luma[:, :, None], uv], -1)


def to_rgb_u8(frame, fmt):
    """A frame in ``fmt`` as uint8 ``[h,w,3]`` RGB."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8
    if fmt == "rgb":
        return frame.copy()
    if fmt == "bgr":
        return np.ascontiguousarray(frame[:, :, ::-1])
    return yuv_to_rgb(yuv444(frame, fmt))


def native_shape(fmt, h, w):
    return {"rgb": (h, w, 3), "bgr": (h, w, 3), "yuyv": (h, w, 2), "nv12": (h * 3 // 2, w)}[fmt]


def native_frame(fmt, h, w, seed, dark=False):
    """Seeded uint8 frame of picture size (h, w) in ``fmt``: every byte uniform over 0 .. 255; ``dark``: a picture whose
    network input has a mean below the demos' 0.08 (luma 16 .. 40 and near-neutral chroma for the YUV formats)."""
    rng = np.random.RandomState(seed)
    shape = native_shape(fmt, h, w)
    if not dark:
        return rng.randint(0, 256, shape).astype(np.uint8)
    if fmt in ("rgb", "bgr"):
        return rng.randint(0, 26, shape).astype(np.uint8)
    frame = rng.randint(120, 137, shape).astype(np.uint8)    # chroma everywhere ...
    luma = rng.randint(16, 41, (h, w)).astype(np.uint8)      # ... then the luma bytes
    if fmt == "nv12":
        frame[:h] = luma
    else:
        frame[:, :, 0] = luma
    return frame


class NativeSource:
    """Picklable pipeline source: ``n`` steps of ``len(formats)`` native frames (the same every step; stream ``s`` has the
    picture size ``sizes[s % len(sizes)]``, odd streams are dark) + the radar streams of tests/multistream_helpers."""

    def __init__(self, n, formats, sizes=((32, 48), (40, 36))):
        self.n, self.formats, self.sizes = n, list(formats), sizes
        self._frames = None

    def step(self, f):
        from tests import multistream_helpers as mh
        if self._frames is None:
            self._frames = [native_frame(fmt, *self.sizes[s % len(self.sizes)], seed=70 + s, dark=s % 2 == 1)
                            for s, fmt in enumerate(self.formats)]
        return self._frames, [mh.stream_radar(s, f) for s in range(len(self.formats))]

    def __call__(self):
        for f in range(self.n):
            yield self.step(f)
