"""Shared inputs of the surface tests (tests/test_surfaces_cpu.py, tests/test_gpu_surfaces.py): a seeded dense frame in each
pixel format (tests/pixel_format_refs.py) embedded in a larger buffer - at a byte offset, with a row pitch, the NV12 chroma
plane behind a gap and with a pitch of its own - every byte that is not the picture's filled from a second seed.  The dense
copy is what the dense entry points read; the surface must give its bits whatever the second seed is."""
import numpy as np
import torch

from tests import pixel_format_refs as pf

ROW_BYTES = {"rgb": 3, "bgr": 3, "yuyv": 2, "nv12": 1}   # bytes of plane 0 per pixel of a row


def layout(fmt, h, w, offset=0, pitch_extra=0, uv_gap=0, uv_pitch_extra=0, tail=0):
    """``(pitch, uv_offset, uv_pitch, nbytes)`` of the embedding; the buffer ends ``tail`` bytes behind the picture's last byte."""
    row = ROW_BYTES[fmt] * w
    pitch = row + pitch_extra
    end = offset + (h - 1) * pitch + row
    if fmt != "nv12":
        return pitch, None, None, end + tail
    uv_offset, uv_pitch = offset + h * pitch + uv_gap, w + uv_pitch_extra
    return pitch, uv_offset, uv_pitch, uv_offset + (h // 2 - 1) * uv_pitch + w + tail


def embed_bytes(dense, fmt, h, w, fill_seed, **where):
    """The uint8 numpy buffer of :func:`layout` holding ``dense`` (a native frame of tests/pixel_format_refs.py), every other
    byte uniform from ``fill_seed``."""
    pitch, uv_offset, uv_pitch, nbytes = layout(fmt, h, w, **where)
    offset, row = where.get("offset", 0), ROW_BYTES[fmt] * w
    buf = np.random.RandomState(fill_seed).randint(0, 256, nbytes).astype(np.uint8)
    plane0 = np.asarray(dense).reshape(-1)[:h * row].reshape(h, row)
    for y in range(h):
        buf[offset + y * pitch:offset + y * pitch + row] = plane0[y]
    if fmt == "nv12":
        chroma = np.asarray(dense)[h:]
        for y in range(h // 2):
            buf[uv_offset + y * uv_pitch:uv_offset + y * uv_pitch + w] = chroma[y]
    return buf


def embedded(fmt, h, w, seed, fill_seed=1, flip=False, device="cpu", **where):
    """``(surface, dense, row)``: the ``FrameSurface`` of a seeded ``fmt`` picture embedded by :func:`embed_bytes` in a buffer on
    ``device``, the dense frame (numpy, native layout) and the surface's ``[10]`` descriptor row for the buffer where it is."""
    from millieye_amd.utils.datasets import FrameSurface
    dense = pf.native_frame(fmt, h, w, seed=seed)
    pitch, uv_offset, uv_pitch, _ = layout(fmt, h, w, **where)
    buffer = torch.from_numpy(embed_bytes(dense, fmt, h, w, fill_seed, **where)).to(device)
    surface = FrameSurface(buffer, h, w, fmt, where.get("offset", 0), pitch, uv_offset, uv_pitch)
    return surface, dense, surface.row(buffer.data_ptr(), buffer.numel(), 0, flip)


def extract(surface):
    """The picture of a surface on a CPU buffer copied out into a dense native frame (numpy): what the dense entry points
    would be given."""
    buf, h, w, fmt = surface.buffer.numpy(), surface.h, surface.w, surface.pixel_format
    row = ROW_BYTES[fmt] * w
    plane0 = np.stack([buf[surface.offset + y * surface.pitch:][:row] for y in range(h)])
    if fmt != "nv12":
        return plane0.reshape(h, w, ROW_BYTES[fmt]).copy()
    chroma = np.stack([buf[surface.uv_offset + y * surface.uv_pitch:][:w] for y in range(h // 2)])
    return np.concatenate([plane0, chroma], 0)
