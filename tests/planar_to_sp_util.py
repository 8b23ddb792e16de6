"""Planar frames in, semi-planar surfaces out, for the tests of vfgs_hip_add_grain_frame_list_to_sp_dev / _to_sp8_dev (TEST INFRASTRUCTURE).

The contract (include/vfgs_hip.h) is stated on the planar SOURCE itself: every written container is the sample the planar copy list writes
for the position -- the unchanged oracle's add_grain_frame on a copy of the source, behind vfgs_set_seed(seeds[f]) where seeds are given --
<< sample_shift and truncated to the container, Cb and Cr interleaved (semiplanar_util.to_semiplanar).  The narrowed form narrows first, as
yuv_to_8bit does ((v + 2) >> 2 at depth 10, (v + 8) >> 4 at depth 12).  The result is pasted into the destination's previous bytes exactly
where the call writes (semiplanar_util.written_region: whole 16-sample blocks of the rows of the picture); every other byte is the fill's."""
from __future__ import annotations

import numpy as np

import semiplanar_out8_util as SP8
import semiplanar_util as SP
import vfgs_testlib as T


def dst_frame(width, height, depth, suby, shift, seed, pad=0, uv_pad=None) -> SP.SPFrame:
    """a destination in the depth's container, filled with garbage over the full container range; pitches = whole blocks + pad / uv_pad
    containers (multiples of 16 bytes)"""
    uv_pad = pad if uv_pad is None else uv_pad
    dtype = np.uint16 if depth > 8 else np.uint8
    sz = np.dtype(dtype).itemsize
    assert (pad * sz) % 16 == 0 and (uv_pad * sz) % 16 == 0
    nb16 = (width + 15) // 16 * 16
    crows = (height + suby - 1) // suby
    rng = np.random.default_rng(seed)
    hi = 1 << (8 * sz)
    Y = rng.integers(0, hi, (height, nb16 + pad)).astype(dtype)
    UV = rng.integers(0, hi, (crows, nb16 + uv_pad)).astype(dtype)
    return SP.SPFrame(width, height, depth, suby, nb16 + pad, nb16 + uv_pad, shift, Y, UV)


def paste(twin: SP.SPFrame, fill: SP.SPFrame) -> SP.SPFrame:
    """fill with the written region of `twin` (the semi-planar twin of a grained planar frame) over it"""
    rows, crows, cols = SP.written_region(twin)
    assert fill.dtype == twin.dtype and fill.Y.shape[0] >= rows and fill.UV.shape[0] >= crows and min(fill.stride, fill.uv_stride) >= cols
    w = fill.copy()
    w.Y[:rows, :cols] = twin.Y[:rows, :cols]
    w.UV[:crows, :cols] = twin.UV[:crows, :cols]
    return w


def _fill_of(dst_fill, i):
    return dst_fill[i] if isinstance(dst_fill, (list, tuple)) else dst_fill


def expected(ora, frames, seeds, shift, dst_fill):
    """What _to_sp_dev leaves in the destination of every frame (planar T.Frame sources; dst_fill: one SPFrame for all, or one per frame)."""
    out = []
    for i, f in enumerate(frames):
        g = f.copy()
        if seeds is not None:
            ora.set_seed(seeds[i])
        ora.add_grain_frame(g)
        out.append(paste(SP.to_semiplanar(g, shift), _fill_of(dst_fill, i)))
    return out


def narrowed(g: T.Frame) -> T.Frame:
    """a grained 10- / 12-bit planar frame as yuv_to_8bit leaves it: the same geometry in bytes"""
    n = T.Frame(g.width, g.height, 8, g.subx, g.suby, g.stride, g.cstride)
    n.Y[...], n.U[...], n.V[...] = SP8.narrow(g.Y, g.depth), SP8.narrow(g.U, g.depth), SP8.narrow(g.V, g.depth)
    return n


def expected8(ora, frames, seeds, dst_fill):
    """What _to_sp8_dev leaves in the destination of every frame: narrowed first, then interleaved and pasted."""
    out = []
    for i, f in enumerate(frames):
        assert f.depth in (10, 12)
        g = f.copy()
        if seeds is not None:
            ora.set_seed(seeds[i])
        ora.add_grain_frame(g)
        out.append(paste(SP.to_semiplanar(narrowed(g), 0), _fill_of(dst_fill, i)))
    return out
