"""Semi-planar frames with the narrowed 8-bit destination, for the tests of vfgs_hip_add_grain_sp_frame_list_copy8_dev (TEST INFRASTRUCTURE).

The contract (include/vfgs_hip.h) is stated on D(p), the planar low-aligned picture of the semi-planar SOURCE p: the bytes written are the
planar _copy8 list's on D(p) -- the oracle's frame, every sample narrowed as yuv_to_8bit does (yuv.c:216-258: (v + 2) >> 2 at depth 10,
(v + 8) >> 4 at depth 12, cast to uint8) -- with Cb and Cr interleaved again.  The expectation is written over a copy of the destination's
fill exactly where the call writes (semiplanar_util.written_region: whole 16-sample blocks of the rows of the picture; a UV row as byte
pairs); every other byte of it is the fill's."""
from __future__ import annotations

import numpy as np

import semiplanar_util as SP


def narrow(a, depth):
    """yuv_to_8bit on an array of `depth`-bit samples"""
    assert depth in (10, 12)
    bs = depth - 8
    return ((a.astype(np.uint32) + (1 << (bs - 1))) >> bs).astype(np.uint8)


def dst_frame(width, height, suby, seed, pad=0, uv_pad=None) -> SP.SPFrame:
    """a destination: uint8 planes of garbage; pitches = whole blocks + pad / uv_pad bytes (multiples of 16)"""
    uv_pad = pad if uv_pad is None else uv_pad
    assert pad % 16 == 0 and uv_pad % 16 == 0
    nb16 = (width + 15) // 16 * 16
    crows = (height + suby - 1) // suby
    rng = np.random.default_rng(seed)
    Y = rng.integers(0, 256, (height, nb16 + pad)).astype(np.uint8)
    UV = rng.integers(0, 256, (crows, nb16 + uv_pad)).astype(np.uint8)
    return SP.SPFrame(width, height, 8, suby, nb16 + pad, nb16 + uv_pad, 0, Y, UV)


def expected8(ora, frames, seeds, shift, dst_fill):
    """What the call leaves in the destination of every frame: dst_fill (one SPFrame of uint8 for all frames, or one per frame) with the
    oracle on D(frame) -- behind vfgs_set_seed(seeds[f]) where seeds are given -- narrowed, interleaved and written where the call writes."""
    out = []
    for i, sp in enumerate(frames):
        assert sp.shift == shift and sp.depth in (10, 12)
        d = SP.to_planar(sp)
        if seeds is not None:
            ora.set_seed(seeds[i])
        ora.add_grain_frame(d)
        rows, crows, cols = SP.written_region(sp)
        fill = dst_fill[i] if isinstance(dst_fill, (list, tuple)) else dst_fill
        assert fill.dtype == np.uint8 and fill.Y.shape[0] >= rows and fill.UV.shape[0] >= crows and min(fill.stride, fill.uv_stride) >= cols
        w = fill.copy()
        w.Y[:rows, :cols] = narrow(d.Y[:rows, :cols], sp.depth)
        w.UV[:crows, 0:cols:2] = narrow(d.U[:crows, :cols // 2], sp.depth)
        w.UV[:crows, 1:cols:2] = narrow(d.V[:crows, :cols // 2], sp.depth)
        out.append(w)
    return out
