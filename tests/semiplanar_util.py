"""Semi-planar frames for the tests of vfgs_hip_add_grain_sp_frame_list_dev (TEST INFRASTRUCTURE).

A semi-planar picture p is a luma plane plus ONE plane of interleaved Cb/Cr pairs (NV12 / NV16 / P010 / P210 / P012); its planar,
low-aligned picture D(p) has U = the even containers of UV, V = the odd ones, every container >> shift.  The contract of the call
(include/vfgs_hip.h) is stated on D(p), so the expectation here is the unchanged oracle on D(p), interleaved again and shifted back --
written over a copy of the source exactly where the call writes: whole 16-sample blocks of the rows of the picture.  Every other
container of the expectation is the source's, low bits included.
"""
from __future__ import annotations

import numpy as np

import vfgs_testlib as T


class SPFrame:
    """Y: (rows, stride) containers; UV: (chroma rows, uv_stride) containers, Cb0 Cr0 Cb1 Cr1 ...; samples sit `shift` bits up."""

    def __init__(self, width, height, depth, suby, stride, uv_stride, shift, Y, UV):
        self.width, self.height, self.depth, self.suby = width, height, depth, suby
        self.stride, self.uv_stride, self.shift = stride, uv_stride, shift
        self.Y, self.UV = Y, UV
        self.dtype = Y.dtype

    def copy(self):
        return SPFrame(self.width, self.height, self.depth, self.suby, self.stride, self.uv_stride, self.shift, self.Y.copy(), self.UV.copy())

    def equal_all(self, other) -> bool:
        return np.array_equal(self.Y, other.Y) and np.array_equal(self.UV, other.UV)


def to_semiplanar(f: T.Frame, shift=0, low_bits_seed=None) -> SPFrame:
    """The semi-planar twin of a planar frame with csubx == 2: UV row = the U and V rows interleaved (2 x cstride containers), every
    container << shift; low_bits_seed: the low `shift` bits of every container are random instead of zero."""
    assert f.subx == 2
    assert shift == 0 or (f.depth > 8 and shift == 16 - f.depth)
    UV = np.empty((f.U.shape[0], 2 * f.cstride), f.dtype)
    UV[:, 0::2], UV[:, 1::2] = f.U, f.V
    Y = f.Y.copy()
    if shift:
        # (a planar container above the depth's range has no high-aligned twin: only the depth's bits travel)
        Y, UV = (Y << shift).astype(f.dtype), (UV << shift).astype(f.dtype)
        if low_bits_seed is not None:
            rng = np.random.default_rng(low_bits_seed)
            Y |= rng.integers(0, 1 << shift, Y.shape).astype(f.dtype)
            UV |= rng.integers(0, 1 << shift, UV.shape).astype(f.dtype)
    return SPFrame(f.width, f.height, f.depth, f.suby, f.stride, 2 * f.cstride, shift, Y, UV)


def to_planar(sp: SPFrame) -> T.Frame:
    """D(p): U = even containers of UV, V = odd, every container >> shift."""
    f = T.Frame(sp.width, sp.height, sp.depth, 2, sp.suby, sp.stride, sp.uv_stride // 2)
    assert f.Y.shape == sp.Y.shape and f.U.shape[0] == sp.UV.shape[0] and 2 * f.U.shape[1] == sp.UV.shape[1]
    f.Y[...] = sp.Y >> sp.shift
    f.U[...] = sp.UV[:, 0::2] >> sp.shift
    f.V[...] = sp.UV[:, 1::2] >> sp.shift
    return f


def written_region(sp: SPFrame):
    """(luma rows, chroma rows, containers of a row) the call writes: whole blocks of the rows of the picture"""
    return sp.height, (sp.height + sp.suby - 1) // sp.suby, (sp.width + 15) // 16 * 16


def expected(ora, frames, seeds, shift):
    """What the call leaves in the destination of every frame when that destination held the source's bytes: the oracle on D(frame) --
    behind vfgs_set_seed(seeds[f]) where seeds are given -- interleaved, shifted back and written where the call writes."""
    out = []
    for i, sp in enumerate(frames):
        assert sp.shift == shift
        d = to_planar(sp)
        if seeds is not None:
            ora.set_seed(seeds[i])
        ora.add_grain_frame(d)
        rows, crows, cols = written_region(sp)
        w = sp.copy()
        w.Y[:rows, :cols] = d.Y[:rows, :cols] << shift
        w.UV[:crows, 0:cols:2] = d.U[:crows, :cols // 2] << shift
        w.UV[:crows, 1:cols:2] = d.V[:crows, :cols // 2] << shift
        out.append(w)
    return out


def garbage_sp_frame(width, height, depth, suby, shift, seed) -> SPFrame:
    """containers of both planes, padding included, over the full container range"""
    f = T.Frame(width, height, depth, 2, suby)
    rng = np.random.default_rng(seed)
    hi = 1 << (16 if depth > 8 else 8)
    Y = rng.integers(0, hi, f.Y.shape).astype(f.dtype)
    UV = rng.integers(0, hi, (f.U.shape[0], 2 * f.cstride)).astype(f.dtype)
    return SPFrame(width, height, depth, suby, f.stride, 2 * f.cstride, shift, Y, UV)
