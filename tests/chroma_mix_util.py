"""Expected pictures for the luma / chroma mix of the chroma look-up index (include/vfgs_hip.h: vfgs_hip_set_chroma_mix), derived
from the UNCHANGED oracle / reference -- not from the code under test and not from a second restatement of the grain algorithm.

The grain g the hardware layer adds to a chroma sample depends on the sample only through its look-up index (vfgs_hw.c:211-239).
So: F' = the input F with each chroma plane replaced by the mix m (numpy, from the definition), run the oracle on F' with the same
programmed state, take g = out' - m wherever out' is not on a clip bound (there the clip cannot have acted: g is exact), and
expect chroma = clip(C + g, C_min << bs, C_max << bs), luma = the oracle's luma.  Samples whose out' sits on a bound are left out
of the comparison and COUNTED; the tests assert the count (0 for mid-range content).
"""
from __future__ import annotations

import numpy as np

import vfgs_testlib as T

NEUTRAL = (0, 64, 0)
SUPPORTED_TRACES = ("fgs_afgs1_test1_10_420", "fgs_afgs1_test1_8_444", "fgs_afgs1_test1_8_420")
SIX_TRACES = SUPPORTED_TRACES + ("fgs_sei_10_422", "fgs_sei_ff_test6_10_440", "fgs_sei_10_420")


def legal_range(records) -> bool:
    legal = 0
    for op, a, _b, _p in records:
        if op == T.OP_LEGAL_RANGE:
            legal = a
    return bool(legal)


def one_pattern_model(records) -> bool:
    """Every component's pattern LUT selects one slot for every intensity (the AFGS1 models): what the kernels of the mix serve."""
    st = T.StateModel()
    T.replay(st, records)
    return all(len({b >> 4 for b in st.plut[c]}) == 1 for c in range(3))


def mix_plane(Y, Cp, width, depth, subx, suby, mix):
    """m for every sample of chroma plane Cp that has luma above it (the definition, 32-bit arithmetic); mix = (luma_mult, chroma_mult, offset)
    or None (no mix for this component: the sample itself)."""
    if mix is None:
        return Cp.copy()
    lm, cm, off = mix
    bs = depth - 8
    rows = min(Cp.shape[0], (Y.shape[0] + suby - 1) // suby)
    cols = min(Cp.shape[1], Y.shape[1] // subx)
    L = Y[0:rows * suby:suby].astype(np.int64)
    lx0 = np.arange(cols) * subx
    if subx == 2:
        avg = (L[:, lx0] + L[:, np.minimum(lx0 + 1, width - 1)] + 1) >> 1
    else:
        avg = L[:, lx0]
    m = ((avg * lm + Cp[:rows, :cols].astype(np.int64) * cm) >> 6) + off * (1 << bs)
    out = Cp.copy()
    out[:rows, :cols] = np.clip(m, 0, (1 << depth) - 1).astype(Cp.dtype)
    return out


def index_frame(f: T.Frame, mixes) -> T.Frame:
    """F': chroma planes replaced by their mix; mixes = (mix for Cb, mix for Cr)."""
    g = f.copy()
    g.U[...] = mix_plane(f.Y, f.U, f.width, f.depth, f.subx, f.suby, mixes[0])
    g.V[...] = mix_plane(f.Y, f.V, f.width, f.depth, f.subx, f.suby, mixes[1])
    return g


def expect_from(f: T.Frame, fi: T.Frame, out: T.Frame, legal: bool):
    """f: input, fi: index_frame(f), out: what the oracle / reference made of fi.  -> (expected frame, mask frame planes (U, V) of compared
    samples, number of excluded samples)."""
    bs = f.depth - 8
    lo, hi = ((16 << bs), (240 << bs)) if legal else (0, (255 << bs))
    bounds = np.array([0, (1 << f.depth) - 1, 16 << bs, 240 << bs, 255 << bs])      # (255 << bs: the full range's upper limit, below 2^depth - 1 above 8 bit)
    want = f.copy()
    want.Y[...] = out.Y
    masks, excluded = [], 0
    for C, M, O, Wp in ((f.U, fi.U, out.U, want.U), (f.V, fi.V, out.V, want.V)):
        area = processed_area(f, C.shape)
        on_bound = np.isin(O, bounds)
        g = O.astype(np.int64) - M.astype(np.int64)
        val = np.clip(C.astype(np.int64) + g, lo, hi).astype(C.dtype)
        assert np.array_equal(O[~area], M[~area]), "the checker touched samples outside the picture's blocks"
        Wp[...] = np.where(area, val, C)
        ex = area & on_bound
        excluded += int(ex.sum())
        masks.append(~ex)
    return want, masks, excluded


def processed_area(f: T.Frame, shape):
    """Chroma samples the hardware layer processes: rows with a luma line inside the picture, whole 16-sample luma blocks (vfgs_hw.c:301)."""
    rows = (f.height + f.suby - 1) // f.suby
    cols = ((f.width + 15) // 16) * (16 // f.subx)
    a = np.zeros(shape, bool)
    a[:rows, :cols] = True
    return a


def expected_frames(make_checker, records, frames, mixes):
    """frames: inputs processed as consecutive frames.  make_checker() -> a fresh OracleHW / ReferenceHW (programmed here with `records`).
    -> (list of (expected, masks), excluded, checker)."""
    ck = make_checker()
    T.replay(ck, records)
    legal = legal_range(records)
    res, excluded = [], 0
    for f in frames:
        fi = index_frame(f, mixes)
        out = fi.copy()
        ck.add_grain_frame(out)
        want, masks, ex = expect_from(f, fi, out, legal)
        res.append((want, masks))
        excluded += ex
    return res, excluded, ck


def mismatches(got: T.Frame, want: T.Frame, masks) -> int:
    n = int((got.Y != want.Y).sum())
    n += int(((got.U != want.U) & masks[0]).sum())
    n += int(((got.V != want.V) & masks[1]).sum())
    return n


def ranged_frames(width, height, depth, subx, suby, nframes, seed, lo=0.3, hi=0.7, clo=None, chi=None):
    """Frames whose visible AND padded samples are drawn uniformly from [lo, hi) x 2^depth (chroma: [clo, chi) if given)."""
    rng = np.random.default_rng(seed)
    full = 1 << depth
    out = []
    for _ in range(nframes):
        f = T.Frame(width, height, depth, subx, suby)
        f.Y[...] = rng.integers(int(lo * full), int(hi * full), f.Y.shape).astype(f.dtype)
        a, b = (lo if clo is None else clo), (hi if chi is None else chi)
        for p in (f.U, f.V):
            p[...] = rng.integers(int(a * full), int(b * full), p.shape).astype(f.dtype)
        out.append(f)
    return out
