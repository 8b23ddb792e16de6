"""Expected pictures of vfgs_hip_add_grain_sp_frame_list_dev under an active luma / chroma mix (TEST INFRASTRUCTURE).

The contract (include/vfgs_hip.h) is stated on D(p), the planar low-aligned picture of a semi-planar picture p: the samples written are
those of the planar copy list on D(src) with the same mix active, interleaved again, every written container << sample_shift.  So the
expectation composes what the two features' own tests use and adds no arithmetic of its own:

    semiplanar_util.to_planar               p -> D(p)
    chroma_mix_util.index_frame/expect_from the unchanged oracle on the frame whose chroma planes hold the mix, its grain moved onto the
                                            real chroma (the two steps of chroma_mix_util.expected_frames, per frame, so that a seed can
                                            be set in front of a frame and one oracle can run through several calls)
    interleave, << shift                    written over a copy of the source exactly where the call writes (semiplanar_util.expected)

The samples the derivation leaves out (chroma_mix_util: the oracle's output sits on a clip bound) come back as a mask over the UV plane,
and their number is returned: the tests assert it.
"""
from __future__ import annotations

import numpy as np

import chroma_mix_util as X
import semiplanar_util as SP
import vfgs_testlib as T


def expected(ora, records, frames, seeds, shift, mixes):
    """ora: an oracle programmed with `records` (its seed registers move as the call's do); frames: SPFrames; seeds: None or one per frame;
    mixes: (mix of Cb, mix of Cr), each (luma_mult, chroma_mult, offset) or None.
    -> (list of (expected SPFrame, UV mask of compared containers), number of excluded chroma samples)"""
    legal = X.legal_range(records)
    res, excluded = [], 0
    for i, sp in enumerate(frames):
        assert sp.shift == shift
        d = SP.to_planar(sp)
        if seeds is not None:
            ora.set_seed(seeds[i])
        fi = X.index_frame(d, mixes)
        out = fi.copy()
        ora.add_grain_frame(out)
        want, masks, ex = X.expect_from(d, fi, out, legal)
        excluded += ex
        rows, crows, cols = SP.written_region(sp)
        w = sp.copy()
        w.Y[:rows, :cols] = want.Y[:rows, :cols] << shift
        w.UV[:crows, 0:cols:2] = want.U[:crows, :cols // 2] << shift
        w.UV[:crows, 1:cols:2] = want.V[:crows, :cols // 2] << shift
        m = np.ones(sp.UV.shape, bool)
        m[:crows, 0:cols:2] = masks[0][:crows, :cols // 2]
        m[:crows, 1:cols:2] = masks[1][:crows, :cols // 2]
        res.append((w, m))
    return res, excluded


def mismatches(got: SP.SPFrame, want: SP.SPFrame, uv_mask) -> int:
    return int((got.Y != want.Y).sum()) + int(((got.UV != want.UV) & uv_mask).sum())


def ranged_sp_frames(width, height, depth, suby, shift, nframes, seed, low_bits=True, **ranges):
    """Semi-planar twins of chroma_mix_util.ranged_frames (padding included); with a shift the low bits of every container are random."""
    fr = X.ranged_frames(width, height, depth, 2, suby, nframes, seed, **ranges)
    return [SP.to_semiplanar(f, shift, (seed * 1000 + i) if (shift and low_bits) else None) for i, f in enumerate(fr)]


def saturated_samples(frames, mixes, uv_masks):
    """Chroma samples of the processed area whose mix sits on 2^depth - 1 or on 0 -- where the clamp of the index acts -- and how many of
    them the UV masks of expected() keep in the comparison.  -> (saturated, compared)"""
    sat = compared = 0
    for sp, m in zip(frames, uv_masks):
        d = SP.to_planar(sp)
        fi = X.index_frame(d, mixes)
        rows, crows, cols = SP.written_region(sp)
        for k, p in enumerate((fi.U, fi.V)):
            s = (((p == (1 << sp.depth) - 1) | (p == 0)) & X.processed_area(d, p.shape))[:crows, :cols // 2]
            sat += int(s.sum())
            compared += int((s & m[:crows, k:cols:2]).sum())
    return sat, compared


def chroma_samples(frames) -> int:
    return sum(f.UV.size for f in frames)
