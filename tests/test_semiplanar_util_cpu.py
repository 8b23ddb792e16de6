"""CPU: the expectation of the semi-planar tests (tests/semiplanar_util.py) pinned against output the reference itself recorded, so that
what the GPU suite compares with is the reference's arithmetic and not a model of this file's own making."""
import numpy as np
import pytest

import semiplanar_util as SP
import vfgs_testlib as T

SUB = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "440": (1, 2)}
FILES = sorted(p.stem for p in (T.GOLDEN / "frames").glob("*.npz"))


def recorded(stem):
    """(trace name, width, height, depth, subx, suby, the reference's first output picture)"""
    name, size = stem.rsplit("_", 1)
    w, h = map(int, size.split("x"))
    sx, sy = SUB[name.split("_")[-1]]
    with np.load(T.GOLDEN / "frames" / f"{stem}.npz") as z:
        return name, w, h, int(name.split("_")[-2]), sx, sy, z["out"]


def oracle(name):
    ora = T.OracleHW()
    T.replay(ora, T.load_trace(name))
    return ora


def test_the_recorded_frames_are_there():
    assert len(FILES) >= 3 and any(s.startswith("fgs_sei_10_420") for s in FILES) and any("_422_" in s for s in FILES)


@pytest.mark.parametrize("stem", [s for s in FILES if "_444_" not in s])      # (4:4:4 has no semi-planar form)
def test_expectation_equals_recorded_reference_output(stem):
    name, w, h, depth, sx, sy, want = recorded(stem)
    frames, _ = T.lcg_frames(w, h, depth, sx, sy, 1)
    sp = SP.to_semiplanar(frames[0], 0)
    assert SP.to_planar(sp).equal_all(frames[0])                       # interleave, de-interleave: the recorded input
    got = SP.to_planar(SP.expected(oracle(name), [sp], None, 0)[0])
    assert np.array_equal(np.frombuffer(got.picture_bytes(), dtype=want.dtype), want)


@pytest.mark.parametrize("stem", [s for s in FILES if "_10_" in s and "_444_" not in s])
def test_high_aligned_samples(stem):
    """shift = 16 - depth: the written containers' low bits are zero, the values are the shift-0 result << shift, the source's low bits
    are ignored and everything that is not written keeps them"""
    name, w, h, depth, sx, sy, _ = recorded(stem)
    shift = 16 - depth
    frames, _ = T.lcg_frames(w, h, depth, sx, sy, 1)
    low = SP.expected(oracle(name), [SP.to_semiplanar(frames[0], 0)], None, 0)[0]
    src = SP.to_semiplanar(frames[0], shift, low_bits_seed=5)
    assert (src.Y & ((1 << shift) - 1)).any() and SP.to_planar(src).equal_all(frames[0])
    high = SP.expected(oracle(name), [src], None, shift)[0]
    rows, crows, cols = SP.written_region(src)
    for got, ref, s, r in ((high.Y, low.Y, src.Y, rows), (high.UV, low.UV, src.UV, crows)):
        assert not (got[:r, :cols] & ((1 << shift) - 1)).any()
        assert np.array_equal(got[:r, :cols], ref[:r, :cols].astype(np.uint32) << shift)
        assert np.array_equal(got[r:], s[r:]) and np.array_equal(got[:, cols:], s[:, cols:])


@pytest.mark.parametrize("w,h,depth,suby", [(1032, 90, 10, 2), (136, 17, 8, 2), (264, 33, 8, 1), (200, 70, 12, 1)])
def test_written_region_is_what_the_oracle_writes(w, h, depth, suby):
    """garbage over the full container range, odd heights: D(expectation) is the oracle's frame, padding included -- the region the helper
    overwrites is exactly the region the oracle changes"""
    name = {10: "fgs_sei_10_420", 8: "fgs_sei_8_420", 12: "fgs_sei_10_420"}[depth] if suby == 2 else {10: "fgs_sei_10_422", 8: "fgs_sei_ff_test6_8_422", 12: "fgs_sei_10_422"}[depth]
    rec = T.load_trace(name)
    if depth == 12:
        rec = [(op, 12 if op == T.OP_DEPTH else a, b, p) for op, a, b, p in rec]
    a, b = T.OracleHW(), T.OracleHW()
    T.replay(a, rec); T.replay(b, rec)
    sp = SP.garbage_sp_frame(w, h, depth, suby, 0, 3)
    d = SP.to_planar(sp)
    a.add_grain_frame(d)
    assert SP.to_planar(SP.expected(b, [sp], None, 0)[0]).equal_all(d)
    assert a.seed_state() == b.seed_state()
