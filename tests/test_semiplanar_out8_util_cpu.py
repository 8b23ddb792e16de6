"""CPU: the expectation of the narrowed semi-planar tests (tests/semiplanar_out8_util.py) pinned against output the reference itself
recorded (tests/golden/frames/fgs_sei_10_420_192x144.npz), so that what the GPU suite compares with is the reference's arithmetic: the
helper on the recorded source equals the recorded output picture narrowed as yuv_to_8bit does and interleaved; and the helper touches the
destination's fill exactly where the call writes."""
import numpy as np
import pytest

import semiplanar_out8_util as SP8
import semiplanar_util as SP
import vfgs_testlib as T

STEM, NAME, W, H, DEPTH = "fgs_sei_10_420_192x144", "fgs_sei_10_420", 192, 144, 10


def oracle(name, depth=None):
    rec = T.load_trace(name)
    if depth:
        rec = [(op, depth if op == T.OP_DEPTH else a, b, p) for op, a, b, p in rec]
    ora = T.OracleHW()
    T.replay(ora, rec)
    return ora


@pytest.fixture(scope="module")
def recorded_out():
    with np.load(T.GOLDEN / "frames" / f"{STEM}.npz") as z:
        out = z["out"]
    assert out.dtype == np.uint16 and out.size == W * H * 3 // 2
    y, u, v = np.split(out, [W * H, W * H + W * H // 4])
    return y.reshape(H, W), u.reshape(H // 2, W // 2), v.reshape(H // 2, W // 2)


@pytest.mark.parametrize("shift", [0, 6])
def test_expectation_equals_the_narrowed_interleaved_recorded_output(recorded_out, shift):
    y, u, v = recorded_out
    frames, _ = T.lcg_frames(W, H, DEPTH, 2, 2, 1)
    src = SP.to_semiplanar(frames[0], shift, low_bits_seed=3 if shift else None)
    fill = SP8.dst_frame(W, H, 2, 11, pad=16, uv_pad=32)
    got = SP8.expected8(oracle(NAME), [src], None, shift, fill)[0]
    # the recorded reference output, narrowed by the rule itself (yuv.c:216-258 at 10 bit) and interleaved
    assert np.array_equal(got.Y[:H, :W], ((y.astype(np.uint32) + 2) >> 2).astype(np.uint8))
    assert np.array_equal(got.UV[:H // 2, 0:W:2], ((u.astype(np.uint32) + 2) >> 2).astype(np.uint8))
    assert np.array_equal(got.UV[:H // 2, 1:W:2], ((v.astype(np.uint32) + 2) >> 2).astype(np.uint8))
    # ... and everything else is the fill's
    assert np.array_equal(got.Y[:, W:], fill.Y[:, W:]) and np.array_equal(got.UV[:, W:], fill.UV[:, W:])


def test_rounding_rule():
    assert SP8.narrow(np.array([0, 1, 2, 5, 6, 1019, 1020, 1021, 1022, 1023], np.uint16), 10).tolist() == [0, 0, 1, 1, 2, 255, 255, 255, 0, 0]
    assert SP8.narrow(np.array([0, 7, 8, 23, 24, 4087, 4088], np.uint16), 12).tolist() == [0, 0, 1, 1, 2, 255, 0]


@pytest.mark.parametrize("w,h,depth,suby,shift", [(1032, 90, 10, 2, 6), (136, 17, 10, 1, 0), (200, 70, 12, 1, 4), (264, 33, 12, 2, 0)])
def test_written_region(w, h, depth, suby, shift):
    """garbage sources over the full container range, odd heights: inside the written region the bytes are the oracle's frame on D(p),
    narrowed; outside it the fill is untouched; the registers are the oracle's; the source is not changed"""
    name = "fgs_sei_10_420" if suby == 2 else "fgs_sei_10_422"
    a, b = oracle(name, depth), oracle(name, depth)
    src = SP.garbage_sp_frame(w, h, depth, suby, shift, 3)
    keep = src.copy()
    d = SP.to_planar(src)
    a.add_grain_frame(d)
    fill = SP8.dst_frame(w, h, suby, 5, pad=32, uv_pad=16)
    got = SP8.expected8(b, [src], None, shift, fill)[0]
    assert a.seed_state() == b.seed_state() and src.equal_all(keep)
    rows, crows, cols = SP.written_region(src)
    assert np.array_equal(got.Y[:rows, :cols], SP8.narrow(d.Y[:rows, :cols], depth))
    assert np.array_equal(got.UV[:crows, 0:cols:2], SP8.narrow(d.U[:crows, :cols // 2], depth))
    assert np.array_equal(got.UV[:crows, 1:cols:2], SP8.narrow(d.V[:crows, :cols // 2], depth))
    mask_y, mask_uv = np.ones_like(got.Y, bool), np.ones_like(got.UV, bool)
    mask_y[:rows, :cols] = False
    mask_uv[:crows, :cols] = False
    assert np.array_equal(got.Y[mask_y], fill.Y[mask_y]) and np.array_equal(got.UV[mask_uv], fill.UV[mask_uv])
    assert fill.stride != fill.uv_stride and mask_y.any() and mask_uv.any()
