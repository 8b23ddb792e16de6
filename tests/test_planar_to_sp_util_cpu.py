"""CPU: the expectation of the planar-to-semi-planar tests (tests/planar_to_sp_util.py) pinned on hand-made frames -- the interleave order,
truncation under the shift, untouched padding, the narrowing rule in front of the interleave -- and, for the oracle in front of it, against
output the reference itself recorded (tests/golden/frames/fgs_sei_10_420_192x144.npz)."""
import numpy as np
import pytest

import planar_to_sp_util as P2
import semiplanar_util as SP
import vfgs_testlib as T


class Identity:
    """an 'oracle' that adds no grain and records its seeds: what is left is the helper's own work"""

    def __init__(self):
        self.seeds = []

    def set_seed(self, s):
        self.seeds.append(s)

    def add_grain_frame(self, f):
        pass


def hand_made(depth, suby=2, w=144, h=20):
    f = T.Frame(w, h, depth, 2, suby)
    hi = 1 << (16 if depth > 8 else 8)
    # every container its own value, over the full container range (above the depth's range too)
    f.Y[...] = (np.arange(f.Y.size).reshape(f.Y.shape) * 37 + 5) % hi
    f.U[...] = (np.arange(f.U.size).reshape(f.U.shape) * 101 + 1) % hi
    f.V[...] = (np.arange(f.V.size).reshape(f.V.shape) * 211 + 2) % hi
    return f


@pytest.mark.parametrize("depth,shift", [(8, 0), (10, 0), (10, 6), (12, 4)])
def test_interleave_order_truncation_and_padding(depth, shift):
    f = hand_made(depth)
    keep = f.copy()
    fill = P2.dst_frame(f.width, f.height, depth, 2, shift, 9, pad=16, uv_pad=32)
    ora = Identity()
    got = P2.expected(ora, [f, f], [7, 8], shift, fill)[1]
    assert ora.seeds == [7, 8] and f.equal_all(keep)
    rows, crows, cols = f.height, f.height // 2, 144
    mask = (1 << (8 * f.Y.itemsize)) - 1
    assert np.array_equal(got.Y[:rows, :cols], (f.Y[:rows, :cols].astype(np.uint32) << shift) & mask)
    # UV[2 i] = U[i], UV[2 i + 1] = V[i], each << shift and truncated to the container
    for r in (0, crows - 1):
        for i in (0, 1, cols // 2 - 1):
            assert got.UV[r, 2 * i] == (int(f.U[r, i]) << shift) & mask and got.UV[r, 2 * i + 1] == (int(f.V[r, i]) << shift) & mask
    assert np.array_equal(got.UV[:crows, 0:cols:2], (f.U[:crows, :cols // 2].astype(np.uint32) << shift) & mask)
    assert np.array_equal(got.UV[:crows, 1:cols:2], (f.V[:crows, :cols // 2].astype(np.uint32) << shift) & mask)
    if shift:
        assert (int(f.Y.max()) << shift) > mask       # (something WAS truncated)
    # everything outside the written region is the fill's
    assert np.array_equal(got.Y[:, cols:], fill.Y[:, cols:]) and np.array_equal(got.UV[:, cols:], fill.UV[:, cols:])
    assert got.Y.shape == fill.Y.shape and got.UV.shape == fill.UV.shape and fill.stride != fill.uv_stride


@pytest.mark.parametrize("depth", [10, 12])
def test_narrowed_form_narrows_first(depth):
    f = hand_made(depth, suby=1, w=136, h=17)
    f.Y &= (1 << depth) - 1
    f.U &= (1 << depth) - 1
    f.V &= (1 << depth) - 1
    fill = P2.dst_frame(f.width, f.height, 8, 1, 0, 3, pad=32, uv_pad=16)
    got = P2.expected8(Identity(), [f], None, fill)[0]
    bs = depth - 8
    n = lambda a: ((a.astype(np.uint32) + (1 << (bs - 1))) >> bs).astype(np.uint8)
    assert got.dtype == np.uint8
    assert np.array_equal(got.Y[:17, :144], n(f.Y[:17, :144]))
    assert np.array_equal(got.UV[:17, 0:144:2], n(f.U[:17, :72])) and np.array_equal(got.UV[:17, 1:144:2], n(f.V[:17, :72]))
    assert np.array_equal(got.Y[:, 144:], fill.Y[:, 144:]) and np.array_equal(got.UV[:, 144:], fill.UV[:, 144:])


def test_odd_chroma_rows_and_ragged_width():
    """250 x 38 at 4:2:0 is 19 chroma rows of 16 blocks; 250 x 37: the chroma rows round up"""
    for h, crows in ((38, 19), (37, 19)):
        f = hand_made(10, 2, 250, h)
        fill = P2.dst_frame(250, h, 10, 2, 6, 1)
        assert fill.UV.shape == (crows, 256) and fill.Y.shape == (h, 256)
        got = P2.expected(Identity(), [f], None, 6, fill)[0]
        assert np.array_equal(got.UV[:crows, 0:256:2], (f.U[:crows, :128].astype(np.uint32) << 6) & 0xffff)


def test_expectation_equals_the_recorded_reference_output():
    W, H = 192, 144
    with np.load(T.GOLDEN / "frames" / "fgs_sei_10_420_192x144.npz") as z:
        out = z["out"]
    y, u, v = np.split(out, [W * H, W * H + W * H // 4])
    y, u, v = y.reshape(H, W), u.reshape(H // 2, W // 2), v.reshape(H // 2, W // 2)
    frames, _ = T.lcg_frames(W, H, 10, 2, 2, 1)
    ora = T.OracleHW()
    T.replay(ora, T.load_trace("fgs_sei_10_420"))
    fill = P2.dst_frame(W, H, 10, 2, 6, 4, pad=8, uv_pad=24)
    got = P2.expected(ora, frames, None, 6, fill)[0]
    assert np.array_equal(got.Y[:H, :W], y << 6)
    assert np.array_equal(got.UV[:H // 2, 0:W:2], u << 6) and np.array_equal(got.UV[:H // 2, 1:W:2], v << 6)
    assert np.array_equal(got.Y[:, W:], fill.Y[:, W:]) and np.array_equal(got.UV[:, W:], fill.UV[:, W:])
