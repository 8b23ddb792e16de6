"""Helpers of the tests of a model per picture with the narrowed 8-bit destination (TEST INFRASTRUCTURE):
vfgs_hip_add_grain_frame_list_models_copy8_dev and vfgs_hip_add_grain_sp_frame_list_models_copy8_dev (include/vfgs_hip.h).

Both contracts are the loop of the calls with models -- program the state models[f] was made from; with seeds vfgs_set_seed(seeds[f]) --
around the one-frame _copy8 list, so the ground truth is composed from the parents' helpers and nothing else:

* planar: model_list_util.expect_seeded / expect_unseeded give the grained 10- or 12-bit frames and the registers, semiplanar_out8_util.narrow
  is yuv_to_8bit, and the result is written over a garbage-filled uint8 destination exactly where the call writes: the whole 16-sample
  blocks of the rows of the picture, per plane.  Every other byte of the expectation is the fill's.
* semi-planar: semiplanar_out8_util.expected8 per frame, by an oracle that holds that frame's model (a seed per picture: one oracle per
  model, reseeded per frame; one sequence: ONE oracle into which the frame's model program is replayed without its seed records).

The case tables of the two GPU files live here as well, so that tests/test_model_out8_cases_cpu.py can run them on the oracle alone."""
from __future__ import annotations

import numpy as np

import model_list_util as U
import semiplanar_out8_util as SP8
import vfgs_testlib as T

W, H = 1032, 90      # 65 blocks x 6 block rows, the last one ragged


class Dst8:
    """a planar destination of bytes: Y (rows, stride), U / V (chroma rows, cstride); pitches = whole blocks + pad bytes (multiples of 16)"""

    def __init__(self, width, height, subx, suby, Y, U, V):
        self.width, self.height, self.subx, self.suby = width, height, subx, suby
        self.Y, self.U, self.V = Y, U, V
        self.stride, self.cstride = Y.shape[1], U.shape[1]

    def planes(self):
        return (self.Y, self.U, self.V)

    def copy(self):
        return Dst8(self.width, self.height, self.subx, self.suby, self.Y.copy(), self.U.copy(), self.V.copy())

    def equal_all(self, other) -> bool:
        return all(np.array_equal(a, b) for a, b in zip(self.planes(), other.planes()))


def dst_frame(width, height, subx, suby, seed, pad=16, cpad=48) -> Dst8:
    """planes of garbage bytes whose pitches exceed the rows and differ between luma and chroma"""
    assert pad % 16 == 0 and cpad % 16 == 0
    nb16 = (width + 15) // 16 * 16
    crows = (height + suby - 1) // suby
    rng = np.random.default_rng(seed)
    mk = lambda r, c: rng.integers(0, 256, (r, c)).astype(np.uint8)
    cpitch = (nb16 // subx + cpad + 15) & ~15      # (a chroma row of an odd number of blocks at 4:2:x is no multiple of 16 bytes; its pitch must be)
    return Dst8(width, height, subx, suby, mk(height, nb16 + pad), mk(crows, cpitch), mk(crows, cpitch))


def written_region(f):
    """(luma rows, chroma rows, luma columns, chroma columns) the planar call writes: whole blocks of the rows of the picture"""
    nb16 = (f.width + 15) // 16 * 16
    return f.height, (f.height + f.suby - 1) // f.suby, nb16, nb16 // f.subx


def narrowed_over(fill: Dst8, grained: T.Frame) -> Dst8:
    rows, crows, cols, ccols = written_region(grained)
    w = fill.copy()
    w.Y[:rows, :cols] = SP8.narrow(grained.Y[:rows, :cols], grained.depth)
    w.U[:crows, :ccols] = SP8.narrow(grained.U[:crows, :ccols], grained.depth)
    w.V[:crows, :ccols] = SP8.narrow(grained.V[:crows, :ccols], grained.depth)
    return w


def expect_planar(recs, pick, frames, seeds, fill, ora=None):
    """-> (expected Dst8 per frame, the four registers afterwards, the oracle of an unseeded run or None)"""
    if seeds is not None:
        want, regs = U.expect_seeded(recs, pick, frames, seeds)
    else:
        ora = ora or U.oracle_programmed(recs[-1])
        want, regs = U.expect_unseeded(ora, recs, pick, frames)
    return [narrowed_over(fill, w) for w in want], regs, ora


def expect_sp(recs, pick, frames, seeds, fill, ora=None):
    """the same for semi-planar frames (semiplanar_util.SPFrame sources, a semiplanar_out8_util.dst_frame fill)"""
    shift = frames[0].shift
    want = []
    if seeds is not None:
        oras = [U.oracle_programmed(r) for r in recs]
        for sp, k, s in zip(frames, pick, seeds):
            want += SP8.expected8(oras[k], [sp], [s], shift, fill)
        return want, oras[pick[-1]].seed_state(), None
    ora = ora or U.oracle_programmed(recs[-1])
    for sp, k in zip(frames, pick):
        T.replay(ora, U.without_seed(recs[k]))
        want += SP8.expected8(ora, [sp], None, shift, fill)
    return want, ora.seed_state(), ora


def garbage_frame(width, height, depth, sx, sy, seed):
    """tests/test_gpu_frame_list.py garbage_frame, for the tests that run without a GPU: every container of every plane, padding included,
    over the full container range"""
    rng = np.random.default_rng(seed)
    f = T.Frame(width, height, depth, sx, sy)
    for p in f.planes():
        p[...] = rng.integers(0, 1 << (16 if depth > 8 else 8), p.shape).astype(f.dtype)
    return f


def fresh_seeds(n, seed):
    return [int(s) for s in np.random.default_rng(seed).integers(0, 1 << 32, n)]


# ---- the case tables of tests/test_gpu_model_list_out8.py and tests/test_gpu_sp_model_list_out8.py ------------------------------------
# name -> (model programs, pick, (width, height), frames' seed); sizes above 2048 samples a row run on the GPU only (the CPU file says so)

PLANAR_CONFIGS = {
    "10_420": ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"],
    "10_420_general": ["fgs_sei_10_420", "default_10_420", "fgs_sei_ff_test6_10_420"],
    "10_422": ["fgs_sei_10_422", "fgs_afgs1_test3_10_422"],
    "10_444": ["fgs_sei_10_444", "fgs_sei_ff_test6_10_444", "fgs_afgs1_test1_10_444"],
    "10_440": ["fgs_sei_10_440", "fgs_sei_ff_test6_10_440"],
    "12_420": ["fgs_sei_10_420@depth12", "fgs_afgs1_test1_10_420@depth12"],
}
SAME_FORM = ["fgs_afgs1_test1_10_420", "fgs_afgs1_test9_10_420", "fgs_afgs1_test2_10_420"]
SAME_FORM_PICK = [0, 1, 2, 1, 0, 2, 2, 1, 0]
FORM_CHANGE = ["fgs_sei_10_420", "fgs_afgs1_test1_10_420"]
FORM_CHANGE_PICK = [0, 0, 1, 1, 1, 0]
NARROW = ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"]
NARROW_PICK = [0, 1, 1, 0, 1, 2, 2]
PAIR = ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"]

PLANAR_CASES = {f"every_format_{c}": (PLANAR_CONFIGS[c], "ABAB", (W, H), 10) for c in PLANAR_CONFIGS}
PLANAR_CASES.update({
    "same_form": (SAME_FORM, SAME_FORM_PICK, (W, H), 30),
    "form_change": (FORM_CHANGE, FORM_CHANGE_PICK, (W, H), 40),
    "34_frames": (PAIR, [i & 1 for i in range(34)], (136, 32), 700),
    "narrow_1920": (NARROW, NARROW_PICK, (1920, 48), 70),
    "narrow_960": (NARROW, NARROW_PICK, (960, 48), 71),
    "two_fronts": (PAIR, [0, 1, 0], (8192, 1366), 50),
    "definition": (PAIR, [0, 1, 1, 0], (520, 70), 90),
    "both_masters": (PAIR, [0, 1, 0], (520, 70), 100),
    "overlap_region": (PAIR, [0, 1, 1, 0, 1, 0, 0], (520, 70), 150),
})

SP_CONFIGS = {
    "p010": (["fgs_sei_10_420", "fgs_sei_ff_test6_10_420", "fgs_afgs1_test1_10_420"], 6, True),        # (programs A, B, C: C of another form; shift; random low bits)
    "p210": (["fgs_sei_10_422", "general_y_one_c_10_422", "fgs_afgs1_test3_10_422"], 6, False),
    "p012": (["fgs_sei_10_420@depth12", "fgs_sei_ff_test6_10_420@depth12", "fgs_afgs1_test1_10_420@depth12"], 4, False),
    "low_aligned": (["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"], 0, False),
}
SP_SIZES = [(1047, 40), (1032, 90)]
SP_PICK = [0, 1, 0, 2, 1]      # A B A C B

SP_CASES = {f"{c}_{w}x{h}": (SP_CONFIGS[c][0], SP_PICK, (w, h), 10) for c in SP_CONFIGS for w, h in SP_SIZES}
SP_CASES.update({
    "34_frames": (PAIR, [i & 1 for i in range(34)], (136, 33), 700),
    "two_fronts": (PAIR, [0, 1, 0], (8192, 1366), 50),
    "definition": (PAIR, [0, 1, 1, 0], (520, 70), 90),
})


def pick_of(pick, nmodels, n=7):
    return [i % nmodels for i in range(n)] if pick == "ABAB" else list(pick)
