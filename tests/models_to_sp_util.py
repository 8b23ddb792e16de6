"""Helpers of the tests of a model per picture from planar pictures onto semi-planar surfaces (TEST INFRASTRUCTURE):
vfgs_hip_add_grain_frame_list_models_to_sp_dev and vfgs_hip_add_grain_frame_list_models_to_sp8_dev (include/vfgs_hip.h).

Both contracts are the loop of the calls with models -- program the state models[f] was made from; with seeds vfgs_set_seed(seeds[f]) --
around the one-frame _to_sp / _to_sp8 call, so the ground truth is composed from the parents' helpers and nothing else:

* model_list_util.expect_seeded / expect_unseeded give the grained planar frames of the planar copy list with a model per frame (a seed
  per picture: one oracle per model, reseeded per frame; one sequence: ONE oracle into which the frame's model program is replayed
  without its seed records) and the registers;
* the narrowed form narrows them as yuv_to_8bit does (planar_to_sp_util.narrowed: the planar _copy8 expectation);
* semiplanar_util.to_semiplanar interleaves Cb and Cr and shifts up, planar_to_sp_util.paste writes the result over a garbage-filled
  destination exactly where the call writes: the whole 16-sample blocks of the rows of the picture.  Every other byte is the fill's.

The case tables of tests/test_gpu_models_to_sp.py live here as well, so that tests/test_models_to_sp_cases_cpu.py can run them on the
oracle alone."""
from __future__ import annotations

import numpy as np

import model_list_util as U
import planar_to_sp_util as P2
import semiplanar_out8_util as SP8
import semiplanar_util as SP
import vfgs_testlib as T

# the three shapes of the GPU file -- none may be larger: 9 blocks and the smallest row served with three block rows, the last of one line; a
# ragged width (66 blocks, 1047 = 65 x 16 + 7) with a partial last block row; 65 blocks x 6 block rows, the last one of 10 lines
SHAPES = [(136, 33), (1047, 40), (1032, 90)]


def fill_for(width, height, depth, suby, shift, out8, seed, pad=16, uv_pad=48):
    """a garbage-filled destination in the call's container whose Y and UV pitches exceed the rows and differ"""
    if out8:
        return SP8.dst_frame(width, height, suby, seed, pad, uv_pad)
    return P2.dst_frame(width, height, depth, suby, shift, seed, pad, uv_pad)


def surface_of(grained: T.Frame, shift, out8, fill):
    return P2.paste(SP.to_semiplanar(P2.narrowed(grained), 0) if out8 else SP.to_semiplanar(grained, shift), fill)


def expect(recs, pick, frames, seeds, shift, out8, fill, ora=None):
    """-> (expected destination per frame, the four registers afterwards, the oracle of an unseeded run or None); frames: planar T.Frame
    sources, fill: one destination for all"""
    if seeds is not None:
        want, regs = U.expect_seeded(recs, pick, frames, seeds)
    else:
        ora = ora or U.oracle_programmed(recs[-1])
        want, regs = U.expect_unseeded(ora, recs, pick, frames)
    return [surface_of(w, shift, out8, fill) for w in want], regs, ora


def garbage_frame(width, height, depth, sy, seed):
    """a planar 4:2:x source: every container of every plane, padding included, over the full container range"""
    rng = np.random.default_rng(seed)
    f = T.Frame(width, height, depth, 2, sy)
    for p in f.planes():
        p[...] = rng.integers(0, 1 << (16 if depth > 8 else 8), p.shape).astype(f.dtype)
    return f


def fresh_seeds(n, seed):
    return [int(s) for s in np.random.default_rng(seed).integers(0, 1 << 32, n)]


def second_model(rec):
    """`rec` with halved scale LUTs, the other range and another scale shift behind it: the same patterns and pattern LUTs, so the same
    form, and a record that differs in lo2 / hi2 and the shift (tests/test_gpu_sp_model_list.py second_model, for the files without a GPU)"""
    slut, shift, legal = {}, None, 0
    for op, a, b, p in rec:
        if op == T.OP_SCALE_LUT:
            slut[a] = bytes(p)
        elif op == T.OP_SCALE_SHIFT:
            shift = a
        elif op == T.OP_LEGAL_RANGE:
            legal = a
    assert len(slut) == 3 and shift is not None
    more = [(T.OP_SCALE_LUT, c, 0, bytes(v >> 1 for v in slut[c])) for c in range(3)]
    more += [(T.OP_LEGAL_RANGE, 0 if legal else 1, 0, b""), (T.OP_SCALE_SHIFT, shift + 1 if shift < 7 else shift - 1, 0, b"")]
    return list(rec) + more


def records(programs):
    return [U.model_records(p) if isinstance(p, str) else list(p) for p in programs]


# ---- the case tables of tests/test_gpu_models_to_sp.py ------------------------------------------------------------------------------------
# surface -> (programs A, B, C with C of another form than A; sample_shift; narrowed)

SURFACES = {
    "p010": (["fgs_sei_10_420", "fgs_sei_ff_test6_10_420", "fgs_afgs1_test1_10_420"], 6, False),
    "p210": (["fgs_sei_10_422", "general_y_one_c_10_422", "fgs_afgs1_test3_10_422"], 6, False),
    "p012": (["fgs_sei_10_420@depth12", "fgs_sei_ff_test6_10_420@depth12", "fgs_afgs1_test1_10_420@depth12"], 4, False),
    "low_aligned": (["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"], 0, False),
    "nv12": (["fgs_sei_8_420", "fgs_sei_ff_test6_8_420", "fgs_afgs1_test1_8_420"], 0, False),
    "nv16": (["fgs_sei_8_422", "general_y_one_c_8_422", "fgs_sei_ff_test6_8_422"], 0, False),
    "10_to_nv12": (["fgs_sei_10_420", "fgs_sei_ff_test6_10_420", "fgs_afgs1_test1_10_420"], 0, True),
    "10_to_nv16": (["fgs_sei_10_422", "general_y_one_c_10_422", "fgs_afgs1_test3_10_422"], 0, True),
    "12_to_nv12": (["fgs_sei_10_420@depth12", "fgs_sei_ff_test6_10_420@depth12", "fgs_afgs1_test1_10_420@depth12"], 0, True),
    "12_to_nv16": (["general_runs_12_422", "general_y_one_c_12_422", "one_same_slot_12_422"], 0, True),
}
SURFACE_SIZES = SHAPES[1:]
PICK = [0, 1, 0, 2, 1]      # A B A C B
PAIR = ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"]
BOUNDS_PICK = [1, 0, 0, 1, 0, 1, 1]      # B A A B A B B

# name -> (programs, pick, (width, height), sample_shift, narrowed, frames' seed); "bounds_*": the second program is second_model(first)
CASES = {f"{s}_{w}x{h}": (SURFACES[s][0], PICK, (w, h), SURFACES[s][1], SURFACES[s][2], 10) for s in SURFACES for w, h in SURFACE_SIZES}
CASES.update({
    "bounds_p010": (["fgs_afgs1_test1_10_420"], BOUNDS_PICK, (1032, 90), 6, False, 30),
    "bounds_nv12": (["fgs_afgs1_test1_10_420"], BOUNDS_PICK, (1032, 90), 0, True, 31),
    "34_frames_p010": (PAIR, [i & 1 for i in range(34)], (136, 33), 6, False, 700),
    "34_frames_nv12": (PAIR, [i & 1 for i in range(34)], (136, 33), 0, True, 701),
    "definition_p010": (PAIR, [0, 1, 1, 0], (136, 33), 6, False, 90),
    "definition_nv12": (PAIR, [0, 1, 1, 0], (136, 33), 0, True, 91),
    "overlap_region": (PAIR, [0, 1, 1, 0, 1, 0, 0], (136, 33), 6, False, 150),
})


def case_records(case):
    names = CASES[case][0]
    recs = records(names)
    if case.startswith("bounds_"):
        recs.append(second_model(recs[0]))
    return recs
