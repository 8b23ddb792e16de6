"""The cases of vfgs_hip_add_grain_sp_frame_list_to_planar_dev / _models_to_planar_dev and their expectation (TEST INFRASTRUCTURE; numpy and
the oracle only).

The contract (include/vfgs_hip.h): every written sample is what vfgs_hip_add_grain_sp_frame_list_dev (with models: _models_dev) writes out
of place for the same container of the source, shifted right by sample_shift, U from the even containers of UV and V from the odd ones; only
the whole 16-sample blocks of the picture's rows are written.  So the expectation is the existing helpers' -- semiplanar_util.expected, or
sp_model_list_util.expect_seeded / expect_unseeded with a model per picture -- taken apart with semiplanar_util.to_planar and pasted over
the destination's previous bytes where the call writes.

tests/test_sp_to_planar_cases_cpu.py checks the table on the oracle alone; tests/test_gpu_sp_to_planar.py runs it."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import layout_arena as LA
import model_list_util as U
import semiplanar_util as SP
import sp_model_list_util as SU
import vfgs_testlib as T

NFRAMES = 3
HEIGHTS = (33, 39)        # both odd with a ragged last block row; 39 at 4:2:0 also ends on an odd chroma row
# blocks of a row: the narrowest UV row served; odd (an 8-bit chroma row ends in half a unit); one block past a 16-bit position (mid-position
# at 8 bit); one past a 16-bit ring group and an 8-bit position; one past an 8-bit ring group; the widest row served
BLOCKS = (9, 21, 65, 129, 257, 512)

# program: a trace of tests/golden/traces, "<trace>@depth12", or a generated program of tests/model_programs.py -- those the existing
# semi-planar tests use; models: None, or the programs of the models A, B (one form) and C (another form) of a case with a model per picture
Case = namedtuple("Case", "id program shift blocks height seeded models pad cpad")

# (depth, format) -> program and the sample_shift values served
FORMATS = {
    "nv12": ("fgs_afgs1_test1_8_420", (0,)),
    "nv16": ("fgs_sei_ff_test6_8_422", (0,)),
    "p010": ("fgs_sei_10_420", (6, 0)),
    "p210": ("fgs_sei_10_422", (6, 0)),
    "p012": ("fgs_sei_10_420@depth12", (4,)),
}
# general / one-pattern luma over general / one-pattern chroma
FORMS = ("general_runs_8_420", "fgs_sei_10_420", "one_y_general_c_10_420", "fgs_afgs1_test1_10_420")
# the form (one_y, one_c) of the table image each program of a case without models gets -- the host's choice of form is not this call's, it is
# the one the plain semi-planar call reports for the same program (at 4:2:2 the two recorded programs get a general-form and a one-pattern
# plane each) -- so the kernel a launch must name
FORM_OF = {
    "general_runs_8_420": (0, 0), "fgs_sei_10_420": (0, 1), "one_y_general_c_10_420": (1, 0), "fgs_afgs1_test1_10_420": (1, 1),
    "fgs_afgs1_test1_8_420": (1, 1), "fgs_sei_ff_test6_8_422": (1, 0), "fgs_sei_10_422": (0, 1), "fgs_sei_10_420@depth12": (0, 1),
}
MODEL_SETS = {
    "8_420": ("fgs_afgs1_test1_8_420", "fgs_afgs1_test9_8_420", "fgs_sei_8_420"),
    "10_420": ("fgs_sei_10_420", "fgs_sei_10_420~2", "fgs_afgs1_test1_10_420"),
    "10_422": ("fgs_sei_10_422", "fgs_sei_10_422~2", "fgs_afgs1_test3_10_422"),
    "12_420": ("fgs_sei_10_420@depth12", "fgs_sei_10_420@depth12~2", "fgs_afgs1_test1_10_420@depth12"),
}
MODEL_PICK = (0, 1, 0)          # two models of one form alternate in one launch ...
MODEL_PICK_SPLIT = (0, 1, 2)    # ... a third of another form splits it


def _cases():
    out = []
    # row geometry: every width but the widest in every format, heights and shifts in turn; the widest once per depth
    k = 0
    for fmt, (prog, shifts) in FORMATS.items():
        for b in BLOCKS[:-1]:
            out.append(Case(f"{fmt}-{b}", prog, shifts[k % len(shifts)], b, HEIGHTS[k % 2], k % 3 == 0, None, 0, 0))
            k += 1
    for fmt in ("nv12", "p010", "p012"):
        prog, shifts = FORMATS[fmt]
        out.append(Case(f"{fmt}-512", prog, shifts[0], 512, 33, False, None, 0, 0))
    # all four forms, one seed sequence and a seed per picture; a generous pitch: the padding beyond the whole blocks keeps its bytes
    for i, prog in enumerate(FORMS):
        depth = 8 if "_8_" in prog else 10
        for seeded in (False, True):
            out.append(Case(f"form-{prog}-{'seeded' if seeded else 'sequence'}", prog, 6 if (depth > 8 and not seeded) else 0, 65, HEIGHTS[i % 2], seeded, None, 48, 80))
    # a model per picture
    for i, (name, progs) in enumerate(MODEL_SETS.items()):
        depth = int(name.split("_")[0])
        for seeded in (False, True):
            out.append(Case(f"models-{name}-{'seeded' if seeded else 'sequence'}", progs[0], 16 - depth if (depth > 8 and seeded == (i % 2 == 0)) else 0,
                            (21, 65, 129, 9)[i], HEIGHTS[(i + seeded) % 2], seeded, progs, 16 * seeded, 16))
    return out


CASES = _cases()


def second_model(rec):
    """`rec` with halved scale LUTs, the other range and another scale shift behind it: the same patterns and pattern LUTs, so the same form,
    and another picture (as tests/test_gpu_sp_model_list.py builds its second model)"""
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


def records_of(name):
    """a program by name; "<name>~2": its second model"""
    if name.endswith("~2"):
        return second_model(U.model_records(name[:-2]))
    return U.model_records(name)


def geometry(case):
    depth, sx, sy = T.trace_geometry(records_of(case.program))
    assert sx == 2
    return depth, sy


def seeds_of(case):
    return [int(s) for s in np.random.default_rng(len(case.id)).integers(0, 1 << 32, NFRAMES)] if case.seeded else None


def pick_of(case):
    if case.models is None:
        return None
    return MODEL_PICK_SPLIT if case.seeded else MODEL_PICK


def sources(case):
    """NFRAMES semi-planar pictures: one LCG run through the pictures, garbage over the full container range in the padding, the low bits
    below the shift random"""
    depth, sy = geometry(case)
    planar, _ = T.lcg_frames(16 * case.blocks - 7, case.height, depth, 2, sy, NFRAMES, state=1 + len(case.id), garbage_padding=True)
    return [SP.to_semiplanar(f, case.shift, low_bits_seed=100 + i) for i, f in enumerate(planar)]


class Planes:
    """a planar destination: Y (rows, stride), U and V (chroma rows, cstride) of low-aligned samples; exactly the rows the call addresses"""

    def __init__(self, Y, U, V):
        self.Y, self.U, self.V = Y, U, V
        self.stride, self.cstride = Y.shape[1], U.shape[1]

    def copy(self):
        return Planes(self.Y.copy(), self.U.copy(), self.V.copy())

    def planes(self):
        return (("Y", self.Y), ("U", self.U), ("V", self.V))


def written(sp):
    """(luma rows, chroma rows, luma samples of a row) the call writes"""
    return SP.written_region(sp)


def fill_for(sp, seed, pad=0, cpad=0):
    """a destination pre-filled with garbage: the smallest legal pitches plus pad / cpad samples, the addressed rows"""
    rows, crows, cols = written(sp)
    rng = np.random.default_rng(seed)
    hi = 1 << (16 if sp.depth > 8 else 8)
    mk = lambda r, c: rng.integers(0, hi, (r, c)).astype(sp.dtype)
    # (a pitch is whole 16-byte units: an 8-bit chroma row of an odd number of blocks has 8 pad bytes behind it)
    sz = 2 if sp.depth > 8 else 1
    ccols = LA.min_pitch(cols // 16, sz, 2) // sz
    return Planes(mk(rows, cols + pad), mk(crows, ccols + cpad), mk(crows, ccols + cpad))


def paste(want_sp, fill):
    """the semi-planar call's out-of-place result, taken apart and shifted down, over the destination's previous bytes where the call writes"""
    rows, crows, cols = written(want_sp)
    d = SP.to_planar(want_sp)
    out = fill.copy()
    out.Y[:rows, :cols] = d.Y[:rows, :cols]
    out.U[:crows, :cols // 2] = d.U[:crows, :cols // 2]
    out.V[:crows, :cols // 2] = d.V[:crows, :cols // 2]
    return out


def expected_sp(case, frames, ora=None):
    """-> (what the semi-planar call leaves out of place in a destination that held the source's bytes, per frame; the registers afterwards).
    ora: the oracle whose registers are the library's in front of the call (one seed sequence); programmed here when None"""
    seeds, pick = seeds_of(case), pick_of(case)
    if case.models is None:
        ora = ora or U.oracle_programmed(records_of(case.program))
        want = SP.expected(ora, frames, seeds, case.shift)
        return want, ora.seed_state()
    recs = [records_of(m) for m in case.models]
    if seeds is not None:
        return SU.expect_seeded(recs, pick, frames, seeds, case.shift)
    ora = ora or U.oracle_programmed(recs[-1])
    return SU.expect_unseeded(ora, recs, pick, frames, case.shift)


def expected(case, frames, fills, ora=None):
    """-> ([Planes] the call leaves in destinations that held `fills`, the four seed registers afterwards)"""
    want, regs = expected_sp(case, frames, ora)
    return [paste(w, f) for w, f in zip(want, fills)], regs
