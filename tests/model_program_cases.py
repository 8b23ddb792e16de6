"""Which generated program goes through which surface call (TEST INFRASTRUCTURE): the case table that tests/test_gpu_model_programs_surfaces.py
runs on the GPU and tests/test_model_program_cases_cpu.py checks on the oracle alone, so that the GPU tests cannot pass vacuously.

Programs: every name of tests/model_programs.py whose format has csubx == 2 (4:2:0 and 4:2:2; the semi-planar calls serve no other) -- 114.
Shapes, the smallest that reach each mechanism (a UV position of the kernels is 2 KiB): 1032 x 40 in 16-bit containers (65 blocks: one whole
position and a ragged one, 2.5 block rows), 2056 x 40 at 8 bit (129 blocks: an odd block count ends the row in half a 32-byte unit).

Sources are MP.content(name, width, 40, n, variant), turned semi-planar with SP.to_semiplanar for the semi-planar calls (with a shift the low
bits of every container are random); the planar-source calls take the MP.content frames themselves.

Paths:
  "sp"         vfgs_hip_add_grain_sp_frame_list_dev in place, one seed sequence: EVERY program, two frames.  Depth 8 runs at shift 0; the
               programs of depth 10 / 12 take shift 0 with in-range content and the high alignment (6 / 4) with garbage in turn (garbage in
               16-bit containers at shift 0 lies mostly above the range, where the clip hides what the tables did: the other paths have such
               sources); depth 8 alternates its content.  The turn moves on from class to class, so that every format meets both.
  "sp_seeded"  the same call with a seed per picture            \
  "sp_copy8"   vfgs_hip_add_grain_sp_frame_list_copy8_dev        | every class at one depth and format each, three frames, in a rotation
  "to_sp"      vfgs_hip_add_grain_frame_list_to_sp_dev           | in the manner of test_gpu_model_programs.path_cases()
  "to_sp8"     vfgs_hip_add_grain_frame_list_to_sp8_dev         /
  "mix"        the in-place call under an active chroma mix: the 40 programs at 8 and 10 bit whose form is all one-pattern, under two
               mixes, depth 10 high-aligned, in-range content, two frames.
"""
from __future__ import annotations

from collections import namedtuple

import model_programs as MP
import semiplanar_util as SP
import vfgs_testlib as T

H = 40
SEEDS = [0, 0xFFFFFFFF, 12345]
PROGRAMS = [n for n in MP.names() if MP.SUB[MP.parse(n)[2]][0] == 2]
FORMATS = ("420", "422")
PATHS = ("sp_seeded", "sp_copy8", "to_sp", "to_sp8")
NARROWED = ("sp_copy8", "to_sp8")                      # 10 / 12 bit only: there is no narrower output of 8 bit
PLANAR_SOURCE = ("to_sp", "to_sp8")
# differ: Cb and Cr get different multipliers, so that a component mix-up shows; cb_only: Cr keeps its own sample as the index
MIXES = {"differ": ((32, 32, 0), (-16, 80, 12)), "cb_only": ((64, 119, -238), None)}
MIX_CAPS = {"differ": 0.10, "cb_only": 0.15}           # share of the chroma samples semiplanar_mix_util.expected may leave out
REFUSED_UNDER_A_MIX = ["general_runs_10_420", "one_y_general_c_8_422", "general_y_one_c_10_422", "m128_cr_only_8_420", "pk16_split_8_420_s7"]

# pad / uv_pad: containers added to the destination's pitches (out-of-place paths)
Case = namedtuple("Case", "path name shift variant nframes seeds pad uv_pad mix")


def case_id(c: Case) -> str:
    return "-".join([c.path, c.name, f"shift{c.shift}", c.variant] + ([c.mix] if c.mix else []))


def width_of(depth: int) -> int:
    return 2056 if depth == 8 else 1032


def in_place_cases() -> list[Case]:
    out = []
    for i, name in enumerate(PROGRAMS):
        cls, depth, _, _ = MP.parse(name)
        k = i + MP.classes().index(cls)
        turn = ((k >> 1) ^ k) & 1 if depth > 8 else k & 1         # (0 1 1 0 over a class's four programs of depth 10 / 12: both formats meet both)
        out.append(Case("sp", name, (16 - depth) if depth > 8 and turn else 0, MP.VARIANTS[turn], 2, None, 0, 0, None))
    return out


def path_cases() -> list[Case]:
    out = []
    for p, path in enumerate(PATHS):
        for i, cls in enumerate(MP.classes()):
            depths = (10, 12) if path in NARROWED else MP.DEPTHS
            if cls == "pk16_split":
                if path in NARROWED:
                    continue
                depths = (8,)
            pick = MP.names(cls, depths[(i + p) % len(depths)], FORMATS[(i // 2 + p) % 2])
            name = pick[(i + p) % len(pick)]
            depth = MP.parse(name)[1]
            high = depth > 8 and path != "to_sp8" and (i // 3 + p) % 2 == 0          # (_to_sp8_dev takes no shift: its source is planar)
            pad, uv_pad = ((16, 48), (0, 0), (32, 16))[(i + p) % 3] if path != "sp_seeded" else (0, 0)
            out.append(Case(path, name, (16 - depth) if high else 0, MP.VARIANTS[(i // 2 + i + p) % 2], 3,
                            SEEDS if path == "sp_seeded" else None, pad, uv_pad, None))
    return out


def mix_cases() -> list[Case]:
    out = []
    for name in PROGRAMS:
        depth = MP.parse(name)[1]
        if depth <= 10 and MP.expected_form(MP.program(name)) == (True, True):
            out += [Case("mix", name, 6 if depth == 10 else 0, "in_range", 2, None, 0, 0, m) for m in MIXES]
    return out


# ---- what a case is made of --------------------------------------------------------------------------------------------------------

def planar_frames(c: Case, variant=None):
    """the MP.content frames of the case (what the planar-source calls take)"""
    depth = MP.parse(c.name)[1]
    return MP.content(c.name, width_of(depth), H, c.nframes, variant or c.variant)


def sp_frames(c: Case, variant=None):
    """... turned semi-planar at the case's alignment; with a shift the low bits of every container are random"""
    return [SP.to_semiplanar(f, c.shift, 7000 + i if c.shift else None) for i, f in enumerate(planar_frames(c, variant))]


def oracle_for(rec):
    ora = T.OracleHW()
    T.replay(ora, rec)
    return ora


def cb_cr_exchanged(rec):
    """the same program with the scale LUT and pattern LUT records of components 1 and 2 exchanged: what a kernel that took Cb's tables for
    Cr, and Cr's for Cb, would compute"""
    return [(op, 3 - a if op in (T.OP_SCALE_LUT, T.OP_PATTERN_LUT) and a in (1, 2) else a, b, p) for op, a, b, p in rec]
