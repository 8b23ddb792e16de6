"""One launch recipe per kernel key (TEST INFRASTRUCTURE): the table that tests/test_gpu_kernel_keys.py runs on the GPU, a case per line of
tests/golden/kernel_keys.txt, and that tests/test_kernel_key_cases_cpu.py checks on the oracle alone, so that the GPU ledger cannot pass vacuously.

A key is a kernel's name as vfgs_layout.h kernel_name() prints it (`grain_rw_kernel<10,2,2,false,false,true,false,true>`); `case_for(name)`
parses it and derives everything by rule -- there is no list of keys here.

Program     f"{cls}_{depth}_{fmt}" of tests/model_programs.py, the class by the key's (oney, onec): CLASS_OF_FORM.  The families whose kernels
            take no form (mix, sp_mix: all one-pattern) get one_same_slot.
Entry       the public call that asks for the family: ENTRY_OF; planar frames with the narrowed destination go through the copy8 call,
            persistent luma workgroups through the contiguous batch call (or the copy8 call, which is one).
Shape       the smallest that reaches the mechanism, as the rest of the suite has them: 328 x 56 x 2 frames (21 blocks, 3.5 block rows);
            8200 x 40 x 1 for rows walked in parts (513 blocks: two parts, the second a single ragged block); 136 x 33 x 1100 in one launch
            for persistent luma workgroups (one luma task a frame: more than a round of the part's workgroup slots; the GPU test asserts that
            the launch record reports persistence); model_program_cases.width_of(depth) x 40 x 2 for the surface kernels (a UV position and a
            ragged one).  Depth 10 / 12 surfaces carry their samples high-aligned (shift 16 - depth; the narrowed destination of a planar
            source has no shift).
Content     MP.content(program, w, h, n, "in_range") for every key -- where the grain is visible --, and a second launch with "garbage" for
            every key that is neither persistent nor under a mix.
Mix         the mix families run under MIX (model_program_cases.MIXES["differ"]) on in-range content; the expectation is
            chroma_mix_util's / semiplanar_mix_util's, which leave out the samples they cannot derive: MIX_CAP bounds their share.
"""
from __future__ import annotations

import re
from collections import namedtuple
from pathlib import Path

import chroma_mix_util as X
import model_program_cases as C
import model_programs as MP
import semiplanar_mix_util as M
import semiplanar_util as SP
import vfgs_testlib as T

FIXTURE = Path(__file__).resolve().parent / "golden" / "kernel_keys.txt"

# template arguments by family, in the order of vfgs_layout.h kernel_name()
ARGS = {"rw": ("depth", "csubx", "csuby", "out8", "oney", "onec", "wide", "persist"),
        "ml": ("depth", "csubx", "csuby", "oney", "onec"),
        "mix": ("depth", "csubx", "csuby", "out8", "wide"),
        "sp": ("depth", "csuby", "oney", "onec"), "spml": ("depth", "csuby", "oney", "onec"), "sp8": ("depth", "csuby", "oney", "onec"),
        "p2sp": ("depth", "csuby", "oney", "onec"), "p2sp8": ("depth", "csuby", "oney", "onec"),
        "sp_mix": ("depth", "csuby")}
SEMIPLANAR = ("sp", "spml", "sp8", "p2sp", "p2sp8", "sp_mix")
MIX_FAMILIES = ("mix", "sp_mix")
CLASS_OF_FORM = {(False, False): "general_runs", (True, False): "one_y_general_c", (False, True): "general_y_one_c", (True, True): "one_same_slot"}
# the entry point that asks for a family (hw.VfgsHip); "rw": RW_ENTRY
ENTRY_OF = {"ml": "add_grain_frame_list_models_dev", "sp": "add_grain_sp_frame_list_dev", "spml": "add_grain_sp_frame_list_models_dev",
            "sp8": "add_grain_sp_frame_list_copy8_dev", "p2sp": "add_grain_frame_list_to_sp_dev", "p2sp8": "add_grain_frame_list_to_sp8_dev",
            "sp_mix": "add_grain_sp_frame_list_dev"}
MIX = C.MIXES["differ"]
MIX_CAP = C.MIX_CAPS["differ"]

NARROW, WIDE, PERSISTENT = (328, 56, 2), (8200, 40, 1), (136, 33, 1100)
SP_H, SP_FRAMES = C.H, 2

# Keys the public entry points cannot reach: key name -> the host-code line that proves it.  The GPU test then asserts that the nearest request
# (the key's own recipe) launches a DIFFERENT existing key.  Empty: every key of the table is reachable.
UNREACHABLE: dict = {}

Key = namedtuple("Key", "family depth csubx csuby out8 oney onec wide persist")
# key: the parsed Key; the rest is the recipe.  variants: the content of each launch of the case; mix: None or MIX
Case = namedtuple("Case", "key program entry width height nframes shift variants mix")


def parse_key(name: str) -> Key:
    m = re.fullmatch(r"grain_(\w+?)_kernel<([\w,]+)>", name)
    assert m and m.group(1) in ARGS, f"not a kernel key: {name}"
    family, vals = m.group(1), m.group(2).split(",")
    assert len(vals) == len(ARGS[family]), name
    got = {}
    for arg, v in zip(ARGS[family], vals):
        if arg in ("depth", "csubx", "csuby"):
            got[arg] = int(v)
        else:
            assert v in ("true", "false"), name
            got[arg] = v == "true"
    # what a family pins (vfgs_layout.h kernel_exists: "a family pins every parameter it does not take")
    if family in SEMIPLANAR:
        got["csubx"] = 2
    if family in MIX_FAMILIES:
        got["oney"] = got["onec"] = True
    got.setdefault("out8", family in ("sp8", "p2sp8"))
    got.setdefault("wide", False)
    got.setdefault("persist", False)
    return Key(family, *(got[f] for f in Key._fields[1:]))


def key_name(k: Key) -> str:
    """the inverse of parse_key: vfgs_layout.h kernel_name()"""
    return T.kernel_name(f"grain_{k.family}_kernel", *(getattr(k, a) for a in ARGS[k.family]))


def format_of(k: Key) -> str:
    return {v: f for f, v in MP.SUB.items()}[k.csubx, k.csuby]


def rw_entry(k: Key) -> str:
    if k.out8:
        return "add_grain_copy8_dev"
    return "add_grain_frames_dev" if k.persist else "add_grain_frame_dev"


def case_for(name: str) -> Case:
    k = parse_key(name)
    program = f"{CLASS_OF_FORM[k.oney, k.onec]}_{k.depth}_{format_of(k)}"
    entry = ENTRY_OF[k.family] if k.family in ENTRY_OF else rw_entry(k)
    if k.family in SEMIPLANAR:
        w, h, n = C.width_of(k.depth), SP_H, SP_FRAMES
    else:
        w, h, n = WIDE if k.wide else PERSISTENT if k.persist else NARROW
    shift = 16 - k.depth if k.family in SEMIPLANAR and k.family != "p2sp8" and k.depth > 8 else 0
    mixed = k.family in MIX_FAMILIES
    variants = ("in_range",) if mixed or k.persist else MP.VARIANTS
    return Case(k, program, entry, w, h, n, shift, variants, MIX if mixed else None)


def recipe(c: Case):
    """what makes two cases different launches (the key itself left out)"""
    return c[1:]


def fixture():
    """-> [(key name, lds bytes)] of tests/golden/kernel_keys.txt, in the file's order"""
    return [(n, int(lds)) for n, lds in (l.split() for l in FIXTURE.read_text().splitlines() if l.strip())]


def blocks(c: Case) -> int:
    return (c.width + 15) // 16


# ---- what a case is made of (oracle side: no GPU) ------------------------------------------------------------------------------------

def planar_frames(c: Case, variant: str):
    """the MP.content frames of one launch of the case: what the planar calls take"""
    return MP.content(c.program, c.width, c.height, c.nframes, variant)


def sp_frames(c: Case, variant: str):
    """... turned semi-planar at the case's alignment; with a shift the low bits of every container are random"""
    return [SP.to_semiplanar(f, c.shift, 7000 + i if c.shift else None) for i, f in enumerate(planar_frames(c, variant))]


def surface_case(c: Case, variant: str, pad=16, uv_pad=48) -> C.Case:
    """a case of the out-of-place surface calls as tests/model_program_cases.py states one (they run through that table's runner); the
    destination's pitches exceed its rows by pad / uv_pad containers"""
    path = {"sp8": "sp_copy8", "p2sp": "to_sp", "p2sp8": "to_sp8"}[c.key.family]
    return C.Case(path, c.program, c.shift, variant, c.nframes, None, pad, uv_pad, None)


def changed_shares(before, after, w, h):
    """per plane, the share of the picture's samples (w x h of luma, the chroma planes' own) that differ between two lists of planar frames"""
    out = []
    for k in range(3):
        n = d = 0
        for a, b in zip(before, after):
            pw, ph = (w, h) if k == 0 else (a.cwidth, a.cheight)
            d += int((a.planes()[k][:ph, :pw] != b.planes()[k][:ph, :pw]).sum())
            n += pw * ph
        out.append(d / n)
    return out


def grained(rec, frames):
    """-> (copies of the planar frames with the oracle's grain, the oracle)"""
    ora = C.oracle_for(rec)
    want = [f.copy() for f in frames]
    for w in want:
        ora.add_grain_frame(w)
    return want, ora


def mix_expectation(c: Case):
    """The expectation of a mix case on its in-range content.
    -> (res, excluded, processed, ora): res as chroma_mix_util.expected_frames (planar) / semiplanar_mix_util.expected (semi-planar) return
    it, the number of chroma samples the derivation leaves out, the number it could have compared, the oracle behind the call"""
    assert c.mix is not None and c.variants == ("in_range",)
    rec = MP.program(c.program)
    if c.key.family == "sp_mix":
        frames = sp_frames(c, "in_range")
        ora = C.oracle_for(rec)
        res, excluded = M.expected(ora, rec, frames, None, c.shift, c.mix)
        _rows, crows, cols = SP.written_region(frames[0])
        return res, excluded, len(frames) * crows * cols, ora
    frames = planar_frames(c, "in_range")
    res, excluded, ora = X.expected_frames(T.OracleHW, rec, frames, c.mix)
    processed = sum(int(X.processed_area(f, p.shape).sum()) for f in frames for p in (f.U, f.V))
    return res, excluded, processed, ora


def mix_effect(c: Case, res) -> float:
    """the share of the compared chroma samples in which the expectation under the mix differs from the oracle's output without one"""
    rec = MP.program(c.program)
    n = d = 0
    if c.key.family == "sp_mix":
        frames = sp_frames(c, "in_range")
        plain = SP.expected(C.oracle_for(rec), frames, None, c.shift)
        _rows, crows, cols = SP.written_region(frames[0])
        for (w, mask), p in zip(res, plain):
            m = mask[:crows, :cols]
            d += int(((w.UV[:crows, :cols] != p.UV[:crows, :cols]) & m).sum())
            n += int(m.sum())
        return d / n
    frames = planar_frames(c, "in_range")
    plain, _ = grained(rec, frames)
    for (w, masks), p, f in zip(res, plain, frames):
        for wp, pp, mask in ((w.U, p.U, masks[0]), (w.V, p.V, masks[1])):
            m = mask & X.processed_area(f, wp.shape)
            d += int(((wp != pp) & m).sum())
            n += int(m.sum())
    return d / n
