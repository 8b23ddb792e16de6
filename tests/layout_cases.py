"""The layout ledger's table (TEST INFRASTRUCTURE; no GPU): every kernel key and every public entry on the memory a real caller hands over --
one allocation, planes back to back at bases that are 16 but never 256 aligned, the smallest legal pitches, exactly the addressed rows,
random guards around them (tests/layout_arena.py).  tests/test_gpu_layouts.py runs it on the GPU, tests/test_layout_cases_cpu.py checks it
on the oracle alone.

(a) key_cases(): one case per line of tests/golden/kernel_keys.txt, derived from kernel_key_cases.case_for(name): the same program, entry,
    width, frame count, shift and mix; only the layout changes, and the height, which becomes odd (56 -> 55, 40 -> 39, 33 stays): the last
    block row is ragged and at csuby 2 the last chroma row has a single luma row over it.  In-range content, one launch per key.
(b) entry_cases(): one case per public entry that takes picture memory (ENTRIES, and the host pipe), with fgs_sei_10_420 and, where the entry
    accepts depth 8, once more with fgs_sei_ff_test6_8_422, at 328 x 55; three frames wherever the entry takes more than one; SEEDS wherever
    it takes seeds; stripe and part entries on lines [16, 48) and on lines [32, 55), which reach the ragged end -- the arena holds only those
    lines; a captured model of the same program wherever the entry takes models; host-memory entries pinned and pageable.

expected(arena, case) copies rows out of the arena into the objects the existing helpers take (T.Frame, semiplanar_util.SPFrame), lets them
state the result (T.OracleHW, semiplanar_util.expected, planar_to_sp_util, semiplanar_out8_util, chroma_mix_util / semiplanar_mix_util,
model_list_util's loops, `narrowed` / `written`) and copies the destination's addressed rows back: no second statement of the algorithm."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import chroma_mix_util as X
import kernel_key_cases as K
import layout_arena as A
import model_list_util as U
import model_programs as MP
import planar_to_sp_util as P2
import semiplanar_mix_util as M
import semiplanar_out8_util as SP8
import semiplanar_util as SP
import vfgs_testlib as T
from test_gpu_model_programs import narrowed, written

HEIGHTS = {56: 55, 40: 39, 33: 33}
SEEDS = [0, 0xFFFFFFFF, 12345]
PROGRAMS = ("fgs_sei_10_420", "fgs_sei_ff_test6_8_422")
# MP.content names its frames by a generated program: the stand-ins of the two traces (same depth and format)
CONTENT_OF = {"fgs_sei_10_420": "general_runs_10_420", "fgs_sei_ff_test6_8_422": "one_same_slot_8_422"}
W, H, NFRAMES = 328, 55, 3
PARTS = ((16, 32), (32, 23))          # (part_y, part_height): lines [16, 48) and [32, 55)

# id; index: the case's number (rotates the base residues); key: the parsed kernel key, or None; entry: the method of hw.VfgsHip ("host_pipe":
# the pipe); program: what model_list_util.model_records takes; content: the name MP.content takes; src: "planar" / "sp"; dst: None (in
# place), "planar", "planar8", "sp", "sp8"; part: None or (part_y, part_height); stripe: the part is a stripe (lines handed over as
# vfgs_add_grain_line would get them: the registers move for those lines only); seeds: None or a seed per frame; models: the entry takes a
# model per picture; mix: None or the two mixes; contig: the frames follow frame 0 at a frame pitch; mem: "device", "pinned", "pageable"
Case = namedtuple("Case", "id index key entry program content width height nframes src dst shift part stripe seeds models mix contig mem")

# src, dst, parts: runs on PARTS (stripe: as a stripe), whole: also / only on the whole picture, seeded, models, contig, frames, host, depth8
Spec = namedtuple("Spec", "src dst parts stripe whole seeded models contig frames host depth8")


def _s(src="planar", dst=None, parts=False, stripe=False, whole=True, seeded=False, models=False, contig=False, frames=NFRAMES, host=False,
       depth8=True):
    return Spec(src, dst, parts, stripe, whole, seeded, models, contig, frames, host, depth8)


ENTRIES = {
    "add_grain_stripe": _s(parts=True, stripe=True, whole=False, frames=1, host=True),
    "add_grain_stripe_dev": _s(parts=True, stripe=True, whole=False, frames=1),
    "add_grain_frame_dev": _s(frames=1),
    "add_grain_frame_part_dev": _s(parts=True, whole=False, frames=1),
    "add_grain_frames_dev": _s(contig=True),
    "add_grain_frames_part_dev": _s(parts=True, whole=False, contig=True),
    "add_grain_copy_dev": _s(dst="planar", parts=True, contig=True),
    "add_grain_copy8_dev": _s(dst="planar8", parts=True, contig=True, depth8=False),
    "add_grain_frame_list_dev": _s(),
    "add_grain_frame_list_part_dev": _s(parts=True, whole=False),
    "add_grain_frame_list_copy_dev": _s(dst="planar"),
    "add_grain_frame_list_copy8_dev": _s(dst="planar8", depth8=False),
    "add_grain_frame_list_seeded_dev": _s(seeded=True),
    "add_grain_frame_list_seeded_part_dev": _s(parts=True, whole=False, seeded=True),
    "add_grain_frame_list_seeded_copy_dev": _s(dst="planar", seeded=True),
    "add_grain_frame_list_seeded_copy8_dev": _s(dst="planar8", seeded=True, depth8=False),
    "add_grain_sp_frame_list_dev": _s(src="sp", seeded=True),
    "add_grain_sp_frame_list_copy8_dev": _s(src="sp", dst="sp8", seeded=True, depth8=False),
    "add_grain_frame_list_to_sp_dev": _s(dst="sp", seeded=True),
    "add_grain_frame_list_to_sp8_dev": _s(dst="sp8", seeded=True, depth8=False),
    "add_grain_frame_list_models_dev": _s(seeded=True, models=True),
    "add_grain_sp_frame_list_models_dev": _s(src="sp", seeded=True, models=True),
    "add_grain_frame_list_models_copy8_dev": _s(dst="planar8", seeded=True, models=True, depth8=False),
    "add_grain_sp_frame_list_models_copy8_dev": _s(src="sp", dst="sp8", seeded=True, models=True, depth8=False),
    "add_grain_frame_list_models_to_sp_dev": _s(dst="sp", seeded=True, models=True),
    "add_grain_frame_list_models_to_sp8_dev": _s(dst="sp8", seeded=True, models=True, depth8=False),
    "add_grain_frames_host": _s(host=True),
}
# the host pipe (hw.VfgsHip.host_pipe: submit and wait): in place, into a destination of its own, narrowed; a model and a seed per picture
PIPE = {"in_place": _s(seeded=True, models=True, host=True), "destination": _s(dst="planar", seeded=True, models=True, host=True),
        "narrowed": _s(dst="planar8", seeded=True, models=True, host=True, depth8=False)}


def records(c: Case):
    return U.model_records(c.program)


def geometry(c: Case):
    """(depth, csubx, csuby) of the case's program"""
    return T.trace_geometry(records(c))


# ---- the table -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def key_cases():
    out = []
    for index, (name, _lds) in enumerate(K.fixture()):
        kc = K.case_for(name)
        family = kc.key.family
        src = "sp" if family in ("sp", "spml", "sp8", "sp_mix") else "planar"
        dst = {"sp8": "sp8", "p2sp": "sp", "p2sp8": "sp8"}.get(family) or ("planar8" if kc.entry == "add_grain_copy8_dev" else None)
        out.append(Case(name, index, kc.key, kc.entry, kc.program, kc.program, kc.width, HEIGHTS[kc.height], kc.nframes, src, dst, kc.shift,
                        None, False, None, family in ("ml", "spml"), kc.mix, kc.entry in ("add_grain_frames_dev", "add_grain_copy8_dev"),
                        "device"))
    return out


@functools.lru_cache(None)
def entry_cases():
    out = []
    index = len(K.fixture())
    for entry, s in list(ENTRIES.items()) + [(f"host_pipe.{k}", v) for k, v in PIPE.items()]:
        for program in PROGRAMS:
            depth = MP.parse(CONTENT_OF[program])[1]
            if depth == 8 and not s.depth8:
                continue
            shift = 16 - depth if depth > 8 and (s.src == "sp" or s.dst == "sp") else 0
            for part in ((None,) if s.whole else ()) + (PARTS if s.parts else ()):
                for mem in (("pinned", "pageable") if s.host else ("device",)):
                    where = "whole" if part is None else f"lines{part[0]}-{part[0] + part[1]}"
                    out.append(Case(f"{entry}-{program}-{where}-{mem}", index, None, entry.split(".")[0], program, CONTENT_OF[program], W, H,
                                    s.frames, s.src, s.dst, shift, part, s.stripe, SEEDS[:s.frames] if s.seeded else None, s.models, None,
                                    s.contig, mem))
                    index += 1
    return out


def all_cases():
    return key_cases() + entry_cases()


# ---- a case's arena --------------------------------------------------------------------------------------------------------------------

def extent(c: Case):
    """(part_y, luma rows, first chroma row, chroma rows) the call addresses"""
    sy = geometry(c)[2]
    py, ph = c.part or (0, c.height)
    cy0 = py // sy
    return py, ph, cy0, -(-(py + ph) // sy) - cy0


def plane_wants(c: Case, kind):
    """[(role, pitch, rows, rowbytes, sz, row0)] of one picture of the kind: the smallest legal pitches, exactly the addressed rows"""
    depth, sx, _sy = geometry(c)
    nblk = (c.width + 15) // 16
    py, rows, cy0, crows = extent(c)
    sz = 1 if kind in ("planar8", "sp8") or depth == 8 else 2
    luma = ("Y", A.min_pitch(nblk, sz), rows, 16 * nblk * sz, sz, py)
    if kind in ("sp", "sp8"):
        return [luma, ("UV", A.min_pitch(nblk, sz), crows, 16 * nblk * sz, sz, cy0)]
    return [luma] + [(r, A.min_pitch(nblk, sz, sx), crows, 16 * nblk // sx * sz, sz, cy0) for r in "UV"]


def groups_of(c: Case):
    """the planes of the call, grouped as they lie back to back: a contiguous batch's plane of every frame; else every plane alone"""
    groups = []
    for side, kind in ([("io", c.src)] if c.dst is None else [("src", c.src), ("dst", c.dst)]):
        wants = plane_wants(c, kind)
        if c.contig:
            groups += [[A.Want(f"{side}.f{f}.{w[0]}", w[0], side, f, *w[1:]) for f in range(c.nframes)] for w in wants]
        else:
            groups += [[A.Want(f"{side}.f{f}.{w[0]}", w[0], side, f, *w[1:])] for f in range(c.nframes) for w in wants]
    return groups


@functools.lru_cache(4)
def _content(name, width, height, nframes):
    return MP.content(name, width, height, nframes, "in_range")


def sources(c: Case):
    """the pictures of the case as the helpers take them (whole pictures, also for a part): MP.content, SP.to_semiplanar for surfaces"""
    frames = _content(c.content, c.width, c.height, c.nframes)
    if c.src == "sp":
        return [SP.to_semiplanar(f, c.shift, 7000 + i if c.shift else None) for i, f in enumerate(frames)]
    return [f.copy() for f in frames]


def planes_of(obj):
    return (("Y", obj.Y), ("UV", obj.UV)) if isinstance(obj, SP.SPFrame) else (("Y", obj.Y), ("U", obj.U), ("V", obj.V))


def make_arena(c: Case) -> A.Arena:
    """guards, pads and out-of-place destinations random, the sources copied row by row into place"""
    a = A.Arena(groups_of(c), c.index, 100000 + c.index)
    side = "io" if c.dst is None else "src"
    for i, f in enumerate(sources(c)):
        for role, arr in planes_of(f):
            a.put(a.plane(side, i, role), arr)
    return a


# ---- the expectation -------------------------------------------------------------------------------------------------------------------

# buf: the expected arena; compared: None, or False where a byte is left out of the comparison (the mix, inside the region only); regs: the
# four seed registers afterwards; excluded, processed: the chroma samples the derivation of the mix leaves out / could have compared
Expectation = namedtuple("Expectation", "buf compared regs excluded processed")


def _fill(c: Case):
    depth, sx, sy = geometry(c)
    if c.dst == "planar":
        return T.Frame(c.width, c.height, depth, sx, sy)
    if c.dst == "planar8":
        return T.Frame(c.width, c.height, 8, sx, sy)
    if c.dst == "sp":
        return P2.dst_frame(c.width, c.height, depth, sy, c.shift, 0)
    return SP8.dst_frame(c.width, c.height, sy, 0)


def _from_arena(a: A.Arena, side, objs):
    for i, o in enumerate(objs):
        for role, arr in planes_of(o):
            a.get(a.plane(side, i, role), arr)
    return objs


def _lines(ora, f, y0, n):
    """a stripe: vfgs_add_grain_line for its lines, in order"""
    for y in range(y0, y0 + n):
        ora.add_grain_line(f.Y[y].ctypes.data, f.U[y // f.suby].ctypes.data, f.V[y // f.suby].ctypes.data, y, f.width)


def expected(a: A.Arena, c: Case) -> Expectation:
    rec = records(c)
    n = c.nframes
    srcs = _from_arena(a, "io" if c.dst is None else "src", sources(c))
    fills = None if c.dst is None else _from_arena(a, "dst", [_fill(c) for _ in range(n)])
    ora = U.oracle_programmed(rec)
    regs = masks = None
    excluded = processed = 0
    if c.stripe:
        assert c.src == "planar" and c.dst is None and n == 1 and not c.mix
        want = [srcs[0].copy()]
        _lines(ora, want[0], *c.part)
    elif c.mix and c.src == "sp":
        res, excluded = M.expected(ora, rec, srcs, c.seeds, c.shift, c.mix)
        want, masks = [w for w, _ in res], [{"UV": m} for _, m in res]
        _rows, crows, cols = SP.written_region(srcs[0])
        processed = n * crows * cols
    elif c.mix:
        assert c.seeds is None and not c.models
        res, excluded, ora = X.expected_frames(T.OracleHW, rec, srcs, c.mix)
        want, masks = [w for w, _ in res], [{"U": m[0], "V": m[1]} for _, m in res]
        processed = sum(int(X.processed_area(f, p.shape).sum()) for f in srcs for p in (f.U, f.V))
    elif c.src == "sp":
        want = SP.expected(ora, srcs, c.seeds, c.shift) if c.dst is None else SP8.expected8(ora, srcs, c.seeds, c.shift, fills)
    elif c.dst == "sp":
        want = P2.expected(ora, srcs, c.seeds, c.shift, fills)
    elif c.dst == "sp8":
        want = P2.expected8(ora, srcs, c.seeds, fills)
    elif c.models and c.seeds is not None:
        want, regs = U.expect_seeded([rec], [0] * n, srcs, c.seeds)
    elif c.models:
        want, regs = U.expect_unseeded(ora, [rec], [0] * n, srcs)
    else:
        want = [f.copy() for f in srcs]
        for i, w in enumerate(want):
            if c.seeds is not None:
                ora.set_seed(c.seeds[i])
            ora.add_grain_frame(w)
    if c.src == "planar" and c.dst == "planar":
        want = [written(w, f) for w, f in zip(want, fills)]
    elif c.src == "planar" and c.dst == "planar8":
        want = [written(narrowed(w), f) for w, f in zip(want, fills)]
    buf = a.buf.copy()
    side = "io" if c.dst is None else "dst"
    for i, w in enumerate(want):
        for role, arr in planes_of(w):
            a.put(a.plane(side, i, role), arr, buf)
    compared = None
    if masks is not None:
        compared = np.ones(buf.size, bool)
        for i, m in enumerate(masks):
            for role, m2 in m.items():
                a.sample_mask(a.plane(side, i, role), m2, compared)
    return Expectation(buf, compared, regs or ora.seed_state(), excluded, processed)
