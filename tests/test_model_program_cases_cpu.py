"""CPU: the case table of tests/model_program_cases.py, checked on the oracle alone -- what tests/test_gpu_model_programs_surfaces.py runs
cannot pass vacuously.

* coverage of the table, as asserts;
* a Cb / Cr mix-up is visible: the expectation of the program with the tables of Cb and Cr exchanged differs from the true one in at least
  25 % of the written UV containers of every in-place case (the slot8_chroma programs leave both components untouched: exactly 0 there);
* the share of the chroma samples the derivation of the mix cases leaves out stays within MIX_CAPS (of the processed chroma samples, the
  stricter of the two denominators in use: semiplanar_mix_util.chroma_samples counts the padding as well);
* where a program leaves ONE chroma component untouched, which one it is, and that the other one moves.

The shares are printed (pytest -s)."""
import numpy as np
import pytest

import chroma_mix_util as X
import model_program_cases as C
import model_programs as MP
import semiplanar_mix_util as M
import semiplanar_util as SP
import vfgs_testlib as T

IN_PLACE, PATHS, MIX = C.in_place_cases(), C.path_cases(), C.mix_cases()
ALL_ONE = ["one_same_slot", "one_cb_cr_differ", "slot8_luma", "slot8_cb", "slot8_chroma", "m128_unselected", "m128_outside_window", "pk16_split",
           "shuffled_1", "shuffled_2"]


def cls_of(c):
    return MP.parse(c.name)[0]


# ---- coverage ----------------------------------------------------------------------------------------------------------------------

def test_the_programs_and_their_forms():
    """114 programs; their forms by depth as the table of the module that generates them has them"""
    assert len(C.PROGRAMS) == 114 == len(set(C.PROGRAMS))
    t, f = True, False
    count = {}
    for n in C.PROGRAMS:
        key = (MP.parse(n)[1], MP.expected_form(MP.program(n)))
        count[key] = count.get(key, 0) + 1
    assert count == {(8, (t, t)): 22, (8, (f, f)): 10, (8, (t, f)): 8, (8, (f, t)): 6,
                     (10, (t, t)): 18, (10, (f, f)): 10, (10, (t, f)): 4, (10, (f, t)): 2,
                     (12, (t, t)): 18, (12, (f, f)): 10, (12, (t, f)): 4, (12, (f, t)): 2}, count


def test_every_program_runs_in_place():
    assert [c.name for c in IN_PLACE] == C.PROGRAMS
    assert all(c.path == "sp" and c.nframes == 2 and c.seeds is None for c in IN_PLACE)
    assert all(c.shift == 0 for c in IN_PLACE if MP.parse(c.name)[1] == 8)
    assert all(c.shift in (0, 16 - MP.parse(c.name)[1]) for c in IN_PLACE)


def test_every_class_meets_both_alignments_and_both_contents_in_place():
    """(pk16_split exists at 8 bit only, where there is one alignment)"""
    for cls in MP.classes():
        mine = [c for c in IN_PLACE if cls_of(c) == cls]
        assert {c.variant for c in mine} == set(MP.VARIANTS), cls
        if cls != "pk16_split":
            assert {bool(c.shift) for c in mine} == {False, True}, cls
            # shift 0 with in-range content, the high alignment with garbage (in 16-bit containers at shift 0 garbage mostly ends on the clip)
            assert {(bool(c.shift), c.variant) for c in mine if MP.parse(c.name)[1] > 8} == {(False, "in_range"), (True, "garbage")}, cls
            assert {c.variant for c in mine if MP.parse(c.name)[1] == 8} == set(MP.VARIANTS), cls
    deep = [c for c in IN_PLACE if MP.parse(c.name)[1] > 8]
    assert {(MP.parse(c.name)[1], MP.parse(c.name)[2], bool(c.shift)) for c in deep} == {(d, f, s) for d in (10, 12) for f in C.FORMATS for s in (False, True)}


def test_every_class_runs_through_every_other_path():
    assert {c.path for c in PATHS} == set(C.PATHS)
    for path in C.PATHS:
        mine = [c for c in PATHS if c.path == path]
        depths = {10, 12} if path in C.NARROWED else set(MP.DEPTHS)
        assert {cls_of(c) for c in mine} >= set(MP.classes()) - {"pk16_split"}, path
        assert ("pk16_split" in {cls_of(c) for c in mine}) == (path not in C.NARROWED)
        assert {(MP.parse(c.name)[1], MP.parse(c.name)[2]) for c in mine if cls_of(c) != "pk16_split"} == {(d, f) for d in depths for f in C.FORMATS}, path
        assert all(c.name in C.PROGRAMS and c.nframes == 3 for c in mine)
        assert all((c.seeds == C.SEEDS) == (path == "sp_seeded") for c in mine)
        assert {c.variant for c in mine} == set(MP.VARIANTS)
        if path != "to_sp8":
            assert {(MP.parse(c.name)[1], bool(c.shift)) for c in mine if MP.parse(c.name)[1] > 8} == {(d, s) for d in (10, 12) for s in (False, True)}, path
        else:
            assert all(c.shift == 0 for c in mine)
        if path != "sp_seeded":
            assert any(c.pad and c.uv_pad and c.pad != c.uv_pad for c in mine) and any(c.pad == c.uv_pad == 0 for c in mine), path
    # every form through every path
    for path in C.PATHS:
        assert {MP.expected_form(MP.program(c.name)) for c in PATHS if c.path == path} == {(a, b) for a in (False, True) for b in (False, True)}, path


def test_garbage_above_the_range_reaches_the_other_calls_at_shift_0():
    """16-bit containers above the depth's range at shift 0 (they behave as in the planar calls: tests/test_gpu_planar_to_sp.py
    test_garbage_sources_at_shift_0) are among the sources of every one of the four calls"""
    for path in C.PATHS:
        hit = [c for c in PATHS if c.path == path and c.variant == "garbage" and c.shift == 0 and MP.parse(c.name)[1] > 8]
        assert hit, path
        for c in hit:
            top = 1 << MP.parse(c.name)[1]
            if path in C.PLANAR_SOURCE:
                assert any(int(f.Y.max()) >= top and int(f.U.max()) >= top and int(f.V.max()) >= top for f in C.planar_frames(c))
            else:
                assert any(int(f.Y.max()) >= top and int(f.UV.max()) >= top for f in C.sp_frames(c))


def test_the_mix_cases():
    names = sorted({c.name for c in MIX})
    assert len(names) == 40 and len(MIX) == 80
    assert names == sorted(n for n in C.PROGRAMS if MP.parse(n)[1] <= 10 and MP.parse(n)[0] in ALL_ONE
                           and (MP.parse(n)[0] != "pk16_split" or MP.parse(n)[3] in ("s2", "s2y")))
    assert {cls_of(c) for c in MIX} == set(ALL_ONE)
    for c in MIX:
        assert MP.expected_form(MP.program(c.name)) == (True, True) and c.variant == "in_range"
        assert c.shift == (6 if MP.parse(c.name)[1] == 10 else 0)
    assert {c.mix for c in MIX} == set(C.MIXES) == set(C.MIX_CAPS)


def test_the_refused_programs_are_general_forms():
    for n in C.REFUSED_UNDER_A_MIX:
        assert n in C.PROGRAMS and MP.expected_form(MP.program(n)) != (True, True), n
    assert {MP.expected_form(MP.program(n)) for n in C.REFUSED_UNDER_A_MIX} == {(False, False), (True, False), (False, True)}


# ---- a Cb / Cr mix-up must be visible ----------------------------------------------------------------------------------------------

def uv_written(frames):
    rows, crows, cols = SP.written_region(frames[0])
    return np.stack([f.UV[:crows, :cols] for f in frames])


@pytest.mark.parametrize("case", IN_PLACE, ids=C.case_id)
def test_a_cb_cr_mix_up_is_visible(case):
    rec = MP.program(case.name)
    frames = C.sp_frames(case)
    true = uv_written(SP.expected(C.oracle_for(rec), frames, None, case.shift))
    mixed_up = uv_written(SP.expected(C.oracle_for(C.cb_cr_exchanged(rec)), frames, None, case.shift))
    share = float((true != mixed_up).mean())
    print(f"{C.case_id(case)}: {share:.4f} of the written UV containers differ with Cb and Cr exchanged")
    if cls_of(case) == "slot8_chroma":
        assert share == 0.0
        # both components untouched: the source's samples, its low bits cleared (a sample outside the range is clipped into it, as in every call)
        src = (uv_written(frames) >> case.shift).astype(np.int64)
        bs = MP.parse(case.name)[1] - 8
        lo, hi = (16 << bs, 240 << bs) if X.legal_range(rec) else (0, 255 << bs)
        if case.variant == "in_range":
            pic = src[..., :frames[0].width]           # (the last block's columns behind the picture hold garbage)
            assert pic.min() >= lo and pic.max() <= hi
        assert np.array_equal(true, (np.clip(src, lo, hi) << case.shift).astype(true.dtype))
    else:
        assert share >= 0.25, "change the case's content variant or seed, not the threshold"


# ---- the derivation under the mix --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", MIX, ids=C.case_id)
def test_derivation_caps_under_the_mix(case):
    rec = MP.program(case.name)
    frames = C.sp_frames(case)
    res, excluded = M.expected(C.oracle_for(rec), rec, frames, None, case.shift, C.MIXES[case.mix])
    rows, crows, cols = SP.written_region(frames[0])
    processed = len(frames) * crows * cols
    assert excluded == sum(int((~m).sum()) for _, m in res)
    share = excluded / processed
    print(f"{C.case_id(case)}: {share:.4f} of the processed chroma samples left out by the derivation ({excluded / M.chroma_samples(frames):.4f} of all)")
    assert share <= C.MIX_CAPS[case.mix], "change the case's content, not the cap"


# ---- one chroma component untouched ------------------------------------------------------------------------------------------------

def untouched_component(name):
    """1 / 2 where the program leaves exactly Cb / Cr as it is, else None"""
    st = T.StateModel()
    T.replay(st, MP.program(name))
    still = [c for c in (1, 2) if {b >> 4 for b in st.plut[c]} == {8} or not any(st.slut[c])]
    return still[0] if len(still) == 1 else None


ONE_STILL = [c for c in IN_PLACE if untouched_component(c.name)]


def test_which_programs_leave_one_chroma_component_untouched():
    want = {n: 1 for n in C.PROGRAMS if MP.parse(n)[0] == "slot8_cb"}
    for n in C.PROGRAMS:
        cls, depth, fmt, _ = MP.parse(n)
        c = (MP.FORMATS.index(fmt) + MP.DEPTHS.index(depth)) % 3
        if cls == "zero_scale_one_component" and c:
            want[n] = c
    assert {c.name: untouched_component(c.name) for c in ONE_STILL} == want and len(want) == 10


@pytest.mark.parametrize("case", ONE_STILL, ids=C.case_id)
def test_the_other_chroma_component_moves(case):
    """in-range content: the untouched component is the source's, the other one changes in at least 40 % of its samples (the generator's own
    condition for luma, tests/test_model_programs_cpu.py)"""
    still = untouched_component(case.name)
    frames = C.sp_frames(case, "in_range")
    want = SP.expected(C.oracle_for(MP.program(case.name)), frames, None, case.shift)
    w, _h = frames[0].width, frames[0].height
    crows = SP.written_region(frames[0])[1]
    src, out = [np.stack([f.UV[:crows, :w] >> case.shift for f in fr]) for fr in (frames, want)]
    changed = [float((src[..., k::2] != out[..., k::2]).mean()) for k in (0, 1)]
    print(f"{C.case_id(case)}: component {still} untouched; changed shares Cb {changed[0]:.4f} Cr {changed[1]:.4f}")
    assert changed[still - 1] == 0.0 and changed[2 - still] >= 0.40, changed
