"""CPU: the recipe table of tests/kernel_key_cases.py against tests/golden/kernel_keys.txt, on the oracle alone -- what
tests/test_gpu_kernel_keys.py runs cannot pass vacuously.

* the cases cover the fixture exactly: 326 keys, a case each, no two keys with the same recipe, the key's name recovered from the case;
* every case's program has the key's depth, format and -- by MP.expected_form, with `wide` for rows walked in parts -- the key's
  (oney, onec); wide shapes have more than 512 blocks, the others at most 512;
* the grain is visible: on the in-range content of every distinct (program, shape) the oracle changes at least a quarter of the picture's
  samples in every plane;
* under the mix, the share of the chroma samples the derivation leaves out stays within the cap the project has for this mix
  (model_program_cases.MIX_CAPS), and the mix matters: the expectation differs from the oracle's output without a mix in at least a quarter
  of the compared chroma samples.

The shares are printed (pytest -s)."""
import pytest

import kernel_key_cases as K
import model_programs as MP
import vfgs_testlib as T

FIXTURE = K.fixture()
NAMES = [n for n, _ in FIXTURE]
CASES = [K.case_for(n) for n in NAMES]
MIXED = [c for c in CASES if c.mix]
# (a program grains a shape the same way whichever key it is launched for: each pair once, in the table's order)
SHAPES = list(dict.fromkeys((c.program, c.width, c.height, c.nframes) for c in CASES))
id_of = lambda c: K.key_name(c.key)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------

def test_the_fixture_is_the_table_of_DESIGN_4_10():
    assert len(NAMES) == 326 == len(set(NAMES))
    assert [sum(1 for n in NAMES if K.parse_key(n).depth == d) for d in (8, 10, 12)] == [72, 134, 120]
    assert all(lds > 0 for _, lds in FIXTURE)


def test_the_cases_cover_the_fixture_exactly():
    """no key without a case, no case without its key, no two keys with one recipe"""
    assert [K.key_name(c.key) for c in CASES] == NAMES
    assert len({K.recipe(c) for c in CASES}) == len(set(CASES)) == len(NAMES)
    assert not K.UNREACHABLE.keys() - set(NAMES)
    for c in CASES:
        assert c.variants[0] == "in_range" and set(c.variants) <= set(MP.VARIANTS)
        assert (len(c.variants) == 2) == (not c.key.persist and c.mix is None), id_of(c)
        assert (c.mix == K.MIX) == (c.key.family in K.MIX_FAMILIES) and (c.mix is None) == (c.key.family not in K.MIX_FAMILIES)


def test_every_family_has_its_entry_point():
    by_family = {}
    for c in CASES:
        by_family.setdefault(c.key.family, set()).add(c.entry)
    assert by_family == {"rw": {"add_grain_frame_dev", "add_grain_frames_dev", "add_grain_copy8_dev"},
                         "mix": {"add_grain_frame_dev", "add_grain_copy8_dev"},
                         "ml": {"add_grain_frame_list_models_dev"}, "sp": {"add_grain_sp_frame_list_dev"},
                         "spml": {"add_grain_sp_frame_list_models_dev"}, "sp8": {"add_grain_sp_frame_list_copy8_dev"},
                         "p2sp": {"add_grain_frame_list_to_sp_dev"}, "p2sp8": {"add_grain_frame_list_to_sp8_dev"},
                         "sp_mix": {"add_grain_sp_frame_list_dev"}}
    for c in CASES:
        if c.key.family in ("rw", "mix"):
            assert (c.entry == "add_grain_copy8_dev") == c.key.out8, id_of(c)
            assert (c.entry == "add_grain_frames_dev") == (c.key.persist and not c.key.out8), id_of(c)


@pytest.mark.parametrize("case", CASES, ids=id_of)
def test_the_program_and_the_shape_are_the_keys(case):
    k = case.key
    rec = MP.program(case.program)
    assert case.program in MP.names()
    assert T.trace_geometry(rec) == (k.depth, k.csubx, k.csuby)
    assert MP.expected_form(rec, k.wide) == (k.oney, k.onec), (case.program, MP.expected_form(rec, k.wide))
    assert (K.blocks(case) > 512) == k.wide and case.width > 128
    assert (case.nframes == 1100) == k.persist
    semiplanar = k.family in K.SEMIPLANAR
    assert (case.shift == 16 - k.depth) if (semiplanar and k.depth > 8 and k.family != "p2sp8") else case.shift == 0
    if semiplanar:
        assert (case.width, case.height) == (2056 if k.depth == 8 else 1032, 40)
    else:
        assert (case.width, case.height) == ((8200, 40) if k.wide else (136, 33) if k.persist else (328, 56))


@pytest.mark.parametrize("case", [c for c in CASES if c.key.family in ("sp8", "p2sp", "p2sp8")], ids=id_of)
def test_the_out_of_place_surface_cases_are_the_other_tables(case):
    """they run through the runner of tests/model_program_cases.py: the same sources, at the same alignment, from both tables"""
    import model_program_cases as C
    for variant in case.variants:
        sc = K.surface_case(case, variant)
        assert sc.path == {"sp8": "sp_copy8", "p2sp": "to_sp", "p2sp8": "to_sp8"}[case.key.family] and (sc.path in C.NARROWED) == case.key.out8
        assert (sc.name, sc.shift, sc.nframes, sc.seeds, sc.mix) == (case.program, case.shift, case.nframes, None, None) and sc.pad != sc.uv_pad
        if sc.path in C.PLANAR_SOURCE:
            assert all(a.equal_all(b) for a, b in zip(C.planar_frames(sc), K.planar_frames(case, variant)))
        else:
            assert all(a.equal_all(b) and a.shift == case.shift for a, b in zip(C.sp_frames(sc), K.sp_frames(case, variant)))


# ---- the grain is visible ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("program, w, h, n", SHAPES, ids=lambda v: str(v))
def test_the_grain_is_visible(program, w, h, n):
    frames = MP.content(program, w, h, n, "in_range")
    want, _ = K.grained(MP.program(program), frames)
    shares = K.changed_shares(frames, want, w, h)
    print(f"{program} {w}x{h}x{n}: changed shares Y {shares[0]:.4f} Cb {shares[1]:.4f} Cr {shares[2]:.4f}")
    assert min(shares) >= 0.25, "change the case's content or seed, not the threshold"


# ---- under the mix -----------------------------------------------------------------------------------------------------------------

def test_the_mix_cases_span_what_the_mix_serves():
    """all 8- and 10-bit formats at the planar shape, 4:2:0 and 4:4:4 at the wide one, the surface shapes"""
    planar = {(c.key.depth, K.format_of(c.key), c.key.wide, c.key.out8) for c in MIXED if c.key.family == "mix"}
    assert planar == ({(d, f, False, False) for d in (8, 10) for f in MP.FORMATS} | {(10, f, False, True) for f in MP.FORMATS}
                      | {(d, f, True, False) for d in (8, 10) for f in ("420", "444")} | {(10, f, True, True) for f in ("420", "444")})
    assert {(c.key.depth, K.format_of(c.key)) for c in MIXED if c.key.family == "sp_mix"} == {(d, f) for d in (8, 10) for f in ("420", "422")}


@pytest.mark.parametrize("case", MIXED, ids=id_of)
def test_the_derivation_under_the_mix(case):
    res, excluded, processed, _ = K.mix_expectation(case)
    left_out = excluded / processed
    effect = K.mix_effect(case, res)
    print(f"{id_of(case)}: {left_out:.4f} of the processed chroma samples left out; the mix changes {effect:.4f} of the compared ones")
    assert left_out <= K.MIX_CAP == 0.10, "change the case's content, not the cap"
    assert effect >= 0.25, "change the case's content, not the threshold"
