"""CPU: the generated programs of tests/model_programs.py -- the oracle pinned to the REAL reference hardware layer for every 8- and
10-bit program, and the generator's own claims.

Reference output is stored as md5 digests under the keys model/<name> of tests/golden/reference_hw_md5.json and handled as in
tests/test_oracle_vs_reference.py: where oracle/_ref/libvfgs_ref.so was built the reference also runs live and must write what the
fixture holds; VFGS_WRITE_REFERENCE_MD5=1 records the fixture there, and only when the oracle agrees.

The reference has no depth 12.  All that pins the oracle at depth 12 is that its line form equals its closed form, and the relation
tests/test_depth12_cpu.py uses: the same program at depth 10 on content >> 2 reads the same intensities, so it draws the same grain.

Generator conditions (conditions on the programs, not tolerances; asserted on the ORACLE's output for the in-range content):
  * at most 10 % of the picture's luma samples end on a clip limit   -- observed over the set: at most 6.2 % (one_y_general_c_10_422)
  * at least 40 % of the luma samples change wherever luma is neither slot 8 nor zero scale  -- observed: at least 46.1 % (m128_unselected_8_422)
"""
import numpy as np
import pytest

import model_programs as MP
import test_oracle_vs_reference as R
import vfgs_testlib as T

W = 200
REFERENCE_NAMES = [n for n in MP.names() if MP.parse(n)[1] in (8, 10)]
NAMES_12 = MP.names(depth=12)


def geometry(name):
    _, depth, fmt, _ = MP.parse(name)
    sx, sy = MP.SUB[fmt]
    return depth, sx, sy, (70 if sy == 1 else 72)


def inputs(name):
    """two frames of 200 x 72 (200 x 70 where csuby == 1) in both content variants"""
    h = geometry(name)[3]
    return [MP.content(name, W, h, 2, v) for v in MP.VARIANTS]


def run(make, rec, sets, **kw):
    """every content variant through a freshly programmed implementation -> all output frames in order"""
    out = []
    for frames in sets:
        hw = make()
        T.replay(hw, rec)
        for f in frames:
            g = f.copy()
            hw.add_grain_frame(g, **kw)
            out.append(g)
    return out


@pytest.mark.parametrize("name", REFERENCE_NAMES)
def test_oracle_equals_reference(name):
    rec, sets = MP.program(name), inputs(name)
    key = f"model/{name}"
    want = R.reference_digests(key, lambda: run(T.ReferenceHW, rec, sets))
    R.check(key, want, run(T.OracleHW, rec, sets))
    R.check(key, want, run(T.OracleHW, rec, sets, closed_form=True))


@pytest.mark.parametrize("name", NAMES_12)
def test_depth_12_line_form_equals_closed_form_and_reads_the_10_bit_twins_intensities(name):
    """No reference exists at depth 12, and this is all that pins the oracle there (see the module docstring): its line form equals
    its closed form on both content variants, and the same program ending at depth 10, on the content >> 2, stores a shift 2 larger,
    reads the same intensity for every sample and moves the seed registers alike."""
    rec = MP.program(name)
    sets = inputs(name)
    a, b = run(T.OracleHW, rec, sets), run(T.OracleHW, rec, sets, closed_form=True)
    assert all(x.equal_all(y) for x, y in zip(a, b))
    rec10 = MP.at_depth(rec, 10)
    s12, s10 = T.StateModel(), T.StateModel()
    T.replay(s12, rec)
    T.replay(s10, rec10)
    assert (s12.bs, s10.bs) == (4, 2) and s12.shift == s10.shift - 2
    assert (s12.slut, s12.plut, s12.rng, s12.seed) == (s10.slut, s10.plut, s10.rng, s10.seed)
    depth, sx, sy, h = geometry(name)
    for frames in sets:
        o12, o10 = T.OracleHW(), T.OracleHW()
        T.replay(o12, rec)
        T.replay(o10, rec10)
        for f12 in frames:
            f10 = T.Frame(W, h, 10, sx, sy)
            for p10, p12 in zip(f10.planes(), f12.planes()):
                p10[...] = p12 >> 2
                assert np.array_equal((p12 >> 4) & 255, (p10 >> 2) & 255)      # the intensity the look-up tables are read with
            o12.add_grain_frame(f12.copy())
            o10.add_grain_frame(f10)
        assert o12.seed_state() == o10.seed_state()


def legal_range_of(rec):
    legal = 0
    for op, a, _b, _p in rec:
        if op == T.OP_LEGAL_RANGE:
            legal = a
    return bool(legal)


# --------------------------------------------------------------------------- the generator's own claims

def state_of(name):
    """the reference's state after the program (T.StateModel), the chroma bank as the FINAL format reads it"""
    st = MP._FullBanks()
    T.replay(st, MP.program(name))
    st.chroma = {k: st.cbank[k, :64 // st.suby, :64 // st.subx] for k in range(8)}
    return st


def slots_of(st, c):
    return sorted({b >> 4 for b in st.plut[c]})


_shares = {}


def shares(name):
    """(share of picture luma samples on a clip limit, share of luma samples changed), oracle, in-range content"""
    if name not in _shares:
        rec = MP.program(name)
        depth, sx, sy, h = geometry(name)
        bs = depth - 8
        lo, hi = (16 << bs, 235 << bs) if legal_range_of(rec) else (0, 255 << bs)
        frames = MP.content(name, W, h, 2, "in_range")
        out = run(T.OracleHW, rec, [frames])
        y0 = np.stack([f.Y[:h, :W] for f in frames])
        y1 = np.stack([f.Y[:h, :W] for f in out])
        assert y0.min() >= 64 << bs and y0.max() < 192 << bs
        _shares[name] = (float(((y1 == lo) | (y1 == hi)).mean()), float((y1 != y0).mean()))
    return _shares[name]


@pytest.mark.parametrize("name", MP.names())
def test_generator_conditions(name):
    st = state_of(name)
    clipped, changed = shares(name)
    print(f"{name}: clipped {clipped:.4f} changed {changed:.4f}")
    assert clipped <= 0.10, "at most 10 % of the luma samples may end on a clip limit: change the generator"
    if slots_of(st, 0) != [8] and any(st.slut[0]):
        assert changed >= 0.40, "at least 40 % of the luma samples must change: change the generator"
    if slots_of(st, 0) == [8] or not any(st.slut[0]):
        assert changed == clipped == 0.0      # (in-range content lies inside both ranges: the clip does nothing)


def test_observed_extremes_are_those_of_the_docstring():
    """the figures the module docstring records, so that they cannot go stale"""
    worst_clip = max(MP.names(), key=lambda n: shares(n)[0])
    moving = [n for n in MP.names() if slots_of(state_of(n), 0) != [8] and any(state_of(n).slut[0])]
    least_change = min(moving, key=lambda n: shares(n)[1])
    print(worst_clip, shares(worst_clip), least_change, shares(least_change))
    assert f"{100 * shares(worst_clip)[0]:.1f} % ({worst_clip}" in __doc__
    assert f"{100 * shares(least_change)[1]:.1f} % ({least_change}" in __doc__


def test_names_cover_every_class_depth_and_format():
    seen = {MP.parse(n)[:3] for n in MP.names()}
    for cls in MP.classes():
        for d in MP.DEPTHS:
            for f in MP.FORMATS:
                want = not (cls == "m128_outside_window" and f == "444") and not (cls == "pk16_split" and d != 8)
                assert ((cls, d, f) in seen) == want, (cls, d, f)
    assert len(set(MP.names())) == len(MP.names())
    assert {MP.parse(n)[3] for n in MP.names("pk16_split")} == {"s2", "s5", "s7", "s2y", "s5y", "s7y"}
    # the same name, the same bytes
    MP._cache.clear()
    a = MP.program("shuffled_2_10_422")
    MP._cache.clear()
    assert a == MP.program("shuffled_2_10_422")


def test_rng_known_answers():
    """splitmix64 from state 0: the published first outputs"""
    r = MP.Rng("")
    r.s = 0
    assert [r.next() for _ in range(2)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    # FNV-1a 64 of "a"
    assert MP.Rng("a").s == 0xaf63dc4c8601ec8c


@pytest.mark.parametrize("depth", MP.DEPTHS)
def test_every_shift_and_every_form_at_every_depth(depth):
    shifts, forms = set(), set()
    for n in MP.names(depth=depth):
        st = state_of(n)
        shifts.add(st.shift - 6 + st.bs)
        forms.add(MP.expected_form(MP.program(n)))
    assert shifts == {2, 3, 4, 5, 6, 7}
    assert forms == {(False, False), (False, True), (True, False), (True, True)}
    gen = {state_of(n).shift - 6 + state_of(n).bs for n in MP.names("general_runs", depth) + MP.names("general_per_intensity", depth)}
    assert gen == {2, 3, 4, 5, 6, 7}


@pytest.mark.parametrize("name", MP.names())
def test_every_class_has_the_property_it_is_named_for(name):
    cls, depth, fmt, variant = MP.parse(name)
    if cls in MP.SHUFFLED_TWINS:
        cls = MP.SHUFFLED_TWINS[cls]
    rec = MP.program(name)
    st = state_of(name)
    sl = [slots_of(st, c) for c in range(3)]
    form = MP.expected_form(rec)
    has128 = lambda bank, k: bool((bank[k] == -128).any())
    assert st.bs == depth - 8 and (st.subx, st.suby) == MP.SUB[fmt]
    assert sorted(st.luma) == sorted(st.chroma) == list(range(8))
    for c in range(3):
        assert len({b & 15 for b in st.plut[c]}) > 8, "garbage low nibbles"
        assert max(s for s in sl[c]) <= 8
    if cls in ("general_runs", "general_per_intensity", "slot8_some", "zero_scale_one_component"):
        assert form == (False, False) and all(len(s) > 1 for s in sl)
    if cls == "general_runs":
        assert any(has128(st.luma, k) for k in range(8)) and any(has128(st.chroma, k) for k in range(8))
        assert set(sum(sl, [])) == set(range(9)) and max(max(st.slut[c]) for c in range(3)) == 255
        for c in range(3):
            runs = np.diff(np.flatnonzero(np.diff([b >> 4 for b in st.plut[c]]) != 0))
            assert runs.max() <= 80 and runs.max() > 1          # (equal neighbours merge: at most two runs of 40)
    if cls == "general_per_intensity":
        for c in range(3):
            v = [b >> 4 for b in st.plut[c]]
            assert all(a != b for a, b in zip(v, v[1:]))
    if cls == "one_y_general_c":
        assert form == (True, False) and len(sl[0]) == 1 and 1 <= sl[0][0] <= 7 and len(sl[1]) > 1 and len(sl[2]) > 1
    if cls == "general_y_one_c":
        assert form == (False, True) and len(sl[0]) > 1 and len(sl[1]) == len(sl[2]) == 1 and 1 <= sl[1][0] <= 7 and 1 <= sl[2][0] <= 7
    if cls == "one_same_slot":
        assert form == (True, True) and sl[0] == sl[1] == sl[2] and 1 <= sl[0][0] <= 7
        assert not any(has128(st.luma, k) or has128(st.chroma, k) for k in range(8))
    if cls == "one_cb_cr_differ":
        assert form == (True, True) and len(sl[0]) == len(sl[1]) == len(sl[2]) == 1 and sl[1] != sl[2]
        assert (st.chroma[sl[1][0]] != st.chroma[sl[2][0]]).mean() > 0.9
    if cls.startswith("slot8_") and cls != "slot8_some":
        assert form == (True, True)
        assert [s == [8] for s in sl] == {"slot8_luma": [True, False, False], "slot8_cb": [False, True, False], "slot8_chroma": [False, True, True]}[cls]
    if cls == "slot8_some":
        for c in range(3):
            assert 8 in sl[c] and sum(b >> 4 == 8 for b in st.plut[c]) >= 20
    if cls == "m128_unselected":
        assert form == (True, True)
        assert all(has128(st.luma, k) for k in range(8) if [k] != sl[0]) and not has128(st.luma, sl[0][0])
        assert all(has128(st.chroma, k) for k in range(8) if k not in (sl[1][0], sl[2][0]))
    if cls == "m128_cr_only":
        assert form == (True, False) and sl[1] != sl[2]
        assert not has128(st.luma, sl[0][0]) and not has128(st.chroma, sl[1][0]) and has128(st.chroma, sl[2][0])
        # without Cr's -128 the form is all one-pattern: the flip is that byte's doing
        cleaned = [(op, a, b, bytes(127 if x == 0x80 else x for x in p) if op == T.OP_CHROMA_PATTERN else p) for op, a, b, p in rec]
        assert MP.expected_form(cleaned) == (True, True)
    if cls == "m128_outside_window":
        assert form == (True, True)
        copied = MP.copied_offsets(fmt)
        for op, a, b, p in rec:
            if op == T.OP_CHROMA_PATTERN and a in (sl[1][0], sl[2][0]):
                at = np.flatnonzero(np.frombuffer(p, np.int8) == -128)
                assert len(at) > 50 and not np.isin(at, copied).any()
        assert not has128(st.chroma, sl[1][0]) and not has128(st.chroma, sl[2][0])
    if cls == "pk16_split":
        shift = int(variant[1])
        limit = MP.fits16_limit(shift)
        assert st.shift == shift + 6 and limit == {2: 257, 5: 249, 7: 225}[shift]
        mx = [max(st.slut[c]) for c in range(3)]
        if variant.endswith("y"):
            assert mx[0] == min(limit + 1, 255) and mx[1] < min(limit, 255) and mx[2] < min(limit, 255)
            assert form == ((limit >= 255), True)
        else:
            assert mx[0] == mx[1] == min(limit, 255) and mx[2] == min(limit + 1, 255)
            assert form == (True, limit >= 255)
        assert all(np.isin(np.abs(st.luma[k]), (126, 127)).mean() > 0.6 for k in range(8))
    if cls == "zero_scale_one_component":
        assert sum(not any(st.slut[c]) for c in range(3)) == 1
    # wide rows: one-pattern forms only where csubx == csuby and chroma is one-pattern
    wide = MP.expected_form(rec, wide=True)
    assert wide == (form if (st.subx == st.suby and form[1]) else (False, False))


def test_zero_scale_rotates_over_the_components():
    zero = {c for n in MP.names("zero_scale_one_component") for c in range(3) if not any(state_of(n).slut[c])}
    assert zero == {0, 1, 2}


@pytest.mark.parametrize("name", [n for n in MP.names() if MP.parse(n)[0] in MP.SHUFFLED_TWINS])
def test_shuffled_program_ends_in_its_twins_state(name):
    """as the reference defines the state (T.StateModel: vfgs_hw.c:314-380), and through a setter sequence that really is another"""
    rec, twin = MP.program(name), MP.program(MP.twin_of(name))
    a, b = T.StateModel(), T.StateModel()
    T.replay(a, rec)
    T.replay(b, twin)
    assert (a.shift, a.bs, a.rng, a.seed, a.subx, a.suby) == (b.shift, b.bs, b.rng, b.seed, b.subx, b.suby)
    assert a.slut == b.slut and a.plut == b.plut
    sx, sy = a.subx, a.suby
    for k in range(8):
        assert np.array_equal(a.luma[k], b.luma[k])
    full_a, full_b = MP._FullBanks(), MP._FullBanks()
    T.replay(full_a, rec)
    T.replay(full_b, twin)
    assert np.array_equal(full_a.cbank[:, :64 // sy, :64 // sx], full_b.cbank[:, :64 // sy, :64 // sx])
    assert MP.expected_form(rec) == MP.expected_form(twin)
    ops = [r[0] for r in rec]
    assert [r[1] for r in rec if r[0] == T.OP_DEPTH] == [8, 10, MP.parse(name)[1]]
    d = [i for i, o in enumerate(ops) if o == T.OP_DEPTH]
    assert any(o == T.OP_SCALE_SHIFT for o in ops[d[0]:d[1]]) and any(o == T.OP_SCALE_SHIFT for o in ops[d[1]:d[2]])
    subs = [i for i, o in enumerate(ops) if o == T.OP_CHROMA_SUBSAMPLING]
    assert len(subs) == 2 and (rec[subs[0]][1], rec[subs[0]][2]) != (sx, sy) and (rec[subs[1]][1], rec[subs[1]][2]) == (sx, sy)
    between = [r[1] for r in rec[subs[0]:subs[1]] if r[0] == T.OP_CHROMA_PATTERN]
    assert len(set(between)) == 4                                        # half the chroma patterns under the other subsampling
    first_pattern = min(i for i, o in enumerate(ops) if o == T.OP_LUMA_PATTERN)
    assert max(i for i, o in enumerate(ops) if o in (T.OP_SCALE_LUT, T.OP_PATTERN_LUT)) < first_pattern      # LUTs before the patterns
    for op in (T.OP_LUMA_PATTERN, T.OP_CHROMA_PATTERN, T.OP_SCALE_LUT, T.OP_PATTERN_LUT):
        calls = {}
        for o, a_, _b, p in rec:
            if o == op:
                calls.setdefault(a_, []).append(p)
        assert all(len(v) == 2 and v[0] != v[1] for v in calls.values()), op
    for op in (T.OP_SCALE_SHIFT, T.OP_LEGAL_RANGE, T.OP_SEED):
        v = [r[1] for r in rec if r[0] == op]
        assert len(v) == 2 and v[0] != v[1]
    assert ops != [r[0] for r in twin]


# --------------------------------------------------------------------------- host state of the product (no GPU needed)

@pytest.mark.parametrize("name", [n for n in MP.names() if MP.parse(n)[0] in MP.SHUFFLED_TWINS])
def test_library_state_after_a_shuffled_program(name):
    """params() and luts(c) of the built library equal the reference's state model for the program and for its unshuffled twin"""
    from versatilefilmgrain_amd import build as B
    if not B.LIB.exists():
        pytest.skip("versatilefilmgrain_amd/libvfgs_hip.so is not built")
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip()
    try:
        for rec in (MP.program(name), MP.program(MP.twin_of(name))):
            st = T.StateModel()
            T.replay(st, rec)
            h.lib.vfgs_hip_reset_state()
            T.replay(h, rec)
            p = h.params()
            assert (p["scale_shift"], p["bs"], p["csubx"], p["csuby"]) == (st.shift, st.bs, st.subx, st.suby)
            assert (p["ymin"], p["ymax"], p["cmin"], p["cmax"]) == st.rng
            for c in range(3):
                assert h.luts(c) == (st.slut[c], st.plut[c])
            assert h.seed_state() == (st.seed,) * 4
    finally:
        h.lib.vfgs_hip_reset_state()
