"""CPU: the layout ledger's table (tests/layout_cases.py) and its memory (tests/layout_arena.py) on the oracle alone -- what
tests/test_gpu_layouts.py runs cannot pass vacuously.

* coverage: part (a) covers tests/golden/kernel_keys.txt exactly, its recipes the key ledger's apart from height and layout; part (b) names
  every method of hw.VfgsHip that takes picture memory, found by introspection (a new entry without a case fails here), and what a case
  passes -- parts, seeds, models, the 8-bit program -- follows from the method's signature and name;
* layouts: every base 16-aligned and none 0 mod 256; every plane role of every family meets a base of 16 mod 32; every pitch the smallest
  legal one and every plane exactly the addressed rows; the 8 pad bytes of 8-bit subsampled chroma in rw, ml, p2sp and mix; guards in front
  of, between and behind the planes, sized by the ring groups of vfgs_layout.h; the arena is guards and planes and nothing else;
* the oracle stays inside the region: for every distinct (program, shape) expected() leaves every byte outside region_mask() unchanged, and
  for the planar in-place shapes the oracle run DIRECTLY on the arena -- tight pitches, exact rows, odd heights -- gives expected()'s bytes;
* the grain is visible: at least a quarter of the region's containers change, per plane role;
* under the mix the left-out share stays within kernel_key_cases.MIX_CAP at the new heights, and the mix matters;
* the comparison sees what it is for: five single-byte mutations of an expected arena fail, and the message says where.

The shares are printed (pytest -s)."""
import inspect

import numpy as np
import pytest

import kernel_key_cases as K
import layout_arena as A
import layout_cases as L
import model_list_util as U
import vfgs_testlib as T

KEYS, ENTRY_CASES = L.key_cases(), L.entry_cases()
CASES = KEYS + ENTRY_CASES
ident = lambda c: c.id


def shape_of(c):
    """what decides the bytes of a case's arena and expectation (the entry and the memory's kind do not)"""
    return (c.program, c.width, c.height, c.nframes, c.src, c.dst, c.shift, c.part, c.stripe, c.seeds is not None, c.mix, c.contig, c.models)


SHAPES = list({shape_of(c): c for c in CASES}.values())
family_of = lambda c: c.key.family if c.key else f"{c.src}->{c.dst or 'in place'}"


def bare_arena(c):
    """the case's layout without its sources (the properties below are the layout's)"""
    return A.Arena(L.groups_of(c), c.index, 1)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------

def test_part_a_covers_the_fixture_with_the_key_ledgers_recipes():
    names = [n for n, _ in K.fixture()]
    assert [c.id for c in KEYS] == names and len(names) == 326
    for c in KEYS:
        kc = K.case_for(c.id)
        assert (c.key, c.program, c.entry, c.width, c.nframes, c.shift, c.mix) == (kc.key, kc.program, kc.entry, kc.width, kc.nframes, kc.shift, kc.mix)
        assert c.height == {56: 55, 40: 39, 33: 33}[kc.height] and c.height % 2 == 1
        assert c.content == c.program and c.part is None and c.seeds is None and c.mem == "device"
        assert K.blocks(kc) % 2 == 1 and K.blocks(kc) in (21, 513, 9, 65, 129)
    assert len({c.index for c in CASES}) == len(CASES)


def qualifying_methods():
    from versatilefilmgrain_amd import hw
    names = [n for n, v in vars(hw.VfgsHip).items() if n.startswith("add_grain_") and callable(v)]
    first, last = names.index("add_grain_stripe"), names.index("add_grain_frame_list_models_to_sp8_dev")
    return {n: inspect.signature(getattr(hw.VfgsHip, n)).parameters for n in names[first:last + 1] + ["add_grain_frames_host"]}


def test_part_b_names_every_entry_that_takes_picture_memory():
    methods = qualifying_methods()
    assert set(methods) == set(L.ENTRIES) and len(methods) == 27
    assert "add_grain_line" not in methods          # (one line of host memory: the drop-in call has no layout to vary)
    for name, params in methods.items():
        s = L.ENTRIES[name]
        cases = [c for c in ENTRY_CASES if c.entry == name]
        assert s.parts == ("part_y" in params or "stripe" in name) and s.stripe == ("stripe" in name), name
        assert s.seeded == ("seeds" in params) and s.models == ("models" in params), name
        assert s.depth8 == ("copy8" not in name and "sp8" not in name), name
        assert s.src == ("sp" if "_sp_frame" in name else "planar"), name
        assert s.host == (not name.endswith("_dev")), name
        assert {c.program for c in cases} == set(L.PROGRAMS if s.depth8 else L.PROGRAMS[:1]), name
        assert {c.part for c in cases} == ({None} if s.whole else set()) | (set(L.PARTS) if s.parts else set()), name
        assert {c.mem for c in cases} == ({"pinned", "pageable"} if s.host else {"device"}), name
        for c in cases:
            assert (c.width, c.height) == (328, 55) and c.nframes == s.frames and c.nframes in (1, 3), c.id
            assert c.seeds == (L.SEEDS[:c.nframes] if s.seeded else None) and c.models == s.models and c.mix is None, c.id
            assert T.trace_geometry(L.records(c))[0] == (10 if c.program == L.PROGRAMS[0] else 8), c.id
    assert L.SEEDS == [0, 0xFFFFFFFF, 12345] and L.PARTS == ((16, 32), (32, 23)) and L.PROGRAMS == ("fgs_sei_10_420", "fgs_sei_ff_test6_8_422")
    assert all(n == 3 for n in (L.ENTRIES[e].frames for e in methods if "list" in e or "frames" in e or "copy" in e))


def test_the_host_pipe_is_covered_in_place_with_a_destination_and_narrowed():
    pipe = [c for c in ENTRY_CASES if c.entry == "host_pipe"]
    assert {(c.dst, c.mem) for c in pipe if c.program == L.PROGRAMS[0]} == {(d, m) for d in (None, "planar", "planar8") for m in ("pinned", "pageable")}
    assert {(c.dst, c.mem) for c in pipe if c.program == L.PROGRAMS[1]} == {(d, m) for d in (None, "planar") for m in ("pinned", "pageable")}
    assert all(c.nframes == 3 and c.seeds == L.SEEDS and c.models for c in pipe)


# ---- layouts -----------------------------------------------------------------------------------------------------------------------

def test_the_guards_are_sized_by_the_ring_groups_of_vfgs_layout_h():
    planar, uv = A.ring_group_bytes()
    text = A.LAYOUT_H.read_text()
    assert "constexpr int kMaxUnits = 64;" in text and "#define VFGS_RING 4 " in text and "constexpr int kSpRing = 2;" in text
    assert planar == 4 * 1024 and uv == 2 * 2048          # a planar group is 4 x 1 KiB, a UV group ring x 2 KiB
    assert A.guard_bytes() == max(16 << 10, 2 * max(planar, uv)) >= 16 << 10
    assert A.ring_group_bytes("constexpr int kMaxUnits = 64;\n#define VFGS_RING 4\n#define VFGS_RING_X 16\nconstexpr int kSpRing = 2;") == (16 << 10, 4 << 10)


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_every_plane_lies_where_the_ledger_says(case):
    a = bare_arena(case)
    depth, sx, sy = L.geometry(case)
    nblk = (case.width + 15) // 16
    py, ph = case.part or (0, case.height)
    g = A.guard_bytes()
    # guards and planes tile the arena: a guard in front of every group and behind the last, the planes of a group back to back
    assert len(a.guards) == len(a.groups) + 1
    at = 0
    for i, group in enumerate(a.groups):
        assert a.guards[i][0] == at and a.guards[i][1] - at >= g
        at = a.guards[i][1]
        first = a.planes[group[0]]
        assert first.off == at and first.off % 256 == A.RESIDUES[(i + case.index) % 8] != 0
        for k in group:
            p = a.planes[k]
            assert p.off == at and p.off % 16 == 0
            at += p.pitch * p.rows
        assert case.contig == (len(group) > 1) or case.nframes == 1
        if case.contig:
            assert [a.planes[k].frame for k in group] == list(range(case.nframes)) and len({a.planes[k].role for k in group}) == 1
    assert a.guards[-1] == (at, at + g) and a.buf.size == at + g
    # the smallest legal pitches, exactly the addressed rows
    kinds = {"io": case.src} if case.dst is None else {"src": case.src, "dst": case.dst}
    assert {p.side for p in a.planes} == set(kinds)
    for p in a.planes:
        kind = kinds[p.side]
        sz = 1 if kind in ("planar8", "sp8") or depth == 8 else 2
        samples = 16 * nblk // sx if p.role in ("U", "V") else 16 * nblk
        assert p.sz == sz and p.rowbytes == samples * sz and p.pitch == -(-p.rowbytes // 16) * 16 and p.pitch - p.rowbytes in (0, 8)
        assert p.role in (("Y", "UV") if kind in ("sp", "sp8") else ("Y", "U", "V"))
        if p.role == "Y":
            assert (p.row0, p.rows) == (py, ph)
        else:
            assert p.row0 == py // sy and p.row0 + p.rows == -(-(py + ph) // sy)
    assert len(a.planes) == case.nframes * sum(2 if k in ("sp", "sp8") else 3 for k in kinds.values())
    # the region: the whole blocks of the rows of what is written, nothing of a source
    m = a.region_mask()
    assert int(m.sum()) == sum(p.rows * p.rowbytes for p in a.planes if p.side != "src")
    for lo, hi in a.guards:
        assert not m[lo:hi].any()


def test_every_role_of_every_family_meets_a_base_of_16_mod_32():
    met = {}
    for c in CASES:
        a = bare_arena(c)
        for group in a.groups:
            p = a.planes[group[0]]
            met.setdefault((family_of(c), p.side, p.role), set()).add(p.off % 32)
    assert {f for f, _, _ in met} >= {"rw", "ml", "mix", "sp", "spml", "sp8", "p2sp", "p2sp8", "sp_mix"}
    missing = [k for k, v in met.items() if 16 not in v]
    assert not missing, missing


def test_the_8_pad_bytes_are_met_in_rw_ml_p2sp_and_mix():
    padded = {}
    for c in KEYS:
        depth, sx, _sy = L.geometry(c)
        if depth == 8 and sx == 2:
            a = bare_arena(c)
            if any(p.pitch - p.rowbytes == 8 and p.role in ("U", "V") for p in a.planes):
                padded.setdefault(c.key.family, []).append(c.id)
    assert set(padded) >= {"rw", "ml", "p2sp", "mix"}, sorted(padded)


# ---- the oracle stays inside the region; the grain is visible ------------------------------------------------------------------------

class _View:
    """the planes of one planar in-place picture as they lie in the arena, for T.OracleHW.add_grain_frame"""

    def __init__(self, a, buf, c, f):
        (self.Y, ys), (self.U, cs), (self.V, _) = [self._plane(a, buf, a.plane("io", f, r)) for r in "YUV"]
        self.width, self.height, self.stride, self.cstride = c.width, c.height, ys, cs

    @staticmethod
    def _plane(a, buf, p):
        return a.rows(p, buf), p.pitch // p.sz


def changed_shares(a, before, after):
    """per role of the written planes: the share of the region's containers that differ"""
    n, d = {}, {}
    for p in a.planes:
        if p.side != "src":
            dt = np.uint8 if p.sz == 1 else np.uint16
            x, y = (np.ascontiguousarray(a.rows(p, b)[:, :p.rowbytes]).view(dt) for b in (before, after))
            n[p.role] = n.get(p.role, 0) + x.size
            d[p.role] = d.get(p.role, 0) + int((x != y).sum())
    return {r: d[r] / n[r] for r in n}


@pytest.mark.parametrize("case", SHAPES, ids=ident)
def test_the_oracle_stays_inside_the_region_and_the_grain_is_visible(case):
    a = L.make_arena(case)
    before = a.buf.copy()
    e = L.expected(a, case)
    assert np.array_equal(a.buf, before), "expected() changed the arena it was given"
    region = a.region_mask()
    outside = (e.buf != before) & ~region
    assert not outside.any(), a.describe(int(np.flatnonzero(outside)[0]))
    direct = case.src == "planar" and case.dst is None and not case.mix and not case.stripe and case.part is None
    if direct:
        # the oracle itself on the caller's memory: smallest pitches, exact rows, the ragged last block row, random bytes all around
        buf = before.copy()
        if case.seeds is None:
            ora = U.oracle_programmed(L.records(case))
        for f in range(case.nframes):
            if case.seeds is not None:
                ora = U.oracle_programmed(L.records(case))
                ora.set_seed(case.seeds[f])
            ora.add_grain_frame(_View(a, buf, case, f))
        A.compare(a, buf, e.buf, None, "the oracle on the arena itself")
        assert ora.seed_state() == e.regs
    if case.dst is None:
        shares = changed_shares(a, before, e.buf)
        print(f"{case.id}: changed shares {shares}" + (" (the oracle ran on the arena itself)" if direct else ""))
        assert min(shares.values()) >= 0.25, "change the case's content or seed, not the threshold"


# ---- under the mix ---------------------------------------------------------------------------------------------------------------------

MIXED = [c for c in KEYS if c.mix]


@pytest.mark.parametrize("case", MIXED, ids=ident)
def test_the_mix_stays_within_its_cap_at_the_new_heights(case):
    a = L.make_arena(case)
    e = L.expected(a, case)
    plain = L.expected(a, case._replace(mix=None))
    left_out = e.excluded / e.processed
    assert e.compared is not None and not (~e.compared & ~a.region_mask()).any(), "a byte outside the region is left out of the comparison"
    chroma = np.zeros(a.buf.size, bool)
    for p in a.planes:
        if p.side != "src" and p.role != "Y":
            a.rows(p, chroma)[:, :p.rowbytes] = True
    assert not (~e.compared & ~chroma).any(), "only chroma is masked"
    compared = chroma & e.compared
    effect = int(((e.buf != plain.buf) & compared).sum()) / int(compared.sum())
    print(f"{case.id}: {left_out:.4f} of the processed chroma samples left out; the mix changes {effect:.4f} of the compared chroma bytes")
    assert len(MIXED) == 22 and left_out <= K.MIX_CAP == 0.10, "change the case's content, not the cap"
    assert effect >= 0.25, "change the case's content, not the threshold"
    assert e.regs == plain.regs


# ---- the comparison sees what it is for --------------------------------------------------------------------------------------------

def by_id(i):
    return next(c for c in CASES if c.id == i)


def mutated(case, offset_of):
    a = L.make_arena(case)
    e = L.expected(a, case)
    A.compare(a, e.buf.copy(), e.buf, e.compared, "unchanged")
    got = e.buf.copy()
    o = offset_of(a)
    got[o] ^= 0x40
    with pytest.raises(AssertionError) as err:
        A.compare(a, got, e.buf, e.compared, case.id)
    return a, str(err.value)


def test_a_byte_of_the_guard_in_front_of_plane_0_is_seen():
    a, msg = mutated(KEYS[0], lambda a: a.planes[0].off - 1)
    assert "plane io.f0.Y, row -1 " in msg and "in front of the plane" in msg and "in a guard" in msg and f"byte {a.planes[0].pitch - 1} of the row" in msg


@pytest.mark.parametrize("plane", [0, 1, 2, 5])
def test_the_byte_directly_behind_a_planes_last_row_is_seen(plane):
    a, msg = mutated(KEYS[0], lambda a: a.planes[plane].off + a.planes[plane].rows * a.planes[plane].pitch)
    p = a.planes[plane]
    assert f"plane {p.name}, row {p.rows} " in msg and "behind the plane" in msg and "byte 0 of the row: in a guard" in msg


@pytest.mark.parametrize("k", range(8))
def test_each_of_the_8_pad_bytes_of_an_8_bit_chroma_row_is_seen(k):
    case = KEYS[0]
    assert L.geometry(case) == (8, 2, 2)
    a, msg = mutated(case, lambda a: a.plane("io", 1, "V").off + 27 * a.plane("io", 1, "V").pitch + 168 + k)
    p = a.plane("io", 1, "V")
    assert (p.pitch, p.rowbytes, p.rows) == (176, 168, 28)
    assert f"plane io.f1.V, row 27 (row 27 of the arena's), byte {168 + k} of the row: in the pad" in msg


def test_a_byte_of_a_source_of_an_out_of_place_case_is_seen():
    case = next(c for c in KEYS if c.key.family == "p2sp8")
    a, msg = mutated(case, lambda a: a.plane("src", 1, "U").off + 3 * a.plane("src", 1, "U").pitch + 7)
    assert "plane src.f1.U, row 3 (row 3 of the arena's), byte 7 of the row: in a source" in msg


@pytest.mark.parametrize("entry", ["add_grain_frame_part_dev", "add_grain_stripe_dev", "add_grain_frame_list_seeded_part_dev"])
def test_a_byte_of_the_row_above_a_part_and_of_the_line_behind_it_are_seen(entry):
    case = next(c for c in ENTRY_CASES if c.entry == entry and c.part == (16, 32) and c.program == L.PROGRAMS[0])
    a, msg = mutated(case, lambda a: a.plane("io", 0, "Y").off - a.plane("io", 0, "Y").pitch + 5)
    assert "plane io.f0.Y, row 15 (row -1 of the arena's: in front of the plane), byte 5 of the row: in a guard" in msg
    a, msg = mutated(case, lambda a: a.plane("io", 0, "U").off + a.plane("io", 0, "U").rows * a.plane("io", 0, "U").pitch + 9)
    assert "plane io.f0.U, row 24 (row 16 of the arena's: behind the plane), byte 9 of the row: in a guard" in msg


def test_a_masked_sample_under_the_mix_is_the_only_thing_left_out():
    case = MIXED[0]
    a = L.make_arena(case)
    e = L.expected(a, case)
    left = np.flatnonzero(~e.compared)
    assert len(left) and a.region_mask()[left].all()
    got = e.buf.copy()
    got[left[0]] ^= 1
    A.compare(a, got, e.buf, e.compared, "a left-out sample")
    with pytest.raises(AssertionError):
        A.compare(a, got, e.buf, None, "the same without the mask")
