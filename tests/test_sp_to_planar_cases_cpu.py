"""CPU: the case table of tests/sp_to_planar_cases.py on the oracle alone, so that tests/test_gpu_sp_to_planar.py cannot pass vacuously:
every case changes at least a quarter of the written samples of every plane role, the models of a case with a model per picture are told
apart in Y, Cb and Cr, the sources' low bits are non-zero where sample_shift > 0 and the expectation ignores them, no case leaves a sample
of the picture out, and the table covers what the issue of this feature lists."""
import numpy as np
import pytest

import semiplanar_util as SP
import sp_model_list_util as SU
import sp_to_planar_cases as C


@pytest.fixture(scope="module")
def worked():
    """case id -> (sources, fills, expectation, registers): computed once"""
    out = {}
    for c in C.CASES:
        frames = C.sources(c)
        fills = [C.fill_for(f, 7 + i, c.pad, c.cpad) for i, f in enumerate(frames)]
        want, regs = C.expected(c, frames, fills)
        out[c.id] = (frames, fills, want, regs)
    return out


def test_the_table_covers_the_widths_heights_and_formats():
    ids = [c.id for c in C.CASES]
    assert len(ids) == len(set(ids))
    plain = [c for c in C.CASES if c.models is None]
    for fmt, (prog, shifts) in C.FORMATS.items():
        mine = [c for c in plain if c.program == prog]
        assert {c.blocks for c in mine} >= set(C.BLOCKS[:-1]), fmt
        assert {c.shift for c in mine} == set(shifts) and {c.height for c in mine} == set(C.HEIGHTS), fmt
    depths_at_512 = {C.geometry(c)[0] for c in C.CASES if c.blocks == 512}
    assert depths_at_512 == {8, 10, 12}
    assert {C.geometry(c)[1] for c in C.CASES} == {1, 2}
    for prog in C.FORMS:
        assert {c.seeded for c in plain if c.program == prog and c.pad} == {False, True}, prog
    # the four forms, and a form on record for every program a case without models names
    assert {C.FORM_OF[p] for p in C.FORMS} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c.program for c in plain} <= set(C.FORM_OF)
    with_models = [c for c in C.CASES if c.models]
    assert {C.geometry(c)[0] for c in with_models} == {8, 10, 12} and {c.seeded for c in with_models} == {False, True}
    assert all(c.height in C.HEIGHTS and c.blocks in C.BLOCKS for c in C.CASES)
    assert any(C.geometry(c) == (8, 2) and c.blocks % 2 for c in C.CASES)     # an 8-bit chroma row that ends in half a unit


@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_case_cannot_pass_vacuously(worked, case):
    frames, fills, want, regs = worked[case.id]
    assert len(frames) == C.NFRAMES
    depth, sy = C.geometry(case)
    for f, fill, w in zip(frames, fills, want):
        rows, crows, cols = C.written(f)
        # no sample of the picture is left out: the written region holds every row and every column of the picture, in every plane
        assert rows == f.height and crows == -(-f.height // sy) and cols >= f.width and cols % 16 == 0 and cols - f.width < 16
        assert w.Y.shape[0] == rows and w.U.shape[0] == crows and w.V.shape[0] == crows
        src = SP.to_planar(f)
        for (role, got), s, (_, before), n in zip(w.planes(), src.planes(), fill.planes(), (cols, cols // 2, cols // 2)):
            r = got.shape[0]
            changed = np.count_nonzero(got[:, :n] != s[:r, :n])
            assert 4 * changed >= r * n, (case.id, role, changed, r * n)
            assert np.array_equal(got[:, n:], before[:, n:]), (case.id, role)       # the padding keeps its bytes
            assert int(got[:, :n].max()) < (1 << depth) or case.shift == 0, (case.id, role)
        if case.shift:
            low = (1 << case.shift) - 1
            assert (f.Y & low).any() and (f.UV & low).any(), case.id
    if case.shift:
        # ... and the expectation ignores them
        cleared = [SP.SPFrame(f.width, f.height, f.depth, f.suby, f.stride, f.uv_stride, f.shift, f.Y & ~np.array((1 << case.shift) - 1, f.dtype),
                              f.UV & ~np.array((1 << case.shift) - 1, f.dtype)) for f in frames]
        again, regs2 = C.expected(case, cleared, fills)
        assert regs2 == regs
        for a, b in zip(again, want):
            assert all(np.array_equal(x, y) for (_, x), (_, y) in zip(a.planes(), b.planes())), case.id


@pytest.mark.parametrize("case", [c for c in C.CASES if c.models], ids=[c.id for c in C.CASES if c.models])
def test_models_are_told_apart_in_every_plane(case):
    recs = [C.records_of(m) for m in case.models]
    f = C.sources(case)[:1]
    outs = [SP.to_planar(SU.expect_seeded(recs, [k], f, [5], case.shift)[0][0]) for k in range(len(recs))]
    rows, crows, cols = C.written(f[0])
    for a in range(len(outs)):
        for b in range(a + 1, len(outs)):
            for pa, pb, r, n in zip(outs[a].planes(), outs[b].planes(), (rows, crows, crows), (cols, cols // 2, cols // 2)):
                assert not np.array_equal(pa[:r, :n], pb[:r, :n]), (case.id, a, b)
    assert set(C.pick_of(case)) == ({0, 1, 2} if case.seeded else {0, 1})
