"""CPU: the case tables of tests/test_gpu_models_to_sp.py (tests/models_to_sp_util.py SURFACES, CASES) on the oracle alone, so that what the
GPU file compares against is known to be worth comparing before a GPU runs:

* every case's expectation distinguishes its models: for every model of a case's list there is a frame whose expected containers under
  its own model differ, in Y, in Cb AND in Cr, from what another model of the list gives for the same frame and seed -- a kernel that
  took another frame's image, bounds or shift cannot pass by luck;
* every surface case holds a model of another form (model_programs.expected_form), and A B A C B makes at least three runs;
* no sample is left out of the comparison: the expectation has the destination's full planes, padding included; the region it writes
  covers every sample of the picture (whole blocks of every row); outside it every container is the fill's, inside it the containers are
  the oracle's (they differ from a garbage fill almost everywhere)."""
import numpy as np
import pytest

import model_list_util as U
import model_programs as MP
import models_to_sp_util as M
import semiplanar_util as SP
import vfgs_testlib as T


def planes(x):
    return [x.Y, x.UV[:, 0::2], x.UV[:, 1::2]]


def check_coverage(want, fill, w, h, sy):
    rows, crows, cols = SP.written_region(want)
    assert rows >= h and cols >= w and crows >= (h + sy - 1) // sy and cols >= 2 * ((w + 1) // 2)
    for name, r in (("Y", rows), ("UV", crows)):
        a, f = getattr(want, name), getattr(fill, name)
        assert a.shape == f.shape and a.dtype == f.dtype and r <= a.shape[0] and cols <= a.shape[1], (name, a.shape, r, cols)
        outside = np.ones(a.shape, bool)
        outside[:r, :cols] = False
        assert outside.any() and np.array_equal(a[outside], f[outside]), name
        assert (a[:r, :cols] != f[:r, :cols]).mean() > 0.9, name


@pytest.mark.parametrize("case", sorted(M.CASES))
def test_case(case):
    names, pick, (w, h), shift, out8, fseed = M.CASES[case]
    recs = M.case_records(case)
    depth, sx, sy = T.trace_geometry(recs[-1])
    assert sx == 2 and all(T.trace_geometry(r) == (depth, sx, sy) for r in recs) and shift in (0, 16 - depth) and (depth > 8 or not out8)
    assert (w, h) in M.SHAPES and max(pick) == len(recs) - 1
    frames = [M.garbage_frame(w, h, depth, sy, fseed + i) for i in range(len(pick))]
    seeds = M.fresh_seeds(len(pick), 1)
    fill = M.fill_for(w, h, depth, sy, shift, out8, 4321)
    assert fill.stride != fill.uv_stride and fill.Y.dtype == (np.uint8 if out8 or depth == 8 else np.uint16)
    own, regs, _ = M.expect(recs, pick, frames, seeds, shift, out8, fill)
    assert len(own) == len(frames) and len(regs) == 4
    for o in own:
        check_coverage(o, fill, w, h, sy)

    # every model of the list is told apart in EVERY plane from another one of the list, and every two models in at least one plane
    used = sorted(set(pick))
    assert len(used) >= 2, "a case with one model says nothing about models"

    def differs(a, b):
        i = pick.index(a)
        other, _, _ = M.expect(recs, [b], [frames[i]], [seeds[i]], shift, out8, fill)
        return [not np.array_equal(p, q) for p, q in zip(planes(own[i]), planes(other[0]))]

    apart = {(a, b): differs(a, b) for a in used for b in used if a != b}
    for a in used:
        assert any(all(apart[a, b]) for b in used if b != a), (case, a, apart)
    assert all(any(d) for d in apart.values()), (case, apart)

    # the models of ONE launch (a run of one form) differ in all three planes on that run's frames
    forms = [MP.expected_form(r) for r in recs]
    f0 = 0
    for n in U.runs_of(forms, pick):
        run = sorted(set(pick[f0:f0 + n]))
        for a in run:
            assert all(all(apart[a, b]) for b in run if b != a), (case, f0, n, a)
        f0 += n

    # one seed sequence: the same loop on one oracle; frame 0 of it is a frame of its model as well
    seq, regs2, _ = M.expect(recs, pick, frames, None, shift, out8, fill)
    assert len(regs2) == 4 and not seq[0].equal_all(fill)


@pytest.mark.parametrize("surface", sorted(M.SURFACES))
def test_a_surface_case_holds_a_model_of_another_form(surface):
    names, shift, out8 = M.SURFACES[surface]
    forms = [MP.expected_form(r) for r in M.records(names)]
    assert forms[2] != forms[0], forms
    assert len(U.runs_of(forms, M.PICK)) >= 3, forms


def test_the_bounds_cases_differ_in_range_shift_and_scale_luts():
    for case in ("bounds_p010", "bounds_nv12"):
        a, b = M.case_records(case)
        assert MP.expected_form(a) == MP.expected_form(b)
        last = lambda rec, op: [r for r in rec if r[0] == op][-1]
        assert last(a, T.OP_LEGAL_RANGE)[1] != last(b, T.OP_LEGAL_RANGE)[1] and last(a, T.OP_SCALE_SHIFT)[1] != last(b, T.OP_SCALE_SHIFT)[1]
        for c in range(3):
            la = [r for r in a if r[0] == T.OP_SCALE_LUT and r[1] == c][-1]
            lb = [r for r in b if r[0] == T.OP_SCALE_LUT and r[1] == c][-1]
            assert bytes(la[3]) != bytes(lb[3])


def test_the_tables_hold_what_the_issue_lists():
    assert M.SHAPES == [(136, 33), (1047, 40), (1032, 90)] and M.SURFACE_SIZES == [(1047, 40), (1032, 90)]
    assert M.PICK == [0, 1, 0, 2, 1] and M.BOUNDS_PICK == [1, 0, 0, 1, 0, 1, 1]
    assert {s: (v[1], v[2]) for s, v in M.SURFACES.items()} == {
        "p010": (6, False), "p210": (6, False), "p012": (4, False), "low_aligned": (0, False), "nv12": (0, False), "nv16": (0, False),
        "10_to_nv12": (0, True), "10_to_nv16": (0, True), "12_to_nv12": (0, True), "12_to_nv16": (0, True)}
    geo = {s: T.trace_geometry(M.records(v[0])[-1]) for s, v in M.SURFACES.items()}
    assert geo == {"p010": (10, 2, 2), "p210": (10, 2, 1), "p012": (12, 2, 2), "low_aligned": (10, 2, 2), "nv12": (8, 2, 2), "nv16": (8, 2, 1),
                   "10_to_nv12": (10, 2, 2), "10_to_nv16": (10, 2, 1), "12_to_nv12": (12, 2, 2), "12_to_nv16": (12, 2, 1)}, geo
    assert len(M.CASES["34_frames_p010"][1]) == 34 and M.CASES["34_frames_p010"][2] == (136, 33) and M.CASES["34_frames_nv12"][4]
    assert all(wh in M.SHAPES for _, _, wh, _, _, _ in M.CASES.values())
