"""CPU: the case tables of tests/test_gpu_model_list_out8.py and tests/test_gpu_sp_model_list_out8.py (tests/model_out8_util.py PLANAR_CASES,
SP_CASES) on the oracle alone, so that what the GPU files compare against is known to be worth comparing before a GPU runs:

* every case's expectation distinguishes its models: for every model of a case's list there is a frame whose expected bytes under its
  own model differ, in every plane, from what another model of the list gives for the same frame and seed -- a kernel that took another
  frame's image, bounds or shift cannot pass by luck;
* no sample is left out of the comparison: the expectation has the destination's full planes, padding included; the region it writes
  covers every sample of the picture (whole blocks of every row); outside it every byte is the fill's, inside it the bytes are the
  oracle's (they differ from a garbage fill almost everywhere).

The cases run at their own widths; the two-front cases keep their width (8192) and run 48 rows here -- the height only decides how a launch
is scheduled, which is the GPU's business."""
import numpy as np
import pytest

import model_list_util as U
import model_out8_util as M8
import semiplanar_out8_util as SP8
import semiplanar_util as SP
import vfgs_testlib as T

CPU_ROWS = 48


def records(programs):
    return [U.model_records(p) if isinstance(p, str) else list(p) for p in programs]


def size_of(case, wh):
    w, h = wh
    return (w, CPU_ROWS) if case.startswith("two_fronts") else (w, h)


def assert_every_model_is_told_apart(case, recs, pick, differs):
    """differs(a, b): per plane, whether a frame of model a under model b (same frame, same seed) is another picture.  Every model of the
    list must be told apart in EVERY plane from another one of the list, and every two models in at least one plane -- but for fgs_sei
    and default in the set the cases take over from tests/test_gpu_model_list.py CONFIGS: the same message twice."""
    used = sorted(set(pick))
    assert len(used) >= 2, "a case with one model says nothing about models"
    apart = {(a, b): differs(a, b) for a in used for b in used if a != b}
    for a in used:
        assert any(all(apart[a, b]) for b in used if b != a), (case, a)
    same = sorted((a, b) for (a, b), d in apart.items() if not any(d))
    assert same == ([(0, 1), (1, 0)] if case == "every_format_10_420_general" else []), (case, same)


def check_coverage(want, fill, regions, width, height):
    """regions: per plane (rows, cols, picture rows, picture cols)"""
    for name, (rows, cols, prow, pcol) in regions.items():
        w, f = getattr(want, name), getattr(fill, name)
        assert w.shape == f.shape and w.dtype == np.uint8
        assert rows >= prow and cols >= pcol and rows <= w.shape[0] and cols <= w.shape[1], (name, rows, cols, prow, pcol, w.shape)
        outside = np.ones(w.shape, bool)
        outside[:rows, :cols] = False
        assert np.array_equal(w[outside], f[outside]), name
        assert (w[:rows, :cols] != f[:rows, :cols]).mean() > 0.9, name


@pytest.mark.parametrize("case", sorted(M8.PLANAR_CASES))
def test_planar_case(case):
    names, pick, wh, fseed = M8.PLANAR_CASES[case]
    recs = records(names)
    pick = M8.pick_of(pick, len(names))
    w, h = size_of(case, wh)
    depth, sx, sy = T.trace_geometry(recs[-1])
    frames = [M8.garbage_frame(w, h, depth, sx, sy, fseed + i) for i in range(len(pick))]
    seeds = M8.fresh_seeds(len(pick), 1)
    fill = M8.dst_frame(w, h, sx, sy, 4321)
    own, regs, _ = M8.expect_planar(recs, pick, frames, seeds, fill)
    assert len(own) == len(frames) and len(regs) == 4
    rows, crows, cols, ccols = M8.written_region(frames[0])
    cw, ch = (w + sx - 1) // sx, (h + sy - 1) // sy
    for o in own:
        check_coverage(o, fill, {"Y": (rows, cols, h, w), "U": (crows, ccols, ch, cw), "V": (crows, ccols, ch, cw)}, w, h)
    def differs(a, b):
        i = pick.index(a)
        other, _, _ = M8.expect_planar(recs, [b], [frames[i]], [seeds[i]], fill)
        return [not np.array_equal(p, q) for p, q in zip(own[i].planes(), other[0].planes())]
    assert_every_model_is_told_apart(case, recs, pick, differs)
    # one seed sequence: the same loop on one oracle; frame 0 of it is a frame of its model as well
    seq, regs2, _ = M8.expect_planar(recs, pick, frames, None, fill)
    assert len(regs2) == 4 and not seq[0].equal_all(fill)


@pytest.mark.parametrize("case", sorted(M8.SP_CASES))
def test_semi_planar_case(case):
    names, pick, wh, fseed = M8.SP_CASES[case]
    recs = records(names)
    w, h = size_of(case, wh)
    depth, sx, sy = T.trace_geometry(recs[-1])
    assert sx == 2
    shift = next((M8.SP_CONFIGS[c][1] for c in M8.SP_CONFIGS if case.startswith(c + "_")), 16 - depth)
    frames = [SP.garbage_sp_frame(w, h, depth, sy, shift, fseed + i) for i in range(len(pick))]
    seeds = M8.fresh_seeds(len(pick), 1)
    fill = SP8.dst_frame(w, h, sy, 4321, 16, 48)
    own, regs, _ = M8.expect_sp(recs, pick, frames, seeds, fill)
    assert len(own) == len(frames) and len(regs) == 4
    rows, crows, cols = SP.written_region(frames[0])
    for o in own:
        check_coverage(o, fill, {"Y": (rows, cols, h, w), "UV": (crows, cols, (h + sy - 1) // sy, 2 * ((w + 1) // 2))}, w, h)
    def differs(a, b):
        i = pick.index(a)
        other, _, _ = M8.expect_sp(recs, [b], [frames[i]], [seeds[i]], fill)
        o, x = own[i], other[0]
        return [not np.array_equal(o.Y, x.Y), not np.array_equal(o.UV[:, 0::2], x.UV[:, 0::2]), not np.array_equal(o.UV[:, 1::2], x.UV[:, 1::2])]
    assert_every_model_is_told_apart(case, recs, pick, differs)
    seq, regs2, _ = M8.expect_sp(recs, pick, frames, None, fill)
    assert len(regs2) == 4 and not seq[0].equal_all(fill)


def test_the_tables_hold_what_the_issue_lists():
    assert sorted(M8.PLANAR_CONFIGS) == ["10_420", "10_420_general", "10_422", "10_440", "10_444", "12_420"]
    assert {c: M8.PLANAR_CASES[c][2] for c in ("34_frames", "narrow_1920", "narrow_960", "two_fronts")} == \
        {"34_frames": (136, 32), "narrow_1920": (1920, 48), "narrow_960": (960, 48), "two_fronts": (8192, 1366)}
    assert len(M8.PLANAR_CASES["34_frames"][1]) == 34 and M8.FORM_CHANGE_PICK == [0, 0, 1, 1, 1, 0]
    assert sorted(M8.SP_CONFIGS) == ["low_aligned", "p010", "p012", "p210"] and M8.SP_SIZES == [(1047, 40), (1032, 90)] and M8.SP_PICK == [0, 1, 0, 2, 1]
    assert [M8.SP_CONFIGS[c][1] for c in ("p010", "p210", "p012", "low_aligned")] == [6, 6, 4, 0]
