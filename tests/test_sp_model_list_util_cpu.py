"""CPU: the expectation of the tests of semi-planar frames with a model per picture (tests/sp_model_list_util.py) pinned against its two
parents' helpers, which are pinned themselves (tests/test_semiplanar_util_cpu.py against recorded reference output):

* with ONE model on every frame the contract's loop is the plain semi-planar call: tests/semiplanar_util.py's expectation;
* on the planar twin D(frame) it is the planar models call: tests/model_list_util.py's expectation, on the written region -- whole blocks
  of the picture's rows -- and on the four registers."""
import numpy as np
import pytest

import model_list_util as U
import semiplanar_util as SP
import sp_model_list_util as SU

SETS = {
    "8_420": (["fgs_afgs1_test1_8_420", "fgs_sei_8_420"], 0),
    "10_420": (["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"], 6),
    "10_422": (["fgs_sei_10_422", "fgs_afgs1_test3_10_422"], 0),
    "12_420": (["fgs_sei_10_420@depth12", "fgs_afgs1_test1_10_420@depth12"], 4),
}
W, H = 200, 41


def frames_of(recs, n, shift, seed):
    import vfgs_testlib as T
    depth, sx, sy = T.trace_geometry(recs[-1])
    assert sx == 2
    return [SP.garbage_sp_frame(W, H, depth, sy, shift, seed + i) for i in range(n)]


def same(a, b):
    return all(x.equal_all(y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("cfg", sorted(SETS))
def test_one_model_on_every_frame_is_the_plain_semi_planar_call(cfg, seeded):
    names, shift = SETS[cfg]
    recs = [U.model_records(n) for n in names]
    frames = frames_of(recs, 4, shift, 10)
    seeds = [7, 0, 0xFFFFFFFF, 7] if seeded else None
    for k in range(len(recs)):
        ora = U.oracle_programmed(recs[k])
        want = SP.expected(ora, frames, seeds, shift)
        if seeded:
            got, regs = SU.expect_seeded(recs, [k] * 4, frames, seeds, shift)
        else:
            got, regs = SU.expect_unseeded(U.oracle_programmed(recs[k]), recs, [k] * 4, frames, shift)
        assert same(got, want) and regs == ora.seed_state()


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("cfg", sorted(SETS))
def test_on_the_planar_twin_it_is_the_planar_models_call(cfg, seeded):
    names, shift = SETS[cfg]
    recs = [U.model_records(n) for n in names]
    pick = [i % len(recs) for i in range(5)]
    frames = frames_of(recs, 5, shift, 20)
    planar = [SP.to_planar(f) for f in frames]
    seeds = [3, 3, 0x80000000, 12345, 1]
    if seeded:
        got, regs = SU.expect_seeded(recs, pick, frames, seeds, shift)
        want, pregs = U.expect_seeded(recs, pick, planar, seeds)
    else:
        got, regs = SU.expect_unseeded(U.oracle_programmed(recs[-1]), recs, pick, frames, shift)
        want, pregs = U.expect_unseeded(U.oracle_programmed(recs[-1]), recs, pick, planar)
    assert regs == pregs
    rows, crows, cols = SP.written_region(frames[0])
    for g, w, src in zip(got, want, frames):
        d = SP.to_planar(g)
        assert np.array_equal(d.Y[:rows, :cols], w.Y[:rows, :cols])
        assert np.array_equal(d.U[:crows, :cols // 2], w.U[:crows, :cols // 2]) and np.array_equal(d.V[:crows, :cols // 2], w.V[:crows, :cols // 2])
        # everything else keeps the source's containers, low bits included; the written ones have zero low bits
        assert np.array_equal(g.Y[rows:], src.Y[rows:]) and np.array_equal(g.Y[:, cols:], src.Y[:, cols:])
        assert np.array_equal(g.UV[crows:], src.UV[crows:]) and np.array_equal(g.UV[:, cols:], src.UV[:, cols:])
        assert not (g.Y[:rows, :cols] & ((1 << shift) - 1)).any() and not (g.UV[:crows, :cols] & ((1 << shift) - 1)).any()


def test_the_models_of_a_set_differ():
    """(or the tests above would hold for a helper that ignores `pick`)"""
    for cfg, (names, shift) in SETS.items():
        recs = [U.model_records(n) for n in names]
        frames = frames_of(recs, 1, shift, 30)
        a, _ = SU.expect_seeded(recs, [0], frames, [9], shift)
        b, _ = SU.expect_seeded(recs, [1], frames, [9], shift)
        assert not a[0].equal_all(b[0]), cfg
