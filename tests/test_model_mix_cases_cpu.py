"""CPU: the case table of tests/test_gpu_model_list_mix.py (tests/model_mix_list_util.py) through the oracle alone, before anything runs on a
GPU: for every case the derivation of tests/chroma_mix_util.py leaves out NO sample -- its condition for the GPU comparison to cover every
chroma sample -- the models of a list do differ in their mix and in their pictures, and the helpers say what the firmware layer derives."""
import numpy as np
import pytest

import chroma_mix_util as X
import model_mix_list_util as MU
import semiplanar_util as SP
import vfgs_testlib as T


def cases():
    for cid, (spec, w, h) in MU.PLANAR.items():
        yield pytest.param(spec, w, h, id="planar-" + cid)
    for cid, (spec, w, h, _shift) in MU.SEMIPLANAR.items():
        yield pytest.param(spec, w, h, id="sp-" + cid)
    yield pytest.param(MU.CYCLE, *MU.CYCLE_SIZE, id="cycle")


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("spec, w, h", list(cases()))
def test_no_sample_is_left_out(spec, w, h, seeded):
    models = MU.case_models(spec)
    pick = MU.PICK if len(spec) == 3 else [i % len(spec) for i in range(34)]
    frames = MU.case_frames(spec, w, h, len(pick), 5)
    res, excluded, _regs, _ = MU.expect_list(models, pick, frames, MU.fresh_seeds(len(pick), 1) if seeded else None)
    total = sum(f.U.size + f.V.size for f in frames)
    print(f"excluded by the derivation: {excluded} of {total} chroma samples")
    assert excluded == 0
    # grain was added, and luma is the oracle's
    assert all(not np.array_equal(want.U, f.U) and not np.array_equal(want.Y, f.Y) for (want, _), f in zip(res, frames))


def test_models_of_a_list_differ_in_their_pictures():
    """the same frame through model A's mix and through none is another picture: a launch that ignored the mix would be seen"""
    spec, w, h = MU.PLANAR["10_420_1047x40"]
    (rec, mixes) = MU.case_models(spec)[0]
    f = MU.case_frames(spec, w, h, 1, 9)
    a, _, _, _ = MU.expect_list([(rec, mixes)], [0], f, [7])
    b, _, _, _ = MU.expect_list([(rec, (None, None))], [0], f, [7])
    assert np.array_equal(a[0][0].Y, b[0][0].Y) and not np.array_equal(a[0][0].U, b[0][0].U) and not np.array_equal(a[0][0].V, b[0][0].V)


def test_mix_of_is_what_the_firmware_layer_derives():
    assert MU.mix_of("luma_only") == ((64, 0, 0), (64, 0, 0)) and MU.mix_of("neutral") == (X.NEUTRAL, X.NEUTRAL)
    assert MU.mix_of("tbl") == ((64, 119, -238), (54, 101, -202)) and MU.mix_of("cfl") == ((64, 0, 0), (64, 0, 0))
    assert MU.mix_of("none") == (None, None) and MU.mix_of("cb_only")[1] is None
    a = MU.parameter_set("fgs_afgs1_test1_10_420", "tbl")
    assert (a.cb_mult, a.cb_luma_mult, a.cb_offset, a.cr_mult, a.cr_luma_mult, a.cr_offset) == (247, 192, 18, 229, 182, 54)
    assert MU.parameter_set("fgs_afgs1_test1_10_420", "cfl").chroma_scaling_from_luma == 1
    rec = MU.records("fgs_afgs1_test1_10_420", "cfl")
    luts = {a: p for op, a, _b, p in rec if op == T.OP_SCALE_LUT}
    assert luts[1] == luts[0] == luts[2]


def test_semiplanar_expectation_round_trips():
    spec, w, h, shift = MU.SEMIPLANAR["p010_1047x40"]
    f = MU.case_frames(spec, w, h, 1, 3)[0]
    sp = SP.to_semiplanar(f, shift, 11)
    d = SP.to_planar(sp)
    assert d.equal_all(f)
    w_, m = MU.to_sp_expectation(sp, f, [np.ones(f.U.shape, bool), np.ones(f.V.shape, bool)])
    rows, crows, cols = SP.written_region(sp)
    assert np.array_equal(w_.Y[:rows, :cols], f.Y[:rows, :cols] << shift) and np.array_equal(w_.Y[:, cols:], sp.Y[:, cols:]) and m.all()
