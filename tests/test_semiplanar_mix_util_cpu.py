"""CPU: the expectation of the semi-planar call under a chroma mix (tests/semiplanar_mix_util.py) has the properties the GPU tests lean on,
and every input of tests/test_gpu_semiplanar_mix.py stays within its exclusion cap on the oracle alone."""
import numpy as np
import pytest

import chroma_mix_util as X
import semiplanar_mix_util as M
import semiplanar_util as SP
import test_gpu_semiplanar_mix as G
import vfgs_testlib as T


def oracle(rec):
    ora = T.OracleHW()
    T.replay(ora, rec)
    return ora


@pytest.mark.parametrize("name,shift", [("fgs_afgs1_test1_8_420", 0), ("fgs_afgs1_test1_10_420", 6), ("fgs_afgs1_test3_10_422", 0)])
def test_neutral_mix_is_the_plain_expectation(name, shift):
    """(0, 64, 0): the index is the sample, so for in-range content the result is semiplanar_util.expected, with nothing left out of
    the comparison that differs"""
    rec = T.load_trace(name)
    depth, sx, sy = T.trace_geometry(rec)
    frames = M.ranged_sp_frames(333, 33, depth, sy, shift, 2, 5, lo=0.0, hi=1.0)
    seeds = [9, 0xFFFFFFFF]
    a, b = oracle(rec), oracle(rec)
    res, _ = M.expected(a, rec, frames, seeds, shift, (X.NEUTRAL, X.NEUTRAL))
    plain = SP.expected(b, frames, seeds, shift)
    for (w, m), p in zip(res, plain):
        assert w.equal_all(p)
    assert a.seed_state() == b.seed_state()


@pytest.mark.parametrize("shift", [0, 6])
def test_outside_the_whole_blocks_the_expectation_is_the_source(shift):
    rec = T.load_trace("fgs_afgs1_test1_10_420")
    frames = M.ranged_sp_frames(345, 17, 10, 2, shift, 2, 6)
    res, _ = M.expected(oracle(rec), rec, frames, None, shift, G.BOTH)
    rows, crows, cols = SP.written_region(frames[0])
    assert cols == 352 and crows == 9 and frames[0].stride > cols
    for f, (w, m) in zip(frames, res):
        assert np.array_equal(w.Y[:, cols:], f.Y[:, cols:]) and np.array_equal(w.Y[rows:], f.Y[rows:])
        assert np.array_equal(w.UV[:, cols:], f.UV[:, cols:]) and np.array_equal(w.UV[crows:], f.UV[crows:])
        assert m[:, cols:].all() and m[crows:].all()
        assert not np.array_equal(w.UV[:crows, :cols], f.UV[:crows, :cols])
        if shift:
            assert (f.UV[:, cols:] & 63).any() and not (w.UV[:crows, :cols] & 63).any() and not (w.Y[:rows, :cols] & 63).any()


def test_source_low_bits_do_not_change_the_expectation():
    rec = T.load_trace("fgs_afgs1_test1_10_420")
    noisy = M.ranged_sp_frames(345, 17, 10, 2, 6, 2, 7)
    clean = M.ranged_sp_frames(345, 17, 10, 2, 6, 2, 7, low_bits=False)
    assert any((f.Y & 63).any() and (f.UV & 63).any() for f in noisy) and not any((f.Y & 63).any() or (f.UV & 63).any() for f in clean)
    a, _ = M.expected(oracle(rec), rec, noisy, None, 6, G.CORPUS)
    b, _ = M.expected(oracle(rec), rec, clean, None, 6, G.CORPUS)
    rows, crows, cols = SP.written_region(noisy[0])
    for (w, m), (v, n) in zip(a, b):
        assert np.array_equal(w.Y[:rows, :cols], v.Y[:rows, :cols]) and np.array_equal(w.UV[:crows, :cols], v.UV[:crows, :cols])
        assert np.array_equal(m, n)


def test_the_synthetic_program_is_a_one_pattern_model():
    assert X.one_pattern_model(G.records_of(G.P8_422)) and T.trace_geometry(G.records_of(G.P8_422)) == (8, 2, 1)
    for name in G.NAMES.values():
        assert X.one_pattern_model(G.records_of(name)), name


@pytest.mark.parametrize("key", G.CASE_KEYS, ids=lambda k: "-".join(str(x) for x in k[:4]))
def test_every_gpu_input_stays_within_its_exclusion_cap(key):
    c = G.case(key)
    res, excluded = M.expected(oracle(c["rec"]), c["rec"], c["frames"], c["seeds"], c["shift"], c["mixes"])
    total = M.chroma_samples(c["frames"])
    print(f"{key}: excluded {excluded} of {total}, cap {c['cap']}")
    assert excluded <= c["cap"], (key, excluded, total)
    if key[0] == "clamp":
        # samples where the clamp of the index acts stay in the comparison (test_gpu_semiplanar_mix.py CLAMP_NAMES)
        assert X.one_pattern_model(c["rec"]) and not X.legal_range(c["rec"])
        sat, compared = M.saturated_samples(c["frames"], c["mixes"], [m for _, m in res])
        print(f"saturated index samples: {sat}, of them compared: {compared}")
        assert sat > 0 and compared >= sat // 8, (sat, compared)
