"""CPU: oracle/vfgs_fw_oracle.py (numpy restatement of the reference's pattern generators) against
the pattern bytes the real reference firmware programmed (tests/golden/traces) on six traces, and the
same three comparisons with the C restatement's generator (oracle/vfgs_fw_oracle.c, fw_oracle_util.job_pattern)
on every trace of each kind."""
import sys

import numpy as np
import pytest

import fw_oracle_util as O
import fw_space as S
import vfgs_testlib as T

sys.path.insert(0, str(T.ROOT / "oracle"))
import vfgs_fw_oracle as F  # noqa: E402

from versatilefilmgrain_amd import fw  # noqa: E402


def programmed(name):
    want = T.BankModel()
    T.replay(want, T.load_trace(name))
    _, cfgs = T.load_fwcfg(name)
    return want, fw.struct_from_bytes(*cfgs[-1])


@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_sei_ff_test6_10_420", "default_8_420"])
def test_frequency_filtered_patterns(name):
    want, sei = programmed(name)
    # interval 0 of a component with ascending bounds is pattern 0 of its bank (vfgs_fw.c:552-568)
    v = sei.comp_model_value[0][0]
    assert np.array_equal(F.ff_pattern(64, v[1], v[2], 0), want.luma[0])
    if sei.comp_model_present_flag[1]:
        v = sei.comp_model_value[1][0]
        assert np.array_equal(F.ff_pattern(32, v[1], v[2], 1), want.chroma[0][:32, :32])


def test_sei_auto_regressive_pattern():
    want, sei = programmed("fgs_sei_ar_test1_10_420")
    v = list(sei.comp_model_value[0][0])
    taps = F.sei_ar_taps(v, sei.log2_scale_factor)
    assert np.array_equal(F.ar_pattern(False, taps, sei.log2_scale_factor, 1, 0), want.luma[0])


@pytest.mark.parametrize("name", ["fgs_afgs1_test1_10_420", "fgs_afgs1_test3_8_420"])
def test_afgs1_patterns(name):
    want, a = programmed(name)
    lag, scale, shift = a.ar_coeff_lag, a.ar_coeff_shift, a.grain_scale_shift + 1
    assert np.array_equal(F.ar_pattern(False, F.afgs1_taps(list(a.ar_coeffs_y), lag), scale, shift, 0), want.luma[0])
    assert np.array_equal(F.ar_pattern(True, F.afgs1_taps(list(a.ar_coeffs_cb), lag), scale, shift, 1), want.chroma[0][:32, :32])
    assert np.array_equal(F.ar_pattern(True, F.afgs1_taps(list(a.ar_coeffs_cr), lag), scale, shift, 2), want.chroma[1][:32, :32])


# ---- the same with the C generator, on every trace of each kind ------------------------------------------------------------------------

def _kind(name):
    k, raw = T.load_fwcfg(name)[1][-1]
    return "afgs1" if k else ("ar" if fw.struct_from_bytes(k, raw).model_id else "ff")


NAMES = sorted(p.stem for p in T.FWCFG.glob("*.npz"))
BY_KIND = {k: [n for n in NAMES if _kind(n) == k] for k in ("ff", "ar", "afgs1")}


def test_every_trace_has_a_kind():
    assert sum(len(v) for v in BY_KIND.values()) == len(NAMES) and all(BY_KIND.values())


def programmed_state(name):
    """-> the tables the trace leaves, the pattern payloads as the reference handed them over {(bank, slot): 4096 bytes}, the structure"""
    want = T.StateModel()
    T.replay(want, T.load_trace(name))
    return want, O.patterns_of(T.load_trace(name)), fw.struct_from_bytes(*T.load_fwcfg(name)[1][-1])


def _sei_patterns(name, job_of):
    """every interval of every present component against the slot the recorded pattern LUT names for its lower bound"""
    want, payloads, sei = programmed_state(name)
    done = 0
    for c in range(3):
        if not sei.comp_model_present_flag[c]:
            continue
        for k in range(sei.num_intensity_intervals[c]):
            lo, hi = sei.intensity_interval_lower_bound[c][k], sei.intensity_interval_upper_bound[c][k]
            if hi < lo:
                continue
            slot = want.plut[c][lo] >> 4
            v = [int(x) for x in sei.comp_model_value[c][k]]
            got = O.job_pattern(job_of(sei, c, v))
            assert got == payloads[(1 if c else 0, slot)][:len(got)], (name, c, k, slot)
            done += 1
    assert done


@pytest.mark.parametrize("name", BY_KIND["ff"])
def test_frequency_filtered_patterns_c(name):
    _sei_patterns(name, lambda sei, c, v: S._job(0, c > 0, 1 if c else 0, v[1], v[2]))


@pytest.mark.parametrize("name", BY_KIND["ar"])
def test_sei_auto_regressive_patterns_c(name):
    _sei_patterns(name, lambda sei, c, v: S._job(1, c > 0, 1 if c else 0, scale=sei.log2_scale_factor, shift=1,
                                                 taps=F.sei_ar_taps(v, sei.log2_scale_factor)))


@pytest.mark.parametrize("name", BY_KIND["afgs1"])
def test_afgs1_patterns_c(name):
    _, payloads, a = programmed_state(name)
    lag, scale, shift = a.ar_coeff_lag, a.ar_coeff_shift, a.grain_scale_shift + 1
    for bank, slot, ar, seed in ((0, 0, a.ar_coeffs_y, 0), (1, 0, a.ar_coeffs_cb, 1), (1, 1, a.ar_coeffs_cr, 2)):
        got = O.job_pattern(S._job(1, bank, seed, scale=scale, shift=shift, taps=F.afgs1_taps(list(ar), lag)))
        assert got == payloads[(bank, slot)][:len(got)], (name, slot)
