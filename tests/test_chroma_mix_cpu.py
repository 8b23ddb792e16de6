"""CPU: the host side of the luma / chroma mix of the chroma look-up index (include/vfgs_hip.h: vfgs_hip_set_chroma_mix,
include/vfgs_hip_fw.h: vfgs_hip_afgs1_chroma_mix) -- exports, range checks, reset, the firmware switch and its environment
variable, configuration files -- and the derivation the GPU tests take their expected pictures from (tests/chroma_mix_util.py),
validated against the oracle and, where oracle/_ref was built, the real reference hardware layer.
"""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import chroma_mix_util as X
import vfgs_testlib as T

import versatilefilmgrain_amd.build as B
from versatilefilmgrain_amd import fw, hw


@pytest.fixture(scope="module")
def hip():
    B.build()
    h = hw.VfgsHip()
    yield h
    fw.afgs1_chroma_mix(False)
    h.lib.vfgs_hip_reset_state()


def checkers():
    return [T.OracleHW] + ([T.ReferenceHW] if T.have_reference() else [])


def test_exports_and_power_on_state(hip):
    for name in ("vfgs_hip_set_chroma_mix", "vfgs_hip_clear_chroma_mix", "vfgs_hip_get_chroma_mix", "vfgs_hip_afgs1_chroma_mix"):
        assert hasattr(hip.lib, name) and name in hw.EXPORTS + fw.EXPORTS
    hip.lib.vfgs_hip_reset_state()
    assert hip.chroma_mix(1) == (0, 0, 0, 0) and hip.chroma_mix(2) == (0, 0, 0, 0)


def test_setter_range_checks_change_nothing(hip):
    hip.lib.vfgs_hip_reset_state()
    hip.set_chroma_mix(1, -128, 127, -256)
    hip.set_chroma_mix(2, 127, -128, 255)
    assert hip.chroma_mix(1) == (-128, 127, -256, 1) and hip.chroma_mix(2) == (127, -128, 255, 1)
    for bad in ((0, 1, 1, 1), (3, 1, 1, 1), (1, 128, 0, 0), (1, -129, 0, 0), (2, 0, 128, 0), (2, 0, -129, 0), (1, 0, 0, 256), (1, 0, 0, -257)):
        assert hip.lib.vfgs_hip_set_chroma_mix(*bad) == 37 and hip.lib.vfgs_hip_last_error() == 37
    assert hip.lib.vfgs_hip_get_chroma_mix(0, (C.c_int * 4)()) == 37 and hip.lib.vfgs_hip_get_chroma_mix(1, None) == 37
    assert hip.chroma_mix(1) == (-128, 127, -256, 1) and hip.chroma_mix(2) == (127, -128, 255, 1)
    hip.clear_chroma_mix()
    assert hip.chroma_mix(1) == (0, 0, 0, 0) and hip.chroma_mix(2) == (0, 0, 0, 0)
    hip.set_chroma_mix(2, 1, 2, 3)
    hip.lib.vfgs_hip_reset_state()
    assert hip.chroma_mix(2) == (0, 0, 0, 0)


def test_the_mix_moves_neither_the_seed_registers_nor_the_other_state(hip):
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, T.load_trace("fgs_afgs1_test1_10_420"))
    before = hip.seed_state(), hip.params(), hip.luts(1), hip.luts(2)
    hip.set_chroma_mix(1, 32, 32, 0)
    hip.clear_chroma_mix()
    assert (hip.seed_state(), hip.params(), hip.luts(1), hip.luts(2)) == before


def afgs1_of(name):
    _, cfgs = T.load_fwcfg(name)
    return [fw.struct_from_bytes(k, raw) for k, raw in cfgs if k == 1][0]


def test_firmware_switch_programs_the_mix_of_the_corpus(hip):
    """fgs_afgs1_test1 carries 247 / 192 / 18 and 229 / 192 / 54, test2 AV1's defaults 128 / 192 / 256 ("index by luma")"""
    t1, t2 = afgs1_of("fgs_afgs1_test1_10_420"), afgs1_of("fgs_afgs1_test2_10_420")
    assert (t1.cb_mult, t1.cb_luma_mult, t1.cb_offset, t1.cr_mult, t1.cr_luma_mult, t1.cr_offset) == (247, 192, 18, 229, 192, 54)
    assert (t2.cb_mult, t2.cb_luma_mult, t2.cb_offset, t2.cr_mult, t2.cr_luma_mult, t2.cr_offset) == (128, 192, 256, 128, 192, 256)
    hip.lib.vfgs_hip_reset_state()
    try:
        fw.afgs1_chroma_mix(False)
        fw.init_afgs1(t1)
        off_state = hip.seed_state(), hip.params(), [hip.luts(c) for c in range(3)]
        assert hip.chroma_mix(1)[3] == 0 and hip.chroma_mix(2)[3] == 0
        fw.afgs1_chroma_mix(True)
        fw.init_afgs1(t1)
        assert (hip.chroma_mix(1), hip.chroma_mix(2)) == ((64, 119, -238, 1), (64, 101, -202, 1))
        assert (hip.seed_state(), hip.params(), [hip.luts(c) for c in range(3)]) == off_state      # nothing else differs
        fw.init_afgs1(t2)
        assert (hip.chroma_mix(1), hip.chroma_mix(2)) == ((64, 0, 0, 1), (64, 0, 0, 1))
        t1.chroma_scaling_from_luma = 1
        fw.init_afgs1(t1)
        assert (hip.chroma_mix(1), hip.chroma_mix(2)) == ((64, 0, 0, 1), (64, 0, 0, 1))
        # an SEI model clears it; so does AFGS1 with the switch off
        _, cfgs = T.load_fwcfg("fgs_afgs1_test1_10_420")
        fw.init(fw.struct_from_bytes(*cfgs[0]))
        assert hip.chroma_mix(1)[3] == 0 and hip.chroma_mix(2)[3] == 0
        fw.init_afgs1(t2)
        fw.afgs1_chroma_mix(False)
        fw.init_afgs1(t2)
        assert hip.chroma_mix(1)[3] == 0 and hip.chroma_mix(2)[3] == 0
    finally:
        fw.afgs1_chroma_mix(False)


@pytest.mark.parametrize("env, want", [("1", 1), ("0", 0), (None, 0)])
def test_switch_from_the_environment(hip, env, want):
    """a process that never calls vfgs_hip_afgs1_chroma_mix takes VFGS_HIP_AFGS1_CHROMA_MIX=1 (the unchanged reference CLI)"""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import vfgs_testlib as T
from versatilefilmgrain_amd import fw, hw
h = hw.VfgsHip()
_, cfgs = T.load_fwcfg("fgs_afgs1_test1_10_420")
fw.init_afgs1([fw.struct_from_bytes(k, raw) for k, raw in cfgs if k == 1][0])
print("MIX", h.chroma_mix(1), h.chroma_mix(2))
fw.afgs1_chroma_mix(False)
fw.init_afgs1([fw.struct_from_bytes(k, raw) for k, raw in cfgs if k == 1][0])
print("OFF", h.chroma_mix(1)[3])
""" % (str(T.ROOT), str(T.ROOT / "tests"))
    import os
    e = {k: v for k, v in os.environ.items() if k != "VFGS_HIP_AFGS1_CHROMA_MIX"}
    if env is not None:
        e["VFGS_HIP_AFGS1_CHROMA_MIX"] = env
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("MIX (64, 119, -238, 1) (64, 101, -202, 1)" in r.stdout) == bool(want), r.stdout
    assert "OFF 0" in r.stdout      # the call overrides the environment


def test_cfg_files_give_identical_structures_with_the_switch_on_or_off(hip, tmp_path):
    with np.load(T.GOLDEN / "cfg_corpus.npz") as z:
        files = {name: z[name].tobytes() for name in z.files}
    out = {}
    try:
        for on in (False, True):
            fw.afgs1_chroma_mix(on)
            for name, data in sorted(files.items()):
                p = tmp_path / name
                p.write_bytes(data)
                st = fw.Cfg.defaults()
                rc = st.read(p)
                out[(on, name)] = rc, C.string_at(C.addressof(st), C.sizeof(st))
    finally:
        fw.afgs1_chroma_mix(False)
    assert len(files) >= 26
    for name in files:
        assert out[(False, name)] == out[(True, name)], name


# ---- the derivation of the expected pictures ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", X.SIX_TRACES)
def test_neutral_mix_derivation_equals_the_plain_output(name):
    """(0, 64, 0): m = the sample, so the derived expectation must be what the checker writes for the plain frame (in-range content)"""
    rec = T.load_trace(name)
    depth, sx, sy = T.trace_geometry(rec)
    frames = X.ranged_frames(346, 112, depth, sx, sy, 2, 2, lo=0.25, hi=0.75)
    for make in checkers():
        res, excluded, ck = X.expected_frames(make, rec, frames, (X.NEUTRAL, X.NEUTRAL))
        plain = make()
        T.replay(plain, rec)
        assert excluded == 0
        for f, (want, masks) in zip(frames, res):
            g = f.copy()
            plain.add_grain_frame(g)
            assert g.equal_all(want) and all(m.all() for m in masks)
        if isinstance(ck, T.OracleHW):
            assert ck.seed_state() == plain.seed_state()


@pytest.mark.parametrize("mix", [(32, 32, 0), (64, 0, 0)], ids=str)
@pytest.mark.parametrize("name", X.SIX_TRACES)
def test_nothing_is_excluded_on_mid_range_content(name, mix):
    """the condition under which the exact GPU tests compare every sample: planes uniform in [0.3, 0.7) x 2^d at 320x192"""
    rec = T.load_trace(name)
    depth, sx, sy = T.trace_geometry(rec)
    frames = X.ranged_frames(320, 192, depth, sx, sy, 2, 1)
    for make in checkers():
        res, excluded, _ = X.expected_frames(make, rec, frames, (mix, mix))
        assert excluded == 0
        # and the mix is not a no-op: the expectation differs from the plain output
        plain = make()
        T.replay(plain, rec)
        differ = 0
        for f, (want, _m) in zip(frames, res):
            g = f.copy()
            plain.add_grain_frame(g)
            assert np.array_equal(g.Y, want.Y)
            differ += int((g.U != want.U).sum() + (g.V != want.V).sum())
        assert differ > 0


def test_oracle_and_reference_give_the_same_expectation():
    if not T.have_reference():
        return      # (nothing to compare where oracle/_ref was not built; the oracle itself is checked against the stored reference digests elsewhere)
    rec = T.load_trace("fgs_afgs1_test1_10_420")
    frames = X.ranged_frames(346, 112, 10, 2, 2, 2, 3, lo=0.4, hi=0.6, clo=0.4, chi=0.5)
    a, ea, _ = X.expected_frames(T.OracleHW, rec, frames, ((64, 119, -238), (64, 101, -202)))
    b, eb, _ = X.expected_frames(T.ReferenceHW, rec, frames, ((64, 119, -238), (64, 101, -202)))
    assert ea == eb == 0 and all(x[0].equal_all(y[0]) for x, y in zip(a, b))


def test_mix_definition_on_a_hand_made_row():
    """the definition itself, spelled out on a few samples: pair average with the last luma sample paired with itself, >> 6 as an
    arithmetic shift, the offset in 8-bit code values, the clip"""
    f = T.Frame(160, 16, 10, 2, 2)
    f.Y[0, :8] = [100, 101, 1023, 1023, 0, 0, 7, 8]
    f.Y[0, 158:160] = [500, 900]
    f.U[0, :4] = [100, 0, 1023, 64]
    f.U[0, 79] = 10
    m = X.mix_plane(f.Y, f.U, 159, 10, 2, 2, (64, -32, -3))      # width 159: sample 158 is the last one
    # avgL: (100 + 101 + 1) >> 1 = 101; 1023; 0; (7 + 8 + 1) >> 1 = 8;   column 79: (500 + 500 + 1) >> 1 = 500
    # (101 * 64 - 100 * 32) >> 6 = 51; 1023; (0 - 1023 * 32) >> 6 = -512; (8 * 64 - 64 * 32) >> 6 = -24;   offset -3 code values = -12
    assert list(m[0, :4]) == [39, 1011, 0, 0]
    assert m[0, 79] == ((500 * 64 - 10 * 32) >> 6) - 12 == 483
    assert ((-1) >> 6) == -1      # arithmetic shift, as the definition wants
    m8 = X.mix_plane(np.array([[250, 250]], np.uint8), np.array([[250, 3]], np.uint8), 2, 8, 1, 1, (127, 127, 255))
    assert list(m8[0]) == [255, 255]
