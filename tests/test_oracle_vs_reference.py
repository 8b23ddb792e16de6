"""CPU: the oracle against the REAL reference hardware layer.

Covers what the md5 fixtures cannot: padding bytes, ragged widths, garbage (out of
range) samples, every chroma format, the seed registers after each call, and the
line API called with arbitrary y.

What the reference wrote for every case below is stored as the md5 of each output frame
(all planes, stride padding included) in tests/golden/reference_hw_md5.json, so these tests
run everywhere.  Where oracle/_ref/libvfgs_ref.so was built (compiled in place from the
reference's vfgs_hw.c), the reference is also run live and must still write what the fixture
holds.  VFGS_WRITE_REFERENCE_MD5=1 (only where oracle/_ref exists) rewrites the fixture from
the live reference; the oracle must agree with it for a case to be written.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import vfgs_testlib as T

FIXTURE = T.GOLDEN / "reference_hw_md5.json"
SUB = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "440": (1, 2)}


def digest(f):
    return hashlib.md5(b"".join(p.tobytes() for p in f.planes())).hexdigest()


def reference_digests(key, run):
    """md5 of every frame the reference writes in case `key`: `run()` -> those frames, on the live reference (oracle/_ref)."""
    stored = json.loads(FIXTURE.read_text()).get(key) if FIXTURE.exists() else None
    if not T.have_reference():
        assert stored is not None, f"{key}: no reference output stored in {FIXTURE.name}"
        return stored
    live = [digest(f) for f in run()]
    if os.environ.get("VFGS_WRITE_REFERENCE_MD5") == "1":
        return live          # (written by check() once the oracle agrees)
    assert stored is not None, f"{key}: no reference output stored in {FIXTURE.name} (VFGS_WRITE_REFERENCE_MD5=1 writes it)"
    assert live == stored, f"{key}: the reference writes other bytes than {FIXTURE.name} holds"
    return stored


def check(key, want, got_frames):
    got = [digest(f) for f in got_frames]
    assert got == want
    if T.have_reference() and os.environ.get("VFGS_WRITE_REFERENCE_MD5") == "1":
        data = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else {}
        data[key] = want
        FIXTURE.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")


def programmed(hw, name):
    rec = T.load_trace(name)
    T.replay(hw, rec)
    return hw, T.trace_geometry(rec)


def run_frames(hw, frames):
    out = []
    for f in frames:
        a = f.copy()
        hw.add_grain_frame(a)
        out.append(a)
    return out


@pytest.mark.parametrize("name", T.list_traces())
def test_every_cfg_full_buffer(name):
    """All planes incl. stride padding, 2 frames, garbage in the padding, W%16 != 0."""
    ora, (depth, sx, sy) = programmed(T.OracleHW(), name)
    frames, _ = T.lcg_frames(200, 150 if sy == 1 else 152, depth, sx, sy, 2, garbage_padding=True)
    want = reference_digests(f"full_buffer/{name}", lambda: run_frames(programmed(T.ReferenceHW(), name)[0], frames))
    check(f"full_buffer/{name}", want, run_frames(ora, frames))
    # closed form on a fresh context, frame by frame
    ora2, _ = programmed(T.OracleHW(), name)
    out = []
    for f in frames:
        c = f.copy()
        ora2.add_grain_frame(c, closed_form=True)
        out.append(c)
    check(f"full_buffer/{name}", want, out)


@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_8_444", "fgs_sei_8_422", "fgs_sei_10_440"])
def test_out_of_range_samples(name):
    """10-bit containers holding up to 16-bit garbage: intensity wraps as a uint8 (quirk 8)."""
    ora, (depth, sx, sy) = programmed(T.OracleHW(), name)
    f = T.Frame(256, 144, depth, sx, sy)
    rng = np.random.default_rng(7)
    for p in f.planes():
        p[...] = rng.integers(0, 1 << (16 if depth > 8 else 8), p.shape).astype(f.dtype)
    want = reference_digests(f"out_of_range/{name}", lambda: run_frames(programmed(T.ReferenceHW(), name)[0], [f]))
    check(f"out_of_range/{name}", want, run_frames(ora, [f]))
    T.replay(ora, T.load_trace(name))  # re-seed
    c = f.copy()
    ora.add_grain_frame(c, closed_form=True)
    check(f"out_of_range/{name}", want, [c])


def test_seed_registers_track_reference_stream():
    """After set_seed the four registers follow the closed-form offsets; checked through output
    of a *following* frame with a different height (state carries across frames, quirk 4)."""
    sizes = ((192, 144), (320, 208), (192, 130))

    def inputs(depth, sx, sy):
        return [T.lcg_frames(w, h, depth, sx, sy, 1, state=w)[0][0] for w, h in sizes]

    def run_ref():
        ref, geo = programmed(T.ReferenceHW(), "fgs_sei_10_420")
        return run_frames(ref, inputs(*geo))
    want = reference_digests("seed_registers", run_ref)
    for closed in (False, True):
        ora, geo = programmed(T.OracleHW(), "fgs_sei_10_420")
        out = []
        for f in inputs(*geo):
            b = f.copy()
            ora.add_grain_frame(b, closed_form=closed)
            out.append(b)
        check("seed_registers", want, out)


def test_line_api_arbitrary_y_order():
    """Lines fed out of order / repeated: the seed state machine must match call for call."""
    order = [0, 1, 16, 17, 5, 32, 32, 33, 48, 2, 64, 65, 80, 15, 16, 96]

    def run(hw):
        hw, (depth, sx, sy) = programmed(hw, "fgs_sei_10_420")
        f, _ = T.lcg_frames(192, 144, depth, sx, sy, 1)
        fr = f[0].copy()
        for y in order:
            hw.add_grain_line(fr.Y[y].ctypes.data, fr.U[y // 2].ctypes.data, fr.V[y // 2].ctypes.data, y, fr.width)
        return [fr]
    want = reference_digests("line_api_order", lambda: run(T.ReferenceHW()))
    check("line_api_order", want, run(T.OracleHW()))


def test_default_power_on_state():
    """No programming at all: 0xdeadbeef seeds, zero banks/LUTs -> only the clip acts."""
    f, _ = T.lcg_frames(192, 144, 10, 2, 2, 1)

    def run(hw):
        hw.set_depth(10)
        return run_frames(hw, f)
    want = reference_digests("power_on", lambda: run(T.ReferenceHW()))
    out = run(T.OracleHW())
    check("power_on", want, out)
    assert out[0].Y.max() <= 1020  # quirk 1: 255<<2


def test_lfsr_stream_word_recurrence():
    lib = T.oracle_lib()
    for reg in (0xdeadbeef, 12345 << 1, 1 << 31, 0xFFFFFFFF, 2):
        n = 4096
        words = np.zeros(n, np.uint32)
        lib.vfgs_oracle_lfsr_stream(reg, words.ctypes.data, n)
        # bit-serial check of windows at many offsets
        r = reg
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        for target in range(0, 70000):
            if target % 4999 == 0:
                win = int(np.packbits(bits[target:target + 32], bitorder="little").view(np.uint32)[0])
                assert win == r, (hex(reg), target)
            r = lib.vfgs_oracle_lfsr_step(r)
