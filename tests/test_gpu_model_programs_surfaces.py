"""GPU (MI355X): the generated programs of tests/model_programs.py through the surface kernels -- grain_sp_kernel, grain_sp_mix_kernel,
grain_sp8_kernel, grain_p2sp_kernel, grain_p2sp8_kernel -- byte for byte against the oracle, through the C ABI.

tests/test_gpu_model_programs.py runs these programs through the planar entry points only.  The surface kernels stage their tables on their
own and place Cb and Cr on their own: a UV workgroup runs the grain once with Cb's parameters and tables and once with Cr's.  Cb and Cr on
different uniform slots, one of them on slot 8 beside a live one, a -128 in Cr's slot only, one chroma component one over the packed 16-bit
limit at 8 bit: taking Cb's table for Cr, or mis-addressing the second sub-image, shows exactly there.

Which program goes through which call, at which alignment and with which content, is tests/model_program_cases.py's decision;
tests/test_model_program_cases_cpu.py checks on the oracle alone that the table covers what it has to and that a Cb / Cr mix-up would be
visible in every in-place case.  The ground truth is the existing helpers' (semiplanar_util, semiplanar_out8_util, planar_to_sp_util,
semiplanar_mix_util): no arithmetic is added here.  Every case compares every container of both planes of every frame, padding included, the
sources of the out-of-place calls (unchanged), the destination's fill outside the written region, and the four seed registers; and asserts
from last_launch_info() the form against MP.expected_form, the depth, the kernel's name and the number of launches -- a case that silently
ran another form would prove nothing.  (One launch a case; in place under a mix the call is two launches, UV rows first, as
tests/test_gpu_semiplanar_mix.py has it.)
"""
import numpy as np
import pytest

import model_program_cases as C
import model_programs as MP
import planar_to_sp_util as P2
import semiplanar_mix_util as M
import semiplanar_out8_util as SP8
import semiplanar_util as SP
import vfgs_testlib as T
from gpu_util import stream_ptr
from test_gpu_planar_to_sp import destinations, scattered as planar_scattered
from test_gpu_semiplanar import assert_equal, launches, scattered

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = 40


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.clear_chroma_mix()
    h.lib.vfgs_hip_reset_state()


def program(hip, rec):
    """-> an oracle in the same programmed state"""
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, rec)
    return C.oracle_for(rec)


def check_launch(hip, rec, kernel, n0, nframes, in_place, out8, nlaunches=1):
    info = hip.last_launch_info()
    depth, sx, sy = T.trace_geometry(rec)
    form = MP.expected_form(rec)
    assert (bool(info["one_y"]), bool(info["one_c"])) == form, (info["kernel"], form)
    assert info["depth"] == depth and (info["csubx"], info["csuby"]) == (sx, sy), info
    one = lambda v: "true" if v else "false"
    args = f"{depth},{sy}" if kernel == "grain_sp_mix_kernel" else f"{depth},{sy},{one(form[0])},{one(form[1])}"
    assert info["kernel"] == f"{kernel}<{args}>", info
    assert info["launches"] - n0 == nlaunches and info["nframes"] == nframes and info["listed"] == 1, info
    assert info["in_place"] == in_place and info["out8"] == out8, info
    return info


# ---- every program, semi-planar, in place ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.in_place_cases(), ids=C.case_id)
def test_every_program_semi_planar_in_place(hip, case):
    """two frames, one seed sequence; depth 10 / 12 at shift 0 and high-aligned in turn (random low bits in the sources, which the call
    ignores and clears)"""
    rec = MP.program(case.name)
    depth = MP.parse(case.name)[1]
    frames = C.sp_frames(case)
    f0 = frames[0]
    if case.shift:
        assert any((f.Y & ((1 << case.shift) - 1)).any() and (f.UV & ((1 << case.shift) - 1)).any() for f in frames)
    ora = program(hip, rec)
    want = SP.expected(ora, frames, None, case.shift)
    dev = scattered(frames, 1)
    n0 = launches(hip)
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, None, f0.width, f0.height, f0.stride, f0.uv_stride, case.shift, stream_ptr())
    for i, (d, w) in enumerate(zip(dev, want)):
        assert_equal(d.download(), w, f"frame {i}")
    assert hip.seed_state() == ora.seed_state()
    check_launch(hip, rec, "grain_sp_kernel", n0, len(frames), 1, 0)
    assert (f0.width, f0.height) == (C.width_of(depth), C.H)


# ---- every class through the other four calls ------------------------------------------------------------------------------------

def run_sp_seeded(hip, ora, case, rec):
    frames = C.sp_frames(case)
    f0 = frames[0]
    want = SP.expected(ora, frames, case.seeds, case.shift)
    dev = scattered(frames, 2)
    n0 = launches(hip)
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, case.seeds, f0.width, f0.height, f0.stride, f0.uv_stride, case.shift, stream_ptr())
    for i, (d, w) in enumerate(zip(dev, want)):
        assert_equal(d.download(), w, f"frame {i}")
    assert hip.seeded_stream_stats()["last_launch_used_it"]
    return check_launch(hip, rec, "grain_sp_kernel", n0, len(frames), 1, 0)


def run_out_of_place(hip, ora, case, rec):
    """sp_copy8, to_sp, to_sp8: into pre-filled destinations; whatever the call does not write keeps the fill, the sources stay"""
    depth, _sx, sy = T.trace_geometry(rec)
    planar = case.path in C.PLANAR_SOURCE
    out8 = case.path in C.NARROWED
    frames = C.planar_frames(case) if planar else C.sp_frames(case)
    f0 = frames[0]
    if out8:
        fill = SP8.dst_frame(f0.width, f0.height, sy, 4321, case.pad, case.uv_pad)
    else:
        fill = P2.dst_frame(f0.width, f0.height, depth, sy, case.shift, 4321, case.pad, case.uv_pad)
    if case.path == "sp_copy8":
        want = SP8.expected8(ora, frames, None, case.shift, fill)
    elif case.path == "to_sp":
        want = P2.expected(ora, frames, None, case.shift, fill)
    else:
        want = P2.expected8(ora, frames, None, fill)
    src = (planar_scattered if planar else scattered)(frames, 3)
    dst = destinations(len(frames), fill, 3)
    s, d = [x.ptrs() for x in src], [x.ptrs() for x in dst]
    n0 = launches(hip)
    st = stream_ptr()
    if case.path == "sp_copy8":
        hip.add_grain_sp_frame_list_copy8_dev(s, d, None, f0.width, f0.height, f0.stride, f0.uv_stride, fill.stride, fill.uv_stride, case.shift, st)
    elif case.path == "to_sp":
        hip.add_grain_frame_list_to_sp_dev(s, d, None, f0.width, f0.height, f0.stride, f0.cstride, fill.stride, fill.uv_stride, case.shift, st)
    else:
        hip.add_grain_frame_list_to_sp8_dev(s, d, None, f0.width, f0.height, f0.stride, f0.cstride, fill.stride, fill.uv_stride, st)
    for i, (a, b, f, w) in enumerate(zip(src, dst, frames, want)):
        assert_equal(b.download(), w, f"destination {i}")          # what is written, and every other byte as it was
        assert a.download().equal_all(f), f"source {i} changed"
    kernel = {"sp_copy8": "grain_sp8_kernel", "to_sp": "grain_p2sp_kernel", "to_sp8": "grain_p2sp8_kernel"}[case.path]
    return check_launch(hip, rec, kernel, n0, len(frames), 0, 1 if out8 else 0)


@pytest.mark.parametrize("case", C.path_cases(), ids=C.case_id)
def test_every_class_through_the_other_calls(hip, case):
    rec = MP.program(case.name)
    ora = program(hip, rec)
    (run_sp_seeded if case.path == "sp_seeded" else run_out_of_place)(hip, ora, case, rec)
    assert hip.seed_state() == ora.seed_state()


# ---- under the luma / chroma mix -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.mix_cases(), ids=C.case_id)
def test_one_pattern_programs_under_the_mix(hip, case):
    """in place (two launches: UV rows first); compared through the masks of the derivation, whose share of left-out samples is asserted on
    the oracle by tests/test_model_program_cases_cpu.py and printed here"""
    rec = MP.program(case.name)
    mixes = C.MIXES[case.mix]
    frames = C.sp_frames(case)
    f0 = frames[0]
    ora = program(hip, rec)
    res, excluded = M.expected(ora, rec, frames, None, case.shift, mixes)
    rows, crows, cols = SP.written_region(f0)
    share = excluded / (len(frames) * crows * cols)
    print(f"{C.case_id(case)}: {share:.4f} of the processed chroma samples left out by the derivation")
    assert share <= C.MIX_CAPS[case.mix]
    dev = scattered(frames, 4)
    try:
        for c, m in enumerate(mixes, 1):
            if m is not None:
                hip.set_chroma_mix(c, *m)
        n0 = launches(hip)
        hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, None, f0.width, f0.height, f0.stride, f0.uv_stride, case.shift, stream_ptr())
        check_launch(hip, rec, "grain_sp_mix_kernel", n0, len(frames), 1, 0, nlaunches=2)
    finally:
        hip.clear_chroma_mix()
    assert hip.chroma_mix(1)[3] == 0 and hip.chroma_mix(2)[3] == 0
    for i, (d, (w, mask)) in enumerate(zip(dev, res)):
        n = M.mismatches(d.download(), w, mask)
        assert n == 0, f"frame {i}: {n} containers differ from the expectation"
    assert hip.seed_state() == ora.seed_state()


@pytest.mark.parametrize("name", C.REFUSED_UNDER_A_MIX)
def test_chroma_mix_is_refused_for_a_general_form(hip, name):
    """the semi-planar call's own code; frames, registers and the launch count stay (test_gpu_model_programs.py has the planar calls')"""
    import torch
    from versatilefilmgrain_amd.hw import VfgsHipError
    rec = MP.program(name)
    assert MP.expected_form(rec) != (True, True)
    depth = MP.parse(name)[1]
    case = C.Case("sp", name, 0, "in_range", 1, None, 0, 0, "cb_only")
    frames = C.sp_frames(case)
    f0 = frames[0]
    program(hip, rec)
    dev = scattered(frames)
    hip.set_chroma_mix(1, *C.MIXES["cb_only"][0])
    try:
        seeds, n0 = hip.seed_state(), launches(hip)
        with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}:.*chroma mix.*general-form"):
            hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, None, f0.width, f0.height, f0.stride, f0.uv_stride, 0, stream_ptr())
        assert hip.lib.vfgs_hip_last_error() == E_UNSUPPORTED
        torch.cuda.synchronize()
        assert hip.seed_state() == seeds and launches(hip) == n0
        for d, f in zip(dev, frames):
            assert_equal(d.download(), f)
    finally:
        hip.clear_chroma_mix()
    assert (f0.width, f0.height) == (C.width_of(depth), C.H)
