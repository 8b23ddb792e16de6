"""GPU (MI355X): vfgs_hip_add_grain_sp_frame_list_models_copy8_dev -- P010 / P210 / P012 (or low-aligned containers) in, NV12 / NV16 out, a
model per picture in one launch -- against the oracle, through the C ABI, bit for bit: every byte of both destination planes of every
frame, padding included, every container of the sources (unchanged), and the four seed registers.

The contract (include/vfgs_hip.h) is the loop of the calls with models around the one-frame vfgs_hip_add_grain_sp_frame_list_copy8_dev; the
expectation is semiplanar_out8_util.expected8 per frame by an oracle that holds that frame's model (tests/model_out8_util.py, whose case
tables tests/test_model_out8_cases_cpu.py runs on the oracle alone).  The launches are grain_sp8_kernel's.  Frames are separate
allocations listed out of address order; sources hold garbage over the whole container (with a shift: random low bits), destinations are
pre-filled with garbage and have pitches that exceed the rows and differ between Y and UV."""
import ctypes as C

import numpy as np
import pytest

import model_list_util as U
import model_out8_util as M8
import semiplanar_out8_util as SP8
import vfgs_testlib as T
from gpu_util import stream_ptr
from test_gpu_semiplanar import DevSP, assert_equal, mk, scattered
from test_gpu_semiplanar_out8 import check8, destinations
from test_gpu_sp_model_list import Models

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


def call(hip, src, dst, models, seeds, f0, fill, shift=None, stream=None):
    hip.add_grain_sp_frame_list_models_copy8_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], models, seeds, f0.width, f0.height, f0.stride, f0.uv_stride,
                                                 fill.stride, fill.uv_stride, f0.shift if shift is None else shift, stream_ptr() if stream is None else stream)


def run(hip, ms, pick, frames, seeds=None, ora=None, shuffle=0, pad=16, uv_pad=48):
    f0 = frames[0]
    fill = SP8.dst_frame(f0.width, f0.height, f0.suby, 4321 + shuffle, pad, uv_pad)
    want, regs, ora = M8.expect_sp(ms.recs, pick, frames, seeds, fill, ora)
    src, dst = scattered(frames, shuffle), destinations(frames, fill, shuffle)
    call(hip, src, dst, [ms.handles[k] for k in pick], seeds, f0, fill)
    check8(src, dst, frames, want)
    assert hip.seed_state() == regs
    return src, dst, ora


def kernel_of(ms, k):
    return T.kernel_name("grain_sp8_kernel", ms.depth, ms.sy, *ms.forms[k])


# ---- surfaces, sizes, A B A C B ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("size", M8.SP_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("surface", sorted(M8.SP_CONFIGS))
def test_surfaces(hip, surface, size, seeded):
    """P010 (shift 6, random low bits), P210, P012 (shift 4) and low-aligned containers; a ragged 1047 x 40 and 1032 x 90; models A B A C B
    with C of another form: a launch per run"""
    names, pick, (w, h), fseed = M8.SP_CASES["%s_%dx%d" % ((surface,) + size)]
    shift = M8.SP_CONFIGS[surface][1]
    ms = Models(hip, names)
    try:
        assert ms.forms[2] != ms.forms[0] and shift in (0, 16 - ms.depth)
        frames = mk(len(pick), w, h, ms.depth, ms.sy, shift, fseed)
        assert shift == 0 or all((f.Y & ((1 << shift) - 1)).any() and (f.UV & ((1 << shift) - 1)).any() for f in frames)
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, M8.fresh_seeds(len(pick), 1) if seeded else None, shuffle=1)
        info = hip.last_launch_info()
        runs = U.runs_of(ms.forms, pick)
        assert len(runs) >= 3 and info["launches"] - n0 == len(runs) and info["nframes"] == runs[-1], (info, runs)
        assert info["listed"] == 1 and info["out8"] == 1 and info["in_place"] == 0 and info["persistent_luma_workgroups"] == 0 and info["depth"] == ms.depth, info
        assert info["kernel"] == kernel_of(ms, pick[-1]) and info["lds_bytes_per_workgroup"] == 40960, info
    finally:
        ms.release()


def test_bounds_and_shift_are_the_frames_own(hip):
    """two models of one form that differ in range, scale shift and scale LUTs, B A A B A B B in ONE launch: a workgroup -- luma or UV, whose
    16-byte store holds Cb and Cr clipped with the same pair of bounds -- that took the launch's record would be wrong on the other model's
    frames; the oracle alone says that the two models differ in both planes on these frames"""
    from test_gpu_sp_model_list import second_model
    rec = U.model_records("fgs_afgs1_test1_10_420")
    ms = Models(hip, [rec, second_model(rec)])
    try:
        assert ms.forms[0] == ms.forms[1] and ms.info[0]["legal_range"] != ms.info[1]["legal_range"], ms.info
        pick = [1, 0, 0, 1, 0, 1, 1]
        frames = mk(len(pick), 1032, 90, 10, 2, 6, 30)
        fill = SP8.dst_frame(1032, 90, 2, 5)
        a, _, _ = M8.expect_sp(ms.recs, [0], frames[:1], [5], fill)
        b, _, _ = M8.expect_sp(ms.recs, [1], frames[:1], [5], fill)
        cb, cr = (lambda x: x.UV[:, 0::2]), (lambda x: x.UV[:, 1::2])
        assert not np.array_equal(a[0].Y, b[0].Y) and not np.array_equal(cb(a[0]), cb(b[0])) and not np.array_equal(cr(a[0]), cr(b[0]))
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, None, shuffle=2)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 1 and info["nframes"] == len(pick) and info["kernel"] == kernel_of(ms, 0), info
    finally:
        ms.release()


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_more_frames_than_one_launch_holds(hip, seeded):
    """34 frames of 136 x 33, two models of one form alternating: launches of 32 + 2"""
    names, pick, (w, h), fseed = M8.SP_CASES["34_frames"]
    ms = Models(hip, names)
    try:
        n0 = U.launches(hip)
        run(hip, ms, pick, mk(len(pick), w, h, ms.depth, ms.sy, 6, fseed), M8.fresh_seeds(len(pick), 4) if seeded else None, shuffle=4)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 2 and info["nframes"] == 2 and info["out8"] == 1, info
    finally:
        ms.release()


def test_two_frame_fronts(hip):
    """three P010 frames of 8192 x 1366 (tests/test_gpu_semiplanar_out8.py::test_two_frame_fronts), models A B A: frames 2m and 2m + 1 are
    swept together, each with its own model"""
    names, pick, (w, h), fseed = M8.SP_CASES["two_fronts"]
    ms = Models(hip, names)
    try:
        run(hip, ms, pick, mk(len(pick), w, h, ms.depth, ms.sy, 6, fseed), None, shuffle=5, pad=0, uv_pad=16)
        info = hip.last_launch_info()
        assert info["frames_per_front"] == 2 and info["nframes"] == 3 and info["out8"] == 1, info
    finally:
        ms.release()


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_the_call_equals_its_definition_on_the_gpu(hip, seeded):
    """per frame: program, set_seed, the one-frame semi-planar _copy8 list -- identical planes and registers"""
    names, pick, (w, h), fseed = M8.SP_CASES["definition"]
    ms = Models(hip, names)
    try:
        frames = mk(len(pick), w, h, ms.depth, ms.sy, 6, fseed)
        seeds = M8.fresh_seeds(len(pick), 6) if seeded else None
        f0 = frames[0]
        fill = SP8.dst_frame(w, h, ms.sy, 9, 16, 32)
        src, dst = scattered(frames, 9), destinations(frames, fill, 9)
        regs0 = hip.seed_state()
        call(hip, src, dst, [ms.handles[k] for k in pick], seeds, f0, fill)
        got, regs = [d.download() for d in dst], hip.seed_state()
        dst2 = destinations(frames, fill, 10)
        U.program(hip, ms.recs[-1])
        assert hip.seed_state() == regs0          # (the library programmed with the model captured last, as in front of the call)
        for i, (k, s, d) in enumerate(zip(pick, src, dst2)):
            T.replay(hip, U.without_seed(ms.recs[k]))
            if seeds is not None:
                hip.set_seed(seeds[i])
            hip.add_grain_sp_frame_list_copy8_dev([s.ptrs()], [d.ptrs()], None, w, h, f0.stride, f0.uv_stride, fill.stride, fill.uv_stride, 6, stream_ptr())
        assert hip.seed_state() == regs
        for i, (a, d) in enumerate(zip(got, dst2)):
            assert_equal(a, d.download(), f"frame {i}")
    finally:
        ms.release()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

REFUSALS = ["15_plane_reaches_the_2_gib_window", "18_destination_is_its_own_source", "18_uv_overlaps_another_frames_y", "7_misaligned_plane", "6_destination_uv_stride", "8_destination_pitch", "16_depth_8",
            "40_csubx", "40_sample_shift", "40_width", "40_before_41", "41_null_models", "41_released_entry", "41_other_depth", "41_programmed_chroma_mix",
            "41_model_carries_a_mix"]


@pytest.mark.parametrize("case", REFUSALS)
def test_a_refusal_changes_nothing(hip, case):
    """each refusal with its code and its cause in the message; afterwards the registers, the launch count and every byte of the sources and
    the destinations are what they were; then the list is served"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_10_420"])
    extra, undo = [], (lambda: None)
    try:
        w, h = (8208, 17) if case == "40_width" else (520, 70)
        frames = mk(3, w, h, 10, 2, 6, 170)
        fill = SP8.dst_frame(w, h, 2, 77, 16, 32)
        src, dst = scattered(frames), destinations(frames, fill)
        f0 = frames[0]
        sp, dp = [d.ptrs() for d in src], [d.ptrs() for d in dst]
        hm = [ms.handles[0], ms.handles[1], ms.handles[0]]
        geo = dict(width=w, height=h, stride=f0.stride, uv_stride=f0.uv_stride, dst_stride=fill.stride, dst_uv_stride=fill.uv_stride, shift=6)
        seeds = M8.fresh_seeds(3, 8)
        code, match = int(case.split("_")[0]), None
        n = 3
        if case == "15_plane_reaches_the_2_gib_window":
            # ONE surface of 1864136 rows x 576 containers x 2 bytes: refused before anything is touched, so its planes are addresses, 8 GiB
            # apart.  The list checks find nothing; the destination pitch is too small (6), the shift is bad (40) and the models are NULL
            # (41) as well: 15 comes first.
            n, sp, dp, hm, match = 1, [(1 << 33, 2 << 33)], [(4 << 33, 5 << 33)], None, "2 GiB"
            geo.update(height=1864136, dst_stride=512, shift=4)
        if case.startswith("15_"):
            pass
        elif case == "18_destination_is_its_own_source":
            dp[1], match = (dp[1][0], sp[1][1]), "shares bytes"
        elif case == "18_uv_overlaps_another_frames_y":
            dp[1], match = (dp[1][0], dp[0][0] + 1024), "overlap"
        elif case == "7_misaligned_plane":
            dp[1], match = (dp[1][0], dp[1][1] + 8), "16-byte aligned"
        elif case == "6_destination_uv_stride":
            geo["dst_uv_stride"], match = 272, "destination stride"
        elif case == "8_destination_pitch":
            geo["dst_stride"], match = fill.stride - 8, "multiples of 16"      # (still a row of whole blocks, and inside the allocation: the list checks find nothing)
        elif case == "16_depth_8":
            hip.set_depth(8)
            undo, match = (lambda: hip.set_depth(10)), "8-bit output"
            geo.update(stride=2 * f0.stride, uv_stride=2 * f0.uv_stride, shift=0)     # (the planes as they are, in 8-bit containers: the list checks come first)
        elif case == "40_csubx":
            hip.set_chroma_subsampling(1, 2)       # (4:4:0: the chroma rows of the planes as they are)
            undo, match = (lambda: hip.set_chroma_subsampling(2, 2)), "csubx 1"
        elif case == "40_sample_shift":
            geo["shift"], match = 4, "sample_shift 4 at depth 10"
        elif case == "40_width":
            match = "width 8208"
        elif case == "40_before_41":
            geo["shift"], hm, match = 4, None, "sample_shift 4"
        elif case == "41_null_models":
            hm, match = None, "null list of models"
        elif case == "41_released_entry":
            gone = Models(hip, ["fgs_sei_10_420"])
            gone.release()
            hm[2], match = gone.handles[0], "frame 2 is not a live model"
        elif case == "41_other_depth":
            extra.append(Models(hip, ["fgs_sei_10_420@depth12"]))
            U.program(hip, ms.recs[-1])
            hm[1], match = extra[0].handles[0], "depth 12"
        elif case == "41_programmed_chroma_mix":
            hip.set_chroma_mix(1, 32, 32, 0)
            undo, match = hip.clear_chroma_mix, "chroma mix"
        elif case == "41_model_carries_a_mix":
            U.program(hip, ms.recs[0])
            hip.set_chroma_mix(1, 32, 32, 0)
            extra.append(hip.model_capture_mix(stream_ptr()))
            hip.clear_chroma_mix()
            U.program(hip, ms.recs[-1])
            hm[0], match = extra[0], "chroma mix"
        st0, n0, b0 = hip.seed_state(), U.launches(hip), hip.model_build_stats()
        try:
            s, d = hip.sp_frame_list(sp), hip.sp_frame_list(dp)
            arr = None if hm is None else (C.c_void_p * 3)(*hm)
            rc = hip.lib.vfgs_hip_add_grain_sp_frame_list_models_copy8_dev(s, d, arr, hip.seed_list(seeds[:n]), n, *geo.values(), stream_ptr())
            assert rc == code and hip.lib.vfgs_hip_last_error() == code, (rc, hip.lib.vfgs_hip_last_error_string())
            assert match in hip.lib.vfgs_hip_last_error_string().decode(), hip.lib.vfgs_hip_last_error_string()
            if hm is not None:
                with pytest.raises(VfgsHipError, match=f"error {code}"):          # ... and through the Python method
                    hip.add_grain_sp_frame_list_models_copy8_dev(sp, dp, hm, seeds, *geo.values(), stream_ptr())
        finally:
            undo()
        assert hip.seed_state() == st0 and U.launches(hip) == n0 and hip.model_build_stats() == b0
        check8(src, dst, frames, [fill] * 3, "after the refusal:")
        if case != "40_width":
            pick = [0, 1, 0]
            want, regs, _ = M8.expect_sp(ms.recs, pick, frames, seeds, fill)
            call(hip, src, dst, [ms.handles[k] for k in pick], seeds, f0, fill)
            check8(src, dst, frames, want)
            assert hip.seed_state() == regs
    finally:
        for x in [ms] + extra:
            x.release() if isinstance(x, Models) else hip.model_release(x)


def test_an_empty_list_is_no_call_at_all(hip):
    st0, n0 = hip.seed_state(), U.launches(hip)
    hip.add_grain_sp_frame_list_models_copy8_dev([], [], [], None, 520, 70, 576, 576, 528, 528, 6, stream_ptr())
    assert hip.lib.vfgs_hip_add_grain_sp_frame_list_models_copy8_dev(None, None, None, None, 0, 100, 70, 0, 0, 0, 0, 99, stream_ptr()) == 0
    assert hip.seed_state() == st0 and U.launches(hip) == n0
