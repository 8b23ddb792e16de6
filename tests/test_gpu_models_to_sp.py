"""GPU (MI355X): vfgs_hip_add_grain_frame_list_models_to_sp_dev and _to_sp8_dev -- planar pictures in, semi-planar surfaces out (yuv420p10le
-> P010 or NV12, yuv420p -> NV12, yuv422p10le -> P210 ...), a model per picture in one launch -- against the oracle, through the C ABI, bit
for bit: every container of both destination planes of every frame, padding included (pre-filled garbage survives), every sample of the
sources (unchanged), and the four seed registers.

The contract (include/vfgs_hip.h) is the loop of the calls with models around the one-frame _to_sp / _to_sp8 call; the expectation is
tests/models_to_sp_util.py's, whose case tables tests/test_models_to_sp_cases_cpu.py runs on the oracle alone.  The launches are
grain_p2sp_kernel's and grain_p2sp8_kernel's, which decide at run time where image, bounds and shift come from.  Frames are separate
allocations listed out of address order; sources hold garbage over the whole container, destinations have Y and UV pitches that exceed
the rows and differ.  Shapes: 136 x 33 (9 blocks, the smallest row served), 1047 x 40 (a ragged width, a partial last block row),
1032 x 90 -- none larger."""
import ctypes as C

import pytest

import model_list_util as U
import models_to_sp_util as M
import vfgs_testlib as T
from gpu_util import stream_ptr
from test_gpu_planar_to_sp import check, destinations, scattered
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


def call(hip, src, dst, models, seeds, f0, fill, shift, out8, stream=None):
    st = stream_ptr() if stream is None else stream
    s, d = [x.ptrs() for x in src], [x.ptrs() for x in dst]
    if out8:
        hip.add_grain_frame_list_models_to_sp8_dev(s, d, models, seeds, f0.width, f0.height, f0.stride, f0.cstride, fill.stride, fill.uv_stride, st)
    else:
        hip.add_grain_frame_list_models_to_sp_dev(s, d, models, seeds, f0.width, f0.height, f0.stride, f0.cstride, fill.stride, fill.uv_stride, shift, st)


def mk(n, w, h, depth, sy, seed):
    return [M.garbage_frame(w, h, depth, sy, seed + i) for i in range(n)]


def run(hip, recs, handles, pick, frames, shift, out8, seeds=None, ora=None, shuffle=0):
    f0 = frames[0]
    fill = M.fill_for(f0.width, f0.height, f0.depth, f0.suby, shift, out8, 4321 + shuffle)
    assert fill.stride != fill.uv_stride
    want, regs, ora = M.expect(recs, pick, frames, seeds, shift, out8, fill, ora)
    src, dst = scattered(frames, shuffle), destinations(len(frames), fill, shuffle)
    call(hip, src, dst, [handles[k] for k in pick], seeds, f0, fill, shift, out8)
    check(src, dst, frames, want)
    assert hip.seed_state() == regs
    return ora


def kernel_of(ms, k, out8):
    return T.kernel_name("grain_p2sp8_kernel" if out8 else "grain_p2sp_kernel", ms.depth, ms.sy, *ms.forms[k])


def assert_launch(info, ms, k, out8, nframes):
    assert info["listed"] == 1 and info["in_place"] == 0 and info["out8"] == (1 if out8 else 0) and info["depth"] == ms.depth, info
    assert info["persistent_luma_workgroups"] == 0 and info["nframes"] == nframes and info["kernel"] == kernel_of(ms, k, out8), info


# ---- 1. surfaces, sizes, A B A C B ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("size", M.SURFACE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("surface", sorted(M.SURFACES))
def test_surfaces(hip, surface, size, seeded):
    """to P010 (shift 6), P210, P012 (shift 4), low-aligned containers, NV12 and NV16 at depth 8; narrowed: depth 10 and 12 to NV12 / NV16;
    a ragged 1047 x 40 and 1032 x 90; models A B A C B with C of another form: a launch per run"""
    names, pick, (w, h), shift, out8, fseed = M.CASES["%s_%dx%d" % ((surface,) + size)]
    ms = Models(hip, names)
    try:
        assert ms.forms[2] != ms.forms[0] and shift in (0, 16 - ms.depth)
        n0 = U.launches(hip)
        run(hip, ms.recs, ms.handles, pick, mk(len(pick), w, h, ms.depth, ms.sy, fseed), shift, out8, M.fresh_seeds(len(pick), 1) if seeded else None, shuffle=1)
        info = hip.last_launch_info()
        runs = U.runs_of(ms.forms, pick)
        assert len(runs) >= 3 and info["launches"] - n0 == len(runs), (info, runs)
        assert_launch(info, ms, pick[-1], out8, runs[-1])
        assert bool(hip.seeded_stream_stats()["last_launch_used_it"]) == seeded
    finally:
        ms.release()


# ---- 2. bounds and shift are the frame's own ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["bounds_p010", "bounds_nv12"])
def test_bounds_and_shift_are_the_frames_own(hip, case):
    """two models of one form that differ in legal range, scale shift and scale LUTs, B A A B A B B in ONE launch: a workgroup -- luma, or UV
    whose store holds Cb and Cr clipped with one pair of bounds -- that took the launch's record would be wrong on the other model's frames
    (tests/test_models_to_sp_cases_cpu.py: the two differ in all three planes on these frames)"""
    _, pick, (w, h), shift, out8, fseed = M.CASES[case]
    ms = Models(hip, M.case_records(case))
    try:
        assert ms.forms[0] == ms.forms[1] and ms.info[0]["legal_range"] != ms.info[1]["legal_range"], ms.info
        assert ms.info[0]["scale_shift"] != ms.info[1]["scale_shift"], ms.info
        n0 = U.launches(hip)
        run(hip, ms.recs, ms.handles, pick, mk(len(pick), w, h, ms.depth, ms.sy, fseed), shift, out8, None, shuffle=2)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 1
        assert_launch(info, ms, 0, out8, len(pick))
    finally:
        ms.release()


# ---- 3. more frames than a launch holds ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("case", ["34_frames_p010", "34_frames_nv12"])
def test_more_frames_than_one_launch_holds(hip, case, seeded):
    """34 frames of 136 x 33, two models of one form alternating: launches of 32 + 2"""
    names, pick, (w, h), shift, out8, fseed = M.CASES[case]
    ms = Models(hip, names)
    try:
        assert ms.forms[0] == ms.forms[1]
        n0 = U.launches(hip)
        run(hip, ms.recs, ms.handles, pick, mk(len(pick), w, h, ms.depth, ms.sy, fseed), shift, out8, M.fresh_seeds(len(pick), 4) if seeded else None, shuffle=4)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 2
        assert_launch(info, ms, 1, out8, 2)
    finally:
        ms.release()


# ---- 4. general-form and SEI-built / AFGS1-built models beside captured ones ----------------------------------------------------------------

@pytest.mark.parametrize("out8", [False, True], ids=["container", "narrowed"])
def test_models_of_three_origins(hip, out8):
    """handles of vfgs_hip_models_from_sei, vfgs_hip_models_from_afgs1 and vfgs_hip_model_capture interleaved in one list at 10-bit 4:2:0,
    general-form and one-pattern models among them: the surfaces are the oracle's loop, the launches the runs of equal form"""
    from versatilefilmgrain_amd import fw
    from test_gpu_models_from_sei import sei_of, set_format
    sei_names = ["default_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"]
    afgs1_names = ["fgs_afgs1_test1_10_420", "fgs_afgs1_test9_10_420"]
    cap_names = ["fgs_sei_ff_test2_10_420", "fgs_afgs1_test3_10_420"]
    caps = U.capture_all(hip, [U.model_records(n) for n in cap_names], stream_ptr())
    set_format(hip, 10, 2, 2)
    models = hip.models_from_sei([sei_of(n) for n in sei_names], stream_ptr())
    models += hip.models_from_afgs1([fw.struct_from_bytes(1, T.load_fwcfg(n)[1][-1][1]) for n in afgs1_names], stream_ptr())
    models += caps
    try:
        names = sei_names + afgs1_names + cap_names
        recs = [U.model_records(n) for n in names]
        forms = [(hip.model_info(m)["one_y"], hip.model_info(m)["one_c"]) for m in models]
        assert (0, 1) in forms and (1, 1) in forms, forms
        pick = [0, 3, 5, 1, 4, 6, 2, 0, 5, 3, 1, 6]
        n0 = U.launches(hip)
        run(hip, recs, models, pick, mk(len(pick), 1047, 40, 10, 2, 700), 0 if out8 else 6, out8, M.fresh_seeds(len(pick), 66), shuffle=5)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == len(U.runs_of(forms, pick)), (forms, pick, info)
        assert info["kernel"].startswith("grain_p2sp8_kernel<" if out8 else "grain_p2sp_kernel<") and info["out8"] == int(out8), info
    finally:
        for m in models:
            hip.model_release(m)


# ---- 5. the call equals the loop of its contract, run by the library itself ------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("case", ["definition_p010", "definition_nv12"])
def test_the_call_equals_its_definition_on_the_gpu(hip, case, seeded):
    """per frame: program, set_seed, the one-picture _to_sp / _to_sp8 call -- identical surfaces and registers"""
    names, pick, (w, h), shift, out8, fseed = M.CASES[case]
    ms = Models(hip, names)
    try:
        frames = mk(len(pick), w, h, ms.depth, ms.sy, fseed)
        seeds = M.fresh_seeds(len(pick), 6) if seeded else None
        f0 = frames[0]
        fill = M.fill_for(w, h, ms.depth, ms.sy, shift, out8, 9, 16, 32)
        src, dst = scattered(frames, 9), destinations(len(frames), fill, 9)
        regs0 = hip.seed_state()
        call(hip, src, dst, [ms.handles[k] for k in pick], seeds, f0, fill, shift, out8)
        got, regs = [d.download() for d in dst], hip.seed_state()
        dst2 = destinations(len(frames), fill, 10)
        U.program(hip, ms.recs[-1])
        assert hip.seed_state() == regs0          # (the library programmed with the model captured last, as in front of the call)
        for i, (k, s, d) in enumerate(zip(pick, src, dst2)):
            T.replay(hip, U.without_seed(ms.recs[k]))
            if seeds is not None:
                hip.set_seed(seeds[i])
            geo = (w, h, f0.stride, f0.cstride, fill.stride, fill.uv_stride)
            if out8:
                hip.add_grain_frame_list_to_sp8_dev([s.ptrs()], [d.ptrs()], None, *geo, stream_ptr())
            else:
                hip.add_grain_frame_list_to_sp_dev([s.ptrs()], [d.ptrs()], None, *geo, shift, stream_ptr())
        assert hip.seed_state() == regs
        check(src, dst2, frames, got, "the loop:")
    finally:
        ms.release()


# ---- 6. the programmed state is untouched ----------------------------------------------------------------------------------------------------

def test_the_programmed_state_is_untouched(hip):
    """params, LUTs and mix behind the call are those in front of it, and a programmed one-picture _to_sp_dev grains with the model
    programmed last (general-form luma), not the one listed last (one-pattern): the same surface as in front of the call"""
    import planar_to_sp_util as P2
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"])      # programmed last: fgs_sei_10_420
    try:
        w, h = 136, 33
        probe = mk(1, w, h, 10, 2, 77)
        fill = M.fill_for(w, h, 10, 2, 6, False, 5)
        f0 = probe[0]

        def programmed_picture():
            src, dst = scattered(probe, 1), destinations(1, fill, 1)
            hip.set_seed(1234)
            hip.add_grain_frame_list_to_sp_dev([src[0].ptrs()], [dst[0].ptrs()], None, w, h, f0.stride, f0.cstride, fill.stride, fill.uv_stride, 6, stream_ptr())
            return dst[0].download(), hip.last_launch_info()["kernel"]

        def state():
            return {"params": hip.params(), "luts": [hip.luts(c) for c in range(3)], "mix": [hip.chroma_mix(c) for c in (1, 2)]}

        before, kernel0 = programmed_picture()
        ora = U.oracle_programmed(ms.recs[2])
        ora.set_seed(1234)
        assert before.equal_all(P2.expected(ora, probe, None, 6, fill)[0]) and kernel0 == "grain_p2sp_kernel<10,2,false,true>"
        st0 = state()
        for out8 in (False, True):
            run(hip, ms.recs, ms.handles, [0, 1, 0, 1, 1], mk(5, w, h, 10, 2, 90), 0 if out8 else 6, out8, None, ora=ora, shuffle=9)
            assert hip.last_launch_info()["kernel"] == kernel_of(ms, 1, out8) and ms.forms[1] == (1, 1)
            assert state() == st0
            T.replay(ora, U.without_seed(ms.recs[2]))
        after, kernel1 = programmed_picture()
        assert after.equal_all(before) and kernel1 == kernel0
    finally:
        ms.release()


# ---- 7. inside an overlap region -------------------------------------------------------------------------------------------------------------

def test_two_calls_inside_an_overlap_region(hip):
    names, pick, (w, h), shift, _, fseed = M.CASES["overlap_region"]
    ms = Models(hip, names)
    try:
        a, b = mk(4, w, h, ms.depth, ms.sy, fseed), mk(3, w, h, ms.depth, ms.sy, fseed + 10)
        fa, fb = M.fill_for(w, h, ms.depth, ms.sy, shift, False, 5, 16, 32), M.fill_for(w, h, ms.depth, ms.sy, 0, True, 6, 32, 16)
        ora = U.oracle_programmed(ms.recs[-1])
        wa, _, _ = M.expect(ms.recs, pick[:4], a, None, shift, False, fa, ora)
        wb, regs, _ = M.expect(ms.recs, pick[4:], b, None, 0, True, fb, ora)
        sa, sb, da, db = scattered(a, 8), scattered(b, 9), destinations(4, fa, 8), destinations(3, fb, 9)
        hm = [ms.handles[k] for k in pick]
        st = stream_ptr()
        hip.overlap_begin(st)
        call(hip, sa, da, hm[:4], None, a[0], fa, shift, False, st)
        call(hip, sb, db, hm[4:], None, a[0], fb, 0, True, st)
        hip.overlap_end(st)
        check(sa + sb, da + db, a + b, wa + wb)
        assert hip.seed_state() == regs
    finally:
        ms.release()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------

REFUSALS = ["40_csubx", "40_sample_shift", "40_width", "40_before_16_and_41", "16_depth_8", "16_before_18", "18_null_source_list", "18_null_destination_list",
            "18_null_plane", "18_two_destinations_share_bytes", "18_destination_on_a_source_plane", "18_destination_on_another_frames_source",
            "6_destination_stride", "6_destination_uv_stride", "8_destination_pitch", "6_before_the_list_checks", "7_misaligned_source",
            "7_misaligned_destination", "5_width", "6_source_stride", "8_source_pitch", "15_plane_reaches_the_2_gib_window", "18_before_41",
            "41_null_models", "41_null_entry", "41_released_entry", "41_other_depth", "41_other_chroma_format", "41_programmed_chroma_mix",
            "41_model_carries_a_mix"]


# (error 16 is the narrowed call's alone, and it takes no sample_shift)
REFUSAL_PARAMS = [(c, o) for c in REFUSALS for o in (False, True) if not (c.startswith("16_") and not o) and not (c == "40_sample_shift" and o)]


@pytest.mark.parametrize("case,out8", REFUSAL_PARAMS, ids=["%s-%s" % (c, "narrowed" if o else "container") for c, o in REFUSAL_PARAMS])
def test_a_refusal_changes_nothing(hip, case, out8):
    """each refusal with its code and its cause in the message, in the order the header states; afterwards the registers, the launch count
    and every byte of the sources and the destinations are what they were; then the list is served"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_10_420"])
    extra, undo = [], (lambda: None)
    try:
        w, h = (8208, 17) if case == "40_width" else (136, 33)
        good = 0 if out8 else 6
        frames = mk(3, w, h, 10, 2, 170)
        fill = M.fill_for(w, h, 10, 2, good, out8, 77, 16, 32)
        src, dst = scattered(frames), destinations(3, fill)
        f0 = frames[0]
        sp, dp = [d.ptrs() for d in src], [d.ptrs() for d in dst]
        hm = [ms.handles[0], ms.handles[1], ms.handles[0]]
        geo = dict(width=w, height=h, stride=f0.stride, cstride=f0.cstride, dst_stride=fill.stride, dst_uv_stride=fill.uv_stride)
        shift = good
        seeds = M.fresh_seeds(3, 8)
        code, match = int(case.split("_")[0]), None
        n, null_src, null_dst = 3, False, False
        if case == "40_csubx":
            hip.set_chroma_subsampling(1, 2)       # (4:4:0: the chroma rows of the planes as they are)
            undo, match = (lambda: hip.set_chroma_subsampling(2, 2)), "csubx 1"
        elif case == "40_sample_shift":
            shift, match = 4, "sample_shift 4 at depth 10"
        elif case == "40_width":
            match = "width 8208"
        elif case == "40_before_16_and_41":
            # 4:4:4 at depth 8 with null models: the chroma format is named first
            hip.set_depth(8)
            hip.set_chroma_subsampling(1, 1)
            undo = lambda: (hip.set_depth(10), hip.set_chroma_subsampling(2, 2))
            hm, shift, match = None, 0, "csubx 1"
        elif case == "16_depth_8":
            hip.set_depth(8)
            undo, match = (lambda: hip.set_depth(10)), "8-bit output"
        elif case == "16_before_18":
            hip.set_depth(8)
            undo, null_src, hm, match = (lambda: hip.set_depth(10)), True, None, "8-bit output"
        elif case == "18_null_source_list":
            null_src, match = True, "null list"
        elif case == "18_null_destination_list":
            null_dst, match = True, "null list"
        elif case == "18_null_plane":
            sp[1], match = (sp[1][0], sp[1][1], 0), "null plane"
        elif case == "18_two_destinations_share_bytes":
            dp[2], match = dp[0], "listed twice"
        elif case == "18_destination_on_a_source_plane":
            dp[1], match = (sp[1][0], dp[1][1]), "shares bytes"
        elif case == "18_destination_on_another_frames_source":
            dp[1], match = (dp[1][0], sp[2][0]), "shares bytes"
        elif case == "6_destination_stride":
            geo["dst_stride"], match = 128, "destination stride"
        elif case == "6_destination_uv_stride":
            geo["dst_uv_stride"], match = 80, "destination stride"      # (a UV row is as many containers as the luma row)
        elif case == "8_destination_pitch":
            geo["dst_stride"], match = fill.stride - 4, "multiples of 16"     # (still a row of whole blocks)
        elif case == "6_before_the_list_checks":
            geo["dst_stride"], sp[1], match = 128, (sp[1][0], sp[1][1] + 8, sp[1][2]), "destination stride"
        elif case == "7_misaligned_source":
            sp[1], match = (sp[1][0], sp[1][1] + 8, sp[1][2]), "16-byte aligned"
        elif case == "7_misaligned_destination":
            dp[1], match = (dp[1][0], dp[1][1] + 8), "16-byte aligned"
        elif case == "5_width":
            geo["width"], match = 100, "width 100"
        elif case == "6_source_stride":
            geo["cstride"], match = 64, "too small"
        elif case == "8_source_pitch":
            geo["stride"], match = f0.stride + 4, "multiple of 16"
        elif case == "15_plane_reaches_the_2_gib_window":
            # ONE picture of 1864136 rows x 576 samples x 2 bytes: refused before anything is touched, so its planes are addresses, 8 GiB
            # apart.  The list checks find nothing; the models are NULL (41) as well: 15 comes first.
            n, sp, dp, hm, match = 1, [(1 << 33, 2 << 33, 3 << 33)], [(4 << 33, 5 << 33)], None, "2 GiB"
            geo.update(width=520, height=1864136, stride=576, cstride=288, dst_stride=528, dst_uv_stride=544)
        elif case == "18_before_41":
            dp[2], hm, match = dp[0], None, "listed twice"
        elif case == "41_null_models":
            hm, match = None, "null list of models"
        elif case == "41_null_entry":
            hm[1], match = None, "frame 1 is null"
        elif case == "41_released_entry":
            gone = Models(hip, ["fgs_sei_10_420"])
            gone.release()
            hm[2], match = gone.handles[0], "frame 2 is not a live model"
        elif case == "41_other_depth":
            extra.append(Models(hip, ["fgs_sei_10_420@depth12"]))
            U.program(hip, ms.recs[-1])
            hm[1], match = extra[0].handles[0], "depth 12"
        elif case == "41_other_chroma_format":
            extra.append(Models(hip, ["fgs_sei_10_422"]))
            U.program(hip, ms.recs[-1])
            hm[1], match = extra[0].handles[0], "chroma subsampling 2,1"
        elif case == "41_programmed_chroma_mix":
            hip.set_chroma_mix(1, 32, 32, 0)
            undo, match = hip.clear_chroma_mix, "chroma mix"
        elif case == "41_model_carries_a_mix":
            U.program(hip, ms.recs[0])
            hip.set_chroma_mix(1, 32, 32, 0)
            extra.append(hip.model_capture_mix(stream_ptr()))
            hip.clear_chroma_mix()
            U.program(hip, ms.recs[-1])
            hm[0], match = extra[0], "carries a chroma mix"
        st0, n0, b0 = hip.seed_state(), U.launches(hip), hip.model_build_stats()
        tail = (stream_ptr(),) if out8 else (shift, stream_ptr())
        try:
            s, d = (None if null_src else hip.frame_list(sp)), (None if null_dst else hip.sp_frame_list(dp))
            arr = None if hm is None else (C.c_void_p * 3)(*hm)
            fn = hip.lib.vfgs_hip_add_grain_frame_list_models_to_sp8_dev if out8 else hip.lib.vfgs_hip_add_grain_frame_list_models_to_sp_dev
            rc = fn(s, d, arr, hip.seed_list(seeds[:n]), n, *geo.values(), *tail)
            assert rc == code and hip.lib.vfgs_hip_last_error() == code, (rc, hip.lib.vfgs_hip_last_error_string())
            assert match in hip.lib.vfgs_hip_last_error_string().decode(), hip.lib.vfgs_hip_last_error_string()
            if hm is not None and not null_src and not null_dst:
                method = hip.add_grain_frame_list_models_to_sp8_dev if out8 else hip.add_grain_frame_list_models_to_sp_dev
                with pytest.raises(VfgsHipError, match=f"error {code}"):          # ... and through the Python method
                    method(sp, dp, hm, seeds, *geo.values(), *tail)
        finally:
            undo()
        assert hip.seed_state() == st0 and U.launches(hip) == n0 and hip.model_build_stats() == b0
        check(src, dst, frames, [fill] * 3, "after the refusal:")
        if case != "40_width":
            pick = [0, 1, 0]
            want, regs, _ = M.expect(ms.recs, pick, frames, seeds, good, out8, fill)
            call(hip, src, dst, [ms.handles[k] for k in pick], seeds, f0, fill, good, out8)
            check(src, dst, frames, want)
            assert hip.seed_state() == regs and U.launches(hip) == n0 + len(U.runs_of(ms.forms, pick))
    finally:
        for x in [ms] + extra:
            x.release() if isinstance(x, Models) else hip.model_release(x)


def test_the_programmed_calls_keep_their_refusal_under_a_mix(hip):
    """vfgs_hip_add_grain_frame_list_to_sp_dev / _to_sp8_dev under a programmed mix: error 40 as before"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    ms = Models(hip, ["fgs_afgs1_test1_10_420"])
    try:
        frames = mk(1, 136, 33, 10, 2, 3)
        f0 = frames[0]
        src = scattered(frames)
        hip.set_chroma_mix(1, 32, 32, 0)
        try:
            for out8 in (False, True):
                fill = M.fill_for(136, 33, 10, 2, 0, out8, 7)
                dst = destinations(1, fill)
                geo = (136, 33, f0.stride, f0.cstride, fill.stride, fill.uv_stride)
                with pytest.raises(VfgsHipError, match="error 40:.*chroma mix"):
                    if out8:
                        hip.add_grain_frame_list_to_sp8_dev([src[0].ptrs()], [dst[0].ptrs()], None, *geo, stream_ptr())
                    else:
                        hip.add_grain_frame_list_to_sp_dev([src[0].ptrs()], [dst[0].ptrs()], None, *geo, 0, stream_ptr())
        finally:
            hip.clear_chroma_mix()
    finally:
        ms.release()


# ---- 9. an empty list --------------------------------------------------------------------------------------------------------------------------

def test_an_empty_list_is_no_call_at_all(hip):
    st0, n0 = hip.seed_state(), U.launches(hip)
    hip.add_grain_frame_list_models_to_sp_dev([], [], [], None, 520, 70, 576, 288, 528, 528, 6, stream_ptr())
    hip.add_grain_frame_list_models_to_sp8_dev([], [], [], None, 520, 70, 576, 288, 528, 528, stream_ptr())
    assert hip.lib.vfgs_hip_add_grain_frame_list_models_to_sp_dev(None, None, None, None, 0, 100, 70, 0, 0, 0, 0, 99, stream_ptr()) == 0
    assert hip.lib.vfgs_hip_add_grain_frame_list_models_to_sp8_dev(None, None, None, None, 0, 100, 70, 0, 0, 0, 0, stream_ptr()) == 0
    assert hip.seed_state() == st0 and U.launches(hip) == n0
