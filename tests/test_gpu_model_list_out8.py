"""GPU (MI355X): vfgs_hip_add_grain_frame_list_models_copy8_dev -- planar 10- or 12-bit pictures in, planar 8-bit pictures out, a model per
picture in one launch -- against the oracle, through the C ABI, bit for bit: every byte of every destination plane, padding included, every
sample of the sources (unchanged), and the four seed registers.

The contract (include/vfgs_hip.h) is a loop -- program the state models[f] was made from; with seeds vfgs_set_seed(seeds[f]); the one-frame
_copy8 list on frame f -- so the ground truth is the oracle run as that loop, narrowed as yuv_to_8bit does and written over a garbage-filled
destination exactly where the call writes (tests/model_out8_util.py, whose case tables tests/test_model_out8_cases_cpu.py runs on the oracle
alone).  The launches are grain_rw_kernel's, the kernels of the programmed _copy8 calls, which take image, bounds and shift from each
frame's model where a launch names models.  Frames are separate allocations listed out of address order; sources hold garbage over the full
container range, so the clip bounds bind on most samples."""
import ctypes as C

import numpy as np
import pytest

import model_list_util as U
import model_out8_util as M8
import vfgs_testlib as T
from gpu_util import stream_ptr
from test_gpu_frame_list import garbage_frame, scattered
from test_gpu_model_list import Models

pytestmark = pytest.mark.gpu

W, H = M8.W, M8.H


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


class Dev8:
    """a model_out8_util.Dst8 resident on the device, planes contiguous"""

    def __init__(self, d):
        import torch
        self.d = d
        self.t = [torch.from_numpy(p.copy()).cuda() for p in d.planes()]

    def ptrs(self):
        return tuple(t.data_ptr() for t in self.t)

    def download(self):
        import torch
        torch.cuda.synchronize()
        g = self.d.copy()
        for p, t in zip(g.planes(), self.t):
            p[...] = t.cpu().numpy()
        return g


def destinations(n, fill, seed=0):
    order = np.random.default_rng(1000 + seed).permutation(n)
    dst = [None] * n
    for i in order:
        dst[i] = Dev8(fill)
    return dst


def fill_for(f0, seed, pad=16, cpad=48):
    return M8.dst_frame(f0.width, f0.height, f0.subx, f0.suby, 4321 + seed, pad, cpad)


def call(hip, src, dst, models, seeds, f0, fill, stream=None):
    hip.add_grain_frame_list_models_copy8_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], models, seeds, f0.width, f0.height, f0.stride, f0.cstride,
                                              fill.stride, fill.cstride, stream_ptr() if stream is None else stream)


def check(src, dst, frames, want, what=""):
    for i, (s, d, f, w) in enumerate(zip(src, dst, frames, want)):
        g = d.download()
        for name, a, b in zip("YUV", g.planes(), w.planes()):
            assert np.array_equal(a, b), f"{what} destination {i} plane {name}: {int((a != b).sum())} bytes differ"
        assert s.download().equal_all(f), f"{what} source {i}"


def run(hip, ms, pick, frames, seeds=None, ora=None, shuffle=0, stream=None, pad=16, cpad=48):
    """the list through the call vs the contract's loop; -> (sources, destinations, the oracle of an unseeded run)"""
    f0 = frames[0]
    fill = fill_for(f0, shuffle, pad, cpad)
    want, regs, ora = M8.expect_planar(ms.recs, pick, frames, seeds, fill, ora)
    src, dst = scattered(frames, shuffle), destinations(len(frames), fill, shuffle)
    call(hip, src, dst, [ms.handles[k] for k in pick], seeds, f0, fill, stream)
    check(src, dst, frames, want)
    assert hip.seed_state() == regs
    return src, dst, ora


def kernel_of(ms, k):
    b = lambda v: "true" if v else "false"
    oy, oc = ms.forms[k]
    return f"grain_rw_kernel<{ms.depth},{ms.sx},{ms.sy},true,{b(oy)},{b(oc)},false,false>"


def assert_record(info, ms, pick, n0):
    runs = U.runs_of(ms.forms, pick)
    assert info["launches"] - n0 == len(runs) and info["nframes"] == runs[-1], (info, runs)
    assert info["listed"] == 1 and info["out8"] == 1 and info["in_place"] == 0 and info["persistent_luma_workgroups"] == 0 and info["depth"] == ms.depth, info
    assert info["kernel"] == kernel_of(ms, pick[-1]), info


# ---- every format -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("cfg", sorted(M8.PLANAR_CONFIGS))
def test_every_format(hip, cfg, seeded):
    """7 frames of 1032 x 90, models A B A B ...: depth 10 at 4:2:0 (one-pattern and general), 4:2:2, 4:4:4, 4:4:0, depth 12"""
    names, pick, (w, h), fseed = M8.PLANAR_CASES[f"every_format_{cfg}"]
    ms = Models(hip, names)
    try:
        pick = M8.pick_of(pick, len(names))
        n0 = U.launches(hip)
        run(hip, ms, pick, ms.frames(len(pick), fseed, w, h), M8.fresh_seeds(len(pick), 1) if seeded else None, shuffle=1)
        assert_record(hip.last_launch_info(), ms, pick, n0)
    finally:
        ms.release()


# ---- one form, different content, one launch ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_same_form_different_content_in_one_launch(hip, seeded):
    """AFGS1 models with other scale LUTs, two scale shifts and the legal range on (test1) and off: ONE launch.  The content covers the full
    container range, so the clip bounds bind; a workgroup that took the launch's bounds (frame 0's) would be wrong on the frames of the
    other range -- asserted on the oracle alone before the GPU runs."""
    names, pick, (w, h), fseed = M8.PLANAR_CASES["same_form"]
    ms = Models(hip, names)
    try:
        assert len(set(ms.forms)) == 1 and ms.forms[0] == (1, 1), ms.forms
        assert len({i["scale_shift"] for i in ms.info}) == 2 and {i["legal_range"] for i in ms.info} == {0, 1}, ms.info
        frames = ms.frames(len(pick), fseed, w, h)
        seeds = M8.fresh_seeds(len(pick), 2)
        fill = fill_for(frames[0], 2)
        own, _, _ = M8.expect_planar(ms.recs, pick, frames, seeds, fill)
        first, _, _ = M8.expect_planar(ms.recs, [pick[0]] * len(pick), frames, seeds, fill)
        assert any(not a.equal_all(b) for a, b in zip(own, first)), "frame 0's model gives the same bytes on every frame: the case proves nothing"
        assert all(not np.array_equal(a.U, b.U) for a, b, k in zip(own, first, pick) if ms.info[k]["legal_range"] != ms.info[pick[0]]["legal_range"])
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, seeds if seeded else None, shuffle=2)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 1 and info["nframes"] == len(pick) and info["kernel"] == kernel_of(ms, 0), info
    finally:
        ms.release()


# ---- forms change, more frames than a launch holds ------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_forms_change_inside_the_list(hip, seeded):
    """A A B B B A with A general luma, B one-pattern: three launches, each with its slice of the frames (and of the seeds)"""
    names, pick, (w, h), fseed = M8.PLANAR_CASES["form_change"]
    ms = Models(hip, names)
    try:
        assert ms.forms[0] != ms.forms[1]
        n0 = U.launches(hip)
        run(hip, ms, pick, ms.frames(len(pick), fseed, w, h), M8.fresh_seeds(len(pick), 3) if seeded else None, shuffle=3)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 3 and info["nframes"] == 1 and info["kernel"] == kernel_of(ms, 0), info
    finally:
        ms.release()


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_more_frames_than_one_launch_holds(hip, seeded):
    """34 frames of 136 x 32, two models of one form alternating: launches of 32 + 2"""
    names, pick, (w, h), fseed = M8.PLANAR_CASES["34_frames"]
    ms = Models(hip, names)
    try:
        n0 = U.launches(hip)
        run(hip, ms, pick, ms.frames(len(pick), fseed, w, h), M8.fresh_seeds(len(pick), 4) if seeded else None, shuffle=4)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 2 and info["nframes"] == 2 and info["out8"] == 1, info
    finally:
        ms.release()


# ---- row geometry ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width,positions", [(1920, 2), (960, 1)])
def test_narrow_chroma_rows(hip, width, positions):
    """chroma rows of two positions and of one: several rows per group of the ring (run_plane_rw NARROW), each row's frame with its model"""
    names, pick, (w, h), fseed = M8.PLANAR_CASES[f"narrow_{width}"]
    ms = Models(hip, names)
    try:
        run(hip, ms, pick, ms.frames(len(pick), fseed, w, h), None, shuffle=7)
        assert hip.last_launch_info()["positions_per_row"][1] == positions
        run(hip, ms, pick, ms.frames(len(pick), fseed + 10, w, h), M8.fresh_seeds(len(pick), 5), shuffle=6)
        info = hip.last_launch_info()
        assert info["positions_per_row"][1] == positions and info["out8"] == 1, info
    finally:
        ms.release()


def test_two_frame_fronts(hip):
    """three frames of 8192 x 1366, models A B A: 2 x (16384 + 2 x 4096) x 1366 bytes of source planes are the first 64 MiB at that width
    (1365 rows stay below), so frames 2m and 2m + 1 are swept together, the odd front a plane phase behind, each frame with its own model"""
    names, pick, (w, h), fseed = M8.PLANAR_CASES["two_fronts"]
    ms = Models(hip, names)
    try:
        run(hip, ms, pick, ms.frames(len(pick), fseed, w, h), None, shuffle=5, pad=0, cpad=16)
        info = hip.last_launch_info()
        assert info["frames_per_front"] == 2 and info["nframes"] == 3 and info["out8"] == 1, info
    finally:
        ms.release()


# ---- the call is its definition ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_the_call_equals_its_definition_on_the_gpu(hip, seeded):
    """per frame: program, set_seed, the one-frame _copy8 list -- identical planes and registers"""
    names, pick, (w, h), fseed = M8.PLANAR_CASES["definition"]
    ms = Models(hip, names)
    try:
        frames = ms.frames(len(pick), fseed, w, h)
        seeds = M8.fresh_seeds(len(pick), 6) if seeded else None
        f0 = frames[0]
        fill = fill_for(f0, 9)
        src, dst = scattered(frames, 9), destinations(len(frames), fill, 9)
        regs0 = hip.seed_state()
        call(hip, src, dst, [ms.handles[k] for k in pick], seeds, f0, fill)
        got, regs = [d.download() for d in dst], hip.seed_state()
        # the definition, from the same registers
        dst2 = destinations(len(frames), fill, 10)
        U.program(hip, ms.recs[-1])
        assert hip.seed_state() == regs0          # (the library programmed with the model captured last, as in front of the call)
        for k, s, d, i in zip(pick, src, dst2, range(len(pick))):
            T.replay(hip, U.without_seed(ms.recs[k]))
            if seeds is not None:
                hip.set_seed(seeds[i])
            hip.add_grain_frame_list_copy8_dev([s.ptrs()], [d.ptrs()], w, h, f0.stride, f0.cstride, fill.stride, fill.cstride, stream_ptr())
        assert hip.seed_state() == regs
        for i, (a, d) in enumerate(zip(got, dst2)):
            assert a.equal_all(d.download()), i
    finally:
        ms.release()


def test_the_kernels_serve_both_masters(hip):
    """a models call, the programmed _copy8 list, a models call again on one stream: each matches its oracle, the programmed state --
    LUTs, parameters, mix -- is what it was, and both kinds of launch name the same kernel family"""
    names, pick, (w, h), fseed = M8.PLANAR_CASES["both_masters"]
    ms = Models(hip, names + ["fgs_sei_10_420"])          # programmed last: fgs_sei_10_420 (general luma)
    try:
        luts0, params0, mix0 = [hip.luts(c) for c in range(3)], hip.params(), [hip.chroma_mix(c) for c in (1, 2)]
        _, _, ora = run(hip, ms, pick, ms.frames(len(pick), fseed, w, h), None, shuffle=1)
        assert hip.last_launch_info()["kernel"] == kernel_of(ms, pick[-1])
        assert [hip.luts(c) for c in range(3)] == luts0 and hip.params() == params0 and [hip.chroma_mix(c) for c in (1, 2)] == mix0
        # the programmed list: the model programmed last, the registers the models call left
        T.replay(ora, U.without_seed(ms.recs[2]))
        frames = ms.frames(3, fseed + 10, w, h)
        grained = [f.copy() for f in frames]
        for g in grained:
            ora.add_grain_frame(g)
        fill = fill_for(frames[0], 2)
        src, dst = scattered(frames, 2), destinations(3, fill, 2)
        f0 = frames[0]
        hip.add_grain_frame_list_copy8_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], w, h, f0.stride, f0.cstride, fill.stride, fill.cstride, stream_ptr())
        check(src, dst, frames, [M8.narrowed_over(fill, g) for g in grained], "programmed:")
        info = hip.last_launch_info()
        assert hip.seed_state() == ora.seed_state() and info["kernel"] == "grain_rw_kernel<10,2,2,true,false,true,false,false>", info
        # ... and the models call continues the registers in turn
        run(hip, ms, [1, 0], ms.frames(2, fseed + 20, w, h), None, ora=ora, shuffle=3)
        assert [hip.luts(c) for c in range(3)] == luts0 and hip.params() == params0 and [hip.chroma_mix(c) for c in (1, 2)] == mix0
    finally:
        ms.release()


# ---- built models -----------------------------------------------------------------------------------------------------------------------

def test_built_models_are_taken_as_they_are(hip):
    """models from vfgs_hip_models_from_afgs1 and vfgs_hip_models_from_sei, one list (two forms: two runs), a seed per picture"""
    import test_gpu_models_from_afgs1 as A
    import test_gpu_models_from_sei as S
    an, sn = ["fgs_afgs1_test1_10_420", "fgs_afgs1_test9_10_420"], ["fgs_sei_10_420", "fgs_sei_ar_test1_10_420"]
    S.set_format(hip, 10, 2, 2, 0)
    acfg = [A.afgs1_of(n) for n in an]
    models = hip.models_from_afgs1(acfg, stream_ptr()) + hip.models_from_sei([S.sei_of(n) for n in sn], stream_ptr())
    try:
        recs = [U.model_records(n) for n in an + sn]
        pick = [0, 1, 3, 2, 2, 0]
        seeds = [A.fw().afgs1_seed(acfg[k]) if k < 2 else 1000 + i for i, k in enumerate(pick)]
        frames = [garbage_frame(264, 88, 10, 2, 2, 300 + i) for i in range(len(pick))]
        fill = fill_for(frames[0], 5)
        want, regs, _ = M8.expect_planar(recs, pick, frames, seeds, fill)
        src, dst = scattered(frames, 5), destinations(len(frames), fill, 5)
        n0 = U.launches(hip)
        call(hip, src, dst, [models[k] for k in pick], seeds, frames[0], fill)
        check(src, dst, frames, want)
        forms = [(i["one_y"], i["one_c"]) for i in map(hip.model_info, models)]
        assert hip.seed_state() == regs and U.launches(hip) - n0 == len(U.runs_of(forms, pick))
    finally:
        for m in models:
            hip.model_release(m)


# ---- an overlap region ------------------------------------------------------------------------------------------------------------------

def test_two_calls_inside_an_overlap_region(hip):
    names, pick, (w, h), fseed = M8.PLANAR_CASES["overlap_region"]
    ms = Models(hip, names)
    try:
        frames = ms.frames(len(pick), fseed, w, h)
        fill = fill_for(frames[0], 14)
        want, regs, _ = M8.expect_planar(ms.recs, pick, frames, None, fill)
        src, dst = scattered(frames, 14), destinations(len(frames), fill, 14)
        hm = [ms.handles[k] for k in pick]
        st = stream_ptr()
        hip.overlap_begin(st)
        call(hip, src[:4], dst[:4], hm[:4], None, frames[0], fill, st)
        call(hip, src[4:], dst[4:], hm[4:], None, frames[0], fill, st)
        hip.overlap_end(st)
        check(src, dst, frames, want)
        assert hip.seed_state() == regs
    finally:
        ms.release()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

REFUSALS = ["15_plane_reaches_the_2_gib_window", "18_null_source_list", "18_null_plane", "18_destination_listed_twice", "18_destinations_overlap", "18_source_of_another_frame", "7_misaligned_destination",
            "5_width", "6_source_stride", "8_source_pitch", "6_destination_stride", "6_destination_cstride", "8_destination_pitch", "16_depth_8",
            "16_depth_8_before_41", "41_null_models", "41_null_entry", "41_released_entry", "41_other_depth", "41_other_chroma_format", "41_width",
            "41_programmed_chroma_mix", "41_model_carries_a_mix"]


@pytest.mark.parametrize("case", REFUSALS)
def test_a_refusal_changes_nothing(hip, case):
    """each refusal with its code and its cause in the message; no byte written, no launch counted, registers and build stats unchanged;
    then the list is served"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_10_420"])
    extra, undo = [], (lambda: None)
    try:
        w, h = (8208, 17) if case == "41_width" else (520, 70)
        frames = ms.frames(3, 170, w, h)
        f0 = frames[0]
        fill = fill_for(f0, 77, 16, 32)
        src, dst = scattered(frames), destinations(3, fill)
        sp, dp = [d.ptrs() for d in src], [d.ptrs() for d in dst]
        hm = [ms.handles[0], ms.handles[1], ms.handles[0]]
        geo = dict(width=w, height=h, stride=f0.stride, cstride=f0.cstride, dst_stride=fill.stride, dst_cstride=fill.cstride)
        seeds = M8.fresh_seeds(3, 8)
        code, match, null_src = int(case.split("_")[0]), None, False
        n = 3
        if case == "15_plane_reaches_the_2_gib_window":
            # ONE picture of 1864136 rows x 576 samples x 2 bytes: refused before anything is touched, so its planes are addresses, 8 GiB apart.
            # The list checks find nothing; the destination pitch is too small (6) and the models are NULL (41) as well: 15 comes first.
            n, sp, dp, hm, match = 1, [(1 << 33, 2 << 33, 3 << 33)], [(4 << 33, 5 << 33, 6 << 33)], None, "2 GiB"
            geo.update(height=1864136, dst_stride=512)
        if case.startswith("15_"):
            pass
        elif case == "18_null_source_list":
            null_src, match = True, "null list"
        elif case == "18_null_plane":
            dp[1], match = (dp[1][0], 0, dp[1][2]), "null plane"
        elif case == "18_destination_listed_twice":
            dp[2], match = dp[0], "listed twice"
        elif case == "18_destinations_overlap":
            dp[1], match = (dp[1][0], dp[0][0] + 1024, dp[1][2]), "overlap"
        elif case == "18_source_of_another_frame":
            dp[1], match = (dp[1][0], sp[2][0] + 4096, dp[1][2]), "shares bytes"
        elif case == "7_misaligned_destination":
            dp[1], match = (dp[1][0], dp[1][1] + 8, dp[1][2]), "16-byte aligned"
        elif case == "5_width":
            geo["width"] = 100
        elif case == "6_source_stride":
            geo["stride"] = 512
        elif case == "8_source_pitch":
            geo["stride"] = f0.stride + 4
        elif case == "6_destination_stride":
            geo["dst_stride"], match = 512, "destination stride"
        elif case == "6_destination_cstride":
            geo["dst_cstride"], match = 256, "destination stride"
        elif case == "8_destination_pitch":
            geo["dst_cstride"], match = fill.cstride - 8, "multiples of 16"      # (still a row of whole blocks, and inside the allocation: the list checks find nothing)
        elif case in ("16_depth_8", "16_depth_8_before_41"):
            hip.set_depth(8)
            undo, match = (lambda: hip.set_depth(10)), "8-bit output"
            geo["stride"], geo["cstride"] = 2 * f0.stride, 2 * f0.cstride       # (the planes as they are, in 8-bit samples: the list checks come first)
            if case.endswith("41"):
                hm = None
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
            extra.append(Models(hip, ["fgs_afgs1_test3_10_422"]))
            U.program(hip, ms.recs[-1])
            hm[0], match = extra[0].handles[0], "chroma subsampling 2,1"
        elif case == "41_width":
            match = "width 8208"
        elif case == "41_programmed_chroma_mix":
            hip.set_chroma_mix(1, 32, 32, 0)
            undo, match = hip.clear_chroma_mix, "chroma mix"
        elif case == "41_model_carries_a_mix":
            U.program(hip, ms.recs[0])
            hip.set_chroma_mix(1, 32, 32, 0)
            extra.append(hip.model_capture_mix(stream_ptr()))
            hip.clear_chroma_mix()
            U.program(hip, ms.recs[-1])
            hm[2], match = extra[0], "chroma mix"
        st0, n0, b0 = hip.seed_state(), U.launches(hip), hip.model_build_stats()
        try:
            s, d = (None if null_src else hip.frame_list(sp)), hip.frame_list(dp)
            arr = None if hm is None else (C.c_void_p * 3)(*hm)
            rc = hip.lib.vfgs_hip_add_grain_frame_list_models_copy8_dev(s, d, arr, hip.seed_list(seeds[:n]), n, geo["width"], geo["height"], geo["stride"], geo["cstride"],
                                                                        geo["dst_stride"], geo["dst_cstride"], stream_ptr())
            assert rc == code and hip.lib.vfgs_hip_last_error() == code, (rc, hip.lib.vfgs_hip_last_error_string())
            assert match is None or match in hip.lib.vfgs_hip_last_error_string().decode(), hip.lib.vfgs_hip_last_error_string()
            if hm is not None and not null_src:
                with pytest.raises(VfgsHipError, match=f"error {code}"):          # ... and through the Python method
                    hip.add_grain_frame_list_models_copy8_dev(sp, dp, hm, seeds, *geo.values(), stream_ptr())
        finally:
            undo()
        assert hip.seed_state() == st0 and U.launches(hip) == n0 and hip.model_build_stats() == b0
        check(src, dst, frames, [fill] * 3, "after the refusal:")
        if case != "41_width":
            # the same list, its cause removed, is served
            pick = [0, 1, 0]
            want, regs, _ = M8.expect_planar(ms.recs, pick, frames, seeds, fill)
            call(hip, src, dst, [ms.handles[k] for k in pick], seeds, f0, fill)
            check(src, dst, frames, want)
            assert hip.seed_state() == regs
    finally:
        for x in [ms] + extra:
            x.release() if isinstance(x, Models) else hip.model_release(x)


def test_an_empty_list_is_no_call_at_all(hip):
    ms = Models(hip, ["fgs_afgs1_test1_10_420"])
    try:
        st0, n0 = hip.seed_state(), U.launches(hip)
        hip.add_grain_frame_list_models_copy8_dev([], [], [], None, 520, 70, 576, 288, 528, 272, stream_ptr())
        assert hip.lib.vfgs_hip_add_grain_frame_list_models_copy8_dev(None, None, None, None, 0, 100, 70, 0, 0, 0, 0, stream_ptr()) == 0
        assert hip.seed_state() == st0 and U.launches(hip) == n0
    finally:
        ms.release()
