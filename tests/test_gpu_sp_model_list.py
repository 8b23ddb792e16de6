"""GPU (MI355X): vfgs_hip_add_grain_sp_frame_list_models_dev -- semi-planar frames (NV12 / NV16 / P010 / P210 / P012) with a model per picture
in one launch (grain_spml_kernel) -- against the oracle, through the C ABI, bit for bit: every container of both planes of every frame,
padding included, and the four seed registers.

The contract (include/vfgs_hip.h) is a loop -- program the state models[f] was captured from; with seeds vfgs_set_seed(seeds[f]); the
one-frame semi-planar call on frame f -- so the ground truth is the oracle run as that loop (tests/sp_model_list_util.py, pinned against its
two parents' helpers by tests/test_sp_model_list_util_cpu.py).  Frames are separate allocations listed out of address order, with garbage
over the full container range in both planes.  Shapes are the smallest that reach each mechanism: a UV position is 2 KiB -- 1024 luma
samples of a row at 16-bit containers, 2048 at 8 bit."""
import ctypes as C

import numpy as np
import pytest

import model_list_util as U
import semiplanar_util as SP
import sp_model_list_util as SU
import vfgs_testlib as T
from gpu_util import stream_ptr
from test_gpu_semiplanar import DevSP, assert_equal, scattered

pytestmark = pytest.mark.gpu

W, H = 1032, 90      # 65 blocks x 6 block rows, the last one ragged


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


class Models:
    """models captured in turn from named programs (tests/model_list_util.py: a trace, a trace@depth12, a generated program) or from
    records given as they are; the library stays programmed with the last one"""

    def __init__(self, hip, programs, stream=None):
        self.hip = hip
        self.recs = [U.model_records(p) if isinstance(p, str) else list(p) for p in programs]
        self.handles = U.capture_all(hip, self.recs, stream_ptr() if stream is None else stream)
        self.info = [hip.model_info(m) for m in self.handles]
        self.forms = [(i["one_y"], i["one_c"]) for i in self.info]
        self.depth, self.sx, self.sy = T.trace_geometry(self.recs[-1])
        assert self.sx == 2

    def release(self):
        for m in self.handles:
            self.hip.model_release(m)

    def frames(self, n, seed, w=W, h=H, shift=0):
        return [SP.garbage_sp_frame(w, h, self.depth, self.sy, shift, seed + i) for i in range(n)]

    def kernel(self, k):
        return T.kernel_name("grain_spml_kernel", self.depth, self.sy, *self.forms[k])


def fresh_seeds(n, seed):
    return [int(s) for s in np.random.default_rng(seed).integers(0, 1 << 32, n)]


def call(hip, src, dst, models, seeds, f0, stream=None):
    hip.add_grain_sp_frame_list_models_dev(src, dst, models, seeds, f0.width, f0.height, f0.stride, f0.uv_stride, f0.shift,
                                           stream_ptr() if stream is None else stream)


def check(dev, want):
    for i, (d, w) in enumerate(zip(dev, want)):
        assert_equal(d.download(), w, f"frame {i}")


def run(hip, ms, pick, frames, seeds=None, ora=None, shuffle=0, out_of_place=False, stream=None):
    """the list through the call vs the contract's loop; returns (device frames that hold the result, the oracle of an unseeded run)"""
    f0 = frames[0]
    if seeds is not None:
        want, regs = SU.expect_seeded(ms.recs, pick, frames, seeds, f0.shift)
    else:
        ora = ora or U.oracle_programmed(ms.recs[-1])
        want, regs = SU.expect_unseeded(ora, ms.recs, pick, frames, f0.shift)
    src = scattered(frames, shuffle)
    models = [ms.handles[k] for k in pick]
    if out_of_place:
        fill = SP.garbage_sp_frame(f0.width, f0.height, f0.depth, f0.suby, f0.shift, 999)
        dst = [DevSP(fill) for _ in frames]
        dst[1] = src[1]                                # one pair in place
        call(hip, [d.ptrs() for d in src], [d.ptrs() for d in dst], models, seeds, f0, stream)
        rows, crows, cols = SP.written_region(f0)
        for i, (s, d, w, f) in enumerate(zip(src, dst, want, frames)):
            g = d.download()
            if i == 1:
                assert_equal(g, w, "the pair in place")
                continue
            e = fill.copy()
            e.Y[:rows, :cols] = w.Y[:rows, :cols]
            e.UV[:crows, :cols] = w.UV[:crows, :cols]
            assert_equal(g, e, f"destination {i}")     # what is written, and the padding as it was
            assert_equal(s.download(), f, f"source {i}")
        dev = dst
    else:
        call(hip, [d.ptrs() for d in src], None, models, seeds, f0, stream)
        check(src, want)
        dev = src
    assert hip.seed_state() == regs
    return dev, ora


# ---- every class ------------------------------------------------------------------------------------------------------------------

CONFIGS = {
    "8_420_one": ["fgs_afgs1_test1_8_420", "fgs_afgs1_test9_8_420"],
    "8_420_general": ["fgs_sei_8_420", "fgs_sei_ff_test6_8_420"],
    "8_422": ["fgs_sei_8_422", "fgs_sei_ff_test6_8_422"],
    "10_420_one": ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"],
    "10_420_general": ["fgs_sei_10_420", "default_10_420", "fgs_sei_ff_test6_10_420"],
    "10_422": ["fgs_sei_10_422", "fgs_afgs1_test3_10_422"],
    "12_420": ["fgs_sei_10_420@depth12", "fgs_afgs1_test1_10_420@depth12"],
    # generated programs (tests/model_programs.py) for the two forms the traces do not have, each beside a trace of its depth and format
    "10_420_one_y_general_c": ["one_y_general_c_10_420", "fgs_sei_10_420"],
    "8_422_general_y_one_c": ["general_y_one_c_8_422", "fgs_sei_8_422"],
}


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("out_of_place", [False, True], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_every_class(hip, cfg, out_of_place, seeded):
    """7 frames of 1032 x 90, models A B A B ..., low-aligned samples"""
    ms = Models(hip, CONFIGS[cfg])
    try:
        n = 7
        pick = [i % len(ms.handles) for i in range(n)]
        frames = ms.frames(n, 10)
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, fresh_seeds(n, 1) if seeded else None, shuffle=1, out_of_place=out_of_place)
        info = hip.last_launch_info()
        runs = U.runs_of(ms.forms, pick)
        assert info["launches"] - n0 == len(runs) and info["nframes"] == runs[-1] and info["listed"] == 1, (info, runs)
        assert info["kernel"] == ms.kernel(pick[-1]), info
        assert info["in_place"] == (0 if out_of_place else 1) and info["persistent_luma_workgroups"] == 0 and info["depth"] == ms.depth
    finally:
        ms.release()


def test_all_four_forms(hip):
    """general / one-pattern luma over general / one-pattern chroma: each form's kernel is launched and named"""
    seen = {}
    for name in ("general_runs_8_420", "fgs_sei_10_420", "one_y_general_c_10_420", "general_y_one_c_8_422", "fgs_afgs1_test1_10_420"):
        ms = Models(hip, [name])
        try:
            run(hip, ms, [0, 0, 0], ms.frames(3, 20), None)
            info = hip.last_launch_info()
            assert info["kernel"] == ms.kernel(0), info
            seen[ms.forms[0]] = info["kernel"]
        finally:
            ms.release()
    assert set(seen) == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen
    assert all(k.startswith("grain_spml_kernel<") for k in seen.values()), seen


# ---- per-frame bounds and shift in the UV workgroup -----------------------------------------------------------------------------------

def second_model(rec):
    """`rec` with halved scale LUTs and the other range behind it, as tools/sp_model_list_bench.py builds its second model, and another scale
    shift on top: the same patterns and pattern LUTs, so the same form, and a record that differs in lo2 / hi2 and pk_shift"""
    slut, shift, legal = {}, None, 0
    for op, a, b, p in rec:
        if op == T.OP_SCALE_LUT:
            slut[a] = bytes(p)
        elif op == T.OP_SCALE_SHIFT:
            shift = a
        elif op == T.OP_LEGAL_RANGE:
            legal = a
    assert len(slut) == 3 and shift is not None
    more = [(T.OP_SCALE_LUT, c, 0, bytes(v >> 1 for v in slut[c])) for c in range(3)]
    more += [(T.OP_LEGAL_RANGE, 0 if legal else 1, 0, b""), (T.OP_SCALE_SHIFT, shift + 1 if shift < 7 else shift - 1, 0, b"")]
    return list(rec) + more


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("name", ["fgs_afgs1_test1_8_420", "fgs_afgs1_test1_10_420", "fgs_sei_10_422"], ids=["8bit_packed", "10bit", "10bit_422_general"])
def test_bounds_and_shift_are_the_frames_own(hip, name, seeded):
    """two models of one form that differ only in range, scale shift and scale LUTs, B A A B A B B: ONE launch, and a workgroup -- luma or
    UV -- that took frame 0's record would clip with the wrong bounds (the garbage content lies mostly outside the legal range) and, in the
    8-bit packed form, scale with the wrong shift on every frame of the other model"""
    rec = U.model_records(name)
    ms = Models(hip, [rec, second_model(rec)])
    try:
        assert ms.forms[0] == ms.forms[1], ms.forms
        assert ms.info[0]["scale_shift"] != ms.info[1]["scale_shift"] and ms.info[0]["legal_range"] != ms.info[1]["legal_range"], ms.info
        pick = [1, 0, 0, 1, 0, 1, 1]
        frames = ms.frames(len(pick), 30)
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, fresh_seeds(len(pick), 2) if seeded else None, shuffle=2)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 1 and info["nframes"] == len(pick) and info["kernel"] == ms.kernel(0), info
        # (the two models do differ on these frames: the same frame through the other model is another picture)
        a, _ = SU.expect_seeded(ms.recs, [0], frames[:1], [5], 0)
        b, _ = SU.expect_seeded(ms.recs, [1], frames[:1], [5], 0)
        assert not np.array_equal(a[0].UV, b[0].UV) and not np.array_equal(a[0].Y, b[0].Y)
    finally:
        ms.release()


# ---- high-aligned samples ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("names", [["fgs_sei_10_420", "default_10_420"], ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"], ["fgs_sei_10_422", "fgs_afgs1_test3_10_422"],
                                   ["fgs_sei_10_420@depth12", "fgs_afgs1_test1_10_420@depth12"]], ids=["p010_general", "p010_one", "p210", "p012"])
def test_high_aligned_samples(hip, names):
    """P010 / P210 (shift 6) and P012 (shift 4): the sources' low bits are random and ignored, the written containers' low bits are zero"""
    ms = Models(hip, names)
    try:
        shift = 16 - ms.depth
        planar, _ = T.lcg_frames(W, H, ms.depth, 2, ms.sy, 4)
        frames = [SP.to_semiplanar(f, shift, low_bits_seed=40 + i) for i, f in enumerate(planar)]
        assert all((f.Y & ((1 << shift) - 1)).any() and (f.UV & ((1 << shift) - 1)).any() for f in frames)
        dev, _ = run(hip, ms, [0, 1, 1, 0], frames, None, shuffle=3)
        rows, crows, cols = SP.written_region(frames[0])
        for d in dev:
            g = d.download()
            assert not (g.Y[:rows, :cols] & ((1 << shift) - 1)).any() and not (g.UV[:crows, :cols] & ((1 << shift) - 1)).any()
        # ... and garbage over the whole container, seeded, out of place
        run(hip, ms, [1, 0, 1], ms.frames(3, 50, shift=shift), fresh_seeds(3, 3), shuffle=4, out_of_place=True)
    finally:
        ms.release()


# ---- row geometry -------------------------------------------------------------------------------------------------------------------

WIDTHS = [136, 1016, 1024, 1032, 2056, 4104, 8192]
HEIGHTS = [17, 33, 70]
GROUPS = {"8bit": ["fgs_afgs1_test1_8_420", "fgs_afgs1_test9_8_420"], "10bit": ["fgs_sei_10_420", "default_10_420"],
          "422": ["fgs_sei_ff_test6_8_422", "fgs_sei_8_422"]}
GROUP_422_10BIT = ["fgs_sei_10_422", "fgs_afgs1_test3_10_422"]
# every width with a height in turn, in every group (21 combinations; every height at least twice a group); the 4:2:2 group alternates its
# depth through the widths
GEOMETRY = [(g, w, HEIGHTS[(i + k) % 3]) for k, g in enumerate(GROUPS) for i, w in enumerate(WIDTHS)]


@pytest.mark.parametrize("group,width,height", GEOMETRY)
def test_row_geometry(hip, group, width, height):
    """3 frames, two models: 1016 / 1024 / 1032 straddle the 2 KiB UV position at 16-bit containers, 2056 at 8 bit"""
    names = GROUPS[group]
    if group == "422" and WIDTHS.index(width) % 2:
        names = GROUP_422_10BIT
    ms = Models(hip, names)
    try:
        run(hip, ms, [0, 1, 0], ms.frames(3, width + height, width, height), None, shuffle=2)
        info = hip.last_launch_info()
        unit_samples = 64 * 32 // (2 if ms.depth > 8 else 1)     # containers of a UV position
        nblk = (width + 15) // 16
        assert info["positions_per_row"][1] == (-(-nblk * 16 // (unit_samples // 64)) + 64) // 64, info
        assert info["kernel"] == ms.kernel(0), info      # (the 4:2:2 pairs differ in form: their lists are three launches)
    finally:
        ms.release()


def test_geometry_covers_every_width_and_height_in_every_group():
    assert len(GEOMETRY) == 21
    for g in GROUPS:
        assert {w for gg, w, _ in GEOMETRY if gg == g} == set(WIDTHS) and {h for gg, _, h in GEOMETRY if gg == g} == set(HEIGHTS)


# ---- more frames than a launch holds, form changes --------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_more_frames_than_one_launch_holds(hip, seeded):
    """35 frames of 136 x 33, two models of one form alternating: launches of 32 + 3"""
    ms = Models(hip, ["fgs_afgs1_test1_8_420", "fgs_afgs1_test9_8_420"])
    try:
        pick = [i & 1 for i in range(35)]
        n0 = U.launches(hip)
        run(hip, ms, pick, ms.frames(35, 700, 136, 33), fresh_seeds(35, 4) if seeded else None, shuffle=4)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 2 and info["nframes"] == 3, info
    finally:
        ms.release()


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_forms_change_inside_the_list(hip, seeded):
    """X X Y X with X general luma, Y one-pattern: three launches, each with its slice of the frames (and of the seeds)"""
    ms = Models(hip, ["fgs_sei_10_420", "fgs_afgs1_test1_10_420"])
    try:
        assert ms.forms[0] != ms.forms[1]
        pick = [0, 0, 1, 0]
        n0 = U.launches(hip)
        run(hip, ms, pick, ms.frames(4, 40, shift=6), fresh_seeds(4, 3) if seeded else None, shuffle=3)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 3 and info["nframes"] == 1 and info["kernel"] == ms.kernel(0), info
    finally:
        ms.release()


# ---- the seed sequence and the programmed state ---------------------------------------------------------------------------------------

def plain_sp_list(hip, ora, frames, seeds=None):
    """the plain semi-planar call, in place, against `ora` as it stands"""
    want = SP.expected(ora, frames, seeds, frames[0].shift)
    dev = scattered(frames, 5)
    f0 = frames[0]
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, seeds, f0.width, f0.height, f0.stride, f0.uv_stride, f0.shift, stream_ptr())
    check(dev, want)
    assert hip.seed_state() == ora.seed_state()


def test_the_seed_sequence_continues_across_calls(hip):
    """a plain semi-planar list, the models call, a plain list, the models call: one sequence of registers"""
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"])
    try:
        ora = U.oracle_programmed(ms.recs[-1])
        plain_sp_list(hip, ora, ms.frames(2, 60, 520, 70, 6))
        run(hip, ms, [0, 1, 0], ms.frames(3, 70, 520, 70, 6), None, ora=ora, shuffle=6)
        T.replay(ora, U.without_seed(ms.recs[-1]))      # (the library is still programmed with the model captured last)
        plain_sp_list(hip, ora, ms.frames(2, 80, 520, 70, 6))
        assert hip.last_launch_info()["kernel"].startswith("grain_sp_kernel<")
        run(hip, ms, [1, 1], ms.frames(2, 90, 520, 70, 6), None, ora=ora, shuffle=7)
    finally:
        ms.release()


def test_the_programmed_state_is_untouched(hip):
    """the following plain call grains with the model programmed last (general luma), not the one listed last (one-pattern)"""
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"])      # programmed last: fgs_sei_10_420
    try:
        luts0, params0 = [hip.luts(c) for c in range(3)], hip.params()
        _, ora = run(hip, ms, [0, 1, 0, 1, 1], ms.frames(5, 90, 520, 70), None, shuffle=9)
        assert hip.last_launch_info()["kernel"] == ms.kernel(1)
        assert [hip.luts(c) for c in range(3)] == luts0 and hip.params() == params0
        T.replay(ora, U.without_seed(ms.recs[2]))
        plain_sp_list(hip, ora, ms.frames(2, 100, 520, 70))
        info = hip.last_launch_info()
        assert info["kernel"] == "grain_sp_kernel<10,2,false,true>" and ms.forms[1] == (1, 1), info
    finally:
        ms.release()


# ---- streams ------------------------------------------------------------------------------------------------------------------------

def test_capture_on_one_stream_use_on_another_release_right_after_the_call(hip):
    import torch
    from versatilefilmgrain_amd.hw import VfgsHipError
    other, third = torch.cuda.Stream(), torch.cuda.Stream()
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"], stream=other.cuda_stream)     # captured on one stream ...
    pick = [0, 1, 0, 1, 1, 0, 1]
    frames = ms.frames(7, 140, 520, 70, 6)
    seeds = fresh_seeds(7, 7)
    want, regs = SU.expect_seeded(ms.recs, pick, frames, seeds, 6)
    dev = scattered(frames, 13)
    torch.cuda.synchronize()        # (the frames are there; nothing else orders the streams)
    call(hip, [d.ptrs() for d in dev], None, [ms.handles[k] for k in pick], seeds, frames[0], third.cuda_stream)      # ... used on another
    ms.release()                    # as soon as the call has returned
    assert hip.seed_state() == regs
    # captures that follow (they program the library anew) take buffers of their own while the released ones may still be read ...
    ms2 = Models(hip, ["fgs_sei_10_420", "default_10_420"], stream=other.cuda_stream)
    try:
        torch.cuda.synchronize()
        check(dev, want)
        with pytest.raises(VfgsHipError, match="error 41"):
            hip.model_info(ms.handles[0])
        # ... and are used in turn
        run(hip, ms2, [1, 0, 1], ms2.frames(3, 150, 520, 70, 6), fresh_seeds(3, 8), shuffle=14, stream=third.cuda_stream)
    finally:
        ms2.release()


def test_two_calls_inside_an_overlap_region(hip):
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"])
    try:
        a, b = ms.frames(4, 150, 520, 70, 6), ms.frames(3, 160, 520, 70, 6)
        pick = [0, 1, 1, 0, 1, 0, 0]
        ora = U.oracle_programmed(ms.recs[-1])
        want, regs = SU.expect_unseeded(ora, ms.recs, pick, a + b, 6)
        da, db = scattered(a, 14), scattered(b, 15)
        st = stream_ptr()
        hm = [ms.handles[k] for k in pick]
        hip.overlap_begin(st)
        call(hip, [d.ptrs() for d in da], None, hm[:4], None, a[0], st)
        call(hip, [d.ptrs() for d in db], None, hm[4:], None, a[0], st)
        hip.overlap_end(st)
        check(da + db, want)
        assert hip.seed_state() == regs
    finally:
        ms.release()


def test_two_frame_fronts(hip):
    """three P010 frames of 8192 x 1366 (tests/test_gpu_semiplanar.py::test_two_frame_fronts), models A B A: frames 2m and 2m + 1 are swept
    together, each with its own model"""
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"])
    try:
        run(hip, ms, [0, 1, 0], ms.frames(3, 50, 8192, 1366, 6), None, shuffle=5)
        info = hip.last_launch_info()
        assert info["frames_per_front"] == 2 and info["nframes"] == 3, info
    finally:
        ms.release()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

REFUSALS = ["40_csubx", "40_sample_shift", "40_sample_shift_at_depth_8", "40_width", "41_null_models", "41_null_entry", "41_released_entry", "41_other_depth",
            "41_other_chroma_format", "41_chroma_mix", "18_uv_overlaps_another_frames_y", "7_misaligned_plane"]


@pytest.mark.parametrize("case", REFUSALS)
def test_a_refusal_changes_nothing(hip, case):
    """each refusal alone, with its code and its cause in the message; afterwards the registers, the launch count and every container of
    the sources and the destinations are what they were; then the list is served"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_10_420"])
    extra = []
    try:
        w, h = (8208, 17) if case == "40_width" else (520, 70)
        frames = ms.frames(3, 170, w, h, 6)
        fill = SP.garbage_sp_frame(w, h, 10, 2, 6, 998)
        dev, out = scattered(frames), [DevSP(fill) for _ in frames]
        f0 = frames[0]
        ptrs, optrs = [d.ptrs() for d in dev], [d.ptrs() for d in out]
        hm = [ms.handles[0], ms.handles[1], ms.handles[0]]
        seeds = fresh_seeds(3, 8)
        shift, code, match = 6, int(case.split("_")[0]), None
        undo = lambda: None
        if case == "40_csubx":
            hip.set_chroma_subsampling(1, 2)       # (4:4:0: the chroma rows of the planes as they are -- the list checks come first)
            undo, match = (lambda: hip.set_chroma_subsampling(2, 2)), "csubx 1"
        elif case == "40_sample_shift":
            shift, match = 4, "sample_shift 4 at depth 10"
        elif case == "40_sample_shift_at_depth_8":
            hip.set_depth(8)
            undo, match = (lambda: hip.set_depth(10)), "sample_shift 6 at depth 8"
        elif case == "40_width":
            match = "width 8208"
        elif case == "41_null_models":
            hm, match = None, "null list of models"
        elif case == "41_null_entry":
            hm[1], match = None, "frame 1 is null"
        elif case == "41_released_entry":
            gone = Models(hip, ["fgs_sei_10_420"])
            gone.release()
            hm[2], match = gone.handles[0], "frame 2 is not a live model"
        elif case == "41_other_depth":
            extra.append(Models(hip, ["fgs_afgs1_test1_8_420"]))
            U.program(hip, ms.recs[-1])
            hm[1], match = extra[0].handles[0], "captured at depth 8"
        elif case == "41_other_chroma_format":
            extra.append(Models(hip, ["fgs_afgs1_test3_10_422"]))
            U.program(hip, ms.recs[-1])
            hm[0], match = extra[0].handles[0], "chroma subsampling 2,1"
        elif case == "41_chroma_mix":
            hip.set_chroma_mix(1, 32, 32, 0)
            undo, match = hip.clear_chroma_mix, "chroma mix"
        elif case == "18_uv_overlaps_another_frames_y":
            optrs[1] = (optrs[1][0], optrs[0][0] + 1024 * f0.Y.itemsize)
            match = "overlap"
        elif case == "7_misaligned_plane":
            optrs[1] = (optrs[1][0], optrs[1][1] + 8)
            match = "16-byte aligned"
        st0, n0 = hip.seed_state(), U.launches(hip)
        try:
            s, d = hip.sp_frame_list(ptrs), hip.sp_frame_list(optrs)
            arr = None if hm is None else (C.c_void_p * 3)(*hm)
            rc = hip.lib.vfgs_hip_add_grain_sp_frame_list_models_dev(s, d, arr, hip.seed_list(seeds), 3, f0.width, f0.height, f0.stride, f0.uv_stride, shift, stream_ptr())
            assert rc == code and hip.lib.vfgs_hip_last_error() == code, (rc, hip.lib.vfgs_hip_last_error_string())
            assert match in hip.lib.vfgs_hip_last_error_string().decode(), hip.lib.vfgs_hip_last_error_string()
            if hm is not None:
                with pytest.raises(VfgsHipError, match=f"error {code}"):          # ... and through the Python method
                    hip.add_grain_sp_frame_list_models_dev(ptrs, optrs, hm, seeds, f0.width, f0.height, f0.stride, f0.uv_stride, shift, stream_ptr())
        finally:
            undo()
        assert hip.seed_state() == st0 and U.launches(hip) == n0
        for dd, f in zip(dev + out, frames + [fill] * 3):
            assert_equal(dd.download(), f)
        if case != "40_width":
            # the same list, its cause removed, is served
            good = [ms.handles[0], ms.handles[1], ms.handles[0]]
            want, regs = SU.expect_seeded(ms.recs, [0, 1, 0], frames, seeds, 6)
            call(hip, ptrs, None, good, seeds, f0)
            check(dev, want)
            assert hip.seed_state() == regs
    finally:
        for x in [ms] + extra:
            x.release()


def test_an_empty_list_is_no_call_at_all(hip):
    ms = Models(hip, ["fgs_afgs1_test1_10_420"])
    try:
        st0, n0 = hip.seed_state(), U.launches(hip)
        hip.add_grain_sp_frame_list_models_dev([], None, [], None, 520, 70, 576, 576, 6, stream_ptr())
        hip.add_grain_sp_frame_list_models_dev([], [], [], [], 520, 70, 576, 576, 6, stream_ptr())
        assert hip.lib.vfgs_hip_add_grain_sp_frame_list_models_dev(None, None, None, None, 0, 100, 70, 0, 0, 99, stream_ptr()) == 0
        assert hip.seed_state() == st0 and U.launches(hip) == n0
    finally:
        ms.release()
