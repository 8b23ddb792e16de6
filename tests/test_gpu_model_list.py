"""GPU (MI355X): film grain models as device objects -- vfgs_hip_model_capture and vfgs_hip_add_grain_frame_list_models_dev, a model per
picture in one launch -- against the oracle, through the C ABI, bit for bit (every sample of every plane, padding included, and the four
seed registers).

The contract (include/vfgs_hip.h) is a loop -- program the state models[f] was captured from; with seeds vfgs_set_seed(seeds[f]); grain
frame f -- so the ground truth is the oracle run as that loop (tests/model_list_util.py).  Every frame is an allocation of its own, listed
out of address order (the helpers of tests/test_gpu_frame_list.py)."""
import numpy as np
import pytest

import model_list_util as U
import vfgs_testlib as T
from gpu_util import DevFrame, stream_ptr
from test_gpu_frame_list import garbage_frame, scattered

pytestmark = pytest.mark.gpu

W, H = 1032, 90      # 65 blocks x 6 block rows


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


class Models:
    """the named models, captured in turn; the library stays programmed with the last one"""

    def __init__(self, hip, names, stream=None):
        self.hip, self.names = hip, list(names)
        self.recs = [U.model_records(n) for n in names]
        self.handles = U.capture_all(hip, self.recs, stream_ptr() if stream is None else stream)
        self.info = [hip.model_info(m) for m in self.handles]
        self.forms = [(i["one_y"], i["one_c"]) for i in self.info]
        self.depth, self.sx, self.sy = T.trace_geometry(self.recs[-1])

    def release(self):
        for m in self.handles:
            self.hip.model_release(m)

    def frames(self, n, seed, w=W, h=H):
        return [garbage_frame(w, h, self.depth, self.sx, self.sy, seed + i) for i in range(n)]


def fresh_seeds(n, seed):
    return [int(s) for s in np.random.default_rng(seed).integers(0, 1 << 32, n)]


def check(dev, want):
    for i, (d, w) in enumerate(zip(dev, want)):
        assert d.download().equal_all(w), i


def run(hip, ms, pick, frames, seeds=None, ora=None, shuffle=0, out_of_place=False, stream=None):
    """the list through the call vs the contract's loop; returns (device frames that hold the result, the oracle of an unseeded run)"""
    if seeds is not None:
        want, regs = U.expect_seeded(ms.recs, pick, frames, seeds)
    else:
        ora = ora or U.oracle_programmed(ms.recs[-1])
        want, regs = U.expect_unseeded(ora, ms.recs, pick, frames)
    src = scattered(frames, shuffle)
    f0 = frames[0]
    models = [ms.handles[k] for k in pick]
    st = stream_ptr() if stream is None else stream
    if out_of_place:
        blank = T.Frame(f0.width, f0.height, f0.depth, f0.subx, f0.suby)
        dst = [DevFrame(blank) for _ in frames]
        dst[1] = src[1]                                # one pair in place
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], models, seeds, f0.width, f0.height, f0.stride, f0.cstride, st)
        cy, sx, sy, h = (f0.width + 15) // 16 * 16, f0.subx, f0.suby, f0.height
        for i, (s, d, w, f) in enumerate(zip(src, dst, want, frames)):
            g = d.download()
            if i == 1:
                assert g.equal_all(w)
                continue
            assert np.array_equal(g.Y[:h, :cy], w.Y[:h, :cy]) and np.array_equal(g.U[:h // sy, :cy // sx], w.U[:h // sy, :cy // sx]) \
                and np.array_equal(g.V[:h // sy, :cy // sx], w.V[:h // sy, :cy // sx]), i
            assert not g.Y[:, cy:].any() and not g.Y[h:].any() and not g.U[:, cy // sx:].any() and not g.V[h // sy:].any(), i     # the destination's padding is never written
            assert s.download().equal_all(f), i         # the sources stay as they were
        dev = dst
    else:
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in src], None, models, seeds, f0.width, f0.height, f0.stride, f0.cstride, st)
        check(src, want)
        dev = src
    assert hip.seed_state() == regs
    return dev, ora


CONFIGS = {
    "8_420": ["fgs_afgs1_test1_8_420", "fgs_afgs1_test9_8_420"],
    "10_420": ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"],
    "10_420_general": ["fgs_sei_10_420", "default_10_420", "fgs_sei_ff_test6_10_420"],
    "10_422": ["fgs_sei_10_422", "fgs_afgs1_test3_10_422"],
    "10_444": ["fgs_sei_10_444", "fgs_sei_ff_test6_10_444", "fgs_afgs1_test1_10_444"],
    "8_444": ["fgs_afgs1_test1_8_444", "fgs_sei_ff_test6_8_444"],
    "10_440": ["fgs_sei_10_440", "fgs_sei_ff_test6_10_440"],
    "8_440": ["fgs_afgs1_test1_8_440", "fgs_afgs1_test1_8_440"],
    "12_420": ["fgs_sei_10_420@depth12", "fgs_afgs1_test1_10_420@depth12"],
}


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("out_of_place", [False, True], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_every_depth_and_format(hip, cfg, out_of_place, seeded):
    ms = Models(hip, CONFIGS[cfg])
    try:
        n = 7
        pick = [i % len(ms.handles) for i in range(n)]     # A B A B ...
        frames = ms.frames(n, 10)
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, fresh_seeds(n, 1) if seeded else None, shuffle=1, out_of_place=out_of_place)
        info = hip.last_launch_info()
        runs = U.runs_of(ms.forms, pick)
        assert info["launches"] - n0 == len(runs) and info["nframes"] == runs[-1] and info["listed"] == 1, (info, runs)
        oy, oc = ms.forms[pick[-1]]
        b = lambda v: "true" if v else "false"
        assert info["kernel"] == f"grain_ml_kernel<{ms.depth},{ms.sx},{ms.sy},{b(oy)},{b(oc)}>", info
        assert info["in_place"] == (0 if out_of_place else 1) and info["persistent_luma_workgroups"] == 0
    finally:
        ms.release()


def test_the_models_span_three_forms(hip):
    ms = Models(hip, ["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_ff_test6_10_420", "default_10_420"])
    try:
        assert len(set(ms.forms)) >= 3, ms.forms
        assert ms.forms[0] == (0, 1) and ms.forms[1] == (1, 1), ms.forms       # general luma over one-pattern chroma; all one-pattern
        for i, rec in zip(ms.info, ms.recs):
            assert (i["depth"], i["csubx"], i["csuby"]) == (10, 2, 2) and i["device_bytes"] > 4096, i
        assert ms.info[1]["legal_range"] == 1 and ms.info[0]["legal_range"] == 0
        assert ms.info[2]["scale_shift"] == ms.info[1]["scale_shift"] - 1       # (4 against 5, as stored)
    finally:
        ms.release()


@pytest.mark.parametrize("names", [["fgs_afgs1_test1_10_420", "fgs_afgs1_test9_10_420", "fgs_afgs1_test2_10_420"],
                                   ["fgs_afgs1_test1_8_420", "fgs_afgs1_test9_8_420", "fgs_afgs1_test2_8_420"]], ids=["10bit", "8bit_packed"])
@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_same_form_different_content_in_one_launch(hip, names, seeded):
    """AFGS1 models with other scale LUTs, another scale shift (test9: 4, the others 5) and the legal range on (test1) and off: one launch;
    a workgroup that took frame 0's clip bounds or shift would be wrong on every other frame.  At 8 bit the packed 16-bit form reads the shift."""
    ms = Models(hip, names)
    try:
        assert len(set(ms.forms)) == 1 and ms.forms[0] == (1, 1), ms.forms
        assert len({i["scale_shift"] for i in ms.info}) == 2 and {i["legal_range"] for i in ms.info} == {0, 1}, ms.info
        pick = [0, 1, 2, 1, 0, 2, 2, 1, 0]
        frames = ms.frames(len(pick), 30)
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, fresh_seeds(len(pick), 2) if seeded else None, shuffle=2)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 1 and info["nframes"] == len(pick), info
    finally:
        ms.release()


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
def test_forms_change_inside_the_list(hip, seeded):
    """A A B B B A with A general, B one-pattern: three launches, each with its slice of the frames (and of the seeds)"""
    ms = Models(hip, ["fgs_sei_10_420", "fgs_afgs1_test1_10_420"])
    try:
        pick = [0, 0, 1, 1, 1, 0]
        frames = ms.frames(6, 40)
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, fresh_seeds(6, 3) if seeded else None, shuffle=3)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 3 and info["nframes"] == 1 and info["kernel"] == "grain_ml_kernel<10,2,2,false,true>", info
    finally:
        ms.release()


def test_more_frames_than_one_launch_holds(hip):
    """70 frames, two models of one form alternating: launches of 32 + 32 + 6"""
    ms = Models(hip, ["fgs_afgs1_test1_8_420", "fgs_afgs1_test9_8_420"])
    try:
        pick = [i & 1 for i in range(70)]
        frames = ms.frames(70, 700, 264, 40)
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, None, shuffle=4)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 3 and info["nframes"] == 6, info
        frames = ms.frames(70, 800, 264, 40)
        run(hip, ms, pick, frames, fresh_seeds(70, 4), shuffle=5)
    finally:
        ms.release()


def test_two_frame_fronts(hip):
    """4320p x 3, models A B A: frames 2m and 2m + 1 are swept together, each with its own model"""
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"])
    try:
        frames = ms.frames(3, 50, 7680, 4320)
        run(hip, ms, [0, 1, 0], frames, None, shuffle=5)
        info = hip.last_launch_info()
        assert info["frames_per_front"] == 2 and info["nframes"] == 3, info
    finally:
        ms.release()


@pytest.mark.parametrize("width,positions", [(1920, 2), (960, 1)])
def test_narrow_chroma_rows(hip, width, positions):
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"])
    try:
        pick = [0, 1, 1, 0, 1, 2, 2]
        frames = ms.frames(len(pick), 70, width, 48)
        run(hip, ms, pick, frames, None, shuffle=7)          # (first: its oracle begins at the registers of the model programmed last)
        assert hip.last_launch_info()["positions_per_row"][1] == positions
        frames = ms.frames(len(pick), 60, width, 48)
        run(hip, ms, pick, frames, fresh_seeds(len(pick), 5), shuffle=6)
        assert hip.last_launch_info()["positions_per_row"][1] == positions
    finally:
        ms.release()


def test_firmware_programmed_models(hip):
    """vfgs_init_sei / vfgs_init_afgs1 on two recorded configurations -- patterns generated on the device, which capture patches into the
    model's image there -- capturing after each; expected: the oracle replaying the traces of the same names"""
    from test_gpu_fw import program_by_firmware
    names = ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"]
    handles = []
    for n in names:
        program_by_firmware(hip, n)
        handles.append(hip.model_capture(stream_ptr()))
    try:
        recs = [U.model_records(n) for n in names]
        assert [hip.model_info(m)["one_y"] for m in handles] == [1, 1]
        pick = [0, 1, 1, 0, 1]
        frames = [garbage_frame(W, H, 10, 2, 2, 80 + i) for i in range(5)]
        seeds = fresh_seeds(5, 6)
        want, regs = U.expect_seeded(recs, pick, frames, seeds)
        dev = scattered(frames, 8)
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev], None, [handles[k] for k in pick], seeds, W, H, frames[0].stride, frames[0].cstride, stream_ptr())
        check(dev, want)
        assert hip.seed_state() == regs
        assert hip.last_launch_info()["nframes"] == 5
    finally:
        for m in handles:
            hip.model_release(m)


def test_the_programmed_state_survives(hip):
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"])      # programmed last: fgs_sei_10_420
    try:
        luts0, params0 = [hip.luts(c) for c in range(3)], hip.params()
        pick = [0, 1, 0, 1, 1]
        _, ora = run(hip, ms, pick, ms.frames(5, 90), None, shuffle=9)
        assert [hip.luts(c) for c in range(3)] == luts0 and hip.params() == params0
        # a plain frame call: the model programmed last, the registers the list left
        T.replay(ora, U.without_seed(ms.recs[2]))
        f = ms.frames(1, 100)[0]
        w = f.copy(); ora.add_grain_frame(w)
        d = DevFrame(f)
        hip.add_grain_frame_dev(*d.ptrs(), W, H, f.stride, f.cstride, stream_ptr())
        assert d.download().equal_all(w) and hip.seed_state() == ora.seed_state()
        assert hip.last_launch_info()["kernel"].startswith("grain_rw_kernel<10,2,2,false,false,true")
        # an unseeded plain list afterwards continues the registers
        fr = ms.frames(3, 110)
        want = [x.copy() for x in fr]
        for x in want:
            ora.add_grain_frame(x)
        dev = scattered(fr, 10)
        hip.add_grain_frame_list_dev([x.ptrs() for x in dev], W, H, fr[0].stride, fr[0].cstride, stream_ptr())
        check(dev, want)
        assert hip.seed_state() == ora.seed_state()
        # ... and the models call continues them in turn
        run(hip, ms, [1, 0], ms.frames(2, 120), None, ora=ora, shuffle=11)
    finally:
        ms.release()


def test_capture_is_a_snapshot(hip):
    """capture, re-program something else (same slots, other patterns, LUTs, shift and range), then use the model"""
    ms = Models(hip, ["fgs_afgs1_test1_10_420"])
    try:
        U.program(hip, U.model_records("fgs_sei_ff_test6_10_420"))
        hip.set_legal_range(0)
        recs = ms.recs + [U.model_records("fgs_sei_ff_test6_10_420")]
        frames = ms.frames(5, 130)
        ora = U.oracle_programmed(recs[1])
        want, regs = U.expect_unseeded(ora, recs, [0] * 5, frames)
        dev = scattered(frames, 12)
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev], None, [ms.handles[0]] * 5, None, W, H, frames[0].stride, frames[0].cstride, stream_ptr())
        check(dev, want)
        assert hip.seed_state() == regs
    finally:
        ms.release()


def test_release_right_after_the_call_and_capture_on_another_stream(hip):
    import torch
    other, third = torch.cuda.Stream(), torch.cuda.Stream()
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"], stream=other.cuda_stream)     # captured on one stream ...
    pick = [0, 1, 0, 1, 1, 0, 1]
    frames = ms.frames(7, 140)
    seeds = fresh_seeds(7, 7)
    want, regs = U.expect_seeded(ms.recs, pick, frames, seeds)
    dev = scattered(frames, 13)
    torch.cuda.synchronize()        # (the frames are there; nothing else orders the streams)
    hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev], None, [ms.handles[k] for k in pick], seeds, W, H, frames[0].stride, frames[0].cstride,
                                        third.cuda_stream)                                                 # ... used on another
    ms.release()                    # as soon as the call has returned
    assert hip.seed_state() == regs
    # captures that follow (they program the library anew) take buffers of their own while the released ones may still be read
    ms2 = Models(hip, ["fgs_sei_10_420", "default_10_420"], stream=other.cuda_stream)
    torch.cuda.synchronize()
    check(dev, want)
    from versatilefilmgrain_amd.hw import VfgsHipError
    with pytest.raises(VfgsHipError, match="error 41"):
        hip.model_info(ms.handles[0])
    hip.model_release(ms.handles[0])        # a second release, and NULL: no-ops
    hip.model_release(None)
    ms2.release()


def test_two_calls_inside_an_overlap_region(hip):
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"])
    try:
        a, b = ms.frames(4, 150, 520, 70), ms.frames(3, 160, 520, 70)
        pick = [0, 1, 1, 0, 1, 0, 0]
        ora = U.oracle_programmed(ms.recs[-1])
        want, regs = U.expect_unseeded(ora, ms.recs, pick, a + b)
        da, db = scattered(a, 14), scattered(b, 15)
        st = stream_ptr()
        hm = [ms.handles[k] for k in pick]
        hip.overlap_begin(st)
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in da], None, hm[:4], None, 520, 70, a[0].stride, a[0].cstride, st)
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in db], None, hm[4:], None, 520, 70, a[0].stride, a[0].cstride, st)
        hip.overlap_end(st)
        check(da + db, want)
        assert hip.seed_state() == regs
    finally:
        ms.release()


def test_refusals_change_nothing(hip):
    """... in particular they do not reseed, launch or write"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    import ctypes as C
    ms = Models(hip, ["fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420"])
    m8 = Models(hip, ["fgs_afgs1_test1_8_420"])
    m422 = Models(hip, ["fgs_afgs1_test3_10_422"])
    gone = Models(hip, ["fgs_sei_10_420"])
    gone.release()
    U.program(hip, ms.recs[1])
    try:
        frames = ms.frames(3, 170, 520, 70)
        dev = scattered(frames)
        f0 = frames[0]
        geo = (f0.width, f0.height, f0.stride, f0.cstride, stream_ptr())
        ptrs = [d.ptrs() for d in dev]
        hm = [ms.handles[0], ms.handles[1], ms.handles[0]]
        seeds = fresh_seeds(3, 8)
        st0, n0 = hip.seed_state(), U.launches(hip)

        def refused(match, src, dst, models, sd=seeds, g=geo):
            with pytest.raises(VfgsHipError, match=match):
                hip.add_grain_frame_list_models_dev(src, dst, models, sd, *g)
            assert match.startswith("error") or match in hip.lib.vfgs_hip_last_error_string().decode()

        # error 41, each cause
        fl = hip.frame_list(ptrs)
        assert hip.lib.vfgs_hip_add_grain_frame_list_models_dev(fl, fl, None, None, 3, *geo) == 41 and b"null list of models" in hip.lib.vfgs_hip_last_error_string()
        refused("error 41.*frame 1 is null", ptrs, None, [hm[0], None, hm[2]])
        refused("error 41.*frame 2 is not a live model", ptrs, None, [hm[0], hm[1], gone.handles[0]])
        refused("error 41.*captured at depth 8", ptrs, None, [hm[0], m8.handles[0], hm[2]])
        refused("error 41.*chroma subsampling 2,1", ptrs, None, [m422.handles[0], hm[1], hm[2]])
        refused("error 41.*width 8200", ptrs, None, hm, g=(8200, 70, 8256, 4160, stream_ptr()))
        try:
            hip.set_chroma_mix(1, 32, 32, 0)
            refused("error 41.*chroma mix", ptrs, None, hm)
        finally:
            hip.clear_chroma_mix()
        # what the list calls refuse, with their codes
        assert hip.lib.vfgs_hip_add_grain_frame_list_models_dev(None, None, (C.c_void_p * 3)(*hm), None, 3, *geo) == 18
        refused("error 18.*listed twice", [ptrs[0], ptrs[1], ptrs[0]], None, hm)
        refused("error 18.*null plane", [ptrs[0], (ptrs[1][0], 0, ptrs[1][2]), ptrs[2]], None, hm)
        refused("error 18.*shares bytes", [ptrs[0], ptrs[1], ptrs[2]], [ptrs[1], ptrs[0], ptrs[2]], hm)
        refused("error 7", [ptrs[0], (ptrs[1][0] + 8, ptrs[1][1], ptrs[1][2]), ptrs[2]], None, hm)
        refused("error 6", ptrs, None, hm, g=(f0.width, f0.height, 512, f0.cstride, stream_ptr()))
        refused("error 5", ptrs, None, hm, g=(128, f0.height, f0.stride, f0.cstride, stream_ptr()))
        # an empty list is no call at all, with or without models and seeds
        hip.add_grain_frame_list_models_dev([], None, [], None, *geo)
        assert hip.lib.vfgs_hip_add_grain_frame_list_models_dev(None, None, None, None, 0, *geo) == 0
        assert hip.seed_state() == st0 and U.launches(hip) == n0
        for d, f in zip(dev, frames):
            assert d.download().equal_all(f)
        # ... and the same list is served afterwards
        want, regs = U.expect_seeded(ms.recs, [0, 1, 0], frames, seeds)
        hip.add_grain_frame_list_models_dev(ptrs, None, hm, seeds, *geo)
        check(dev, want)
        assert hip.seed_state() == regs
        # capture refuses what the processing calls refuse of the programmed state: an undefined pattern-LUT entry
        lut = bytearray(hip.luts(0)[1]); lut[7] = 0x90
        hip.set_pattern_lut(0, bytes(lut))
        with pytest.raises(VfgsHipError, match="error 4"):
            hip.model_capture(stream_ptr())
        # ... which does not stand in the way of models captured before
        frames2 = ms.frames(3, 180, 520, 70)
        want, regs = U.expect_seeded(ms.recs, [0, 1, 0], frames2, seeds)
        dev2 = scattered(frames2, 1)
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev2], None, hm, seeds, *geo)
        check(dev2, want)
        assert hip.seed_state() == regs
    finally:
        for x in (ms, m8, m422):
            x.release()
