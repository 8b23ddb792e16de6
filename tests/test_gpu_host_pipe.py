"""GPU (MI355X): pictures in HOST memory as a stream -- vfgs_hip_host_pipe_open / _submit / _wait / _close (include/vfgs_hip.h): a model
and a seed per picture, in place, into a destination of its own or into a narrowed 8-bit one, collected later by ticket -- against the
oracle, through the Python wrapper over the C ABI, bit for bit: every byte of every plane, padding included, and the four seed registers
behind every submit.

A submit computes what the matching one-picture device call computes, so the expectations are the helpers of those calls' tests and nothing
else: model_list_util.expect_seeded / expect_unseeded, model_out8_util.expect_planar, model_mix_list_util.expect_list, and the models of
test_gpu_model_list.Models.  Sources hold garbage over the full container range (the pictures under a mix: the content of that call's case
table) and destinations are pre-filled with garbage.

Shapes: the smallest that wrap the ring's slots, rag the last block of a row and leave a partial block row."""
import ctypes as C

import numpy as np
import pytest

import model_list_util as U
import model_mix_list_util as MX
import model_out8_util as O8
import vfgs_testlib as T
from gpu_util import DevFrame, stream_ptr
from test_gpu_frame_list import garbage_frame
from test_gpu_model_list import Models, fresh_seeds

pytestmark = pytest.mark.gpu

# name -> (model A: general-form luma, model B: one-pattern (4:2:2: the two recorded programs), width, height)
SHAPES = {
    "10_420_416x240": ("fgs_sei_10_420", "fgs_afgs1_test1_10_420", 416, 240),
    "8_444_200x152": ("fgs_sei_ff_test6_8_444", "fgs_afgs1_test1_8_444", 200, 152),
    "8_422_264x136": ("fgs_sei_8_422", "fgs_sei_ff_test6_8_422", 264, 136),
    "10_440_1000x70": ("fgs_sei_10_440", "fgs_afgs1_test1_10_440", 1000, 70),
    "12_420_416x96": ("fgs_sei_10_420@depth12", "fgs_afgs1_test1_10_420@depth12", 416, 96),
}
PICK8 = [0, 1, 0, 1, 0, 1, 0, 1]      # A B A B ...: the form of the image changes with every picture


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


class HostMem:
    """the planes of frames moved into pinned memory of the library's (pinned), or left where numpy put them (pageable)"""

    def __init__(self, hip, pinned):
        self.hip, self.pinned, self.keep = hip, pinned, []

    def place(self, f):
        if self.pinned:
            f.Y, f.U, f.V = (self._pinned_like(a) for a in f.planes())
        return f

    def _pinned_like(self, arr):
        p = self.hip.host_alloc(arr.nbytes + 64)
        self.keep.append(p)
        out = np.frombuffer((C.c_char * arr.nbytes).from_address(p), dtype=arr.dtype).reshape(arr.shape)
        out[...] = arr
        return out

    def free(self):
        for p in self.keep:
            self.hip.host_free(p)
        self.keep = []


def ptrs(f):
    return (f.Y.ctypes.data, f.U.ctypes.data, f.V.ctypes.data)


def region(f):
    """(luma rows, chroma rows, luma columns, chroma columns) a picture's call writes: whole blocks of the rows of the picture"""
    cols = (f.width + 15) // 16 * 16
    return f.height, (f.height + f.suby - 1) // f.suby, cols, cols // f.subx


def written_over(fill, want):
    rows, crows, cols, ccols = region(want)
    e = fill.copy()
    e.Y[:rows, :cols] = want.Y[:rows, :cols]
    e.U[:crows, :ccols] = want.U[:crows, :ccols]
    e.V[:crows, :ccols] = want.V[:crows, :ccols]
    return e


def destination(f0, seed, extra=64, cextra=32):
    """a garbage-filled frame of f0's picture with row pitches of its own"""
    g = T.Frame(f0.width, f0.height, f0.depth, f0.subx, f0.suby, f0.stride + extra, f0.cstride + cextra)
    rng = np.random.default_rng(seed)
    for p in g.planes():
        p[...] = rng.integers(0, 1 << (16 if g.depth > 8 else 8), p.shape).astype(g.dtype)
    return g


def same(got, want, what):
    for n, a, b in zip("YUV", got.planes(), want.planes()):
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what} plane {n}: {len(bad)} samples differ, first at {tuple(bad[0])}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}")


def b(v):
    return "true" if v else "false"


def stream(hip, ms, pick, frames, seeds, dst_mode, pinned, slots=3, wait="each_late", ora=None):
    """the pictures through a pipe, a model each (pick), against the contract's loop frame by frame: the registers behind every submit, the
    launch record, and after the waits every byte.  dst_mode: None (in place), "copy", "dst8"."""
    f0 = frames[0]
    mem = HostMem(hip, pinned)
    src = [mem.place(f.copy()) for f in frames]
    fill8 = O8.dst_frame(f0.width, f0.height, f0.subx, f0.suby, 99) if dst_mode == "dst8" else None
    if dst_mode == "copy":
        fills = [destination(f0, 500 + i) for i in range(len(frames))]
        dst = [mem.place(f.copy()) for f in fills]
        geo = (dst[0].stride, dst[0].cstride, False)
    elif dst_mode == "dst8":
        dst = [mem.place(fill8.copy()) for _ in frames]
        geo = (fill8.stride, fill8.cstride, True)
    else:
        dst, geo = None, (0, 0, False)
    if seeds is None:
        ora = ora or U.oracle_programmed(ms.recs[-1])      # (the library is programmed with the last model, registers included)
    try:
        with hip.host_pipe(f0.width, f0.height, f0.stride, f0.cstride, geo[0], geo[1], geo[2], slots) as pipe:
            tickets, want = [], []
            for i, f in enumerate(frames):
                k = pick[i]
                sd = None if seeds is None else [seeds[i]]
                if dst_mode == "dst8":
                    w, regs, _ = O8.expect_planar(ms.recs, [k], [f], sd, fill8, ora)
                elif sd:
                    w, regs = U.expect_seeded(ms.recs, [k], [f], sd)
                else:
                    w, regs = U.expect_unseeded(ora, ms.recs, [k], [f])
                want.append(written_over(fills[i], w[0]) if dst_mode == "copy" else w[0])
                n0 = U.launches(hip)
                t = pipe.submit(ptrs(src[i]), None if dst is None else ptrs(dst[i]), ms.handles[k], None if sd is None else sd[0])
                tickets.append(t)
                assert t == i + 1
                assert hip.seed_state() == regs, i
                info = hip.last_launch_info()
                assert info["launches"] - n0 == 1 and info["internal"] == 1 and info["listed"] == 1 and info["nframes"] == 1, info
                assert info["in_place"] == (1 if dst is None else 0) and info["out8"] == (1 if dst_mode == "dst8" else 0), info
                oy, oc = ms.forms[k]
                name = f"grain_rw_kernel<{ms.depth},{ms.sx},{ms.sy},true,{b(oy)},{b(oc)},false,false>" if dst_mode == "dst8" \
                    else f"grain_ml_kernel<{ms.depth},{ms.sx},{ms.sy},{b(oy)},{b(oc)}>"
                assert info["kernel"] == name, info
                if wait == "each_late" and i >= 2:
                    pipe.wait(tickets[i - 2])      # display order, two pictures behind the decoder
            if wait == "each_late":
                pipe.wait(tickets[-1])
            elif wait == "reversed":
                for t in reversed(tickets):
                    pipe.wait(t)
                pipe.wait(tickets[0])
            # wait == "close": nothing is waited for, close brings everything home
        for i, (s, f) in enumerate(zip(src, frames)):
            if dst is None:
                same(s, want[i], f"picture {i}")
            else:
                same(s, f, f"source {i}")
                same(dst[i], want[i], f"destination {i}")
    finally:
        del src, dst
        mem.free()
    return ora


# ---- 1, 2: eight pictures through three slots, a model and a seed each; in place and into a destination; pinned and pageable ---------

@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("dst_mode", [None, "copy"], ids=["in_place", "destination"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_model_and_a_seed_per_picture(hip, shape, dst_mode, pinned):
    a, bname, w, h = SHAPES[shape]
    ms = Models(hip, [a, bname])
    try:
        if shape.startswith(("10_420", "12_420")):
            assert ms.forms == [(0, 1), (1, 1)], ms.forms      # general-form luma, then all one-pattern: the form changes with every picture
        frames = ms.frames(8, 20, w, h)
        stream(hip, ms, PICK8, frames, fresh_seeds(8, 6), dst_mode, pinned)
    finally:
        ms.release()


# ---- 3: the narrowed 8-bit destination ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [True, False], ids=["seeded", "one_sequence"])
@pytest.mark.parametrize("shape", ["10_420_416x240", "12_420_416x96"])
def test_the_8_bit_destination(hip, shape, seeded):
    a, bname, w, h = SHAPES[shape]
    ms = Models(hip, [a, bname])
    try:
        frames = ms.frames(8, 30, w, h)
        stream(hip, ms, PICK8, frames, fresh_seeds(8, 7) if seeded else None, "dst8", pinned=seeded)
    finally:
        ms.release()


# ---- 4: the programmed state, with and without a seed, in one seed sequence with the other entry points -----------------------------

@pytest.mark.parametrize("dst_mode", [None, "copy", "dst8"], ids=["in_place", "destination", "dst8"])
def test_the_programmed_state_interleaves_with_every_entry(hip, dst_mode):
    """submit / vfgs_hip_add_grain_frames_host / submit with a seed / vfgs_add_grain_stripe / submit / a device list call / submit: one
    sequence of the four registers against ONE oracle"""
    rec = T.load_trace("fgs_sei_10_420")
    U.program(hip, rec)
    ora = U.oracle_programmed(rec)
    depth, sx, sy = T.trace_geometry(rec)
    w, h = 416, 240
    fr = [garbage_frame(w, h, depth, sx, sy, 40 + i) for i in range(7)]
    f0 = fr[0]
    fill8 = O8.dst_frame(w, h, sx, sy, 98)
    fills = [destination(f0, 600 + i) for i in range(7)]
    dst = None if dst_mode is None else [f.copy() for f in fills] if dst_mode == "copy" else [fill8.copy() for _ in fr]
    geo = (0, 0, False) if dst_mode is None else (dst[0].stride, dst[0].cstride, dst_mode == "dst8")
    src = [f.copy() for f in fr]
    want = [f.copy() for f in fr]
    dev = DevFrame(fr[5])

    def through_the_pipe(pipe, i, seed=None):
        if seed is not None:
            ora.set_seed(seed)
        ora.add_grain_frame(want[i])
        t = pipe.submit(ptrs(src[i]), None if dst is None else ptrs(dst[i]), None, seed)
        assert hip.seed_state() == ora.seed_state(), i
        return t

    with hip.host_pipe(w, h, f0.stride, f0.cstride, *geo) as pipe:
        through_the_pipe(pipe, 0)
        ora.add_grain_frame(want[1])
        hip.add_grain_frames_host([src[1].Y.ctypes.data], [src[1].U.ctypes.data], [src[1].V.ctypes.data], w, h, f0.stride, f0.cstride)
        assert hip.seed_state() == ora.seed_state()
        through_the_pipe(pipe, 2, 0x9e3779b9)
        ora.add_grain_frame(want[3])
        hip.add_grain_stripe(*ptrs(src[3]), 0, w, h, f0.stride, f0.cstride)
        assert hip.seed_state() == ora.seed_state()
        through_the_pipe(pipe, 4)
        ora.add_grain_frame(want[5])
        hip.add_grain_frame_list_dev([dev.ptrs()], w, h, f0.stride, f0.cstride, stream_ptr())
        assert hip.last_launch_info()["internal"] == 0
        assert hip.seed_state() == ora.seed_state()
        last = through_the_pipe(pipe, 6)
        assert last == 4
        pipe.wait(last)
        for i in (0, 2, 4, 6):
            if dst is None:
                same(src[i], want[i], f"picture {i}")
                continue
            same(src[i], fr[i], f"source {i}")
            same(dst[i], O8.narrowed_over(fill8, want[i]) if dst_mode == "dst8" else written_over(fills[i], want[i]), f"destination {i}")
    same(src[1], want[1], "the picture of vfgs_hip_add_grain_frames_host")
    same(src[3], want[3], "the picture of vfgs_add_grain_stripe")
    same(dev.download(), want[5], "the picture of the device list call")


# ---- 5: AFGS1 models that carry a mix -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [True, False], ids=["seeded", "one_sequence"])
@pytest.mark.parametrize("dst_mode", [None, "copy"], ids=["in_place", "destination"])
@pytest.mark.parametrize("cid", ["10_420_1047x40", "8_444_183x33"])
def test_models_that_carry_a_mix(hip, cid, dst_mode, seeded):
    """models A B A C B of that call's case table (A and B carry different mixes, C none), each honoured for its picture"""
    from test_gpu_model_list_mix import build, release
    spec, w, h = MX.PLANAR[cid]
    handles, (depth, sx, sy) = build(hip, spec)
    mem = HostMem(hip, True)
    try:
        models = MX.case_models(spec)
        frames = MX.case_frames(spec, w, h, len(MX.PICK), 5)
        seeds = MX.fresh_seeds(len(MX.PICK), 1) if seeded else None
        hip.set_seed(1234)
        ora = None
        if not seeded:
            ora = T.OracleHW()
            ora.set_seed(1234)
        f0 = frames[0]
        src = [mem.place(f.copy()) for f in frames]
        fills = [destination(f0, 700 + i) for i in range(len(frames))] if dst_mode else None
        dst = [mem.place(f.copy()) for f in fills] if dst_mode else None
        excluded = 0
        with hip.host_pipe(w, h, f0.stride, f0.cstride, dst[0].stride if dst else 0, dst[0].cstride if dst else 0) as pipe:
            want = []
            for i, k in enumerate(MX.PICK):
                res, ex, regs, ora = MX.expect_list(models, [k], [frames[i]], None if seeds is None else [seeds[i]], ora)
                excluded += ex
                want.append(res[0][0])
                n0 = U.launches(hip)
                pipe.submit(ptrs(src[i]), ptrs(dst[i]) if dst else None, handles[k], None if seeds is None else seeds[i])
                assert hip.seed_state() == regs, i
                info = hip.last_launch_info()
                mixed = MX.mix_of(spec[k][1]) != (None, None)
                assert info["launches"] - n0 == (2 if mixed and not dst else 1) and info["internal"] == 1 and info["listed"] == 1, info      # (in place under a mix: chroma first)
                assert info["kernel"].startswith("grain_mix_kernel<" if mixed else "grain_ml_kernel<"), info
            pipe.wait(len(MX.PICK))
        assert excluded == 0
        for i, f in enumerate(frames):
            if dst:
                same(src[i], f, f"source {i}")
                same(dst[i], written_over(fills[i], want[i]), f"destination {i}")
            else:
                same(src[i], want[i], f"picture {i}")
    finally:
        del src, dst
        mem.free()
        release(hip, handles)


# ---- 6, 7: two slots and no wait until close; waits out of order, repeated; a model released right after its submit --------------------

@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_two_slots_seven_pictures_and_no_wait_until_close(hip, pinned):
    a, bname, w, h = SHAPES["10_420_416x240"]
    ms = Models(hip, [a, bname])
    try:
        frames = ms.frames(7, 50, w, h)
        stream(hip, ms, PICK8[:7], frames, fresh_seeds(7, 8), "copy", pinned, slots=2, wait="close")
    finally:
        ms.release()


def test_waits_out_of_order_and_a_model_released_behind_its_submit(hip):
    a, bname, w, h = SHAPES["8_444_200x152"]
    ms = Models(hip, [a, bname])
    try:
        frames = ms.frames(6, 60, w, h)
        stream(hip, ms, [0, 1, 1, 0, 1, 0], frames, fresh_seeds(6, 9), None, True, slots=8, wait="reversed")
        # a model of its own for one picture, released as soon as submit has returned, with captures right behind it
        f = frames[0]
        want, regs = U.expect_seeded(ms.recs, [0], [f], [77])
        mem = HostMem(hip, True)
        src = mem.place(f.copy())
        try:
            with hip.host_pipe(w, h, f.stride, f.cstride) as pipe:
                U.program(hip, ms.recs[0])
                m = hip.model_capture(stream_ptr())
                t = pipe.submit(ptrs(src), None, m, 77)
                hip.model_release(m)
                others = [hip.model_capture(stream_ptr()) for _ in range(12)]      # (more than the queue of released buffers holds)
                for o in others:
                    hip.model_release(o)
                pipe.wait(t)
                pipe.wait(t)
                same(src, want[0], "the picture")
                assert hip.seed_state() == regs
        finally:
            del src
            mem.free()
    finally:
        ms.release()


# ---- 8: two pipes of different geometry, interleaved --------------------------------------------------------------------------------

def test_two_pipes_interleaved(hip):
    a, bname, _, _ = SHAPES["10_420_416x240"]
    ms = Models(hip, [a, bname])
    mem = HostMem(hip, True)
    try:
        big = ms.frames(5, 70, 416, 240)
        small = ms.frames(5, 80, 264, 136)
        seeds = fresh_seeds(10, 10)
        fills = [destination(small[0], 800 + i) for i in range(5)]
        sb, ss, ds = [mem.place(f.copy()) for f in big], [mem.place(f.copy()) for f in small], [mem.place(f.copy()) for f in fills]
        want_b, want_s = [], []
        with hip.host_pipe(416, 240, big[0].stride, big[0].cstride, slots=2) as pb, \
                hip.host_pipe(264, 136, small[0].stride, small[0].cstride, fills[0].stride, fills[0].cstride) as ps:
            for i in range(5):
                w, regs = U.expect_seeded(ms.recs, [i & 1], [big[i]], [seeds[2 * i]])
                want_b.append(w[0])
                assert pb.submit(ptrs(sb[i]), None, ms.handles[i & 1], seeds[2 * i]) == i + 1 and hip.seed_state() == regs
                w, regs = U.expect_seeded(ms.recs, [1 - (i & 1)], [small[i]], [seeds[2 * i + 1]])
                want_s.append(written_over(fills[i], w[0]))
                assert ps.submit(ptrs(ss[i]), ptrs(ds[i]), ms.handles[1 - (i & 1)], seeds[2 * i + 1]) == i + 1 and hip.seed_state() == regs
            ps.wait(5)
            for i in range(5):
                same(ds[i], want_s[i], f"small destination {i}")
                same(ss[i], small[i], f"small source {i}")
            pb.wait(3)
            pb.wait(5)
        for i in range(5):
            same(sb[i], want_b[i], f"big picture {i}")
    finally:
        mem.free()
        ms.release()


# ---- 9: the launch record is the matching device call's ------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [True, False], ids=["seeded", "one_sequence"])
@pytest.mark.parametrize("dst_mode", [None, "copy", "dst8"], ids=["in_place", "destination", "dst8"])
@pytest.mark.parametrize("with_model", [True, False], ids=["model", "programmed"])
def test_the_launch_record_is_the_device_calls(hip, with_model, dst_mode, seeded):
    a, bname, w, h = SHAPES["10_420_416x240"]
    ms = Models(hip, [a, bname])      # (programmed: model B's state)
    try:
        f = ms.frames(1, 90, w, h)[0]
        fill = O8.dst_frame(w, h, ms.sx, ms.sy, 97) if dst_mode == "dst8" else destination(f, 900, 0, 0)
        sdev, ddev = DevFrame(f), DevFrame(fill)
        s, d = [sdev.ptrs()], ([ddev.Y.data_ptr(), ddev.U.data_ptr(), ddev.V.data_ptr()] if dst_mode else None)
        seeds = [4711] if seeded else None
        st = stream_ptr()
        if with_model and dst_mode == "dst8":
            hip.add_grain_frame_list_models_copy8_dev(s, [d], [ms.handles[0]], seeds, w, h, f.stride, f.cstride, fill.stride, fill.cstride, st)
        elif with_model:
            hip.add_grain_frame_list_models_dev(s, [d] if d else None, [ms.handles[0]], seeds, w, h, f.stride, f.cstride, st)
        elif dst_mode == "dst8" and seeded:
            hip.add_grain_frame_list_seeded_copy8_dev(s, [d], seeds, w, h, f.stride, f.cstride, fill.stride, fill.cstride, st)
        elif dst_mode == "dst8":
            hip.add_grain_frame_list_copy8_dev(s, [d], w, h, f.stride, f.cstride, fill.stride, fill.cstride, st)
        elif seeded:
            hip.add_grain_frame_list_seeded_copy_dev(s, [d] if d else s, seeds, w, h, f.stride, f.cstride, st)
        else:
            hip.add_grain_frame_list_copy_dev(s, [d] if d else s, w, h, f.stride, f.cstride, st)
        dev = hip.last_launch_info()
        assert dev["internal"] == 0
        src, dst = f.copy(), fill.copy()
        with hip.host_pipe(w, h, f.stride, f.cstride, fill.stride if dst_mode else 0, fill.cstride if dst_mode else 0, dst_mode == "dst8") as pipe:
            pipe.wait(pipe.submit(ptrs(src), ptrs(dst) if dst_mode else None, ms.handles[0] if with_model else None, 4711 if seeded else None))
        got = hip.last_launch_info()
        assert got["internal"] == 1 and got["listed"] == 1 and got["launches"] == dev["launches"] + 1
        for k in dev:
            if k not in ("internal", "launches"):
                assert got[k] == dev[k], (k, got, dev)
    finally:
        ms.release()


# ---- 10: every refusal changes nothing ----------------------------------------------------------------------------------------------

def refused(hip, code, call, text=None):
    """the call raises with that code (and text), and neither a seed register nor the launch count has moved"""
    from versatilefilmgrain_amd import hw
    regs, n = hip.seed_state(), U.launches(hip)
    with pytest.raises(hw.VfgsHipError) as e:
        call()
    assert f"libvfgs_hip error {code}:" in str(e.value) and (text is None or text in str(e.value)), str(e.value)
    assert hip.seed_state() == regs and U.launches(hip) == n


def test_every_refusal_changes_nothing(hip):
    """(error 9, a programmed scale shift out of range, is behind these in the device calls; no setter of the library programs one)"""
    U.program(hip, U.model_records("fgs_afgs1_test1_8_420"))
    m8 = hip.model_capture(stream_ptr())
    U.program(hip, U.model_records("fgs_sei_10_422"))
    m422 = hip.model_capture(stream_ptr())
    a, bname, w, h = SHAPES["10_420_416x240"]
    ms = Models(hip, [a, bname])      # (programmed: B, all one-pattern)
    hip.set_chroma_mix(1, 32, 32, 0)
    mixed = hip.model_capture_mix(stream_ptr())
    hip.clear_chroma_mix()
    gone = hip.model_capture(stream_ptr())
    hip.model_release(gone)
    A = ms.handles[0]
    from versatilefilmgrain_amd import hw
    try:
        f, g = ms.frames(2, 95, w, h)
        fill8 = O8.dst_frame(w, h, ms.sx, ms.sy, 96)
        src, src2, dst = f.copy(), g.copy(), fill8.copy()
        S, CS, D, CD = f.stride, f.cstride, fill8.stride, fill8.cstride
        op = lambda *a, **k: (lambda: hip.host_pipe(*a, **k))
        # open: the pipe's own (43), then the geometry with the device calls' codes, then 16
        for bad in (dict(slots=1), dict(slots=9), dict(dst8=True), dict(dst_stride=D), dict(dst_cstride=CD, dst8=True)):
            refused(hip, 43, op(w, h, S, CS, **bad), "vfgs_hip_host_pipe_open")
        refused(hip, 5, op(128, h, S, CS), "vfgs_hip_host_pipe_open: width 128")
        refused(hip, 17, op(31760, h, 31808, 15904))
        refused(hip, 6, op(w, h, 400, CS))
        refused(hip, 6, op(w, h, S, CS, 400, CD, True))
        refused(hip, 8, op(w, h, S, CS + 4))
        refused(hip, 8, op(w, h, S, CS, D, CD + 8, True))
        refused(hip, 15, op(w, 2400000, S, CS))
        hip.set_depth(8)
        refused(hip, 16, op(w, h, S, CS, D, CD, True))
        hip.set_depth(10)
        hip.init_devices([0, 0])
        refused(hip, 43, op(w, h, S, CS), "devices")
        hip.init_devices([0])
        assert hip.lib.vfgs_hip_host_pipe_open(None, C.byref(C.c_void_p())) == 43 and hip.lib.vfgs_hip_host_pipe_open(C.byref(hw.HostPipeDesc()), None) == 43

        with hip.host_pipe(w, h, S, CS, D, CD, True) as p8, hip.host_pipe(w, h, S, CS) as pin, hip.host_pipe(8208, 16, 8256, 4128) as wide:
            assert p8.submit(ptrs(src), ptrs(dst), A, 5) == 1
            p8.wait(1)
            want, regs1, _ = O8.expect_planar(ms.recs, [0], [f], [5], fill8)
            same(dst, want[0], "the first picture")
            assert hip.seed_state() == regs1
            n1 = U.launches(hip)
            dst2 = fill8.copy()
            sub = lambda **k: (lambda: p8.submit(k.get("src", ptrs(src2)), k.get("dst", ptrs(dst2)), k.get("model", A), 6))
            lib, t = hip.lib, C.c_uint64(99)
            regs_in_front = hip.seed_state()
            fp = lambda x: C.byref(hw.FramePtrs(*x))
            # 43
            assert lib.vfgs_hip_host_pipe_submit(None, fp(ptrs(src2)), fp(ptrs(dst2)), A, None, C.byref(t)) == 43
            assert lib.vfgs_hip_host_pipe_submit(p8.handle, None, fp(ptrs(dst2)), A, None, C.byref(t)) == 43
            assert lib.vfgs_hip_host_pipe_submit(p8.handle, fp(ptrs(src2)), fp(ptrs(dst2)), A, None, None) == 43
            assert lib.vfgs_hip_host_pipe_submit(C.addressof(t), fp(ptrs(src2)), fp(ptrs(dst2)), A, None, C.byref(t)) == 43      # never a pipe
            assert hip.seed_state() == regs_in_front and U.launches(hip) == n1
            refused(hip, 43, sub(dst=None), "destination")
            refused(hip, 43, lambda: pin.submit(ptrs(src2), ptrs(src), None, None), "in place")
            refused(hip, 43, lambda: p8.wait(2), "never issued")
            refused(hip, 43, lambda: p8.wait(0))
            hip.set_depth(12)
            refused(hip, 43, sub(), "depth 12")
            hip.set_depth(10)
            hip.set_chroma_subsampling(2, 1)
            refused(hip, 43, sub())
            hip.set_chroma_subsampling(2, 2)
            hip.overlap_begin(stream_ptr())
            refused(hip, 43, sub(), "overlap")
            hip.overlap_end(stream_ptr())
            hip.init_devices([0, 0])
            refused(hip, 43, sub(), "devices")
            hip.init_devices([0])
            # the device calls' refusals, with their codes behind the pipe's name
            refused(hip, 18, sub(src=(src2.Y.ctypes.data, 0, src2.V.ctypes.data)), "vfgs_hip_host_pipe_submit: frame list")
            refused(hip, 18, sub(dst=(dst2.Y.ctypes.data, dst2.U.ctypes.data, dst2.U.ctypes.data)))
            refused(hip, 18, sub(dst=(src2.Y.ctypes.data, dst2.U.ctypes.data, dst2.V.ctypes.data)), "shares bytes")
            refused(hip, 41, sub(model=gone), "not a live model")
            refused(hip, 41, sub(model=m8), "depth 8")
            refused(hip, 41, sub(model=m422), "2,1")
            refused(hip, 41, sub(model=mixed), "carries a chroma mix")
            hip.set_chroma_mix(1, 32, 32, 0)
            refused(hip, 41, sub(), "a chroma mix is active")
            hip.clear_chroma_mix()
            refused(hip, 41, lambda: wide.submit(ptrs(src2), None, A, None), "width 8208")      # (refused before a plane is looked at)
            # the programmed state of a submit without a model: an undefined pattern-LUT entry (4); a general-form model under a mix (38)
            keep = hip.luts(1)[1]
            hip.set_pattern_lut(1, bytes([0x90]) * 256)
            refused(hip, 4, sub(model=None))
            hip.set_pattern_lut(1, keep)
            U.program(hip, ms.recs[0])
            hip.set_chroma_mix(1, 32, 32, 0)
            refused(hip, 38, lambda: pin.submit(ptrs(src2), None, None, None), "general-form")
            hip.clear_chroma_mix()
            U.program(hip, ms.recs[1])
            # nothing moved: bytes, launches, tickets
            assert t.value == 99 and U.launches(hip) == n1
            same(src2, g, "the refused source")
            same(dst2, fill8, "the refused destination")
            same(src, f, "the first source")
            # the next submit gets the next ticket and is correct
            assert p8.submit(ptrs(src2), ptrs(dst2), A, 6) == 2
            want, regs2, _ = O8.expect_planar(ms.recs, [0], [g], [6], fill8)
            assert hip.seed_state() == regs2
            assert pin.submit(ptrs(src), None, ms.handles[1], 7) == 1
            p8.wait(2)
            pin.wait(1)
            same(dst2, want[0], "the second picture")
            same(src, U.expect_seeded(ms.recs, [1], [f], [7])[0][0], "the in-place picture")
            stale = p8.handle
        assert hip.lib.vfgs_hip_host_pipe_wait(stale, 1) == 43 and hip.lib.vfgs_hip_host_pipe_close(stale) == 43
    finally:
        hip.clear_chroma_mix()
        for m in (m8, m422, mixed):
            hip.model_release(m)
        ms.release()
