"""GPU (MI355X): the luma / chroma mix of the chroma look-up index (vfgs_hip_set_chroma_mix; AFGS1 cb_mult / cb_luma_mult /
cb_offset) through the C ABI, bit-exact against expectations derived from the unchanged oracle (tests/chroma_mix_util.py: the
oracle runs on the frame whose chroma planes hold the mix, the grain it added is moved onto the real chroma).  Every exact
test first asserts, on the oracle's output, how many samples the derivation had to leave out (0 for mid-range content).

The kernels of the mix serve the one-pattern banks of the AFGS1 models; a model that needs a general-form bank is REFUSED
(error 38, nothing changed), which is what the three SEI traces of the list check.
"""

import numpy as np
import pytest

import chroma_mix_util as X
import vfgs_testlib as T

pytestmark = pytest.mark.gpu

W, H = 320, 192
MIXES = [(32, 32, 0), (64, 0, 0), (64, 119, -238)]
E_UNSUPPORTED = 38


def content_range(mix):
    """Plane ranges (fractions of 2^depth) that keep m inside [0.2, 0.8]: luma, chroma."""
    return dict(lo=0.4, hi=0.6, clo=0.4, chi=0.5) if mix == (64, 119, -238) else dict(lo=0.3, hi=0.7)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


def records_of(name):
    """A trace, or 'trace@XY': the trace with its chroma subsampling replaced by X, Y (both implementations get the same records)."""
    if "@" not in name:
        return T.load_trace(name)
    base, sub = name.split("@")
    return [(op, int(sub[0]), int(sub[1]), p) if op == T.OP_CHROMA_SUBSAMPLING else (op, a, b, p) for op, a, b, p in T.load_trace(base)]


def program(hip, rec, mixes):
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, rec)
    for c, m in enumerate(mixes, 1):
        if m is not None:
            hip.set_chroma_mix(c, *m)


def expect(rec, frames, mixes, max_excluded=0):
    res, excluded, ora = X.expected_frames(T.OracleHW, rec, frames, mixes)
    total = sum(f.U.size + f.V.size for f in frames)
    print(f"excluded by the derivation: {excluded} of {total} chroma samples")
    assert excluded <= max_excluded, (excluded, total)
    return res, ora


def check(got, res):
    for i, (g, (want, masks)) in enumerate(zip(got, res)):
        n = X.mismatches(g, want, masks)
        assert n == 0, f"frame {i}: {n} samples differ from the expectation"


# ---- one runner per entry point: frames in -> frames out, the seed registers left as after whole frames ----------------------
# reprogram(): back to the programmed state of before the first frame (the part entries process one part per 'rank')

def stack(frames, rows=None):
    import torch
    r = rows or (slice(None), slice(None))
    return [torch.from_numpy(np.stack([p[r[k > 0]] for p in ps]).view(np.uint8).copy()).cuda()
            for k, ps in enumerate(zip(*[f.planes() for f in frames]))]


def unstack(ts, frames, rows=None):
    import torch
    torch.cuda.synchronize()
    out = [f.copy() for f in frames]
    r = rows or (slice(None), slice(None))
    for k, t in enumerate(ts):
        a = t.cpu().numpy()
        for i, f in enumerate(out):
            p = f.planes()[k]
            p[r[k > 0]] = a[i].view(f.dtype).reshape(p[r[k > 0]].shape)
    return out


def run_frame_dev(hip, frames, reprogram):
    from gpu_util import DevFrame, stream_ptr
    out = []
    for f in frames:
        d = DevFrame(f)
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        out.append(d.download())
    return out


def run_stripe_dev(hip, frames, reprogram):
    """stripes that do not start at 0, uneven, one of them inside a block row"""
    from gpu_util import DevFrame, stream_ptr
    out = []
    for f in frames:
        d = DevFrame(f)
        y = 0
        for h in (48, 6, 26, 64, f.height - 144):
            hip.add_grain_stripe_dev(*d.ptrs(y), y, f.width, h, f.stride, f.cstride, stream_ptr())
            y += h
        out.append(d.download())
    return out


def run_frames_dev(hip, frames, reprogram):
    from gpu_util import stream_ptr
    f0 = frames[0]
    Y, U, V = stack(frames)
    hip.add_grain_frames_dev(Y.data_ptr(), U.data_ptr(), V.data_ptr(), f0.width, f0.height, f0.stride, f0.cstride, len(frames),
                             Y[0].numel(), U[0].numel(), stream_ptr())
    return unstack((Y, U, V), frames)


PARTS = [(0, 64), (64, 48), (112, 80)]


def run_frame_part_dev(hip, frames, reprogram):
    from gpu_util import DevFrame, stream_ptr
    devs = [DevFrame(f) for f in frames]
    for k, (py, ph) in enumerate(PARTS):
        if k:
            reprogram()
        for d, f in zip(devs, frames):
            hip.add_grain_frame_part_dev(*d.ptrs(py), f.width, f.height, py, ph, f.stride, f.cstride, stream_ptr())
    return [d.download() for d in devs]


def run_frames_part_dev(hip, frames, reprogram):
    from gpu_util import stream_ptr
    f0 = frames[0]
    out = [f.copy() for f in frames]
    for k, (py, ph) in enumerate(PARTS):
        if k:
            reprogram()
        rows = (slice(py, py + ph), slice(py // f0.suby, (py + ph) // f0.suby))
        Y, U, V = stack(frames, rows)
        hip.add_grain_frames_part_dev(Y.data_ptr(), U.data_ptr(), V.data_ptr(), f0.width, f0.height, py, ph, f0.stride, f0.cstride,
                                      len(frames), Y[0].numel(), U[0].numel(), stream_ptr())
        part = unstack((Y, U, V), frames, rows)
        for o, p in zip(out, part):
            for a, b, r in zip(o.planes(), p.planes(), (rows[0], rows[1], rows[1])):
                a[r] = b[r]
    return out


def run_copy_dev(hip, frames, reprogram):
    from gpu_util import stream_ptr
    f0 = frames[0]
    src, dst = stack(frames), stack(frames)
    hip.add_grain_copy_dev(*[t.data_ptr() for t in src], *[t.data_ptr() for t in dst], f0.width, f0.height, 0, f0.height, f0.stride, f0.cstride,
                           len(frames), src[0][0].numel(), src[1][0].numel(), stream_ptr())
    for a, b in zip(unstack(src, frames), frames):
        assert a.equal_all(b), "the source of an out-of-place call changed"
    return unstack(dst, frames)


def narrowed(f):
    """yuv_to_8bit (yuv.c:216-258) of a 10-bit frame, same geometry in samples"""
    g = T.Frame(f.width, f.height, 8, f.subx, f.suby, f.stride, f.cstride)
    for a, b in zip(g.planes(), f.planes()):
        a[...] = ((b.astype(np.int32) + 2) >> 2).astype(np.uint8)
    return g


def run_copy8_dev(hip, frames, reprogram):
    """-> 8-bit frames; rows / columns the call does not write hold the narrowed INPUT (so that they compare equal to the narrowed expectation)"""
    from gpu_util import stream_ptr
    f0 = frames[0]
    src, dst = stack(frames), stack([narrowed(f) for f in frames])
    hip.add_grain_copy8_dev(*[t.data_ptr() for t in src], *[t.data_ptr() for t in dst], f0.width, f0.height, 0, f0.height, f0.stride, f0.cstride,
                            f0.stride, f0.cstride, len(frames), src[0][0].numel(), src[1][0].numel(), dst[0][0].numel(), dst[1][0].numel(), stream_ptr())
    return unstack(dst, [narrowed(f) for f in frames])


def run_list_dev(hip, frames, reprogram):
    from gpu_util import DevFrame, stream_ptr
    f0 = frames[0]
    devs = [DevFrame(f) for f in frames]
    hip.add_grain_frame_list_dev([d.ptrs() for d in devs], f0.width, f0.height, f0.stride, f0.cstride, stream_ptr())
    return [d.download() for d in devs]


def run_list_part_dev(hip, frames, reprogram):
    from gpu_util import DevFrame, stream_ptr
    f0 = frames[0]
    devs = [DevFrame(f) for f in frames]
    for k, (py, ph) in enumerate(PARTS):
        if k:
            reprogram()
        hip.add_grain_frame_list_part_dev([d.ptrs(py) for d in devs], f0.width, f0.height, py, ph, f0.stride, f0.cstride, stream_ptr())
    return [d.download() for d in devs]


def run_list_copy_dev(hip, frames, reprogram):
    from gpu_util import DevFrame, stream_ptr
    f0 = frames[0]
    src, dst = [DevFrame(f) for f in frames], [DevFrame(f) for f in frames]
    hip.add_grain_frame_list_copy_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], f0.width, f0.height, f0.stride, f0.cstride, stream_ptr())
    for d, f in zip(src, frames):
        assert d.download().equal_all(f), "the source of an out-of-place call changed"
    return [d.download() for d in dst]


def run_list_copy8_dev(hip, frames, reprogram):
    from gpu_util import DevFrame, stream_ptr
    f0 = frames[0]
    src, dst = [DevFrame(f) for f in frames], [DevFrame(narrowed(f)) for f in frames]
    hip.add_grain_frame_list_copy8_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], f0.width, f0.height, f0.stride, f0.cstride,
                                       f0.stride, f0.cstride, stream_ptr())
    return [d.download() for d in dst]


def run_frames_host(hip, frames, reprogram):
    out = [f.copy() for f in frames]
    f0 = out[0]
    hip.add_grain_frames_host([f.Y.ctypes.data for f in out], [f.U.ctypes.data for f in out], [f.V.ctypes.data for f in out],
                              f0.width, f0.height, f0.stride, f0.cstride)
    return out


def run_line(hip, frames, reprogram):
    out = [f.copy() for f in frames]
    for f in out:
        for y in range(f.height):
            hip.add_grain_line(f.Y[y].ctypes.data, f.U[y // f.suby].ctypes.data, f.V[y // f.suby].ctypes.data, y, f.width)
    return out


def run_stripe(hip, frames, reprogram):
    out = [f.copy() for f in frames]
    for f in out:
        y = 0
        for h in (6, 26, 32, 1, 15, 64, f.height - 144):
            hip.add_grain_stripe(f.Y[y].ctypes.data, f.U[y // f.suby].ctypes.data, f.V[y // f.suby].ctypes.data, y, f.width, h, f.stride, f.cstride)
            y += h
    return out


ENTRIES = {
    "frame_dev": run_frame_dev, "frames_dev": run_frames_dev, "stripe_dev": run_stripe_dev, "frame_part_dev": run_frame_part_dev,
    "frames_part_dev": run_frames_part_dev, "copy_dev": run_copy_dev, "copy8_dev": run_copy8_dev, "frame_list_dev": run_list_dev,
    "frame_list_part_dev": run_list_part_dev, "frame_list_copy_dev": run_list_copy_dev, "frame_list_copy8_dev": run_list_copy8_dev,
    "frames_host": run_frames_host, "add_grain_line": run_line, "add_grain_stripe": run_stripe,
}
OUT8 = ("copy8_dev", "frame_list_copy8_dev")
VOID = ("add_grain_line", "add_grain_stripe")      # drop-in calls: no error code, a refusal aborts the process (as the reference asserts)


def run_and_check(hip, entry, name, mixes, width=W, height=H, nframes=3, seed=1, max_excluded=0, frames=None):
    rec = records_of(name)
    depth, sx, sy = T.trace_geometry(rec)
    if frames is None:
        frames = X.ranged_frames(width, height, depth, sx, sy, nframes, seed, **content_range(mixes[0]))
    res, ora = expect(rec, frames, mixes, max_excluded)
    reprogram = lambda: program(hip, rec, mixes)
    reprogram()
    got = ENTRIES[entry](hip, frames, reprogram)
    if entry in OUT8:
        res = [(narrowed(w), m) for w, m in res]
    check(got, res)
    assert hip.seed_state() == ora.seed_state()
    assert hip.last_launch_info()["kernel"].startswith(f"grain_mix_kernel<{depth},{sx},{sy},")
    return frames, got


def entry_cases():
    """every entry point x the six traces x the three mixes, without what cannot be called at all: the narrowed destination exists for
    10-bit sources, and a void drop-in call has no error code to refuse a general-form model with (it aborts; not provoked here)"""
    for entry in sorted(ENTRIES):
        for name in X.SIX_TRACES:
            rec = T.load_trace(name)
            if (entry in OUT8 and T.trace_geometry(rec)[0] != 10) or (entry in VOID and not X.one_pattern_model(rec)):
                continue
            for mix in MIXES:
                yield pytest.param(entry, name, mix, id=f"{entry}-{name}-{mix[0]}_{mix[1]}_{mix[2]}")


@pytest.mark.parametrize("entry, name, mix", list(entry_cases()))
def test_every_entry_point_every_trace(hip, entry, name, mix):
    rec = records_of(name)
    depth, sx, sy = T.trace_geometry(rec)
    if X.one_pattern_model(rec):
        run_and_check(hip, entry, name, (mix, mix))
        return
    # a model with a general-form bank: refused, nothing changed
    frames = X.ranged_frames(W, H, depth, sx, sy, 2, 1)
    program(hip, rec, (mix, mix))
    seeds = hip.seed_state()
    from versatilefilmgrain_amd.hw import VfgsHipError
    if entry in ("frames_host",):
        keep = [f.copy() for f in frames]
        with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
            run_frames_host_inplace(hip, frames)
        assert all(a.equal_all(b) for a, b in zip(frames, keep))
    else:
        with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
            ENTRIES[entry](hip, frames, lambda: None)
    assert hip.lib.vfgs_hip_last_error() == E_UNSUPPORTED
    assert hip.seed_state() == seeds


def run_frames_host_inplace(hip, frames):
    f0 = frames[0]
    hip.add_grain_frames_host([f.Y.ctypes.data for f in frames], [f.U.ctypes.data for f in frames], [f.V.ctypes.data for f in frames],
                              f0.width, f0.height, f0.stride, f0.cstride)


def test_refused_device_call_leaves_planes_and_seeds(hip):
    import torch
    from gpu_util import DevFrame, stream_ptr
    from versatilefilmgrain_amd.hw import VfgsHipError
    rec = records_of("fgs_sei_10_420")
    f = X.ranged_frames(W, H, 10, 2, 2, 1, 3)[0]
    program(hip, rec, ((32, 32, 0), None))
    seeds = hip.seed_state()
    d = DevFrame(f)
    n0 = hip.last_launch_info()["launches"] if hip.last_launch_info() else 0
    with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
    torch.cuda.synchronize()
    assert d.download().equal_all(f) and hip.seed_state() == seeds
    assert (hip.last_launch_info()["launches"] if hip.last_launch_info() else 0) == n0
    # the same model WITHOUT a mix is today's call
    hip.clear_chroma_mix()
    ora = T.OracleHW()
    T.replay(ora, rec)
    want = f.copy()
    ora.add_grain_frame(want)
    hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
    assert d.download().equal_all(want) and hip.seed_state() == ora.seed_state()


FORMATS = ["fgs_afgs1_test1_10_420", "fgs_afgs1_test3_10_422", "fgs_afgs1_test1_10_444", "fgs_afgs1_test1_10_440",
           "fgs_afgs1_test1_8_420", "fgs_afgs1_test1_8_420@21", "fgs_afgs1_test1_8_444", "fgs_afgs1_test1_8_440"]


@pytest.mark.parametrize("width", [346, 333, 1042, 2048])
@pytest.mark.parametrize("name", FORMATS)
def test_formats_depths_and_ragged_widths(hip, name, width):
    """8 and 10 bit x 4:2:0, 4:2:2, 4:4:4, 4:4:0; widths that end inside a block, an odd one (the last luma sample pairs with itself), rows of
    several positions, a row that ends on a position boundary; Cb and Cr with different mixes; in place and out of place"""
    mixes = ((32, 32, 0), (64, 0, 0))
    a, got = run_and_check(hip, "frame_dev", name, mixes, width=width, height=80, nframes=2, seed=width)
    _, got2 = run_and_check(hip, "copy_dev", name, mixes, frames=a)
    assert all(x.equal_all(y) for x, y in zip(got, got2))


@pytest.mark.parametrize("entry", ["frame_dev", "frames_dev", "copy_dev", "copy8_dev", "frame_list_dev", "stripe_dev"])
def test_one_component_only_and_narrowed_destination(hip, entry):
    """a mix for Cb alone (Cr keeps the sample as its index), and for Cr alone"""
    run_and_check(hip, entry, "fgs_afgs1_test1_10_420", ((32, 32, 0), None))
    run_and_check(hip, entry, "fgs_afgs1_test1_10_444", (None, (64, 0, 0)))


@pytest.mark.parametrize("name, width", [("fgs_afgs1_test1_10_420", 8400), ("fgs_afgs1_test1_8_444", 8208), ("fgs_afgs1_test1_10_444", 16400)])
@pytest.mark.parametrize("entry", ["frame_dev", "copy_dev", "frames_dev"])
def test_rows_wider_than_8192_samples(hip, name, width, entry):
    run_and_check(hip, entry, name, ((32, 32, 0), (64, 0, 0)), width=width, height=48, nframes=2, seed=5)
    assert hip.last_launch_info()["kernel"].endswith(",true>") and hip.last_launch_info()["parts_per_row"] >= 2


def test_wide_one_pattern_model_at_422_is_refused(hip):
    from gpu_util import DevFrame, stream_ptr
    from versatilefilmgrain_amd.hw import VfgsHipError
    rec = records_of("fgs_afgs1_test3_10_422")
    f = X.ranged_frames(8400, 48, 10, 2, 1, 1, 1)[0]
    program(hip, rec, ((32, 32, 0), (32, 32, 0)))
    seeds = hip.seed_state()
    d = DevFrame(f)
    with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
    assert d.download().equal_all(f) and hip.seed_state() == seeds


@pytest.mark.parametrize("name, width, height", [("fgs_afgs1_test1_10_420", 3840, 2160), ("fgs_afgs1_test1_8_420", 7680, 4320)])
def test_luma_hazard_in_place_equals_out_of_place_at_full_size(hip, name, width, height):
    """Luma and chroma workgroups of one frame are resident together at these sizes: in place, chroma must still read the luma of
    before the call.  Two frames per call (the second one's workgroups run beside the first one's)."""
    mixes = ((32, 32, 0), (32, 32, 0))
    frames, a = run_and_check(hip, "frames_dev", name, mixes, width=width, height=height, nframes=2, seed=9)
    _, b = run_and_check(hip, "copy_dev", name, mixes, frames=frames)
    _, c = run_and_check(hip, "frame_list_dev", name, mixes, frames=frames)
    assert all(x.equal_all(y) and x.equal_all(z) for x, y, z in zip(a, b, c))


@pytest.mark.parametrize("name", ["fgs_afgs1_test1_10_420", "fgs_afgs1_test1_8_444"])
def test_full_range_content(hip, name):
    """One test per depth on full-range input: the derivation may leave out at most 3 % of the chroma samples (asserted on the oracle)."""
    rec = records_of(name)
    depth, sx, sy = T.trace_geometry(rec)
    frames, _ = T.lcg_frames(W, H, depth, sx, sy, 3)
    total = sum(f.U.size + f.V.size for f in frames)
    for entry in ("frame_dev", "copy_dev"):
        run_and_check(hip, entry, name, ((32, 32, 0), (32, 32, 0)), frames=frames, max_excluded=int(0.03 * total))


@pytest.mark.parametrize("name", ["fgs_afgs1_test1_10_420", "fgs_afgs1_test1_8_420", "fgs_afgs1_test1_8_444"])
def test_neutral_mix_equals_mix_off_byte_for_byte(hip, name):
    from gpu_util import DevFrame, stream_ptr
    rec = records_of(name)
    depth, sx, sy = T.trace_geometry(rec)
    frames = X.ranged_frames(1920, 1080, depth, sx, sy, 2, 4, lo=0.0, hi=1.0)      # in-range content: every sample inside 0 .. 2^d - 1
    out = {}
    for tag, mixes in (("off", (None, None)), ("neutral", (X.NEUTRAL, X.NEUTRAL))):
        program(hip, rec, mixes)
        devs = [DevFrame(f) for f in frames]
        for d, f in zip(devs, frames):
            hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        out[tag] = [d.download() for d in devs], hip.seed_state(), hip.last_launch_info()["kernel"]
    assert out["off"][2].startswith("grain_rw_kernel<") and out["neutral"][2].startswith("grain_mix_kernel<")
    assert all(a.equal_all(b) for a, b in zip(out["off"][0], out["neutral"][0])) and out["off"][1] == out["neutral"][1]
    ora = T.OracleHW()
    T.replay(ora, rec)
    for f, g in zip(frames, out["off"][0]):
        w = f.copy()
        ora.add_grain_frame(w)
        assert g.equal_all(w)


@pytest.mark.parametrize("how", ["clear", "reset"])
def test_after_clear_and_after_reset_the_result_is_todays(hip, how):
    from gpu_util import DevFrame, stream_ptr
    name = "fgs_afgs1_test1_10_420"
    rec = records_of(name)
    frames = X.ranged_frames(W, H, 10, 2, 2, 2, 6)
    run_and_check(hip, "frame_dev", name, ((32, 32, 0), (64, 0, 0)), frames=frames)
    if how == "clear":
        hip.clear_chroma_mix()
        T.replay(hip, rec)                    # (the same model again, seed included: the oracle below starts there too)
    else:
        hip.lib.vfgs_hip_reset_state()
        T.replay(hip, rec)
    assert hip.chroma_mix(1)[3] == 0 and hip.chroma_mix(2)[3] == 0
    ora = T.OracleHW()
    T.replay(ora, rec)
    for f in frames:
        w = f.copy()
        ora.add_grain_frame(w)
        d = DevFrame(f)
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        assert d.download().equal_all(w)
        assert hip.last_launch_info()["kernel"].startswith("grain_rw_kernel<")
    assert hip.seed_state() == ora.seed_state()


def firmware_program(hip, name):
    """vfgs_main.c:750-781 with the library's firmware: depth, subsampling, init(default), seed, init(cfg)"""
    from versatilefilmgrain_amd import fw
    depth, sx, sy = T.trace_geometry(T.load_trace(name))
    seed, cfgs = T.load_fwcfg(name)
    hip.lib.vfgs_hip_reset_state()
    hip.set_depth(depth)
    hip.set_chroma_subsampling(sx, sy)
    for i, (kind, raw) in enumerate(cfgs):
        fw.init(fw.struct_from_bytes(kind, raw))
        if i == 0:
            hip.set_seed(seed)
    return cfgs


@pytest.mark.parametrize("name, mixes", [("fgs_afgs1_test1_10_420", ((64, 119, -238), (64, 101, -202))), ("fgs_afgs1_test1_8_420", ((64, 119, -238), (64, 101, -202))),
                                         ("fgs_afgs1_test2_10_420", ((64, 0, 0), (64, 0, 0)))])
def test_firmware_path_programs_the_mix_of_the_corpus(hip, name, mixes):
    import json
    from gpu_util import DevFrame, stream_ptr
    from versatilefilmgrain_amd import fw
    rec = T.load_trace(name)
    depth, sx, sy = T.trace_geometry(rec)
    try:
        # switch off: today's picture (the reference CLI's md5)
        fw.afgs1_chroma_mix(False)
        firmware_program(hip, name)
        assert hip.chroma_mix(1)[3] == 0 and hip.chroma_mix(2)[3] == 0
        frames, _ = T.lcg_frames(192, 144, depth, sx, sy, 3)
        for f in frames:
            hip.add_grain_stripe(f.Y.ctypes.data, f.U.ctypes.data, f.V.ctypes.data, 0, f.width, f.height, f.stride, f.cstride)
        assert T.md5_frames(frames) == json.loads((T.GOLDEN / "md5.json").read_text())["small"][name]
        # switch on
        fw.afgs1_chroma_mix(True)
        cfgs = firmware_program(hip, name)
        assert (hip.chroma_mix(1), hip.chroma_mix(2)) == (mixes[0] + (1,), mixes[1] + (1,))
        frames = X.ranged_frames(W, H, depth, sx, sy, 2, 8, lo=0.4, hi=0.6, clo=0.4, chi=0.5)
        res, ora = expect(rec, frames, mixes)
        got = []
        for f in frames:
            d = DevFrame(f)
            hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
            got.append(d.download())
        check(got, res)
        assert hip.seed_state() == ora.seed_state()
        # an SEI model afterwards clears the mix
        fw.init(fw.struct_from_bytes(*cfgs[0]))
        assert hip.chroma_mix(1)[3] == 0 and hip.chroma_mix(2)[3] == 0
    finally:
        fw.afgs1_chroma_mix(False)


def test_line_call_with_a_mix_does_not_work_ahead_and_sees_late_luma_edits(hip):
    """The drop-in line call under a mix: every line is computed when it is handed over, from the luma and chroma of that moment"""
    name = "fgs_afgs1_test1_10_420"
    rec = records_of(name)
    mixes = ((32, 32, 0), (32, 32, 0))
    frames = X.ranged_frames(W, H, 10, 2, 2, 2, 11)
    res, ora = expect(rec, frames, mixes)
    program(hip, rec, mixes)
    hip.line_lookahead(True)
    got = [f.copy() for f in frames]
    for f in got:
        keep = f.Y[100].copy()
        f.Y[100] = 0                          # a caller that fills in a line late ...
        for y in range(f.height):
            if y == 100:
                f.Y[100] = keep               # ... but before it hands it over
            hip.add_grain_line(f.Y[y].ctypes.data, f.U[y // 2].ctypes.data, f.V[y // 2].ctypes.data, y, f.width)
    check(got, res)
    assert hip.seed_state() == ora.seed_state()
