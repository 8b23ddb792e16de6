"""GPU (MI355X): sample depth 12 through the C ABI, bit-exact against the oracle (oracle/vfgs_oracle.c, written in bs = depth - 8 like the
reference's hardware layer: intensity (I >> 4) & 0xff, clip limits I_min << 4 and I_max << 4, scale shift shift + 6 - 4): every sample
of every plane, row padding included, and the four seed registers; no tolerance, nothing left out.

The configurations are the 10-bit traces of tests/golden/traces with their depth record replaced by 12 when they are loaded (both
implementations are programmed from the same records); 'trace@XY' also replaces the chroma subsampling.  One runner per entry point,
as in tests/test_gpu_chroma_mix.py (whose runners are used where they do not depend on the depth).  The fused 8-bit output at depth
12 is (v + 8) >> 4 of the grained, clipped sample.
"""
import numpy as np
import pytest

import vfgs_testlib as T
import test_gpu_chroma_mix as M

pytestmark = pytest.mark.gpu

W, H = 320, 192
E_OUT8_DEPTH, E_UNSUPPORTED = 16, 38
TRACES_10 = [n for n in T.list_traces() if "_10_" in n]
# (the corpus holds fgs_sei_ff_test6 at 4:2:2 as an 8-bit recording only; the firmware's output does not depend on the depth -- the
# recordings of one model differ in their depth record alone -- so that trace with its depth record replaced is the 4:2:2 case)
FF6_422 = "fgs_sei_ff_test6_8_422"
FIVE = ["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_afgs1_test1_10_444", FF6_422, "fgs_sei_10_420@12"]


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    assert h.lib.vfgs_hip_supports_depth(12) == 1      # (asked first: vfgs_set_depth is a void drop-in call and aborts on a depth it does not have)
    yield h
    h.lib.vfgs_hip_reset_state()


def records12(name, legal=None, depth=12):
    """the trace `name` ('trace@XY': chroma subsampling X, Y) with its depth record replaced; legal: its range record too"""
    rec = M.records_of(name)
    assert (T.trace_geometry(rec)[0] == 10 or name == FF6_422) and sum(op == T.OP_DEPTH for op, *_ in rec) >= 1
    out = []
    for op, a, b, p in rec:
        if op == T.OP_DEPTH:
            a = depth
        elif op == T.OP_LEGAL_RANGE and legal is not None:
            a = legal
        out.append((op, a, b, p))
    if legal is not None and not any(op == T.OP_LEGAL_RANGE for op, *_ in out):
        out.append((T.OP_LEGAL_RANGE, legal, 0, b""))
    return out


def oracle_for(rec):
    ora = T.OracleHW()
    T.replay(ora, rec)
    return ora


def program(hip, rec):
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, rec)


def narrowed12(f):
    """the 8-bit picture of a 12-bit frame: (v + 8) >> 4, same geometry in samples (as uint8, like the store)"""
    g = T.Frame(f.width, f.height, 8, f.subx, f.suby, f.stride, f.cstride)
    for a, b in zip(g.planes(), f.planes()):
        a[...] = ((b.astype(np.int32) + 8) >> 4).astype(np.uint8)
    return g


def garbage_frames(n, width, height, sx, sy, seed, top=1 << 16):
    """every sample of every plane, the row padding included, anything below `top` (65536: containers that hold values above 4095)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        f = T.Frame(width, height, 12, sx, sy)
        for p in f.planes():
            p[...] = rng.integers(0, top, p.shape).astype(f.dtype)
        out.append(f)
    return out


# ---- runners: frames in -> frames out, the seed registers left as after whole frames (the depth-independent ones: test_gpu_chroma_mix) ----

def run_copy8_dev(hip, frames, reprogram):
    from gpu_util import stream_ptr
    f0 = frames[0]
    src, dst = M.stack(frames), M.stack([narrowed12(f) for f in frames])
    hip.add_grain_copy8_dev(*[t.data_ptr() for t in src], *[t.data_ptr() for t in dst], f0.width, f0.height, 0, f0.height, f0.stride, f0.cstride,
                            f0.stride, f0.cstride, len(frames), src[0][0].numel(), src[1][0].numel(), dst[0][0].numel(), dst[1][0].numel(), stream_ptr())
    for a, b in zip(M.unstack(src, frames), frames):
        assert a.equal_all(b), "the source of an out-of-place call changed"
    return M.unstack(dst, [narrowed12(f) for f in frames])


def run_list_copy8_dev(hip, frames, reprogram):
    from gpu_util import DevFrame, stream_ptr
    f0 = frames[0]
    src, dst = [DevFrame(f) for f in frames], [DevFrame(narrowed12(f)) for f in frames]
    hip.add_grain_frame_list_copy8_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], f0.width, f0.height, f0.stride, f0.cstride,
                                       f0.stride, f0.cstride, stream_ptr())
    return [d.download() for d in dst]


def run_overlap_region(hip, frames, reprogram):
    """device-resident frames one per call inside an overlap region (two internal streams)"""
    from gpu_util import DevFrame, stream_ptr
    devs = [DevFrame(f) for f in frames]
    hip.overlap_begin(stream_ptr())
    for d, f in zip(devs, frames):
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
    hip.overlap_end(stream_ptr())
    return [d.download() for d in devs]


def run_line_lookahead(hip, frames, reprogram):
    """the drop-in line call with the frame declared: the library works ahead from the first line on"""
    out = [f.copy() for f in frames]
    hip.line_lookahead(True)
    try:
        for f in out:
            hip.declare_frame(f.Y.ctypes.data, f.U.ctypes.data, f.V.ctypes.data, f.width, f.height, f.stride, f.cstride)
            for y in range(f.height):
                hip.add_grain_line(f.Y[y].ctypes.data, f.U[y // f.suby].ctypes.data, f.V[y // f.suby].ctypes.data, y, f.width)
    finally:
        hip.declare_frame(None, None, None, 0, 0, 0, 0)
    return out


ENTRIES = dict(M.ENTRIES)
ENTRIES.update({"copy8_dev": run_copy8_dev, "frame_list_copy8_dev": run_list_copy8_dev, "overlap_region": run_overlap_region,
                "add_grain_line_lookahead": run_line_lookahead})
OUT8 = M.OUT8


def run_and_check(hip, entry, rec, frames, closed_form=False):
    ora = oracle_for(rec)
    want = [f.copy() for f in frames]
    for w in want:
        ora.add_grain_frame(w, closed_form=closed_form)
    reprogram = lambda: program(hip, rec)
    reprogram()
    got = ENTRIES[entry](hip, frames, reprogram)
    if entry in OUT8:
        want = [narrowed12(w) for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        for pl, a, b in zip("YUV", g.planes(), w.planes()):
            n = int(np.count_nonzero(a != b))
            assert n == 0, f"{entry}: frame {i} plane {pl}: {n} samples differ from the oracle"
    assert hip.seed_state() == ora.seed_state()
    info = hip.last_launch_info()
    assert info["depth"] == 12 and info["kernel"].startswith("grain_rw_kernel<12,") and info["out8"] == (entry in OUT8), info
    return got, want


# ---- every 10-bit trace ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TRACES_10)
def test_every_10_bit_trace_at_depth_12(hip, name):
    rec = records12(name)
    depth, sx, sy = T.trace_geometry(rec)
    assert depth == 12
    frames, _ = T.lcg_frames(192, 144, 12, sx, sy, 3)
    got, want = run_and_check(hip, "frame_dev", rec, frames)
    # grain was added, and nothing leaves the full range's 255 << 4 (vfgs_hw.c:265)
    changed = sum(int(np.count_nonzero(a != b)) for g, f in zip(got, frames) for a, b in zip(g.planes(), f.planes()))
    assert changed > 0 and max(int(p.max()) for g in got for p in g.planes()) <= 255 << 4


# ---- every entry point ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIVE)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_entry_point(hip, entry, name):
    rec = records12(name)
    _, sx, sy = T.trace_geometry(rec)
    frames, _ = T.lcg_frames(W, H, 12, sx, sy, 3, state=7)
    run_and_check(hip, entry, rec, frames)
    info = hip.last_launch_info()
    assert (info["csubx"], info["csuby"]) == (sx, sy), info
    if "afgs1" in name or name.startswith("fgs_sei_10_420"):      # (the AFGS1 models: one pattern; the default SEI model: eight luma patterns)
        assert info["one_y"] == ("afgs1" in name), info


# ---- row geometry ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [333, 346, 1042])
@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_afgs1_test1_10_444", FF6_422, "fgs_sei_10_420@12"])
def test_ragged_widths(hip, name, width):
    rec = records12(name)
    _, sx, sy = T.trace_geometry(rec)
    frames, _ = T.lcg_frames(width, 80, 12, sx, sy, 2, state=width, garbage_padding=True)
    a, _ = run_and_check(hip, "frame_dev", rec, frames)
    b, _ = run_and_check(hip, "frames_dev", rec, frames)
    assert all(x.equal_all(y) for x, y in zip(a, b))
    run_and_check(hip, "copy8_dev", rec, frames)


@pytest.mark.parametrize("entry", ["frame_dev", "copy_dev", "copy8_dev", "frame_list_dev"])
@pytest.mark.parametrize("name, width", [("fgs_sei_10_420", 8400), ("fgs_afgs1_test1_10_420", 8400), ("fgs_afgs1_test1_10_444", 16400),
                                         ("fgs_sei_10_420", 16400), (FF6_422, 8400)])
def test_rows_wider_than_8192_samples(hip, name, width, entry):
    rec = records12(name)
    _, sx, sy = T.trace_geometry(rec)
    frames, _ = T.lcg_frames(width, 48, 12, sx, sy, 2, state=5)
    run_and_check(hip, entry, rec, frames)
    info = hip.last_launch_info()
    assert info["parts_per_row"] >= 2 and info["kernel"].endswith(",true,false>"), info


@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_sei_10_444"])
@pytest.mark.parametrize("entry", ["frames_dev", "copy_dev", "copy8_dev"])
def test_small_general_form_picture_takes_the_persistent_path(hip, name, entry):
    rec = records12(name)
    _, sx, sy = T.trace_geometry(rec)
    frames = garbage_frames(230, 384, 224, sx, sy, 300)
    run_and_check(hip, entry, rec, frames)
    info = hip.last_launch_info()
    assert info["persistent_luma_workgroups"] > 0 and info["kernel"].endswith(",true>") and info["one_y"] == 0, info
    assert info["persistent_luma_workgroups"] <= 4 * hip.device_info()["cu_count"]


@pytest.mark.parametrize("name, entry", [("fgs_afgs1_test1_10_444", "frames_dev"), ("fgs_afgs1_test1_10_444", "copy_dev")])
def test_two_frame_fronts(hip, name, entry):
    """an odd number of large frames in one launch: two are swept at a time, the last front is half empty"""
    rec = records12(name)
    _, sx, sy = T.trace_geometry(rec)
    frames, _ = T.lcg_frames(3840, 2160, 12, sx, sy, 3, state=3)
    run_and_check(hip, entry, rec, frames, closed_form=True)
    assert hip.last_launch_info()["frames_per_front"] == 2, hip.last_launch_info()


# ---- value ranges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_10_444", FF6_422])
def test_legal_range(hip, name):
    rec = records12(name, legal=1)
    _, sx, sy = T.trace_geometry(rec)
    frames, _ = T.lcg_frames(W, H, 12, sx, sy, 2, state=2)
    for entry in ("frame_dev", "copy8_dev"):
        got, want = run_and_check(hip, entry, rec, frames)
    # (the oracle's own picture: 16 << 4 .. 235 << 4 for luma, .. 240 << 4 for chroma, vfgs_hw.c:265,366-378)
    got, want = run_and_check(hip, "frame_dev", rec, frames)
    for w in want:
        assert w.Y[:H, :W].min() >= 16 << 4 and w.Y[:H, :W].max() == 235 << 4
        assert w.U[:H // sy, :W // sx].max() <= 240 << 4 and w.U[:H // sy, :W // sx].min() >= 16 << 4
    full, _ = run_and_check(hip, "frame_dev", records12(name, legal=0), frames)
    assert max(int(f.Y.max()) for f in full) == 255 << 4       # full range clips at 4080, not at 4095


def extreme_records(name, shift, lowest):
    """scale 255 for every intensity, patterns of +-127 (lowest = -128: the value the one-pattern form cannot negate), the given shift:
    the largest products and the largest grain the arithmetic can meet (stored shift 4 at shift 2: entries of 255 << 12)"""
    rng = np.random.default_rng(100 * shift - lowest)
    rec = [r for r in records12(name) if r[0] not in (T.OP_SCALE_SHIFT,)]
    out = []
    for op, a, b, p in rec:
        if op in (T.OP_LUMA_PATTERN, T.OP_CHROMA_PATTERN):
            n = len(p)
            if a % 2 == 0:
                P = np.full(n, lowest, np.int8)      # whole blocks at the extreme (the block signs make it +-): the blend and the edge filter at their largest
            else:
                P = rng.choice(np.array([lowest, lowest, 127, 127, 127, lowest, -1, 1], dtype=np.int8), size=n).astype(np.int8)
            p = P.tobytes()
        elif op == T.OP_SCALE_LUT:
            p = bytes([255]) * len(p)
        out.append((op, a, b, p))
    out.append((T.OP_SCALE_SHIFT, shift, 0, b""))
    return out


@pytest.mark.parametrize("lowest", [-127, -128])
@pytest.mark.parametrize("shift", [2, 7])
@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_afgs1_test1_10_444"])
def test_range_derivation_at_its_limit(hip, name, shift, lowest):
    rec = extreme_records(name, shift, lowest)
    _, sx, sy = T.trace_geometry(rec)
    program(hip, rec)
    assert hip.params()["bs"] == 4 and hip.params()["scale_shift"] == shift + 2
    assert all(set(hip.luts(c)[0]) == {255} for c in range(3))
    lcg, _ = T.lcg_frames(1936, 112, 12, sx, sy, 2, state=shift)
    for frames in (lcg, garbage_frames(2, 1936, 112, sx, sy, shift)):
        for entry in ("frame_dev", "copy8_dev"):
            got, want = run_and_check(hip, entry, rec, frames)
    info = hip.last_launch_info()
    if "afgs1" in name:
        assert info["one_y"] == (lowest == -127), info      # -128 has no negation in a byte: the general form serves it


@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_afgs1_test1_10_444", FF6_422])
@pytest.mark.parametrize("entry", ["frame_dev", "copy_dev", "copy8_dev", "add_grain_stripe", "frames_host"])
def test_containers_above_4095_and_garbage_row_padding(hip, name, entry):
    """a uint16 may hold anything: the intensity wraps ((I >> 4) & 0xff), the sum is clipped; row padding beyond the last block keeps its bytes"""
    rec = records12(name)
    _, sx, sy = T.trace_geometry(rec)
    frames = garbage_frames(2, 346, H, sx, sy, 17)
    assert max(int(f.Y.max()) for f in frames) > 0xf000
    got, want = run_and_check(hip, entry, rec, frames)
    if entry not in OUT8:
        f0 = frames[0]
        assert np.array_equal(got[0].Y[:, 352:], f0.Y[:, 352:]) and f0.stride > 352      # behind the last whole block: the caller's bytes


# ---- state ----------------------------------------------------------------------------------------------------------------------

def test_depth_switches_within_one_process_equal_fresh_state(hip):
    """8 -> 12 -> 10 -> 12 without a reset in between: every depth's result is the one a fresh state gives"""
    from gpu_util import DevFrame, stream_ptr
    hip.lib.vfgs_hip_reset_state()
    sei12, afgs12 = records12("fgs_sei_10_420"), records12("fgs_afgs1_test1_10_420")
    steps = [("sei", 8, T.load_trace("fgs_sei_8_420")), ("sei", 12, sei12), ("sei", 10, T.load_trace("fgs_sei_10_420")), ("sei", 12, sei12),
             ("afgs1", 12, afgs12), ("afgs1", 8, T.load_trace("fgs_afgs1_test1_8_420")), ("afgs1", 12, afgs12)]
    results = {}
    for k, (tag, depth, rec) in enumerate(steps):
        T.replay(hip, rec)           # (a trace programs everything, the depth and the seed included)
        ora = oracle_for(rec)
        frames, _ = T.lcg_frames(W, H, depth, 2, 2, 2, state=9)
        for f in frames:
            d = DevFrame(f)
            hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
            ora.add_grain_frame(f)
            assert d.download().equal_all(f), (k, depth)
        assert hip.seed_state() == ora.seed_state() and hip.last_launch_info()["depth"] == depth
        results.setdefault((tag, depth), []).append(T.md5_frames(frames))
    assert len(results[("sei", 12)]) == 2 and len(results[("afgs1", 12)]) == 2 and all(len(set(v)) == 1 for v in results.values())
    # and the fresh state
    frames, _ = T.lcg_frames(W, H, 12, 2, 2, 2, state=9)
    got, _ = run_and_check(hip, "frame_dev", sei12, frames)
    assert T.md5_frames(got) == results[("sei", 12)][0]


def test_reset_state_returns_to_8_bit(hip):
    program(hip, records12("fgs_sei_10_420"))
    assert hip.params()["bs"] == 4
    hip.lib.vfgs_hip_reset_state()
    p = hip.params()
    assert p["bs"] == 0 and p["scale_shift"] == 5 + 6
    rec = T.load_trace("fgs_sei_8_420")
    frames, _ = T.lcg_frames(W, H, 8, 2, 2, 1)
    from gpu_util import DevFrame, stream_ptr
    T.replay(hip, rec)
    ora = oracle_for(rec)
    d = DevFrame(frames[0])
    hip.add_grain_frame_dev(*d.ptrs(), W, H, frames[0].stride, frames[0].cstride, stream_ptr())
    ora.add_grain_frame(frames[0])
    assert d.download().equal_all(frames[0]) and hip.last_launch_info()["depth"] == 8


def test_copy8_is_refused_at_depth_8_only(hip):
    from versatilefilmgrain_amd.hw import VfgsHipError
    rec = T.load_trace("fgs_sei_8_420")
    program(hip, rec)
    frames, _ = T.lcg_frames(W, H, 8, 2, 2, 1)
    seeds = hip.seed_state()
    with pytest.raises(VfgsHipError, match=f"error {E_OUT8_DEPTH}"):
        M.run_copy8_dev(hip, frames, None)
    assert hip.seed_state() == seeds


@pytest.mark.parametrize("entry", sorted(set(M.ENTRIES) - set(M.VOID)) + ["overlap_region"])
def test_active_mix_at_depth_12_is_refused_and_changes_nothing(hip, entry):
    """the kernels of the luma / chroma mix exist at 8 and 10 bit: error 38, planes and seed registers as before, nothing launched"""
    import torch
    from gpu_util import DevFrame, stream_ptr
    from versatilefilmgrain_amd.hw import VfgsHipError
    rec = records12("fgs_afgs1_test1_10_420")       # (a one-pattern model: at 10 bit the mix serves it)
    frames, _ = T.lcg_frames(W, H, 12, 2, 2, 2, state=4)
    program(hip, rec)
    hip.set_chroma_mix(1, 32, 32, 0)
    seeds = hip.seed_state()
    n0 = (hip.last_launch_info() or {"launches": 0})["launches"]
    try:
        if entry == "frames_host":
            keep = [f.copy() for f in frames]
            with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
                M.run_frames_host_inplace(hip, frames)
            assert all(a.equal_all(b) for a, b in zip(frames, keep))
        elif entry == "overlap_region":
            d = DevFrame(frames[0])
            hip.overlap_begin(stream_ptr())
            try:
                with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
                    hip.add_grain_frame_dev(*d.ptrs(), W, H, frames[0].stride, frames[0].cstride, stream_ptr())
            finally:
                hip.overlap_end(stream_ptr())
            assert d.download().equal_all(frames[0])
        elif entry == "frame_dev":
            d = DevFrame(frames[0])
            with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
                hip.add_grain_frame_dev(*d.ptrs(), W, H, frames[0].stride, frames[0].cstride, stream_ptr())
            assert d.download().equal_all(frames[0])
        else:
            with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
                ENTRIES[entry](hip, frames, lambda: None)
        torch.cuda.synchronize()
        assert hip.lib.vfgs_hip_last_error() == E_UNSUPPORTED
        assert hip.seed_state() == seeds
        assert (hip.last_launch_info() or {"launches": 0})["launches"] == n0
        # the mix cleared: the call of always
        hip.clear_chroma_mix()
        run_and_check(hip, "frame_dev", rec, frames)
    finally:
        hip.clear_chroma_mix()


# ---- firmware, several devices --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_sei_10_422", "fgs_sei_ff_test6_10_444", "fgs_sei_ar_test1_10_420"])
def test_firmware_chain_at_depth_12_equals_the_trace_replay(hip, name):
    """vfgs_main.c:750-781 with the library's firmware and depth 12: the configuration the reference CLI handed to ITS firmware (tests/golden/fwcfg)
    programs the same state as the recorded trace with its depth record replaced"""
    from gpu_util import DevFrame, stream_ptr
    from versatilefilmgrain_amd import fw
    rec = records12(name)
    _, sx, sy = T.trace_geometry(rec)
    seed, cfgs = T.load_fwcfg(name)
    hip.lib.vfgs_hip_reset_state()
    hip.set_depth(12)
    hip.set_chroma_subsampling(sx, sy)
    for i, (kind, raw) in enumerate(cfgs):
        fw.init(fw.struct_from_bytes(kind, raw))
        if i == 0:
            hip.set_seed(seed)
    assert hip.params()["bs"] == 4 and hip.chroma_mix(1)[3] == 0 and hip.chroma_mix(2)[3] == 0
    ora = oracle_for(rec)
    frames, _ = T.lcg_frames(192, 144, 12, sx, sy, 3)
    for i, f in enumerate(frames):
        d = DevFrame(f)
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        ora.add_grain_frame(f)
        assert d.download().equal_all(f), i
    assert hip.seed_state() == ora.seed_state() and hip.last_launch_info()["depth"] == 12


@pytest.mark.parametrize("name, width, height", [("fgs_sei_10_420", 416, 240), ("fgs_afgs1_test1_10_444", 200, 152), ("fgs_sei_10_420", 1920, 1080)])
def test_init_devices_with_device_0_listed_twice(hip, name, width, height):
    rec = records12(name)
    _, sx, sy = T.trace_geometry(rec)
    hip.init_devices([0, 0])
    try:
        frames = garbage_frames(5, width, height, sx, sy, width)
        run_and_check(hip, "frames_host", rec, frames)
        if height >= 144:
            run_and_check(hip, "add_grain_stripe", rec, frames[:2])
        # the device-pointer entries stay on the primary device
        run_and_check(hip, "frame_dev", rec, frames[:2])
    finally:
        hip.init_devices([0])


# ---- full size ------------------------------------------------------------------------------------------------------------------

def test_full_size_batch_in_one_launch_equals_the_closed_form(hip):
    """7680x4320 4:2:0 x 8 in one launch (the shape tests/test_gpu_soak.py checks at 10 bit and bench.py times) against the oracle's closed form"""
    import torch
    w, hh, batch, sx, sy = 7680, 4320, 8, 2, 2
    rec = records12("fgs_sei_10_420")
    program(hip, rec)
    ora = oracle_for(rec)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(12)
    mk = lambda r, c: torch.randint(0, 1 << 12, (batch, r, c), dtype=torch.int32, device="cuda", generator=g).to(torch.int16)
    Y, U, V = mk(hh, w), mk(hh // sy, w // sx), mk(hh // sy, w // sx)
    src = tuple(t.cpu().numpy().view(np.uint16) for t in (Y, U, V))
    torch.cuda.synchronize()
    hip.add_grain_frames_part_dev(Y.data_ptr(), U.data_ptr(), V.data_ptr(), w, hh, 0, hh, w, w // sx, batch, Y[0].numel() * 2, U[0].numel() * 2, st)
    torch.cuda.synchronize()
    info = hip.last_launch_info()
    assert info["launches"] and info["nframes"] == batch and info["frames_per_front"] == 2 and info["kernel"].startswith("grain_rw_kernel<12,2,2,false,false,true,"), info
    got = tuple(t.cpu().numpy().view(np.uint16) for t in (Y, U, V))
    bad = []
    for f in range(batch):
        fr = T.Frame(w, hh, 12, sx, sy, stride=w, cstride=w // sx)
        fr.Y[:hh], fr.U[:hh // sy], fr.V[:hh // sy] = src[0][f], src[1][f], src[2][f]
        ora.add_grain_frame(fr, closed_form=True)
        if not (np.array_equal(fr.Y[:hh], got[0][f]) and np.array_equal(fr.U[:hh // sy], got[1][f]) and np.array_equal(fr.V[:hh // sy], got[2][f])):
            bad.append(f)
    assert not bad, f"frames that differ from the oracle: {bad}"
    assert hip.seed_state() == ora.seed_state()
