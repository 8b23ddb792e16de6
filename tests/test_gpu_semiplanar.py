"""GPU (MI355X): vfgs_hip_add_grain_sp_frame_list_dev -- semi-planar frames (NV12 / NV16 / P010 / P210 / P012) -- against the oracle,
through the C ABI, bit for bit: every container of both planes of every frame, padding included, and the four seed registers.

The contract (include/vfgs_hip.h) is stated on D(p), the planar low-aligned picture of a semi-planar picture p; the expectation is
tests/semiplanar_util.py's (the unchanged oracle on D(p), interleaved and shifted back; pinned against recorded reference output by
tests/test_semiplanar_util_cpu.py).  Frames are separate allocations listed out of address order, with garbage over the full container
range in both planes.  Shapes are the smallest that reach each mechanism: a UV position is 2 KiB -- 1024 luma samples of a row at 16-bit
containers, 2048 at 8 bit.

Widths 16 and 48: the call is defined as the planar copy list on D(p), and every planar entry point refuses pictures of 128 samples and
narrower with error 5 (vfgs_hw.c:168, which the oracle restates) -- "bad geometry keeps its code".  Those two widths are therefore
asserted as that refusal, with nothing changed."""
import ctypes as C

import numpy as np
import pytest

import model_programs as MP
import semiplanar_util as SP
import vfgs_testlib as T
from gpu_util import stream_ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


class DevSP:
    """an SPFrame resident on the GPU, an allocation per plane"""

    def __init__(self, sp):
        import torch
        self.sp = sp
        self.Y = torch.from_numpy(sp.Y.view(np.uint8).copy()).cuda()
        self.UV = torch.from_numpy(sp.UV.view(np.uint8).copy()).cuda()

    def ptrs(self):
        return (self.Y.data_ptr(), self.UV.data_ptr())

    def download(self):
        import torch
        torch.cuda.synchronize()
        g = self.sp.copy()
        g.Y[...] = self.Y.cpu().numpy().view(g.dtype)
        g.UV[...] = self.UV.cpu().numpy().view(g.dtype)
        return g


def scattered(frames, seed=0):
    """one device allocation per plane and frame, allocated in a shuffled order: list order != address order"""
    order = np.random.default_rng(seed).permutation(len(frames))
    dev = [None] * len(frames)
    for i in order:
        dev[i] = DevSP(frames[i])
    return dev


def records_of(name):
    if name.endswith("@depth12"):
        import test_gpu_depth12 as D
        return D.records12(name.split("@")[0])
    if name.startswith("fgs_"):
        return T.load_trace(name)
    return MP.program(name)


def program(hip, name):
    rec = records_of(name)
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, rec)
    ora = T.OracleHW()
    T.replay(ora, rec)
    return ora, T.trace_geometry(rec)


def mk(n, w, h, depth, sy, shift, seed):
    return [SP.garbage_sp_frame(w, h, depth, sy, shift, seed + i) for i in range(n)]


def launches(hip):
    return (hip.last_launch_info() or {"launches": 0})["launches"]


def assert_equal(got, want, what=""):
    for plane in ("Y", "UV"):
        a, b = getattr(got, plane), getattr(want, plane)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what} plane {plane}: {len(bad)} containers differ, first at {tuple(bad[0])}: got {a[tuple(bad[0])]:#x}, want {b[tuple(bad[0])]:#x}")


def run_in_place(hip, ora, frames, seeds=None, shuffle=0, stream=None):
    shift = frames[0].shift
    want = SP.expected(ora, frames, seeds, shift)
    dev = scattered(frames, shuffle)
    f0 = frames[0]
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, seeds, f0.width, f0.height, f0.stride, f0.uv_stride, shift,
                                    stream_ptr() if stream is None else stream)
    for i, (d, w) in enumerate(zip(dev, want)):
        assert_equal(d.download(), w, f"frame {i}")
    assert hip.seed_state() == ora.seed_state()
    return dev


# ---- every kernel class ---------------------------------------------------------------------------------------------------------

CLASSES = ["fgs_sei_10_420", "fgs_sei_8_420", "fgs_afgs1_test1_8_420", "fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_422",
           "fgs_sei_ff_test6_8_422", "fgs_sei_10_420@depth12", "one_y_general_c_10_420", "general_y_one_c_8_422", "general_runs_8_420"]


@pytest.mark.parametrize("name", CLASSES)
def test_every_kernel_class(hip, name):
    """7 frames of 1032 x 90 (65 blocks, a ragged last block row), in place, low-aligned samples, one launch"""
    ora, (depth, sx, sy) = program(hip, name)
    assert sx == 2
    n0 = launches(hip)
    run_in_place(hip, ora, mk(7, 1032, 90, depth, sy, 0, 10))
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 1 and info["nframes"] == 7 and info["listed"] == 1 and info["in_place"] == 1 and info["depth"] == depth, info
    one = lambda v: "true" if v else "false"
    assert info["kernel"] == f"grain_sp_kernel<{depth},{sy},{one(info['one_y'])},{one(info['one_c'])}>", info
    assert info["kernel"].startswith("grain_sp_kernel<")


def test_all_four_forms(hip):
    """general / one-pattern luma over general / one-pattern chroma: each form's kernel is launched and named (three frames each)"""
    seen = {}
    for name in ("general_runs_8_420", "fgs_sei_10_420", "one_y_general_c_10_420", "fgs_afgs1_test1_10_420"):
        ora, (depth, sx, sy) = program(hip, name)
        run_in_place(hip, ora, mk(3, 1032, 90, depth, sy, 0, 20))
        info = hip.last_launch_info()
        seen[(info["one_y"], info["one_c"])] = info["kernel"]
    one = lambda v: "true" if v else "false"
    assert set(seen) == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen
    assert all(k.startswith("grain_sp_kernel<") and k.endswith(f"{one(y)},{one(c)}>") for (y, c), k in seen.items()), seen


# ---- high-aligned samples -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_sei_10_422", "fgs_sei_10_420@depth12", "one_same_slot_12_422"])
def test_high_aligned_samples(hip, name):
    """P010 / P210 (shift 6) and P012 (shift 4), general and one-pattern models; the sources' low bits are random and ignored, the
    written containers' low bits are zero"""
    ora, (depth, sx, sy) = program(hip, name)
    shift = 16 - depth
    frames = mk(3, 1032, 90, depth, sy, shift, 40)
    assert any((f.Y & ((1 << shift) - 1)).any() for f in frames)
    dev = run_in_place(hip, ora, frames, shuffle=1)
    rows, crows, cols = SP.written_region(frames[0])
    for d in dev:
        g = d.download()
        assert not (g.Y[:rows, :cols] & ((1 << shift) - 1)).any() and not (g.UV[:crows, :cols] & ((1 << shift) - 1)).any()


# ---- row geometry ---------------------------------------------------------------------------------------------------------------

WIDTHS = [16, 48, 136, 1016, 1024, 1032, 2056, 4104, 8192]
HEIGHTS = [16, 17, 33, 70]
GROUPS = {"8bit": "fgs_afgs1_test1_8_420", "10bit": "fgs_sei_10_420", "422": "fgs_sei_ff_test6_8_422"}
# every width with a height in turn, in every group (27 combinations; every height at least twice a group); the 4:2:2 group alternates its
# depth through the widths' second half
GEOMETRY = [(g, w, HEIGHTS[(i + k) % 4]) for k, g in enumerate(GROUPS) for i, w in enumerate(WIDTHS)]


@pytest.mark.parametrize("group,width,height", GEOMETRY)
def test_row_geometry(hip, group, width, height):
    from versatilefilmgrain_amd.hw import VfgsHipError
    name = GROUPS[group]
    if group == "422" and WIDTHS.index(width) % 2:
        name = "fgs_sei_10_422"
    ora, (depth, sx, sy) = program(hip, name)
    frames = mk(3, width, height, depth, sy, 0, width + height)
    if width <= 128:
        # the planar calls' own refusal (module docstring): error 5, nothing changes
        dev = scattered(frames)
        st0 = hip.seed_state()
        f0 = frames[0]
        with pytest.raises(VfgsHipError, match="error 5"):
            hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, None, width, height, f0.stride, f0.uv_stride, 0, stream_ptr())
        assert hip.seed_state() == st0
        for d, f in zip(dev, frames):
            assert_equal(d.download(), f)
        return
    run_in_place(hip, ora, frames, shuffle=2)
    info = hip.last_launch_info()
    unit_samples = 64 * 32 // (2 if depth > 8 else 1)     # containers of a UV position
    nblk = (width + 15) // 16
    assert info["positions_per_row"][1] == (-(-nblk * 16 // (unit_samples // 64)) + 64) // 64, info


def test_geometry_covers_every_width_and_height_in_every_group():
    assert len(GEOMETRY) >= 20
    for g in GROUPS:
        assert {w for gg, w, _ in GEOMETRY if gg == g} == set(WIDTHS) and {h for gg, _, h in GEOMETRY if gg == g} == set(HEIGHTS)


# ---- out of place, seeds ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shift", [("fgs_sei_10_420", 6), ("fgs_afgs1_test1_8_420", 0), ("fgs_sei_10_422", 0)])
def test_out_of_place_with_seeds(hip, name, shift):
    """src[f] -> dst[f] with a seed per picture; one pair in place; the sources stay as they were; the destination's padding is never written"""
    ora, (depth, sx, sy) = program(hip, name)
    frames = mk(6, 1032, 90, depth, sy, shift, 30)
    seeds = [0, 0x80000000, 0xFFFFFFFF, 12345, 12345, 0x5eed1e55]
    want = SP.expected(ora, frames, seeds, shift)
    src = scattered(frames, 6)
    fill = SP.garbage_sp_frame(1032, 90, depth, sy, shift, 999)
    dst = [DevSP(fill) for _ in frames]
    dst[2] = src[2]
    f0 = frames[0]
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], seeds, f0.width, f0.height, f0.stride, f0.uv_stride, shift, stream_ptr())
    rows, crows, cols = SP.written_region(f0)
    for i, (s, d, w, f) in enumerate(zip(src, dst, want, frames)):
        g = d.download()
        if i == 2:
            assert_equal(g, w, "the pair in place")
            continue
        e = fill.copy()
        e.Y[:rows, :cols] = w.Y[:rows, :cols]
        e.UV[:crows, :cols] = w.UV[:crows, :cols]
        assert_equal(g, e, f"destination {i}")         # what is written, and the padding as it was
        assert_equal(s.download(), f, f"source {i}")
    assert hip.seed_state() == ora.seed_state()
    info = hip.last_launch_info()
    assert info["in_place"] == 0 and info["kernel"].startswith("grain_sp_kernel<"), info
    assert hip.seeded_stream_stats()["last_launch_used_it"]


def test_one_seed_sequence_across_entry_points(hip):
    """a planar frame, a semi-planar list without seeds, a planar list, vfgs_set_seed + a semi-planar list of one, a seeded semi-planar
    list: the registers equal the oracle's after each step"""
    from gpu_util import DevFrame
    from test_gpu_frame_list import garbage_frame
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    W, H = 520, 70

    def planar(n, seed):
        fr = [garbage_frame(W, H, depth, sx, sy, seed + i) for i in range(n)]
        want = [f.copy() for f in fr]
        for w in want:
            ora.add_grain_frame(w)
        dev = [DevFrame(f) for f in fr]
        if n == 1:
            hip.add_grain_frame_dev(*dev[0].ptrs(), W, H, fr[0].stride, fr[0].cstride, stream_ptr())
        else:
            hip.add_grain_frame_list_dev([d.ptrs() for d in dev], W, H, fr[0].stride, fr[0].cstride, stream_ptr())
        for d, w in zip(dev, want):
            assert d.download().equal_all(w)
        assert hip.seed_state() == ora.seed_state()

    planar(1, 0)
    run_in_place(hip, ora, mk(5, W, H, depth, sy, 6, 100), shuffle=1)
    assert not hip.seeded_stream_stats()["last_launch_used_it"]
    planar(3, 200)
    hip.set_seed(777); ora.set_seed(777)
    run_in_place(hip, ora, mk(1, W, H, depth, sy, 0, 300))
    run_in_place(hip, ora, mk(4, W, H, depth, sy, 6, 400), seeds=[5, 0, 0xC0FFEE, 5], shuffle=3)
    planar(1, 500)


@pytest.mark.parametrize("seeded", [False, True])
def test_more_frames_than_one_launch_holds(hip, seeded):
    """70 frames = launches of 32 + 32 + 6"""
    ora, (depth, sx, sy) = program(hip, "fgs_afgs1_test1_8_420")
    frames = mk(70, 264, 40, depth, sy, 0, 700)
    seeds = [int(s) for s in np.random.default_rng(3).integers(0, 1 << 32, 70)] if seeded else None
    n0 = launches(hip)
    run_in_place(hip, ora, frames, seeds, shuffle=3)
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 3 and info["nframes"] == 6 and info["listed"] == 1, info


def test_two_calls_inside_an_overlap_region(hip):
    ora, (depth, sx, sy) = program(hip, "fgs_sei_ar_test1_10_420")
    a, b = mk(4, 520, 70, depth, sy, 6, 80), mk(3, 520, 70, depth, sy, 6, 90)
    seeds = [11, 22, 33]
    want = SP.expected(ora, a, None, 6) + SP.expected(ora, b, seeds, 6)
    da, db = scattered(a, 8), scattered(b, 9)
    st = stream_ptr()
    hip.overlap_begin(st)
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in da], None, None, 520, 70, a[0].stride, a[0].uv_stride, 6, st)
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in db], None, seeds, 520, 70, a[0].stride, a[0].uv_stride, 6, st)
    hip.overlap_end(st)
    for i, (d, w) in enumerate(zip(da + db, want)):
        assert_equal(d.download(), w, f"frame {i}")
    assert hip.seed_state() == ora.seed_state()


def test_two_frame_fronts(hip):
    """the host sweeps two frames at a time where a frame's planes hold 32 MiB (the row walk's rule, on the bytes of Y + UV): three P010
    frames of 8192 x 1366, the smallest even height at the widest row"""
    ora, (depth, sx, sy) = program(hip, "fgs_afgs1_test1_10_420")
    run_in_place(hip, ora, mk(3, 8192, 1366, depth, sy, 6, 50), shuffle=5)
    info = hip.last_launch_info()
    assert info["frames_per_front"] == 2 and info["nframes"] == 3, info
    run_in_place(hip, ora, mk(2, 8192, 1360, depth, sy, 6, 60))
    assert hip.last_launch_info()["frames_per_front"] == 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(hip):
    """every refusal of the contract with its code; then the registers and every byte are compared; then the same list is served"""
    from versatilefilmgrain_amd.hw import SpFrame, VfgsHipError
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    frames = mk(3, 520, 70, depth, sy, 6, 0)
    dev = scattered(frames)
    other = scattered(mk(3, 520, 70, depth, sy, 6, 7), 1)
    f0 = frames[0]
    geo = (f0.width, f0.height, f0.stride, f0.uv_stride)
    st = stream_ptr()
    seeds = [1, 2, 3]
    st0, n0 = hip.seed_state(), launches(hip)
    ptrs, optrs = [d.ptrs() for d in dev], [d.ptrs() for d in other]
    call = lambda s, d, sd, *a: hip.add_grain_sp_frame_list_dev(s, d, sd, *a)

    def refused(code, s, d=None, sd=seeds, g=geo, shift=6, match=None):
        with pytest.raises(VfgsHipError, match=match or f"error {code}:"):
            call(s, d, None if sd is None else sd[:len(s)], *g, shift, st)
        assert hip.lib.vfgs_hip_last_error() == code

    # everything the frame lists refuse, with their codes
    arr = hip.sp_frame_list(ptrs)
    assert hip.lib.vfgs_hip_add_grain_sp_frame_list_dev(None, arr, None, 3, *geo, 6, st) == 18
    assert hip.lib.vfgs_hip_add_grain_sp_frame_list_dev(arr, None, None, 3, *geo, 6, st) == 18
    refused(18, [ptrs[0], (ptrs[1][0], 0)], match="null plane")
    refused(18, [ptrs[0], (0, ptrs[1][1])], match="null plane")
    refused(7, [ptrs[0], (ptrs[1][0] + 8, ptrs[1][1])])
    refused(7, [ptrs[0], (ptrs[1][0], ptrs[1][1] + 8)])
    refused(7, ptrs, [optrs[0], (optrs[1][0], optrs[1][1] + 4), optrs[2]])
    refused(6, ptrs, g=(f0.width, f0.height, 512, f0.uv_stride))                 # a luma row of less than whole blocks
    refused(6, ptrs, g=(f0.width, f0.height, f0.stride, 512))                    # ... a UV row: as many containers as the luma row
    refused(8, ptrs, g=(f0.width, f0.height, f0.stride + 4, f0.uv_stride))       # pitch in bytes no multiple of 16
    refused(5, ptrs, g=(100, f0.height, f0.stride, f0.uv_stride))                # vfgs_hw.c:168
    refused(18, [ptrs[0], ptrs[1], ptrs[0]], match="listed twice")
    refused(18, ptrs, [optrs[0], (optrs[1][0], optrs[0][0]), optrs[2]], match="listed twice|overlap")      # a UV plane that is another frame's Y
    refused(18, ptrs, [optrs[0], (optrs[1][0], optrs[0][0] + 1024 * f0.Y.itemsize), optrs[2]], match="overlap")     # ... that overlaps it
    refused(18, ptrs, [optrs[0], (optrs[1][0], ptrs[2][1]), optrs[2]], match="shares bytes")                # a source of frame 2 is frame 1's destination
    refused(18, ptrs, [ptrs[1], ptrs[0], ptrs[2]], match="shares bytes")                              # frames 0 and 1 swapped
    # what this call alone refuses: error 40, the cause in the message
    refused(40, ptrs, shift=4, match="sample_shift 4 at depth 10")
    refused(40, ptrs, shift=10, match="sample_shift")
    refused(40, ptrs, g=(8208, f0.height, 8256, 8256), match="width 8208")
    hip.set_depth(8)
    try:
        refused(40, ptrs, shift=8, match="sample_shift 8 at depth 8")
        refused(40, ptrs, shift=6, match="sample_shift 6 at depth 8")
    finally:
        hip.set_depth(10)
    for subx, suby in ((1, 1), (1, 2)):
        hip.set_chroma_subsampling(subx, suby)
        try:
            refused(40, ptrs, match="csubx 1")
        finally:
            hip.set_chroma_subsampling(sx, sy)
    try:
        hip.set_chroma_mix(1, 32, 32, 0)
        refused(40, ptrs, match="chroma mix")
        refused(40, ptrs, sd=None, match="chroma mix")
    finally:
        hip.clear_chroma_mix()
    call([], None, None, *geo, 6, st)           # an empty list is no call at all ...
    call([], [], [], *geo, 6, st)               # ... with or without seeds, whatever else it is handed
    assert hip.lib.vfgs_hip_add_grain_sp_frame_list_dev(None, None, None, 0, 100, 70, 0, 0, 99, st) == 0
    assert hip.seed_state() == st0 and launches(hip) == n0
    for d, f in zip(dev + other, frames + [o.sp for o in other]):
        assert_equal(d.download(), f)
    # ... and the same list is served afterwards
    want = SP.expected(ora, frames, seeds, 6)
    call(ptrs, None, seeds, *geo, 6, st)
    for d, w in zip(dev, want):
        assert_equal(d.download(), w)
    assert hip.seed_state() == ora.seed_state()
