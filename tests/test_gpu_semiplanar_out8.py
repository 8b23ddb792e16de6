"""GPU (MI355X): vfgs_hip_add_grain_sp_frame_list_copy8_dev -- semi-planar frames with the narrowed 8-bit destination (P010 / P210 / P012
in, NV12 / NV16 out) -- against the oracle, through the C ABI, bit for bit: every byte of both destination planes of every frame, padding
included, every container of the sources (unchanged), and the four seed registers.

The contract (include/vfgs_hip.h) is stated on D(p), the planar low-aligned picture of the semi-planar source p; the expectation is
tests/semiplanar_out8_util.py's (the unchanged oracle on D(p), narrowed as yuv_to_8bit does, interleaved; pinned against recorded reference
output by tests/test_semiplanar_out8_util_cpu.py).  Frames are separate allocations listed out of address order, sources hold garbage over
the full container range, destinations are pre-filled with garbage.  Shapes are the smallest that reach each mechanism: a UV source
position is 2 KiB -- 1024 luma samples of a row -- and the destination position 1 KiB.

Widths 16 and 48 are asserted as the planar calls' own refusal (error 5, vfgs_hw.c:168) with nothing changed, as in
tests/test_gpu_semiplanar.py."""
import numpy as np
import pytest

import semiplanar_out8_util as SP8
import semiplanar_util as SP
import vfgs_testlib as T
from gpu_util import stream_ptr
from test_gpu_semiplanar import DevSP, assert_equal, launches, mk, program, scattered

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


def one(v):
    return "true" if v else "false"


def destinations(frames, fill, seed=0):
    """one pre-filled destination per frame, allocated in an order of its own"""
    order = np.random.default_rng(1000 + seed).permutation(len(frames))
    dst = [None] * len(frames)
    for i in order:
        dst[i] = DevSP(fill)
    return dst


def call8(hip, src, dst, seeds, f0, fill, shift, stream=None):
    hip.add_grain_sp_frame_list_copy8_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], seeds, f0.width, f0.height, f0.stride, f0.uv_stride,
                                          fill.stride, fill.uv_stride, shift, stream_ptr() if stream is None else stream)


def check8(src, dst, frames, want, what=""):
    for i, (s, d, f, w) in enumerate(zip(src, dst, frames, want)):
        assert_equal(d.download(), w, f"{what} destination {i}")       # what is written, and every other byte as it was
        assert_equal(s.download(), f, f"{what} source {i}")


def run8(hip, ora, frames, seeds=None, pad=16, uv_pad=48, shuffle=0, stream=None):
    """out of place into destinations whose pitches exceed the rows and differ between Y and UV; everything is compared"""
    f0 = frames[0]
    fill = SP8.dst_frame(f0.width, f0.height, f0.suby, 4321 + shuffle, pad, uv_pad)
    want = SP8.expected8(ora, frames, seeds, f0.shift, fill)
    src, dst = scattered(frames, shuffle), destinations(frames, fill, shuffle)
    call8(hip, src, dst, seeds, f0, fill, f0.shift, stream)
    check8(src, dst, frames, want)
    assert hip.seed_state() == ora.seed_state()
    return src, dst


# ---- every form -----------------------------------------------------------------------------------------------------------------

MODELS = ["fgs_sei_10_420", "fgs_afgs1_test1_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_422", "one_y_general_c_10_420", "fgs_sei_10_420@depth12",
          "one_same_slot_12_422"]
# (those seven reach three of the four forms of the table image -- every one of them has one-pattern chroma or one-pattern luma; the generated
# program adds general-form luma over general-form chroma at 10 bit, so that every grain_sp8_kernel form is launched)
FORM_MODELS = MODELS + ["general_runs_10_420"]


@pytest.mark.parametrize("high", [False, True], ids=["low_aligned", "high_aligned"])
@pytest.mark.parametrize("name", FORM_MODELS)
def test_every_form(hip, name, high):
    """7 frames of 1032 x 90 (65 blocks, a ragged last block row), one launch; with the shift the sources' low bits are random"""
    ora, (depth, sx, sy) = program(hip, name)
    assert sx == 2 and depth in (10, 12)
    shift = 16 - depth if high else 0
    frames = mk(7, 1032, 90, depth, sy, shift, 10)
    assert not high or any((f.Y & ((1 << shift) - 1)).any() and (f.UV & ((1 << shift) - 1)).any() for f in frames)
    n0 = launches(hip)
    run8(hip, ora, frames, shuffle=int(high))
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 1 and info["nframes"] == 7 and info["listed"] == 1 and info["in_place"] == 0 and info["depth"] == depth, info
    assert info["out8"] == 1, info
    assert info["kernel"] == f"grain_sp8_kernel<{depth},{sy},{one(info['one_y'])},{one(info['one_c'])}>", info
    assert info["lds_bytes_per_workgroup"] == 40960, info


def test_all_four_forms(hip):
    """general / one-pattern luma over general / one-pattern chroma: the models above reach each form's kernel (two frames of 136 x 33 each)"""
    seen = {}
    for name in FORM_MODELS:
        ora, (depth, sx, sy) = program(hip, name)
        run8(hip, ora, mk(2, 136, 33, depth, sy, 16 - depth, 20))
        info = hip.last_launch_info()
        seen.setdefault((info["one_y"], info["one_c"]), []).append(info["kernel"])
    assert set(seen) == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen
    assert all(k.startswith("grain_sp8_kernel<") and k.endswith(f"{one(y)},{one(c)}>") for (y, c), ks in seen.items() for k in ks), seen


# ---- row geometry ---------------------------------------------------------------------------------------------------------------

WIDTHS = [136, 1016, 1024, 1032, 2056, 4104, 8192]
HEIGHTS = [16, 17, 33, 70]
GROUPS = {"420": "fgs_sei_10_420", "422": "fgs_sei_10_422"}
GEOMETRY = [(g, w, HEIGHTS[(i + k) % 4]) for k, g in enumerate(GROUPS) for i, w in enumerate(WIDTHS)]


@pytest.mark.parametrize("group,width,height", GEOMETRY)
def test_row_geometry(hip, group, width, height):
    """one, two, four and eight UV positions a row and their neighbours, an odd block count; P010 / P210 and low-aligned samples in turn"""
    ora, (depth, sx, sy) = program(hip, GROUPS[group])
    shift = 6 if WIDTHS.index(width) % 2 == 0 else 0
    run8(hip, ora, mk(3, width, height, depth, sy, shift, width + height), pad=32 if width < 8192 else 0, uv_pad=16, shuffle=2)
    info = hip.last_launch_info()
    nblk = (width + 15) // 16            # a lane's 32-byte source unit is one block of the row; the position behind the last unit is walked too
    assert info["positions_per_row"][1] == (nblk + 64) // 64 and info["out8"] == 1, info


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("width", [16, 48])
def test_narrow_pictures_are_refused(hip, group, width):
    from versatilefilmgrain_amd.hw import VfgsHipError
    ora, (depth, sx, sy) = program(hip, GROUPS[group])
    frames = mk(3, width, 33, depth, sy, 6, width)
    fill = SP8.dst_frame(width, 33, sy, 9, 16, 32)
    src, dst = scattered(frames), destinations(frames, fill)
    st0, n0 = hip.seed_state(), launches(hip)
    with pytest.raises(VfgsHipError, match="error 5"):
        call8(hip, src, dst, None, frames[0], fill, 6)
    assert hip.seed_state() == st0 and launches(hip) == n0
    check8(src, dst, frames, [fill] * 3)


def test_geometry_covers_every_width_and_height_in_every_group():
    for g in GROUPS:
        assert {w for gg, w, _ in GEOMETRY if gg == g} == set(WIDTHS) and {h for gg, _, h in GEOMETRY if gg == g} == set(HEIGHTS)


# ---- destination pitches --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad,uv_pad", [(0, 0), (16, 0), (0, 16), (112, 48), (1024, 2064)])
def test_destination_pitches(hip, pad, uv_pad):
    """pitches equal to the rows, larger than them, different for Y and UV, larger than a position: the padding keeps its bytes (run8
    compares every byte of both planes with the fill outside the written region)"""
    ora, (depth, sx, sy) = program(hip, "fgs_sei_ar_test1_10_420")
    src, dst = run8(hip, ora, mk(3, 1032, 33, depth, sy, 6, 70), pad=pad, uv_pad=uv_pad)
    assert dst[0].sp.stride == 1040 + pad and dst[0].sp.uv_stride == 1040 + uv_pad


# ---- seeds ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shift", [("fgs_sei_10_420", 6), ("fgs_sei_10_422", 0), ("fgs_sei_10_420@depth12", 4)])
def test_a_seed_per_picture(hip, name, shift):
    ora, (depth, sx, sy) = program(hip, name)
    seeds = [0, 0x80000000, 0xFFFFFFFF, 12345, 12345, 0x5eed1e55]
    run8(hip, ora, mk(6, 1032, 90, depth, sy, shift, 30), seeds, shuffle=6)
    info = hip.last_launch_info()
    assert info["out8"] == 1 and info["kernel"].startswith("grain_sp8_kernel<"), info
    assert hip.seeded_stream_stats()["last_launch_used_it"]


@pytest.mark.parametrize("seeded", [False, True])
def test_more_frames_than_one_launch_holds(hip, seeded):
    """33 frames of 136 x 16 = launches of 32 + 1"""
    ora, (depth, sx, sy) = program(hip, "fgs_afgs1_test1_10_420")
    seeds = [int(s) for s in np.random.default_rng(3).integers(0, 1 << 32, 33)] if seeded else None
    n0 = launches(hip)
    run8(hip, ora, mk(33, 136, 16, depth, sy, 6, 700), seeds, shuffle=3)
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 2 and info["nframes"] == 1 and info["listed"] == 1 and info["out8"] == 1, info


# ---- mixing with other calls ----------------------------------------------------------------------------------------------------

def test_two_calls_inside_an_overlap_region(hip):
    ora, (depth, sx, sy) = program(hip, "fgs_sei_ar_test1_10_420")
    a, b = mk(4, 520, 70, depth, sy, 6, 80), mk(3, 520, 70, depth, sy, 6, 90)
    seeds = [11, 22, 33]
    fill = SP8.dst_frame(520, 70, sy, 5, 16, 32)
    want = SP8.expected8(ora, a, None, 6, fill) + SP8.expected8(ora, b, seeds, 6, fill)
    sa, sb, da, db = scattered(a, 8), scattered(b, 9), destinations(a, fill, 8), destinations(b, fill, 9)
    st = stream_ptr()
    hip.overlap_begin(st)
    call8(hip, sa, da, None, a[0], fill, 6, st)
    call8(hip, sb, db, seeds, a[0], fill, 6, st)
    hip.overlap_end(st)
    check8(sa + sb, da + db, a + b, want)
    assert hip.seed_state() == ora.seed_state()


def test_two_frame_fronts(hip):
    """the shape of tests/test_gpu_semiplanar.py::test_two_frame_fronts: three P010 frames of 8192 x 1366 are swept two at a time (the rule
    is on the bytes of the SOURCE's planes), two of 8192 x 1360 are not"""
    ora, (depth, sx, sy) = program(hip, "fgs_afgs1_test1_10_420")
    run8(hip, ora, mk(3, 8192, 1366, depth, sy, 6, 50), pad=0, uv_pad=16, shuffle=5)
    info = hip.last_launch_info()
    assert info["frames_per_front"] == 2 and info["nframes"] == 3 and info["out8"] == 1, info
    run8(hip, ora, mk(2, 8192, 1360, depth, sy, 6, 60), pad=0, uv_pad=0)
    assert hip.last_launch_info()["frames_per_front"] == 1


def test_one_seed_sequence_with_the_existing_calls(hip):
    """the new call, the existing semi-planar call in place, a planar _copy8 list, the new call with seeds, the new call again: the registers
    are the oracle's after each step and every call's bytes are its own contract's"""
    import torch
    from gpu_util import DevFrame
    from test_gpu_frame_list import garbage_frame
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    W, H = 520, 70
    run8(hip, ora, mk(5, W, H, depth, sy, 6, 100), shuffle=1)
    assert not hip.seeded_stream_stats()["last_launch_used_it"]
    # the existing semi-planar call, in place
    frames = mk(3, W, H, depth, sy, 6, 200)
    want = SP.expected(ora, frames, None, 6)
    dev = scattered(frames, 2)
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, None, W, H, frames[0].stride, frames[0].uv_stride, 6, stream_ptr())
    for d, w in zip(dev, want):
        assert_equal(d.download(), w)
    assert hip.seed_state() == ora.seed_state() and hip.last_launch_info()["kernel"].startswith("grain_sp_kernel<")
    # a planar _copy8 list
    pf = [garbage_frame(W, H, depth, sx, sy, 300 + i) for i in range(3)]
    pw = [f.copy() for f in pf]
    for w in pw:
        ora.add_grain_frame(w)
    psrc = [DevFrame(f) for f in pf]
    f8 = T.Frame(W, H, 8, sx, sy)
    pdst = [tuple(torch.full(p.shape, 0x5a, dtype=torch.uint8, device="cuda") for p in f8.planes()) for _ in pf]
    hip.add_grain_frame_list_copy8_dev([d.ptrs() for d in psrc], [tuple(t.data_ptr() for t in d) for d in pdst], W, H, pf[0].stride, pf[0].cstride,
                                       f8.stride, f8.cstride, stream_ptr())
    torch.cuda.synchronize()
    cols = (W + 15) // 16 * 16
    for w, d in zip(pw, pdst):
        for got, w16, rows, c in ((d[0], w.Y, H, cols), (d[1], w.U, H // sy, cols // sx), (d[2], w.V, H // sy, cols // sx)):
            assert np.array_equal(got.cpu().numpy()[:rows, :c], SP8.narrow(w16[:rows, :c], depth))
    assert hip.seed_state() == ora.seed_state() and hip.last_launch_info()["kernel"].startswith("grain_rw_kernel<")
    # the new call with seeds, and again without
    run8(hip, ora, mk(4, W, H, depth, sy, 0, 400), seeds=[5, 0, 0xC0FFEE, 5], shuffle=3)
    run8(hip, ora, mk(2, W, H, depth, sy, 6, 500))
    assert hip.last_launch_info()["kernel"].startswith("grain_sp8_kernel<")


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(hip):
    """every refusal of the contract with its code; then the registers and every byte of every plane are compared; then the same lists are served"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    frames = mk(3, 520, 70, depth, sy, 6, 0)
    fill = SP8.dst_frame(520, 70, sy, 77, 16, 32)
    src, dst = scattered(frames), destinations(frames, fill)
    f0 = frames[0]
    geo = (f0.width, f0.height, f0.stride, f0.uv_stride, fill.stride, fill.uv_stride)
    st = stream_ptr()
    seeds = [1, 2, 3]
    st0, n0 = hip.seed_state(), launches(hip)
    sp, dp = [d.ptrs() for d in src], [d.ptrs() for d in dst]

    def refused(code, s=sp, d=dp, sd=seeds, g=geo, shift=6, match=None):
        with pytest.raises(VfgsHipError, match=match or f"error {code}:"):
            hip.add_grain_sp_frame_list_copy8_dev(s, d, None if sd is None else sd[:len(s)], *g, shift, st)
        assert hip.lib.vfgs_hip_last_error() == code

    def with_geo(**kw):
        names = ("width", "height", "stride", "uv_stride", "dst_stride", "dst_uv_stride")
        return tuple(kw.get(n, v) for n, v in zip(names, geo))

    # depth 8: the planar _copy8 calls' code
    hip.set_depth(8)
    try:
        refused(16, shift=0)
        refused(40, shift=6, match="sample_shift 6 at depth 8")
    finally:
        hip.set_depth(10)
    # what the semi-planar call refuses with error 40
    for subx, suby in ((1, 1), (1, 2)):
        hip.set_chroma_subsampling(subx, suby)
        try:
            refused(40, match="csubx 1")
        finally:
            hip.set_chroma_subsampling(sx, sy)
    refused(40, shift=4, match="sample_shift 4 at depth 10")
    refused(40, shift=10, match="sample_shift")
    refused(40, g=(8208, f0.height, 8256, 8256, 8256, 8256), match="width 8208")
    try:
        hip.set_chroma_mix(1, 32, 32, 0)
        refused(40, match="chroma mix")
        refused(40, sd=None, match="chroma mix")
    finally:
        hip.clear_chroma_mix()
    # null list or plane
    arr_s, arr_d = hip.sp_frame_list(sp), hip.sp_frame_list(dp)
    assert hip.lib.vfgs_hip_add_grain_sp_frame_list_copy8_dev(None, arr_d, None, 3, *geo, 6, st) == 18
    assert hip.lib.vfgs_hip_add_grain_sp_frame_list_copy8_dev(arr_s, None, None, 3, *geo, 6, st) == 18
    refused(18, s=[sp[0], (sp[1][0], 0), sp[2]], match="null plane")
    refused(18, d=[dp[0], (0, dp[1][1]), dp[2]], match="null plane")
    # misaligned source, misaligned destination
    refused(7, s=[sp[0], (sp[1][0], sp[1][1] + 8), sp[2]])
    refused(7, d=[dp[0], (dp[1][0] + 8, dp[1][1]), dp[2]])
    refused(7, d=[dp[0], (dp[1][0], dp[1][1] + 4), dp[2]])
    # geometry of the source, with the semi-planar call's codes
    refused(6, g=with_geo(stride=512))
    refused(6, g=with_geo(uv_stride=512))
    refused(8, g=with_geo(stride=f0.stride + 4))
    refused(5, g=with_geo(width=100))
    # the destination's pitches, with the planar _copy8 list's codes: a UV row of bytes is as long as the luma row
    refused(6, g=with_geo(dst_stride=512))
    refused(6, g=with_geo(dst_uv_stride=512))
    refused(6, g=with_geo(dst_uv_stride=272))
    refused(8, g=with_geo(dst_stride=fill.stride + 8))
    refused(8, g=with_geo(dst_uv_stride=fill.uv_stride + 8))
    # two destinations that share bytes
    refused(18, d=[dp[0], dp[1], dp[0]], match="listed twice")
    refused(18, d=[dp[0], (dp[1][0], dp[0][0] + 1024), dp[2]], match="overlap")
    # a destination that shares bytes with a source plane: of the same frame, of another frame; the source list as the destination
    refused(18, d=[dp[0], (sp[1][0], dp[1][1]), dp[2]], match="shares bytes")
    refused(18, d=[dp[0], (dp[1][0], sp[1][1]), dp[2]], match="shares bytes")
    refused(18, d=[dp[0], (dp[1][0], sp[2][0] + 4096), dp[2]], match="shares bytes")
    refused(18, d=[(sp[2][1] + 2048, dp[0][1]), dp[1], dp[2]], match="shares bytes")
    refused(18, d=sp, match="shares bytes")
    hip.add_grain_sp_frame_list_copy8_dev([], [], None, *geo, 6, st)           # an empty list is no call at all
    assert hip.seed_state() == st0 and launches(hip) == n0
    check8(src, dst, frames, [fill] * 3, "after the refusals:")
    # ... and the same lists are served afterwards
    want = SP8.expected8(ora, frames, seeds, 6, fill)
    hip.add_grain_sp_frame_list_copy8_dev(sp, dp, seeds, *geo, 6, st)
    check8(src, dst, frames, want)
    assert hip.seed_state() == ora.seed_state()
