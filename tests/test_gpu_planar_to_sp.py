"""GPU (MI355X): vfgs_hip_add_grain_frame_list_to_sp_dev and _to_sp8_dev -- planar frames in, semi-planar surfaces out (yuv420p -> NV12,
yuv420p10le -> P010 or NV12, yuv422p10le -> P210 ...) -- against the oracle, through the C ABI, bit for bit: every byte of both destination
planes of every frame, padding included, every container of the sources (unchanged), and the four seed registers.

The expectation is tests/planar_to_sp_util.py's: the unchanged oracle on a copy of the planar source, interleaved, shifted up (or narrowed)
and pasted into the destination's previous bytes where the call writes; pinned by tests/test_planar_to_sp_util_cpu.py.  The models are the
hardware-layer programming the reference recorded for the configurations of tests/golden/fwcfg (tests/golden/traces, same names): fgs_sei
(general-form luma over one-pattern chroma at 4:2:0, general-form chroma at 4:2:2 -- generated programs add the two remaining forms),
fgs_sei_ff_test6 and fgs_afgs1_test1 (one pattern each); recorded at the hardware layer they carry no chroma mix, which these calls refuse.
12 bit: the 10-bit recording with its depth record replaced (tests/test_gpu_depth12.py).  Frames are separate allocations listed out of
address order; sources hold garbage over the full container range, padding included, destinations are pre-filled with garbage.

Shapes are the smallest that can go wrong: 264 x 40 (17 blocks: a UV row that ends in half a unit at 8 bit), 250 x 38 (a ragged width, 19
chroma rows at 4:2:0), 1032 x 90 (65 blocks: two positions a row at 16-bit containers, a last block row of 10 lines), 8192 x 16 (the widest
row, one block row)."""
import numpy as np
import pytest

import planar_to_sp_util as P2
import semiplanar_out8_util as SP8
import semiplanar_util as SP
import vfgs_testlib as T
from gpu_util import DevFrame, stream_ptr
from test_gpu_frame_list import garbage_frame
from test_gpu_semiplanar import DevSP, assert_equal, launches, program

pytestmark = pytest.mark.gpu

SHAPES = [(264, 40), (250, 38), (1032, 90), (8192, 16)]
SEI = ["fgs_sei_8_420", "fgs_sei_8_422", "fgs_sei_10_420", "fgs_sei_10_422", "fgs_sei_10_420@depth12", "fgs_sei_10_422@depth12"]
ONE = ["fgs_sei_ff_test6_8_420", "fgs_sei_ff_test6_8_422", "fgs_sei_ff_test6_10_420", "fgs_sei_ff_test6_10_420@depth12",
       "fgs_afgs1_test1_8_420", "fgs_afgs1_test1_10_420", "fgs_afgs1_test1_10_420@depth12"]
# (generated programs: one-pattern luma over general-form chroma, general-form luma over general-form chroma at 4:2:0)
FORMS = ["one_y_general_c_10_420", "general_runs_10_420", "general_runs_8_420"]
MODELS = SEI + ONE + FORMS


def deep(names):
    return [n for n in names if "_8_" not in n]


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


def mk(n, w, h, depth, sy, seed):
    return [garbage_frame(w, h, depth, 2, sy, seed + i) for i in range(n)]


def scattered(frames, seed=0):
    order = np.random.default_rng(seed).permutation(len(frames))
    dev = [None] * len(frames)
    for i in order:
        dev[i] = DevFrame(frames[i])
    return dev


def destinations(n, fill, seed=0):
    order = np.random.default_rng(1000 + seed).permutation(n)
    dst = [None] * n
    for i in order:
        dst[i] = DevSP(fill)
    return dst


def call(hip, src, dst, seeds, f0, fill, shift, out8, stream=None):
    st = stream_ptr() if stream is None else stream
    s, d = [x.ptrs() for x in src], [x.ptrs() for x in dst]
    if out8:
        hip.add_grain_frame_list_to_sp8_dev(s, d, seeds, f0.width, f0.height, f0.stride, f0.cstride, fill.stride, fill.uv_stride, st)
    else:
        hip.add_grain_frame_list_to_sp_dev(s, d, seeds, f0.width, f0.height, f0.stride, f0.cstride, fill.stride, fill.uv_stride, shift, st)


def check(src, dst, frames, want, what=""):
    for i, (s, d, f, w) in enumerate(zip(src, dst, frames, want)):
        assert_equal(d.download(), w, f"{what} destination {i}")       # what is written, and every other byte as it was
        assert s.download().equal_all(f), f"{what} source {i} changed"


def fill_for(f0, shift, out8, seed, pad, uv_pad):
    if out8:
        return SP8.dst_frame(f0.width, f0.height, f0.suby, seed, pad, uv_pad)
    return P2.dst_frame(f0.width, f0.height, f0.depth, f0.suby, shift, seed, pad, uv_pad)


def run(hip, ora, frames, shift=0, out8=False, seeds=None, pad=16, uv_pad=48, shuffle=0, stream=None):
    """into destinations whose pitches exceed the rows, differ between Y and UV and from the source's; everything is compared"""
    f0 = frames[0]
    fill = fill_for(f0, shift, out8, 4321 + shuffle, pad, uv_pad)
    want = P2.expected8(ora, frames, seeds, fill) if out8 else P2.expected(ora, frames, seeds, shift, fill)
    src, dst = scattered(frames, shuffle), destinations(len(frames), fill, shuffle)
    call(hip, src, dst, seeds, f0, fill, shift, out8, stream)
    check(src, dst, frames, want)
    assert hip.seed_state() == ora.seed_state()
    return src, dst, fill


def kernel_name(info, out8):
    return T.kernel_name("grain_p2sp8_kernel" if out8 else "grain_p2sp_kernel", info["depth"], info["csuby"], info["one_y"], info["one_c"])


def assert_launch(info, out8, depth, nframes):
    assert info["listed"] == 1 and info["in_place"] == 0 and info["out8"] == (1 if out8 else 0) and info["depth"] == depth, info
    assert info["nframes"] == nframes and info["kernel"] == kernel_name(info, out8) and info["lds_bytes_per_workgroup"] == 40960, info


# ---- formats --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,high", [(n, False) for n in MODELS] + [(n, True) for n in deep(MODELS)])
def test_every_format(hip, name, high):
    """3 frames of 264 x 40 per model, depth and chroma format; sample_shift 0 and 16 - depth (depth 8: 0 only)"""
    ora, (depth, sx, sy) = program(hip, name)
    assert sx == 2 and (depth > 8 or not high)
    shift = 16 - depth if high else 0
    n0 = launches(hip)
    run(hip, ora, mk(3, 264, 40, depth, sy, 10), shift, shuffle=int(high))
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 1
    assert_launch(info, False, depth, 3)


@pytest.mark.parametrize("name", deep(MODELS))
def test_every_format_narrowed(hip, name):
    ora, (depth, sx, sy) = program(hip, name)
    n0 = launches(hip)
    run(hip, ora, mk(3, 264, 40, depth, sy, 20), out8=True, pad=32, uv_pad=16, shuffle=2)
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 1
    assert_launch(info, True, depth, 3)


def test_all_four_forms(hip):
    seen = {}
    for name in ("fgs_sei_10_420", "fgs_afgs1_test1_10_420", "one_y_general_c_10_420", "general_runs_10_420"):
        ora, (depth, sx, sy) = program(hip, name)
        for out8 in (False, True):
            run(hip, ora, mk(2, 264, 40, depth, sy, 30), 0 if out8 else 6, out8)
            info = hip.last_launch_info()
            seen.setdefault((info["one_y"], info["one_c"]), set()).add(info["kernel"].split("<")[0])
    assert set(seen) == {(0, 0), (0, 1), (1, 0), (1, 1)} and all(v == {"grain_p2sp_kernel", "grain_p2sp8_kernel"} for v in seen.values()), seen


# ---- shapes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("name", SEI)
def test_shapes(hip, name, w, h):
    """two frames a shape; the shift alternates over the shapes, so every depth sees both"""
    ora, (depth, sx, sy) = program(hip, name)
    shift = 16 - depth if (depth > 8 and SHAPES.index((w, h)) % 2 == 0) else 0
    run(hip, ora, mk(2, w, h, depth, sy, w + h), shift, pad=0 if w == 8192 else 16, uv_pad=16 if w == 8192 else 48, shuffle=3)
    info = hip.last_launch_info()
    nblk = (w + 15) // 16
    units = (nblk * 8 * (2 if depth > 8 else 1) + 15) // 16          # 16-byte units of ONE component's source row
    assert info["positions_per_row"][1] == (units + 64) // 64 and info["kernel"].startswith("grain_p2sp_kernel<"), info


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("name", deep(SEI))
def test_shapes_narrowed(hip, name, w, h):
    ora, (depth, sx, sy) = program(hip, name)
    run(hip, ora, mk(2, w, h, depth, sy, w + h + 1), out8=True, pad=0 if w == 8192 else 48, uv_pad=16, shuffle=4)
    assert hip.last_launch_info()["kernel"].startswith("grain_p2sp8_kernel<")


@pytest.mark.parametrize("name", ["fgs_sei_ff_test6_8_422", "fgs_afgs1_test1_10_420"])
@pytest.mark.parametrize("w,h", SHAPES[1:])
def test_shapes_one_pattern(hip, name, w, h):
    ora, (depth, sx, sy) = program(hip, name)
    run(hip, ora, mk(2, w, h, depth, sy, w), 16 - depth if depth > 8 else 0, shuffle=5)
    if depth > 8:
        run(hip, ora, mk(2, w, h, depth, sy, w + 7), out8=True, shuffle=6)


# ---- call forms -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out8", [False, True], ids=["container", "narrowed"])
@pytest.mark.parametrize("seeded", [False, True])
def test_thirty_five_frames(hip, seeded, out8):
    """35 frames of 264 x 40 = launches of 32 + 3"""
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    seeds = [int(s) for s in np.random.default_rng(3).integers(0, 1 << 32, 35)] if seeded else None
    n0 = launches(hip)
    run(hip, ora, mk(35, 264, 40, depth, sy, 700), 0 if out8 else 6, out8, seeds, shuffle=7)
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 2
    assert_launch(info, out8, depth, 3)
    assert bool(hip.seeded_stream_stats()["last_launch_used_it"]) == seeded


@pytest.mark.parametrize("name,shift", [("fgs_sei_10_422", 6), ("fgs_sei_8_420", 0), ("fgs_sei_10_420@depth12", 4)])
def test_a_seed_per_picture(hip, name, shift):
    ora, (depth, sx, sy) = program(hip, name)
    seeds = [0, 0x80000000, 0xFFFFFFFF, 12345, 12345, 0x5eed1e55]
    run(hip, ora, mk(6, 1032, 90, depth, sy, 30), shift, seeds=seeds, shuffle=8)
    if depth > 8:
        run(hip, ora, mk(6, 1032, 90, depth, sy, 40), out8=True, seeds=seeds, shuffle=9)


@pytest.mark.parametrize("pad,uv_pad", [(0, 0), (16, 0), (0, 16), (112, 48), (1024, 2064)])
def test_destination_strides(hip, pad, uv_pad):
    """pitches equal to the rows, larger than them, different for Y and UV, larger than a position, none the source's (1088 / 576): the
    padding keeps its bytes (run compares every byte of both planes)"""
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    frames = mk(3, 1032, 33, depth, sy, 70)
    assert frames[0].stride == 1088 and frames[0].cstride == 576
    _, dst, fill = run(hip, ora, frames, 6, pad=pad, uv_pad=uv_pad)
    assert fill.stride == 1040 + pad and fill.uv_stride == 1040 + uv_pad
    run(hip, ora, frames, out8=True, pad=pad, uv_pad=uv_pad)
    ora8, (d8, _, sy8) = program(hip, "fgs_sei_8_422")
    run(hip, ora8, mk(3, 1032, 33, d8, sy8, 71), 0, pad=pad, uv_pad=uv_pad)


@pytest.mark.parametrize("name", ["fgs_sei_8_420", "fgs_sei_10_422", "fgs_sei_10_420@depth12"])
def test_garbage_sources_at_shift_0(hip, name):
    """containers over the full container range, above the depth's range included: they behave as in the planar calls (the oracle's)"""
    ora, (depth, sx, sy) = program(hip, name)
    frames = mk(3, 1032, 90, depth, sy, 90)
    assert any(int(f.Y.max()) >= (1 << depth) and int(f.U.max()) >= (1 << depth) for f in frames) or depth == 8
    run(hip, ora, frames, 0, shuffle=10)


def test_two_calls_inside_an_overlap_region(hip):
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    a, b = mk(4, 520, 70, depth, sy, 80), mk(3, 520, 70, depth, sy, 90)
    seeds = [11, 22, 33]
    fa, fb = fill_for(a[0], 6, False, 5, 16, 32), fill_for(a[0], 0, True, 6, 32, 16)
    want = P2.expected(ora, a, None, 6, fa) + P2.expected8(ora, b, seeds, fb)
    sa, sb, da, db = scattered(a, 8), scattered(b, 9), destinations(4, fa, 8), destinations(3, fb, 9)
    st = stream_ptr()
    hip.overlap_begin(st)
    call(hip, sa, da, None, a[0], fa, 6, False, st)
    call(hip, sb, db, seeds, a[0], fb, 0, True, st)
    hip.overlap_end(st)
    check(sa + sb, da + db, a + b, want)
    assert hip.seed_state() == ora.seed_state()


# ---- equivalence with the existing calls (no oracle) ------------------------------------------------------------------------------

def in_range(frames, depth):
    for f in frames:
        for p in f.planes():
            p &= (1 << depth) - 1
    return frames


@pytest.mark.parametrize("name,shift", [("fgs_sei_10_420", 6), ("fgs_sei_10_422", 0), ("fgs_sei_8_420", 0), ("fgs_sei_10_420@depth12", 4),
                                        ("fgs_afgs1_test1_10_420", 6)])
@pytest.mark.parametrize("seeded", [False, True])
def test_equals_the_semi_planar_call_on_the_twin(hip, name, shift, seeded):
    """_to_sp_dev == vfgs_hip_add_grain_sp_frame_list_dev out of place on the to_semiplanar twin of the same source, and _to_sp8_dev ==
    _sp_frame_list_copy8_dev on it; seed registers included.  Sources inside the depth's range: only those have a high-aligned twin."""
    from test_gpu_semiplanar import scattered as sp_scattered
    _, (depth, sx, sy) = program(hip, name)
    W, H = 1032, 90
    frames = in_range(mk(4, W, H, depth, sy, 300), depth)
    twins = [SP.to_semiplanar(f, shift) for f in frames]
    seeds = [9, 0, 0xC0FFEE, 9] if seeded else None
    st = stream_ptr()
    for out8 in ((False, True) if depth > 8 else (False,)):
        fill = fill_for(frames[0], shift, out8, 55, 16, 48)
        src, tsrc = scattered(frames, 1), sp_scattered(twins, 2)
        d_new, d_old = destinations(4, fill, 3), destinations(4, fill, 4)
        hip.set_seed(77)
        call(hip, src, d_new, seeds, frames[0], fill, shift, out8, st)
        regs_new = hip.seed_state()
        hip.set_seed(77)
        t0 = twins[0]
        if out8:
            hip.add_grain_sp_frame_list_copy8_dev([d.ptrs() for d in tsrc], [d.ptrs() for d in d_old], seeds, W, H, t0.stride, t0.uv_stride,
                                                  fill.stride, fill.uv_stride, shift, st)
        else:
            # (the existing call out of place writes at the SOURCE's pitches: destinations of the twin's geometry, compared over the written region)
            d_old = sp_scattered([SP.SPFrame(W, H, depth, sy, t0.stride, t0.uv_stride, shift, np.zeros_like(t0.Y), np.zeros_like(t0.UV)) for _ in twins], 5)
            hip.add_grain_sp_frame_list_dev([d.ptrs() for d in tsrc], [d.ptrs() for d in d_old], seeds, W, H, t0.stride, t0.uv_stride, shift, st)
        assert hip.seed_state() == regs_new
        rows, crows, cols = SP.written_region(t0)
        for a, b in zip(d_new, d_old):
            ga, gb = a.download(), b.download()
            assert np.array_equal(ga.Y[:rows, :cols], gb.Y[:rows, :cols]) and np.array_equal(ga.UV[:crows, :cols], gb.UV[:crows, :cols])
            if out8:
                assert ga.equal_all(gb)


def test_existing_calls_still_work_afterwards(hip):
    """KernelArgs::sp_kernel gained a value: the semi-planar call and the planar copy list, once each behind a _to_sp call in the same
    process, still match their own expectations"""
    from test_gpu_semiplanar import mk as sp_mk, scattered as sp_scattered
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    W, H = 520, 70
    run(hip, ora, mk(3, W, H, depth, sy, 100), 6)
    assert hip.last_launch_info()["kernel"].startswith("grain_p2sp_kernel<")
    # the existing semi-planar call, in place
    frames = sp_mk(3, W, H, depth, sy, 6, 200)
    want = SP.expected(ora, frames, None, 6)
    dev = sp_scattered(frames, 2)
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, None, W, H, frames[0].stride, frames[0].uv_stride, 6, stream_ptr())
    for d, w in zip(dev, want):
        assert_equal(d.download(), w)
    assert hip.seed_state() == ora.seed_state() and hip.last_launch_info()["kernel"].startswith("grain_sp_kernel<")
    # the planar copy list
    pf = mk(3, W, H, depth, sy, 300)
    pw = [f.copy() for f in pf]
    for w in pw:
        ora.add_grain_frame(w)
    psrc, pdst = scattered(pf, 3), scattered(pf, 4)
    hip.add_grain_frame_list_copy_dev([d.ptrs() for d in psrc], [d.ptrs() for d in pdst], W, H, pf[0].stride, pf[0].cstride, stream_ptr())
    cols = (W + 15) // 16 * 16
    for d, w in zip(pdst, pw):
        g = d.download()
        assert np.array_equal(g.Y[:H, :cols], w.Y[:H, :cols]) and np.array_equal(g.U[:H // sy, :cols // 2], w.U[:H // sy, :cols // 2])
        assert np.array_equal(g.V[:H // sy, :cols // 2], w.V[:H // sy, :cols // 2])
    assert hip.seed_state() == ora.seed_state() and hip.last_launch_info()["kernel"].startswith("grain_rw_kernel<")
    # ... and the new calls again
    run(hip, ora, mk(2, W, H, depth, sy, 400), 0, out8=True)
    assert hip.last_launch_info()["kernel"].startswith("grain_p2sp8_kernel<")


# ---- refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out8", [False, True], ids=["container", "narrowed"])
def test_refusals_change_nothing(hip, out8):
    """every refusal of the contract with its code and its cause; then the registers, `launches` and every byte of every plane are compared;
    then the same lists are served"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    frames = mk(3, 520, 70, depth, sy, 0)
    f0 = frames[0]
    good = 0 if out8 else 6
    fill = fill_for(f0, good, out8, 77, 16, 32)
    src, dst = scattered(frames), destinations(3, fill)
    geo = (f0.width, f0.height, f0.stride, f0.cstride, fill.stride, fill.uv_stride)
    st = stream_ptr()
    seeds = [1, 2, 3]
    st0, n0 = hip.seed_state(), launches(hip)
    sp, dp = [d.ptrs() for d in src], [d.ptrs() for d in dst]

    def raw(s, d, sd, g, shift):
        if out8:
            return hip.add_grain_frame_list_to_sp8_dev(s, d, sd, *g, st)
        return hip.add_grain_frame_list_to_sp_dev(s, d, sd, *g, shift, st)

    def refused(code, s=sp, d=dp, sd=seeds, g=geo, shift=good, match=None):
        with pytest.raises(VfgsHipError, match=match or f"error {code}:"):
            raw(s, d, None if sd is None else sd[:len(s)], g, shift)
        assert hip.lib.vfgs_hip_last_error() == code

    def with_geo(**kw):
        names = ("width", "height", "stride", "cstride", "dst_stride", "dst_uv_stride")
        return tuple(kw.get(n, v) for n, v in zip(names, geo))

    # depth 8: the narrowed form has the planar _copy8 calls' code; a shift there is a bad shift
    hip.set_depth(8)
    try:
        if out8:
            refused(16)
        else:
            refused(40, shift=6, match="sample_shift 6 at depth 8")
    finally:
        hip.set_depth(10)
    # what the semi-planar calls refuse with error 40, the cause named
    for subx, suby in ((1, 1), (1, 2)):
        hip.set_chroma_subsampling(subx, suby)
        try:
            refused(40, match="csubx 1")
        finally:
            hip.set_chroma_subsampling(sx, sy)
    if not out8:
        refused(40, shift=4, match="sample_shift 4 at depth 10")
        refused(40, shift=10, match="sample_shift")
    refused(40, g=(8208, f0.height, 8256, 4160, 8256, 8256), match="width 8208")
    try:
        hip.set_chroma_mix(1, 32, 32, 0)
        refused(40, match="chroma mix")
        refused(40, sd=None, match="chroma mix")
    finally:
        hip.clear_chroma_mix()
    # null list or plane
    arr_s, arr_d = hip.frame_list(sp), hip.sp_frame_list(dp)
    fn = hip.lib.vfgs_hip_add_grain_frame_list_to_sp8_dev if out8 else hip.lib.vfgs_hip_add_grain_frame_list_to_sp_dev
    tail = (st,) if out8 else (good, st)
    assert fn(None, arr_d, None, 3, *geo, *tail) == 18
    assert fn(arr_s, None, None, 3, *geo, *tail) == 18
    refused(18, s=[sp[0], (sp[1][0], 0, sp[1][2]), sp[2]], match="null plane")
    refused(18, s=[sp[0], (sp[1][0], sp[1][1], 0), sp[2]], match="null plane")
    refused(18, d=[dp[0], (0, dp[1][1]), dp[2]], match="null plane")
    refused(18, d=[dp[0], (dp[1][0], 0), dp[2]], match="null plane")
    # misaligned source, misaligned destination
    refused(7, s=[sp[0], (sp[1][0], sp[1][1] + 8, sp[1][2]), sp[2]])
    refused(7, d=[dp[0], (dp[1][0] + 8, dp[1][1]), dp[2]])
    refused(7, d=[dp[0], (dp[1][0], dp[1][1] + 4), dp[2]])
    # geometry of the source, with the planar list's codes
    refused(6, g=with_geo(stride=512))
    refused(6, g=with_geo(cstride=256))
    refused(8, g=with_geo(stride=f0.stride + 4))
    refused(8, g=with_geo(cstride=f0.cstride + 4))
    refused(5, g=with_geo(width=100))
    # the destination's pitches: a UV row is as many containers as the luma row
    refused(6, g=with_geo(dst_stride=512))
    refused(6, g=with_geo(dst_uv_stride=512))
    refused(6, g=with_geo(dst_uv_stride=272))
    refused(8, g=with_geo(dst_stride=fill.stride + 4))
    refused(8, g=with_geo(dst_uv_stride=fill.uv_stride + 4))
    # two destination planes that share bytes
    refused(18, d=[dp[0], dp[1], dp[0]], match="listed twice")
    refused(18, d=[dp[0], (dp[1][0], dp[0][0] + 1024), dp[2]], match="overlap")
    # a destination plane that shares bytes with ANY source plane: of the same frame, of another frame -- there is no in-place form
    refused(18, d=[dp[0], (sp[1][0], dp[1][1]), dp[2]], match="shares bytes")
    # (a source chroma plane is smaller than a UV plane: in an arena of its own, so that the UV plane on it reaches no other destination)
    import torch
    arena_t = torch.zeros(1 << 17, dtype=torch.uint8, device="cuda")
    arena = arena_t.data_ptr()
    refused(18, s=[sp[0], (sp[1][0], arena, sp[1][2]), sp[2]], d=[dp[0], (dp[1][0], arena), dp[2]], match="shares bytes")
    refused(18, s=[sp[0], (sp[1][0], sp[1][1], arena), sp[2]], d=[dp[0], (dp[1][0], arena), dp[2]], match="shares bytes")
    refused(18, s=[(sp[0][0], sp[0][1], arena + 4096), sp[1], sp[2]], d=[dp[0], (dp[1][0], arena), dp[2]], match="shares bytes")
    refused(18, d=[dp[0], (dp[1][0], sp[2][0] + 4096), dp[2]], match="shares bytes")
    refused(18, s=[sp[0], sp[1], (sp[2][0], sp[2][1], arena)], d=[(arena + 2048, dp[0][1]), dp[1], dp[2]], match="shares bytes")
    # (the sources' own Y and U planes as the destination: a UV plane on a U plane runs on into whatever lies behind it, which may be another
    # of these destinations -- either cause is a true one)
    refused(18, d=[(p[0], p[1]) for p in sp], match="shares bytes|overlap")
    del arena_t
    raw([], [], None, geo, good)           # an empty list is no call at all
    assert hip.seed_state() == st0 and launches(hip) == n0
    check(src, dst, frames, [fill] * 3, "after the refusals:")
    # ... and the same lists are served afterwards
    want = P2.expected8(ora, frames, seeds, fill) if out8 else P2.expected(ora, frames, seeds, good, fill)
    raw(sp, dp, seeds, geo, good)
    check(src, dst, frames, want)
    assert hip.seed_state() == ora.seed_state() and launches(hip) == n0 + 1
