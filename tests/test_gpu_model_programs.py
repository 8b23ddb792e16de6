"""GPU (MI355X): the generated programs of tests/model_programs.py through every form of the table image, byte for byte against the
oracle (which tests/test_model_programs_cpu.py pins to the reference hardware layer for exactly these programs).

vfgs_host.cpp turns the programmed model into a kernel form in four places (uniform_slot, image_form, build_tables, upload_tables);
the firmware traces the rest of the suite is programmed from never reach a general luma AND chroma LUT, slot 8, Cb and Cr on
different slots, a -128, a scale LUT at the packed 16-bit limit of ONE component, or scale_shift 7.  Every test here compares whole
buffers (row padding included) and the four seed registers after every call, and asserts the form and depth the launch reports
(last_launch_info) against MP.expected_form -- a class that silently ran the general form would prove nothing.
The surface kernels (semi-planar frames) and the model-list kernel: tests/test_gpu_model_programs_surfaces.py, tests/test_gpu_model_list_programs.py.

Shapes: 328 x 56 (21 blocks: the shifted 8-bit kernels at 4:2:0 / 4:2:2, the last block half in the padding, 3.5 block rows),
352 x 56 (22 blocks: the aligned 8-bit kernels), 8208 x 40 (rows walked in two parts).
"""
import numpy as np
import pytest

import chroma_mix_util as X
import model_programs as MP
import vfgs_testlib as T

pytestmark = pytest.mark.gpu

W, H = 328, 56
E_UNSUPPORTED = 38


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.clear_chroma_mix()
    h.lib.vfgs_hip_reset_state()


def oracle_for(rec):
    ora = T.OracleHW()
    T.replay(ora, rec)
    return ora


def program(hip, rec):
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, rec)


def check_form(hip, rec, wide=False):
    info = hip.last_launch_info()
    st = T.StateModel()
    T.replay(st, rec)
    assert (bool(info["one_y"]), bool(info["one_c"])) == MP.expected_form(rec, wide), (info["kernel"], MP.expected_form(rec, wide))
    assert info["depth"] == 8 + st.bs and (info["csubx"], info["csuby"]) == (st.subx, st.suby), info
    assert (info["parts_per_row"] > 1) == wide, info
    return info


def assert_equal(got, want, what=""):
    for pl, a, b in zip("YUV", got.planes(), want.planes()):
        n = int(np.count_nonzero(a != b))
        assert n == 0, f"{what}: plane {pl}: {n} samples differ from the oracle"


def frames_in_place(hip, ora, rec, frames, wide=False):
    """consecutive frames through vfgs_hip_add_grain_frame_dev, each checked, the form and the registers after every call"""
    from gpu_util import DevFrame, stream_ptr
    for i, f in enumerate(frames):
        d = DevFrame(f)
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        check_form(hip, rec, wide)
        want = f.copy()
        ora.add_grain_frame(want)
        assert_equal(d.download(), want, f"frame {i}")
        assert hip.seed_state() == ora.seed_state()


# ---- every program ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MP.names())
def test_every_program_frame_dev(hip, name):
    """two consecutive frames in place, row pitch padded by 64 samples, both content variants"""
    _, depth, fmt, _ = MP.parse(name)
    rec = MP.program(name)
    for w in (W, 352) if depth == 8 and fmt in ("420", "422") else (W,):
        for variant in MP.VARIANTS:
            frames = MP.content(name, w, H, 2, variant, pad=64)
            assert frames[0].stride >= w + 64
            program(hip, rec)
            frames_in_place(hip, oracle_for(rec), rec, frames)


@pytest.mark.parametrize("depth", MP.DEPTHS)
def test_all_four_forms_at_every_depth(hip, depth):
    """(one_y, one_c) as the launch reports it: every combination, at every depth"""
    seen = {}
    for name in MP.names(depth=depth):
        form = MP.expected_form(MP.program(name))
        if form not in seen:
            rec = MP.program(name)
            program(hip, rec)
            frames_in_place(hip, oracle_for(rec), rec, MP.content(name, W, H, 1, "in_range"))
            info = hip.last_launch_info()
            seen[form] = (bool(info["one_y"]), bool(info["one_c"]))
    assert sorted(seen) == sorted(seen.values()) == [(False, False), (False, True), (True, False), (True, True)]


# ---- every class through the other data paths ------------------------------------------------------------------------------------

def narrowed(f):
    """the fused 8-bit output of a 10- / 12-bit frame: (v + 2) >> 2, (v + 8) >> 4"""
    bs = f.depth - 8
    g = T.Frame(f.width, f.height, 8, f.subx, f.suby, f.stride, f.cstride)
    for a, b in zip(g.planes(), f.planes()):
        a[...] = ((b.astype(np.int32) + (1 << (bs - 1))) >> bs).astype(np.uint8)
    return g


def stack(frames):
    import torch
    return [torch.from_numpy(np.stack(ps).view(np.uint8).copy()).cuda() for ps in zip(*[f.planes() for f in frames])]


def unstack(ts, like):
    import torch
    torch.cuda.synchronize()
    out = [f.copy() for f in like]
    for k, t in enumerate(ts):
        a = t.cpu().numpy()
        for i, f in enumerate(out):
            f.planes()[k][...] = a[i].view(f.dtype).reshape(f.planes()[k].shape)
    return out


def run_copy_dev(hip, frames):
    """out of place: the source stays untouched, the destination keeps its fill behind the last whole block"""
    from gpu_util import stream_ptr
    f0 = frames[0]
    fill = [f.copy() for f in frames]
    for f in fill:
        for p in f.planes():
            p[...] = 0xA5 if f.depth == 8 else 0xA5A5
    src, dst = stack(frames), stack(fill)
    hip.add_grain_copy_dev(*[t.data_ptr() for t in src], *[t.data_ptr() for t in dst], f0.width, f0.height, 0, f0.height, f0.stride, f0.cstride,
                           len(frames), src[0][0].numel(), src[1][0].numel(), stream_ptr())
    for a, b in zip(unstack(src, frames), frames):
        assert a.equal_all(b), "the source of an out-of-place call changed"
    return unstack(dst, fill), fill


def run_copy8_dev(hip, frames):
    from gpu_util import stream_ptr
    f0 = frames[0]
    fill = [narrowed(f) for f in frames]
    for f in fill:
        for p in f.planes():
            p[...] = 0xA5
    src, dst = stack(frames), stack(fill)
    hip.add_grain_copy8_dev(*[t.data_ptr() for t in src], *[t.data_ptr() for t in dst], f0.width, f0.height, 0, f0.height, f0.stride, f0.cstride,
                            f0.stride, f0.cstride, len(frames), src[0][0].numel(), src[1][0].numel(), dst[0][0].numel(), dst[1][0].numel(), stream_ptr())
    for a, b in zip(unstack(src, frames), frames):
        assert a.equal_all(b), "the source of an out-of-place call changed"
    return unstack(dst, fill), fill


def written(want, fill):
    """what an out-of-place call leaves in a destination that held `fill`: the picture's rows and whole 16-sample blocks from
    `want`, everything else untouched"""
    out = fill.copy()
    cols = (want.width + 15) // 16 * 16
    rows = want.height
    out.Y[:rows, :cols] = want.Y[:rows, :cols]
    crows = (rows + want.suby - 1) // want.suby
    for o, w in ((out.U, want.U), (out.V, want.V)):
        o[:crows, :cols // want.subx] = w[:crows, :cols // want.subx]
    return out


def run_frames_dev(hip, frames):
    from gpu_util import stream_ptr
    f0 = frames[0]
    Y, U, V = stack(frames)
    hip.add_grain_frames_dev(Y.data_ptr(), U.data_ptr(), V.data_ptr(), f0.width, f0.height, f0.stride, f0.cstride, len(frames),
                             Y[0].numel(), U[0].numel(), stream_ptr())
    return unstack((Y, U, V), frames)


SEEDS = [0, 0xFFFFFFFF, 12345]


def run_list_seeded(hip, frames):
    from gpu_util import DevFrame, stream_ptr
    f0 = frames[0]
    devs = [DevFrame(f) for f in frames]
    hip.add_grain_frame_list_seeded_dev([d.ptrs() for d in devs], SEEDS, f0.width, f0.height, f0.stride, f0.cstride, stream_ptr())
    return [d.download() for d in devs]


def run_host_stripes(hip, frames):
    """vfgs_add_grain_stripe on host memory, uneven stripes: one inside a block row, one of a single (odd) line"""
    out = [f.copy() for f in frames]
    for f in out:
        y = 0
        for h in (6, 26, 1, 15, f.height - 48):
            hip.add_grain_stripe(f.Y[y].ctypes.data, f.U[y // f.suby].ctypes.data, f.V[y // f.suby].ctypes.data, y, f.width, h, f.stride, f.cstride)
            y += h
        assert y == f.height
    return out


def run_line(hip, frames):
    out = [f.copy() for f in frames]
    for f in out:
        for y in range(f.height):
            hip.add_grain_line(f.Y[y].ctypes.data, f.U[y // f.suby].ctypes.data, f.V[y // f.suby].ctypes.data, y, f.width)
    return out


PATHS = ("copy_dev", "copy8_dev", "frames_dev", "frame_list_seeded_dev", "add_grain_stripe", "add_grain_line")


def path_cases():
    """every class through every path at one depth / format each; the rotation reaches every depth and every format on every path"""
    for p, path in enumerate(PATHS):
        for i, cls in enumerate(MP.classes()):
            depths = (10, 12) if path == "copy8_dev" else MP.DEPTHS
            if cls == "pk16_split":
                if path == "copy8_dev":
                    continue            # (8 bit only: there is no narrower output)
                depths = (8,)
            fmts = [f for f in MP.FORMATS if MP.names(cls, None, f)]
            pick = MP.names(cls, depths[(i + p) % len(depths)], fmts[(i + 2 * p) % len(fmts)])
            yield pytest.param(path, pick[(i + p) % len(pick)], id=f"{path}-{pick[(i + p) % len(pick)]}")


def test_the_path_rotation_reaches_every_depth_and_format():
    for path in PATHS:
        got = [MP.parse(c.values[1]) for c in path_cases() if c.values[0] == path]
        assert {g[2] for g in got} == set(MP.FORMATS)
        assert {g[1] for g in got} == ({10, 12} if path == "copy8_dev" else set(MP.DEPTHS))
        assert {g[0] for g in got} >= set(MP.classes()) - {"pk16_split"}


@pytest.mark.parametrize("path, name", list(path_cases()))
def test_every_class_through_the_other_data_paths(hip, path, name):
    rec = MP.program(name)
    n = 1 if path == "add_grain_line" else 3
    frames = MP.content(name, W, H, n, "garbage" if path in ("copy8_dev", "frames_dev") else "in_range", pad=64 if path != "add_grain_line" else 0)
    ora = oracle_for(rec)
    want = [f.copy() for f in frames]
    for k, w in enumerate(want):
        if path == "frame_list_seeded_dev":
            ora.set_seed(SEEDS[k])
        ora.add_grain_frame(w)
    program(hip, rec)
    if path == "copy_dev":
        got, fill = run_copy_dev(hip, frames)
        want = [written(w, f) for w, f in zip(want, fill)]
    elif path == "copy8_dev":
        got, fill = run_copy8_dev(hip, frames)
        want = [written(narrowed(w), f) for w, f in zip(want, fill)]
    else:
        got = {"frames_dev": run_frames_dev, "frame_list_seeded_dev": run_list_seeded, "add_grain_stripe": run_host_stripes,
               "add_grain_line": run_line}[path](hip, frames)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_equal(g, w, f"{path}: frame {i}")
    assert hip.seed_state() == ora.seed_state()
    info = check_form(hip, rec)
    assert info["out8"] == (path == "copy8_dev")


# ---- rows walked in parts --------------------------------------------------------------------------------------------------------

WIDE = ["general_runs_8_420", "general_runs_10_444", "one_same_slot_10_420", "one_same_slot_8_444", "one_same_slot_8_422", "one_same_slot_10_422",
        "one_cb_cr_differ_12_420", "one_cb_cr_differ_8_444", "slot8_chroma_8_420", "slot8_chroma_12_444", "one_y_general_c_10_420",
        "one_y_general_c_10_444"]


@pytest.mark.parametrize("name", WIDE)
def test_wide_rows_then_a_narrow_frame(hip, name):
    """8208 x 40: parts_per_row == 2.  The form is expected_form(wide=True) -- general at 4:2:2 whatever the model -- and the narrow
    frame that follows, with nothing reprogrammed, gets the narrow form back (upload_tables: img_wide), then wide and narrow once more."""
    rec = MP.program(name)
    fmt = MP.parse(name)[2]
    if fmt == "422":
        assert MP.expected_form(rec, wide=True) == (False, False) and MP.expected_form(rec) == (True, True)
    program(hip, rec)
    ora = oracle_for(rec)
    for k, w in enumerate((8208, W, 8208, W)):
        frames = MP.content(name, w, 40 if w > W else H, 1, MP.VARIANTS[k % 2])
        frames_in_place(hip, ora, rec, frames, wide=w > 8192)


# ---- persistent luma workgroups --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["general_runs_10_420", "general_runs_12_444", "slot8_some_12_420", "slot8_some_10_422"])
def test_persistent_luma_workgroups(hip, name):
    """one launch of 1100 frames of 136 x 33 (the smallest case of test_gpu_rowwalk.test_persistent_luma_workgroups)"""
    rec = MP.program(name)
    frames = MP.content(name, 136, 33, 1100, "garbage")
    ora = oracle_for(rec)
    want = [f.copy() for f in frames]
    for w in want:
        ora.add_grain_frame(w)
    program(hip, rec)
    got = run_frames_dev(hip, frames)
    info = check_form(hip, rec)
    assert info["persistent_luma_workgroups"] > 0 and info["nframes"] == len(frames), info
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if not g.equal_all(w)]
    assert not bad, f"{len(bad)} frames differ from the oracle, first {bad[:5]}"
    assert hip.seed_state() == ora.seed_state()


# ---- reprogramming with launches in flight ---------------------------------------------------------------------------------------

def uniform_lut(slot, low=0):
    return bytes([(slot << 4) | low]) * 256


@pytest.mark.parametrize("depth", [8, 10])
def test_reprogramming_with_launches_in_flight(hip, depth):
    """One stream, no synchronisation until the end, exactly one setter call between consecutive frames, each chosen to flip or
    to keep the form: the table ring and tables_dirty.  Every frame's form is checked right after its call, every frame's bytes
    after the single sync.  The last steps run at both depths; the 16-bit limit acts at 8 bit only (the form check says so)."""
    import torch
    from gpu_util import DevFrame, stream_ptr
    def shift_of(n):
        st = T.StateModel()
        T.replay(st, MP.program(n))
        return st.shift - 6 + st.bs
    name = next(n for n in MP.names("one_cb_cr_differ", depth) if shift_of(n) >= 4)      # (from shift 4 on the 16-bit limit lies below 255)
    rec = list(MP.program(name))
    st = T.StateModel()
    T.replay(st, rec)
    shift = shift_of(name)
    ysl, cbsl, crsl = (st.plut[c][0] >> 4 for c in range(3))
    free = [k for k in range(8) if k not in (cbsl, crsl)]
    limit = min(MP.fits16_limit(shift), 255)
    rng = MP.Rng(name + "/reprogram")
    moved = bytearray(uniform_lut(ysl))
    moved[100] = ((ysl + 1) % 8) << 4                 # an intensity of the in-range content
    cr_at = bytes(min(b, limit) for b in st.slut[2])
    over = bytearray(cr_at)
    over[130] = min(limit + 1, 255)
    clean = MP._pattern(rng, lowest=-127)
    dirty = clean.copy()
    dirty[5] = -128
    steps = [
        (T.OP_PATTERN_LUT, 0, 0, uniform_lut(ysl)),            # 0: uniform luma LUT (low nibbles cleared: a changed LUT, the same form)
        (T.OP_PATTERN_LUT, 0, 0, bytes(moved)),                # 1: one entry on another slot -> general luma
        (T.OP_PATTERN_LUT, 0, 0, uniform_lut(ysl)),            # 2: moved back
        (T.OP_SCALE_LUT, 2, 0, bytes(over)),                   # 3: Cr one over the 16-bit limit -> general chroma at 8 bit
        (T.OP_SCALE_LUT, 2, 0, cr_at),                         # 4: pulled back
        (T.OP_CHROMA_PATTERN, cbsl, 0, dirty.tobytes()),       # 5: a -128 in the selected Cb slot -> general chroma
        (T.OP_CHROMA_PATTERN, cbsl, 0, clean.tobytes()),       # 6: overwritten without it
        (T.OP_PATTERN_LUT, 0, 0, uniform_lut(8)),              # 7: luma on slot 8
        (T.OP_SCALE_SHIFT, shift - 1, 0, b""),                 # 8: another scale_shift (a smaller one: every scale still fits)
        (T.OP_CHROMA_PATTERN, free[0], 0, dirty.tobytes()),    # 9: a -128 in an unselected slot: no form change
    ]
    frames = MP.content(name, W, H, len(steps), "in_range", pad=64)
    devs = [DevFrame(f) for f in frames]
    torch.cuda.synchronize()
    program(hip, rec)
    ora = oracle_for(rec)
    forms, seeds = [], []
    for step, d, f in zip(steps, devs, frames):
        rec.append(step)
        T.replay(hip, [step])
        T.replay(ora, [step])
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        info = check_form(hip, rec)
        forms.append((bool(info["one_y"]), bool(info["one_c"])))
        ora.add_grain_frame(f)
        seeds.append((hip.seed_state(), ora.seed_state()))
    torch.cuda.synchronize()
    for i, (d, f) in enumerate(zip(devs, frames)):
        assert_equal(d.download(), f, f"frame {i}")
    assert all(a == b for a, b in seeds)
    t, f_ = True, False
    fits = depth != 8
    assert limit < 255
    assert forms == [(t, t), (f_, t), (t, t), (t, fits), (t, t), (t, f_), (t, t), (t, t), (t, t), (t, t)], forms


# ---- device-generated slots ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_8_420"])
def test_device_generated_slots(hip, name):
    """Programmed through the firmware (patterns generated on the device, never on the host), then reprogrammed through the setters:
    fw_patch_tables has to fill a one-pattern image from a device slot, from slot 8, and from a mix of device and host slots."""
    from gpu_util import DevFrame, stream_ptr
    from versatilefilmgrain_amd import fw
    rec = list(T.load_trace(name))
    depth, sx, sy = T.trace_geometry(rec)
    seed, cfgs = T.load_fwcfg(name)
    hip.lib.vfgs_hip_reset_state()
    hip.set_depth(depth)
    hip.set_chroma_subsampling(sx, sy)
    for i, (kind, raw) in enumerate(cfgs):
        fw.init(fw.struct_from_bytes(kind, raw))
        if i == 0:
            hip.set_seed(seed)
    ora = oracle_for(rec)
    rng = MP.Rng(name + "/device slots")
    ys = sorted({a for op, a, _b, _p in rec if op == T.OP_LUMA_PATTERN})
    cs = sorted({a for op, a, _b, _p in rec if op == T.OP_CHROMA_PATTERN})
    ydev, cdev = ys[min(3, len(ys) - 1)], cs[0]                       # slots the firmware generated
    chost = next((k for k in range(7, -1, -1) if k not in cs), 5)    # a chroma slot it did not (or one to overwrite)
    host_c = MP._pattern(rng, lowest=-127)
    host_y = MP._with_m128(MP._pattern(rng), rng)
    steps = [
        [],                                                                      # as the firmware left it
        [(T.OP_PATTERN_LUT, 0, 0, uniform_lut(ydev, 9))],                        # a one-pattern luma image from a device slot
        [(T.OP_PATTERN_LUT, 0, 0, uniform_lut(8, 1))],                           # ... from slot 8
        [(T.OP_PATTERN_LUT, 0, 0, uniform_lut(ydev)), (T.OP_CHROMA_PATTERN, chost, 0, host_c.tobytes()),
         (T.OP_PATTERN_LUT, 1, 0, uniform_lut(cdev, 3)), (T.OP_PATTERN_LUT, 2, 0, uniform_lut(chost, 7))],      # Cb on a device slot, Cr on a host slot
        [(T.OP_LUMA_PATTERN, ydev, 0, host_y.tobytes())],                           # the selected luma slot from the host, with -128: general
    ]
    frames = MP.content(f"general_runs_{depth}_420", W, H, len(steps), "in_range", pad=64)
    forms = []
    for k, (step, f) in enumerate(zip(steps, frames)):
        rec += step
        T.replay(hip, step)
        T.replay(ora, step)
        d = DevFrame(f)
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        info = check_form(hip, rec)
        forms.append((bool(info["one_y"]), bool(info["one_c"])))
        want = f.copy()
        ora.add_grain_frame(want)
        assert_equal(d.download(), want, f"step {k}")
        assert hip.seed_state() == ora.seed_state()
    assert [f[0] for f in forms[1:]] == [True, True, True, False] and forms[3][1], forms


# ---- the luma / chroma mix -------------------------------------------------------------------------------------------------------

MIXES = {"neutral": ((0, 64, 0), (0, 64, 0)), "low": ((127, -128, -256), (127, -128, -256)), "high": ((-128, 127, 255), (-128, 127, 255)),
         "cb_only": ((64, 119, -238), None), "differ": ((32, 32, 0), (-16, 80, 12))}


def mix_cases():
    for cls in ("one_same_slot", "one_cb_cr_differ", "slot8_luma", "slot8_cb"):
        for depth in (8, 10):
            for fmt in MP.FORMATS:
                for m in MIXES:
                    yield pytest.param(f"{cls}_{depth}_{fmt}", m, id=f"{cls}_{depth}_{fmt}-{m}")


@pytest.mark.parametrize("name, mix", list(mix_cases()))
def test_chroma_mix_on_one_pattern_programs(hip, name, mix):
    """The mix is admitted for all-one-pattern forms.  Expected pictures: tests/chroma_mix_util.py (the oracle on the frame whose
    chroma planes hold the mix; samples it leaves on a clip bound cannot be derived and are left out, their number is printed).
    The two saturating mixes pin the index at 0 / at the top for every sample: there the derivation sees only the samples the
    grain moves off the bound, and up to 57 % of the chroma samples are left out (luma and every other chroma sample are compared);
    with the neutral mix the index is the sample itself and at most the program's own clipping is left out."""
    from gpu_util import DevFrame, stream_ptr
    rec = MP.program(name)
    depth = MP.parse(name)[1]
    mixes = MIXES[mix]
    assert MP.expected_form(rec) == (True, True)
    frames = MP.content(name, W, H, 2, "in_range", pad=64)
    res, excluded, ora = X.expected_frames(T.OracleHW, rec, frames, mixes)
    total = sum(f.U.size + f.V.size for f in frames)
    print(f"{name} {mix}: {excluded} of {total} chroma samples left out by the derivation")
    if mix == "neutral":
        assert excluded <= total // 10       # (the index is the sample: only the program's own clipping, which the generator keeps rare)
    entries = ["frame_dev", "copy_dev"] + (["copy8_dev"] if depth == 10 else [])
    for entry in entries:
        hip.lib.vfgs_hip_reset_state()
        T.replay(hip, rec)
        for c, m in enumerate(mixes, 1):
            if m is not None:
                hip.set_chroma_mix(c, *m)
        try:
            if entry == "frame_dev":
                got = []
                for f in frames:
                    d = DevFrame(f)
                    hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
                    got.append(d.download())
                want = res
            elif entry == "copy_dev":
                got, fill = run_copy_dev(hip, frames)
                want = [(written(w, f), m) for (w, m), f in zip(res, fill)]
            else:
                got, fill = run_copy8_dev(hip, frames)
                want = [(written(narrowed(w), f), m) for (w, m), f in zip(res, fill)]
            info = hip.last_launch_info()
            assert info["one_y"] == 1 and info["one_c"] == 1 and info["depth"] == depth and info["kernel"].startswith("grain_mix_kernel<"), info
        finally:
            hip.clear_chroma_mix()
        for i, (g, (w, masks)) in enumerate(zip(got, want)):
            n = X.mismatches(g, w, masks)
            assert n == 0, f"{entry}: frame {i}: {n} samples differ from the expectation"
        assert hip.seed_state() == ora.seed_state()


@pytest.mark.parametrize("name", ["general_runs_10_420", "one_y_general_c_8_444", "general_y_one_c_10_422", "m128_cr_only_8_440", "pk16_split_8_420_s7"])
def test_chroma_mix_is_refused_for_a_general_form(hip, name):
    import torch
    from gpu_util import DevFrame, stream_ptr
    from versatilefilmgrain_amd.hw import VfgsHipError
    rec = MP.program(name)
    assert MP.expected_form(rec) != (True, True)
    f = MP.content(name, W, H, 1, "in_range")[0]
    program(hip, rec)
    hip.set_chroma_mix(1, 64, 119, -238)
    try:
        seeds = hip.seed_state()
        d = DevFrame(f)
        with pytest.raises(VfgsHipError, match=f"error {E_UNSUPPORTED}"):
            hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        torch.cuda.synchronize()
        assert d.download().equal_all(f) and hip.seed_state() == seeds
    finally:
        hip.clear_chroma_mix()
