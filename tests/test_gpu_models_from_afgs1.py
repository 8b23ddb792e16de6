"""GPU (MI355X): vfgs_hip_models_from_afgs1 -- film grain models built on the device straight from AFGS1 parameter sets, a chunk of models per
launch (fw_models_kernel) -- through the C ABI.  Every comparison is exact and over all bytes: every sample of every plane of every picture,
padding included, the four seed registers, and every byte of a model's record + image (vfgs_hip_model_image).

The contract (include/vfgs_hip_fw.h): at the programmed depth and chroma format, out[i] is what
    vfgs_hip_afgs1_chroma_mix(0); vfgs_init_afgs1(&cfgs[i]); vfgs_hip_model_capture(&out[i], stream);
gives, and the programmed state is untouched.  The truth of the pictures is the oracle programmed with the reference firmware's own
recorded programming of the same parameter set (tests/golden/traces beside tests/golden/fwcfg), run as the models call's loop
(tests/model_list_util.py); the truth of the bytes is the capture path.

Planar frames are 264 x 88 (17 blocks, the last ragged, by 6 block rows, the last ragged), separate allocations with garbage over the whole
container range; the semi-planar surfaces are those of tests/test_gpu_sp_model_list.py."""
import ctypes as C

import numpy as np
import pytest

import model_list_util as U
import semiplanar_util as SP
import sp_model_list_util as SU
import vfgs_testlib as T
from fw_space import generated_set         # (the generator lives with the others of the firmware's space; the draws are the same)
from gpu_util import stream_ptr
from test_gpu_frame_list import garbage_frame, scattered

pytestmark = pytest.mark.gpu

W, H = 264, 88
AFGS1 = sorted(p.stem for p in T.FWCFG.glob("fgs_afgs1_*.npz"))
DEPTH12 = ["fgs_afgs1_test1_10_420@depth12", "fgs_afgs1_test9_10_420@depth12"]
FORMATS = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "440": (1, 2)}


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


def fw():
    from versatilefilmgrain_amd import fw as m
    return m


def afgs1_of(name):
    """the AFGS1 structure the reference CLI handed to its firmware for this configuration"""
    kind, raw = T.load_fwcfg(name.split("@")[0])[1][-1]
    assert kind == 1
    return fw().struct_from_bytes(1, raw)


def geometry(name):
    return T.trace_geometry(U.model_records(name))


def set_format(hip, depth, sx, sy):
    hip.lib.vfgs_hip_reset_state()
    hip.set_depth(depth)
    hip.set_chroma_subsampling(sx, sy)


def groups():
    out = {}
    for n in AFGS1 + DEPTH12:
        out.setdefault(geometry(n), []).append(n)
    return out


GROUPS = groups()


def test_the_fixtures_are_the_issue_s():
    assert len(AFGS1) == 35 and {afgs1_of(n).ar_coeff_lag for n in AFGS1} == {2, 3}
    assert set(GROUPS) == {(8, 2, 2), (10, 2, 2), (10, 2, 1), (8, 1, 1), (10, 1, 1), (12, 2, 2)}, sorted(GROUPS)


def release(hip, models):
    for m in models:
        hip.model_release(m)


def grain_and_check(hip, models, recs, seeds, pick, depth, sx, sy, frame_seed, stream=None):
    """one picture per entry of pick through ONE planar models call against the oracle's loop; -> the device frames"""
    frames = [garbage_frame(W, H, depth, sx, sy, frame_seed + i) for i in range(len(pick))]
    sd = [seeds[k] for k in pick]
    want, regs = U.expect_seeded(recs, pick, frames, sd)
    dev = scattered(frames, frame_seed)
    f0 = frames[0]
    hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev], None, [models[k] for k in pick], sd, W, H, f0.stride, f0.cstride,
                                        stream_ptr() if stream is None else stream)
    for i, (d, w) in enumerate(zip(dev, want)):
        assert d.download().equal_all(w), (i, pick[i])
    assert hip.seed_state() == regs
    return dev


# ---- 1. reference truth ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geo", sorted(GROUPS), ids=lambda g: "%d_%d%d" % g)
def test_reference_truth(hip, geo):
    """every recorded AFGS1 parameter set of this depth and format, built in ONE call; a picture per model in one launch, models shuffled"""
    names = GROUPS[geo]
    depth, sx, sy = geo
    set_format(hip, depth, sx, sy)
    cfgs = [afgs1_of(n) for n in names]
    models = hip.models_from_afgs1(cfgs, stream_ptr())
    try:
        assert len(models) == len(names) and all(models) and len(set(models)) == len(models)
        recs = [U.model_records(n) for n in names]
        seeds = [fw().afgs1_seed(c) for c in cfgs]
        pick = [int(k) for k in np.random.default_rng(depth + sx + sy).permutation(len(names))]
        grain_and_check(hip, models, recs, seeds, pick, depth, sx, sy, 100)
        for m in models:
            i = hip.model_info(m)
            assert (i["depth"], i["csubx"], i["csuby"]) == geo and i["one_y"] == 1 and i["one_c"] == 1, i
    finally:
        release(hip, models)


# ---- 2. against the capture path, byte for byte ------------------------------------------------------------------------------------

def captured(hip, cfg):
    fw().afgs1_chroma_mix(False)
    fw().init_afgs1(cfg)
    return hip.model_capture(stream_ptr())


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_bytes_equal_the_capture_path(hip, depth, fmt):
    """40 generated sets in ONE call (two chunks): info equal everywhere, record + image equal wherever both components are one-pattern (a
    general-form image of the capture path also holds the slots no LUT selects, which the built one leaves zero)"""
    sx, sy = FORMATS[fmt]
    set_format(hip, depth, sx, sy)
    rng = np.random.default_rng(1000 * depth + 10 * sx + sy)
    n = 40
    assert n > hip.model_build_stats()["models_per_launch"] == 32
    cfgs = [generated_set(rng) for _ in range(n)]
    s0 = hip.model_build_stats()
    built = hip.models_from_afgs1(cfgs, stream_ptr())
    try:
        s1 = hip.model_build_stats()
        assert s1["calls"] - s0["calls"] == 1 and s1["models"] - s0["models"] == n and s1["launches"] - s0["launches"] == 2 \
            and s1["copies"] - s0["copies"] == 2, (s0, s1)
        images = [hip.model_image(m) for m in built]       # (before the capture path programs anything)
        infos = [hip.model_info(m) for m in built]
        compared = 0
        for i, cfg in enumerate(cfgs):
            m = captured(hip, cfg)
            try:
                info = hip.model_info(m)
                assert infos[i] == info, (i, infos[i], info)
                assert len(images[i]) == info["device_bytes"]
                if info["one_y"] and info["one_c"]:
                    want = hip.model_image(m)
                    if images[i] != want:
                        a, b = np.frombuffer(images[i], np.uint8), np.frombuffer(want, np.uint8)
                        bad = np.flatnonzero(a != b)
                        raise AssertionError(f"set {i}: {len(bad)} bytes differ, first at {bad[0]} of {len(a)}: {a[bad[0]]} != {b[bad[0]]}")
                    compared += 1
            finally:
                hip.model_release(m)
        assert compared >= (n // 2 if depth == 8 else n), compared       # (above 8 bit every AFGS1 model is all one-pattern)
    finally:
        release(hip, built)


# ---- 3. the 8-bit fall-back to the general form ------------------------------------------------------------------------------------

def c_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def scaling_lut(xs, ys):
    """vfgs_fw.c:649-661 restated: zero outside the points, rounded interpolation with C's division between them"""
    lut = [0] * 256
    for s in range(len(xs) - 1):
        x0, span, rise = xs[s], xs[s + 1] - xs[s], ys[s + 1] - ys[s]
        for t in range(x0, x0 + span + (1 if s + 2 == len(xs) else 0)):
            lut[t] = (ys[s] + c_div(rise * (t - x0) + span // 2, span)) & 255
    return bytes(lut)


def oracle_program_420(cfg, depth):
    """what the reference firmware programs for an AFGS1 set at 4:2:0 (vfgs_fw.c:663-708), from the numpy restatement of its generator"""
    import sys
    sys.path.insert(0, str(T.ORACLE_DIR))
    import vfgs_fw_oracle as FO
    lag = cfg.ar_coeff_lag
    rec = [(T.OP_DEPTH, depth, 0, b""), (T.OP_CHROMA_SUBSAMPLING, 2, 2, b"")]
    ly = scaling_lut(list(cfg.point_y_values)[:cfg.num_y_points], list(cfg.point_y_scaling)[:cfg.num_y_points])
    lcb = ly if cfg.chroma_scaling_from_luma else scaling_lut(list(cfg.point_cb_values)[:cfg.num_cb_points], list(cfg.point_cb_scaling)[:cfg.num_cb_points])
    lcr = ly if cfg.chroma_scaling_from_luma else scaling_lut(list(cfg.point_cr_values)[:cfg.num_cr_points], list(cfg.point_cr_scaling)[:cfg.num_cr_points])
    for c, l in enumerate((ly, lcb, lcr)):
        rec.append((T.OP_SCALE_LUT, c, 0, l))
    n = 2 * lag * (lag + 1)
    P = FO.ar_pattern(0, FO.afgs1_taps(list(cfg.ar_coeffs_y)[:n], lag), cfg.ar_coeff_shift, cfg.grain_scale_shift + 1, 0)
    rec.append((T.OP_LUMA_PATTERN, 0, 0, P.tobytes()))
    for slot, ar in ((0, cfg.ar_coeffs_cb), (1, cfg.ar_coeffs_cr)):
        Pc = FO.ar_pattern(1, FO.afgs1_taps(list(ar)[:n], lag), cfg.ar_coeff_shift, cfg.grain_scale_shift + 1, 1 + slot)
        rec.append((T.OP_CHROMA_PATTERN, slot, 0, Pc.tobytes() + bytes(4096 - 1024)))
    rec += [(T.OP_PATTERN_LUT, 0, 0, bytes(256)), (T.OP_PATTERN_LUT, 1, 0, bytes(256)), (T.OP_PATTERN_LUT, 2, 0, bytes([1]) * 256),
            (T.OP_SCALE_SHIFT, cfg.grain_scaling - 6, 0, b""), (T.OP_LEGAL_RANGE, cfg.clip_to_restricted_range, 0, b"")]
    return rec


def fallback_set(chroma_255):
    a = fw().FgsAfgs1()
    a.grain_seed = 4711
    a.num_y_points = 2
    a.point_y_values[0], a.point_y_values[1] = 0, 255
    a.point_y_scaling[0], a.point_y_scaling[1] = 60, 255
    a.num_cb_points = a.num_cr_points = 2
    a.point_cb_values[0], a.point_cb_values[1] = 0, 240
    a.point_cb_scaling[0], a.point_cb_scaling[1] = 30, 255 if chroma_255 else 200
    a.point_cr_values[0], a.point_cr_values[1] = 10, 255
    a.point_cr_scaling[0], a.point_cr_scaling[1] = 90, 40
    a.grain_scaling = 11
    a.ar_coeff_lag = 2
    for k in range(12):
        a.ar_coeffs_y[k] = (5, -9, 14, -3, 7, 11, -20, 9, 30, -6, 12, 40)[k]
        a.ar_coeffs_cb[k] = (-4, 8, 3, -12, 6, 2, 17, -8, 9, 25, -3, 33)[k]
        a.ar_coeffs_cr[k] = (9, 9, -9, 9, -9, 9, 9, -9, 9, 9, -9, 9)[k]
    a.ar_coeff_shift = 7
    a.grain_scale_shift = 0
    a.clip_to_restricted_range = 1
    return a


@pytest.mark.parametrize("chroma_255", [False, True], ids=["general_y_one_c", "general_y_general_c"])
def test_the_8_bit_fall_back_to_the_general_form(hip, chroma_255):
    """grain_scaling 11 with a scaling point of 255: 255 x 127 + 2^10 does not fit an int16, the component takes the general form"""
    set_format(hip, 8, 2, 2)
    plain = afgs1_of("fgs_afgs1_test1_8_420")
    cfgs = [fallback_set(chroma_255), plain]
    built = hip.models_from_afgs1(cfgs, stream_ptr())
    caps = []
    try:
        forms = [(hip.model_info(m)["one_y"], hip.model_info(m)["one_c"]) for m in built]
        assert forms == [(0, 0 if chroma_255 else 1), (1, 1)], forms
        recs = [oracle_program_420(cfgs[0], 8), U.model_records("fgs_afgs1_test1_8_420")]
        seeds = [fw().afgs1_seed(c) for c in cfgs]
        pick = [0, 1, 0, 0, 1]
        dev_b = grain_and_check(hip, built, recs, seeds, pick, 8, 2, 2, 300)          # == the oracle's
        caps = [captured(hip, c) for c in cfgs]
        assert [hip.model_info(m) for m in caps] == [hip.model_info(m) for m in built]
        dev_c = grain_and_check(hip, caps, recs, seeds, pick, 8, 2, 2, 300)           # the same frames through the captured models
        for a, b in zip(dev_b, dev_c):
            assert a.download().equal_all(b.download())
    finally:
        release(hip, built + caps)


# ---- 4. the programmed state is untouched --------------------------------------------------------------------------------------------

def recorded_state(hip):
    return {"params": hip.params(), "luts": [hip.luts(c) for c in range(3)],
            "patterns": [fw().get_pattern(b, k) for b in range(2) for k in range(8)],
            "seed": hip.seed_state(), "mix": [hip.chroma_mix(c) for c in (1, 2)]}


def test_the_programmed_state_is_untouched(hip):
    """fgs_sei_10_420 programmed by vfgs_init_sei (its slots are device-generated), a seed, a frame, a chroma mix on Cb; then 8 AFGS1 models
    are built.  (The mix is set behind the frame, not in front of it: this model's luma image is general-form, which the kernels of the mix
    refuse.)"""
    name = "fgs_sei_10_420"
    rec = T.load_trace(name)
    seed, cfgs = T.load_fwcfg(name)
    set_format(hip, 10, 2, 2)
    structs = [fw().struct_from_bytes(k, raw) for k, raw in cfgs]
    for i, s in enumerate(structs):
        fw().init(s)
        if i == 0:
            hip.set_seed(seed)
    ora = T.OracleHW()
    T.replay(ora, rec)
    hip.set_seed(99)
    ora.set_seed(99)

    def frames_through(call_list, first_seed):
        frames = [garbage_frame(W, H, 10, 2, 2, first_seed + i) for i in range(2)]
        want = [f.copy() for f in frames]
        for w in want:
            ora.add_grain_frame(w)
        dev = scattered(frames, first_seed)
        call_list([d.ptrs() for d in dev], W, H, frames[0].stride, frames[0].cstride, stream_ptr())
        for d, w in zip(dev, want):
            assert d.download().equal_all(w)
        assert hip.seed_state() == ora.seed_state()

    frames_through(hip.add_grain_frame_list_dev, 400)
    hip.set_chroma_mix(1, 40, -30, 7)
    before = recorded_state(hip)
    launches = U.launches(hip)
    built = hip.models_from_afgs1([afgs1_of(n) for n in GROUPS[(10, 2, 2)][:8]], stream_ptr())
    try:
        assert recorded_state(hip) == before and U.launches(hip) == launches
    finally:
        release(hip, built)
    assert recorded_state(hip) == before
    hip.clear_chroma_mix()
    frames_through(hip.add_grain_frame_list_dev, 410)          # the oracle's NEXT frames for fgs_sei_10_420
    # the request vfgs_init_sei made last is still the library's most recent one: re-sending it generates nothing, and the banks it
    # would have to regenerate had the build disturbed them are still right
    regs = hip.seed_state()
    fw().init(structs[-1])
    assert hip.seed_state() == regs
    frames_through(hip.add_grain_frame_list_dev, 420)


# ---- 5. semi-planar surfaces -----------------------------------------------------------------------------------------------------------

def test_semi_planar_surfaces(hip):
    """four built models at 10-bit 4:2:0 on P010 surfaces of 1032 x 90: A B C D A B C, seeded, in place"""
    from test_gpu_semiplanar import DevSP, assert_equal, scattered as sp_scattered
    names = ["fgs_afgs1_test1_10_420", "fgs_afgs1_test9_10_420", "fgs_afgs1_test3_10_420", "fgs_afgs1_test12_10_420"]
    set_format(hip, 10, 2, 2)
    cfgs = [afgs1_of(n) for n in names]
    built = hip.models_from_afgs1(cfgs, stream_ptr())
    try:
        pick = [0, 1, 2, 3, 0, 1, 2]
        recs = [U.model_records(n) for n in names]
        seeds = [fw().afgs1_seed(cfgs[k]) for k in pick]
        frames = [SP.garbage_sp_frame(1032, 90, 10, 2, 6, 500 + i) for i in range(len(pick))]
        want, regs = SU.expect_seeded(recs, pick, frames, seeds, 6)
        dev = sp_scattered(frames, 5)
        f0 = frames[0]
        hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in dev], None, [built[k] for k in pick], seeds, f0.width, f0.height,
                                               f0.stride, f0.uv_stride, 6, stream_ptr())
        for i, (d, w) in enumerate(zip(dev, want)):
            assert_equal(d.download(), w, f"frame {i}")
        assert hip.seed_state() == regs
        assert hip.last_launch_info()["kernel"] == T.kernel_name("grain_spml_kernel", 10, 2, True, True)
    finally:
        release(hip, built)


# ---- 6. lifetime and streams -----------------------------------------------------------------------------------------------------------

def test_lifetime_and_streams(hip):
    import torch
    geo = (10, 2, 2)
    names = (GROUPS[geo] * 2)[:32]
    set_format(hip, *geo)
    cfgs = [afgs1_of(n) for n in names]
    recs = [U.model_records(n) for n in names]
    seeds = [fw().afgs1_seed(c) for c in cfgs]
    s_build, s_grain = torch.cuda.Stream(), torch.cuda.Stream()
    rng = np.random.default_rng(6)

    # built on one stream, grained on another: the first use waits for the build by event
    built = hip.models_from_afgs1(cfgs, s_build.cuda_stream)
    pick = [int(k) for k in rng.permutation(32)[:9]]
    grain_and_check(hip, built, recs, seeds, pick, *geo, 600, stream=s_grain.cuda_stream)

    # the chunk released in shuffled order while a queued launch still reads half of it
    half = [int(k) for k in rng.permutation(32)[:16]]
    frames = [garbage_frame(W, H, 10, 2, 2, 620 + i) for i in range(16)]
    sd = [seeds[k] for k in half]
    want, regs = U.expect_seeded(recs, half, frames, sd)
    dev = scattered(frames, 7)
    hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev], None, [built[k] for k in half], sd, W, H, frames[0].stride, frames[0].cstride,
                                        s_grain.cuda_stream)
    for k in rng.permutation(32):
        hip.model_release(built[int(k)])
    with pytest.raises(Exception, match="41"):
        hip.model_info(built[0])
    again = hip.models_from_afgs1(cfgs, s_build.cuda_stream)           # (takes the slab that was just left: waits for its readers)
    for d, w in zip(dev, want):
        assert d.download().equal_all(w)
    grain_and_check(hip, again, recs, seeds, pick, *geo, 640, stream=s_grain.cuda_stream)
    release(hip, again)

    # build / grain / release: no allocation and no free after the first cycle; a launch and a copy per chunk
    marks = []
    for cycle in range(3):
        s0 = hip.model_build_stats()
        ms = hip.models_from_afgs1(cfgs, stream_ptr())
        s1 = hip.model_build_stats()
        assert s1["launches"] - s0["launches"] == 1 and s1["copies"] - s0["copies"] == 1 and s1["models"] - s0["models"] == 32, (s0, s1)
        grain_and_check(hip, ms, recs, seeds, pick[:3], *geo, 660 + cycle)
        release(hip, ms)
        s2 = hip.model_build_stats()
        marks.append((s2["allocations"], s2["frees"]))
    assert marks[1] == marks[0] and marks[2] == marks[0], marks
    # ceil(n / 32) launches and copies per call
    for n in (1, 33):
        s0 = hip.model_build_stats()
        ms = hip.models_from_afgs1((cfgs * 2)[:n], stream_ptr())
        s1 = hip.model_build_stats()
        assert s1["launches"] - s0["launches"] == (n + 31) // 32 == s1["copies"] - s0["copies"], (n, s0, s1)
        release(hip, ms)
    torch.cuda.synchronize()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------

def spoil(cause):
    """-> (what to do to a valid parameter set, the code the call answers with)"""
    def points(a, which, xs):
        setattr(a, f"num_{which}_points", len(xs))
        for k, x in enumerate(xs):
            getattr(a, f"point_{which}_values")[k] = x

    table = {
        "lag_0": (lambda a: setattr(a, "ar_coeff_lag", 0), 42),
        "lag_4": (lambda a: setattr(a, "ar_coeff_lag", 4), 42),
        "y_points_15": (lambda a: setattr(a, "num_y_points", 15), 42),
        "cb_points_11": (lambda a: setattr(a, "num_cb_points", 11), 42),
        "cr_points_11": (lambda a: setattr(a, "num_cr_points", 11), 42),
        "y_points_equal": (lambda a: points(a, "y", [10, 50, 50, 90]), 42),
        "y_points_falling": (lambda a: points(a, "y", [10, 50, 40]), 42),
        "cb_points_equal": (lambda a: (setattr(a, "chroma_scaling_from_luma", 0), points(a, "cb", [0, 0])), 42),
        "cr_points_falling": (lambda a: (setattr(a, "chroma_scaling_from_luma", 0), points(a, "cr", [9, 200, 100])), 42),
        "ar_coeff_shift_0": (lambda a: setattr(a, "ar_coeff_shift", 0), 42),
        "ar_coeff_shift_16": (lambda a: setattr(a, "ar_coeff_shift", 16), 42),
        "grain_scale_shift_7": (lambda a: setattr(a, "grain_scale_shift", 7), 42),
        "grain_scaling_7": (lambda a: setattr(a, "grain_scaling", 7), 9),
        "grain_scaling_14": (lambda a: setattr(a, "grain_scaling", 14), 9),
    }
    return table[cause]


CAUSES = ["lag_0", "lag_4", "y_points_15", "cb_points_11", "cr_points_11", "y_points_equal", "y_points_falling", "cb_points_equal",
          "cr_points_falling", "ar_coeff_shift_0", "ar_coeff_shift_16", "grain_scale_shift_7", "grain_scaling_7", "grain_scaling_14"]


def raw_call(hip, arr, n, out):
    rc = hip.lib.vfgs_hip_models_from_afgs1(arr, n, out, stream_ptr())
    return rc, hip.lib.vfgs_hip_last_error_string().decode()


@pytest.mark.parametrize("at", [0, 4], ids=["first", "last"])
@pytest.mark.parametrize("cause", CAUSES)
def test_refusals(hip, cause, at):
    set_format(hip, 8, 2, 2)
    hip.set_seed(31)
    arr = (fw().FgsAfgs1 * 5)(*[afgs1_of(n) for n in GROUPS[(8, 2, 2)][:5]])
    change, code = spoil(cause)
    change(arr[at])
    out = (C.c_void_p * 5)(*[0xdead0 + i for i in range(5)])
    stats, regs, launches = hip.model_build_stats(), hip.seed_state(), U.launches(hip)
    rc, msg = raw_call(hip, arr, 5, out)
    assert rc == code and f"parameter set {at}:" in msg, (rc, msg)
    assert all(v is None for v in out), list(out)
    assert hip.model_build_stats() == stats and hip.seed_state() == regs and U.launches(hip) == launches


def test_refusals_of_the_pointers_and_the_empty_call(hip):
    set_format(hip, 8, 2, 2)
    arr = (fw().FgsAfgs1 * 2)(*[afgs1_of(n) for n in GROUPS[(8, 2, 2)][:2]])
    out = (C.c_void_p * 2)(0xdead0, 0xdead1)
    stats = hip.model_build_stats()
    assert raw_call(hip, arr, 2, None)[0] == 41
    rc, msg = raw_call(hip, None, 2, out)
    assert rc == 41 and list(out) == [None, None], (rc, msg)
    out = (C.c_void_p * 2)(0xdead0, 0xdead1)
    assert raw_call(hip, arr, 0, out)[0] == 0 and list(out) == [0xdead0, 0xdead1]      # n == 0 is no call at all
    assert raw_call(hip, None, 0, None)[0] == 0
    assert hip.models_from_afgs1([]) == []
    assert hip.model_build_stats() == stats
    # what is NOT refused: Cb / Cr points out of order under chroma_scaling_from_luma -- those functions are not used
    a = afgs1_of(GROUPS[(8, 2, 2)][0])
    a.chroma_scaling_from_luma = 1
    a.num_cb_points = 2
    a.point_cb_values[0], a.point_cb_values[1] = 80, 20
    ms = hip.models_from_afgs1([a], stream_ptr())
    release(hip, ms)
