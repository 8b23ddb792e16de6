"""GPU (MI355X): vfgs_hip_models_from_sei -- film grain models built on the device straight from FGC SEI messages, a chunk of models per launch
(fw_sei_build_kernel) -- through the C ABI.  Every comparison is exact and over all bytes: every sample of every plane of every picture,
padding included, the four seed registers, and every byte of a model's record + image (vfgs_hip_model_image) in EVERY form.

The contract (include/vfgs_hip_fw.h): at the programmed depth, chroma format and legal range, out[i] is what
    vfgs_hip_reset_state(); vfgs_set_depth; vfgs_set_chroma_subsampling; vfgs_set_legal_range; vfgs_init_sei(&cfgs[i]); vfgs_hip_model_capture(&out[i], stream);
gives, and the programmed state is untouched.  The truth of the pictures is the oracle programmed with the reference firmware's own recorded
programming of the same message (tests/golden/traces beside tests/golden/fwcfg), run as the models call's loop (tests/model_list_util.py);
the truth of the bytes is the capture path from a reset state.

Planar frames are 264 x 88 (17 blocks, the last ragged, by 6 block rows, the last ragged), separate allocations with garbage over the whole
container range; the semi-planar surfaces are those of tests/test_gpu_sp_model_list.py."""
import ctypes as C

import numpy as np
import pytest

import model_list_util as U
import sei_model_util as G
import semiplanar_util as SP
import sp_model_list_util as SU
import vfgs_testlib as T
from gpu_util import stream_ptr
from test_gpu_frame_list import garbage_frame, scattered

pytestmark = pytest.mark.gpu

W, H = 264, 88
SEI = sorted(p.stem for pat in ("default*.npz", "fgs_sei*.npz") for p in T.FWCFG.glob(pat))
DEPTH12 = ["default_10_420@depth12", "fgs_sei_ar_test1_10_420@depth12"]
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


def sei_of(name):
    """the SEI structure the reference CLI handed to its firmware last for this configuration"""
    kind, raw = T.load_fwcfg(name.split("@")[0])[1][-1]
    assert kind == 0
    return fw().struct_from_bytes(0, raw)


def geometry(name):
    return T.trace_geometry(U.model_records(name))


def set_format(hip, depth, sx, sy, legal=0):
    hip.lib.vfgs_hip_reset_state()
    hip.set_depth(depth)
    hip.set_chroma_subsampling(sx, sy)
    hip.set_legal_range(legal)


def groups():
    out = {}
    for n in SEI + DEPTH12:
        out.setdefault(geometry(n), []).append(n)
    return out


GROUPS = groups()


def luma_patterns(s):
    return len({tuple(s.comp_model_value[0][k][j] for j in range(1, 6)) for k in range(s.num_intensity_intervals[0])}) if s.comp_model_present_flag[0] else 0


def test_the_fixtures_are_the_issue_s():
    assert len(SEI) == 27
    assert set(GROUPS) == {(8, 2, 2), (10, 2, 2), (8, 2, 1), (10, 2, 1), (8, 1, 1), (10, 1, 1), (12, 2, 2)}, sorted(GROUPS)
    assert luma_patterns(sei_of("default_10_420")) == 8 and max(luma_patterns(sei_of(n)) for n in SEI) == 8
    assert {n for n in SEI if sei_of(n).model_id == 1} == {"fgs_sei_ar_test1_8_420", "fgs_sei_ar_test1_10_420"}


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


def seeds_for(n, salt):
    return [int(v) for v in np.random.default_rng(salt).integers(1, 1 << 32, n)]


# ---- 2. reference truth ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geo", sorted(GROUPS), ids=lambda g: "%d_%d%d" % g)
def test_reference_truth(hip, geo):
    """every recorded SEI message of this depth and format, built in ONE call; a picture per model in one planar models call, models
    shuffled, a seed per picture.  Depth 12: test_gpu_depth12.records12 makes a 12-bit record of any 10-bit trace, so the group (12, 2, 2)
    holds the CLI default (8 luma patterns, frequency filtered) and the auto-regressive message as `name@depth12`."""
    names = GROUPS[geo]
    depth, sx, sy = geo
    set_format(hip, depth, sx, sy)
    cfgs = [sei_of(n) for n in names]
    models = hip.models_from_sei(cfgs, stream_ptr())
    try:
        assert len(models) == len(names) and all(models) and len(set(models)) == len(models)
        recs = [U.model_records(n) for n in names]
        seeds = seeds_for(len(names), depth + sx + sy)
        pick = [int(k) for k in np.random.default_rng(depth + sx + sy).permutation(len(names))]
        grain_and_check(hip, models, recs, seeds, pick, depth, sx, sy, 100)
        for m in models:
            i = hip.model_info(m)
            assert (i["depth"], i["csubx"], i["csuby"]) == geo and i["legal_range"] == 0, i
    finally:
        release(hip, models)


# ---- 3. against the capture path, byte for byte ------------------------------------------------------------------------------------

def captured(hip, depth, sx, sy, legal, cfg):
    set_format(hip, depth, sx, sy, legal)
    fw().init_sei(cfg)
    return hip.model_capture(stream_ptr())


def assert_same_bytes(i, got, want):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        if len(a) != len(b):
            raise AssertionError(f"message {i}: {len(a)} bytes, capture has {len(b)}")
        bad = np.flatnonzero(a != b)
        raise AssertionError(f"message {i}: {len(bad)} bytes differ, first at {bad[0]} of {len(a)}: {a[bad[0]]} != {b[bad[0]]}")


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_bytes_equal_the_capture_path(hip, depth, fmt):
    """40 generated messages in ONE call (two chunks), once per legal range (the range is the programmed state's, not a message's): info
    equal and record + image equal in every form, with no exemption.  What the 40 messages cover is asserted from the messages
    (sei_model_util.facts; on the CPU in tests/test_sei_model_generator_cpu.py) and, for the forms, from the models."""
    sx, sy = FORMATS[fmt]
    n = 40
    cfgs = G.generated_list(fw().FgsSei, G.list_seed(depth, sx, sy), n)
    seen = set().union(*[G.facts(c) for c in cfgs])
    assert not G.REQUIRED - seen, sorted(G.REQUIRED - seen)
    forms = set()
    for legal in (0, 1):
        set_format(hip, depth, sx, sy, legal)
        assert n > hip.model_build_stats()["models_per_launch"] == 32
        s0 = hip.model_build_stats()
        built = hip.models_from_sei(cfgs, stream_ptr())
        try:
            s1 = hip.model_build_stats()
            assert s1["calls"] - s0["calls"] == 1 and s1["models"] - s0["models"] == n and s1["launches"] - s0["launches"] == 2 \
                and s1["copies"] - s0["copies"] == 2, (s0, s1)
            images = [hip.model_image(m) for m in built]       # (before the capture path programs anything)
            infos = [hip.model_info(m) for m in built]
            for i, cfg in enumerate(cfgs):
                m = captured(hip, depth, sx, sy, legal, cfg)
                try:
                    info = hip.model_info(m)
                    assert infos[i] == info and info["legal_range"] == legal, (i, infos[i], info)
                    assert len(images[i]) == info["device_bytes"]
                    assert_same_bytes(i, images[i], hip.model_image(m))
                    f = G.facts(cfg)
                    forms.add((info["one_y"], info["one_c"]))
                    if "chroma_two_uniform_slots" in f and "scale_250" not in f:
                        assert info["one_c"] == 1, (i, info)       # one-pattern chroma over two slots
                    if i % G.CASES == 17:                          # uniform everywhere, scales >= 250 at a stored shift >= 11
                        assert (info["one_y"], info["one_c"]) == ((0, 0) if depth == 8 else (1, 1)), (i, info)
                finally:
                    hip.model_release(m)
        finally:
            release(hip, built)
    # by construction above 8 bit (every scale LUT fits): case 0 is (1, 1), case 9 (0, 1), case 13 -- luma absent -- (1, 0), case 18 (0, 0)
    assert forms == {(0, 0), (0, 1), (1, 0), (1, 1)} if depth > 8 else (0, 0) in forms, forms


# ---- 4. the programmed state is untouched --------------------------------------------------------------------------------------------

def recorded_state(hip, patterns=True):
    return {"params": hip.params(), "luts": [hip.luts(c) for c in range(3)],
            "patterns": [fw().get_pattern(b, k) for b in range(2) for k in range(8)] if patterns else None,
            "seed": hip.seed_state(), "mix": [hip.chroma_mix(c) for c in (1, 2)]}


def test_the_programmed_state_is_untouched(hip):
    """fgs_sei_10_420 programmed by vfgs_init_sei (its slots are device-generated) with luma slot 7 then set from the host, a seed, a frame, a chroma mix on
    Cb; then 8 SEI models are built: banks, LUTs, parameters, registers and mix are what they were.  Then the CLI default is programmed with
    vfgs_init_sei and NOT flushed by anything (no pattern is read back), models are built, and the next frames are the oracle's for the
    default: the pending pattern requests took effect."""
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
    host_slot = np.random.default_rng(5).integers(-127, 128, 4096).astype(np.int8).tobytes()
    for hw in (hip, ora):                    # (the message's eighth luma pattern replaced by a host-set one, in the oracle too)
        T.replay(hw, [(T.OP_LUMA_PATTERN, 7, 0, host_slot)])
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
    assert before["patterns"][7] == host_slot and any(before["patterns"][0])
    launches = U.launches(hip)
    msgs = [sei_of(n) for n in GROUPS[(10, 2, 2)] if "@" not in n][:8]
    built = hip.models_from_sei(msgs, stream_ptr())
    try:
        assert recorded_state(hip) == before and U.launches(hip) == launches
    finally:
        release(hip, built)
    assert recorded_state(hip) == before
    hip.clear_chroma_mix()
    frames_through(hip.add_grain_frame_list_dev, 410)          # the oracle's NEXT frames for fgs_sei_10_420

    # a vfgs_init_sei whose pattern requests are still pending when the models are built
    other = "default_10_420"
    fw().init(sei_of(other))
    T.replay(ora, U.without_seed(T.load_trace(other)))
    pending = recorded_state(hip, patterns=False)
    built = hip.models_from_sei(msgs, stream_ptr())
    try:
        assert recorded_state(hip, patterns=False) == pending
    finally:
        release(hip, built)
    frames_through(hip.add_grain_frame_list_dev, 420)


# ---- 5. semi-planar surfaces -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth,shift", [(10, 6), (8, 0)], ids=["p010", "nv12"])
def test_semi_planar_surfaces(hip, depth, shift):
    """four SEI-built models at 4:2:0 on P010 / NV12 surfaces of 1032 x 90: A B C D A B C, seeded, in place"""
    from test_gpu_semiplanar import assert_equal, scattered as sp_scattered
    names = [f"default_{depth}_420", f"fgs_sei_ar_test1_{depth}_420", f"fgs_sei_{depth}_420", f"fgs_sei_ff_test2_{depth}_420"]
    set_format(hip, depth, 2, 2)
    built = hip.models_from_sei([sei_of(n) for n in names], stream_ptr())
    try:
        pick = [0, 1, 2, 3, 0, 1, 2]
        recs = [U.model_records(n) for n in names]
        seeds = seeds_for(len(pick), 55 + depth)
        frames = [SP.garbage_sp_frame(1032, 90, depth, 2, shift, 500 + i) for i in range(len(pick))]
        want, regs = SU.expect_seeded(recs, pick, frames, seeds, shift)
        dev = sp_scattered(frames, 5)
        f0 = frames[0]
        hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in dev], None, [built[k] for k in pick], seeds, f0.width, f0.height,
                                               f0.stride, f0.uv_stride, shift, stream_ptr())
        for i, (d, w) in enumerate(zip(dev, want)):
            assert_equal(d.download(), w, f"frame {i}")
        assert hip.seed_state() == regs
    finally:
        release(hip, built)


# ---- 6. one list, three origins ----------------------------------------------------------------------------------------------------------

def test_one_list_three_origins(hip):
    """models from this call, from vfgs_hip_models_from_afgs1 and from vfgs_hip_model_capture interleaved in one planar models call at
    10-bit 4:2:0: the pictures are the oracle's loop, and the launches are the runs of equal form"""
    geo = (10, 2, 2)
    sei_names = ["default_10_420", "fgs_sei_ar_test1_10_420", "fgs_sei_10_420"]
    afgs1_names = ["fgs_afgs1_test1_10_420", "fgs_afgs1_test9_10_420"]
    cap_names = ["fgs_sei_ff_test2_10_420", "fgs_afgs1_test3_10_420"]
    caps = U.capture_all(hip, [U.model_records(n) for n in cap_names], stream_ptr())
    set_format(hip, *geo)
    from_sei = hip.models_from_sei([sei_of(n) for n in sei_names], stream_ptr())
    from_afgs1 = hip.models_from_afgs1([fw().struct_from_bytes(1, T.load_fwcfg(n)[1][-1][1]) for n in afgs1_names], stream_ptr())
    models = from_sei + from_afgs1 + caps
    try:
        names = sei_names + afgs1_names + cap_names
        recs = [U.model_records(n) for n in names]
        forms = [(hip.model_info(m)["one_y"], hip.model_info(m)["one_c"]) for m in models]
        assert len(set(forms)) > 1, forms
        pick = [0, 3, 5, 1, 4, 6, 2, 0, 5, 3, 1, 6]
        seeds = seeds_for(len(names), 66)
        l0 = U.launches(hip)
        grain_and_check(hip, models, recs, seeds, pick, *geo, 700)
        assert U.launches(hip) - l0 == len(U.runs_of(forms, pick)), (forms, pick)
    finally:
        release(hip, models)


# ---- 7. lifetime and streams -----------------------------------------------------------------------------------------------------------

def test_lifetime_and_streams(hip):
    import torch
    geo = (10, 2, 2)
    names = ([n for n in GROUPS[geo] if "@" not in n] * 3)[:32]
    set_format(hip, *geo)
    cfgs = [sei_of(n) for n in names]
    recs = [U.model_records(n) for n in names]
    seeds = seeds_for(32, 77)
    s_build, s_grain = torch.cuda.Stream(), torch.cuda.Stream()
    rng = np.random.default_rng(6)

    # built on one stream, grained on another: the first use waits for the build by event
    built = hip.models_from_sei(cfgs, s_build.cuda_stream)
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
    a0 = hip.model_build_stats()["allocations"]
    again = hip.models_from_sei(cfgs, s_build.cuda_stream)           # (takes the slab that was just left: waits for its readers)
    assert hip.model_build_stats()["allocations"] == a0
    for d, w in zip(dev, want):
        assert d.download().equal_all(w)
    grain_and_check(hip, again, recs, seeds, pick, *geo, 640, stream=s_grain.cuda_stream)
    release(hip, again)

    # build / grain / release: no allocation and no free after the first cycle; a launch and a copy per chunk
    marks = []
    for cycle in range(3):
        s0 = hip.model_build_stats()
        ms = hip.models_from_sei(cfgs, stream_ptr())
        s1 = hip.model_build_stats()
        assert s1["launches"] - s0["launches"] == 1 and s1["copies"] - s0["copies"] == 1 and s1["models"] - s0["models"] == 32, (s0, s1)
        grain_and_check(hip, ms, recs, seeds, pick[:3], *geo, 660 + cycle)
        release(hip, ms)
        s2 = hip.model_build_stats()
        marks.append((s2["allocations"], s2["frees"]))
    assert marks[1] == marks[0] and marks[2] == marks[0], marks

    # SEI and AFGS1 builds alternating on the pool: an AFGS1 slab (a smaller job table) is never handed to an SEI build -- results stay exact
    an = [n for n in sorted(p.stem for p in T.FWCFG.glob("fgs_afgs1_*_10_420.npz"))][:6]
    acfgs = [fw().struct_from_bytes(1, T.load_fwcfg(n)[1][-1][1]) for n in an]
    arecs = [U.model_records(n) for n in an]
    aseeds = [fw().afgs1_seed(c) for c in acfgs]
    for cycle in range(3):
        ma = hip.models_from_afgs1(acfgs, stream_ptr())
        release(hip, ma)                                               # an idle AFGS1 slab, the most recent one
        ms = hip.models_from_sei(cfgs, stream_ptr())
        ma = hip.models_from_afgs1(acfgs, stream_ptr())
        grain_and_check(hip, ms, recs, seeds, pick[:4], *geo, 680 + cycle)
        grain_and_check(hip, ma, arecs, aseeds, [3, 0, 5, 1], *geo, 690 + cycle)
        release(hip, ms)
        release(hip, ma)
    torch.cuda.synchronize()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------

def spoil(cause):
    """-> (what to do to a valid message, the code the call answers with)"""
    def intervals(s, c, n, present=1):
        s.comp_model_present_flag[c] = present
        s.num_intensity_intervals[c] = n

    def ar(s, l2s):
        s.model_id = 1
        s.log2_scale_factor = l2s

    table = {
        "luma_257_intervals": (lambda s: intervals(s, 0, 257), 42),
        "cb_300_intervals": (lambda s: intervals(s, 1, 300), 42),
        "cr_65535_intervals": (lambda s: intervals(s, 2, 65535), 42),
        "ar_log2_scale_factor_0": (lambda s: ar(s, 0), 42),
        "ar_log2_scale_factor_16": (lambda s: ar(s, 16), 42),
        "ff_log2_scale_factor_1": (lambda s: setattr(s, "log2_scale_factor", 1), 9),
        "ff_log2_scale_factor_8": (lambda s: setattr(s, "log2_scale_factor", 8), 9),
        "ar_log2_scale_factor_2": (lambda s: ar(s, 2), 9),
        "ar_log2_scale_factor_9": (lambda s: ar(s, 9), 9),
    }
    return table[cause]


CAUSES = ["luma_257_intervals", "cb_300_intervals", "cr_65535_intervals", "ar_log2_scale_factor_0", "ar_log2_scale_factor_16",
          "ff_log2_scale_factor_1", "ff_log2_scale_factor_8", "ar_log2_scale_factor_2", "ar_log2_scale_factor_9"]


def raw_call(hip, arr, n, out):
    rc = hip.lib.vfgs_hip_models_from_sei(arr, n, out, stream_ptr())
    return rc, hip.lib.vfgs_hip_last_error_string().decode()


def five_messages():
    """five frequency-filtered messages with log2_scale_factor inside 2..7"""
    return (fw().FgsSei * 5)(*[s for s in (sei_of(n) for n in GROUPS[(8, 2, 2)]) if s.model_id == 0][:5])


@pytest.mark.parametrize("at", [0, 4], ids=["first", "last"])
@pytest.mark.parametrize("cause", CAUSES)
def test_refusals(hip, cause, at):
    set_format(hip, 8, 2, 2)
    hip.set_seed(31)
    arr = five_messages()
    assert all(m.model_id == 0 for m in arr)
    change, code = spoil(cause)
    change(arr[at])
    out = (C.c_void_p * 5)(*[0xdead0 + i for i in range(5)])
    stats, regs, launches = hip.model_build_stats(), hip.seed_state(), U.launches(hip)
    rc, msg = raw_call(hip, arr, 5, out)
    assert rc == code and "vfgs_hip_models_from_sei" in msg and f"message {at}:" in msg, (rc, msg)
    assert all(v is None for v in out), list(out)
    assert hip.model_build_stats() == stats and hip.seed_state() == regs and U.launches(hip) == launches


def test_42_is_examined_before_9(hip):
    set_format(hip, 8, 2, 2)
    arr = five_messages()
    spoil("ff_log2_scale_factor_8")[0](arr[0])
    spoil("luma_257_intervals")[0](arr[4])
    out = (C.c_void_p * 5)()
    rc, msg = raw_call(hip, arr, 5, out)
    assert rc == 42 and "message 4:" in msg, (rc, msg)


def test_refusals_of_the_pointers_and_the_empty_call(hip):
    set_format(hip, 8, 2, 2)
    arr = five_messages()
    out = (C.c_void_p * 2)(0xdead0, 0xdead1)
    stats = hip.model_build_stats()
    assert raw_call(hip, arr, 2, None)[0] == 41
    rc, msg = raw_call(hip, None, 2, out)
    assert rc == 41 and list(out) == [None, None], (rc, msg)
    out = (C.c_void_p * 2)(0xdead0, 0xdead1)
    assert raw_call(hip, arr, 0, out)[0] == 0 and list(out) == [0xdead0, 0xdead1]      # n == 0 is no call at all
    assert raw_call(hip, None, 0, None)[0] == 0
    assert hip.models_from_sei([]) == []
    assert hip.model_build_stats() == stats
    # what is NOT refused: more than 256 intervals in a component that is absent -- vfgs_init_sei does not look at it
    s = sei_of(GROUPS[(8, 2, 2)][0])
    s.comp_model_present_flag[2] = 0
    s.num_intensity_intervals[2] = 999
    ms = hip.models_from_sei([s], stream_ptr())
    try:
        m = captured(hip, 8, 2, 2, 0, s)
        try:
            assert hip.model_info(m) == hip.model_info(ms[0]) and hip.model_image(m) == hip.model_image(ms[0])
        finally:
            hip.model_release(m)
    finally:
        release(hip, ms)
