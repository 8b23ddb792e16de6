"""GPU (MI355X): models that CARRY a chroma mix through the two list calls with a model per picture -- vfgs_hip_models_from_afgs1_mix,
vfgs_hip_model_capture_mix, vfgs_hip_model_chroma_mix; grain_mix_kernel / grain_sp_mix_kernel with a model per frame -- through the C ABI.

Expected pictures: tests/model_mix_list_util.py (the list call's loop around tests/chroma_mix_util.py's derivation from the unchanged oracle,
per frame with that frame's records and mix).  tests/test_model_mix_cases_cpu.py has confirmed that the derivation leaves out NO sample of
any case of the table, so every byte of every plane is compared here, stride padding included."""
import numpy as np
import pytest

import chroma_mix_util as X
import model_list_util as U
import model_mix_list_util as MU
import semiplanar_util as SP
import vfgs_testlib as T
from gpu_util import DevFrame, stream_ptr
from test_gpu_frame_list import scattered
from test_gpu_semiplanar import DevSP, assert_equal
from test_gpu_semiplanar import scattered as scattered_sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    fw().afgs1_chroma_mix(False)
    h.lib.vfgs_hip_reset_state()


def fw():
    from versatilefilmgrain_amd import fw as m
    return m


def set_format(hip, spec):
    geo = T.trace_geometry(U.model_records(spec[0][0]))
    hip.lib.vfgs_hip_reset_state()
    hip.set_depth(geo[0])
    hip.set_chroma_subsampling(geo[1], geo[2])
    return geo


def build(hip, spec):
    """one model per (parameter set, kind): from the parameter set with its mix, without one (kind none), or programmed and captured (cb_only);
    the programmed state is the power-on state at the models' depth and format afterwards"""
    geo = set_format(hip, spec)
    out = []
    for name, kind in spec:
        if kind == "none":
            out += hip.models_from_afgs1([MU.parameter_set(name, kind)], stream_ptr())
        elif kind == "cb_only":
            U.program(hip, MU.records(name, kind))
            hip.set_chroma_mix(1, *MU.mix_of(kind)[0])
            out.append(hip.model_capture_mix(stream_ptr()))
            set_format(hip, spec)
        else:
            out += hip.models_from_afgs1_mix([MU.parameter_set(name, kind)], stream_ptr())
    for m, (_, kind) in zip(out, spec):
        mx = MU.mix_of(kind)
        assert [hip.model_chroma_mix(m, c) for c in (1, 2)] == [(x + (1,)) if x else (0, 0, 0, 0) for x in mx], kind
    return out, geo


def release(hip, models):
    for m in models:
        hip.model_release(m)


def state(hip):
    return (hip.chroma_mix(1), hip.chroma_mix(2), hip.seed_state(), hip.params(), [hip.luts(c) for c in range(3)])


def exact(got, want, what):
    for n, a, b in zip("YUV", got.planes(), want.planes()):
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what} plane {n}: {len(bad)} samples differ, first at {tuple(bad[0])}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}")


def run_planar(hip, handles, models, pick, frames, seeds, out_of_place, ora=None):
    """-> (frames the call left, the unseeded run's oracle)"""
    res, excluded, regs, ora = MU.expect_list(models, pick, frames, seeds, ora)
    assert excluded == 0
    src = scattered(frames, 1)
    f0 = frames[0]
    hs = [handles[k] for k in pick]
    if out_of_place:
        dst = [DevFrame(_filled(f0, 77 + i)) for i in range(len(frames))]
        before = [d.download() for d in dst]
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], hs, seeds, f0.width, f0.height, f0.stride, f0.cstride, stream_ptr())
        rows, cols = f0.height, (f0.width + 15) // 16 * 16
        crows, ccols = (f0.height + f0.suby - 1) // f0.suby, cols // f0.subx
        got = []
        for i, (s, d, (want, _), f, b) in enumerate(zip(src, dst, res, frames, before)):
            e = b.copy()
            e.Y[:rows, :cols] = want.Y[:rows, :cols]
            e.U[:crows, :ccols] = want.U[:crows, :ccols]
            e.V[:crows, :ccols] = want.V[:crows, :ccols]
            g = d.download()
            exact(g, e, f"destination {i}")          # what is written, and the padding as it was
            exact(s.download(), f, f"source {i}")
            got.append(g)
    else:
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in src], None, hs, seeds, f0.width, f0.height, f0.stride, f0.cstride, stream_ptr())
        got = [d.download() for d in src]
        for i, (g, (want, _)) in enumerate(zip(got, res)):
            exact(g, want, f"frame {i}")
    assert hip.seed_state() == regs
    return got, ora


def _filled(f0, seed):
    g = f0.copy()
    rng = np.random.default_rng(seed)
    for p in g.planes():
        p[...] = rng.integers(0, 1 << (16 if g.depth > 8 else 8), p.shape).astype(g.dtype)
    return g


# ---- planar ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("out_of_place", [True, False], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("cid", sorted(MU.PLANAR))
def test_planar(hip, cid, out_of_place, seeded):
    """models A B A C B -- A and B carry different mixes, C none: runs [A B A], [C], [B]; three launches out of place, five in place (a run
    under a mix over shared luma bytes is two)"""
    spec, w, h = MU.PLANAR[cid]
    handles, (depth, sx, sy) = build(hip, spec)
    try:
        st = state(hip)
        models = MU.case_models(spec)
        frames = MU.case_frames(spec, w, h, len(MU.PICK), 5)
        seeds = MU.fresh_seeds(len(MU.PICK), 1) if seeded else None
        hip.set_seed(1234)
        ora = None
        if not seeded:
            ora = T.OracleHW()
            ora.set_seed(1234)
        n0 = U.launches(hip)
        run_planar(hip, handles, models, MU.PICK, frames, seeds, out_of_place, ora)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == (3 if out_of_place else 5), info
        assert info["kernel"] == f"grain_mix_kernel<{depth},{sx},{sy},false,false>" and info["nframes"] == 1 and info["listed"] == 1, info
        after = state(hip)
        assert after[0] == st[0] and after[1] == st[1] and after[3:] == st[3:]       # the programmed state: mix, parameters, LUTs
        # the run without a mix is grain_ml_kernel's, as before
        f1 = frames[3:4]
        hip.add_grain_frame_list_models_dev([DevFrame(f1[0]).ptrs()], None, [handles[2]], [5], w, h, f1[0].stride, f1[0].cstride, stream_ptr())
        assert hip.last_launch_info()["kernel"].startswith("grain_ml_kernel<"), hip.last_launch_info()
    finally:
        release(hip, handles)


@pytest.mark.parametrize("cid", ["8_444_183x33", "10_422_200x48"])
def test_clip_bounds_are_the_frames_models(hip, cid):
    """The case table's content sits in the middle of the range, where no clip bound binds.  Here luma covers the WHOLE range, and the frames
    of ONE launch alternate between a restricted-range model (what the recorded parameter set says) and a full-range one (both carry a
    mix): a kernel that took lo2 / hi2 from the launch's first frame instead of the frame's record would leave luma below 16 << (depth - 8)
    in the restricted frames, or lift it in the others.  Luma is compared everywhere; chroma where the derivation can state it (an index on a clip bound is left out, as in
    tests/test_gpu_chroma_mix.py) -- the 0-excluded condition is the case table's, not this test's."""
    spec, w, h = MU.PLANAR[cid]
    spec = [s for s in spec if "full" in MU.flags(s[1])] + [(spec[0][0], "luma_only")]      # model 0: the full range, model 1: the restricted; frame 0 is restricted
    handles, (depth, sx, sy) = build(hip, spec)
    try:
        pick = [1, 0, 1, 0]
        frames = X.ranged_frames(w, h, depth, sx, sy, len(pick), 21, lo=0.0, hi=1.0, clo=MU.CONTENT["clo"], chi=MU.CONTENT["chi"])
        seeds = MU.fresh_seeds(len(pick), 4)
        res, _excluded, regs, _ = MU.expect_list(MU.case_models(spec), pick, frames, seeds)
        low = 16 << (depth - 8)
        for k, (want, _), f in zip(pick, res, frames):
            # (the expectation does tell the two ranges apart: the oracle lifted the restricted frames' dark luma to the bound, and only theirs)
            assert (f.Y[:h, :w] < low).any() and ((want.Y[:h, :w] < low).any() == (k == 0))
        src = scattered(frames, 3)
        f0 = frames[0]
        dst = [DevFrame(f.copy()) for f in frames]
        n0 = U.launches(hip)
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], [handles[k] for k in pick], seeds, w, h, f0.stride, f0.cstride, stream_ptr())
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 1 and info["nframes"] == len(pick) and info["kernel"] == f"grain_mix_kernel<{depth},{sx},{sy},false,false>", info
        for i, (d, (want, masks)) in enumerate(zip(dst, res)):
            g = d.download()
            assert np.array_equal(g.Y, want.Y), f"frame {i}: luma"
            assert X.mismatches(g, want, masks) == 0, f"frame {i}"
        assert hip.seed_state() == regs
    finally:
        release(hip, handles)


def test_the_list_equals_the_definition_on_the_gpu(hip):
    """per frame: vfgs_hip_afgs1_chroma_mix(1); vfgs_init_afgs1; vfgs_set_seed; a one-frame copy list -- the planes must be identical; the
    programmed state, the mix and the registers are then restored and compared"""
    spec, w, h = MU.PLANAR["10_420_1047x40"]
    spec = [s for s in spec if s[1] != "none"]
    handles, _ = build(hip, spec)
    try:
        pick = [0, 1, 0, 1, 1]
        frames = MU.case_frames(spec, w, h, len(pick), 6)
        seeds = MU.fresh_seeds(len(pick), 2)
        f0 = frames[0]
        st = state(hip)
        src = scattered(frames, 2)
        dst = [DevFrame(_filled(f0, 50)) for _ in frames]
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], [handles[k] for k in pick], seeds, w, h, f0.stride, f0.cstride, stream_ptr())
        got = [d.download() for d in dst]
        regs = hip.seed_state()
        assert state(hip)[:2] == st[:2] and state(hip)[3:] == st[3:]
        try:
            fw().afgs1_chroma_mix(True)
            for i, k in enumerate(pick):
                fw().init_afgs1(MU.parameter_set(*spec[k]))
                hip.set_seed(seeds[i])
                d = DevFrame(_filled(f0, 50))
                hip.add_grain_frame_list_copy_dev([src[i].ptrs()], [d.ptrs()], w, h, f0.stride, f0.cstride, stream_ptr())
                exact(got[i], d.download(), f"frame {i}")
            assert hip.seed_state() == regs
        finally:
            fw().afgs1_chroma_mix(False)
    finally:
        release(hip, handles)


# ---- semi-planar -----------------------------------------------------------------------------------------------------------------

def run_sp(hip, handles, models, pick, planar_frames, shift, seeds, out_of_place, ora=None):
    sps = [SP.to_semiplanar(f, shift, 300 + i if shift else None) for i, f in enumerate(planar_frames)]
    res, excluded, regs, ora = MU.expect_list(models, pick, [SP.to_planar(s) for s in sps], seeds, ora)
    assert excluded == 0
    want = [MU.to_sp_expectation(s, w, m)[0] for s, (w, m) in zip(sps, res)]
    src = scattered_sp(sps, 3)
    f0 = sps[0]
    hs = [handles[k] for k in pick]
    if out_of_place:
        fill = SP.garbage_sp_frame(f0.width, f0.height, f0.depth, f0.suby, f0.shift, 999)
        dst = [DevSP(fill) for _ in sps]
        hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], hs, seeds, f0.width, f0.height, f0.stride, f0.uv_stride, shift, stream_ptr())
        rows, crows, cols = SP.written_region(f0)
        for i, (s, d, w, f) in enumerate(zip(src, dst, want, sps)):
            e = fill.copy()
            e.Y[:rows, :cols] = w.Y[:rows, :cols]
            e.UV[:crows, :cols] = w.UV[:crows, :cols]
            assert_equal(d.download(), e, f"destination {i}")
            assert_equal(s.download(), f, f"source {i}")
    else:
        hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in src], None, hs, seeds, f0.width, f0.height, f0.stride, f0.uv_stride, shift, stream_ptr())
        for i, (d, w) in enumerate(zip(src, want)):
            assert_equal(d.download(), w, f"frame {i}")
    assert hip.seed_state() == regs
    return ora


@pytest.mark.parametrize("seeded", [False, True], ids=["one_sequence", "seeded"])
@pytest.mark.parametrize("out_of_place", [True, False], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("cid", sorted(MU.SEMIPLANAR))
def test_semiplanar(hip, cid, out_of_place, seeded):
    """P010 (samples 6 bits up, random low bits), NV12, P210; A B A C B: one launch per run out of place, two per run under a mix in place"""
    spec, w, h, shift = MU.SEMIPLANAR[cid]
    handles, (depth, _sx, sy) = build(hip, spec)
    try:
        st = state(hip)
        frames = MU.case_frames(spec, w, h, len(MU.PICK), 7)
        seeds = MU.fresh_seeds(len(MU.PICK), 3) if seeded else None
        hip.set_seed(4321)
        ora = None
        if not seeded:
            ora = T.OracleHW()
            ora.set_seed(4321)
        n0 = U.launches(hip)
        run_sp(hip, handles, MU.case_models(spec), MU.PICK, frames, shift, seeds, out_of_place, ora)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == (3 if out_of_place else 5), info
        assert info["kernel"] == f"grain_sp_mix_kernel<{depth},{sy}>" and info["listed"] == 1, info
        after = state(hip)
        assert after[:2] == st[:2] and after[3:] == st[3:]
    finally:
        release(hip, handles)


# ---- more frames than a launch holds ---------------------------------------------------------------------------------------------------

def test_34_frames_cross_the_limit_of_a_launch(hip):
    """34 frames of 136 x 32 (MU.CYCLE_SIZE), four mixes cycling: 32 + 2, two launches out of place -- a change of the VALUES of the mix starts none"""
    handles, (depth, sx, sy) = build(hip, MU.CYCLE)
    try:
        pick = [i % len(MU.CYCLE) for i in range(34)]
        frames = MU.case_frames(MU.CYCLE, *MU.CYCLE_SIZE, 34, 5)
        n0 = U.launches(hip)
        run_planar(hip, handles, MU.case_models(MU.CYCLE), pick, frames, MU.fresh_seeds(34, 1), True)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == 2 and info["nframes"] == 2 and info["kernel"].startswith("grain_mix_kernel<"), info
    finally:
        release(hip, handles)


def test_two_calls_inside_an_overlap_region(hip):
    spec, _w, _h, shift = MU.SEMIPLANAR["p010_1047x40"]
    handles, _ = build(hip, spec[:2])
    try:
        import torch
        models = MU.case_models(spec[:2])
        a, b = MU.case_frames(spec, 520, 70, 4, 150), MU.case_frames(spec, 520, 70, 3, 160)
        spa, spb = [SP.to_semiplanar(f, shift) for f in a], [SP.to_semiplanar(f, shift) for f in b]
        pa, pb = [0, 1, 1, 0], [1, 0, 1]
        ora = T.OracleHW()
        hip.set_seed(99)
        ora.set_seed(99)
        ra, ex_a, _, ora = MU.expect_list(models, pa, a, None, ora)
        rb, ex_b, regs, ora = MU.expect_list(models, pb, b, None, ora)
        assert ex_a == 0 and ex_b == 0
        da, db = scattered_sp(spa, 4), scattered_sp(spb, 5)
        st = stream_ptr()
        f0 = spa[0]
        hip.overlap_begin(st)
        hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in da], None, [handles[k] for k in pa], None, 520, 70, f0.stride, f0.uv_stride, shift, st)
        hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in db], None, [handles[k] for k in pb], None, 520, 70, f0.stride, f0.uv_stride, shift, st)
        hip.overlap_end(st)
        torch.cuda.synchronize()
        for sps, dev, res in ((spa, da, ra), (spb, db, rb)):
            for i, (s, d, (w, m)) in enumerate(zip(sps, dev, res)):
                assert_equal(d.download(), MU.to_sp_expectation(s, w, m)[0], f"frame {i}")
        assert hip.seed_state() == regs
    finally:
        release(hip, handles)


def test_two_frame_fronts(hip):
    """three P010 frames of 8192 x 1366 (tests/test_gpu_sp_model_list.py::test_two_frame_fronts), models A B A: frames 2m and 2m + 1 are
    swept together, each with its own model and its own mix"""
    spec, _w, _h, shift = MU.SEMIPLANAR["p010_1047x40"]
    handles, _ = build(hip, spec[:2])
    try:
        frames = MU.case_frames(spec, 8192, 1366, 3, 21)
        run_sp(hip, handles, MU.case_models(spec[:2]), [0, 1, 0], frames, shift, MU.fresh_seeds(3, 4), True)
        info = hip.last_launch_info()
        assert info["frames_per_front"] == 2 and info["nframes"] == 3 and info["kernel"].startswith("grain_sp_mix_kernel<"), info
    finally:
        release(hip, handles)


# ---- records ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", sorted(MU.PLANAR))
def test_records_agree_with_the_capture_path(hip, cid):
    """vfgs_hip_models_from_afgs1_mix against switch on + vfgs_init_afgs1 + vfgs_hip_model_capture_mix: record and image byte for byte, the mix
    read back equal; vfgs_hip_models_from_afgs1 and vfgs_hip_model_capture on the same inputs still give records without a mix"""
    spec, _w, _h = MU.PLANAR[cid]
    geo = set_format(hip, spec)
    kinds = ("luma_only", "tbl", "cfl", "neutral")
    cfgs = [MU.parameter_set(spec[0][0], k) for k in kinds]
    st = state(hip)
    built = hip.models_from_afgs1_mix(cfgs, stream_ptr())
    plain = hip.models_from_afgs1(cfgs, stream_ptr())
    assert state(hip) == st
    made = []
    try:
        fw().afgs1_chroma_mix(True)
        for cfg, b, p, kind in zip(cfgs, built, plain, kinds):
            set_format(hip, spec)
            fw().init_afgs1(cfg)
            mixes = (hip.chroma_mix(1), hip.chroma_mix(2))
            assert mixes == tuple(x + (1,) for x in MU.mix_of(kind))
            before = state(hip)
            c = hip.model_capture_mix(stream_ptr())
            d = hip.model_capture(stream_ptr())
            made += [c, d]
            assert state(hip) == before
            img_b, img_c, img_p, img_d = (hip.model_image(m) for m in (b, c, p, d))
            assert img_b == img_c and img_p == img_d
            assert (hip.model_chroma_mix(b, 1), hip.model_chroma_mix(b, 2)) == mixes == (hip.model_chroma_mix(c, 1), hip.model_chroma_mix(c, 2))
            assert img_p[20:32] == bytes(12) and img_b[20:24] == (1).to_bytes(4, "little") and img_b[:20] == img_p[:20] and img_b[32:] == img_p[32:]
            assert hip.model_chroma_mix(p, 1) == hip.model_chroma_mix(d, 2) == (0, 0, 0, 0)
            assert hip.model_info(b) == hip.model_info(c)
        # no mix active: capture_mix is capture
        hip.clear_chroma_mix()
        e, f = hip.model_capture_mix(stream_ptr()), hip.model_capture(stream_ptr())
        made += [e, f]
        assert hip.model_image(e) == hip.model_image(f) and hip.model_chroma_mix(e, 1) == (0, 0, 0, 0)
    finally:
        fw().afgs1_chroma_mix(False)
        release(hip, built + plain + made)
    assert geo == T.trace_geometry(U.model_records(spec[0][0]))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def code_of(err):
    return int(str(err).split("error ")[1].split(":")[0])


def refused(hip, code, fn):
    from versatilefilmgrain_amd.hw import VfgsHipError
    st, n0, stats = state(hip), U.launches(hip), hip.model_build_stats()
    with pytest.raises(VfgsHipError) as e:
        fn()
    assert code_of(e.value) ==code, e.value
    assert state(hip) == st and U.launches(hip) == n0 and hip.model_build_stats() == stats


def test_refusals_change_nothing(hip):
    from versatilefilmgrain_amd.hw import VfgsHipError
    spec, w, h = MU.PLANAR["10_420_1047x40"]
    handles, _ = build(hip, spec)
    try:
        frames = MU.case_frames(spec, w, h, 2, 8)
        dev = scattered(frames, 0)
        f0 = frames[0]
        call = lambda: hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev], None, handles[:2], [1, 2], w, h, f0.stride, f0.cstride, stream_ptr())
        # a PROGRAMMED mix is active: 41, as before
        hip.set_chroma_mix(1, 10, 20, 0)
        refused(hip, 41, call)
        sps = [DevSP(SP.to_semiplanar(f, 6)) for f in frames]
        s0 = sps[0].sp
        refused(hip, 41, lambda: hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in sps], None, handles[:2], None, w, h, s0.stride, s0.uv_stride, 6, stream_ptr()))
        for d, f in zip(dev, frames):
            exact(d.download(), f, "a refused call wrote")
        hip.clear_chroma_mix()
        call()
        # a model that carries a mix, made at another depth: 41, as for any model
        hip.set_depth(8)
        refused(hip, 41, call)
        # ... or for another chroma format
        hip.set_depth(10)
        hip.set_chroma_subsampling(2, 1)
        f422 = X.ranged_frames(w, h, 10, 2, 1, 2, 9, **MU.CONTENT)      # (frames of that format: the list checks come first)
        dev422, sps422 = scattered(f422, 0), [DevSP(SP.to_semiplanar(f, 6)) for f in f422]
        s1 = sps422[0].sp
        refused(hip, 41, lambda: hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev422], None, handles[:2], [1, 2], w, h, f422[0].stride, f422[0].cstride, stream_ptr()))
        refused(hip, 41, lambda: hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in sps422], None, handles[:2], None, w, h, s1.stride, s1.uv_stride, 6, stream_ptr()))
        for d, f in zip(dev422, f422):
            exact(d.download(), f, "a refused call wrote")
        hip.set_chroma_subsampling(2, 2)
        call()
    finally:
        release(hip, handles)
    # capture_mix with a general-form model under a mix
    U.program(hip, U.model_records("fgs_sei_10_420"))
    hip.set_chroma_mix(1, 10, 20, 0)
    refused(hip, 38, lambda: hip.model_capture_mix(stream_ptr()))
    hip.model_release(hip.model_capture(stream_ptr()))      # (capture itself drops the mix and serves)
    # ... and at depth 12
    import test_gpu_depth12 as D
    U.program(hip, D.records12("fgs_afgs1_test1_10_420"))
    hip.set_chroma_mix(2, 10, 20, 0)
    refused(hip, 38, lambda: hip.model_capture_mix(stream_ptr()))
    hip.clear_chroma_mix()
    cfg = MU.parameter_set("fgs_afgs1_test1_10_420", "tbl")
    refused(hip, 38, lambda: hip.models_from_afgs1_mix([cfg, cfg], stream_ptr()))
    release(hip, hip.models_from_afgs1([cfg], stream_ptr()))
    # an 8-bit set whose scaling function falls back to the general form: 38, naming the index
    hip.lib.vfgs_hip_reset_state()
    hot = MU.parameter_set("fgs_afgs1_test1_8_420", "tbl")
    hot.point_y_scaling[1] = 255
    hot.grain_scaling = 11
    ok = MU.parameter_set("fgs_afgs1_test1_8_420", "tbl")
    with pytest.raises(VfgsHipError) as e:
        hip.models_from_afgs1_mix([ok, hot], stream_ptr())
    assert code_of(e.value) ==38 and "parameter set 1:" in str(e.value), e.value
    plain = hip.models_from_afgs1([hot], stream_ptr())
    assert hip.model_info(plain[0])["one_y"] == 0
    release(hip, plain)
    # a mix field the setter would refuse: 42
    bad = MU.parameter_set("fgs_afgs1_test1_8_420", "tbl")
    bad.cr_offset = 512
    with pytest.raises(VfgsHipError) as e:
        hip.models_from_afgs1_mix([ok, ok, bad], stream_ptr())
    assert code_of(e.value) ==42 and "parameter set 2:" in str(e.value), e.value
    release(hip, hip.models_from_afgs1([bad], stream_ptr()))
    # the read-back: a dead handle 41, a bad component 37
    m = hip.models_from_afgs1_mix([ok], stream_ptr())[0]
    with pytest.raises(VfgsHipError) as e:
        hip.model_chroma_mix(m, 3)
    assert code_of(e.value) ==37
    hip.model_release(m)
    for dead in (m, None):
        with pytest.raises(VfgsHipError) as e:
            hip.model_chroma_mix(dead, 1)
        assert code_of(e.value) ==41
