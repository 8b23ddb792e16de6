"""GPU (MI355X): every device path of the firmware layer over its parameter space, against the firmware oracle (oracle/vfgs_fw_oracle.c
through tests/fw_oracle_util.py; pinned on the CPU by tests/test_fw_oracle_c_cpu.py) -- an independent truth, where the comparisons of
tests/test_gpu_models_from_*.py with the capture path are GPU code against GPU code.  The lists are those of tests/fw_space.py; what they
hold is asserted without a GPU in tests/test_fw_space_cpu.py.  Every comparison is exact.

 1. fw_ff_kernel / fw_ar_kernel over the job space (vfgs_hip_generate_patterns, 16 jobs per call, 4:2:0);
 2. fw_commit_chroma: the chroma bank copy at 4:2:2, 4:4:4 and 4:4:0 with the tail of the last luma pattern;
 3. vfgs_init_sei / vfgs_init_afgs1 on 12 geometries: the banks, and a frame against the oracle hardware layer programmed with the
    firmware oracle's records;
 4. fw_models_kernel / fw_sei_build_kernel (vfgs_hip_models_from_afgs1 / _sei) on the same geometries: a picture per model in one
    models call, planar and P010.

Planar frames are 264 x 88 (17 blocks, the last ragged, by 6 block rows, the last ragged) with garbage over the whole container range, so
every LUT entry is exercised.  Depth 12 has no reference: the firmware's records do not depend on the depth and the oracle hardware layer
is pinned there."""
import numpy as np
import pytest

import fw_oracle_util as O
import fw_space as S
import model_list_util as U
import semiplanar_util as SP
import sp_model_list_util as SU
import vfgs_testlib as T
from gpu_util import DevFrame, stream_ptr
from test_gpu_frame_list import garbage_frame, scattered

pytestmark = pytest.mark.gpu

W, H = 264, 88
GEO_IDS = ["%d_%d%d" % g for g in S.GEOMETRIES]


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


def set_format(hip, depth, sx, sy, legal=0):
    hip.lib.vfgs_hip_reset_state()
    hip.set_depth(depth)
    hip.set_chroma_subsampling(sx, sy)
    hip.set_legal_range(legal)


def bank_region(chroma, slot, sx=2, sy=2):
    """the region of a slot the hardware layer reads (vfgs_hw.c:314-325)"""
    p = np.frombuffer(fw().get_pattern(chroma, slot), dtype=np.int8).reshape(64, 64)
    return p[:64 // sy, :64 // sx] if chroma else p


# ---- 1. the pattern kernels over the job space ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["frequency_filtered", "auto_regressive"])
def test_pattern_kernels_over_the_job_space(hip, kind):
    jobs = S.ff_jobs() if kind == "frequency_filtered" else S.ar_jobs()
    set_format(hip, 8, 2, 2)
    done = 0
    for call in S.calls_of(jobs):
        want = [np.frombuffer(O.job_pattern(j), dtype=np.int8).reshape((32, 32) if j.chroma else (64, 64)) for j in call]
        fw().generate_patterns(call)
        for j, w in zip(call, want):
            got = bank_region(j.chroma, j.index)
            if not np.array_equal(got, w):
                bad = np.argwhere(got != w)
                raise AssertionError(f"{kind} bank {j.chroma} slot {j.index} seed {j.seed_index} fh {j.fh} fv {j.fv} scale {j.scale} shift {j.shift} "
                                     f"taps {list(j.coef)}: {len(bad)} samples differ, first at row {bad[0][0]} column {bad[0][1]}: "
                                     f"{got[tuple(bad[0])]} != {w[tuple(bad[0])]}")
            done += 1
    assert done == len(jobs)


@pytest.mark.parametrize("seed_index", [-1, 256])
def test_a_seed_index_outside_the_table_is_refused(hip, seed_index):
    """the seed table has 256 entries: error 32, nothing queued, the banks as they were"""
    from versatilefilmgrain_amd import hw
    set_format(hip, 8, 2, 2)
    good = S._job(0, 0, 255, 3, 3)
    good.index = 2
    fw().generate_patterns([good])
    before = fw().get_pattern(0, 2)
    assert before == O.job_pattern(good)
    bad = S._job(0, 0, seed_index, 9, 9)
    bad.index = 2
    with pytest.raises(hw.VfgsHipError, match="error 32"):
        fw().generate_patterns([good, bad])
    assert fw().get_pattern(0, 2) == before


# ---- 2. the chroma bank copy by format -----------------------------------------------------------------------------------------------

def _some_jobs(rng, kind, chroma, slots):
    out = []
    for slot in slots:
        if kind == 0:
            j = S._job(0, chroma, int(rng.integers(0, 3)), int(rng.integers(1, 16)), int(rng.integers(1, 16)))
        else:
            lag = int(rng.integers(1, 4))
            taps = np.zeros((4, 7), dtype=np.int64)
            for r, c in S._causal(lag):
                taps[3 + r, 3 + c] = int(rng.integers(-60, 61))
            j = S._job(1, chroma, int(rng.integers(0, 3)), scale=int(rng.integers(6, 10)), shift=int(rng.integers(1, 4)), taps=taps)
        j.index = slot
        out.append(j)
    return out


@pytest.mark.parametrize("kind", [0, 1], ids=["frequency_filtered", "auto_regressive"])
@pytest.mark.parametrize("fmt", ["422", "444", "440"])
def test_chroma_bank_copy_by_format(hip, fmt, kind):
    sx, sy = S.FORMATS[fmt]
    rng = np.random.default_rng(50 + 10 * kind + sx + 2 * sy)
    set_format(hip, 10, sx, sy)
    model = T.BankModel()
    model.set_chroma_subsampling(sx, sy)

    def run(luma, chroma, what):
        last = None
        for j in luma:
            last = O.job_pattern(j)
            model.set_luma_pattern(j.index, last)
        for j in chroma:
            model.set_chroma_pattern(j.index, O.job_payload(j, last))
        fw().generate_patterns(luma + chroma)
        for slot in range(8):
            want = model.chroma.get(slot, np.zeros((64 // sy, 64 // sx), np.int8))
            got = bank_region(1, slot, sx, sy)
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)
                raise AssertionError(f"{what}: chroma slot {slot}: {len(bad)} samples differ, first at row {bad[0][0]} column {bad[0][1]}")
        for slot, want in model.luma.items():
            assert np.array_equal(bank_region(0, slot), want), (what, slot)

    # the last luma job sits on a lower slot than earlier ones, and not on slot 0: the tail is the LAST job's pattern
    luma = _some_jobs(rng, kind, 0, [5, 0, 3, 1])
    run(luma, _some_jobs(rng, kind, 1, [2, 7, 0, 4]), "luma then chroma")
    assert len({O.job_pattern(j)[1024:] for j in luma}) == 4          # (the four tails differ, so the wrong one would show)
    run([], _some_jobs(rng, kind, 1, [1, 2, 6]), "chroma only, luma patterns in the banks")
    hip.lib.vfgs_hip_reset_state()
    hip.set_depth(10)
    hip.set_chroma_subsampling(sx, sy)
    model.luma.clear()
    model.chroma.clear()
    run([], _some_jobs(rng, kind, 1, [0, 3, 7]), "chroma only, after a reset")


# ---- 3. vfgs_init_sei / vfgs_init_afgs1 over the space ---------------------------------------------------------------------------------

def program_of(cfg, depth, sx, sy, legal=0):
    """the firmware oracle's records behind the state the format calls leave (the power-on range first, as model_list_util.model_records)"""
    return [(T.OP_LEGAL_RANGE, legal, 0, b""), (T.OP_DEPTH, depth, 0, b""), (T.OP_CHROMA_SUBSAMPLING, sx, sy, b"")] + O.program(cfg)


@pytest.mark.parametrize("geo", S.GEOMETRIES, ids=GEO_IDS)
def test_init_over_the_space(hip, geo):
    depth, sx, sy = geo
    fw().afgs1_chroma_mix(False)
    cfgs = S.sei_init_list(*geo) + S.afgs1_init_list(*geo)
    assert len(cfgs) == 40
    seeds = [int(v) for v in np.random.default_rng(depth + sx + sy).integers(1, 1 << 32, len(cfgs))]
    for i, cfg in enumerate(cfgs):
        afgs1 = hasattr(cfg, "grain_seed")
        rec = program_of(cfg, depth, sx, sy)
        if not afgs1:
            rec.append((T.OP_SEED, seeds[i], 0, b""))
        set_format(hip, depth, sx, sy)
        fw().init(cfg)
        if not afgs1:
            hip.set_seed(seeds[i])
        banks = T.BankModel()
        T.replay(banks, rec)
        for slot, want in banks.luma.items():
            assert np.array_equal(bank_region(0, slot), want), (i, "luma", slot)
        for slot, want in banks.chroma.items():
            assert np.array_equal(bank_region(1, slot, sx, sy), want), (i, "chroma", slot)
        ora = T.OracleHW()
        T.replay(ora, rec)
        f = garbage_frame(W, H, depth, sx, sy, 1000 + i)
        want = f.copy()
        ora.add_grain_frame(want)
        d = DevFrame(f)
        hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
        assert d.download().equal_all(want), (i, "afgs1" if afgs1 else "sei")
        assert hip.seed_state() == ora.seed_state(), i


# ---- 4. both builders against the oracle -----------------------------------------------------------------------------------------------

def afgs1_seed(a):
    return a.grain_seed | (a.grain_seed << 16)         # vfgs_fw.c:672


def built_models(hip, kind, geo, legal):
    """-> (models, their programs, a seed per model)"""
    depth, sx, sy = geo
    if kind == "afgs1":
        cfgs = S.afgs1_build_list(*geo)
        set_format(hip, depth, sx, sy)
        models = hip.models_from_afgs1(cfgs, stream_ptr())
        seeds = [afgs1_seed(c) for c in cfgs]
        recs = [program_of(c, depth, sx, sy) for c in cfgs]
    else:
        cfgs = S.sei_build_list(*geo)
        set_format(hip, depth, sx, sy, legal)
        models = hip.models_from_sei(cfgs, stream_ptr())
        seeds = [int(v) for v in np.random.default_rng(depth + sx + sy).integers(1, 1 << 32, len(cfgs))]
        recs = [program_of(c, depth, sx, sy, legal) for c in cfgs]
    assert len(cfgs) == 40 > hip.model_build_stats()["models_per_launch"]          # two chunks
    return models, recs, seeds


def release(hip, models):
    for m in models:
        if m:
            hip.model_release(m)


@pytest.mark.parametrize("kind", ["afgs1", "sei"])
@pytest.mark.parametrize("geo", S.GEOMETRIES, ids=GEO_IDS)
def test_both_builders_against_the_oracle(hip, geo, kind):
    depth, sx, sy = geo
    legal = 1 if (sx, sy) in ((2, 1), (1, 2)) else 0          # (an SEI carries no range: the call works at the programmed one)
    models, recs, seeds = built_models(hip, kind, geo, legal)
    try:
        assert len(models) == 40 and all(models) and len(set(models)) == 40
        pick = [int(k) for k in np.random.default_rng(depth + sx + sy).permutation(40)]
        frames = [garbage_frame(W, H, depth, sx, sy, 2000 + i) for i in range(40)]
        sd = [seeds[k] for k in pick]
        want, regs = U.expect_seeded(recs, pick, frames, sd)
        dev = scattered(frames, 3)
        f0 = frames[0]
        hip.add_grain_frame_list_models_dev([d.ptrs() for d in dev], None, [models[k] for k in pick], sd, W, H, f0.stride, f0.cstride, stream_ptr())
        for i, (d, w) in enumerate(zip(dev, want)):
            assert d.download().equal_all(w), (i, pick[i])
        assert hip.seed_state() == regs
    finally:
        release(hip, models)


@pytest.mark.parametrize("kind", ["afgs1", "sei"])
def test_both_builders_on_p010_surfaces(hip, kind):
    from test_gpu_semiplanar import assert_equal, scattered as sp_scattered
    geo = (10, 2, 2)
    models, recs, seeds = built_models(hip, kind, geo, 0)
    try:
        assert len(models) == 40 and all(models)
        pick = [int(k) for k in np.random.default_rng(9).permutation(40)]
        sd = [seeds[k] for k in pick]
        frames = [SP.garbage_sp_frame(1032, 90, 10, 2, 6, 3000 + i) for i in range(40)]
        want, regs = SU.expect_seeded(recs, pick, frames, sd, 6)
        dev = sp_scattered(frames, 5)
        f0 = frames[0]
        hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in dev], None, [models[k] for k in pick], sd, f0.width, f0.height,
                                               f0.stride, f0.uv_stride, 6, stream_ptr())
        for i, (d, w) in enumerate(zip(dev, want)):
            assert_equal(d.download(), w, f"frame {i} (model {pick[i]})")
        assert hip.seed_state() == regs
    finally:
        release(hip, models)
