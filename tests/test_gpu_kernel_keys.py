"""GPU (MI355X): every kernel key launched once against the oracle -- a case per line of tests/golden/kernel_keys.txt (the output of
tests/kernel_keys/kernel_keys.cpp, held to the table and to the code objects by tests/test_kernel_keys_cpu.py), 326 in all.

Every key is a template instantiation of its own, with its own `if constexpr` branches over depth, CSUBX / CSUBY, OUT8, ONEY, ONEC, WIDE and
PERSIST: a fault in one combination shows only when that combination is launched.  tests/kernel_key_cases.py derives from the key's name the
program (tests/model_programs.py), the public entry point, the shape and the content that ask the dispatcher for exactly that kernel;
tests/test_kernel_key_cases_cpu.py checks that table on the oracle alone (coverage, forms, visible grain, the mix's caps).

A case resets the state, programs the model, runs its launches (in-range content; garbage as well unless the key is persistent or under the
mix) and asserts
* from last_launch_info(): the kernel's name and LDS bytes as the fixture has them, depth / csubx / csuby / out8 / one_y / one_c as the key
  says, parts_per_row > 1 exactly for the wide keys, persistent luma workgroups exactly for the persistent ones;
* every byte of every plane or container of every frame against the expectation of the existing helpers (T.OracleHW replaying the program):
  stride padding, the destination's fill beyond the written region and the untouched sources of the out-of-place entries included;
* the four seed registers against the oracle's.
The mix families compare under the masks of the derivation, whose share of left-out samples stays within kernel_key_cases.MIX_CAP.
A key in kernel_key_cases.UNREACHABLE (none today) must still give the oracle's bytes, through a DIFFERENT kernel of the fixture."""
import pytest

import chroma_mix_util as X
import kernel_key_cases as K
import model_list_util as U
import model_program_cases as C
import model_programs as MP
import semiplanar_mix_util as M
import vfgs_testlib as T
from test_gpu_model_programs import assert_equal, narrowed, run_copy8_dev, run_frames_dev, written

pytestmark = pytest.mark.gpu

FIXTURE = K.fixture()
NAMES = frozenset(n for n, _ in FIXTURE)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.clear_chroma_mix()
    h.lib.vfgs_hip_reset_state()


def program(hip, rec, mix):
    hip.lib.vfgs_hip_reset_state()
    hip.clear_chroma_mix()
    T.replay(hip, rec)
    for c, m in enumerate(mix or (), 1):
        if m is not None:
            hip.set_chroma_mix(c, *m)


def compare_planar(got, want, masks, what):
    """whole buffers; under a mix through the masks of the derivation"""
    for i, (g, w) in enumerate(zip(got, want)):
        if masks is None:
            assert_equal(g, w, f"{what}: frame {i}")
        else:
            n = X.mismatches(g, w, masks[i])
            assert n == 0, f"{what}: frame {i}: {n} samples differ from the expectation"


def run_planar(hip, case, rec, variant):
    """rw and mix: add_grain_frame_dev frame by frame, add_grain_frames_dev, add_grain_copy8_dev"""
    from gpu_util import DevFrame, stream_ptr
    frames = K.planar_frames(case, variant)
    if case.mix:
        res, excluded, processed, ora = K.mix_expectation(case)
        assert excluded / processed <= K.MIX_CAP, (excluded, processed)
        want, masks = [w for w, _ in res], [m for _, m in res]
    else:
        (want, ora), masks = K.grained(rec, frames), None
    program(hip, rec, case.mix)
    if case.entry == "add_grain_frame_dev":
        got = []
        for f in frames:
            d = DevFrame(f)
            hip.add_grain_frame_dev(*d.ptrs(), f.width, f.height, f.stride, f.cstride, stream_ptr())
            got.append(d.download())
    elif case.entry == "add_grain_frames_dev":
        got = run_frames_dev(hip, frames)
    else:
        got, fill = run_copy8_dev(hip, frames)           # (asserts that the sources stay)
        want = [written(narrowed(w), f) for w, f in zip(want, fill)]
    compare_planar(got, want, masks, f"{case.entry} {variant}")
    assert hip.seed_state() == ora.seed_state()
    return 1 if case.entry == "add_grain_frame_dev" else len(frames)


def run_models(hip, case, rec, variant):
    """ml and spml: the program captured as a model, a list whose every frame names it, in place, one seed sequence"""
    semiplanar = case.key.family == "spml"
    if semiplanar:
        from test_gpu_sp_model_list import Models, run
        frames = K.sp_frames(case, variant)
    else:
        from test_gpu_model_list import Models, run
        frames = K.planar_frames(case, variant)
    ms = Models(hip, [case.program])
    try:
        assert ms.recs[0] == rec
        n0 = U.launches(hip)
        run(hip, ms, [0] * len(frames), frames, None, shuffle=5)      # (compares every frame and the registers with the contract's loop)
        assert U.launches(hip) - n0 == 1
    finally:
        ms.release()
    return len(frames)


def run_surfaces(hip, case, rec, variant):
    """sp, sp_mix in place; sp8, p2sp, p2sp8 into pre-filled destinations"""
    from gpu_util import stream_ptr
    from test_gpu_model_programs_surfaces import run_out_of_place
    from test_gpu_semiplanar import run_in_place, scattered
    family = case.key.family
    program(hip, rec, case.mix)
    if family == "sp":
        run_in_place(hip, C.oracle_for(rec), K.sp_frames(case, variant), shuffle=1)
    elif family == "sp_mix":
        frames = K.sp_frames(case, variant)
        f0 = frames[0]
        res, excluded, processed, ora = K.mix_expectation(case)
        assert excluded / processed <= K.MIX_CAP, (excluded, processed)
        dev = scattered(frames, 4)
        hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, None, f0.width, f0.height, f0.stride, f0.uv_stride, case.shift, stream_ptr())
        for i, (d, (w, mask)) in enumerate(zip(dev, res)):
            n = M.mismatches(d.download(), w, mask)
            assert n == 0, f"frame {i}: {n} containers differ from the expectation"
        assert hip.seed_state() == ora.seed_state()
    else:
        ora = C.oracle_for(rec)
        run_out_of_place(hip, ora, K.surface_case(case, variant), rec)      # (destinations, fill and sources compared whole)
        assert hip.seed_state() == ora.seed_state()
    return case.nframes


def check_launch(hip, name, lds, case, nframes):
    info = hip.last_launch_info()
    k = case.key
    if name in K.UNREACHABLE:
        assert info["kernel"] != name and info["kernel"] in NAMES, (info, K.UNREACHABLE[name])
        return
    assert info["kernel"] == name, info
    assert info["lds_bytes_per_workgroup"] == lds, info
    assert (info["depth"], info["csubx"], info["csuby"]) == (k.depth, k.csubx, k.csuby), info
    assert (bool(info["out8"]), bool(info["one_y"]), bool(info["one_c"])) == (k.out8, k.oney, k.onec), info
    assert (info["parts_per_row"] > 1) == k.wide, info
    assert (info["persistent_luma_workgroups"] > 0) == k.persist, info
    assert info["nframes"] == nframes, info


@pytest.mark.parametrize("name, lds", FIXTURE, ids=[n for n, _ in FIXTURE])
def test_every_kernel_key_against_the_oracle(hip, name, lds):
    case = K.case_for(name)
    rec = MP.program(case.program)
    family = case.key.family
    run = run_planar if family in ("rw", "mix") else run_models if family in ("ml", "spml") else run_surfaces
    try:
        for variant in case.variants:
            nframes = run(hip, case, rec, variant)
            check_launch(hip, name, lds, case, nframes)
    finally:
        hip.clear_chroma_mix()
