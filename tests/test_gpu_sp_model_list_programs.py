"""GPU (MI355X): the generated programs of tests/model_programs.py with a horizontally subsampled chroma format, captured as models
(vfgs_hip_model_capture) and used a model per picture on semi-planar frames (vfgs_hip_add_grain_sp_frame_list_models_dev,
grain_spml_kernel), against the oracle run as the contract's loop (tests/sp_model_list_util.py), bit for bit: every container of both
planes, padding included, and the four seed registers.

The traces of tests/test_gpu_sp_model_list.py have no model with slot 8, with Cb and Cr on different slots, with a -128, at the packed
16-bit limit, with a scale_shift other than 4 / 5, or programmed by a shuffled sequence; the UV workgroup reads the clip bounds and the
packed form's shift from the frame's record and stages BOTH components' tables from the frame's image.  Here every such program is a
model: each (depth, chroma rows) group is ONE list with a model per picture, shuffled -- the form changes inside it --, in place, at
328 x 56 (the generator's shape, the planar twin test's: 21 blocks, 3.5 block rows).  Frames are MP.content of the frame's own model
(in-range and garbage content in turn), interleaved; at 10 and 12 bit the 4:2:2 groups carry their samples high-aligned."""
import pytest

import model_list_util as U
import model_programs as MP
import semiplanar_util as SP
from test_gpu_sp_model_list import Models, fresh_seeds, run

pytestmark = pytest.mark.gpu

W, H = 328, 56
GROUPS = [(d, f) for d in MP.DEPTHS for f in ("420", "422")]
RAN = {}


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


def subsampled_names():
    return [n for n in MP.names() if MP.parse(n)[2] in ("420", "422")]


def test_the_groups_hold_every_subsampled_program():
    got = sorted(n for d, f in GROUPS for n in MP.names(depth=d, fmt=f))
    assert got == sorted(subsampled_names()) and all(MP.names(depth=d, fmt=f) for d, f in GROUPS)
    import vfgs_testlib as T
    assert all(T.trace_geometry(MP.program(n))[1] == 2 for n in got)
    assert not any(T.trace_geometry(MP.program(n))[1] == 2 for n in MP.names() if n not in got)


def run_group(hip, depth, fmt):
    """the group's list through the call, once a session; -> the number of programs it ran"""
    if (depth, fmt) in RAN:
        return RAN[depth, fmt]
    names = MP.names(depth=depth, fmt=fmt)
    assert names
    ms = Models(hip, names)
    try:
        g = GROUPS.index((depth, fmt))
        pick = MP.Rng(f"sp model list/{depth}/{fmt}").shuffle(range(len(names)))
        assert sorted(pick) == list(range(len(names)))
        runs = U.runs_of(ms.forms, pick)
        assert len(set(ms.forms)) == 4 and len(runs) >= 8, (ms.forms, runs)
        shift = 16 - depth if (depth > 8 and fmt == "422") else 0
        frames = [SP.to_semiplanar(MP.content(names[k], W, H, 1, MP.VARIANTS[i % 2])[0], shift, low_bits_seed=i if shift else None) for i, k in enumerate(pick)]
        seeded = g % 2 == 1
        ora = None
        if not seeded:
            # one seed sequence: it begins at registers both sides know
            ora = U.oracle_programmed(ms.recs[-1])
            hip.set_seed(0xC0FFEE + g)
            ora.set_seed(0xC0FFEE + g)
        n0 = U.launches(hip)
        run(hip, ms, pick, frames, fresh_seeds(len(pick), g) if seeded else None, ora=ora, shuffle=g)
        info = hip.last_launch_info()
        assert info["launches"] - n0 == len(runs) and info["nframes"] == runs[-1] and info["listed"] == 1 and info["in_place"] == 1, (info, runs)
        assert info["kernel"] == ms.kernel(pick[-1]), info
        RAN[depth, fmt] = len(pick)
        return len(pick)
    finally:
        ms.release()


@pytest.mark.parametrize("depth, fmt", GROUPS)
def test_every_program_is_a_model_on_a_surface(hip, depth, fmt):
    assert run_group(hip, depth, fmt) == len(MP.names(depth=depth, fmt=fmt)) > 0


def test_no_program_was_left_out(hip):
    """every group ran (here, unless it already has), none is empty, and together they ran every program with csubx == 2"""
    ran = {g: run_group(hip, *g) for g in GROUPS}
    assert all(ran.values()), ran
    assert sum(ran.values()) == len(subsampled_names())
