"""CPU: sample depth 12 where no GPU is needed -- the export that answers which depths exist, the host-only state after
vfgs_set_depth(12) (bs = 4, the shift stored as shift + 2: vfgs_hw.c:349,356-359 with bs = depth - 8), and what the gfx950 code
objects say about the 12-bit kernels: the 64 grain_rw_kernel<12,...> instantiations of the 10-bit class and no grain_mix_kernel<12,...>,
no spill and no scratch, and for each the LDS bytes and the resident workgroups per CU of its 10-bit twin (the two move the same
bytes through the same LDS image).
"""
import re
from pathlib import Path

import pytest

import vfgs_testlib as T

import versatilefilmgrain_amd.build as B
from versatilefilmgrain_amd import hw
from test_code_object_cpu import READELF, code_objects, kernel_records, workgroups_per_cu

needs_readelf = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def lib():
    B.build()
    return hw.load()


def test_the_export_and_its_answers(lib):
    assert "vfgs_hip_supports_depth" in hw.EXPORTS and hasattr(lib, "vfgs_hip_supports_depth")
    assert [d for d in range(-2, 40) if lib.vfgs_hip_supports_depth(d)] == [8, 10, 12]
    h = hw.VfgsHip()
    assert h.supports_depth(12) and h.supports_depth(10) and h.supports_depth(8) and not h.supports_depth(9) and not h.supports_depth(16)


@pytest.mark.parametrize("shift", [2, 5, 7])
def test_host_state_after_set_depth_12(lib, shift):
    assert lib.vfgs_hip_supports_depth(12) == 1
    # in both orders (vfgs_hw.c:349 and :356-359), and against the oracle's model of the setters
    for order in ("shift_first", "depth_first"):
        h, m = hw.VfgsHip(), T.StateModel()
        for x in (h, m):
            if order == "shift_first":
                x.set_scale_shift(shift)
                x.set_depth(12)
            else:
                x.set_depth(12)
                x.set_scale_shift(shift)
        p = h.params()
        assert p["bs"] == 4 == m.bs and p["scale_shift"] == shift + 2 == m.shift, (order, p)
        assert (p["ymin"], p["ymax"], p["cmin"], p["cmax"]) == (0, 255, 0, 255)      # 8-bit units: the kernel arguments hold them << bs
        h.set_legal_range(1)
        p = h.params()
        assert (p["ymin"], p["ymax"], p["cmin"], p["cmax"]) == (16, 235, 16, 240)
        # 12 -> 10 -> 8 -> 12: the stored shift follows bs
        for d in (10, 8, 12):
            h.set_depth(d)
            assert h.params()["bs"] == d - 8 and h.params()["scale_shift"] == shift + 6 - (d - 8)
    hw.VfgsHip()      # (reset)
    assert hw.VfgsHip(reset=False).params()["bs"] == 0


def test_every_10_bit_trace_replays_at_depth_12_without_a_gpu(lib):
    assert lib.vfgs_hip_supports_depth(12) == 1      # (vfgs_set_depth is a void drop-in call: it aborts on a depth it does not have)
    h = hw.VfgsHip()
    for name in T.list_traces():
        rec = T.load_trace(name)
        if T.trace_geometry(rec)[0] != 10:
            continue
        rec12 = [(op, 12 if op == T.OP_DEPTH else a, b, p) for op, a, b, p in rec]
        m10, m12 = T.StateModel(), T.StateModel()
        T.replay(m10, rec)
        T.replay(m12, rec12)
        h.lib.vfgs_hip_reset_state()
        T.replay(h, rec12)
        p = h.params()
        assert p["bs"] == 4 and p["scale_shift"] == m12.shift == m10.shift - 2, name
    h.lib.vfgs_hip_reset_state()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co12")
    rw, mix, per_object = {}, [], []
    for co in code_objects(B.LIB):
        depths = set()
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs15grain_rw_kernelILi(\d+)ELi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                rw[tuple(map(int, m.groups()))] = r
                depths.add(int(m.group(1)))
            m = re.match(r"_ZN4vfgs16grain_mix_kernelILi(\d+)E", r["name"])
            if m:
                mix.append(int(m.group(1)))
        if depths:
            per_object.append(depths)
    return rw, mix, per_object


@needs_readelf
def test_the_12_bit_kernels_are_the_10_bit_class_and_no_mix_kernel(kernels):
    rw, mix, per_object = kernels
    twelve = {k[1:] for k in rw if k[0] == 12}
    ten = {k[1:] for k in rw if k[0] == 10}
    assert len(twelve) == 64 and twelve == ten
    assert 12 not in mix and sorted(set(mix)) == [8, 10]
    # a code object of their own
    assert {12} in per_object and all(d == {12} or 12 not in d for d in per_object)


@needs_readelf
def test_no_spills_and_no_scratch_at_12_bit(kernels):
    rw = kernels[0]
    bad = {k: r for k, r in rw.items() if k[0] == 12 and (r["vgpr_spill"] or r["scratch"])}
    assert len([k for k in rw if k[0] == 12]) == 64 and not bad, bad


@needs_readelf
def test_lds_and_workgroups_per_cu_equal_the_10_bit_twin(kernels):
    rw = kernels[0]
    n = 0
    for k, r in rw.items():
        if k[0] != 12:
            continue
        twin = rw[(10,) + k[1:]]
        assert r["lds"] == twin["lds"] and workgroups_per_cu(r) == workgroups_per_cu(twin), (k, r, twin)
        n += 1
    assert n == 64
