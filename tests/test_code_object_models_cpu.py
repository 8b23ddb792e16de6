"""CPU: what the gfx950 code objects inside libvfgs_hip.so say about the kernels with a model per frame (grain_ml_kernel).

A grain_ml_kernel is its grain_rw_kernel twin -- <depth, csubx, csuby, false, oney, onec, false, false>: in place or out of place, ordinary
rows, no persistence -- with the table image, the clip bounds and the packed form's shift fetched per frame.  That must cost it no
residency: same LDS allocation, same resident workgroups per CU, no vector spill, no scratch.  Read from the AMDGPU metadata notes of the
product library, as tests/test_code_object_cpu.py does (no GPU needed)."""
import re

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import READELF, code_objects, kernel_records, workgroups_per_cu
from pathlib import Path

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_ml")
    ml, rw, per_object = {}, {}, []
    for co in code_objects(B.LIB):
        n = 0
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs15grain_ml_kernelILi(\d+)ELi(\d)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                ml[tuple(map(int, m.groups()))] = r
                n += 1
            m = re.match(r"_ZN4vfgs15grain_rw_kernelILi(\d+)ELi(\d)ELi(\d)ELb0ELb(\d)ELb(\d)ELb0ELb0EEE", r["name"])
            if m:
                rw[tuple(map(int, m.groups()))] = r
        per_object.append(n)
    return ml, rw, per_object


def test_sixteen_instantiations_per_depth(kernels):
    ml, _, per_object = kernels
    want = {(d, x, y, oy, oc) for d in (8, 10, 12) for x, y in ((2, 2), (2, 1), (1, 1), (1, 2)) for oy in (0, 1) for oc in (0, 1)}
    assert set(ml) == want
    assert sorted(per_object) == [0, 16, 16, 16], per_object      # one code object per depth, none in the firmware's


def test_no_vector_register_spills_and_no_scratch(kernels):
    ml, _, _ = kernels
    bad = {k: r for k, r in ml.items() if r["vgpr_spill"] or r["scratch"]}
    assert not bad, bad


def test_lds_and_residency_are_the_twins(kernels):
    ml, rw, _ = kernels
    assert len(ml) == 48
    for k, r in ml.items():
        t = rw[k]
        assert r["lds"] == t["lds"], (k, r, t)
        assert workgroups_per_cu(r) == workgroups_per_cu(t), (k, r, t)
