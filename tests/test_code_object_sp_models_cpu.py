"""CPU: what the gfx950 code objects inside libvfgs_hip.so say about the kernels of semi-planar frames with a model per frame
(grain_spml_kernel).

A grain_spml_kernel is its grain_sp_kernel twin -- <depth, csuby, oney, onec> -- with the tables, the clip bounds and the packed form's shift
fetched per frame, in the luma and in the UV workgroups.  That must cost it no residency: same LDS allocation, same resident workgroups per
CU, no vector spill, no scratch.  Read from the AMDGPU metadata notes of the product library, as tests/test_code_object_models_cpu.py does
(no GPU needed)."""
import re
from pathlib import Path

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import READELF, code_objects, kernel_records, workgroups_per_cu

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_spml")
    spml, sp, per_object = {}, {}, []
    for co in code_objects(B.LIB):
        n = 0
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs17grain_spml_kernelILi(\d+)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                spml[tuple(map(int, m.groups()))] = r
                n += 1
            m = re.match(r"_ZN4vfgs15grain_sp_kernelILi(\d+)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                sp[tuple(map(int, m.groups()))] = r
        per_object.append(n)
    return spml, sp, per_object


def test_eight_instantiations_per_depth(kernels):
    spml, _, per_object = kernels
    want = {(d, y, oy, oc) for d in (8, 10, 12) for y in (2, 1) for oy in (0, 1) for oc in (0, 1)}
    assert set(spml) == want
    assert sorted(per_object) == [0, 8, 8, 8], per_object      # one code object per depth, none in the firmware's


def test_no_vector_register_spills_and_no_scratch(kernels):
    spml, _, _ = kernels
    bad = {k: r for k, r in spml.items() if r["vgpr_spill"] or r["scratch"]}
    assert not bad, bad


def test_lds_and_residency_are_the_twins(kernels):
    spml, sp, _ = kernels
    assert len(spml) == 24
    for k, r in spml.items():
        t = sp[k]
        assert r["lds"] == t["lds"], (k, r, t)
        assert workgroups_per_cu(r) == workgroups_per_cu(t), (k, r, t)
