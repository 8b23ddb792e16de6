"""CPU: what the gfx950 code objects inside libvfgs_hip.so say about the kernels of semi-planar frames (grain_sp_kernel):
the 24 instantiations -- three depths x 4:2:0 / 4:2:2 x the four forms of the table image, eight per code object -- are there under their
names, none spills a vector register or uses scratch, and every one is resident at the four workgroups per CU DESIGN.md 4.7 states: the
LDS allocation says four (40 KB, like the kernels of the mix), and the registers allow at least that."""
import re

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import LDS_PER_CU, READELF, code_objects, kernel_records, workgroups_per_cu

pytestmark = pytest.mark.skipif(not __import__("pathlib").Path(READELF).exists(), reason="needs llvm-readelf")

WORKGROUPS_PER_CU = 4      # DESIGN.md 4.7, every class


@pytest.fixture(scope="module")
def sp_kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_sp")
    per_object = []
    for co in code_objects(B.LIB):
        ks = {}
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs15grain_sp_kernelILi(\d+)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                ks[tuple(map(int, m.groups()))] = r
        if ks:
            per_object.append(ks)
    return per_object


def test_every_instantiation_is_in_the_library(sp_kernels):
    assert len(sp_kernels) == 3 and all(len(ks) == 8 for ks in sp_kernels), [sorted(ks) for ks in sp_kernels]
    assert sorted(sorted({k[0] for k in ks}) for ks in sp_kernels) == [[8], [10], [12]]      # one code object per depth
    want = {(d, sy, oy, oc) for d in (8, 10, 12) for sy in (1, 2) for oy in (0, 1) for oc in (0, 1)}
    assert {k for ks in sp_kernels for k in ks} == want


def test_no_vector_register_spills_and_no_scratch(sp_kernels):
    bad = {k: r for ks in sp_kernels for k, r in ks.items() if r["vgpr_spill"] or r["scratch"]}
    assert not bad, bad


def test_resident_workgroups_per_cu(sp_kernels):
    for ks in sp_kernels:
        for k, r in ks.items():
            assert LDS_PER_CU // r["lds"] == WORKGROUPS_PER_CU and r["lds"] == 40960, (k, r)
            assert workgroups_per_cu(r) == WORKGROUPS_PER_CU, (k, r)
