"""CPU: what the gfx950 code objects inside libvfgs_hip.so say about the kernels of semi-planar frames with the narrowed 8-bit destination
(grain_sp8_kernel): the 16 instantiations -- depths 10 and 12 x 4:2:0 / 4:2:2 x the four forms of the table image, eight in
each of the 10- and 12-bit code objects and none in the 8-bit one -- are there under their names, none spills a vector register or uses
scratch, and every one is resident at the four workgroups per CU of grain_sp_kernel: the LDS allocation says four (40 KB), and the
registers allow at least that."""
import re

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import LDS_PER_CU, READELF, code_objects, kernel_records, workgroups_per_cu

pytestmark = pytest.mark.skipif(not __import__("pathlib").Path(READELF).exists(), reason="needs llvm-readelf")

WORKGROUPS_PER_CU = 4      # kSpWgPerCU


@pytest.fixture(scope="module")
def sp8_kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_sp8")
    per_object = []
    for co in code_objects(B.LIB):
        ks, depths = {}, set()
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs16grain_sp8_kernelILi(\d+)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                ks[tuple(map(int, m.groups()))] = r
            m = re.match(r"_ZN4vfgs15grain_sp_kernelILi(\d+)E", r["name"])      # (which depth's code object this is)
            if m:
                depths.add(int(m.group(1)))
        per_object.append((depths, ks))
    return per_object


def test_every_instantiation_is_in_the_library(sp8_kernels):
    by_depth = {}
    for depths, ks in sp8_kernels:
        if depths:
            assert len(depths) == 1, depths
            by_depth[depths.pop()] = ks
        else:
            assert not ks, sorted(ks)
    assert sorted(by_depth) == [8, 10, 12]
    assert not by_depth[8], sorted(by_depth[8])
    for d in (10, 12):
        assert set(by_depth[d]) == {(d, sy, oy, oc) for sy in (1, 2) for oy in (0, 1) for oc in (0, 1)}, sorted(by_depth[d])
    assert sum(len(ks) for _, ks in sp8_kernels) == 16


def test_no_vector_register_spills_and_no_scratch(sp8_kernels):
    bad = {k: r for _, ks in sp8_kernels for k, r in ks.items() if r["vgpr_spill"] or r["scratch"]}
    assert not bad, bad


def test_resident_workgroups_per_cu(sp8_kernels):
    n = 0
    for _, ks in sp8_kernels:
        for k, r in ks.items():
            assert LDS_PER_CU // r["lds"] == WORKGROUPS_PER_CU and r["lds"] == 40960, (k, r)
            assert workgroups_per_cu(r) == WORKGROUPS_PER_CU, (k, r)
            n += 1
    assert n == 16
