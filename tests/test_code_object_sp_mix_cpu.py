"""CPU: the kernels of semi-planar frames under the luma / chroma mix (grain_sp_mix_kernel) in the gfx950 code objects of
libvfgs_hip.so: the four instantiations the dispatcher can ask for are there under their names -- the 8-bit ones in the 8-bit code object,
the 10-bit ones in the 10-bit one, none at depth 12 --, none spills a vector register or uses scratch, and a CU holds THREE of their
workgroups: by the registers they are compiled for (at most 168) and by the LDS they allocate (53248 bytes), as DESIGN.md 4.7 states.
"""
import re
from pathlib import Path

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import READELF, code_objects, kernel_records, workgroups_per_cu

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")

WORKGROUPS_PER_CU = 3       # DESIGN.md 4.7 "the mix on semi-planar frames"; vfgs_layout.h kSpMixWgPerCU


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    """per code object: (depths of its grain_rw_kernel instantiations, {(depth, csuby): record} of its grain_sp_mix_kernel ones)"""
    B.build()
    tmp = tmp_path_factory.mktemp("co_sp_mix")
    out = []
    for co in code_objects(B.LIB):
        depths, ks = set(), {}
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs15grain_rw_kernelILi(\d+)E", r["name"])
            if m:
                depths.add(int(m.group(1)))
            m = re.match(r"_ZN4vfgs19grain_sp_mix_kernelILi(\d+)ELi(\d)EEE", r["name"])
            if m:
                ks[tuple(map(int, m.groups()))] = r
        if depths:
            out.append((depths, ks))
    return out


def test_every_instantiation_is_in_its_code_object(objects):
    by_depth = {min(d): set(ks) for d, ks in objects if len(d) == 1}
    assert by_depth == {8: {(8, 1), (8, 2)}, 10: {(10, 1), (10, 2)}, 12: set()}, by_depth


def test_no_vector_register_spills_and_no_scratch(objects):
    recs = {k: r for _, ks in objects for k, r in ks.items()}
    assert len(recs) == 4
    bad = {k: r for k, r in recs.items() if r["vgpr_spill"] or r["scratch"]}
    assert not bad, bad


def test_three_resident_workgroups_per_cu(objects):
    assert sum(len(ks) for _, ks in objects) == 4
    for _, ks in objects:
        for k, r in ks.items():
            assert r["lds"] == 53248 and 128 < r["vgpr"] <= 168 and workgroups_per_cu(r) == WORKGROUPS_PER_CU, (k, r)
            assert 163840 // r["lds"] == WORKGROUPS_PER_CU and 512 // ((r["vgpr"] + 7) // 8 * 8) == WORKGROUPS_PER_CU, (k, r)
