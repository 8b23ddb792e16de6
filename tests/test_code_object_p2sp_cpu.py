"""CPU: what the gfx950 code objects inside libvfgs_hip.so say about the kernels of a planar source with a semi-planar destination
(grain_p2sp_kernel, grain_p2sp8_kernel): the 24 grain_p2sp_kernel instantiations -- three depths x 4:2:0 / 4:2:2 x the four
forms of the table image, eight in each depth's code object -- and the 16 grain_p2sp8_kernel ones -- eight in each of the 10- and 12-bit
objects, none in the 8-bit one -- are there under their names, none spills a vector register or uses scratch, and every one is resident at
no fewer workgroups per CU than the grain_sp_kernel / grain_sp8_kernel instantiation with the same template arguments IN THE SAME BUILD:
the bar is read from the code object, not fixed here."""
import re

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import LDS_PER_CU, READELF, code_objects, kernel_records, workgroups_per_cu

pytestmark = pytest.mark.skipif(not __import__("pathlib").Path(READELF).exists(), reason="needs llvm-readelf")

FAMILIES = {"p2sp": "17grain_p2sp_kernel", "p2sp8": "18grain_p2sp8_kernel", "sp": "15grain_sp_kernel", "sp8": "16grain_sp8_kernel"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_p2sp")
    per_object = []
    for co in code_objects(B.LIB):
        fam = {k: {} for k in FAMILIES}
        for r in kernel_records(co, tmp):
            for k, mangled in FAMILIES.items():
                m = re.match(rf"_ZN4vfgs{mangled}ILi(\d+)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
                if m:
                    fam[k][tuple(map(int, m.groups()))] = r
        per_object.append(fam)
    return per_object


def by_depth(kernels):
    out = {}
    for fam in kernels:
        depths = {k[0] for k in fam["sp"]}
        if not depths:
            assert not fam["p2sp"] and not fam["p2sp8"], (sorted(fam["p2sp"]), sorted(fam["p2sp8"]))
            continue
        assert len(depths) == 1, depths
        out[depths.pop()] = fam
    return out


def test_every_instantiation_is_in_the_library(kernels):
    d = by_depth(kernels)
    assert sorted(d) == [8, 10, 12]
    forms = lambda depth: {(depth, sy, oy, oc) for sy in (1, 2) for oy in (0, 1) for oc in (0, 1)}
    for depth in (8, 10, 12):
        assert set(d[depth]["p2sp"]) == forms(depth), sorted(d[depth]["p2sp"])
    assert not d[8]["p2sp8"], sorted(d[8]["p2sp8"])
    for depth in (10, 12):
        assert set(d[depth]["p2sp8"]) == forms(depth), sorted(d[depth]["p2sp8"])
    assert sum(len(f["p2sp"]) for f in kernels) == 24 and sum(len(f["p2sp8"]) for f in kernels) == 16


def test_no_vector_register_spills_and_no_scratch(kernels):
    bad = {k: r for f in kernels for fam in ("p2sp", "p2sp8") for k, r in f[fam].items() if r["vgpr_spill"] or r["scratch"]}
    assert not bad, bad


def test_resident_at_the_workgroups_per_cu_of_the_semi_planar_twin(kernels):
    n = 0
    for f in kernels:
        for fam, twin in (("p2sp", "sp"), ("p2sp8", "sp8")):
            for k, r in f[fam].items():
                t = f[twin][k]
                assert LDS_PER_CU // r["lds"] >= LDS_PER_CU // t["lds"], (fam, k, r, t)
                assert workgroups_per_cu(r) >= workgroups_per_cu(t), (fam, k, r, t)
                n += 1
    assert n == 40
