"""CPU: what the gfx950 code objects inside libvfgs_hip.so say about the kernels that serve a model per picture with the narrowed 8-bit
destination: no kernel of their own, but the 32 grain_rw_kernel<depth, csubx, csuby, true, oney, onec, false, false> and the
16 grain_sp8_kernel<depth, csuby, oney, onec> of depths 10 and 12, which now decide at run time where image, clip bounds and shift come from
(run_plane_rw / run_uv_sp MODELS = 2).  They are there under their names, none spills a vector register or uses scratch, each allocates the
LDS of its key (tests/golden/kernel_keys.txt, the table tests/test_kernel_keys_cpu.py pins) and each is in the residency class the existing
code-object tests state for it: four workgroups per CU -- grain_sp8_kernel at 40960 B (tests/test_code_object_sp_out8_cpu.py), the row walk
with one-pattern luma at 40960 B (39968 B over general-form chroma of subsampled geometry), with general-form luma by its 40 KB image
(tests/test_code_object_cpu.py)."""
import re
from pathlib import Path

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import LDS_PER_CU, READELF, code_objects, kernel_records, workgroups_per_cu

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernel_keys.txt"
b = lambda v: "true" if v else "false"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_models_out8")
    rw, sp8 = {}, {}
    for co in code_objects(B.LIB):
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs15grain_rw_kernelILi(\d+)ELi(\d)ELi(\d)ELb1ELb(\d)ELb(\d)ELb0ELb0EEE", r["name"])
            if m:
                assert tuple(map(int, m.groups())) not in rw
                rw[tuple(map(int, m.groups()))] = r
            m = re.match(r"_ZN4vfgs16grain_sp8_kernelILi(\d+)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                assert tuple(map(int, m.groups())) not in sp8
                sp8[tuple(map(int, m.groups()))] = r
    return rw, sp8


@pytest.fixture(scope="module")
def key_lds():
    return {name: int(lds) for name, lds in (line.split() for line in GOLDEN.read_text().splitlines() if line.strip())}


def test_the_48_kernels_are_in_the_library(kernels):
    rw, sp8 = kernels
    assert set(rw) == {(d, sx, sy, oy, oc) for d in (10, 12) for sx in (1, 2) for sy in (1, 2) for oy in (0, 1) for oc in (0, 1)} and len(rw) == 32
    assert set(sp8) == {(d, sy, oy, oc) for d in (10, 12) for sy in (1, 2) for oy in (0, 1) for oc in (0, 1)} and len(sp8) == 16


def test_no_vector_register_spills_and_no_scratch(kernels):
    bad = {k: r for ks in kernels for k, r in ks.items() if r["vgpr_spill"] or r["scratch"]}
    assert not bad, bad


def test_the_lds_is_the_keys(kernels, key_lds):
    rw, sp8 = kernels
    for (d, sx, sy, oy, oc), r in rw.items():
        assert r["lds"] == key_lds[f"grain_rw_kernel<{d},{sx},{sy},true,{b(oy)},{b(oc)},false,false>"], ((d, sx, sy, oy, oc), r)
    for (d, sy, oy, oc), r in sp8.items():
        assert r["lds"] == key_lds[f"grain_sp8_kernel<{d},{sy},{b(oy)},{b(oc)}>"], ((d, sy, oy, oc), r)


def test_resident_workgroups_per_cu_are_the_existing_classes(kernels):
    rw, sp8 = kernels
    for k, r in sp8.items():
        assert r["lds"] == 40960 and LDS_PER_CU // r["lds"] == 4 and workgroups_per_cu(r) == 4, (k, r)
    for (d, sx, sy, oy, oc), r in rw.items():
        if oy:
            assert r["lds"] == (40960 if oc or sx * sy > 1 else 39968) and workgroups_per_cu(r) == 4, ((d, sx, sy, oy, oc), r)
        else:
            assert r["lds"] <= 40960 and workgroups_per_cu(r) == 4, ((d, sx, sy, oy, oc), r)
