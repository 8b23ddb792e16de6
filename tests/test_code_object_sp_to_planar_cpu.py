"""CPU: what the gfx950 code objects inside libvfgs_hip.so say about the 48 kernels that decide at run time whether their results go onto a
surface or into planes (grain_sp_kernel and grain_spml_kernel, KernelArgs::sp_kernel == 3; DESIGN.md 4.7 "planes out").

The second walk a UV workgroup holds, with a buffer descriptor per destination component, must cost these kernels no residency: no
scratch, no vector spill, the 40960 B of LDS and the four resident workgroups per CU they had -- what tests/test_code_object_semiplanar_cpu.py
and tests/test_code_object_sp_models_cpu.py pin, restated for this change over both families at once.  Read from the AMDGPU metadata notes
of the product library (no GPU needed)."""
import re
from pathlib import Path

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import LDS_PER_CU, READELF, code_objects, kernel_records, workgroups_per_cu

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_sp2p")
    out = {}
    for co in code_objects(B.LIB):
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs1[57]grain_(sp|spml)_kernelILi(\d+)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                out[(m.group(1),) + tuple(map(int, m.groups()[1:]))] = r
    return out


def test_the_48_kernels(kernels):
    want = {(f, d, y, oy, oc) for f in ("sp", "spml") for d in (8, 10, 12) for y in (2, 1) for oy in (0, 1) for oc in (0, 1)}
    assert set(kernels) == want and len(kernels) == 48


def test_no_scratch_and_no_vector_spill(kernels):
    bad = {k: (r["scratch"], r["vgpr_spill"]) for k, r in kernels.items() if r["scratch"] or r["vgpr_spill"]}
    assert not bad, bad


def test_lds_and_four_workgroups_per_cu(kernels):
    for k, r in kernels.items():
        assert r["lds"] == 40960 and LDS_PER_CU // r["lds"] == 4, (k, r)
        assert workgroups_per_cu(r) == 4, (k, r)
