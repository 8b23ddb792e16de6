"""CPU: the two kernel families that now also serve models with a mix of their own (grain_mix_kernel, grain_sp_mix_kernel: the record is read
with scalar loads under a wave-uniform branch) in the gfx950 code objects of libvfgs_hip.so -- still no vector register spill, no scratch,
the LDS of their keys and the registers of their residency class -- and fw_models_kernel, which writes the mix words with the record: still
once in the firmware code object, spill-free, with the LDS vfgs_model_build.h states."""
import re
from pathlib import Path

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import READELF, code_objects, kernel_records, workgroups_per_cu

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_model_mix")
    return [r for co in code_objects(B.LIB) for r in kernel_records(co, tmp)]


def test_the_planar_family(kernels):
    ks = [r for r in kernels if r["name"].startswith("_ZN4vfgs16grain_mix_kernelILi")]
    assert len(ks) == 18
    for r in ks:
        assert not r["vgpr_spill"] and not r["scratch"] and r["lds"] == 40960 and r["vgpr"] <= 128 and workgroups_per_cu(r) == 4, r
    # the instantiations that decide "a model per frame" at run time: neither the narrowed destination nor rows walked in parts
    run_time = [r for r in ks if re.search(r"ELb0ELb0EEE", r["name"])]
    assert len(run_time) == 8, [r["name"] for r in run_time]


def test_the_semi_planar_family(kernels):
    ks = [r for r in kernels if r["name"].startswith("_ZN4vfgs19grain_sp_mix_kernelILi")]
    assert len(ks) == 4
    for r in ks:
        assert not r["vgpr_spill"] and not r["scratch"] and r["lds"] == 53248 and r["vgpr"] <= 168 and workgroups_per_cu(r) == 3, r


def test_the_kernel_that_builds_models(kernels):
    ks = [r for r in kernels if "fw_models_kernel" in r["name"]]
    assert len(ks) == 1
    assert not ks[0]["vgpr_spill"] and not ks[0]["scratch"] and ks[0]["lds"] == 13168, ks[0]
