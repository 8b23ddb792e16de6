"""CPU: what the firmware code object inside libvfgs_hip.so says about fw_models_kernel (vfgs_fw_kernel.hip), the kernel that builds a chunk of
film grain models from AFGS1 parameter sets: it is in the code object of the other firmware kernels, it spills nothing and uses no scratch
(the recursion keeps its windows in registers: a spill would put memory round trips into a chain of some 400 dependent steps), and its
group segment is what the source declares (vfgs_model_build.h: two arenas, the Gaussian table, two LFSR streams).  Read from the AMDGPU
metadata notes of the product library; no GPU needed."""
import re
import shutil
from pathlib import Path

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import READELF, code_objects, kernel_records

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co")
    return [kernel_records(co, tmp) for co in code_objects(B.LIB)]


def declared_lds():
    text = (B.CSRC / "vfgs_model_build.h").read_text()
    m = re.search(r"static_assert\(kFwModelsLdsBytes == (\d+),", text)
    assert m, "vfgs_model_build.h no longer states the group segment"
    arena_y = (256 + 82 * 73 + 128 + 15) & ~15
    arena_c = 256 + 64 * 44 + 128
    assert int(m.group(1)) == arena_y + arena_c + 2048 + 2 * 192 * 4      # what the header's comment says the number is made of
    return int(m.group(1))


def test_the_kernel_is_in_the_firmware_code_object(objects):
    homes = [i for i, recs in enumerate(objects) if any("fw_models_kernel" in r["name"] for r in recs)]
    assert len(homes) == 1, homes
    names = [r["name"] for r in objects[homes[0]]]
    for k in ("fw_ff_kernel", "fw_ar_kernel", "fw_commit_chroma", "fw_patch_tables", "fw_models_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert not any("grain_" in n for n in names), names       # (and no grain kernel moved in with them)


def test_no_spills_no_scratch_and_the_declared_group_segment(objects):
    (r,) = [r for recs in objects for r in recs if "fw_models_kernel" in r["name"]]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["lds"] == declared_lds(), r
    assert r["vgpr"] <= 128, r        # four waves of a workgroup, one per SIMD: at most 128 registers keep four workgroups on a CU
