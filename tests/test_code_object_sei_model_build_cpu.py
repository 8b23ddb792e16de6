"""CPU: what the firmware code object inside libvfgs_hip.so says about fw_sei_build_kernel (vfgs_fw_kernel.hip), the kernel that builds a chunk
of film grain models from FGC SEI messages: it is in the code object of the other firmware kernels, exactly once; it spills nothing and uses
no scratch (the recursion keeps its windows in registers, and an indexed member of the image layout would put the output addresses into
scratch memory); its group segment is what the source declares (vfgs_model_build.h: the larger of the frequency-filtered and the
auto-regressive use of one region); and it fits the registers of its workgroup.  Read from the AMDGPU metadata notes of the product
library; no GPU needed."""
import re
from pathlib import Path

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import READELF, code_objects, kernel_records

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")

KERNEL = "fw_sei_build_kernel"


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co")
    return [kernel_records(co, tmp) for co in code_objects(B.LIB)]


def declared_lds():
    text = (B.CSRC / "vfgs_model_build.h").read_text()
    m = re.search(r"static_assert\(kFwSeiLdsBytes == (\d+),", text)
    assert m, "vfgs_model_build.h no longer states the group segment"
    arena_y = (256 + 82 * 73 + 128 + 15) & ~15
    arena_c = 256 + 64 * 44 + 128
    ff = 8 * 64 * 64 + 8 * 32 * 32 + 2 * 64 * 68 + 64 * 64 * 2 + 32 * 64 * 4 + 2048 + 2 * 40 * 4
    ar = 8 * arena_y + 8 * arena_c + 2048 + 2 * 192 * 4
    assert int(m.group(1)) == max(ff, ar)      # what the header's comment says the number is made of
    return int(m.group(1))


def test_the_kernel_is_in_the_firmware_code_object_once(objects):
    homes = [i for i, recs in enumerate(objects) if any(KERNEL in r["name"] for r in recs)]
    assert len(homes) == 1, homes
    names = [r["name"] for r in objects[homes[0]]]
    assert sum(KERNEL in n for n in names) == 1, names
    for k in ("fw_ff_kernel", "fw_ar_kernel", "fw_commit_chroma", "fw_patch_tables", "fw_models_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
        assert k not in KERNEL


def test_no_spills_no_scratch_the_declared_group_segment_and_the_registers_of_1024_threads(objects):
    (r,) = [r for recs in objects for r in recs if KERNEL in r["name"]]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["lds"] == declared_lds(), r
    assert r["lds"] <= 160 * 1024
    # the workgroup is 1024 threads = 16 wavefronts, four per SIMD: 512 registers per lane of a SIMD / 4 = at most 128
    assert r["vgpr"] <= 128, r
