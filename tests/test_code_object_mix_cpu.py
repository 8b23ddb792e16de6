"""CPU: the kernels of the luma / chroma mix (grain_mix_kernel) in the gfx950 code objects of libvfgs_hip.so: every
instantiation the dispatcher can ask for is there under its own name, none spills a vector register or uses scratch, and a CU
holds FOUR of their workgroups at either depth -- by the 128 registers they are compiled for and by the LDS they allocate.
(The kernels of always are tests/test_code_object_cpu.py's business and come out of the compiler as before.)
"""
import re

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import READELF, code_objects, kernel_records, workgroups_per_cu

from pathlib import Path

pytestmark = pytest.mark.skipif(not Path(READELF).exists(), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def mix_kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_mix")
    ks = {}
    for co in code_objects(B.LIB):
        for r in kernel_records(co, tmp):
            m = re.match(r"_ZN4vfgs16grain_mix_kernelILi(\d+)ELi(\d)ELi(\d)ELb(\d)ELb(\d)EEE", r["name"])
            if m:
                ks[tuple(map(int, m.groups()))] = r
    return ks


def test_every_instantiation_is_in_the_library(mix_kernels):
    # depth x chroma subsampling x (8-bit destination: 10 bit only) x (rows walked in parts: 4:2:0 and 4:4:4 only)
    want = {(d, sx, sy, o8, wide) for d in (8, 10) for sx in (1, 2) for sy in (1, 2) for o8 in ((0, 1) if d == 10 else (0,))
            for wide in ((0, 1) if sx == sy else (0,))}
    assert set(mix_kernels) == want and len(want) == 18


def test_no_vector_register_spills_and_no_scratch(mix_kernels):
    bad = {k: r for k, r in mix_kernels.items() if r["vgpr_spill"] or r["scratch"]}
    assert not bad, bad


def test_four_resident_workgroups_per_cu(mix_kernels):
    for k, r in mix_kernels.items():
        assert r["lds"] == 40960 and r["vgpr"] <= 128 and workgroups_per_cu(r) == 4, (k, r)
