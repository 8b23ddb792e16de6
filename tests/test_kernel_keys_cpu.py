"""CPU: the table of kernel keys (vfgs_layout.h KernelKey: kernel_exists, kernel_name, kernel_lds_bytes) against the kernels in the built library.

The launcher instantiates from kernel_exists() and the launch record names a kernel and its LDS from kernel_name() / kernel_lds_bytes().  A
stand-alone g++ program (tests/kernel_keys/kernel_keys.cpp) prints every key that exists over depths 8 / 10 / 12, the four formats, all bools and
all families; this test mangles the names as the test_code_object_*_cpu.py regexes read them and holds the three depth code objects to the list:
the same set of vfgs::grain_* kernels in both directions, no name twice, every kernel's group segment the key's LDS bytes.  No GPU needed."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import versatilefilmgrain_amd.build as B
from test_code_object_cpu import READELF, code_objects, kernel_records

PROGRAM = Path(__file__).resolve().parent / "kernel_keys" / "kernel_keys.cpp"
pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not Path(READELF).exists(), reason="needs g++ and llvm-readelf")


def mangled(name):
    """grain_sp_kernel<10,2,true,false> -> _ZN4vfgs15grain_sp_kernelILi10ELi2ELb1ELb0EEEvNS_10KernelArgsENS_10FrameTableE"""
    base, args = re.fullmatch(r"(\w+)<([\w,]+)>", name).groups()
    enc = "".join(f"Lb{int(a == 'true')}E" if a in ("true", "false") else f"Li{int(a)}E" for a in args.split(","))
    return f"_ZN4vfgs{len(base)}{base}I{enc}EEvNS_10KernelArgsENS_10FrameTableE"


@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    exe = tmp_path_factory.mktemp("keys") / "kernel_keys"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", str(PROGRAM), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    return [(name, int(lds)) for name, lds in (l.split() for l in lines)]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    B.build()
    tmp = tmp_path_factory.mktemp("co_keys")
    return [r for co in code_objects(B.LIB) for r in kernel_records(co, tmp) if re.match(r"_ZN4vfgs\d+grain_", r["name"])]


def test_one_kernel_has_exactly_one_key(keys):
    names = [n for n, _ in keys]
    assert len(names) == len(set(names)) and len({mangled(n) for n in names}) == len(names)
    # per depth: the dispatcher's table
    assert [sum(1 for n in names if n.split("<")[1].split(",")[0] == d) for d in ("8", "10", "12")] == [72, 134, 120]


def test_the_committed_key_list_is_the_tables(keys):
    """tests/golden/kernel_keys.txt -- what tests/test_gpu_kernel_keys.py launches key by key, without a compiler -- is this program's output
    line for line, and every key it prints has a launch recipe (tests/kernel_key_cases.py) whose program takes the key's form"""
    import kernel_key_cases as K
    import model_programs as MP
    assert K.fixture() == keys, ("regenerate tests/golden/kernel_keys.txt from tests/kernel_keys/kernel_keys.cpp", sorted(set(K.fixture()) ^ set(keys)))
    for name, _ in keys:
        c = K.case_for(name)
        assert K.key_name(c.key) == name and MP.expected_form(MP.program(c.program), c.key.wide) == (c.key.oney, c.key.onec), (name, c.program)


def test_the_code_objects_hold_the_keys_and_nothing_else(keys, kernels):
    have = [r["name"] for r in kernels]
    assert len(have) == len(set(have)), sorted(n for n in set(have) if have.count(n) > 1)
    want = {mangled(n): n for n, _ in keys}
    assert not set(want) - set(have), ("keys without a kernel", sorted(want[m] for m in set(want) - set(have)))
    assert not set(have) - set(want), ("kernels without a key", sorted(set(have) - set(want)))


def test_every_kernel_allocates_the_lds_of_its_key(keys, kernels):
    lds = {r["name"]: r["lds"] for r in kernels}
    wrong = {n: (lds[mangled(n)], want) for n, want in keys if mangled(n) in lds and lds[mangled(n)] != want}
    assert not wrong and all(mangled(n) in lds for n, _ in keys), wrong
