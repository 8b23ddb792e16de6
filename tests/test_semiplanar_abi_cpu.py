"""CPU: the semi-planar call as a C caller sees it: a C99 translation unit that includes the public header, takes the address of
vfgs_hip_add_grain_sp_frame_list_dev with its declared type and fills a vfgs_hip_sp_frame, compiled with -std=c99 -pedantic -Wall -Werror
and linked against the built library (the symbol must resolve); and the library's dynamic symbol table exports it."""
import shutil
import subprocess

import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import build as vbuild

SOURCE = r"""
#include <stdio.h>
#include "vfgs_hip.h"

typedef int (*sp_fn)(const vfgs_hip_sp_frame*, const vfgs_hip_sp_frame*, const uint32_t*, unsigned, unsigned, unsigned, unsigned, unsigned,
                     unsigned, void*);

int main(void)
{
	sp_fn f = vfgs_hip_add_grain_sp_frame_list_dev;
	vfgs_hip_sp_frame fr;
	fr.Y = NULL;
	fr.UV = NULL;
	if (!f || fr.Y || fr.UV || sizeof fr != 2 * sizeof(void*)) return 1;
	puts("abi ok");
	return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c99_caller_compiles_links_and_runs(tmp_path):
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    src = tmp_path / "sp_abi.c"
    src.write_text(SOURCE)
    exe = tmp_path / "sp_abi"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{T.ROOT / 'include'}", str(src), "-o", str(exe),
                        f"-L{vbuild.LIB.parent}", "-lvfgs_hip", f"-Wl,-rpath,{vbuild.LIB.parent}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_the_symbol_is_exported_and_bound():
    import ctypes as C
    from versatilefilmgrain_amd import hw
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    assert "vfgs_hip_add_grain_sp_frame_list_dev" in hw.EXPORTS
    lib = C.CDLL(str(vbuild.LIB))
    assert lib.vfgs_hip_add_grain_sp_frame_list_dev is not None
    assert C.sizeof(hw.SpFrame) == 2 * C.sizeof(C.c_void_p) and [n for n, _ in hw.SpFrame._fields_] == ["Y", "UV"]
