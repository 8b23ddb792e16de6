"""CPU: the semi-planar call with the narrowed 8-bit destination as a C caller sees it: a C99 translation unit that includes the public
header and takes the address of vfgs_hip_add_grain_sp_frame_list_copy8_dev with its declared type, compiled with -std=c99 -pedantic -Wall
-Werror and linked against the built library (the symbol must resolve); the library's dynamic symbol table exports it; the Python wrapper
exists and is bound with the declared argument list."""
import inspect
import shutil
import subprocess

import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import build as vbuild

SOURCE = r"""
#include <stdio.h>
#include "vfgs_hip.h"

typedef int (*sp8_fn)(const vfgs_hip_sp_frame*, const vfgs_hip_sp_frame*, const uint32_t*, unsigned, unsigned, unsigned, unsigned, unsigned,
                      unsigned, unsigned, unsigned, void*);

int main(void)
{
	sp8_fn f = vfgs_hip_add_grain_sp_frame_list_copy8_dev;
	vfgs_hip_sp_frame fr;
	fr.Y = NULL;
	fr.UV = NULL;
	if (!f || fr.Y || fr.UV) return 1;
	puts("abi ok");
	return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c99_caller_compiles_links_and_runs(tmp_path):
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    src = tmp_path / "sp8_abi.c"
    src.write_text(SOURCE)
    exe = tmp_path / "sp8_abi"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{T.ROOT / 'include'}", str(src), "-o", str(exe),
                        f"-L{vbuild.LIB.parent}", "-lvfgs_hip", f"-Wl,-rpath,{vbuild.LIB.parent}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_the_symbol_is_exported_and_declared():
    import ctypes as C
    from versatilefilmgrain_amd import hw
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    name = "vfgs_hip_add_grain_sp_frame_list_copy8_dev"
    assert name in hw.EXPORTS
    assert getattr(C.CDLL(str(vbuild.LIB)), name) is not None
    header = (T.ROOT / "include" / "vfgs_hip.h").read_text()
    assert f"int {name}(const vfgs_hip_sp_frame* src, const vfgs_hip_sp_frame* dst," in header


def test_the_python_wrapper_exists():
    from versatilefilmgrain_amd import hw
    params = list(inspect.signature(hw.VfgsHip.add_grain_sp_frame_list_copy8_dev).parameters)
    assert params == ["self", "src", "dst", "seeds", "width", "height", "stride", "uv_stride", "dst_stride", "dst_uv_stride", "sample_shift", "stream"]
    lib = hw.load()
    assert len(lib.vfgs_hip_add_grain_sp_frame_list_copy8_dev.argtypes) == 12
