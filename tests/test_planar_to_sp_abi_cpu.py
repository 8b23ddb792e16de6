"""CPU: the planar-to-semi-planar calls as a C caller sees them: a C99 translation unit that includes the public header and takes the
addresses of vfgs_hip_add_grain_frame_list_to_sp_dev and _to_sp8_dev with their declared types, compiled with -std=c99 -pedantic -Wall
-Werror and linked against the built library (the symbols must resolve); the library's dynamic symbol table exports both; the Python
wrappers exist and are bound with the declared argument lists.  The refusals all sit behind the library's initialisation, which needs a
device, so they are the GPU suite's (tests/test_gpu_planar_to_sp.py) and the sanitizer walks' (tests/sanitize_p2sp)."""
import inspect
import shutil
import subprocess

import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import build as vbuild

SOURCE = r"""
#include <stdio.h>
#include "vfgs_hip.h"

typedef int (*to_sp_fn)(const vfgs_hip_frame_ptrs*, const vfgs_hip_sp_frame*, const uint32_t*, unsigned, unsigned, unsigned, unsigned, unsigned,
                        unsigned, unsigned, unsigned, void*);
typedef int (*to_sp8_fn)(const vfgs_hip_frame_ptrs*, const vfgs_hip_sp_frame*, const uint32_t*, unsigned, unsigned, unsigned, unsigned, unsigned,
                         unsigned, unsigned, void*);

int main(void)
{
	to_sp_fn f = vfgs_hip_add_grain_frame_list_to_sp_dev;
	to_sp8_fn g = vfgs_hip_add_grain_frame_list_to_sp8_dev;
	vfgs_hip_frame_ptrs s;
	vfgs_hip_sp_frame d;
	s.Y = s.U = s.V = NULL;
	d.Y = d.UV = NULL;
	if (!f || !g || s.Y || d.UV) return 1;
	puts("abi ok");
	return 0;
}
"""

NAMES = ("vfgs_hip_add_grain_frame_list_to_sp_dev", "vfgs_hip_add_grain_frame_list_to_sp8_dev")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c99_caller_compiles_links_and_runs(tmp_path):
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    src = tmp_path / "p2sp_abi.c"
    src.write_text(SOURCE)
    exe = tmp_path / "p2sp_abi"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{T.ROOT / 'include'}", str(src), "-o", str(exe),
                        f"-L{vbuild.LIB.parent}", "-lvfgs_hip", f"-Wl,-rpath,{vbuild.LIB.parent}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("name", NAMES)
def test_the_symbol_is_exported_and_declared(name):
    import ctypes as C
    from versatilefilmgrain_amd import hw
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    assert name in hw.EXPORTS
    assert getattr(C.CDLL(str(vbuild.LIB)), name) is not None
    header = (T.ROOT / "include" / "vfgs_hip.h").read_text()
    assert f"int {name}(const vfgs_hip_frame_ptrs* src" in header


def test_the_python_wrappers_exist():
    from versatilefilmgrain_amd import hw
    common = ["self", "src", "dst", "seeds", "width", "height", "stride", "cstride", "dst_stride", "dst_uv_stride"]
    assert list(inspect.signature(hw.VfgsHip.add_grain_frame_list_to_sp_dev).parameters) == common + ["sample_shift", "stream"]
    assert list(inspect.signature(hw.VfgsHip.add_grain_frame_list_to_sp8_dev).parameters) == common + ["stream"]
    lib = hw.load()
    assert len(lib.vfgs_hip_add_grain_frame_list_to_sp_dev.argtypes) == 12
    assert len(lib.vfgs_hip_add_grain_frame_list_to_sp8_dev.argtypes) == 11
