"""CPU: vfgs_hip_add_grain_sp_frame_list_models_dev as a C caller sees it: a C99 translation unit that includes the public header and takes
the function's address through a pointer of the declared type, compiled with -std=c99 -pedantic -Wall -Werror and linked against the built
library (the symbol must resolve); the library's dynamic symbol table exports it; the Python wrapper exists and is bound with the declared
argument list.  Everything else sits behind the library's initialisation, which needs a device: the GPU suite's
(tests/test_gpu_sp_model_list.py) and the sanitizer walks' (tests/sanitize_sp_models)."""
import inspect
import shutil
import subprocess

import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import build as vbuild

SOURCE = r"""
#include <stdio.h>
#include "vfgs_hip.h"

typedef int (*call_fn)(const vfgs_hip_sp_frame*, const vfgs_hip_sp_frame*, const vfgs_hip_model* const*, const uint32_t*, unsigned, unsigned,
                       unsigned, unsigned, unsigned, unsigned, void*);

int main(void)
{
	call_fn f = vfgs_hip_add_grain_sp_frame_list_models_dev;
	const vfgs_hip_model* const list[1] = { NULL };
	vfgs_hip_sp_frame fr = { NULL, NULL };
	if (!f || list[0] || fr.Y || fr.UV) return 1;
	puts("abi ok");
	return 0;
}
"""

NAME = "vfgs_hip_add_grain_sp_frame_list_models_dev"


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c99_caller_compiles_links_and_runs(tmp_path):
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    src = tmp_path / "sp_models_abi.c"
    src.write_text(SOURCE)
    exe = tmp_path / "sp_models_abi"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{T.ROOT / 'include'}", str(src), "-o", str(exe),
                        f"-L{vbuild.LIB.parent}", "-lvfgs_hip", f"-Wl,-rpath,{vbuild.LIB.parent}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_the_symbol_is_exported_and_declared():
    import ctypes as C
    from versatilefilmgrain_amd import hw
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    assert NAME in hw.EXPORTS
    assert getattr(C.CDLL(str(vbuild.LIB)), NAME) is not None
    header = (T.ROOT / "include" / "vfgs_hip.h").read_text()
    assert f" {NAME}(" in header


def test_the_python_wrapper_exists():
    from versatilefilmgrain_amd import hw
    assert list(inspect.signature(hw.VfgsHip.add_grain_sp_frame_list_models_dev).parameters) == \
        ["self", "src", "dst", "models", "seeds", "width", "height", "stride", "uv_stride", "sample_shift", "stream"]
    lib = hw.load()
    assert len(lib.vfgs_hip_add_grain_sp_frame_list_models_dev.argtypes) == 11
