"""CPU: models as device objects as a C caller sees them: a C99 translation unit that includes the public header and takes the addresses
of vfgs_hip_model_capture, _release, _info and vfgs_hip_add_grain_frame_list_models_dev with their declared types, compiled with -std=c99
-pedantic -Wall -Werror and linked against the built library (the symbols must resolve); the library's dynamic symbol table exports them;
the Python wrappers exist and are bound with the declared argument lists.  Everything else sits behind the library's initialisation, which
needs a device: the GPU suite's (tests/test_gpu_model_list.py) and the sanitizer walks' (tests/sanitize_models)."""
import inspect
import shutil
import subprocess

import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import build as vbuild

SOURCE = r"""
#include <stdio.h>
#include "vfgs_hip.h"

typedef int (*capture_fn)(vfgs_hip_model**, void*);
typedef void (*release_fn)(vfgs_hip_model*);
typedef int (*info_fn)(const vfgs_hip_model*, int[8]);
typedef int (*call_fn)(const vfgs_hip_frame_ptrs*, const vfgs_hip_frame_ptrs*, const vfgs_hip_model* const*, const uint32_t*, unsigned, unsigned,
                       unsigned, unsigned, unsigned, void*);

int main(void)
{
	capture_fn c = vfgs_hip_model_capture;
	release_fn r = vfgs_hip_model_release;
	info_fn i = vfgs_hip_model_info;
	call_fn f = vfgs_hip_add_grain_frame_list_models_dev;
	vfgs_hip_model* m = NULL;
	const vfgs_hip_model* const list[1] = { NULL };
	if (!c || !r || !i || !f || m || list[0]) return 1;
	r(NULL);      /* a no-op that needs no device */
	puts("abi ok");
	return 0;
}
"""

NAMES = ("vfgs_hip_model_capture", "vfgs_hip_model_release", "vfgs_hip_model_info", "vfgs_hip_add_grain_frame_list_models_dev")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c99_caller_compiles_links_and_runs(tmp_path):
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    src = tmp_path / "models_abi.c"
    src.write_text(SOURCE)
    exe = tmp_path / "models_abi"
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
    assert f" {name}(" in header and "typedef struct vfgs_hip_model vfgs_hip_model;" in header


def test_the_python_wrappers_exist():
    from versatilefilmgrain_amd import hw
    assert list(inspect.signature(hw.VfgsHip.model_capture).parameters) == ["self", "stream"]
    assert list(inspect.signature(hw.VfgsHip.model_release).parameters) == ["self", "m"]
    assert list(inspect.signature(hw.VfgsHip.model_info).parameters) == ["self", "m"]
    assert list(inspect.signature(hw.VfgsHip.add_grain_frame_list_models_dev).parameters) == \
        ["self", "src", "dst", "models", "seeds", "width", "height", "stride", "cstride", "stream"]
    lib = hw.load()
    assert len(lib.vfgs_hip_model_capture.argtypes) == 2 and len(lib.vfgs_hip_model_release.argtypes) == 1
    assert len(lib.vfgs_hip_model_info.argtypes) == 2 and len(lib.vfgs_hip_add_grain_frame_list_models_dev.argtypes) == 10
