"""CPU: vfgs_hip_host_pipe_open / _submit / _wait / _close as a C caller sees them, in the manner of tests/test_models_out8_abi_cpu.py: a C99
translation unit that includes the public header, fills a vfgs_hip_host_pipe_desc and takes the four functions' addresses through pointers of
the declared types, compiled with -std=c99 -pedantic -Wall -Werror and linked against the built library (the symbols must resolve); the
library's dynamic symbol table exports them; the Python wrapper exists and is bound with the declared argument lists.

The same translation unit, linked over the host layer and the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp instead of the
library (no sanitizer, no device), gets the documented codes from the refusals that need nothing but the host, opens a pipe, sends one
picture through it and collects it.  Values are the GPU suite's business (tests/test_gpu_host_pipe.py), streams of pictures the sanitizer
walks' (tests/sanitize_host_pipe)."""
import inspect
import shutil
import subprocess

import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import build as vbuild

SOURCE = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vfgs_hip.h"

typedef int (*open_fn)(const vfgs_hip_host_pipe_desc*, vfgs_hip_host_pipe**);
typedef int (*submit_fn)(vfgs_hip_host_pipe*, const vfgs_hip_frame_ptrs*, const vfgs_hip_frame_ptrs*, const vfgs_hip_model*, const uint32_t*, uint64_t*);
typedef int (*wait_fn)(vfgs_hip_host_pipe*, uint64_t);
typedef int (*close_fn)(vfgs_hip_host_pipe*);

static int bad = 0;
#define EXPECT(call, code) do { const int rc_ = (call); if (rc_ != (code) || (code && vfgs_hip_last_error() != (code))) { \
	printf("line %d: %s -> %d, documented %d (%s)\n", __LINE__, #call, rc_, code, vfgs_hip_last_error_string()); bad++; } } while (0)

int main(int argc, char** argv)
{
	open_fn o = vfgs_hip_host_pipe_open;
	submit_fn s = vfgs_hip_host_pipe_submit;
	wait_fn w = vfgs_hip_host_pipe_wait;
	close_fn c = vfgs_hip_host_pipe_close;
	vfgs_hip_host_pipe_desc d;
	if (!o || !s || !w || !c) return 1;
	memset(&d, 0, sizeof d);
	d.width = 200; d.height = 40; d.stride = 208; d.cstride = 112;
	d.dst_stride = 208; d.dst_cstride = 112; d.dst8 = 1; d.slots = 0;
	if (argc > 1)
	{
		vfgs_hip_host_pipe* p = (vfgs_hip_host_pipe*)&d;
		vfgs_hip_host_pipe_desc x;
		vfgs_hip_frame_ptrs src, dst;
		uint64_t t = 7;
		size_t i;
		unsigned char lut[256];
		vfgs_hip_reset_state();
		vfgs_set_depth(10);
		vfgs_set_chroma_subsampling(2, 2);
		EXPECT(o(NULL, &p), 43);
		if (p != NULL) { puts("a refused open leaves a handle"); bad++; }
		EXPECT(o(&d, NULL), 43);
		x = d; x.slots = 1; EXPECT(o(&x, &p), 43);
		x = d; x.slots = 9; EXPECT(o(&x, &p), 43);
		x = d; x.dst_stride = 0; x.dst_cstride = 0; EXPECT(o(&x, &p), 43);
		x = d; x.dst_cstride = 0; EXPECT(o(&x, &p), 43);
		x = d; x.width = 128; EXPECT(o(&x, &p), 5);
		x = d; x.width = 31760; EXPECT(o(&x, &p), 17);
		x = d; x.stride = 200; EXPECT(o(&x, &p), 6);
		x = d; x.cstride = 116; EXPECT(o(&x, &p), 8);
		x = d; x.dst_cstride = 96; EXPECT(o(&x, &p), 6);
		x = d; x.dst_stride = 216; EXPECT(o(&x, &p), 8);
		x = d; x.height = 5200000; EXPECT(o(&x, &p), 15);
		vfgs_set_depth(8);
		EXPECT(o(&d, &p), 16);
		vfgs_set_depth(10);
		EXPECT(s(NULL, &src, &dst, NULL, NULL, &t), 43);
		EXPECT(s((vfgs_hip_host_pipe*)&d, &src, &dst, NULL, NULL, &t), 43);      /* never a pipe: refused, not dereferenced */
		EXPECT(w((vfgs_hip_host_pipe*)&d, 1), 43);
		EXPECT(c((vfgs_hip_host_pipe*)&d), 43);
		EXPECT(c(NULL), 43);
		/* one picture: 10-bit 4:2:0 in, bytes out */
		src.Y = malloc(40 * 208 * 2); src.U = malloc(20 * 112 * 2); src.V = malloc(20 * 112 * 2);
		dst.Y = malloc(40 * 208); dst.U = malloc(20 * 112); dst.V = malloc(20 * 112);
		memset(src.Y, 1, 40 * 208 * 2); memset(src.U, 1, 20 * 112 * 2); memset(src.V, 1, 20 * 112 * 2);
		memset(dst.Y, 0xa5, 40 * 208); memset(dst.U, 0xa5, 20 * 112); memset(dst.V, 0xa5, 20 * 112);
		memset(lut, 0x10, sizeof lut);
		for (i = 0; i < 3; i++) vfgs_set_pattern_lut((int)i, lut);
		EXPECT(o(&d, &p), 0);
		if (p == NULL) return 3;
		EXPECT(s(p, &src, NULL, NULL, NULL, &t), 43);
		EXPECT(s(p, NULL, &dst, NULL, NULL, &t), 43);
		EXPECT(s(p, &src, &dst, NULL, NULL, NULL), 43);
		EXPECT(s(p, &src, &src, NULL, NULL, &t), 18);
		EXPECT(s(p, &src, &dst, (const vfgs_hip_model*)&d, NULL, &t), 41);           /* never a model */
		EXPECT(w(p, 1), 43);
		if (t != 7) { puts("a refused submit wrote a ticket"); bad++; }
		EXPECT(s(p, &src, &dst, NULL, NULL, &t), 0);
		if (t != 1) { puts("the first ticket is 1"); bad++; }
		EXPECT(w(p, 2), 43);
		EXPECT(w(p, 1), 0);
		EXPECT(w(p, 1), 0);
		/* (0x0101 + 2) >> 2 = 64 in the whole blocks of every row, the fill behind them */
		if (((unsigned char*)dst.Y)[0] != 64 || ((unsigned char*)dst.U)[111] != 0xa5 || ((unsigned char*)dst.V)[19 * 112 + 103] != 64) { puts("the picture did not come home"); bad++; }
		EXPECT(c(p), 0);
		EXPECT(c(p), 43);
		free(src.Y); free(src.U); free(src.V); free(dst.Y); free(dst.U); free(dst.V);
		vfgs_hip_shutdown();
		if (bad) return 2;
	}
	puts("abi ok");
	return 0;
}
"""

NAMES = ("vfgs_hip_host_pipe_open", "vfgs_hip_host_pipe_submit", "vfgs_hip_host_pipe_wait", "vfgs_hip_host_pipe_close")


def compile_c(tmp_path):
    src = tmp_path / "host_pipe_abi.c"
    src.write_text(SOURCE)
    obj = tmp_path / "host_pipe_abi.o"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{T.ROOT / 'include'}", "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return obj


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c99_caller_compiles_links_and_runs(tmp_path):
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    obj = compile_c(tmp_path)
    exe = tmp_path / "host_pipe_abi"
    r = subprocess.run(["gcc", str(obj), "-o", str(exe), f"-L{vbuild.LIB.parent}", "-lvfgs_hip", f"-Wl,-rpath,{vbuild.LIB.parent}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_host_only_refusals_and_one_picture(tmp_path):
    import sanitize_build as S
    if shutil.which("gcc") is None or not S.HAVE_TOOLS:
        pytest.skip("needs gcc, g++ and the HIP headers")
    exe = S.build(tmp_path, "host_pipe_refusals", S.PLAIN, [compile_c(tmp_path)])
    r = subprocess.run([str(exe), "refusals"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_the_symbols_are_exported_and_declared():
    import ctypes as C
    from versatilefilmgrain_amd import hw
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    header = (T.ROOT / "include" / "vfgs_hip.h").read_text()
    lib = C.CDLL(str(vbuild.LIB))
    for name in NAMES:
        assert name in hw.EXPORTS and getattr(lib, name) is not None and f" {name}(" in header


def test_the_python_wrapper_exists():
    import ctypes as C
    from versatilefilmgrain_amd import hw
    assert list(inspect.signature(hw.VfgsHip.host_pipe).parameters) == \
        ["self", "width", "height", "stride", "cstride", "dst_stride", "dst_cstride", "dst8", "slots"]
    assert list(inspect.signature(hw.HostPipe.submit).parameters) == ["self", "src", "dst", "model", "seed"]
    assert all(hasattr(hw.HostPipe, n) for n in ("wait", "close", "__enter__", "__exit__"))
    assert [n for n, _ in hw.HostPipeDesc._fields_] == ["width", "height", "stride", "cstride", "dst_stride", "dst_cstride", "dst8", "slots"]
    assert C.sizeof(hw.HostPipeDesc) == 32
    lib = hw.load()
    assert len(lib.vfgs_hip_host_pipe_submit.argtypes) == 6 and len(lib.vfgs_hip_host_pipe_open.argtypes) == 2
