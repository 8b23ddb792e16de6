"""CPU: vfgs_hip_add_grain_frame_list_models_copy8_dev and vfgs_hip_add_grain_sp_frame_list_models_copy8_dev as a C caller sees them, in the
manner of tests/test_sp_models_abi_cpu.py: a C99 translation unit that includes the public header and takes both functions' addresses
through pointers of the declared types, compiled with -std=c99 -pedantic -Wall -Werror and linked against the built library (the symbols
must resolve); the library's dynamic symbol table exports them; the Python wrappers exist and are bound with the declared argument lists.

The same translation unit, linked over the host layer and the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp instead of
the library (no sanitizer, no device), calls both entries and gets the documented codes from the refusals that need nothing but the host:
null lists, null models, a plane that reaches the 2 GiB window (15), the destination's pitches, depth 8, a bad sample_shift, a destination that is its own source -- and their order
(the list checks with 15 behind them, then 6 / 8 for the destination's pitches, then 16, then 40, then 41).  Values are the GPU suite's business (tests/test_gpu_model_list_out8.py,
tests/test_gpu_sp_model_list_out8.py), lists with live models the sanitizer walks' (tests/sanitize_models_out8)."""
import inspect
import shutil
import subprocess

import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import build as vbuild

SOURCE = r"""
#include <stdio.h>
#include "vfgs_hip.h"

typedef int (*planar_fn)(const vfgs_hip_frame_ptrs*, const vfgs_hip_frame_ptrs*, const vfgs_hip_model* const*, const uint32_t*, unsigned, unsigned,
                         unsigned, unsigned, unsigned, unsigned, unsigned, void*);
typedef int (*sp_fn)(const vfgs_hip_sp_frame*, const vfgs_hip_sp_frame*, const vfgs_hip_model* const*, const uint32_t*, unsigned, unsigned,
                     unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, void*);

static int bad = 0;
#define ADDR(k) ((void*)((uintptr_t)(k) << 24))
#define FAR(k) ((void*)((uintptr_t)(k) << 33))      /* 8 GiB apart: planes of 2 GiB and more that share no byte */
#define EXPECT(call, code) do { const int rc_ = (call); if (rc_ != (code) || (code && vfgs_hip_last_error() != (code))) { \
	printf("line %d: %s -> %d, documented %d (%s)\n", __LINE__, #call, rc_, code, vfgs_hip_last_error_string()); bad++; } } while (0)

int main(int argc, char** argv)
{
	planar_fn p = vfgs_hip_add_grain_frame_list_models_copy8_dev;
	sp_fn s = vfgs_hip_add_grain_sp_frame_list_models_copy8_dev;
	if (!p || !s) return 1;
	if (argc > 1)
	{
		/* the refusals that need nothing but the host: no plane is ever touched, so the planes are addresses, 16 MiB apart */
		vfgs_hip_frame_ptrs src[2], dst[2];
		vfgs_hip_sp_frame ssrc[2], sdst[2];
		const vfgs_hip_model* none[2] = { NULL, NULL };
		const uint32_t seeds[2] = { 1, 2 };
		int f;
		for (f = 0; f < 2; f++)
		{
			src[f].Y = ADDR(1 + 8 * f); src[f].U = ADDR(2 + 8 * f); src[f].V = ADDR(3 + 8 * f);
			dst[f].Y = ADDR(4 + 8 * f); dst[f].U = ADDR(5 + 8 * f); dst[f].V = ADDR(6 + 8 * f);
			ssrc[f].Y = src[f].Y; ssrc[f].UV = src[f].U;
			sdst[f].Y = dst[f].Y; sdst[f].UV = dst[f].U;
		}
		vfgs_hip_reset_state();
		vfgs_set_depth(10);
		vfgs_set_chroma_subsampling(2, 2);
		/* planar: 520 x 70, source pitches 576 / 320 samples, destination pitches 528 / 272 bytes */
		EXPECT(p(NULL, dst, none, seeds, 2, 520, 70, 576, 320, 528, 272, NULL), 18);
		EXPECT(p(src, NULL, none, seeds, 2, 520, 70, 576, 320, 528, 272, NULL), 18);
		EXPECT(p(src, dst, NULL, seeds, 2, 520, 70, 576, 320, 528, 272, NULL), 41);
		EXPECT(p(src, dst, none, NULL, 2, 520, 70, 576, 320, 528, 272, NULL), 41);
		EXPECT(p(src, dst, NULL, seeds, 2, 100, 70, 576, 320, 528, 272, NULL), 5);        /* the list checks come first */
		EXPECT(p(src, dst, NULL, seeds, 2, 520, 70, 512, 320, 528, 272, NULL), 6);
		EXPECT(p(src, dst, NULL, seeds, 2, 520, 70, 576, 324, 528, 272, NULL), 8);
		EXPECT(p(src, dst, NULL, seeds, 2, 520, 70, 576, 320, 512, 272, NULL), 6);        /* the destination's pitches */
		EXPECT(p(src, dst, NULL, seeds, 2, 520, 70, 576, 320, 528, 256, NULL), 6);
		EXPECT(p(src, dst, NULL, seeds, 2, 520, 70, 576, 320, 528, 280, NULL), 8);
		EXPECT(p(src, dst, NULL, seeds, 2, 8208, 70, 8256, 4128, 8256, 4128, NULL), 41);  /* rows walked in parts */
		EXPECT(p(NULL, NULL, NULL, NULL, 0, 100, 70, 0, 0, 0, 0, NULL), 0);               /* an empty list is no call at all */
		vfgs_set_depth(8);
		EXPECT(p(src, dst, NULL, seeds, 2, 520, 70, 576, 320, 528, 272, NULL), 16);       /* 16 before 41 */
		EXPECT(s(ssrc, sdst, NULL, seeds, 2, 520, 70, 576, 576, 528, 528, 6, NULL), 16);  /* ... and before 40 */
		vfgs_set_depth(10);
		/* semi-planar: P010, pitches 576 containers, destination pitches 528 bytes */
		EXPECT(s(NULL, sdst, none, seeds, 2, 520, 70, 576, 576, 528, 528, 6, NULL), 18);
		EXPECT(s(ssrc, sdst, NULL, seeds, 2, 520, 70, 576, 576, 528, 528, 6, NULL), 41);
		EXPECT(s(ssrc, sdst, none, seeds, 2, 520, 70, 576, 576, 528, 528, 0, NULL), 41);
		EXPECT(s(ssrc, sdst, NULL, seeds, 2, 520, 70, 576, 576, 528, 528, 4, NULL), 40);  /* 40 before 41 */
		EXPECT(s(ssrc, sdst, NULL, seeds, 2, 8208, 17, 8256, 8256, 8256, 8256, 6, NULL), 40);
		EXPECT(s(ssrc, sdst, NULL, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 6);   /* a UV row of bytes is as long as the luma row */
		EXPECT(s(ssrc, sdst, NULL, seeds, 2, 520, 70, 576, 576, 536, 528, 6, NULL), 8);
		EXPECT(s(ssrc, ssrc, NULL, seeds, 2, 520, 70, 576, 576, 528, 528, 4, NULL), 18);  /* a destination that is its own source: the list checks come first */
		{
			/* 15: a luma plane of 1864136 rows x 576 containers x 2 bytes reaches the 2 GiB buffer window; after the list checks (a destination
			   that is its own source is still 18), before the destination's pitches (6), depth 8 (16), 40 and 41 */
			vfgs_hip_frame_ptrs bs = { FAR(1), FAR(2), FAR(3) }, bd = { FAR(4), FAR(5), FAR(6) };
			vfgs_hip_sp_frame bss = { FAR(1), FAR(2) }, bsd = { FAR(4), FAR(5) };
			EXPECT(p(&bs, &bd, NULL, seeds, 1, 520, 1864136, 576, 320, 512, 272, NULL), 15);
			EXPECT(s(&bss, &bsd, NULL, seeds, 1, 520, 1864136, 576, 576, 512, 528, 4, NULL), 15);
			EXPECT(s(&bss, &bss, NULL, seeds, 1, 520, 1864136, 576, 576, 512, 528, 4, NULL), 18);
			EXPECT(p(&bs, &bd, NULL, seeds, 1, 520, 1864135, 576, 320, 512, 272, NULL), 6);        /* one row fewer: inside the window */
			vfgs_set_depth(8);
			EXPECT(p(&bs, &bd, NULL, seeds, 1, 520, 2 * 1864136, 576, 320, 528, 272, NULL), 15);   /* ... before 16 */
			vfgs_set_depth(10);
		}
		vfgs_set_chroma_subsampling(1, 1);
		EXPECT(s(ssrc, sdst, NULL, seeds, 2, 520, 70, 576, 1152, 528, 1056, 6, NULL), 40);
		EXPECT(s(NULL, NULL, NULL, NULL, 0, 100, 70, 0, 0, 0, 0, 99, NULL), 0);
		vfgs_hip_shutdown();
		if (bad) return 2;
	}
	puts("abi ok");
	return 0;
}
"""

NAMES = ("vfgs_hip_add_grain_frame_list_models_copy8_dev", "vfgs_hip_add_grain_sp_frame_list_models_copy8_dev")


def compile_c(tmp_path):
    src = tmp_path / "models_out8_abi.c"
    src.write_text(SOURCE)
    obj = tmp_path / "models_out8_abi.o"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{T.ROOT / 'include'}", "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return obj


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c99_caller_compiles_links_and_runs(tmp_path):
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    obj = compile_c(tmp_path)
    exe = tmp_path / "models_out8_abi"
    r = subprocess.run(["gcc", str(obj), "-o", str(exe), f"-L{vbuild.LIB.parent}", "-lvfgs_hip", f"-Wl,-rpath,{vbuild.LIB.parent}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_host_only_refusals_have_the_documented_codes(tmp_path):
    import sanitize_build as S
    if shutil.which("gcc") is None or not S.HAVE_TOOLS:
        pytest.skip("needs gcc, g++ and the HIP headers")
    exe = S.build(tmp_path, "models_out8_refusals", S.PLAIN, [compile_c(tmp_path)])
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


def test_the_python_wrappers_exist():
    from versatilefilmgrain_amd import hw
    assert list(inspect.signature(hw.VfgsHip.add_grain_frame_list_models_copy8_dev).parameters) == \
        ["self", "src", "dst", "models", "seeds", "width", "height", "stride", "cstride", "dstride", "dcstride", "stream"]
    assert list(inspect.signature(hw.VfgsHip.add_grain_sp_frame_list_models_copy8_dev).parameters) == \
        ["self", "src", "dst", "models", "seeds", "width", "height", "stride", "uv_stride", "dst_stride", "dst_uv_stride", "sample_shift", "stream"]
    lib = hw.load()
    assert len(lib.vfgs_hip_add_grain_frame_list_models_copy8_dev.argtypes) == 12
    assert len(lib.vfgs_hip_add_grain_sp_frame_list_models_copy8_dev.argtypes) == 13
