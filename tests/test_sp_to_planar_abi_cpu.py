"""CPU: vfgs_hip_add_grain_sp_frame_list_to_planar_dev and vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev as a C caller sees them, in
the manner of tests/test_models_to_sp_abi_cpu.py: a C99 translation unit that includes the public header and takes both functions'
addresses through pointers of the declared types, compiled with -std=c99 -pedantic -Wall -Werror and linked against the built library (the
symbols must resolve); the library's dynamic symbol table exports them; the Python wrappers exist and are bound with the declared argument
lists.

The same translation unit, linked over the host layer and the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp instead of
the library (no sanitizer, no device), calls both entries and gets the documented codes from the refusals that need nothing but the host,
and their order: 40, then 18 for a null list, then 6 / 8 for the destination's pitches, then the list checks, then 15, then 41.  Values are
the GPU suite's business (tests/test_gpu_sp_to_planar.py), served lists the sanitizer walks' (tests/sanitize_sp_to_planar)."""
import inspect
import shutil
import subprocess

import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import build as vbuild

SOURCE = r"""
#include <stdio.h>
#include "vfgs_hip.h"

typedef int (*to_planar_fn)(const vfgs_hip_sp_frame*, const vfgs_hip_frame_ptrs*, const uint32_t*, unsigned, unsigned, unsigned, unsigned, unsigned,
                            unsigned, unsigned, unsigned, void*);
typedef int (*models_to_planar_fn)(const vfgs_hip_sp_frame*, const vfgs_hip_frame_ptrs*, const vfgs_hip_model* const*, const uint32_t*, unsigned,
                                   unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, void*);

static int bad = 0;
#define ADDR(k) ((void*)((uintptr_t)(k) << 24))
#define FAR(k) ((void*)((uintptr_t)(k) << 33))      /* 8 GiB apart: planes of 2 GiB and more that share no byte */
#define EXPECT(call, code) do { const int rc_ = (call); if (rc_ != (code) || (code && vfgs_hip_last_error() != (code))) { \
	printf("line %d: %s -> %d, documented %d (%s)\n", __LINE__, #call, rc_, code, vfgs_hip_last_error_string()); bad++; } } while (0)

int main(int argc, char** argv)
{
	to_planar_fn p = vfgs_hip_add_grain_sp_frame_list_to_planar_dev;
	models_to_planar_fn m = vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev;
	if (!p || !m) return 1;
	if (argc > 1)
	{
		/* the refusals that need nothing but the host: no plane is ever touched, so the planes are addresses, 16 MiB apart */
		vfgs_hip_sp_frame src[2];
		vfgs_hip_frame_ptrs dst[2];
		const vfgs_hip_model* none[2] = { NULL, NULL };
		const uint32_t seeds[2] = { 1, 2 };
		int f;
		for (f = 0; f < 2; f++)
		{
			src[f].Y = ADDR(1 + 8 * f); src[f].UV = ADDR(2 + 8 * f);
			dst[f].Y = ADDR(3 + 8 * f); dst[f].U = ADDR(4 + 8 * f); dst[f].V = ADDR(5 + 8 * f);
		}
		vfgs_hip_reset_state();
		vfgs_set_depth(10);
		vfgs_set_chroma_subsampling(2, 2);
		/* 520 x 70, source pitches 576 / 576 containers, destination pitches 528 / 272 samples */
		EXPECT(p(NULL, dst, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 18);
		EXPECT(p(src, NULL, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 18);
		EXPECT(m(NULL, dst, none, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 18);
		EXPECT(m(src, dst, NULL, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 41);
		EXPECT(m(src, dst, none, NULL, 2, 520, 70, 576, 576, 528, 272, 0, NULL), 41);
		/* 40 in front of everything */
		EXPECT(p(NULL, NULL, seeds, 2, 520, 70, 576, 576, 8, 8, 4, NULL), 40);
		EXPECT(p(NULL, dst, seeds, 2, 8208, 17, 8256, 8256, 8256, 4128, 6, NULL), 40);
		EXPECT(m(src, NULL, NULL, seeds, 2, 8208, 17, 8256, 8256, 8256, 4128, 6, NULL), 40);
		/* a null list in front of the destination's pitches, those in front of the list checks, the list checks in front of 15 and 41 */
		EXPECT(p(NULL, dst, seeds, 2, 520, 70, 576, 576, 512, 272, 6, NULL), 18);
		EXPECT(p(src, dst, seeds, 2, 100, 70, 576, 576, 96, 272, 6, NULL), 6);
		EXPECT(p(src, dst, seeds, 2, 520, 70, 576, 576, 528, 256, 6, NULL), 6);        /* ONE component's row is half as many samples as the luma row */
		EXPECT(m(src, dst, NULL, seeds, 2, 520, 70, 576, 576, 528, 256, 6, NULL), 6);
		EXPECT(p(src, dst, seeds, 2, 100, 70, 576, 576, 532, 272, 6, NULL), 8);
		EXPECT(m(src, dst, NULL, seeds, 2, 100, 70, 576, 576, 528, 276, 6, NULL), 8);
		EXPECT(p(src, dst, seeds, 2, 100, 70, 576, 576, 528, 272, 6, NULL), 5);
		EXPECT(p(src, dst, seeds, 2, 520, 70, 512, 576, 528, 272, 6, NULL), 6);
		EXPECT(p(src, dst, seeds, 2, 520, 70, 576, 512, 528, 272, 6, NULL), 6);        /* a UV row is as many containers as the luma row */
		EXPECT(m(src, dst, NULL, seeds, 2, 520, 70, 580, 576, 528, 272, 6, NULL), 8);
		{
			vfgs_hip_frame_ptrs own[2];
			own[0] = dst[0]; own[1] = dst[1]; own[1].U = src[1].UV;
			EXPECT(p(src, own, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 18);    /* a destination that is its own source: no in-place form */
			own[1] = dst[1]; own[1].Y = src[0].Y;
			EXPECT(m(src, own, NULL, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 18);   /* ... another frame's source */
			own[1] = dst[1]; own[1].V = own[1].U;
			EXPECT(p(src, own, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 18);    /* U and V the same plane */
			own[1] = dst[0];
			EXPECT(p(src, own, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 18);    /* a destination listed twice */
			own[1] = dst[1]; own[1].V = NULL;
			EXPECT(p(src, own, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 18);    /* a null plane */
			own[1] = dst[1]; own[1].V = (char*)dst[1].V + 8;
			EXPECT(p(src, own, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 7);
		}
		{
			/* 15: a luma plane of 1864136 rows x 576 containers x 2 bytes reaches the 2 GiB buffer window; behind the list checks, in front of 41 */
			vfgs_hip_sp_frame bs = { FAR(1), FAR(2) };
			vfgs_hip_frame_ptrs bd = { FAR(3), FAR(4), FAR(5) };
			EXPECT(m(&bs, &bd, NULL, seeds, 1, 520, 1864136, 576, 576, 528, 272, 6, NULL), 15);
			EXPECT(m(&bs, &bd, NULL, seeds, 1, 520, 1864135, 576, 576, 528, 272, 6, NULL), 41);   /* one row fewer: inside the window */
		}
		EXPECT(p(NULL, NULL, NULL, 0, 100, 70, 0, 0, 0, 0, 99, NULL), 0);               /* an empty list is no call at all */
		EXPECT(m(NULL, NULL, NULL, NULL, 0, 100, 70, 0, 0, 0, 0, 99, NULL), 0);
		vfgs_set_depth(8);
		EXPECT(p(src, dst, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 40);        /* a shift at depth 8 */
		EXPECT(m(src, dst, NULL, seeds, 2, 520, 70, 576, 576, 528, 272, 0, NULL), 41);  /* NV12 to yuv420p: served by this call */
		vfgs_set_depth(10);
		vfgs_set_chroma_subsampling(1, 1);
		EXPECT(p(src, dst, seeds, 2, 520, 70, 576, 576, 528, 528, 6, NULL), 40);
		EXPECT(m(src, dst, NULL, seeds, 2, 520, 70, 576, 576, 528, 528, 6, NULL), 40);
		vfgs_set_chroma_subsampling(2, 2);
		/* a programmed chroma mix: 40 in the programmed call, "chroma mix" in the message; 41 with models */
		if (vfgs_hip_set_chroma_mix(1, 32, 32, 0)) bad++;
		EXPECT(p(src, dst, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 40);
		{
			const char* msg = vfgs_hip_last_error_string();
			int k, hit = 0;
			for (k = 0; msg && msg[k]; k++)
				if (msg[k] == 'c' && msg[k + 1] == 'h' && msg[k + 2] == 'r' && msg[k + 3] == 'o' && msg[k + 4] == 'm' && msg[k + 5] == 'a' && msg[k + 6] == ' ' && msg[k + 7] == 'm') hit = 1;
			if (!hit) { printf("the refusal of a programmed mix does not name it: %s\n", msg ? msg : "(null)"); bad++; }
		}
		EXPECT(m(src, dst, none, seeds, 2, 520, 70, 576, 576, 528, 272, 6, NULL), 41);
		vfgs_hip_clear_chroma_mix();
		vfgs_hip_shutdown();
		if (bad) return 2;
	}
	puts("abi ok");
	return 0;
}
"""

NAMES = ("vfgs_hip_add_grain_sp_frame_list_to_planar_dev", "vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev")


def compile_c(tmp_path):
    src = tmp_path / "sp_to_planar_abi.c"
    src.write_text(SOURCE)
    obj = tmp_path / "sp_to_planar_abi.o"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{T.ROOT / 'include'}", "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return obj


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c99_caller_compiles_links_and_runs(tmp_path):
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    obj = compile_c(tmp_path)
    exe = tmp_path / "sp_to_planar_abi"
    r = subprocess.run(["gcc", str(obj), "-o", str(exe), f"-L{vbuild.LIB.parent}", "-lvfgs_hip", f"-Wl,-rpath,{vbuild.LIB.parent}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_host_only_refusals_have_the_documented_codes(tmp_path):
    import sanitize_build as S
    if shutil.which("gcc") is None or not S.HAVE_TOOLS:
        pytest.skip("needs gcc, g++ and the HIP headers")
    exe = S.build(tmp_path, "sp_to_planar_refusals", S.PLAIN, [compile_c(tmp_path)])
    r = subprocess.run([str(exe), "refusals"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_the_symbols_are_in_the_dynamic_symbol_table_and_declared():
    import ctypes as C
    from versatilefilmgrain_amd import hw
    assert vbuild.LIB.exists(), "libvfgs_hip.so has not been built"
    header = (T.ROOT / "include" / "vfgs_hip.h").read_text()
    lib = C.CDLL(str(vbuild.LIB))
    for name in NAMES:
        assert name in hw.EXPORTS and getattr(lib, name) is not None and f" {name}(" in header
    nm = shutil.which("nm")
    if nm:
        table = subprocess.run([nm, "-D", "--defined-only", str(vbuild.LIB)], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert f" T {name}\n" in table, name


def test_the_python_wrappers_exist_behind_the_layout_ledgers_last_entry():
    from versatilefilmgrain_amd import hw
    assert list(inspect.signature(hw.VfgsHip.add_grain_sp_frame_list_to_planar_dev).parameters) == \
        ["self", "src", "dst", "seeds", "width", "height", "stride", "uv_stride", "dst_stride", "dst_cstride", "sample_shift", "stream"]
    assert list(inspect.signature(hw.VfgsHip.add_grain_sp_frame_list_models_to_planar_dev).parameters) == \
        ["self", "src", "dst", "models", "seeds", "width", "height", "stride", "uv_stride", "dst_stride", "dst_cstride", "sample_shift", "stream"]
    lib = hw.load()
    assert len(lib.vfgs_hip_add_grain_sp_frame_list_to_planar_dev.argtypes) == 12
    assert len(lib.vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev.argtypes) == 13
    # (tests/test_layout_cases_cpu.py slices the class's add_grain_* methods up to add_grain_frame_list_models_to_sp8_dev)
    names = [n for n in vars(hw.VfgsHip) if n.startswith("add_grain_")]
    assert names.index("add_grain_sp_frame_list_to_planar_dev") > names.index("add_grain_frame_list_models_to_sp8_dev")
