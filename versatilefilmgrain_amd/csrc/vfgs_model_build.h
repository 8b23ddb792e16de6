// Shared between vfgs_model_build_host.cpp (the entry point vfgs_hip_models_from_afgs1), vfgs_host.cpp (the model bookkeeping: slabs,
// handles, events) and vfgs_fw_kernel.hip (fw_models_kernel): film grain models built on the device straight from AFGS1 parameter
// sets, a chunk of models per launch (include/vfgs_hip_fw.h).
//
// vfgs_host.cpp never names the launcher: the entry point hands it down as a pointer, so a program that links the host layer
// without vfgs_fw_kernel.hip (the sanitizer walks under tests/, against their model of the HIP runtime) links as before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfgs_fw_layout.h"
#include "vfgs_layout.h"

struct vfgs_hip_model;

namespace vfgs {

constexpr int kFwModelChunk = 32;     // models per launch of fw_models_kernel (one workgroup each) and per slab

// LDS of fw_models_kernel: the 82x73 luma and the 44x38 Cb buffer of the recursion, each inside guard zones of 256 bytes in front and 128
// behind (the chroma arena holds 64 rows: every lane of its wavefront reads "its" row), the Gaussian table, two LFSR streams
constexpr int kFwArenaLuma = (256 + 82 * 73 + 128 + 15) & ~15;
constexpr int kFwArenaChroma = 256 + 64 * 44 + 128;
constexpr int kFwModelsLdsBytes = kFwArenaLuma + kFwArenaChroma + 2048 + 2 * kFwStreamWords * 4;     // 13168
static_assert(kFwModelsLdsBytes == 13168, "tests/test_code_object_model_build_cpu.py reads the group segment of the built kernel against this");

// What ONE model is made from: everything fw_models_kernel needs beyond the constants.  The entry point fills the parameter-set side
// (taps, shifts, scale bytes, range); the bookkeeping adds what depends on the programmed depth and format (record, form, dst).
struct FwModelJob {
	uint8_t* dst;             // device: this model's ModelRecord, the table image behind it (16-byte aligned)
	ModelRecord rec;          // the first 32 bytes at dst
	int16_t coef[2][28];      // luma, Cb: the 4x7 causal taps as vfgs_hip_pattern_job::coef holds them (Cr's pattern is never selected)
	int32_t lag;              // 1..3: how far the taps reach
	int32_t scale, shift;     // right shift of the filter sum (ar_coeff_shift), of the Gaussian sample (grain_scale_shift + 1)
	int32_t one_y, one_c;     // form of the image (image_layout)
	int32_t scale_shift;      // the hardware layer's stored shift (vfgs_hw.c:349): pre-shift of the general / wide LUT entries
	int32_t legal;            // clip_to_restricted_range (host only)
	int32_t reserved[3];
	uint8_t slut[3][256];     // scale bytes of Y, Cb, Cr
};
static_assert(sizeof(FwModelJob) % 16 == 0, "jobs of a table are read with aligned scalar and vector loads");

// one launch: jobs[0..n) of a device job table, n <= kFwModelChunk; depth8: one-pattern components take the packed 16-bit form
typedef hipError_t (*FwModelsLauncher)(const FwConstants* k, const FwModelJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream);
hipError_t launch_fw_models(const FwConstants* k, const FwModelJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream);

// vfgs_host.cpp: build jobs[0..n) (parameter-set side filled in, refusals of the parameter sets already made) into n live models at
// the programmed depth and format; out[0..n) are all set, or all NULL with an error code.  who: the entry's name for messages.
int build_models(const char* who, FwModelJob* jobs, unsigned n, vfgs_hip_model** out, void* stream, FwModelsLauncher launch);

int set_error(int code, const char* msg);

}  // namespace vfgs
