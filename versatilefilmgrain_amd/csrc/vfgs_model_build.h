// Shared between vfgs_model_build_host.cpp and vfgs_model_build_sei_host.cpp (the entry points vfgs_hip_models_from_afgs1 and
// vfgs_hip_models_from_sei), vfgs_host.cpp (the model bookkeeping: slabs, handles, events) and vfgs_fw_kernel.hip (fw_models_kernel,
// fw_sei_build_kernel): film grain models built on the device straight from AFGS1 parameter sets or FGC SEI messages, a chunk of models
// per launch (include/vfgs_hip_fw.h).
//
// vfgs_host.cpp never names a launcher: the entry point hands it down as a pointer, so a program that links the host layer
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
	// (host only, vfgs_hip_models_from_afgs1_mix: the bookkeeping turns them into the record's mix words at the programmed depth, and the
	// kernel writes those with the record; zero = a model without a mix)
	int32_t mix_carried;      // the model carries a mix
	uint32_t mix[2];          // Cb, Cr: model_mix_word with the offset as vfgs_hip_set_chroma_mix takes it (not yet << (depth - 8))
	uint8_t slut[3][256];     // scale bytes of Y, Cb, Cr
};
static_assert(sizeof(FwModelJob) % 16 == 0, "jobs of a table are read with aligned scalar and vector loads");

// one launch: jobs[0..n) of a device job table, n <= kFwModelChunk; depth8: one-pattern components take the packed 16-bit form
typedef hipError_t (*FwModelsLauncher)(const FwConstants* k, const FwModelJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream);
hipError_t launch_fw_models(const FwConstants* k, const FwModelJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream);

// vfgs_host.cpp: build jobs[0..n) (parameter-set side filled in, refusals of the parameter sets already made) into n live models at
// the programmed depth and format; out[0..n) are all set, or all NULL with an error code.  who: the entry's name for messages.
int build_models(const char* who, FwModelJob* jobs, unsigned n, vfgs_hip_model** out, void* stream, FwModelsLauncher launch);

// ---- models from FGC SEI messages (vfgs_hip_models_from_sei) ----

// LDS of fw_sei_build_kernel, one region that a model uses in one of two ways.
//   frequency filtered: the finished patterns ([8][64][64] luma, [8][32][32] raw chroma), then fw_ff_kernel's operands -- Bt, Dt (64 rows of
//                       68 bytes), X (64x64 int16), Dp (32x64 dwords) --, the Gaussian table, 40 stream words per plane type
//   auto-regressive   : eight luma and eight chroma arenas of fw_models_kernel's sizes (guard zones included), the Gaussian table, two streams
constexpr int kFwSeiLdsFf = 8 * 4096 + 8 * 1024 + 2 * 64 * 68 + 64 * 64 * 2 + 32 * 64 * 4 + 2048 + 2 * 40 * 4;     // 68416
constexpr int kFwSeiLdsAr = 8 * kFwArenaLuma + 8 * kFwArenaChroma + 2048 + 2 * kFwStreamWords * 4;                 // 80256
constexpr int kFwSeiLdsBytes = kFwSeiLdsFf > kFwSeiLdsAr ? kFwSeiLdsFf : kFwSeiLdsAr;
static_assert(kFwSeiLdsBytes == 80256, "tests/test_code_object_sei_model_build_cpu.py reads the group segment of the built kernel against this");

// What ONE model is made from.  The entry point fills the message side (pattern lists, taps or cut-offs, LUTs, uniform slots); the
// bookkeeping adds what depends on the programmed depth, format and range (record, form, stored shift, dst).
struct FwSeiJob {
	uint8_t* dst;             // device: this model's ModelRecord, the table image behind it (16-byte aligned)
	ModelRecord rec;          // the first 32 bytes at dst
	int32_t one_y, one_c;     // form of the image (image_layout)
	int32_t slot[3];          // Y, Cb, Cr: the slot the pattern LUT selects for every intensity, -1 if it depends on the intensity
	int32_t scale_shift;      // arrives as the argument of vfgs_set_scale_shift, leaves as what that setter stores (vfgs_hw.c:349)
	int32_t kind;             // 0: frequency filtered, 1: auto-regressive (any non-zero model_id)
	int32_t np_luma, np_chroma;     // patterns of the luma list, of the list Cb and Cr share (0..8)
	int32_t ar_scale;         // kind 1: right shift of the filter sum (log2_scale_factor, 1..15)
	int32_t reserved[4];
	int16_t pat[16][28];      // luma patterns 0..7, chroma patterns 8..15 -- kind 0: {fh, fv} (comp_model_value[1], [2]); kind 1: the 4x7 taps
	uint8_t slut[3][256];     // scale bytes of Y, Cb, Cr
	uint8_t plut[3][256];     // pattern LUTs (slot in bits 7:4, vfgs_hw.c:212)
};
static_assert(sizeof(FwSeiJob) % 16 == 0, "jobs of a table are read with aligned scalar and vector loads");

typedef hipError_t (*FwSeiLauncher)(const FwConstants* k, const FwSeiJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream);
hipError_t launch_fw_sei_build(const FwConstants* k, const FwSeiJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream);

// vfgs_host.cpp: as build_models, at the programmed depth, format AND legal range (an SEI message carries none)
int build_models_sei(const char* who, FwSeiJob* jobs, unsigned n, vfgs_hip_model** out, void* stream, FwSeiLauncher launch);

int set_error(int code, const char* msg);

}  // namespace vfgs
