/*
 * libvfgs_hip -- firmware layer on the GPU.
 *
 * Drop-in for the reference's firmware interface, /root/reference/src/vfgs_fw.h:49-92: the
 * two parameter structures (same members, same order, same C layout) and the two entry points
 *
 *     void vfgs_init_sei(fgs_sei* cfg);        vfgs_fw.h:91, vfgs_fw.c:517-644
 *     void vfgs_init_afgs1(fgs_afgs1* cfg);    vfgs_fw.h:92, vfgs_fw.c:663-708
 *
 * Like the reference's, they program the hardware layer (vfgs_hip.h) through its setters; the
 * difference is where the grain patterns are made.  The reference builds every pattern on the
 * CPU (64x64 / 32x32 integer inverse DCT of band-limited Gaussian noise, vfgs_fw.c:297-408, or
 * a causal auto-regressive filter over 82x73 / 44x38 samples, vfgs_fw.c:410-502) and copies it
 * into the hardware layer.  Here the host only derives the small tables (scale / pattern LUTs,
 * shifts, seed) and queues one kernel launch that generates all patterns of the configuration
 * directly in the device-resident pattern banks: no pattern byte crosses PCIe, and a
 * per-frame configuration switch (`-c <poc>:file`, vfgs_main.c:773-781) does not stall the
 * grain kernels that are still queued.
 *
 * A program that also links the reference's vfgs_fw.c keeps using that one (symbols of the
 * executable win); a program that links only vfgs_main.c + yuv.c gets these.
 *
 * Errors: none returned, as in the reference; violations that the reference asserts on
 * (vfgs_fw.c:459 unsupported coefficient count, :656 non-increasing scaling points) abort with
 * a message, HIP failures abort too.  vfgs_hip_last_error_string() has the text.
 */
#ifndef VFGS_HIP_FW_H_
#define VFGS_HIP_FW_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEI_MAX_MODEL_VALUES 6   /* vfgs_fw.h:49 */

/* FGC SEI message (H.274), vfgs_fw.h:51-60 */
typedef struct fgs_sei_s {
	uint8_t model_id;                               /* 0: frequency filtering, 1: auto-regressive */
	uint8_t log2_scale_factor;
	uint8_t comp_model_present_flag[3];
	uint16_t num_intensity_intervals[3];
	uint8_t num_model_values[3];
	uint8_t intensity_interval_lower_bound[3][256];
	uint8_t intensity_interval_upper_bound[3][256];
	int16_t comp_model_value[3][256][SEI_MAX_MODEL_VALUES];
} fgs_sei;

/* AOM film grain metadata (AFGS1), vfgs_fw.h:62-89 */
typedef struct fgs_afgs1_s {
	uint16_t grain_seed;
	uint8_t num_y_points;            /* 0..14 */
	uint8_t point_y_values[14];
	uint8_t point_y_scaling[14];
	uint8_t chroma_scaling_from_luma;
	uint8_t num_cb_points;           /* 0..10 */
	uint8_t point_cb_values[10];
	uint8_t point_cb_scaling[10];
	uint8_t num_cr_points;           /* 0..10 */
	uint8_t point_cr_values[10];
	uint8_t point_cr_scaling[10];
	uint8_t grain_scaling;           /* 8..11 */
	uint8_t ar_coeff_lag;            /* 0..3 */
	int16_t ar_coeffs_y[24];
	int16_t ar_coeffs_cb[25];
	int16_t ar_coeffs_cr[25];
	uint8_t ar_coeff_shift;          /* 6..9 */
	uint8_t grain_scale_shift;       /* 0..3 */
	uint8_t cb_mult;
	uint8_t cb_luma_mult;
	uint16_t cb_offset;
	uint8_t cr_mult;
	uint8_t cr_luma_mult;
	uint16_t cr_offset;
	uint8_t overlap_flag;
	uint8_t clip_to_restricted_range;
} fgs_afgs1;

/* ---- drop-in entry points (vfgs_fw.h:91-92) ------------------------------------------- */
void vfgs_init_sei(fgs_sei* cfg);
void vfgs_init_afgs1(fgs_afgs1* cfg);

/* ---- extensions ---------------------------------------------------------------------- */

/* AFGS1 says how strong the chroma grain is at a sample by a mix of the co-located luma and the chroma sample (cb_mult,
 * cb_luma_mult, cb_offset; the same for Cr; the luma alone with chroma_scaling_from_luma).  The reference reads the fields
 * and drops them (vfgs_fw.c:706), and so does vfgs_init_afgs1 by default.  With this switch on (process-wide; a process
 * that never calls it takes the environment variable VFGS_HIP_AFGS1_CHROMA_MIX=1 as `enable`, which is how the unchanged
 * reference CLI linked against this library gets it) vfgs_init_afgs1 additionally programs the hardware layer's mix
 * (vfgs_hip_set_chroma_mix, vfgs_hip.h) for Cb and Cr:
 *   chroma_scaling_from_luma ? (64, 0, 0) : (cb_luma_mult - 128, cb_mult - 128, cb_offset - 256).
 * With the switch off vfgs_init_afgs1 clears the mix; vfgs_init_sei always clears it. */
void vfgs_hip_afgs1_chroma_mix(int enable);

/* The value vfgs_init_afgs1 passes to vfgs_set_seed for this picture: grain_seed | grain_seed << 16 (vfgs_fw.c:672).  A caller that
 * collects consecutive pictures sharing one model programs the model once and hands their seeds to
 * vfgs_hip_add_grain_frame_list_seeded_dev (vfgs_hip.h) -- this is the seed of each.  Host only, no GPU needed. */
unsigned int vfgs_hip_afgs1_seed(const fgs_afgs1* cfg);

/* MODELS STRAIGHT FROM PARAMETER SETS, a batch per launch.  A player that receives an AFGS1 parameter set with every picture gets its
 * models (vfgs_hip.h "models as objects") without programming anything: at the programmed depth and chroma format (vfgs_set_depth,
 * vfgs_set_chroma_subsampling) out[i] is a live model that no call taking models -- the two list calls with a model per picture,
 * vfgs_hip_model_info, vfgs_hip_model_release -- can tell apart from the result of
 *     vfgs_hip_afgs1_chroma_mix(0); vfgs_init_afgs1(&cfgs[i]); vfgs_hip_model_capture(&out[i], stream);
 * including the form of its image (at 8 bit a component whose scaling function does not fit the packed 16-bit form falls back to the
 * general form; the slots no LUT selects are zero there) and the reference firmware's quirks as vfgs_init_afgs1 restates them.
 * The PROGRAMMED STATE IS UNTOUCHED: host mirror, device pattern banks, pending pattern requests, table images, depth and format, the four
 * seed registers, the chroma mix and its switch are what they were.  The picture's seed stays the caller's business --
 * vfgs_hip_afgs1_seed(&cfgs[i]) goes into the list call's `seeds` -- and cb_mult and the other mix fields are ignored by THIS call: its
 * models carry no mix, as with vfgs_hip_model_capture.  vfgs_hip_models_from_afgs1_mix below attaches them.
 * One kernel serves up to 32 models (one workgroup each: the luma and the Cb recursion side by side, then the whole record + image
 * written from LDS), so a call queues ONE copy (the job table) and ONE launch per 32 models; the models of such a chunk share one device
 * allocation that returns to a small pool with the last release: no allocation and no free in the steady state of build / grain / release
 * (vfgs_hip_get_model_build_stats, vfgs_hip.h).  Asynchronous on `stream`; a first use on another stream waits by event; inside an
 * overlap region pass the region's stream.
 * REFUSALS replace vfgs_init_afgs1's aborts.  A refused call builds nothing, sets out[0..n) to NULL, queues nothing and changes no
 * statistic; the message names the index and the cause:
 *   41  out == NULL, or cfgs == NULL (n > 0)
 *   42  ar_coeff_lag outside 1..3; num_y_points > 14, num_cb_points / num_cr_points > 10; scaling points not strictly increasing in a
 *       function that is used (Cb's and Cr's are not with chroma_scaling_from_luma); ar_coeff_shift outside 1..15; grain_scale_shift > 6
 *    9  the scale shift that vfgs_set_scale_shift(grain_scaling - 6) would store is out of range at the programmed depth (vfgs_hw.c:170),
 *       exactly as vfgs_hip_model_capture refuses it: grain_scaling outside 8..13
 * n == 0 is no call at all and returns 0. */
struct vfgs_hip_model;
int vfgs_hip_models_from_afgs1(const fgs_afgs1* cfgs, unsigned n, struct vfgs_hip_model** out, void* stream);

/* ... WITH THE CHROMA MIX OF EACH PARAMETER SET.  vfgs_hip_models_from_afgs1 in every respect -- refusals 41 / 42 / 9, one copy and one
 * launch per 32 models, the slab pool and its counters, the programmed state untouched, the mix and its switch included -- and in addition
 * out[i] CARRIES the mix vfgs_init_afgs1 programs with the switch of vfgs_hip_afgs1_chroma_mix on, whatever the switch says:
 *   chroma_scaling_from_luma ? (64, 0, 0) : (cb_luma_mult - 128, cb_mult - 128, cb_offset - 256), and the same for Cr,
 * both components active (vfgs_hip_set_chroma_mix's rule: a component that was set is).  out[i] is what
 *     vfgs_hip_afgs1_chroma_mix(1); vfgs_init_afgs1(&cfgs[i]); vfgs_hip_model_capture_mix(&out[i], stream);
 * gives (vfgs_hip.h), record and image byte for byte; vfgs_hip_model_chroma_mix reads the mix back, and the two list calls with a model per
 * picture honour it frame by frame, 32 pictures per launch (grain_mix_kernel / grain_sp_mix_kernel).  The kernel that builds the models
 * writes the mix with the record: no second kernel, no further copy.
 * FURTHER REFUSALS, the message naming the index:
 *   42  a mix field vfgs_hip_set_chroma_mix would refuse (37 there): cb_offset / cr_offset above 511
 *   38  what the processing calls refuse under a mix: the programmed depth is 12; or, at 8 bit, a scaling function that does not fit the
 *       packed 16-bit form, so that the image would fall back to the general form (the models of the mix are all-one-pattern) */
int vfgs_hip_models_from_afgs1_mix(const fgs_afgs1* cfgs, unsigned n, struct vfgs_hip_model** out, void* stream);

/* ... AND FROM FGC SEI MESSAGES.  A VVC / HEVC player that receives an FGC SEI with a picture (the reference CLI's `-c <poc>:<file>`) gets its
 * models the same way.  The call works at the programmed depth, chroma format AND legal range (vfgs_set_depth, vfgs_set_chroma_subsampling,
 * vfgs_set_legal_range: fgs_sei carries no range and vfgs_init_sei sets none); out[i] is a live model that no call taking models -- the two
 * list calls with a model per picture, vfgs_hip_model_info, vfgs_hip_model_image, vfgs_hip_model_release -- can tell apart from the result of
 *     vfgs_hip_reset_state(); vfgs_set_depth; vfgs_set_chroma_subsampling; vfgs_set_legal_range;
 *     vfgs_init_sei(&cfgs[i]); vfgs_hip_model_capture(&out[i], stream);
 * "From a reset state" makes this exact for every byte in every form: a general-form image holds the generated slots 0..np-1 of each list
 * and zeros elsewhere.  The form follows the derived tables as capture's does: luma is one-pattern iff its pattern LUT selects one slot for
 * all 256 intensities and (8 bit) its scale LUT fits the packed 16-bit form; chroma iff Cb's LUT and Cr's LUT are each uniform -- possibly
 * on different slots -- and both scale LUTs fit; a uniform slot the list does not hold (an absent component, the unused entry the
 * reference's pattern search can match) is the zero pattern.  The reference firmware's quirks are those vfgs_init_sei restates.
 * The PROGRAMMED STATE IS UNTOUCHED: host mirror, device pattern banks, pending pattern requests, table images, depth, format and range, the
 * four seed registers, the chroma mix and its switch are what they were.  A model from an SEI carries no mix (an SEI has none;
 * vfgs_hip_models_from_afgs1_mix and vfgs_hip_model_capture_mix make models that do); an SEI carries no seed: the seed stays the caller's
 * (`seeds` of the list call, or the running sequence).
 * One kernel serves up to 32 models (one workgroup each: every pattern of the message -- up to 8 luma and 8 chroma -- made in LDS, then the
 * whole record + image written from there), so a call queues ONE copy (the job table) and ONE launch per 32 models; the models of a chunk
 * share one device allocation from the pool of vfgs_hip_models_from_afgs1, and vfgs_hip_get_model_build_stats counts both calls in the same
 * counters: no allocation and no free in the steady state of build / grain / release.  Asynchronous on `stream`; a first use on another
 * stream waits by event; inside an overlap region pass the region's stream.
 * REFUSALS replace vfgs_init_sei's aborts and out-of-bounds reads.  A refused call builds nothing, sets out[0..n) to NULL, queues nothing and
 * changes no statistic; the message names the index and the cause (all messages are examined for 42 first, then for 9):
 *   41  out == NULL, or cfgs == NULL (n > 0)
 *   42  num_intensity_intervals[c] > 256 for a component whose comp_model_present_flag[c] is set (the arrays hold 256);
 *       model_id != 0 with log2_scale_factor outside 1..15 (the pattern job is refused there and vfgs_init_sei aborts)
 *    9  the scale shift that vfgs_set_scale_shift(log2_scale_factor - (model_id ? 1 : 0)) would store is out of range at the programmed
 *       depth (vfgs_hw.c:170), exactly as vfgs_hip_model_capture refuses it: the argument outside 2..7
 * Everything else is accepted and behaves as vfgs_init_sei does: any non-zero model_id is the auto-regressive model, cut-offs of any int16
 * value clamp as the pattern generator clamps them, more than 8 distinct parameter sets, unsorted or overlapping intervals, gaps and absent
 * components (luma included) give what the reference firmware gives.  n == 0 is no call at all and returns 0. */
int vfgs_hip_models_from_sei(const fgs_sei* cfgs, unsigned n, struct vfgs_hip_model** out, void* stream);

/* One grain pattern to be generated on the device into pattern slot `index`. */
typedef struct vfgs_hip_pattern_job {
	int32_t kind;       /* 0: frequency filtered (vfgs_fw.c:362-408), 1: auto-regressive (vfgs_fw.c:410-502) */
	int32_t chroma;     /* 0: 64x64 luma pattern, noise seed Seed_LUT[0]; 1: 32x32 chroma pattern */
	int32_t index;      /* pattern slot 0..7, as vfgs_set_luma_pattern / vfgs_set_chroma_pattern */
	int32_t seed_index; /* which entry of the seed table, 0..255, starts the noise generator (vfgs_fw.c:369,392,620,...) */
	int32_t fh, fv;     /* kind 0: horizontal / vertical cut-off, comp_model_value[1], [2] (2..14) */
	int32_t scale;      /* kind 1: right shift of the filter sum (log2_scale_factor or ar_coeff_shift), 1..15 */
	int32_t shift;      /* kind 1: right shift of the Gaussian sample, 1..7 */
	int16_t coef[28];   /* kind 1: the 4x7 causal filter taps exactly as vfgs_fw.c:412,424-462 lays them out */
} vfgs_hip_pattern_job;

/* Queue the generation of `n` (<= 16) patterns.  Asynchronous; ordered before every later
 * vfgs_add_grain_* / vfgs_hip_add_grain_* call.  Luma jobs come first: a chroma job on a
 * non-4:2:0 layout inherits the tail of the last luma pattern of the same call, as the
 * reference's shared 64x64 scratch buffer does (vfgs_fw.c:519,603-623 with vfgs_hw.c:320-325).
 * Returns 0 or an error code. */
int vfgs_hip_generate_patterns(const vfgs_hip_pattern_job* jobs, int n);

/* Read back pattern slot `index` of bank `chroma` (0 luma, 1 chroma) as the hardware layer
 * holds it ([64][64], vfgs_hw.c:49).  Synchronises; for tests and debugging. */
int vfgs_hip_get_pattern(int chroma, int index, signed char out[64 * 64]);

/* ---- configuration files ----------------------------------------
 * What the reference CLI does between `-c <file>` and vfgs_init_* (vfgs_main.c:126-195 value
 * readers, :208-232 chroma adjustment, :234-303 checks, :309-434 AFGS1 "grain table" syntax,
 * :436-559 cfg and SEI-dump syntaxes, :561-593 gain), as library calls, so that a host without
 * the reference's vfgs_main.c can go from a configuration file to a programmed device.  Host
 * only; no GPU needed until vfgs_hip_cfg_program().
 *
 * The state is the pair of parameter sets the CLI keeps (vfgs_main.c:69-124).  Reading a file
 * updates it IN PLACE -- fields a file does not mention keep their previous values, exactly as
 * in the CLI, where every file is read on top of the defaults / the previous configuration.
 * AFGS1 is active when afgs1.num_y_points != 0 (vfgs_main.c:297-303). */
typedef struct vfgs_hip_cfg {
	fgs_sei sei;
	fgs_afgs1 afgs1;
} vfgs_hip_cfg;

/* the CLI's built-in SEI (vfgs_main.c:69-120), AFGS1 off */
void vfgs_hip_cfg_defaults(vfgs_hip_cfg* cfg);
/* read one file (any of the three syntaxes); 0, or 1 with the reference's message in vfgs_hip_last_error_string() */
int vfgs_hip_cfg_read(vfgs_hip_cfg* cfg, const char* filename);
/* the CLI's acceptance checks for picture format 420 / 422 / 444 and bit depth 8 / 10; 0 or 1 + message */
int vfgs_hip_cfg_check(const vfgs_hip_cfg* cfg, int format, int depth);
/* SEI frequency cut-offs and scale of the chroma components for subsampled formats (vfgs_main.c:208-232) */
void vfgs_hip_cfg_adjust_chroma(vfgs_hip_cfg* cfg, int format);
/* global strength in percent (vfgs_main.c:561-593); 100 = unchanged */
void vfgs_hip_cfg_apply_gain(vfgs_hip_cfg* cfg, unsigned gain);
/* vfgs_init_afgs1(&cfg->afgs1) or vfgs_init_sei(&cfg->sei), whichever is active (vfgs_main.c:757-760) */
void vfgs_hip_cfg_program(vfgs_hip_cfg* cfg);

#ifdef __cplusplus
}
#endif

#endif /* VFGS_HIP_FW_H_ */
