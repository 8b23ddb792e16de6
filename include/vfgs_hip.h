/*
 * libvfgs_hip -- MI355X (gfx950) film grain synthesis hardware layer.
 *
 * C ABI.  Two groups of entry points:
 *
 * (1) DROP-IN: the ten functions of the reference hardware-layer interface,
 *     /root/reference/src/vfgs_hw.h:51-62, with identical names, argument
 *     meaning and (absence of) error reporting, so that the reference's
 *     vfgs_fw.c (callers: vfgs_fw.c:585,594,637,638,643,672-704) and
 *     vfgs_main.c (callers: vfgs_main.c:674,750,751,760) link against this
 *     library unchanged.  The reference header spells its types with macros
 *     (`int8`, `uint8`, `uint32`, vfgs_hw.h:40-47); the plain C types below
 *     are the same types.  State is a process-global singleton exactly like
 *     the reference's file-scope statics (vfgs_hw.c:49-68); all pointer
 *     arguments are borrowed for the duration of the call only.
 *
 * (2) EXTENSIONS (vfgs_add_grain_stripe, vfgs_hip_*): the throughput path.
 *     The reference has no stripe/frame entry; these are defined here with
 *     the contract "same samples and same seed registers afterwards as
 *     calling vfgs_add_grain_line for every line of the stripe, in order".
 *
 * There is no CPU fallback: every processing call runs HIP kernels and fails
 * loudly (message on stderr + abort for the void drop-in calls, nonzero return
 * for the vfgs_hip_* calls) when no gfx950 device/runtime is usable.
 */
#ifndef VFGS_HIP_H
#define VFGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFGS_HIP_MAX_PATTERNS 8   /* vfgs_hw.h:49 */

/* ---- (1) drop-in hardware-layer interface -------------------------------- */

/* vfgs_hw.h:51 / vfgs_hw.c:314-318 -- P: 64x64 int8, row-major. index 0..7. */
void vfgs_set_luma_pattern(int index, signed char* P);
/* vfgs_hw.h:52 / vfgs_hw.c:320-325 -- copies 64/csuby rows of 64/csubx bytes, source
 * pitch 64/csuby (sic): depends on the subsampling set EARLIER. index 0..7. */
void vfgs_set_chroma_pattern(int index, signed char* P);
/* vfgs_hw.h:53 / vfgs_hw.c:327-331 -- 256 scale factors for component c (0=Y,1=Cb,2=Cr). */
void vfgs_set_scale_lut(int c, unsigned char lut[]);
/* vfgs_hw.h:54 / vfgs_hw.c:333-337 -- 256 pattern selectors; slot = lut[i] >> 4 (must be <= 8). */
void vfgs_set_pattern_lut(int c, unsigned char lut[]);
/* vfgs_hw.h:56 / vfgs_hw.c:339-344 -- loads seed<<1 into all four LFSR registers. */
void vfgs_set_seed(unsigned int seed);
/* vfgs_hw.h:57 / vfgs_hw.c:346-350 -- shift in 2..7. */
void vfgs_set_scale_shift(int shift);
/* vfgs_hw.h:58 / vfgs_hw.c:352-362 -- 8, 10 or 12 (vfgs_hip_supports_depth).  The reference stops at 10 (vfgs_hw.c:354); depth 12 is its
 * formulas with bs = depth - 8 = 4, quirks included: samples are uint16, intensity = (I >> 4) & 0xff (a container value above 4095
 * wraps), clip limits I_min << 4 and I_max << 4 (full range: 4080, not 4095), scale_shift as stored = shift + 2; the seed registers
 * and the LFSR stream do not depend on the depth. */
void vfgs_set_depth(int depth);
/* vfgs_hw.h:59 / vfgs_hw.c:364-380 */
void vfgs_set_legal_range(int legal);
/* vfgs_hw.h:60 / vfgs_hw.c:382-388 -- each 1 or 2. */
void vfgs_set_chroma_subsampling(int subx, int suby);
/* vfgs_hw.h:62 / vfgs_hw.c:288-312 -- Y/U/V: HOST pointers to the start of line y in each
 * plane (U,V: chroma row y/csuby).  In place; complete when the call returns. */
void vfgs_add_grain_line(void* Y, void* U, void* V, int y, int width);

/* ---- (2) extensions ------------------------------------------------------- */

/* vfgs_add_grain_line and lines the caller has not handed over yet.  One drop-in call is one line in host memory and
 * must be complete on return (~90 us: copy in, launch, copy out).  The library therefore works ahead: on a miss it
 * starts computing the lines FOLLOWING the requested one as well -- the rest of the frame, in stripes of about 2 MB whose
 * upload, kernel and download are pipelined on three streams while the caller walks through the stripes already back --
 * keeps those results, and serves the next calls from them when they are exactly the predicted lines with unchanged
 * input bytes.  Lines not yet handed over are only
 * ever READ, and only inside rows the caller has proven to own: either this same buffer (same line-0 pointers and
 * width) has been walked top to bottom once before, or the caller has said so with vfgs_hip_declare_frame().  A first
 * frame, or a frame in a buffer the previous walk did not go through, is computed line by line.
 * vfgs_hip_line_lookahead(0) switches the behaviour off (so does the environment variable VFGS_HIP_LINE_LOOKAHEAD=0);
 * vfgs_hip_declare_frame(Y, U, V, width, height, stride, cstride) (host pointers to line 0, strides in samples)
 * promises that the three planes hold `height` lines at those pitches, which enables working ahead from the first
 * line of the first frame on; it stays valid for walks that start at these pointers; all-NULL revokes it.
 * For a binary that cannot be rebuilt, the environment variable VFGS_HIP_FRAME_HEIGHT=<lines> makes the same promise for
 * every walk that starts at line 0 (planes of at least that many lines at the pitches the first lines show): the first
 * frame then costs three line round trips instead of one per line (4320p: 0.36 s -> 12 ms inside the library; a short run of
 * the unchanged CLI, promised and plain runs interleaved on one box: never slower, 0.1 s faster at 4320p x 3 frames --
 * profiles/r06_cli_short_runs.log; round 5's "slower with the promise" was the order of its runs). */
void vfgs_hip_line_lookahead(int enable);
int vfgs_hip_declare_frame(const void* Y, const void* U, const void* V, unsigned width, unsigned height,
                           unsigned stride, unsigned cstride);

/* Host-memory stripe: lines y .. y+height-1, strides in samples.  Equivalent to `height`
 * consecutive vfgs_add_grain_line calls (one H2D + kernel + D2H instead of `height`). */
void vfgs_add_grain_stripe(void* Y, void* U, void* V, unsigned y, unsigned width,
                           unsigned height, unsigned stride, unsigned cstride);

/* Select the HIP device (default: the current device at first use) and create the
 * device-side state.  Returns 0 on success. */
int vfgs_hip_init(int device);
void vfgs_hip_shutdown(void);

/* Back to the reference's power-on state (vfgs_hw.c:49-63): zero banks and LUTs, seeds
 * 0xdeadbeef, 8-bit, 4:2:0, full range.  The reference has no such call because its state
 * only ever lives for one process; a long-lived library needs one. */
void vfgs_hip_reset_state(void);

/* Luma / chroma mix of the chroma look-up index (AFGS1: cb_mult, cb_luma_mult, cb_offset; off at power-on and after
 * vfgs_hip_reset_state, and then every result is the reference's).  For component c (1 = Cb, 2 = Cr) with a mix, the
 * index of BOTH look-ups (pattern LUT, scale LUT) of the chroma sample C at column cx of row cy is not C >> (depth - 8)
 * (vfgs_hw.c:211) but m >> (depth - 8), where, with L the luma plane and C the chroma plane as they are BEFORE the call
 * adds any grain, W the luma width of the call, 32-bit arithmetic and arithmetic shifts:
 *   avgL = csubx == 2 ? (L[cy * csuby][2 cx] + L[cy * csuby][min(2 cx + 1, W - 1)] + 1) >> 1 : L[cy * csuby][cx]
 *   m    = clip(((avgL * luma_mult + C * chroma_mult) >> 6) + offset * (1 << (depth - 8)), 0, (1 << depth) - 1)
 * luma_mult, chroma_mult: units of 1/64, -128..127; offset: 8-bit code values, -256..255.  (0, 64, 0) is neutral.
 * Nothing else changes: the grain added to luma, the seed registers, clipping.  Every processing entry point of this
 * header honours an active mix, in place (the chroma planes are then computed in a launch of their own in front of luma's)
 * and out of place, with four exceptions that REFUSE with error 38 and change nothing: a programmed model that needs a
 * general-form pattern bank (a pattern LUT that selects more than one pattern; a one-pattern model wider than 8192 samples
 * at 4:2:2 or 4:4:0) -- the kernels of the mix exist for the one-pattern banks of the AFGS1 models --, depth 12 -- they
 * exist at 8 and 10 bit; every processing call refuses while both hold --, and
 * vfgs_add_grain_stripe / vfgs_hip_add_grain_frames_host while several devices are set (vfgs_hip_init_devices).  While a
 * mix is active vfgs_add_grain_line computes line by line (no look-ahead).
 * set: 0, or error 37 (component or range) with nothing changed.  get: out[4] = { luma_mult, chroma_mult, offset, active }. */
int vfgs_hip_set_chroma_mix(int c, int luma_mult, int chroma_mult, int offset);
void vfgs_hip_clear_chroma_mix(void);
int vfgs_hip_get_chroma_mix(int c, int out[4]);

/* Device-resident stripe / frame: dY/dU/dV are DEVICE pointers to the first line of the
 * stripe (dU/dV: chroma row y/csuby); 16-byte aligned, pitch*bytes_per_sample % 16 == 0,
 * stride >= 16*ceil(width/16) (the reference writes whole 16-sample blocks, SURVEY 8a
 * quirk 7).  Bytes outside the whole blocks of a row and rows outside the addressed lines -- above a stripe or
 * part, behind its last line, behind chroma row ceil(height / csuby) - 1 -- are never written or relied upon, in
 * place or out of place, in this and in every planar call below; the smallest pitch is the whole blocks of the row
 * in bytes, rounded up to a multiple of 16 (8-bit 4:2:0 of 21 blocks: luma 336, chroma 168 -> 176), and planes may
 * lie back to back in one allocation.  Asynchronous on `stream` (a hipStream_t, may be NULL).  Returns 0 on success. */
int vfgs_hip_add_grain_stripe_dev(void* dY, void* dU, void* dV, unsigned y, unsigned width,
                                  unsigned height, unsigned stride, unsigned cstride, void* stream);
int vfgs_hip_add_grain_frame_dev(void* dY, void* dU, void* dV, unsigned width, unsigned height,
                                 unsigned stride, unsigned cstride, void* stream);

/* Multi-GPU stripe split (no collective): process only lines [part_y, part_y+part_height)
 * of a frame of `frame_height` lines -- pointers address line part_y -- but advance the
 * seed registers as if the whole frame had been processed, so that every rank stays in
 * lock step.  part_y must be a multiple of 16. */
int vfgs_hip_add_grain_frame_part_dev(void* dY, void* dU, void* dV, unsigned width,
                                      unsigned frame_height, unsigned part_y, unsigned part_height,
                                      unsigned stride, unsigned cstride, void* stream);

/* Batch: `nframes` equally shaped device-resident frames in ONE launch, processed as
 * consecutive frames (frame f+1 continues frame f's seed state).  Plane pointers of frame
 * f are dY + f*y_frame_pitch_bytes etc. */
int vfgs_hip_add_grain_frames_dev(void* dY, void* dU, void* dV, unsigned width, unsigned height,
                                  unsigned stride, unsigned cstride, unsigned nframes,
                                  uint64_t y_frame_pitch_bytes, uint64_t c_frame_pitch_bytes,
                                  void* stream);

/* Batch + stripe split combined: lines [part_y, part_y+part_height) of each of `nframes`
 * consecutive frames in ONE launch (what one rank of an N-GPU stripe split runs per step);
 * pointers address line part_y of frame 0; seeds advance as for whole frames. */
int vfgs_hip_add_grain_frames_part_dev(void* dY, void* dU, void* dV, unsigned width,
                                       unsigned frame_height, unsigned part_y, unsigned part_height,
                                       unsigned stride, unsigned cstride, unsigned nframes,
                                       uint64_t y_frame_pitch_bytes, uint64_t c_frame_pitch_bytes,
                                       void* stream);

/* Out-of-place form of the call above: reads sY/sU/sV, writes dY/dU/dV (same geometry and
 * pitches; src == dst is allowed and is what the in-place entry points pass).  This is how a
 * decoder uses film grain -- the clean picture stays a reference frame, the grained copy goes
 * to the display queue.  Same kernels, same speed within 2-3 % (profiles/r04_config_matrix*.jsonl:
 * 4320p 0.733 out of place / 0.716 in place of the 8 TB/s peak; as PURE streams the order is the
 * other way round on MI355X -- in-place nontemporal 6.6 TB/s, src->dst copy 5.0-5.3 TB/s,
 * BENCH_r03 / bench.py copy_ceilings_gbs). */
int vfgs_hip_add_grain_copy_dev(const void* sY, const void* sU, const void* sV, void* dY, void* dU, void* dV,
                                unsigned width, unsigned frame_height, unsigned part_y, unsigned part_height,
                                unsigned stride, unsigned cstride, unsigned nframes,
                                uint64_t y_frame_pitch_bytes, uint64_t c_frame_pitch_bytes, void* stream);

/* The same with the output narrowed to 8 bit in the store: dst sample = (uint8)((v + 2) >> 2),
 * i.e. the reference CLI's `--outdepth 8` step yuv_to_8bit (yuv.c:216-258, called at
 * vfgs_main.c:787-788) fused into the kernel; at depth 12 (uint8)((v + 8) >> 4), the same rounding (the full-range
 * maximum 4080 gives 255).  Needs vfgs_set_depth(10) or (12); error 16 at depth 8.  Source planes hold
 * uint16 samples (strides in samples), destination planes uint8 samples with their own strides
 * and frame pitches (multiples of 16).  Halves the write traffic of the path. */
int vfgs_hip_add_grain_copy8_dev(const void* sY, const void* sU, const void* sV, void* dY, void* dU, void* dV,
                                 unsigned width, unsigned frame_height, unsigned part_y, unsigned part_height,
                                 unsigned stride, unsigned cstride, unsigned dst_stride, unsigned dst_cstride,
                                 unsigned nframes, uint64_t y_frame_pitch_bytes, uint64_t c_frame_pitch_bytes,
                                 uint64_t dst_y_frame_pitch_bytes, uint64_t dst_c_frame_pitch_bytes, void* stream);

/* Batch of frames that are NOT equally spaced in memory (a decoder's pool of separately allocated frames; the reference's own
 * loop hands over one frame per call, vfgs_main.c:771-790): `nframes` equally shaped device-resident frames, frame f's planes at
 * frames[f].Y / .U / .V (device pointers to line 0, 16-byte aligned), processed as consecutive frames in ONE launch per 32
 * frames -- results and seed registers are those of `nframes` vfgs_hip_add_grain_frame_dev calls in list order.  The list itself
 * is host memory, read during the call only (the pointers travel in the kernel arguments: nothing to keep alive, no copy queued
 * in front of the launch).  A single frame per launch runs at 0.23 (1080p) / 0.49 (2160p) / 0.61 (4320p) of the HBM peak, the
 * same frames handed over 32 / 16 / 8 at a time at 0.70 / 0.76 / 0.72 (a launch costs 5 us of fill and drain).  All frames of
 * a call are in flight together, so the call refuses (error 18, nothing changed) destination planes that share bytes -- the
 * same plane listed twice, or two whose rows overlap -- and, in the _copy forms, a source plane that shares bytes with the
 * destination of ANOTHER frame (consecutive calls would read it grained or not, deterministically; one launch would not).
 * _copy: out of place, src[f] -> dst[f], same geometry (a plane of src[f] may BE the plane of dst[f]: in place);
 * _copy8: 10- or 12-bit source, 8-bit destination as vfgs_hip_add_grain_copy8_dev.  A refused call changes nothing. */
typedef struct vfgs_hip_frame_ptrs { void* Y; void* U; void* V; } vfgs_hip_frame_ptrs;
int vfgs_hip_add_grain_frame_list_dev(const vfgs_hip_frame_ptrs* frames, unsigned nframes, unsigned width, unsigned height,
                                      unsigned stride, unsigned cstride, void* stream);
/* ... lines [part_y, part_y + part_height) of every listed frame only (what one rank of a stripe split runs on its stripes of a
 * pool of frames): frames[f].Y / .U / .V address line part_y (chroma row part_y / csuby) of frame f, part_y a multiple of 16;
 * the seed registers advance as for whole frames of `frame_height` lines (vfgs_hip_add_grain_frames_part_dev). */
int vfgs_hip_add_grain_frame_list_part_dev(const vfgs_hip_frame_ptrs* frames, unsigned nframes, unsigned width,
                                           unsigned frame_height, unsigned part_y, unsigned part_height,
                                           unsigned stride, unsigned cstride, void* stream);
int vfgs_hip_add_grain_frame_list_copy_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_frame_ptrs* dst, unsigned nframes,
                                           unsigned width, unsigned height, unsigned stride, unsigned cstride, void* stream);
int vfgs_hip_add_grain_frame_list_copy8_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_frame_ptrs* dst, unsigned nframes,
                                            unsigned width, unsigned height, unsigned stride, unsigned cstride,
                                            unsigned dst_stride, unsigned dst_cstride, void* stream);

/* The list calls with A SEED PER PICTURE.  The calls above treat their frames as one seed sequence (frame f + 1 continues frame f's
 * registers); AFGS1 carries a grain_seed per picture (vfgs_init_afgs1 calls vfgs_set_seed for each, vfgs_fw.c:672; vfgs_hip_afgs1_seed
 * in vfgs_hip_fw.h), and a player that reseeds an SEI model per picture is in the same position.  seeds: host memory, `nframes` values,
 * read during the call only, each exactly what the caller would pass to vfgs_set_seed.  Samples and seed registers afterwards are those of
 *     for f in list order: vfgs_set_seed(seeds[f]); vfgs_hip_add_grain_frame_dev(frame f)
 * (_part: vfgs_hip_add_grain_frame_part_dev in that loop; _copy / _copy8: their single-frame forms) in ONE launch per 32 frames.  After
 * the call the library is where vfgs_set_seed(seeds[nframes - 1]) and one whole frame leave it: a later call without seeds continues
 * that picture's stream, as the reference would.  If a later launch of a list of more than 32 frames fails with a HIP error, the
 * registers are those behind the last launch that was queued.
 * Everything the list calls above refuse is refused here, with the same codes, before anything changes -- in particular a refused call
 * does NOT reseed -- plus seeds == NULL with nframes > 0 (error 39).  An empty list is no call at all.  An active chroma mix is
 * honoured; inside an overlap region the calls alternate over the two internal streams like every other device-pointer call.
 * Cost: the library builds one short run of the LFSR stream per frame on the host (vfgs_hip_seed_segments below; about a microsecond per
 * 1080p frame) and uploads them in the caller's stream in front of the launch -- 34 KB for 1080p x 32, 130 KB for 4320p x 8.  That copy
 * in front of the kernel costs 11 .. 20 us per launch: 1080p x 32 / 2160p x 16 / 4320p x 8 run at 2.72 / 9.30 / 36.1 us per frame against
 * 2.37 / 8.06 / 33.7 without seeds and 19.3 / 22.6 / 62.5 with vfgs_set_seed + one frame per launch (profiles/per_picture_seeds.json). */
int vfgs_hip_add_grain_frame_list_seeded_dev(const vfgs_hip_frame_ptrs* frames, const uint32_t* seeds, unsigned nframes, unsigned width,
                                             unsigned height, unsigned stride, unsigned cstride, void* stream);
int vfgs_hip_add_grain_frame_list_seeded_part_dev(const vfgs_hip_frame_ptrs* frames, const uint32_t* seeds, unsigned nframes,
                                                  unsigned width, unsigned frame_height, unsigned part_y, unsigned part_height,
                                                  unsigned stride, unsigned cstride, void* stream);
int vfgs_hip_add_grain_frame_list_seeded_copy_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_frame_ptrs* dst, const uint32_t* seeds,
                                                  unsigned nframes, unsigned width, unsigned height, unsigned stride, unsigned cstride,
                                                  void* stream);
int vfgs_hip_add_grain_frame_list_seeded_copy8_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_frame_ptrs* dst, const uint32_t* seeds,
                                                   unsigned nframes, unsigned width, unsigned height, unsigned stride, unsigned cstride,
                                                   unsigned dst_stride, unsigned dst_cstride, void* stream);

/* SEMI-PLANAR frames: what a hardware decoder hands out.  A frame is a luma plane plus ONE plane of interleaved Cb/Cr pairs -- NV12 /
 * NV16 at 8 bit, P010 / P210 / P012 at 10 and 12 bit, where the samples sit in the HIGH bits of their 16-bit containers.  One call for
 * in place and out of place, one seed sequence and a seed per picture:
 *   Y            a luma plane exactly as in the lists above;
 *   UV           ceil(height / csuby) rows of Cb0 Cr0 Cb1 Cr1 ... in the depth's container (uint8 at depth 8, uint16 at 10 and 12);
 *   stride, uv_stride   containers of a Y row / a UV row, each >= 16 * ceil(width / 16): a UV row of whole blocks is as many containers
 *                as the luma row (whole 16-sample blocks are written, as everywhere); pointers 16-byte aligned, pitches in bytes
 *                multiples of 16;
 *   sample_shift 0 (low-aligned samples), or 16 - depth: P010 6, P012 4;
 *   seeds        NULL: one seed sequence, frame f + 1 continues frame f's registers; else `nframes` values as in the seeded lists above;
 *   src == dst (the same list, or dst[f]'s plane == src[f]'s plane) is in place.
 * The chroma format is the programmed one and must have csubx == 2: 4:2:0 gives NV12 / P010 / P012, 4:2:2 gives NV16 / P210.
 * With D(p) the planar, low-aligned picture of a semi-planar picture p (U = the even containers of UV, V = the odd ones, every container
 * >> sample_shift) the samples written are those of vfgs_hip_add_grain_frame_list[_seeded]_copy_dev on D(src[f]), interleaved again, every
 * written container << sample_shift (its low sample_shift bits zero); the four seed registers afterwards are that call's.  The low bits
 * of a SOURCE container are ignored; with sample_shift == 0 a container above the depth's range wraps exactly as in the planar calls
 * (vfgs_set_depth).  Bytes outside the whole blocks of a row and rows outside the picture are never written, in place or out of place.
 * One launch per 32 frames (vfgs_hip_last_launch_info().kernel: grain_sp_kernel<depth,csuby,oney,onec>); inside an overlap region the
 * call alternates over the two internal streams like every other device-pointer call.
 * An active chroma mix (vfgs_hip_set_chroma_mix, or the firmware's AFGS1 programming of it) is HONOURED: the samples written and the seed
 * registers are those of the planar copy list on D(src[f]) with the same mix active -- the luma that enters the mix is the source's,
 * >> sample_shift like every source container, the last luma sample of a row pairs with itself -- for one-pattern models at depth 8 and
 * 10 (kernel: grain_sp_mix_kernel<depth,csuby>; one read of the luma over a UV row serves Cb and Cr, a mix on one component only
 * included).  Chroma reads the luma of BEFORE the call: where any destination luma plane of a launch shares bytes with any source luma
 * plane of it (in place; also a destination Y that is the source Y with the UV plane elsewhere) the 32 frames are TWO launches on the
 * stream, the UV rows first, then luma -- `launches` counts both; fully out of place they are one.
 * Refused before anything changes (a refused call does not reseed): everything the list calls above refuse, with the same codes -- a null
 * list or plane 18, a misaligned pointer 7, bad geometry, destination planes that share bytes 18 (a UV plane that overlaps another
 * frame's Y included), a source plane that shares bytes with another frame's destination 18 -- and, error 40 with a message that names
 * the cause: csubx != 2; sample_shift not in {0, 16 - depth}, or non-zero at depth 8; width > 8192 (rows walked in parts); an active
 * chroma mix ("chroma mix" in the message) with a programmed model that needs a general-form pattern bank, or at depth 12 -- the two
 * cases the planar calls refuse with error 38 on D(src); like every device-pointer call this one runs on the primary device, also while
 * several devices are set (vfgs_hip_init_devices), and honours the mix there.  An empty list is no call at all.
 * Out of scope, on purpose: stripe / part forms, host-memory entry points, 4:4:4 semi-planar, persistent luma workgroups (the narrowed
 * 8-bit destination is the _copy8 call below; a model per picture is vfgs_hip_add_grain_sp_frame_list_models_dev, further down). */
typedef struct vfgs_hip_sp_frame { void* Y; void* UV; } vfgs_hip_sp_frame;
int vfgs_hip_add_grain_sp_frame_list_dev(const vfgs_hip_sp_frame* src, const vfgs_hip_sp_frame* dst,
                                         const uint32_t* seeds,      /* NULL: frame f + 1 continues frame f's registers */
                                         unsigned nframes, unsigned width, unsigned height,
                                         unsigned stride, unsigned uv_stride,   /* in samples (container elements) of a Y row / a UV row */
                                         unsigned sample_shift,      /* 0, or 16 - depth: samples sit in the high bits (P010: 6, P012: 4) */
                                         void* stream);

/* ... with the NARROWED 8-BIT DESTINATION: P010 / P210 / P012 in, NV12 / NV16 out, what a player does that decodes to 10 or 12 bit and
 * displays or encodes 8 bit (the reference CLI's --outdepth 8, yuv_to_8bit, yuv.c:216-258, folded into the store like the planar _copy8
 * calls: the clean picture stays a reference frame, the grained copy leaves at half the write traffic).
 *   src[f]       a semi-planar picture at the programmed depth (10 or 12) in uint16 containers, exactly as above; stride, uv_stride in
 *                containers, sample_shift 0 or 16 - depth;
 *   dst[f]       a semi-planar picture of uint8 containers, no shift: NV12 at 4:2:0, NV16 at 4:2:2; dst_stride, dst_uv_stride in BYTES,
 *                each >= 16 * ceil(width / 16) and a multiple of 16; pointers 16-byte aligned;
 *   seeds        NULL: one seed sequence; else a seed per picture.
 * With D(p) as above, the bytes written are those vfgs_hip_add_grain_frame_list_copy8_dev (with seeds: _seeded_copy8_dev) writes for
 * D(src[f]), Cb and Cr interleaved again: a byte is (uint8)((v + 2) >> 2) of the grained, clipped sample v at depth 10,
 * (uint8)((v + 8) >> 4) at depth 12; the four seed registers afterwards are that call's.  The low bits of a source container are ignored;
 * with sample_shift == 0 a container above the depth's range wraps as in the planar calls.  Bytes outside the whole 16-sample blocks of
 * the picture's rows (16 bytes of a Y row, 16 bytes = 8 Cb/Cr pairs of a UV row, per block) and rows outside the picture are never
 * written.  One launch per 32 frames (vfgs_hip_last_launch_info(): out8 = 1, kernel grain_sp8_kernel<depth,csuby,oney,onec>); inside an
 * overlap region the call alternates over the two internal streams like every other device-pointer call.
 * Refused before anything changes (a refused call does not reseed): everything the call above refuses, with the same codes (40: csubx != 2,
 * a bad sample_shift, width > 8192; 18, 7, 6, 5 as there); depth 8: error 16, as in the planar _copy8 calls; dst_stride or dst_uv_stride
 * too small: 6, not a multiple of 16: 8, as in the planar _copy8 list; a destination plane that shares bytes with another destination
 * plane or with ANY source plane of the call, its own frame's included: 18 -- the containers differ in size, there is no in-place form;
 * an active chroma mix: 40, "chroma mix" in the message (the kernels of the mix have no narrowed semi-planar form).
 * Out of scope, on purpose: the mix with a narrowed destination, stripe / part forms, host-memory entry points, 4:4:4, widths above 8192. */
int vfgs_hip_add_grain_sp_frame_list_copy8_dev(const vfgs_hip_sp_frame* src, const vfgs_hip_sp_frame* dst,
                                               const uint32_t* seeds,      /* NULL: frame f + 1 continues frame f's registers */
                                               unsigned nframes, unsigned width, unsigned height,
                                               unsigned stride, unsigned uv_stride,          /* source, in 16-bit containers */
                                               unsigned dst_stride, unsigned dst_uv_stride,  /* destination, in bytes */
                                               unsigned sample_shift,      /* 0, or 16 - depth */
                                               void* stream);

/* PLANAR frames in, SEMI-PLANAR surfaces out: what a software decoder hands out (vvdec, VTM, libde265, dav1d: yuv420p, yuv420p10le,
 * yuv422p10le ...) goes onto the NV12 / NV16 / P010 / P210 / P012 surface a display, a compositor or a hardware encoder takes, in ONE pass
 * instead of the planar copy list into scratch, an interleave pass and a shift-up (or narrowing) pass (measured: 0.12 .. 0.46 of their time
 * at 1080p x 32 .. 4320p x 8; against the semi-planar call above on the same bytes -3 .. +1 % at 2160p / 4320p to P010, up to +14 % where a
 * chroma row is under 2 KiB; DESIGN.md 4.7, profiles/planar_to_semiplanar.json).
 *   src[f]       a planar picture at the programmed depth: Y, U, V with LOW-aligned samples, stride / cstride in samples, exactly as in
 *                the planar list calls above;
 *   dst[f]       a semi-planar picture in the depth's container (uint8 at depth 8, uint16 at 10 and 12): Y, and UV with
 *                UV[2 i] = U[i], UV[2 i + 1] = V[i]; dst_stride, dst_uv_stride in containers, each >= 16 * ceil(width / 16) (a UV row of
 *                whole blocks is as many containers as the luma row), pitches in bytes multiples of 16, pointers 16-byte aligned;
 *   sample_shift 0, or 16 - depth (P010: 6, P012: 4); only 0 at depth 8;
 *   seeds        NULL: one seed sequence; else a seed per picture.
 * Every written container is the sample vfgs_hip_add_grain_frame_list_copy_dev (with seeds: _seeded_copy_dev) writes for the same position
 * of src[f], << sample_shift, truncated to the container; the four seed registers afterwards are that call's.  A source container above the
 * depth's range behaves exactly as in the planar calls.  Only the whole 16-sample blocks of the picture's rows are written; everything
 * else in the destination keeps its bytes.  One launch per 32 frames (vfgs_hip_last_launch_info(): listed = 1, in_place = 0, out8 = 0,
 * kernel grain_p2sp_kernel<depth,csuby,oney,onec>); inside an overlap region the call alternates over the two internal streams like
 * every other device-pointer call.  General-form models (every fgs_sei* configuration) and one-pattern models alike.
 * Refused before anything changes (a refused call does not reseed): everything the planar list calls refuse for src, with their codes
 * (18 a null list or plane, 7 a misaligned pointer, 5 / 6 / 8 geometry, ...); for dst what the semi-planar calls refuse, with theirs: 18 a
 * null list or plane, 7 a misaligned pointer, 6 / 8 a stride too small / a pitch that is no multiple of 16 bytes; error 40 with a message
 * that names the cause: csubx != 2, a bad sample_shift, width > 8192.  There is no in-place form: a destination plane that shares bytes
 * with another destination plane or with ANY source plane of the call is error 18.  An active chroma mix: error 40, "chroma mix" in the
 * message -- the mix needs the luma over a UV row in the UV workgroup's ring (as in grain_sp_mix_kernel) on top of the planar loads, which
 * is not built; a caller with a mix grains planar with the calls that honour it.  An empty list is no call at all.
 * Out of scope, on purpose: the mix, stripe / part forms, host-memory entry points, 4:4:4, widths above 8192.  The reverse direction (a
 * surface in, planes out): vfgs_hip_add_grain_sp_frame_list_to_planar_dev below.  A model per picture:
 * vfgs_hip_add_grain_frame_list_models_to_sp_dev / _to_sp8_dev below. */
int vfgs_hip_add_grain_frame_list_to_sp_dev(const vfgs_hip_frame_ptrs* src,      /* Y, U, V: planar, low-aligned */
                                            const vfgs_hip_sp_frame* dst,        /* Y, UV */
                                            const uint32_t* seeds,      /* NULL: frame f + 1 continues frame f's registers */
                                            unsigned nframes, unsigned width, unsigned height,
                                            unsigned stride, unsigned cstride,            /* source, in samples */
                                            unsigned dst_stride, unsigned dst_uv_stride,  /* destination, in containers */
                                            unsigned sample_shift,      /* 0, or 16 - depth (P010: 6, P012: 4); 0 only at depth 8 */
                                            void* stream);

/* ... with the NARROWED 8-BIT DESTINATION: planar 10- or 12-bit pictures in, NV12 / NV16 out.  As above with dst[f] a semi-planar picture
 * of bytes, dst_stride / dst_uv_stride in BYTES (each >= 16 * ceil(width / 16) and a multiple of 16); the bytes written are those of
 * vfgs_hip_add_grain_frame_list_copy8_dev (with seeds: _seeded_copy8_dev) on src[f], Cb and Cr interleaved: (uint8)((v + 2) >> 2) at
 * depth 10, (uint8)((v + 8) >> 4) at depth 12; the seed registers are that call's.  vfgs_hip_last_launch_info(): out8 = 1, kernel
 * grain_p2sp8_kernel<depth,csuby,oney,onec>.  Refusals as above; depth 8: error 16, as in the planar _copy8 calls. */
int vfgs_hip_add_grain_frame_list_to_sp8_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_sp_frame* dst,
                                             const uint32_t* seeds,      /* NULL: frame f + 1 continues frame f's registers */
                                             unsigned nframes, unsigned width, unsigned height,
                                             unsigned stride, unsigned cstride,            /* source, in 16-bit samples */
                                             unsigned dst_stride, unsigned dst_uv_stride,  /* destination, in bytes */
                                             void* stream);

/* FILM GRAIN MODELS AS DEVICE OBJECTS: a model per picture in one launch.  The programmed state is one per process, as in the reference;
 * real streams change it between pictures (AV1 film grain parameters are per frame, an FGC SEI may be re-sent for any picture, the
 * reference's CLI switches models with -c <poc>:<file>, vfgs_main.c:595-644,773-781), and re-programming per picture means one frame per
 * launch.  A MODEL is a snapshot of the programmed state that lives on the device; the list call below names one per picture.
 *
 * vfgs_hip_model_capture snapshots what the hardware layer is programmed with NOW, at the programmed depth and chroma format: pattern
 * banks, scale and pattern LUTs, scale shift, clip limits -- slots the firmware layer generated on the device included (they never visit
 * the host) -- into a device-resident table image the model owns, in the form the library would choose for pictures of ordinary width.
 * Capture changes nothing a later call can observe: not the seed registers, not the programmed state.  So a caller programs and captures
 * in turn:   vfgs_init_afgs1(&a); vfgs_hip_model_capture(&mA, s);   vfgs_init_sei(&b); vfgs_hip_model_capture(&mB, s); ...
 * The work is asynchronous on `stream`; a first use of the model on another stream waits for it there (an event, no host wait).  Inside
 * an overlap region pass the region's stream.  Refused with the codes of the processing calls: an undefined pattern-LUT entry (4), a scale
 * shift out of range (9); a null `out`: 41.  On failure *out is NULL.
 * vfgs_hip_model_release (NULL, or a handle released before: no-op) may be called as soon as the call that used the model has returned:
 * the bytes stay alive until the launches queued so far that read them are done (the buffers of released models wait in a short queue and
 * serve later captures; the ninth release in a row may wait on the host for the oldest one's readers).  vfgs_hip_shutdown releases what is left.
 * vfgs_hip_model_info: out[8] = { depth, csubx, csuby, one-pattern luma image 0/1, one-pattern chroma image 0/1, scale_shift as stored
 * (vfgs_hip_get_params), legal range 0/1, device bytes }; 0, or 41 for a null or released handle. */
typedef struct vfgs_hip_model vfgs_hip_model;                 /* opaque */
int  vfgs_hip_model_capture(vfgs_hip_model** out, void* stream);
void vfgs_hip_model_release(vfgs_hip_model* m);
int  vfgs_hip_model_info(const vfgs_hip_model* m, int out[8]);

/* A MODEL WITH A CHROMA MIX OF ITS OWN.  vfgs_hip_model_capture drops an active luma / chroma mix (vfgs_hip_set_chroma_mix): its models
 * carry none.  vfgs_hip_model_capture_mix is that call plus the mix that is active NOW: the model carries it -- per component the values and
 * the `active` flag of vfgs_hip_get_chroma_mix -- in its record, and the two list calls with a model per picture below honour it frame by
 * frame.  With no mix active the result cannot be told apart from vfgs_hip_model_capture's.  With one active the call refuses with 38 what
 * the processing calls refuse under that mix: depth 12, or a programmed model that needs a general-form pattern bank; the other refusals
 * are capture's.  The programmed state, the mix included, is unchanged either way.  Models built from AFGS1 parameter sets get their mix
 * from vfgs_hip_models_from_afgs1_mix (vfgs_hip_fw.h).
 * vfgs_hip_model_chroma_mix: out[4] = { luma_mult, chroma_mult, offset, active } of component c (1 = Cb, 2 = Cr) as the model carries them, in
 * the units of vfgs_hip_get_chroma_mix; all zero for a model without a mix.  41: a null or released handle; 37: c is neither 1 nor 2. */
int  vfgs_hip_model_capture_mix(vfgs_hip_model** out, void* stream);
int  vfgs_hip_model_chroma_mix(const vfgs_hip_model* m, int c, int out[4]);

/* Read back what a model holds on the device: the 32-byte record (clip bounds, the packed form's shift) followed by the table image, *bytes
 * (may be NULL) = their size = out[7] of vfgs_hip_model_info.  Synchronises (it waits for the work that made the model, on whatever stream);
 * for tests and debugging, like vfgs_hip_get_pattern.  41: a null or released handle; 6: `cap` is smaller than the size (or `out` is NULL),
 * with *bytes set to the size needed.  Serves captured models and models built from parameter sets (vfgs_hip_models_from_afgs1,
 * vfgs_hip_models_from_sei, vfgs_hip_fw.h) alike. */
int  vfgs_hip_model_image(const vfgs_hip_model* m, void* out, size_t cap, size_t* bytes);

/* Bookkeeping of vfgs_hip_models_from_afgs1 and vfgs_hip_models_from_sei together (vfgs_hip_fw.h), in the style of vfgs_hip_get_seeded_stream_stats: out[8] = { calls that built,
 * models built, kernel launches, copies queued, device allocations (one slab each, with its pinned job table), device frees, models per
 * launch (the constant), 0 }.  A refused call changes none of them; in the steady state of build / grain / release the allocations and frees
 * stand still. */
void vfgs_hip_get_model_build_stats(uint64_t out[8]);

/* The list call with A MODEL PER PICTURE.  src / dst / seeds / geometry exactly as in vfgs_hip_add_grain_frame_list[_seeded]_copy_dev
 * (src == dst, or dst[f]'s plane == src[f]'s plane: in place; seeds NULL: one seed sequence, frame f + 1 continues frame f's registers;
 * else a seed per picture); models: host memory, `nframes` handles, read during the call only -- repeats are the normal case.  Samples
 * written, padding left alone, and the four seed registers afterwards are those of
 *     for f in list order:
 *         program the state models[f] was captured from;
 *         if (seeds) vfgs_set_seed(seeds[f]);
 *         vfgs_hip_add_grain_frame_list_copy_dev(&src[f], &dst[f], 1, ...)
 * and the library's own programmed state is UNCHANGED by the call: it stays whatever the caller last programmed.
 * Launches: one per run of at most 32 consecutive frames whose models' images share their form (one_y, one_c of vfgs_hip_model_info);
 * a change of form inside the list starts a new launch, a change of anything else -- patterns, LUTs, scale shift, range -- does not.
 * vfgs_hip_last_launch_info(): listed = 1, kernel grain_ml_kernel<depth,csubx,csuby,oney,onec>, `launches` counts every run.  The frames'
 * model images travel in the kernel arguments like their plane pointers: no copy is queued in front of a launch on account of models.
 * MODELS THAT CARRY A MIX (vfgs_hip_model_capture_mix, vfgs_hip_models_from_afgs1_mix): "the state models[f] was captured from" includes
 * its mix, and the single-frame call of the loop honours it -- while the library's programmed mix stays what it was (none: see the
 * refusals).  Whether a model carries a mix is part of what a run shares: a launch holds at most 32 consecutive frames whose models agree
 * in (one_y, one_c, carries a mix); the VALUES of the mix may change from frame to frame inside it.  Such a run is served by
 * grain_mix_kernel<depth,csubx,csuby,false,false>, each workgroup taking image, bounds, shift and mix from its frame's model; runs without
 * a mix are grain_ml_kernel's as before.  The in-place rule is the programmed mix's: where a destination luma plane of the run shares
 * bytes with a source luma plane, the run is TWO launches, chroma first, and `launches` counts both.
 * Inside an overlap region the call alternates over the two internal streams like every device-pointer call; it runs on the primary device.
 * Refused before anything changes (a refused call does not reseed): everything the list calls refuse, with their codes (18 a null list or
 * plane, planes that share bytes; 7; 5 / 6 / 8 / 17 geometry; 15) -- except that the scale shift that counts is each model's, checked at
 * capture, and that a null `seeds` selects the single seed sequence (no error 39) -- and, error 41 with a message that names the cause:
 * models == NULL, or a NULL or released entry; a model captured at another depth or chroma format than the programmed one; width > 8192
 * (rows walked in parts); an active PROGRAMMED chroma mix ("chroma mix" in the message: a mix reaches this call in its models).  A model
 * that carries a mix adds no refusal of its own: depth and form were checked where the mix was attached.  An empty list is no call at all.
 * Out of scope, on purpose: depth 12 or general-form models under a mix, the narrowed 8-bit destination under a mix (without one:
 * vfgs_hip_add_grain_frame_list_models_copy8_dev below), stripe / part forms, widths above 8192, persistent luma workgroups (1080p
 * general-form luma runs without them here).  Semi-planar surfaces have the call below, planar pictures onto semi-planar surfaces
 * vfgs_hip_add_grain_frame_list_models_to_sp_dev / _to_sp8_dev further down; pictures in host memory have
 * vfgs_hip_host_pipe_submit, where semi-planar host surfaces and several devices are still out. */
int vfgs_hip_add_grain_frame_list_models_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_frame_ptrs* dst,
                                             const vfgs_hip_model* const* models,     /* nframes entries */
                                             const uint32_t* seeds,      /* NULL: one seed sequence; else a seed per picture */
                                             unsigned nframes, unsigned width, unsigned height,
                                             unsigned stride, unsigned cstride, void* stream);

/* ... on SEMI-PLANAR surfaces: what a player with a hardware decoder has -- NV12 / NV16 / P010 / P210 / P012 surfaces, and a grain model
 * with each of them.  src / dst / seeds / the geometry / sample_shift and the in-place rule exactly as in
 * vfgs_hip_add_grain_sp_frame_list_dev; models exactly as in vfgs_hip_add_grain_frame_list_models_dev: the same handles, captured from
 * planar or semi-planar programming alike (capture knows no frame layout).  The containers written, the bytes left alone and the four seed
 * registers afterwards are those of
 *     for f in list order:
 *         program the state models[f] was captured from;
 *         if (seeds) vfgs_set_seed(seeds[f]);
 *         vfgs_hip_add_grain_sp_frame_list_dev(&src[f], &dst[f], NULL, 1, ...)      (under the mix models[f] carries, if it carries one)
 * and the library's own programmed state, its mix included, is UNCHANGED by the call.
 * Launches: one per run of at most 32 consecutive frames whose models share (one_y, one_c, carries a mix); a change of any of the three
 * starts a new launch, a change of anything else -- the values of the mix included -- does not.  vfgs_hip_last_launch_info(): listed = 1,
 * kernel grain_spml_kernel<depth,csuby,oney,onec>, for a run of models that carry a mix grain_sp_mix_kernel<depth,csuby>; `launches` counts
 * every launch.  No copy is queued in front of a launch on account of models.  In place is ONE launch for a run without a mix (no luma
 * hazard) and TWO, UV first, for a run with one, where a destination luma plane shares bytes with a source luma plane.
 * Inside an overlap region the call alternates over the two internal streams; it runs on the primary device.
 * Refused before anything changes (a refused call does not reseed): everything vfgs_hip_add_grain_sp_frame_list_dev refuses, with its
 * codes (18 a null list or plane, planes that share bytes -- a UV plane that overlaps another frame's Y included; 7; 5 / 6 / 8 geometry);
 * error 40 for csubx != 2, a bad sample_shift, width > 8192; the scale shift that counts is each model's, checked at capture; error 41 with
 * a message that names the cause: models == NULL, a NULL or released entry, a model captured at another depth or chroma format than the
 * programmed one, an active PROGRAMMED chroma mix ("chroma mix" in the message).  Where several apply: the list checks, then 40, then 41.
 * An empty list is no call at all.
 * Out of scope, on purpose: depth 12 or general-form models under a mix, the narrowed 8-bit destination under a mix (without one:
 * vfgs_hip_add_grain_sp_frame_list_models_copy8_dev below), stripe / part forms (a planar source has
 * vfgs_hip_add_grain_frame_list_models_to_sp_dev below), semi-planar surfaces in host memory
 * (vfgs_hip_host_pipe_submit takes planar pictures), several devices, 4:4:4, widths above 8192. */
int vfgs_hip_add_grain_sp_frame_list_models_dev(const vfgs_hip_sp_frame* src, const vfgs_hip_sp_frame* dst,
                                                const vfgs_hip_model* const* models,   /* nframes entries, host memory */
                                                const uint32_t* seeds,                 /* NULL: one seed sequence; else a seed per picture */
                                                unsigned nframes, unsigned width, unsigned height,
                                                unsigned stride, unsigned uv_stride,   /* containers */
                                                unsigned sample_shift,                 /* 0, or 16 - depth */
                                                void* stream);

/* A MODEL PER PICTURE WITH THE NARROWED 8-BIT DESTINATION: a player that decodes to 10 or 12 bit, keeps the clean picture as a reference
 * frame and displays or encodes 8 bit, with film grain parameters that change from picture to picture.  src / stride / cstride exactly as
 * in vfgs_hip_add_grain_frame_list_copy8_dev (planar pictures at the programmed depth, 10 or 12, in uint16 containers), dst / dst_stride /
 * dst_cstride exactly as there (planar pictures of bytes, pitches in BYTES, each >= the bytes of a row of whole blocks and a multiple of
 * 16); models and seeds exactly as in vfgs_hip_add_grain_frame_list_models_dev.  The bytes written -- (uint8)((v + 2) >> 2) of the
 * grained, clipped sample v at depth 10, (uint8)((v + 8) >> 4) at depth 12 -- the bytes left alone and the four seed registers afterwards
 * are those of
 *     for f in list order:
 *         program the state models[f] was made from;
 *         if (seeds) vfgs_set_seed(seeds[f]);
 *         vfgs_hip_add_grain_frame_list_copy8_dev(&src[f], &dst[f], 1, ...)
 * and the library's own programmed state, its mix included, is UNCHANGED by the call.  Models are the handles of vfgs_hip_model_capture,
 * vfgs_hip_models_from_afgs1 and vfgs_hip_models_from_sei alike; general-form and one-pattern models are both served, at 4:2:0, 4:2:2,
 * 4:4:4 and 4:4:0.
 * Launches: one per run of at most 32 consecutive frames whose models' images share their form (one_y, one_c); a change of form starts a
 * new launch, a change of patterns, LUTs, scale shift or range does not.  No kernel of their own: the launches are those of the programmed
 * _copy8 list, whose kernels take image, clip bounds and shift from each frame's model where a launch names models.
 * vfgs_hip_last_launch_info(): listed = 1, out8 = 1, persistent_luma_workgroups = 0, kernel
 * grain_rw_kernel<depth,csubx,csuby,true,oney,onec,false,false>, `launches` counts every run.  Inside an overlap region the call
 * alternates over the two internal streams like every device-pointer call; it runs on the primary device.
 * Refused before anything changes (a refused call does not reseed).  Where several apply, in this order: everything
 * vfgs_hip_add_grain_frame_list_copy8_dev refuses for its lists and geometry, with its codes (18 a null list or plane, a destination plane
 * that shares bytes with another destination plane or with a source plane of another frame; 7; 5 / 6 / 8 source geometry; 15; 6 a
 * destination pitch that is too small, 8 one that is no multiple of 16) -- except that the scale shift that counts is each model's, checked
 * where the model was made, and that a null `seeds` selects the single seed sequence; depth 8: 16; then error 41 with a message that names
 * the cause: models == NULL, a NULL or released entry, a model of another depth or chroma format than the programmed one, width > 8192, an
 * active PROGRAMMED chroma mix, a model in the list that CARRIES a mix ("chroma mix" in both messages: the kernels of the mix have no
 * narrowed form with a model per frame).  An empty list is no call at all.
 * Out of scope, on purpose: models that carry a mix, widths above 8192, stripe / part forms, persistent luma workgroups.  Pictures in host
 * memory have vfgs_hip_host_pipe_submit (dst8), where semi-planar host surfaces and several devices are still out. */
int vfgs_hip_add_grain_frame_list_models_copy8_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_frame_ptrs* dst,
                                                   const vfgs_hip_model* const* models,     /* nframes entries, host memory */
                                                   const uint32_t* seeds,      /* NULL: one seed sequence; else a seed per picture */
                                                   unsigned nframes, unsigned width, unsigned height,
                                                   unsigned stride, unsigned cstride,            /* source, in 16-bit samples */
                                                   unsigned dst_stride, unsigned dst_cstride,    /* destination, in bytes */
                                                   void* stream);

/* ... on SEMI-PLANAR surfaces: P010 / P210 / P012 (or low-aligned containers) in, NV12 / NV16 out, a model with every picture.  src / dst /
 * the strides / sample_shift exactly as in vfgs_hip_add_grain_sp_frame_list_copy8_dev (never in place), models and seeds as above.  The
 * bytes written, the bytes left alone and the four seed registers afterwards are those of
 *     for f in list order:
 *         program the state models[f] was made from;
 *         if (seeds) vfgs_set_seed(seeds[f]);
 *         vfgs_hip_add_grain_sp_frame_list_copy8_dev(&src[f], &dst[f], NULL, 1, ...)
 * and the library's own programmed state, its mix included, is UNCHANGED.  Launches as above: a run of at most 32 consecutive frames whose
 * models share (one_y, one_c); vfgs_hip_last_launch_info(): listed = 1, out8 = 1, kernel grain_sp8_kernel<depth,csuby,oney,onec> -- the
 * kernels of the programmed call, which decide at run time where image, bounds and shift come from; both components of a Cb/Cr byte pair
 * take the frame's chroma bounds.
 * Refused before anything changes (a refused call does not reseed).  Where several apply: the list checks of
 * vfgs_hip_add_grain_sp_frame_list_copy8_dev with its codes (18 a null list or plane, a destination plane that shares bytes with another
 * destination plane or with ANY source plane of the call, its own frame's included; 7; 5 / 6 / 8; 15; 6 / 8 for dst_stride and
 * dst_uv_stride), then depth 8: 16, then 40 (csubx != 2, a bad sample_shift, width > 8192), then 41 as above (width aside, which is 40
 * here).  An empty list is no call at all.
 * Out of scope, on purpose: models that carry a mix, 4:4:4, widths above 8192, stripe / part forms (a planar source has
 * vfgs_hip_add_grain_frame_list_models_to_sp8_dev below), semi-planar surfaces in host memory (vfgs_hip_host_pipe_submit takes planar pictures), several devices. */
int vfgs_hip_add_grain_sp_frame_list_models_copy8_dev(const vfgs_hip_sp_frame* src, const vfgs_hip_sp_frame* dst,
                                                      const vfgs_hip_model* const* models,   /* nframes entries, host memory */
                                                      const uint32_t* seeds,                 /* NULL: one seed sequence; else a seed per picture */
                                                      unsigned nframes, unsigned width, unsigned height,
                                                      unsigned stride, unsigned uv_stride,          /* source, in 16-bit containers */
                                                      unsigned dst_stride, unsigned dst_uv_stride,  /* destination, in bytes */
                                                      unsigned sample_shift,                 /* 0, or 16 - depth */
                                                      void* stream);

/* A MODEL PER PICTURE FROM PLANAR PICTURES ONTO SEMI-PLANAR SURFACES: the software-decoder pipeline -- dav1d hands out yuv420p10le pictures,
 * each with its own AV1 film grain parameters and grain_seed, and the player wants P010 or NV12 on the device.  src / dst / stride / cstride /
 * dst_stride / dst_uv_stride / sample_shift exactly as in vfgs_hip_add_grain_frame_list_to_sp_dev (planar, low-aligned pictures in; Y and UV
 * in the depth's container out, strides in containers; never in place); models and seeds exactly as in
 * vfgs_hip_add_grain_frame_list_models_dev: the same handles -- vfgs_hip_model_capture, vfgs_hip_models_from_afgs1, vfgs_hip_models_from_sei
 * alike -- general-form and one-pattern models both, seeds == NULL: one seed sequence.  The containers written, the bytes left alone and the
 * four seed registers afterwards are those of
 *     for f in list order:
 *         program the state models[f] was made from;
 *         if (seeds) vfgs_set_seed(seeds[f]);
 *         vfgs_hip_add_grain_frame_list_to_sp_dev(&src[f], &dst[f], NULL, 1, ...)
 * and the library's own programmed state is UNCHANGED by the call.  Formats: 4:2:0 and 4:2:2 at depths 8, 10 and 12.
 * Launches: one per run of at most 32 consecutive frames whose models share (one_y, one_c); a change of form starts a new launch, a change
 * of patterns, LUTs, scale shift or range does not.  No kernel of their own: the launches are those of the programmed call, whose kernels
 * take image, clip bounds and shift from each frame's model where a launch names models; both components of a Cb/Cr pair take the frame's
 * chroma bounds.  vfgs_hip_last_launch_info(): listed = 1, in_place = 0, out8 = 0, kernel grain_p2sp_kernel<depth,csuby,oney,onec>;
 * `launches` counts every run.  No copy is queued in front of a launch on account of models.  Inside an overlap region the call alternates
 * over the two internal streams like every device-pointer call; it runs on the primary device.
 * Refused before anything changes (a refused call does not reseed).  Where several apply, in this order -- that of
 * vfgs_hip_add_grain_frame_list_to_sp_dev, then the models' checks: error 40 (csubx != 2, a bad sample_shift, width > 8192); 18 a null
 * list; 6 / 8 a destination stride too small / a destination pitch that is no multiple of 16 bytes; the list checks (18 a null plane; 7;
 * 5 / 6 / 8 / 17 source geometry -- except that the scale shift that counts is each model's, checked where the model was made; 18 a
 * destination plane that shares bytes with another destination plane or with ANY source plane of the call); 15; then error 41 with a
 * message that names the cause: models == NULL, a NULL or released entry, a model of another depth or chroma format than the programmed
 * one, an active PROGRAMMED chroma mix, a model in the list that CARRIES a mix ("chroma mix" in both messages: the to-surface kernels have
 * no form with the luma over their chroma rows).  An empty list is no call at all.
 * Out of scope, on purpose: models that carry a mix or a programmed mix, 4:4:4 surfaces, widths above 8192, stripe / part forms, a
 * semi-planar destination for vfgs_hip_host_pipe_submit, several devices. */
int vfgs_hip_add_grain_frame_list_models_to_sp_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_sp_frame* dst,
                                                   const vfgs_hip_model* const* models,   /* nframes entries, host memory */
                                                   const uint32_t* seeds,                 /* NULL: one seed sequence; else a seed per picture */
                                                   unsigned nframes, unsigned width, unsigned height,
                                                   unsigned stride, unsigned cstride,            /* source, in samples */
                                                   unsigned dst_stride, unsigned dst_uv_stride,  /* destination, in containers */
                                                   unsigned sample_shift,                 /* 0, or 16 - depth (P010: 6, P012: 4); 0 only at depth 8 */
                                                   void* stream);

/* ... with the NARROWED 8-BIT DESTINATION: planar 10- or 12-bit pictures in, NV12 / NV16 out, a model with every picture.  As above around
 * the one-frame vfgs_hip_add_grain_frame_list_to_sp8_dev: dst[f] a semi-planar picture of bytes, dst_stride / dst_uv_stride in BYTES; the
 * bytes are (uint8)((v + 2) >> 2) of the grained, clipped sample v at depth 10, (uint8)((v + 8) >> 4) at depth 12.
 * vfgs_hip_last_launch_info(): out8 = 1, kernel grain_p2sp8_kernel<depth,csuby,oney,onec>.  Refusals as above, in the same order; depth 8:
 * error 16, behind 40 and in front of everything else, as in vfgs_hip_add_grain_frame_list_to_sp8_dev. */
int vfgs_hip_add_grain_frame_list_models_to_sp8_dev(const vfgs_hip_frame_ptrs* src, const vfgs_hip_sp_frame* dst,
                                                    const vfgs_hip_model* const* models,   /* nframes entries, host memory */
                                                    const uint32_t* seeds,                 /* NULL: one seed sequence; else a seed per picture */
                                                    unsigned nframes, unsigned width, unsigned height,
                                                    unsigned stride, unsigned cstride,            /* source, in 16-bit samples */
                                                    unsigned dst_stride, unsigned dst_uv_stride,  /* destination, in bytes */
                                                    void* stream);

/* SEMI-PLANAR surfaces in, PLANAR pictures out: what a hardware decoder or a capture path hands out (NV12 / NV16 / P010 / P210 / P012) goes
 * to a consumer that takes planes -- a software encoder (x265, SVT-AV1, VTM read yuv420p / yuv420p10le), the planar calls of this library,
 * a tensor per plane -- in ONE pass instead of the semi-planar call out of place into a scratch surface, a de-interleave pass and a
 * shift-down pass (profiles/sp_to_planar.json).
 *   src[f]       a semi-planar picture: Y and UV, stride / uv_stride in containers, sample_shift -- of the SOURCE -- 0, or 16 - depth
 *                (P010: 6, P012: 4; only 0 at depth 8), exactly as in vfgs_hip_add_grain_sp_frame_list_dev;
 *   dst[f]       a planar picture at the programmed depth: Y, U, V with LOW-aligned samples, as the planar list calls take them;
 *                dst_stride, dst_cstride in samples, dst_stride >= 16 * ceil(width / 16), dst_cstride >= 8 * ceil(width / 16), pitches in
 *                bytes multiples of 16, pointers 16-byte aligned; planes may lie back to back at the smallest legal pitches;
 *   seeds        NULL: one seed sequence; else a seed per picture.
 * Samples: every written sample is what vfgs_hip_add_grain_sp_frame_list_dev writes out of place for the same container of src[f], shifted
 * right by sample_shift; U[i] is from UV[2 i], V[i] from UV[2 i + 1].  Source bits below the shift, and containers above the depth's range,
 * therefore behave as in that call.  The four seed registers afterwards are that call's.  Only the whole 16-sample blocks of the addressed
 * rows are written (a chroma row: 8 samples per block and component); everything else in the destination keeps its bytes.  One launch per
 * 32 frames (vfgs_hip_last_launch_info(): listed = 1, in_place = 0, out8 = 0, kernel grain_sp_kernel<depth,csuby,oney,onec> -- no kernel of
 * its own: the kernels of the semi-planar call decide at run time where their results go); inside an overlap region the call alternates
 * over the two internal streams like every other device-pointer call; it runs on the primary device.  General-form and one-pattern models
 * alike.
 * Never in place: a destination plane that shares bytes with another destination plane, or with any source plane of the call, is error 18.
 * Refused before anything changes (a refused call does not reseed), in the order of vfgs_hip_add_grain_frame_list_to_sp_dev with source
 * and destination swapped: error 40 with a message that names the cause (csubx != 2, a bad sample_shift, width > 8192; an active chroma
 * mix, "chroma mix" in the message); 18 a null list; 6 / 8 a destination stride too small / a destination pitch that is no multiple of 16
 * bytes; the list checks (18 a null plane, 7 a misaligned pointer, 5 / 6 / 8 source geometry, 18 planes that share bytes); 15.  An empty
 * list is no call at all.
 * Out of scope, on purpose: the narrowed 8-bit planar destination, the mix (it stays with the calls that honour it: grain the surface with
 * vfgs_hip_add_grain_sp_frame_list_dev), stripe / part forms, host memory and the host pipe, 4:4:4, widths above 8192, several devices. */
int vfgs_hip_add_grain_sp_frame_list_to_planar_dev(const vfgs_hip_sp_frame* src,      /* Y, UV: as in vfgs_hip_add_grain_sp_frame_list_dev */
                                                   const vfgs_hip_frame_ptrs* dst,    /* Y, U, V: planar, LOW-aligned, as the planar list calls take them */
                                                   const uint32_t* seeds,             /* NULL: one seed sequence; else a seed per picture */
                                                   unsigned nframes, unsigned width, unsigned height,
                                                   unsigned stride, unsigned uv_stride,        /* source, in containers */
                                                   unsigned dst_stride, unsigned dst_cstride,  /* destination, in samples */
                                                   unsigned sample_shift,             /* of the SOURCE: 0, or 16 - depth; only 0 at depth 8 */
                                                   void* stream);

/* ... with A MODEL PER PICTURE: models and seeds exactly as in vfgs_hip_add_grain_sp_frame_list_models_dev, everything else as above.  Every
 * written sample is what that call writes out of place for the same container, shifted right by sample_shift; the seed registers are that
 * call's; the library's own programmed state is UNCHANGED.  Launches: one per run of at most 32 consecutive frames whose models share
 * (one_y, one_c); vfgs_hip_last_launch_info(): kernel grain_spml_kernel<depth,csuby,oney,onec>, `launches` counts every run.
 * Refusals as above, in the same order, except that the scale shift that counts is each model's and that a programmed mix is the models'
 * to refuse; then, behind 15, error 41 with a message that names the cause: models == NULL, a NULL or released entry, a model of another
 * depth or chroma format than the programmed one, an active PROGRAMMED chroma mix, a model in the list that CARRIES a mix ("chroma mix" in
 * both messages; out of scope here: the mix stays with the calls that honour it). */
int vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev(const vfgs_hip_sp_frame* src, const vfgs_hip_frame_ptrs* dst,
                                                          const vfgs_hip_model* const* models,   /* nframes entries, host memory */
                                                          const uint32_t* seeds,                 /* NULL: one seed sequence; else a seed per picture */
                                                          unsigned nframes, unsigned width, unsigned height,
                                                          unsigned stride, unsigned uv_stride,        /* source, in containers */
                                                          unsigned dst_stride, unsigned dst_cstride,  /* destination, in samples */
                                                          unsigned sample_shift,                 /* of the SOURCE: 0, or 16 - depth; only 0 at depth 8 */
                                                          void* stream);

/* What a seeded launch uploads, host only (no GPU needed), the counterpart of vfgs_hip_lfsr_segments below: out[f * seg_words + k],
 * f < nseg, k < seg_words = the 32-bit register (vfgs_hw.c:74-79) after first_bit + 32 * k steps from seeds[f] << 1 (vfgs_hw.c:343).
 * `out` holds nseg * seg_words 32-bit words.  first_bit is reached by one jump (a 32 x 32 bit matrix, log2(first_bit) squarings),
 * never by stepping.  For a launch over lines [part_y, part_y + part_height) of pictures `width` wide the library uses, with
 * nblk = ceil(width / 16), b = part_y / 16 and nbr = the block rows the part touches: first_bit = max(b - 1, 0) * nblk,
 * seg_words = ceil((32 + nblk + nbr * nblk + 64) / 32) + 1.  0, or error 19 (a null pointer, nseg or seg_words 0). */
int vfgs_hip_seed_segments(const uint32_t* seeds, unsigned nseg, uint64_t first_bit, unsigned seg_words, uint32_t* out);
/* out[4] = { seeded images built and uploaded (one per launch), 32-bit words of the most recent one, calls that waited on the host
 * (longer than 20 us) for a slot of the images' ring -- a slot packs the images of consecutive calls, 256 KiB by default, and is
 * overwritten only after every kernel that read it --, 1 if the most recent launch read a seeded image }. */
void vfgs_hip_get_seeded_stream_stats(uint64_t out[4]);

/* {rnd, rnd_up, line_rnd, line_rnd_up} as the reference would hold them (vfgs_hw.c:52-55). */
void vfgs_hip_get_seed_state(uint32_t out[4]);

/* The rest of the programmed state, for tests and debugging (host only, no GPU needed):
 * component c's scale and pattern LUTs as vfgs_hw.c:50-51 holds them (either pointer may be NULL), and
 * out[8] = { scale_shift as stored (vfgs_hw.c:56: shift + 6 - bs), bs, Y min, Y max, C min, C max, csubx, csuby }. */
int vfgs_hip_get_luts(int c, unsigned char scale[256], unsigned char pattern[256]);
void vfgs_hip_get_params(int out[8]);
/* ... and of the device copy of the LFSR bit stream (the reference steps its registers, vfgs_hw.c:74-79,309-310; here a window of the
 * stream lives in device memory): out[4] = { windows uploaded in a caller's stream (a bubble between two of its kernels), windows
 * built ahead on the library's copy stream, switches to a window built ahead, 32-bit words of the current window }. */
void vfgs_hip_get_stream_stats(uint64_t out[4]);
/* A batch of stripes (vfgs_hip_add_grain_frames_part_dev, vfgs_hip_add_grain_frame_list_part_dev: what one rank of a stripe split runs
 * per step) that covers at most about two thirds of its frames reads short runs of that stream, a whole frame's steps apart
 * (vfgs_hw.c:291-298,309-310: (ceil(height / 16) - 1) x ceil(width / 16) steps per frame).  The library builds those runs alone, each
 * from the one before by a jump -- the step of vfgs_hw.c:74-79 is linear over GF(2), n steps are one 32 x 32 bit matrix -- and
 * uploads the NEXT call's runs while this call's kernel works: out[4] = { images built in a caller's stream, images built ahead on
 * the copy stream, switches to an image built ahead, 1 if the most recent launch read such an image }.  The environment variable
 * VFGS_HIP_STRIPE_JUMP=0 keeps the contiguous window for those calls too (results are the same either way). */
void vfgs_hip_get_stripe_stream_stats(uint64_t out[4]);
/* The generator behind it, host only (no GPU needed): out[f * seg_words + k], f < nseg, k < seg_words = the 32-bit register
 * (vfgs_hw.c:74-79) after first_bit + f * step_bits + 32 * k steps from `reg` -- what `prng` would return after stepping
 * that far, without the stepping.  0 or an error code. */
int vfgs_hip_lfsr_segments(unsigned int reg, uint64_t first_bit, uint64_t step_bits, unsigned nseg, unsigned seg_words, uint32_t* out);

/* Last error of a vfgs_hip_* call (0 = none) and its text. */
int vfgs_hip_last_error(void);
const char* vfgs_hip_last_error_string(void);

/* Timing helper for harnesses: average device time in microseconds of the grain kernels
 * launched between begin/end on `stream` (hipEvent pair on that stream). */
int vfgs_hip_timer_begin(void* stream);
int vfgs_hip_timer_end(void* stream, float* elapsed_ms);

/* Overlap region for device-resident frames that arrive ONE PER CALL (the reference's call pattern, vfgs_main.c:771-790, with the
 * frames already in HBM): a kernel launch pays its fill and drain -- a 4320p frame runs at 0.60 of the HBM peak alone and at 0.72
 * when the next frame's launch overlaps its tail.  Between _begin(stream) and _end(stream) the caller promises that the
 * device-pointer calls it makes on `stream` are independent of each other (distinct frames) and of anything else queued on
 * `stream` after _begin; the library runs them alternately on two internal streams forked from `stream` at _begin and joined
 * back into it at _end (events only there, nothing between the launches).  Work queued on `stream` before _begin is complete
 * before the first call starts; work queued after _end sees every result.  Results and seed registers are those of the same
 * calls without the region.  One region at a time.  0 or an error code.  (The first region of a process creates the two
 * internal streams and their hardware queues: about 10 ms, once.) */
int vfgs_hip_overlap_begin(void* stream);
int vfgs_hip_overlap_end(void* stream);

/* Several devices in ONE process, for frames that live in host memory (SURVEY 8e x 8f row f3; the reference's frame loop and
 * file I/O, vfgs_main.c:664-682 / yuv.c:162-214, are one process and one thread).  After this call vfgs_add_grain_stripe and
 * vfgs_hip_add_grain_frames_host give every listed device a stripe of whole 16-line block rows of each frame and run the
 * devices concurrently (one PCIe link each, no exchange between them); results and seed registers are those of the
 * single-device call.  devices[0] is the library's device for everything else (the device-pointer entry points, the line
 * call).  A device may be listed more than once (testing on a one-GPU machine).  n = 1 returns to one device.
 * 0 or an error code. */
int vfgs_hip_init_devices(const int* devices, int n);

/* 1 if vfgs_set_depth(depth) is accepted (8, 10, 12), else 0: a way to ask that does not abort like the void drop-in call.
 * Host only, no GPU needed. */
int vfgs_hip_supports_depth(int depth);

/* 1 if this library was built by a developer tool with tuning or ablation knobs (its output may be wrong by design),
 * 0 for the product build.  versatilefilmgrain_amd/build.py only ever builds the latter. */
int vfgs_hip_dev_build(void);

/* SURVEY 8f row f3 -- the data path around the reference's yuv_read / yuv_write (yuv.c:162-214): nframes frames that live
 * in HOST memory, processed in place and pipelined through a ring of three device frames: the upload of frame i, the
 * kernel of frame i-1 and the download of frame i-2 are queued on three streams.  Y/U/V: arrays of nframes plane pointers
 * (any host memory; frames need not be contiguous), all frames with the same geometry, strides in samples as in
 * vfgs_add_grain_stripe.  Only the bytes the reference touches (whole 16-sample blocks of every row) travel; stride
 * padding is never written.  Pinned memory (vfgs_hip_host_alloc) makes the copies asynchronous; with pageable memory the
 * call is correct but the runtime stages every copy and the calling thread blocks for it.  Returns when all frames are
 * back in host memory; the seed registers have advanced as after nframes whole-frame calls.  0 or an error code. */
int vfgs_hip_add_grain_frames_host(void* const* Y, void* const* U, void* const* V, unsigned nframes, unsigned width,
                                   unsigned height, unsigned stride, unsigned cstride);
void* vfgs_hip_host_alloc(uint64_t bytes);   /* pinned host memory (hipHostMalloc); NULL on failure */
void vfgs_hip_host_free(void* p);

/* PICTURES IN HOST MEMORY AS A STREAM: what a software decoder (dav1d, vvdec, VTM, libde265) hands out -- planar pictures in host memory,
 * one at a time, each with its own grain_seed and usually its own parameter set -- through the pipeline of the call above, fed picture by
 * picture.  A pipe is opened for one geometry at the programmed depth and chroma format; vfgs_hip_host_pipe_submit queues upload, launch and
 * download of ONE picture on the library's three pipeline streams and returns a ticket; vfgs_hip_host_pipe_wait(ticket) returns when that
 * picture and every earlier one of the pipe are in host memory.
 * desc: width / height / stride / cstride as in vfgs_hip_add_grain_frames_host (strides in samples).  dst_stride = dst_cstride = 0: every
 * picture is grained in place.  Else every picture has a destination of its own in host memory, rows of dst_stride / dst_cstride
 * destination samples: samples of the source's size, or with dst8 = 1 (depth 10 or 12) bytes, narrowed in the store as in the _copy8 calls.
 * slots: pictures in flight, 0 = 3, else 2..8; a slot holds a device source and, with a destination, a device destination, at pitches of
 * the library's choosing.
 * WHAT A SUBMIT COMPUTES.  After wait(ticket) returned 0 the destination bytes, the bytes left alone and the source are what the matching
 * one-picture device call gives, had the planes been device memory at the moment of the submit:
 *     model, no dst8                        vfgs_hip_add_grain_frame_list_models_dev(&s, &d, &model, seed, 1, ...)
 *     model, dst8                           vfgs_hip_add_grain_frame_list_models_copy8_dev
 *     model == NULL, seed == NULL           vfgs_hip_add_grain_frame_list_copy_dev        dst8: ..._copy8_dev
 *     model == NULL, a seed                 vfgs_hip_add_grain_frame_list_seeded_copy_dev dst8: ..._seeded_copy8_dev
 * (model == NULL: the programmed state as it is at the submit; seed == NULL: the running seed sequence; *seed is read during the call.)
 * Only whole 16-sample blocks of every row travel: stride padding is never written, and a source with a destination of its own is never
 * written at all.  A model that carries a mix is honoured as in the device call.  THE FOUR SEED REGISTERS move at the submit, on the host,
 * exactly as that device call moves them -- vfgs_hip_get_seed_state right behind a submit is the device call's -- so submits interleave
 * with every other entry point in one seed sequence.  The programmed state is left alone, as by the calls with models.
 * HOST MEMORY: source and destination planes stay valid and untouched until the picture's wait returns; the model may be released as soon
 * as submit returns.  Pinned memory (vfgs_hip_host_alloc) makes the copies asynchronous; pageable memory is correct and blocks the caller
 * in submit, as in the call above.  A submit that finds every slot in flight waits on the host for the pipe's oldest picture
 * (back-pressure; no error).
 * TICKETS count 1, 2, 3 ... per pipe; a wait on a ticket that is home returns 0 again.  THREADS: one thread may submit while another
 * waits on the same pipe -- wait does not hold the library's lock while it sleeps --; several pipes, of different geometry, may be open at
 * once (their pictures share the three streams: all of them come home in the order of their submits).  close drains the pipe and frees
 * its ring; vfgs_hip_shutdown drains and closes whatever is open, and every handle is stale behind it.
 * vfgs_hip_last_launch_info(): internal = 1, listed = 1, and the kernel the matching device call records.
 * REFUSED with nothing queued, no ticket issued, no register moved and the pipe usable as before: everything the matching device call
 * refuses, with that call's code and text behind the name of the pipe's function -- 5 / 6 / 8 / 17 and 15 for the geometry (the caller's
 * strides) and 16 for dst8 at depth 8, all at open; at submit 18 (a null plane; a destination plane that shares bytes with another one or
 * with a plane of the source), 41 (the model: NULL entry aside, released, another depth or format, width > 8192, a programmed mix beside
 * a model, a model that carries a mix with dst8), 38, 9 and 4 (the programmed state of a submit without a model).  Error 43, the pipe's
 * own, with the cause in the message: a null desc, out, p, src or ticket; a closed or unknown handle (never dereferenced); slots outside
 * 2..8; dst8 with zero destination strides; pictures without lines; a dst on a pipe opened in place, or none on one opened with
 * destination strides; a wait on a ticket never issued; a submit after the programmed depth or chroma format changed since open; a submit
 * while an overlap region is open; open or submit with more than one device of vfgs_hip_init_devices.  A HIP error in mid-stream drains
 * the three streams before it is returned.
 * Out of scope, on purpose: semi-planar host surfaces, a semi-planar destination, several devices, polling without waiting. */
typedef struct vfgs_hip_host_pipe vfgs_hip_host_pipe;          /* opaque */
typedef struct vfgs_hip_host_pipe_desc {
	unsigned width, height;            /* luma samples, every picture of the pipe */
	unsigned stride, cstride;          /* source rows in samples, as vfgs_hip_add_grain_frames_host */
	unsigned dst_stride, dst_cstride;  /* destination rows in destination samples (bytes with dst8); 0, 0: every picture in place */
	int      dst8;                     /* 1: planar 8-bit destination, narrowed in the store (depth 10 / 12) */
	unsigned slots;                    /* pictures in flight: 0 = 3, else 2..8 */
} vfgs_hip_host_pipe_desc;
int vfgs_hip_host_pipe_open(const vfgs_hip_host_pipe_desc* desc, vfgs_hip_host_pipe** out);
int vfgs_hip_host_pipe_submit(vfgs_hip_host_pipe* p,
                              const vfgs_hip_frame_ptrs* src,    /* HOST planes, line 0 */
                              const vfgs_hip_frame_ptrs* dst,    /* NULL: in place; else HOST planes */
                              const vfgs_hip_model* model,       /* NULL: the programmed state as it is now */
                              const uint32_t* seed,              /* NULL: the running seed sequence */
                              uint64_t* ticket);
int vfgs_hip_host_pipe_wait(vfgs_hip_host_pipe* p, uint64_t ticket);   /* this picture and every earlier one are in host memory */
int vfgs_hip_host_pipe_close(vfgs_hip_host_pipe* p);                   /* drains, frees the ring */

/* Introspection for benchmarks/tests. */
int vfgs_hip_device_info(int* cu_count, int* lds_bytes_per_cu, int* clock_khz, char* name, int name_len);

/* What the most recent grain launch of this process (primary device) actually dispatched -- so that a benchmark labels
 * its numbers with the kernel that ran instead of the kernel it expects.  EVERY grain launch is recorded and counted in
 * `launches`, also those the host-memory entry points make on the library's own staging buffers (`internal` = 1: a line of
 * vfgs_add_grain_line, the stripes it computes ahead -- including ones that are dropped later --, vfgs_add_grain_stripe,
 * vfgs_hip_add_grain_frames_host): after a walk through the line call the record describes such a stripe launch.  `kernel` is the instantiation's name as the
 * profiler prints it (e.g. "grain_rw_kernel<10,2,2,false,false,true,false,false>": depth, chroma subsampling
 * x / y, 8-bit destination of a 10- or 12-bit path, luma one-pattern form, chroma one-pattern form, rows walked in parts,
 * persistent luma workgroups; with a chroma mix active "grain_mix_kernel<10,2,2,false,false>": depth, chroma subsampling x / y,
 * 8-bit destination, rows walked in parts -- an in-place call is two launches of it).  Returns 0, or -1 when nothing has been launched yet. */
typedef struct vfgs_hip_launch_info {
	int depth, csubx, csuby;          /* sample depth and chroma format the launch was compiled for */
	int out8;                         /* 1: 10- or 12-bit source narrowed to 8 bit in the store */
	int one_y, one_c;                 /* 1: one-pattern form of the luma / chroma table image */
	int in_place;                     /* 1: destination planes == source planes */
	int nframes;                      /* frames of the launch */
	int workgroups_per_frame;         /* luma + 2 x chroma */
	int frames_per_front;             /* frames swept at the same time (1 or 2) */
	int rows_per_wave[2];             /* luma, chroma: rows of one block row a wave walks */
	int positions_per_row[2];         /* luma, chroma: 1 KiB wave accesses per row */
	int parts_per_row;                /* passes over the block-parameter table a row needs (1 up to 512 blocks = 8192 samples per row) */
	int persistent_luma_workgroups;   /* 0, or the number of luma workgroups that share the launch's luma tasks (general-form luma of small pictures) */
	int waves_per_workgroup;
	int lds_bytes_per_workgroup;      /* LDS the kernel allocates: table image + block parameters (the 10- and 12-bit all-one-pattern kernels: padded to 40,960, four workgroups per CU) */
	unsigned long long launches;      /* grain launches of this process so far */
	char kernel[96];
	int listed;                       /* 1: the frames' plane pointers came as a list (vfgs_hip_add_grain_frame_list_*) */
	int internal;                     /* 1: launched by a host-memory entry point on the library's staging buffers, not on a caller's device planes */
} vfgs_hip_launch_info;
int vfgs_hip_last_launch_info(vfgs_hip_launch_info* out);

#ifdef __cplusplus
}
#endif

#endif /* VFGS_HIP_H */
