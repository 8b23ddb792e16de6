// Shared between the host state machine (vfgs_host.cpp) and the gfx950 kernels
// (vfgs_kernel.hip): the LDS image of the pattern banks + LUTs and the launch record.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace vfgs {

constexpr int kSlots = 8;        // pattern slots per component, vfgs_hw.h:49
constexpr int kMaxUnits = 64;    // 16-byte units per position (one per lane)
constexpr int kBlock = 16;       // luma samples per grain block

// Tuning knobs (defaults are the shipped configuration; tools/dev/build_variant.sh overrides them).  They change HOW the
// kernels run, never WHAT they compute: the timing-only probes with wrong output that rounds 2 and 3 kept in the kernel source
// (their results: profiles/r02_variants*.log, r03_ab*.log) were removed in round 4, and so were the knobs of
// round 2's tiled kernels when the row walk became the only kernel family.
#ifndef VFGS_WAVES
#define VFGS_WAVES 4          // waves per workgroup (power of two); they share one LDS image
#endif
#ifndef VFGS_WG_PER_CU
#define VFGS_WG_PER_CU 4      // resident workgroups per CU the register allocation is sized for
#endif
#ifndef VFGS_SCHED_FENCE
#define VFGS_SCHED_FENCE 1    // 1: a scheduling fence after every position keeps its store and refill in program order
#endif
#ifndef VFGS_LDAUX_ALIGNED
#define VFGS_LDAUX_ALIGNED 2  // cache policy bits of the sample loads (gfx940+: 1 = sc0, 2 = nt, 16 = sc1): nontemporal
#endif
#ifndef VFGS_STAUX_ALIGNED
#define VFGS_STAUX_ALIGNED 2  // ... of the sample stores
#endif
// Register sets of a wave's ring = positions (1 KiB wave accesses) it has in flight: a position is stored that many positions after its load
// was issued.  Pure streams at the kernels' occupancy prefer a SHORT distance between the load and the store of the same bytes (tools/walk_probe.hip
// depth: one set 0.775, two 0.744, four 0.727 of 8 TB/s at 16-20 waves per CU, profiles/r06_walk_ring_depth.log), the kernels need the loads of the
// next positions in flight while they compute this one: four for the general forms and at 10 bit (two: -1 % at the headline, -3 % for the 8-bit general form),
// two for the packed 16-bit planes of the 8-bit one-pattern kernels (+1.3 .. 3 %, and 8 VGPRs fewer: six waves per SIMD without a spill, +1.4 .. 3.4 %
// together; profiles/r06_ab3 .. r06_ab5).
#ifndef VFGS_RING
#define VFGS_RING 4           // general-form planes
#endif
#ifndef VFGS_RING_ONE10
#define VFGS_RING_ONE10 4     // one-pattern planes at 10 bit
#endif
#ifndef VFGS_RING_PK
#define VFGS_RING_PK 2        // packed 16-bit planes (8-bit one-pattern form)
#endif
#ifndef VFGS_RING_NARROW10
#define VFGS_RING_NARROW10 2  // one-pattern planes at 10 bit whose rows are one or two positions (1080p chroma): 1080p fgs_sei +2.4 % at 8, +1.1 % at 32 frames per launch, ff_test1 +0 .. 0.3 % (profiles/r06_ab8)
#endif
// Resident workgroups per CU of the all-one-pattern kernels, held there by unused LDS behind their tables (lds_allocation below; 0 = as many as fit).
// Their 15 KB of LDS and ~80 registers would let SIX in: 24 waves with four 1 KiB loads each in flight per CU, and the memory system answers a CU
// that asks for less at once better (tools/walk_probe.hip depth: 20-24 KiB of loads in flight per CU stream at 0.79-0.80 of 8 TB/s, 64-96 KiB at
// 0.73-0.75).  At 10 bit FOUR are worth +1.5 .. 4 % from 720p to 4320p (three: up to +5.7 % at 1080p / 2160p, -5 % at 720p;
// profiles/r06_ab13_workgroups_per_cu.log, r06_ab14_workgroups_per_cu_sizes.log); the 8-bit kernels (twice the arithmetic per byte) lose 2-3 % at five
// and four and keep their six.  The general-form kernels are at four by their 40 KB image, and three cost them 2.5 % (r06_ab11).
#ifndef VFGS_ONE10_WG_PER_CU
#define VFGS_ONE10_WG_PER_CU 4
#endif
#ifndef VFGS_ONE8_WG_PER_CU
#define VFGS_ONE8_WG_PER_CU 0
#endif
#ifndef VFGS_RW_CONSEC
#define VFGS_RW_CONSEC 0      // 1 = a wave's rows are consecutive, 0 = the waves of a workgroup take every kWavesPerWG-th row
#endif
// Two frame fronts in one launch (KernelArgs::lfronts == 1): 1 = the odd front of a pair starts one plane phase later (Cb, Cr, Y), so that luma
// and chroma workgroups share the CUs; the launch's last pair keeps the order of memory (front_phase / front_task below).  0 = both fronts
// in the order of memory, 2 = the last pair rotated as well.  4320p 10-bit 4:2:0 fgs_sei x 8: 1 is worth 1.5 % and 2.2 % on two boxes against
// a parent-to-parent spread of 0.01 % and 0.24 %, 2 half of that (the launch drains on luma workgroups); profiles/front_phase.json.
#ifndef VFGS_FRONT_PHASE
#define VFGS_FRONT_PHASE 1
#endif

// The product is built with every knob at its default (versatilefilmgrain_amd/build.py passes none).  The developer tools that
// time variants (tools/dev/build_variant.sh, tools/gpu_variants.sh) define VFGS_DEV_BUILD; without it any
// other value is a build error, so a stray -D cannot produce a library that silently runs something else -- and a
// developer build says so at run time (vfgs_hip_dev_build(), refused by versatilefilmgrain_amd.hw unless asked for).
#if !defined(VFGS_DEV_BUILD)
#if VFGS_WAVES != 4 || VFGS_WG_PER_CU != 4 || VFGS_RING != 4 || VFGS_RING_ONE10 != 4 || VFGS_RING_PK != 2 || VFGS_RING_NARROW10 != 2 || VFGS_ONE10_WG_PER_CU != 4 || VFGS_ONE8_WG_PER_CU != 0 || VFGS_SCHED_FENCE != 1 || VFGS_LDAUX_ALIGNED != 2 || VFGS_STAUX_ALIGNED != 2 || VFGS_RW_CONSEC != 0 || VFGS_FRONT_PHASE != 1 || \
    defined(VFGS_NO_FRONTS) || defined(VFGS_NO_LOOKAHEAD) || defined(VFGS_NO_ONE_PATTERN) || defined(VFGS_NO_PK16) || defined(VFGS_PK_NO_READ2) || defined(VFGS_PK_WAVES) || defined(VFGS_ONE10_WAVES) ||  defined(VFGS_RW_WG_BYTES) || defined(VFGS_RW_MIN_FILL_PCT) || defined(VFGS_PERSIST_MIN_TASKS) || defined(VFGS_PERSIST_MAX_WG_KB)
#error "libvfgs_hip: a tuning knob differs from the shipped configuration; developer variants must define VFGS_DEV_BUILD"
#endif
#endif

constexpr int kWavesPerWG = VFGS_WAVES;
#ifdef VFGS_NO_PK16               // developer builds only: the 8-bit one-pattern components keep round 5's byte bank + dword LUT (same-box A/Bs)
constexpr bool kPk16 = false;
#else
constexpr bool kPk16 = true;      // 8-bit one-pattern components use the packed 16-bit form (below)
#endif

// The kernels (vfgs_kernel.hip "Row walk"): a wave streams whole rows, the workgroup's block parameters live in LDS
// behind the table image: two tables (this block row's registers, the block row above's) of one dword per grain block +
// one block in front.  A table holds kTileBlocks blocks: a row of more blocks is walked in parts, the table refilled between them.
constexpr int kTileBlocks = 512;
constexpr int kParamEntries = kTileBlocks + 4;   // entry e = block e - 1; the lanes behind a row's end read up to block nblk + 2 (clamped values)
constexpr int kParamTableBytes = (kParamEntries * 4 + 15) & ~15;
constexpr int kParamBytes = 2 * kParamTableBytes;

// LDS a grain kernel ALLOCATES: what it uses (table image + block parameters), padded where its class is held at fewer resident
// workgroups per CU than would fit (VFGS_ONE10_WG_PER_CU / VFGS_ONE8_WG_PER_CU above): a size with which exactly that many are resident.
// The kernels with one-pattern luma at 10 bit (rows walked in parts included: 92-95 registers, five would be resident -- 16384-wide AFGS1 +2.5 % at two
// frames per launch, +1 % at four: profiles/r06_ab18) need 15 KB and allocate 40; the kernels with a general-form plane are at four by their 40 KB image.
// (depth10: the 16-bit containers, 10 AND 12 bit -- a 12-bit kernel moves the same bytes through the same LDS image as its 10-bit twin and gets
// every decision of it: this allocation, the ring depths VFGS_RING_ONE10 / VFGS_RING_NARROW10 above, persistence)
constexpr int kLdsPerCU = 163840;
constexpr int lds_allocation(const bool depth10, const bool one_y, const bool one_c, const bool wide, const int need)
{
	// (10 bit: every kernel whose LUMA is one-pattern -- over general-form chroma at 4:2:0 / 4:2:2 it needs 15-23 KB and five would be resident: +0.9 .. 1.3 %,
	// profiles/r06_ab23; over general-form chroma at 4:4:4 the 40 KB image decides anyway)
	const int cap = (depth10 && one_y) ? VFGS_ONE10_WG_PER_CU : ((!depth10 && one_y && one_c && !wide) ? VFGS_ONE8_WG_PER_CU : 0);
	if (cap <= 0) return need;
	const int target = (kLdsPerCU / cap) & ~2047;        // exactly `cap` workgroups resident (well inside any allocation granule) ...
	const int next = (kLdsPerCU / (cap + 1)) & ~2047;    // ... and a size with which cap + 1 would be
	return need > next ? need : (target < 65536 ? target : 65536);
}

// The kernels of the luma / chroma mix (grain_mix_kernel): four workgroups per CU at either depth -- their chroma waves hold the luma over
// their samples in the ring as well and are compiled for 128 registers -- and an LDS allocation that says the same.
constexpr int kMixWgPerCU = 4;
constexpr int mix_lds_allocation(const int need)
{
	const int target = (kLdsPerCU / kMixWgPerCU) & ~2047;
	return need > target ? need : target;
}

// The kernels of semi-planar frames (grain_sp_kernel, vfgs_kernel.hip "UV walk"): luma workgroups are the row walk's; a UV workgroup serves
// BOTH chroma components of its rows and holds both components' tables in LDS:
//   one-pattern chroma : [Cb sub-image][Cr sub-image]                  (each component's +scale table and its own pattern with the negated copy)
//   general form       : [LUT Cb: 2 x 256 dwords][LUT Cr][chroma bank] (the bank once)
// followed by FOUR parameter tables (Cb: this block row, the row above; Cr: the same).  A lane's memory unit is 32 bytes of the
// interleaved row, a wave access 2 KiB, and the ring holds kSpRing of them (as many bytes in flight per wave as the planar kernels' ring of four).
constexpr int kSpRing = 2;
constexpr int kSpWgPerCU = 4;      // resident workgroups per CU of every grain_sp_kernel: its launch bounds AND its LDS allocation (sp_lds_allocation)
constexpr int kSpUnitBytes = 32;
constexpr int sp_uv_image_bytes(const int c_bytes, const int lut_bytes, const bool one_c) { return one_c ? 2 * c_bytes : c_bytes + lut_bytes; }
constexpr int sp_lds_need(const int y_bytes, const int c_bytes, const int lut_bytes, const bool one_c)
{
	const int y = y_bytes + kParamBytes, uv = sp_uv_image_bytes(c_bytes, lut_bytes, one_c) + 2 * kParamBytes;
	return y > uv ? y : uv;
}

// (what a semi-planar kernel ALLOCATES: exactly kSpWgPerCU workgroups per CU, like the kernels of the mix)
constexpr int sp_lds_allocation(const int need)
{
	const int target = (kLdsPerCU / kSpWgPerCU) & ~2047;
	return need > target ? need : target;
}

// The kernels of semi-planar frames under the luma / chroma mix (grain_sp_mix_kernel): a UV wave keeps, per ring position, its 32 bytes of UV
// AND the 32 bytes of luma over them, and per component the index dwords and their carries beside the samples': more than the 128 registers of
// four workgroups per CU.  THREE workgroups per CU (three waves per SIMD: 168 registers), by launch bounds and by an LDS allocation that says
// the same; the ring keeps the two positions of grain_sp_kernel.
constexpr int kSpMixRing = 2;
constexpr int kSpMixWgPerCU = 3;
constexpr int sp_mix_lds_allocation(const int need)
{
	const int target = (kLdsPerCU / kSpMixWgPerCU) & ~2047;
	return need > target ? need : target;
}

// Device image of everything the kernel looks up: one sub-image per plane type (luma; chroma) -- or per chroma
// component -- and a workgroup (which works on ONE plane) copies the sub-image of its plane to LDS offset 0.
//
//   luma image  : [LUT Y : 2 x 256 dwords] [luma bank]          (one-pattern form: 1 x 256 dwords, the +scale table, then the bank and its negated copy)
//   Cb image    : [LUT Cb: 2 x 256 dwords] [chroma bank]        (general form: the chroma bank is stored twice in the device image, so that a
//   Cr image    : [LUT Cr: 2 x 256 dwords] [chroma bank]         workgroup -- which serves ONE component -- stages one LUT pair, not two: with both,
//                                                                 the 4:4:4 chroma image was 2 KB larger than the luma image and a CU held three
//                                                                 workgroups where the kernels are built for four)
//             or: [LUT Cb] [bank of Cb's pattern]   and   [LUT Cr] [bank of Cr's pattern]          (one-pattern form)
//
// GENERAL form of a bank ("slot-interleaved"): for every (row, column) position the eight slots' int8 values sit in 8
// consecutive bytes, so the LDS address of a sample's pattern data does NOT depend on the sample's intensity (the slot
// is picked afterwards in registers with v_perm_b32); four samples are two ds_read_b128.  Each bank row is padded by one
// 16-byte slot so consecutive rows rotate through the sixteen 16-byte LDS slots of a 256-byte bank row.
//
// ONE-PATTERN form: when a component's pattern LUT selects the same slot for every intensity (all AFGS1 models, the
// single-pattern SEI models, the chroma of the default SEI model) only that pattern is stored, one byte per sample, rows
// padded by 16 bytes; four samples are one dword.  An eighth of the LDS traffic and of the LDS footprint.  The bank is
// followed by its NEGATED copy (y_neg / c_neg bytes further on): a block's random sign then is a choice of bank, made once
// per block and row in the address, the values that come out of LDS are the true signed grain (plain edge filter, no
// relative signs) and every sample uses the +scale table at LDS offset 0 (no table select in the gather address).  The host
// only chooses this form for patterns without the value -128, which has no negation in a byte (the firmware's generators
// clip to +-127, vfgs_fw.c:321-323,494).
//
// ONE-PATTERN form at 8 BIT ("packed 16-bit form", round 6): the bank holds the pattern as int16 values (rows of 2 x columns + 16
// bytes, followed by the negated copy) and the LUT is the plain table of the 256 scale BYTES (vfgs_hw.c:50).  Two samples then
// share every vector instruction behind the gathers: a pair's pattern values arrive packed out of LDS (four samples = one
// ds_read_b64), v_pk_mad_i16 (pattern x scale + 2^(shift-1)), v_pk_ashrrev_i16, and the packed add / max / min of the clip --
// exact because |P| <= 127 and the host only chooses the form when max(scale) * 127 + 2^(shift-1) <= 32767 (image_form in
// vfgs_host.cpp; otherwise the general form serves the component).  The two samples at a block edge (after the 3-tap filter
// up to +-159) and the two overlap lines of a block row (after the blend up to +-199) keep 32-bit products.
//
// LUT (one dword per 8-bit intensity; per component TWO tables of 256 entries, the first with
// +scale, the second with -scale, so that a block's random sign is applied by choosing the table
// instead of multiplying every sample).  A component's pair of tables starts at a multiple of
// 2048 bytes below 64 KiB: the LDS address of a sample's entry is (4 * intensity) | base | sign << 10,
// two samples per v_and_or_b32.  Entry:
//   bits 31:24 byte selector for v_perm_b32: slot 0..7, or 0x0c (constant zero) for slot 8
//              (the reference's never-written 9th slot, vfgs_hw.c:49); unused in the one-pattern form
//   bits 23:0  signed scale factor (+-sLUT), pre-shifted: scale << (16 - scale_shift); the stored shift is 8..13 at 8 bit, 6..11 at 10 bit,
//              4..9 at 12 bit (shift + 6 - bs), so an entry reaches 255 << 12 < 2^23 (ranges: vfgs_kernel.hip grain_unit "scale, add, clip")
struct ImageLayout {
	int lut_bytes;              // one component: +scale table, -scale table
	int y_rs, c_rs;             // bank row strides, bytes
	int y_bank, c_bank;         // offsets of the banks inside their sub-images (= LDS offsets)
	int y_neg, c_neg;           // one-pattern form: bytes from a bank to its negated copy (0 in the general form)
	int y_bytes, c_bytes;       // sizes of the sub-images (chroma: of ONE chroma sub-image)
	int y_off, c_off[2];        // offsets of the sub-images of Y, Cb, Cr in the device image
	int c_lut[2];               // LDS offset of Cb's / Cr's LUT pair inside its sub-image
	int bytes;                  // whole device image
	int lds_bytes;              // LDS a workgroup needs
	int cw, ch;                 // chroma bank columns actually addressable, rows
};

constexpr ImageLayout image_layout(int csubx, int csuby, bool one_y, bool one_c, bool depth8)
{
	ImageLayout L{};
	L.lut_bytes = 2 * 256 * 4;
	L.cw = 64 / csubx;
	L.ch = 64 / csuby;
	depth8 = depth8 && kPk16;
	const int ob = depth8 ? 2 : 1;     // bytes per sample of a one-pattern bank (8 bit: the packed 16-bit form)
	L.y_rs = one_y ? 64 * ob + 16 : 64 * kSlots + 16;
	L.c_rs = one_c ? L.cw * ob + 16 : L.cw * kSlots + 16;
	// (the one-pattern form never reads the -scale table: its sign is a choice of bank; only the +scale half is stored -- at 8 bit
	// as the 256 scale bytes)
	L.y_bank = one_y ? (depth8 ? 256 : L.lut_bytes / 2) : L.lut_bytes;
	L.c_bank = one_c ? (depth8 ? 256 : L.lut_bytes / 2) : L.lut_bytes;
	L.y_neg = one_y ? 64 * L.y_rs : 0;
	L.c_neg = one_c ? L.ch * L.c_rs : 0;
	L.y_bytes = L.y_bank + 64 * L.y_rs + L.y_neg;
	L.c_bytes = L.c_bank + L.ch * L.c_rs + L.c_neg;
	L.y_off = 0;
	L.c_off[0] = L.y_bytes;
	L.c_off[1] = L.y_bytes + L.c_bytes;
	L.c_lut[0] = 0;
	L.c_lut[1] = 0;
	L.bytes = L.y_bytes + 2 * L.c_bytes;
	L.lds_bytes = L.y_bytes > L.c_bytes ? L.y_bytes : L.c_bytes;
	return L;
}

// Geometry of one plane type (0 = luma, 1 = the two chroma planes) for one launch.
//
// A row of the plane is cut into 16-byte "units" (one per lane and access), 64 consecutive units are a "position" (one wave
// access, 1 KiB); the lanes compute bytes shifted left against the units so that block edges lie inside lanes / lane pairs
// (vfgs_kernel.hip "Lanes"), which is why a row has one position more than its units fill.  One workgroup = kWavesPerWG waves
// x rw_rpw rows each (wave w: rows w, w + kWavesPerWG, ... of the workgroup's part of ONE block row), rw_splits workgroups per
// block row.
struct PlaneDesc {
	uint32_t pitch, dpitch;       // row pitch of source / destination, bytes
	uint64_t fpitch, dfpitch;     // bytes from frame f to frame f+1
	uint32_t rowbytes, drowbytes; // bytes of a row the reference touches (whole blocks)
	int nrows;                    // rows of the stripe
	int wgs;                      // workgroups per frame for ONE plane of this type
	int rw_segs;                  // positions per row
	int rw_rpw, rw_splits, rw_lsplits;
};

// Frames of a batch that do NOT lie at a constant pitch (a decoder's pool of separately allocated frames, vfgs_hip_add_grain_frame_list_*):
// their plane pointers travel in the kernel arguments themselves -- no device table to upload and keep alive, no copy on the
// stream in front of the launch -- and a workgroup fetches its frame's pointers with one scalar load.  kListFrames frames per
// launch (longer lists: several launches); (2 x 3 + 1) x 8 x kListFrames bytes of the 4 KB argument segment.
constexpr int kListFrames = 32;
struct FrameTable {
	const uint8_t* src[3][kListFrames];   // [component][frame of the launch]: first line of the stripe
	uint8_t* dst[3][kListFrames];
	// A model per frame (KernelArgs::models_kernel, vfgs_hip_add_grain_frame_list_models_dev): the device image of frame f's model, a
	// ModelRecord followed by the table image (image_layout).  Behind the plane pointers: the kernels of before never look this far, and
	// the table is the LAST kernel argument, so nothing they load has moved.
	const uint8_t* model[kListFrames];
};

// What a captured model (vfgs_hip_model_capture) keeps in front of its table image: the values that are one per launch in KernelArgs
// for every other call -- lo2 / hi2 per plane type and pk_shift, exactly as KernelArgs holds them.  A workgroup of grain_ml_kernel reads
// its frame's record with scalar loads before it issues the loads of the image.  32 bytes: the image behind it stays 16-byte aligned.
//
// A model may carry a luma / chroma mix of its own (vfgs_hip_models_from_afgs1_mix, vfgs_hip_model_capture_mix): mix_flags bit 0, and per
// chroma component one word with the four values of KernelArgs::mix in its units (model_mix_word).  All three words zero = a model without
// a mix, which is what every other way to a model writes: the record of before, byte for byte.  The kernels of the mix read the words where
// a launch names a model per frame (KernelArgs::models_kernel with mix_kernel); no other kernel looks at them.
struct ModelRecord {
	uint32_t lo2[2], hi2[2];
	int32_t pk_shift;
	uint32_t mix_flags;           // bit 0: the model carries a mix
	uint32_t mix[2];              // Cb, Cr: model_mix_word
};
constexpr int kModelRecordBytes = 32;
static_assert(sizeof(ModelRecord) == kModelRecordBytes, "the table image begins 32 bytes behind the record");

// One component's mix in a record: bits 7:0 luma_mult, 15:8 chroma_mult (both -128..127), 27:16 offset << (depth - 8) (-256..255 at 8 bit, four
// times that at 10: twelve signed bits), bit 31 active.  Each field comes out with one scalar bit-field extract.
constexpr uint32_t model_mix_word(const int luma_mult, const int chroma_mult, const int offset_scaled, const int active)
{
	return ((uint32_t)luma_mult & 0xffu) | (((uint32_t)chroma_mult & 0xffu) << 8) | (((uint32_t)offset_scaled & 0xfffu) << 16) | (active ? 0x80000000u : 0u);
}
constexpr int model_mix_luma_mult(const uint32_t w) { return (int)(w << 24) >> 24; }
constexpr int model_mix_chroma_mult(const uint32_t w) { return (int)(w << 16) >> 24; }
constexpr int model_mix_offset(const uint32_t w) { return (int)(w << 4) >> 20; }
constexpr int model_mix_active(const uint32_t w) { return (int)(w >> 31); }

// One launch = nframes x (luma workgroups + 2 x chroma workgroups); workgroups are numbered in memory
// order (frame, plane, block row group, split, column group) and are NOT persistent: the hardware
// dispatcher hands them out as CUs free up.
struct KernelArgs {
	const uint8_t* src[3];    // source planes: first line of the stripe, frame 0 (device)
	uint8_t* dst[3];          // destination planes, same geometry (== source: in place)
	PlaneDesc pd[2];
	const uint32_t* stream;   // LFSR bit stream cache (device), bit m = word[m>>5] >> (m&31)
	uint32_t stream_bytes;
	// 1: grain_ml_kernel -- with sp_kernel == 1: grain_spml_kernel -- serves the launch (listed frames; FrameTable::model[f] is frame f's model image and `tables` below frame 0's table
	// image).  The field sits HERE, in the four bytes that used to be padding in front of the pointer below: the frame table is the kernel
	// argument BEHIND this structure, so a field appended at the end would move every plane pointer the kernels of before load (the
	// static_assert below the structure holds its size).
	// With mix_kernel == 1 as well: the kernels of the mix serve listed frames whose models carry a mix (ModelRecord::mix_flags) -- image, bounds,
	// shift AND the mix are the frame's model's, `mix` below is not read.
	// With a key of family rw or sp8 that has out8 (neither wide nor persist): the narrowed kernels serve listed frames with a model each the same way
	// (vfgs_hip_add_grain_frame_list_models_copy8_dev, vfgs_hip_add_grain_sp_frame_list_models_copy8_dev).
	// With sp_kernel == 2: the kernels of p2sp / p2sp8 serve listed planar frames with a model each onto surfaces the same way
	// (vfgs_hip_add_grain_frame_list_models_to_sp_dev / _to_sp8_dev).
	int models_kernel;
	const uint8_t* tables;    // device image (image_layout)
	uint32_t cur_bit0;        // stream bit of the register of block 0, first block row of the stripe, frame 0
	uint32_t up_bit0;         // same for the "upper" register of that first block row
	uint32_t frame_bit_step;  // stream bits between consecutive frames of a batch
	int y0;                   // absolute luma line of the first line of the stripe (multiple of 16 unless the stripe is one block row)
	int nblk;                 // 16-sample blocks per line = ceil(width/16), vfgs_hw.c:301
	int nbrows;               // block rows the stripe touches
	int nframes;
	int listed;               // 1: the planes of frame f are FrameTable::src / dst [.][f] (src / dst above and the frame pitches are unused)
	int lfronts;              // log2 of the frames of a batch that are swept at the same time (their workgroups are dealt out in turn)
	int persist_wgs;          // PERSIST kernels: P luma workgroups share the launch's nframes x pd[0].wgs luma tasks (task t -> workgroup t % P) ...
	int persist_step_f, persist_step_r;   // ... and P = persist_step_f * pd[0].wgs + persist_step_r: what a workgroup advances by
	int pk_shift;             // 8-bit one-pattern forms (packed 16-bit form, above): the scale shift of vfgs_hw.c:263, 8..13 (other depths: unused)
	uint32_t lo2[2], hi2[2];  // clip bounds in sample units (I_min<<bs ...) in both halves of a dword, per plane type (vfgs_hw.c:264-267)
	// Luma / chroma mix of the chroma look-up index (vfgs_hip_set_chroma_mix; all zero = the kernels and the launch of always)
	int mix_kernel;           // 1: grain_mix_kernel serves the launch (all-one-pattern images only)
	int mix_planes;           // ... bit 0: its luma workgroups do nothing, bit 1: its chroma workgroups do nothing (the two launches of an in-place call)
	int mix_lw;               // ... luma width of the call in samples (the last luma sample of a row pairs with itself)
	int mix[2][4];            // ... Cb, Cr: { luma_mult, chroma_mult, offset << (depth - 8), active }
	// Semi-planar frames (vfgs_hip_add_grain_sp_frame_list_dev; all zero = the planar kernels of always)
	int sp_kernel;            // 1: grain_sp_kernel serves the launch: components 1 and 2 are ONE plane of interleaved Cb/Cr pairs, pd[1] describes its row
	                          // 2: grain_p2sp_kernel (out8: grain_p2sp8_kernel): the SOURCE is planar -- src[1] / src[2] are two planes, pd[1].pitch / rowbytes ONE
	                          //    component's row -- the destination is such a UV plane: dst[1] == dst[2], pd[1].dpitch its row pitch and pd[1].drowbytes ONE
	                          //    component's bytes of its row (the row holds twice as many); pd[0].dpitch / drowbytes: the destination's luma row
	                          // 3: grain_sp_kernel (with models_kernel: grain_spml_kernel) again, the source as for 1 -- the DESTINATION is planar: dst[1] / dst[2]
	                          //    are the Cb and the Cr plane of low-aligned samples, pd[1].dpitch / drowbytes ONE component's destination row, pd[0].dpitch /
	                          //    drowbytes the destination's luma row (vfgs_hip_add_grain_sp_frame_list_to_planar_dev); the kernels decide at run time
	uint32_t sp_shift2;       // ... 16-bit containers: the samples sit this many bits up (P010: 6, P012: 4), in both halves of the dword (a packed 16-bit shift each way)
	// The phase between the two frame fronts (front_phase / front_task below; both zero = the fronts in step, every kernel but grain_rw_kernel)
	int front_shift;          // tasks by which the odd front of a pair of frames is rotated: it runs task (r + front_shift) mod per-frame tasks where the even front runs task r
	int front_plain_from;     // ... the first group of frames (blockIdx.y) that is NOT rotated
};
static_assert(sizeof(KernelArgs) == 312, "the frame table follows KernelArgs in the kernel arguments: a new size moves what every kernel loads from it");

// WHICH task a workgroup of a launch's grid (vfgs_kernel.hip grid_of) runs: frame f, task r of the frame's per_frame tasks (luma, Cb, Cr in
// the order of memory).  x = (task, front of a group of 2^lfronts frames), y = group of frames; f may lie behind the launch's last frame
// (an odd number of frames: the kernel returns).  The ODD front of a group in front of front_plain_from runs its tasks rotated by front_shift:
// a bijection of the frame's tasks, so every (f, r) is still dealt out exactly once, and no kernel relies on the order of workgroups.
// (constexpr: host and device code call it alike, like every function of this header)
struct FrontTask { int f, r; };
constexpr FrontTask front_task(const unsigned bx, const unsigned by, const int lfronts, const int per_frame, const int front_shift, const int front_plain_from)
{
	const unsigned front = bx & ((1u << lfronts) - 1);
	FrontTask t{(int)(by << lfronts) + (int)front, (int)(bx >> lfronts)};
	if (VFGS_FRONT_PHASE != 0 && front_shift != 0 && (front & 1) && (int)by < front_plain_from)
	{
		t.r += front_shift;
		if (t.r >= per_frame) t.r -= per_frame;
	}
	return t;
}

// The host's rule for the two fields (vfgs_host.cpp Launch::plan_grid).  Two fronts of the planar row walk: the odd front starts at the first
// chroma task (Cb, Cr, Y) in every group but the launch's last, which keeps the order of memory -- the launch then drains on short chroma
// workgroups, not on luma workgroups that take several times as long.  A launch of one group is the launch of always.
struct FrontPhase { int shift, plain_from; };
constexpr FrontPhase front_phase(const int lfronts, const bool rw_family, const int wgs_y, const int wgs_c, const int nframes)
{
	if (VFGS_FRONT_PHASE == 0 || lfronts != 1 || !rw_family || wgs_y <= 0 || wgs_c <= 0) return FrontPhase{0, 0};
	const int groups = (nframes + 1) >> 1;
	const int plain_from = VFGS_FRONT_PHASE == 2 ? groups : groups - 1;
	return plain_from > 0 ? FrontPhase{wgs_y, plain_from} : FrontPhase{0, 0};
}

// WHICH kernel serves a launch: the kernel family and its template arguments.  The host forms one key per call (vfgs_host.cpp Launch::key), the
// launcher instantiates and dispatches from kernel_exists() (vfgs_kernel.hip launch_key), the launch record names the kernel and its LDS with
// kernel_name() / kernel_lds_bytes(), and tests/test_kernel_keys_cpu.py holds all three against the kernels in the built code objects.
enum class Family {
	rw,        // grain_rw_kernel    <depth, csubx, csuby, out8, oney, onec, wide, persist>: planar frames
	ml,        // grain_ml_kernel    <depth, csubx, csuby, oney, onec>: ... with a model per frame
	mix,       // grain_mix_kernel   <depth, csubx, csuby, out8, wide>: ... under the luma / chroma mix
	sp,        // grain_sp_kernel    <depth, csuby, oney, onec>: semi-planar frames
	spml,      // grain_spml_kernel  <depth, csuby, oney, onec>: ... with a model per frame
	sp8,       // grain_sp8_kernel   <depth, csuby, oney, onec>: ... with the narrowed 8-bit destination
	p2sp,      // grain_p2sp_kernel  <depth, csuby, oney, onec>: a planar source, a semi-planar destination
	p2sp8,     // grain_p2sp8_kernel <depth, csuby, oney, onec>: ... narrowed
	sp_mix,    // grain_sp_mix_kernel<depth, csuby>: semi-planar frames under the mix
};

struct KernelKey {
	int depth, csubx, csuby;
	// out8: the destination holds 8-bit samples of a 10- or 12-bit path; oney / onec: the image holds the one-pattern form for luma / chroma;
	// wide: rows of more than kTileBlocks blocks; persist: KernelArgs::persist_wgs luma workgroups share the launch's luma tasks
	bool out8, oney, onec, wide, persist;
	Family family;
};

constexpr bool family_semiplanar(const Family f) { return f != Family::rw && f != Family::ml && f != Family::mix; }     // (the destination is; p2sp: not the source)

// The family as KernelArgs states it (no kernel reads these three fields; the launcher refuses a key that disagrees with them).  out8 is the
// key's: it tells sp8 from sp and p2sp8 from p2sp.
// with_models: a launch of the two families of the mix that names a model per frame (models that carry a mix; the key has neither out8 nor wide) --
// the same kernels, which decide at run time where the image, the bounds and the mix come from -- or of rw / sp8 with the narrowed destination
// (the key has out8, neither wide nor persist; the launcher holds it to that): the OUT8 kernels decide the same way -- or of p2sp / p2sp8 (a planar
// source onto a surface with a model per frame: every kernel of the two families decides the same way).  Every other family has one answer.
// to_planar: a launch of sp / spml whose destination is a planar picture (sp_kernel 3; the same kernels decide at run time).  No other family has such a form.
struct FamilyFields { int models_kernel, mix_kernel, sp_kernel; };
constexpr FamilyFields family_fields(const Family f, const bool with_models = false, const bool to_planar = false)
{
	const bool mixf = f == Family::mix || f == Family::sp_mix;
	const bool run_time = mixf || f == Family::rw || f == Family::sp8 || f == Family::p2sp || f == Family::p2sp8;     // the families whose kernels serve programmed launches and models alike
	return FamilyFields{f == Family::ml || f == Family::spml || (run_time && with_models), mixf,
	                    !family_semiplanar(f) ? 0 : ((f == Family::p2sp || f == Family::p2sp8) ? 2 : ((to_planar && (f == Family::sp || f == Family::spml)) ? 3 : 1))};
}

// THE TABLE OF INSTANTIATIONS.  A family pins every parameter it does not take, so one kernel has exactly one key.
constexpr bool kernel_exists(const KernelKey& k)
{
	if ((k.depth != 8 && k.depth != 10 && k.depth != 12) || (k.csubx != 1 && k.csubx != 2) || (k.csuby != 1 && k.csuby != 2)) return false;
	const bool all_one = k.oney && k.onec, square = k.csubx == k.csuby;      // (square: 4:2:0 and 4:4:4)
	// semi-planar frames: 4:2:0 / 4:2:2, rows of one parameter table, no persistent luma workgroups
	if (family_semiplanar(k.family) && (k.csubx != 2 || k.wide || k.persist)) return false;
	switch (k.family)
	{
	case Family::rw:
		if (k.out8 && k.depth == 8) return false;
		// rows walked in parts: the general form for every format; at 4:2:0 and 4:4:4 also one-pattern chroma under either luma form
		// (the default SEI model: eight luma patterns, one chroma pattern; AFGS1 and the single-pattern SEI models: one each)
		if (k.wide) return !k.persist && (k.oney ? k.onec && square : !k.onec || square);
		// persistence: 10 and 12 bit, general-form luma
		return !k.persist || (k.depth > 8 && !k.oney);
	case Family::ml:
		return !k.out8 && !k.wide && !k.persist;
	case Family::mix:       // all-one-pattern images at 8 and 10 bit; the 8-bit destination at 10 bit; rows walked in parts at 4:2:0 and 4:4:4
		return all_one && !k.persist && k.depth != 12 && (!k.out8 || k.depth == 10) && (!k.wide || square);
	case Family::sp: case Family::spml: case Family::p2sp:
		return !k.out8;
	case Family::sp8: case Family::p2sp8:
		return k.out8 && k.depth > 8;
	case Family::sp_mix:
		return !k.out8 && all_one && k.depth != 12;
	}
	return false;
}

// what that kernel's __shared__ array is sized to
constexpr int kernel_lds_bytes(const KernelKey& k)
{
	const ImageLayout L = image_layout(k.csubx, k.csuby, k.oney, k.onec, k.depth == 8);
	switch (k.family)
	{
	case Family::rw: case Family::ml: return lds_allocation(k.depth > 8, k.oney, k.onec, k.wide, L.lds_bytes + kParamBytes);
	case Family::mix: return mix_lds_allocation(L.lds_bytes + kParamBytes);
	case Family::sp_mix: return sp_mix_lds_allocation(sp_lds_need(L.y_bytes, L.c_bytes, L.lut_bytes, true));
	case Family::sp: case Family::spml: case Family::sp8: case Family::p2sp: case Family::p2sp8:
		return sp_lds_allocation(sp_lds_need(L.y_bytes, L.c_bytes, L.lut_bytes, k.onec));
	}
	return 0;
}

// the kernel's name as the profiler prints it (vfgs_hip_last_launch_info): the template arguments its family takes, in the order of the table above
// (not constexpr: it formats with snprintf)
inline int kernel_name(const KernelKey& k, char* out, const size_t n)
{
	auto b = [](bool v) { return v ? "true" : "false"; };
	auto sp = [&](const char* name) { return snprintf(out, n, "%s<%d,%d,%s,%s>", name, k.depth, k.csuby, b(k.oney), b(k.onec)); };
	switch (k.family)
	{
	case Family::rw: return snprintf(out, n, "grain_rw_kernel<%d,%d,%d,%s,%s,%s,%s,%s>", k.depth, k.csubx, k.csuby, b(k.out8), b(k.oney), b(k.onec), b(k.wide), b(k.persist));
	case Family::ml: return snprintf(out, n, "grain_ml_kernel<%d,%d,%d,%s,%s>", k.depth, k.csubx, k.csuby, b(k.oney), b(k.onec));
	case Family::mix: return snprintf(out, n, "grain_mix_kernel<%d,%d,%d,%s,%s>", k.depth, k.csubx, k.csuby, b(k.out8), b(k.wide));
	case Family::sp_mix: return snprintf(out, n, "grain_sp_mix_kernel<%d,%d>", k.depth, k.csuby);
	case Family::sp: return sp("grain_sp_kernel");
	case Family::spml: return sp("grain_spml_kernel");
	case Family::sp8: return sp("grain_sp8_kernel");
	case Family::p2sp: return sp("grain_p2sp_kernel");
	case Family::p2sp8: return sp("grain_p2sp8_kernel");
	}
	return snprintf(out, n, "?");
}

}  // namespace vfgs
