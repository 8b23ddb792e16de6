// gfx950 (MI355X, CDNA4) film grain kernels.  Written for wave64 / LDS / HBM3E directly;
// there is no other target.
//
// What is computed is the closed form of the reference hardware layer
// (/root/reference/src/vfgs_hw.c:140-312; derivation in DESIGN.md):
//
//   out = clip( in + round( scale[in>>bs] * F( s * pat[slot[in>>bs]][oy+r][ox+i] (+ overlap) ), shift ) )
//
// where (s, ox, oy) come from a 32-bit window of the LFSR bit stream at bit
// (block_row * blocks_per_line + block), F is the 3-tap filter at block edges, and the
// window of the block row above feeds the 2-line overlap.
//
// Work decomposition ("row walk"; one kernel family since round 4):
//   * every lane moves 16 bytes per access (8 samples at 10 and 12 bit, 16 samples at 8 bit), one wave access = one line-aligned
//     1 KiB "position" of a row;
//   * the lanes COMPUTE bytes shifted left of the block grid by half a block, so every block edge -- the only place where a
//     sample depends on its horizontal neighbours -- lies inside a lane or between the two lanes of a pair: no halo, no
//     inter-wave exchange, in place is race free; the shift between what a lane moves and what it computes is a rotation by
//     one lane in registers (DPP);
//   * a WAVEFRONT owns whole rows and streams them through a ring of four register sets; a WORKGROUP of 4 waves covers a few
//     consecutive rows of ONE block row, is NOT persistent, copies only its plane's banks + LUTs to LDS and computes the block
//     parameters of its block row (LFSR window -> sign, pattern offsets) once, into LDS; workgroups are numbered in memory
//     order, so the chip sweeps the frames front to back and the hardware dispatcher balances the load;
//   * a component whose pattern LUT selects one slot for every intensity is served from a packed one-byte-per-sample bank
//     (ONEY / ONEC kernels, vfgs_layout.h);
//   * rows of more than 512 grain blocks (8192 luma samples) are walked in parts of 512 blocks, the parameter table refilled
//     between the parts; the 8-bit output of a 10- or 12-bit path (yuv.c:216-258) is a narrowing in the store (OUT8 kernels);
//   * the frames of a launch lie at a constant pitch behind the plane pointers of the arguments, or anywhere: then their plane
//     pointers are a table IN the kernel arguments (FrameTable, vfgs_layout.h) and a workgroup reads its frame's with scalar loads;
//   * semi-planar frames (a luma plane + ONE plane of interleaved Cb/Cr pairs, samples possibly in the high bits of their containers) have a
//     kernel family of their own, grain_sp_kernel: the luma walk with a container shift, and a UV walk whose lanes move 32 bytes and split
//     them into one planar Cb unit and one planar Cr unit ("UV walk" below); with the narrowed 8-bit destination (P010 in, NV12 out): grain_sp8_kernel,
//     the same two walks with OUT8 -- a UV lane stores ONE 16-byte unit of Cb/Cr byte pairs;
//   * a PLANAR source with a semi-planar destination (software-decoded pictures onto a display surface): grain_p2sp_kernel / grain_p2sp8_kernel, the same
//     two walks again -- a UV lane loads one 16-byte unit from the Cb row and one from the Cr row instead of splitting 32 bytes of an interleaved row;
//   * a MODEL PER FRAME (captured table images, FrameTable::model[]): grain_ml_kernel for planar frames, grain_spml_kernel for semi-planar ones -- the
//     walks above with the tables, the clip bounds and the packed form's shift taken from the workgroup's frame instead of the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "vfgs_layout.h"

namespace vfgs {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------
// small device helpers
//
// Issue rates measured on MI355X (tools/valu_rate.hip): plain VOP2 integer ops (add, and,
// shifts) and f32 FMA take ~2.4 cycles per wave-instruction; integer VOP3-only, packed-16, SDWA
// and DPP forms (v_perm_b32, v_mad_*, v_pk_*, v_bfe_*, v_add3, v_and_or) take ~4.4.

// One sample's pattern value out of its 8-byte slot group {hi,lo}: the LUT entry's top byte is
// the v_perm_b32 selector (slot 0..7, or 0x0c = constant 0) for result byte 3; the arithmetic
// shift then sign-extends it (the other three result bytes are don't-care).
__device__ __forceinline__ int pick_slot(uint32_t hi, uint32_t lo, uint32_t lut_entry)
{
	return (int)__builtin_amdgcn_perm(hi, lo, lut_entry) >> 24;
}

// x * y.i24 + c: the LUT entry's low 24 bits are the signed scale, pre-shifted so that the product's
// HIGH half is the scaled grain (see grain_unit); the selector byte above them is ignored by the i24 multiply
__device__ __forceinline__ int mad_i24(int x, uint32_t y, int c)
{
	int r;
	asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "s"(c));
	return r;
}

// x * y + c on 24-bit operands, all in VGPRs (or inline constants): the compiler would otherwise pick
// 32-bit multiplies for these
__device__ __forceinline__ int mad_vvv(int x, int y, int c)
{
	int r;
	asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(c));
	return r;
}

// sext(byte B of d) * y.i24: the one-pattern bank holds four pattern bytes per dword; SDWA selects and sign-extends one of them inside
// the multiply (VOP2), which saves the separate extraction where the value itself is not needed (everywhere but at block edges)
__device__ __forceinline__ int mul_byte_i24(const int b, uint32_t d, uint32_t y)       // (b is a constant after unrolling: one case survives)
{
	int r;
	switch (b)
	{
	case 0: asm("v_mul_i32_i24_sdwa %0, sext(%1), %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(r) : "v"(d), "v"(y)); break;
	case 1: asm("v_mul_i32_i24_sdwa %0, sext(%1), %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(r) : "v"(d), "v"(y)); break;
	case 2: asm("v_mul_i32_i24_sdwa %0, sext(%1), %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(r) : "v"(d), "v"(y)); break;
	default: asm("v_mul_i32_i24_sdwa %0, sext(%1), %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(r) : "v"(d), "v"(y)); break;
	}
	return r;
}

// ---- packed 16-bit helpers (8-bit one-pattern form, vfgs_layout.h "packed 16-bit form") ----
// two samples per instruction: {a.lo * b.lo + c.lo, a.hi * b.hi + c.hi} in 16 bits (the host has proven that nothing overflows)
__device__ __forceinline__ uint32_t pk_mad_i16(uint32_t a, uint32_t b, uint32_t c)
{
	uint32_t r;
	asm("v_pk_mad_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
	return r;
}
// both halves shifted right arithmetically by the corresponding half of `sh`
__device__ __forceinline__ uint32_t pk_ashr_i16(uint32_t sh, uint32_t v)
{
	uint32_t r;
	asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(r) : "s"(sh), "v"(v));
	return r;
}
// x.i16 * (HI ? y.hi : y.lo).i16 + c in 32 bits: a block edge's filtered value times its sample's scale, which sits in one half
// of the pair's register
template <bool HI>
__device__ __forceinline__ int mad_i32_i16(int x, uint32_t y, int c)
{
	int r;
	if (HI) asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[0,1,0,0]" : "=v"(r) : "v"(x), "v"(y), "s"(c));
	else asm("v_mad_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "s"(c));
	return r;
}
__device__ __forceinline__ int dot2_i16(uint32_t a, uint32_t b, int c)
{
	return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}
// both 16-bit halves shifted by the corresponding half of `sh` (semi-planar frames: samples in the high bits of their containers)
__device__ __forceinline__ uint32_t pk_lshr_b16(uint32_t sh, uint32_t v)
{
	uint32_t r;
	asm("v_pk_lshrrev_b16 %0, %1, %2" : "=v"(r) : "s"(sh), "v"(v));
	return r;
}
__device__ __forceinline__ uint32_t pk_lshl_b16(uint32_t sh, uint32_t v)
{
	uint32_t r;
	asm("v_pk_lshlrev_b16 %0, %1, %2" : "=v"(r) : "s"(sh), "v"(v));
	return r;
}
__device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b)      // mask ? a : b, bit by bit
{
	uint32_t r;
	asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "v"(a), "v"(b));
	return r;
}

__device__ __forceinline__ int swap_lane_pairs(int v)
{
	// quad_perm:[1,0,3,2]: lane 2m <-> lane 2m+1
	return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);
}

// Global memory goes through raw buffer instructions: the row base is a wave-uniform scalar
// offset, the lane supplies the byte offset inside the row, and a lane that must not touch
// memory supplies kOOB, which the hardware range check (offset >= num_records) turns into
// "load returns 0 / store is dropped".  No exec-mask branches around loads and stores, and a
// whole access can be switched off by a descriptor with zero records (wave-uniform).
constexpr uint32_t kOOB = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const uint8_t* base, uint32_t bytes)
{
	return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
}

// ---------------------------------------------------------------------------------------
// Lanes.
//
// A lane holds 16 bytes of one row = NS samples (8 at 10 bit, 16 at 8 bit) as 4 dwords; lane
// position p of a row covers samples [NS*p - SHIFT, NS*p - SHIFT + NS).  The lane's samples fall
// into NR "runs" that belong to consecutive grain blocks, and into NQ = NS/4 "quads" of 4 samples
// (a quad never straddles a block; its pattern data is two ds_read_b128):
//
//   PAIR  (NS 8, BW 16): the lane is half a block: p - 1 = unit index, block = (p - 1) >> 1; odd p =
//                        first half.  The block edge lies between lanes 2m (last sample in slot 7)
//                        and 2m + 1 (first sample in slot 0): one DPP quad_perm swap.
//   NS 8,  BW 8        : runs = second half of block p-1 | first half of block p; edge between samples 3|4
//   NS 16, BW 16       : the same with 8-sample halves; edge between samples 7|8
//   NS 16, BW 8        : runs = last 4 of block 2p-1 | block 2p | first 4 of block 2p+1; edges 3|4 and 11|12
template <int NS, int BW>
struct LaneMap {
	static constexpr bool PAIR = (NS == 8 && BW == 16);
	static constexpr int SHIFT = PAIR ? 8 : BW / 2;                 // samples
	static constexpr int NR = PAIR ? 1 : NS / BW + 1;
	static constexpr int NQ = NS / 4;
	static constexpr int NE = NR - 1;                               // block edges inside the lane
	static constexpr int BPL = PAIR ? 1 : NS / BW;                  // whole blocks a lane advances by
	__device__ static constexpr int run(int q) { return PAIR ? 0 : (4 * q + BW - SHIFT) / BW; }
	__device__ static constexpr int col(int q) { return PAIR ? 4 * q : (4 * q + BW - SHIFT) % BW; }   // column of the quad's first sample in its block
	__device__ static constexpr int edge_quad(int e) { return PAIR ? 0 : ((e + 1) * BW - (BW - SHIFT)) / 4 - 1; }   // quad left of inner edge e
};

// A block's parameters in ONE dword per run (computed once per workgroup and task into the LDS parameter table; a lane reads
// the 1-3 entries of its runs per position and rebuilds k2, the rounding constants and the relative signs of the edge filter
// from them with a handful of instructions):
//   bits 15:0  LDS byte address of bank[.][oy][ox (+ the lane's column for PAIR)][slot 0], row 0 of the block row; one-pattern
//              form, current row of blocks: of the NEGATED bank if the block's sign is negative (grain_unit)
//   bit  31    the block's sign is negative
template <int NR>
struct RunParam {
	uint32_t pa[NR];
};

// vfgs_hw.c:99-138 with the component as wave-uniform data: the x field is 10 bits at `sx`, the
// y field the low 10 bits of the register rotated right by `sy` (component 1 takes bits 31:24
// and 1:0 -- exactly a rotation by 24), the sign bit at `sb`.  Returns the LDS address; sign in *neg.
template <int SUBX, int SUBY, int RS, int SB>
__device__ __forceinline__ uint32_t block_param(uint32_t v, uint32_t bank_off, int sx, int sy, int sb, bool* neg)
{
	const uint32_t fx = (v >> sx) & 0x3ff;
	const uint32_t fy = __builtin_amdgcn_alignbit(v, v, sy) & 0x3ff;
	const uint32_t ox = (__umul24(fx, 13u) >> 10) * (4 / SUBX);
	const uint32_t oy = (__umul24(fy, 12u) >> 10) * (4 / SUBY);
	*neg = (v >> sb) & 1;
	return __umul24(oy, (uint32_t)RS) + ox * SB + bank_off;     // SB = bytes per sample position: 1 (8-bit one-pattern form: 2) or one per slot
}

// ---------------------------------------------------------------------------------------
// The per-lane grain pipeline for the NS samples of one row.
//
//   w          in/out: samples, 4 dwords (10 bit: 2 x uint16 each; 8 bit: 4 x uint8 each)
//   rp         block parameters of the lane's runs; rowoff = (row inside the block row) * RS
//
// Two forms of the same arithmetic (vfgs_hw.c:211-229, 250-267):
//
// OVERLAP = true (the two lines under a block-row boundary): pattern values are blended as
//   P = (Pcur * m + Pup * n + 16) >> 5 with m = sign_cur * w_cur, n = sign_up * w_up, so P is
//   the signed grain; the +scale tables are used; rel = 1, c = 2.
//
// OVERLAP = false: the block sign s is folded into the scale instead of the pattern value:
//   k2 points at the table of sign * scale, P~ = s * P is used unsigned-by-sign, and
//   round(scale * P, shift) == (s*scale) * P~ ... exactly (s*s == 1).  The 3-tap edge filter
//   F = (l1 + 3 l0 + r0 + 2) >> 2 on true values becomes, in the P~ domain of the lane whose
//   sample is filtered,  F~ = (a~ + 3 b~ + rel * c~ + (s > 0 ? 2 : 1)) >> 2  with rel = s * s'
//   the relative sign of the two blocks: for s = -1, -((-A + 2) >> 2) == (A + 1) >> 2.
//
// MIX (chroma planes of grain_mix_kernel): the look-up index of a sample is not the sample but the luma / chroma mix `ix`, same layout
// as `w` (mix_index below); only the LUT gathers read it.
template <int DEPTH, int BW, bool OVERLAP, bool ONE, bool ALIGN2, int NEG, bool MIX = false>
__device__ __forceinline__ void grain_unit(const uint8_t* lds, uint32_t (&w)[4],
                                            const RunParam<LaneMap<DEPTH == 8 ? 16 : 8, BW>::NR>& rp,
                                            const RunParam<LaneMap<DEPTH == 8 ? 16 : 8, BW>::NR>& up,
                                            const uint32_t lutb, const uint32_t rowoff, const uint32_t uprowoff, const int wcur, const int wup,
                                            const bool (&edge_on)[LaneMap<DEPTH == 8 ? 16 : 8, BW>::PAIR ? 1 : LaneMap<DEPTH == 8 ? 16 : 8, BW>::NE],
                                            const bool first, const uint32_t lo2, const uint32_t hi2, const int pkshift, const uint32_t (&ix)[4])
{
	constexpr int NS = DEPTH == 8 ? 16 : 8;
	using M = LaneMap<NS, BW>;
	constexpr int NR = M::NR, NQ = M::NQ;
	auto index_dword = [&](int d) { return MIX ? ix[d] : w[d]; };
	// 8-bit one-pattern form: int16 bank + table of scale bytes (vfgs_layout.h "packed 16-bit form"); pkshift = the scale shift
	constexpr bool PK = DEPTH == 8 && ONE && kPk16;
	static_assert(!(PK && M::PAIR), "lane pairs are 10-bit lanes");
	// unpack the block parameters
	int sg[NR];              // 0 / -1: the block's sign is negative
	uint32_t ad[NR], k2s[NR];
#pragma unroll
	for (int r = 0; r < NR; r++)
	{
		sg[r] = (int)rp.pa[r] >> 31;
		// one-pattern form: the address of a negative block (of the CURRENT row of blocks; `up` is only used on overlap lines)
		// points into the negated bank (vfgs_layout.h); the overlap lines blend true values by signed weights: back to the bank
		ad[r] = (rp.pa[r] & 0xffffu) + rowoff - ((ONE && OVERLAP) ? ((uint32_t)sg[r] & (uint32_t)NEG) : 0u);
		k2s[r] = ONE ? 0u : (OVERLAP ? lutb : (((uint32_t)sg[r] & 0x04000400u) | lutb));     // OVERLAP: the +scale table
	}
	if constexpr (PK && !OVERLAP)
	{
		// ---- two samples per instruction (every line but the two overlap lines of a block row) ----
		const uint32_t rnd = 1u << (pkshift - 1);
		const uint32_t rpk = rnd * 0x10001u, shpk = (uint32_t)pkshift * 0x10001u;
		const uint8_t* lut = lds + (lutb & 0xffffu);
		uint32_t S[NS / 2], Pp[NS / 2], G[NS / 2];
		// scale gather (vfgs_hw.c:211,239): the sample IS the address; a pair's scales in the two halves of one register
#pragma unroll
		for (int q = 0; q < NQ; q++)
		{
			const uint32_t v = index_dword(q);
			const uint32_t s0 = lut[v & 0xffu], s1 = lut[(v >> 8) & 0xffu], s2 = lut[(v >> 16) & 0xffu], s3 = lut[v >> 24];
			S[2 * q] = s0 | (s1 << 16);
			S[2 * q + 1] = s2 | (s3 << 16);
		}
		// pattern fetch: four int16 = one 8-byte read (two dwords where the block offsets are multiples of 2 samples, ALIGN2)
#pragma unroll
		for (int q = 0; q < NQ; q++)
		{
			uint32_t a8 = ad[M::run(q)] + M::col(q) * 2;
#ifdef VFGS_PK_NO_READ2      // developer A/B: keep the compiler from pairing two quads' 8-byte reads into one ds_read2_b64 (8 LDS cycles where two ds_read_b64 take 2 each)
			if (!ALIGN2 && (q & 1)) asm volatile("" : "+v"(a8));
#endif
			if (ALIGN2) { Pp[2 * q] = *(const uint32_t*)(lds + a8); Pp[2 * q + 1] = *(const uint32_t*)(lds + a8 + 4); }
			else { const u32x2 t = *(const u32x2*)(lds + a8); Pp[2 * q] = t.x; Pp[2 * q + 1] = t.y; }
		}
		// round(scale * P, shift) (vfgs_hw.c:263) for both samples of a pair
#pragma unroll
		for (int m = 0; m < NS / 2; m++) G[m] = pk_ashr_i16(shpk, pk_mad_i16(Pp[m], S[m], rpk));
		// the two samples at a block edge (vfgs_hw.c:250-259): 3-tap filter on the unfiltered neighbours as dot products of the
		// packed pairs, 32-bit product with the sample's scale (the filtered value may reach +-159), result dropped into its half
#pragma unroll
		for (int ed = 0; ed < M::NE; ed++)
		{
			const int s = 4 * M::edge_quad(ed), pa = s / 2 + 1, pb = s / 2 + 2;      // pairs (l1, l0) | (r0, r1)
			const uint32_t A = Pp[pa], B = Pp[pb];
			const int fl = dot2_i16(B, 0x00000001u, dot2_i16(A, 0x00030001u, 2)) >> 2;     // (l1 + 3 l0 + r0 + 2) >> 2
			const int fr = dot2_i16(A, 0x00010000u, dot2_i16(B, 0x00010003u, 2)) >> 2;     // (l0 + 3 r0 + r1 + 2) >> 2
			const int gl = mad_i32_i16<true>(fl, S[pa], (int)rnd), gr = mad_i32_i16<false>(fr, S[pb], (int)rnd);
			const uint32_t mA = edge_on[ed] ? 0xffff0000u : 0u, mB = mA >> 16;
			G[pa] = bfi(mA, (uint32_t)gl << (16 - pkshift), G[pa]);
			G[pb] = bfi(mB, (uint32_t)(gr >> pkshift), G[pb]);
		}
		// add, clip (vfgs_hw.c:264-267), two samples per instruction
#pragma unroll
		for (int d = 0; d < 4; d++)
		{
			const uint32_t v01 = __builtin_amdgcn_perm(0, w[d], 0x0c010c00), v23 = __builtin_amdgcn_perm(0, w[d], 0x0c030c02);
			s16x2 a = __builtin_bit_cast(s16x2, v01) + __builtin_bit_cast(s16x2, G[2 * d]);
			s16x2 b = __builtin_bit_cast(s16x2, v23) + __builtin_bit_cast(s16x2, G[2 * d + 1]);
			a = __builtin_elementwise_min(__builtin_elementwise_max(a, __builtin_bit_cast(s16x2, lo2)), __builtin_bit_cast(s16x2, hi2));
			b = __builtin_elementwise_min(__builtin_elementwise_max(b, __builtin_bit_cast(s16x2, lo2)), __builtin_bit_cast(s16x2, hi2));
			w[d] = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, a), 0x06040200);
		}
		return;
	}
	uint32_t e[NS];
	int P[NS];
	uint32_t pdw[NQ];        // one-pattern form: the four pattern bytes of quad q as they came out of LDS

	// LUT gather: intensity = sample >> bs, as a uint8 (vfgs_hw.c:157,211); entry address = 4 * intensity | table
#pragma unroll
	for (int q = 0; q < NQ; q++)
	{
		const uint32_t k2 = k2s[M::run(q)];
		if (DEPTH > 8)
		{
#pragma unroll
			for (int h = 0; h < 2; h++)
			{
				// 10 bit: sample & 0x3fc IS 4 * intensity.  12 bit: the intensity sits in bits 11:4 of each half-word, two bits further
				// up: one v_lshrrev_b32 for the pair in front of the same v_and_or_b32 (bits 3:2 of the upper sample land in bits 1:0
				// of the upper half and bits 15:14 of the lower, all outside the mask) -- half a VOP2 instruction per sample more than
				// at 10 bit, and no cheaper pair exists: a v_bfe_u32 per sample still needs its << 2
				uint32_t sv = index_dword(2 * q + h);
				if constexpr (DEPTH == 12)
				{
					// (opaque, so that the pair keeps ONE shift: where k2 is 0 -- the one-pattern form -- the compiler otherwise splits the
					// pair first and shifts each half, four instructions for the two indices instead of three)
					sv >>= 2;
					asm("" : "+v"(sv));
				}
				const uint32_t idx = (sv & 0x03fc03fcu) | k2;
				e[4 * q + 2 * h]     = *(const uint32_t*)(lds + (idx & 0xffffu));
				e[4 * q + 2 * h + 1] = *(const uint32_t*)(lds + (idx >> 16));
			}
		}
		else if (PK)
		{
			// (overlap lines of the packed 16-bit form: the scale byte itself)
			const uint32_t v = index_dword(q);
			const uint8_t* lut = lds + (lutb & 0xffffu);
			e[4 * q + 0] = lut[v & 0xffu];
			e[4 * q + 1] = lut[(v >> 8) & 0xffu];
			e[4 * q + 2] = lut[(v >> 16) & 0xffu];
			e[4 * q + 3] = lut[v >> 24];
		}
		else
		{
			const uint32_t v = index_dword(q), k1 = k2 & 0xffffu;
			e[4 * q + 0] = *(const uint32_t*)(lds + (((v << 2) & 0x3fcu) | k1));
			e[4 * q + 1] = *(const uint32_t*)(lds + (((v >> 6) & 0x3fcu) | k1));
			e[4 * q + 2] = *(const uint32_t*)(lds + (((v >> 14) & 0x3fcu) | k1));
			e[4 * q + 3] = *(const uint32_t*)(lds + (((v >> 22) & 0x3fcu) | k1));
		}
	}

	// pattern fetch.  General form: 4 samples x 8 slots = 32 bytes per quad, the sample's slot picked by v_perm_b32.
	// One-pattern form: 4 samples = one dword (at a 2-byte aligned address where the block offsets are multiples of 2
	// samples, ALIGN2: cut out of two aligned dwords), each value sign-extended out of its byte.
	auto fetch4 = [&](uint32_t adq, int q, int (&out)[4], uint32_t& raw) {
		if (PK)
		{
			const uint32_t a8 = adq + M::col(q) * 2;
			uint32_t p01, p23;
			if (ALIGN2) { p01 = *(const uint32_t*)(lds + a8); p23 = *(const uint32_t*)(lds + a8 + 4); }
			else { const u32x2 t = *(const u32x2*)(lds + a8); p01 = t.x; p23 = t.y; }
			raw = p01;
			out[0] = (int)(p01 << 16) >> 16; out[1] = (int)p01 >> 16;
			out[2] = (int)(p23 << 16) >> 16; out[3] = (int)p23 >> 16;
		}
		else if (ONE)
		{
			uint32_t d;
			if (ALIGN2)
			{
				const uint32_t a4 = adq + M::col(q);
				const uint32_t lo = *(const uint32_t*)(lds + (a4 & ~3u)), hi = *(const uint32_t*)(lds + (a4 & ~3u) + 4);
				d = __builtin_amdgcn_alignbit(hi, lo, (a4 & 2u) * 8);
			}
			else
				d = *(const uint32_t*)(lds + adq + M::col(q));
			raw = d;
#pragma unroll
			for (int i = 0; i < 4; i++) out[i] = (int)(d << (24 - 8 * i)) >> 24;
		}
		else
		{
			const u32x4 c0 = *(const u32x4*)(lds + adq + M::col(q) * kSlots), c1 = *(const u32x4*)(lds + adq + M::col(q) * kSlots + 16);
			out[0] = pick_slot(c0.y, c0.x, e[4 * q + 0]); out[1] = pick_slot(c0.w, c0.z, e[4 * q + 1]);
			out[2] = pick_slot(c1.y, c1.x, e[4 * q + 2]); out[3] = pick_slot(c1.w, c1.z, e[4 * q + 3]);
		}
	};
#pragma unroll
	for (int q = 0; q < NQ; q++)
	{
		int v4[4];
		pdw[q] = 0;
		fetch4(ad[M::run(q)], q, v4, pdw[q]);
#pragma unroll
		for (int i = 0; i < 4; i++) P[4 * q + i] = v4[i];
	}
	if (OVERLAP)
	{
#pragma unroll
		for (int q = 0; q < NQ; q++)
		{
			const int r = M::run(q);
			const uint32_t uad = (up.pa[r] & 0xffffu) + uprowoff;
			int Q[4];
			uint32_t rawq;
			fetch4(uad, q, Q, rawq);
			const int m = (wcur ^ sg[r]) - sg[r];                            // sign_cur * weight_cur
			const int usg = (int)up.pa[r] >> 31;
			const int n = (wup ^ usg) - usg;                                 // sign_up * weight_up
#pragma unroll
			for (int i = 0; i < 4; i++) P[4 * q + i] = mad_vvv(Q[i], n, mad_vvv(P[4 * q + i], m, 16)) >> 5;
		}
	}

	// 3-tap filter across the block edge (vfgs_hw.c:250-259), on unfiltered neighbours
	// (all values are small: explicit 24-bit multiply-adds; the compiler otherwise reaches for 32/64-bit
	// multiplies and turns the selects into a branch that copies all the P registers)
	if (M::PAIR)
	{
		const int mine = first ? P[0] : P[7];
		const int inner = first ? P[1] : P[6];
		const int theirs = swap_lane_pairs(mine);
		int f;
		if (OVERLAP || ONE) f = (theirs + mad_vvv(3, mine, inner + 2)) >> 2;
		else
		{
			const int x = sg[0] ^ swap_lane_pairs(sg[0]);                    // 0: the two blocks have the same sign, -1: opposite
			f = (((theirs ^ x) - x) + mad_vvv(3, mine, inner + 2 + sg[0])) >> 2;
		}
		f = edge_on[0] ? f : mine;
		P[0] = first ? f : P[0];
		P[7] = first ? P[7] : f;
	}
	else
	{
		int fl[NR], fr[NR];
#pragma unroll
		for (int ed = 0; ed < M::NE; ed++)
		{
			const int s = 4 * M::edge_quad(ed);              // l1 = P[s+2], l0 = P[s+3] | r0 = P[s+4], r1 = P[s+5]
			if (OVERLAP || ONE)
			{
				fl[ed] = (P[s + 4] + mad_vvv(3, P[s + 3], P[s + 2] + 2)) >> 2;
				fr[ed] = (P[s + 3] + mad_vvv(3, P[s + 4], P[s + 5] + 2)) >> 2;
			}
			else
			{
				const int x = sg[ed] ^ sg[ed + 1];
				fl[ed] = (((P[s + 4] ^ x) - x) + mad_vvv(3, P[s + 3], P[s + 2] + 2 + sg[ed])) >> 2;
				fr[ed] = (((P[s + 3] ^ x) - x) + mad_vvv(3, P[s + 4], P[s + 5] + 2 + sg[ed + 1])) >> 2;
			}
		}
#pragma unroll
		for (int ed = 0; ed < M::NE; ed++)
		{
			const int s = 4 * M::edge_quad(ed);
			P[s + 3] = edge_on[ed] ? fl[ed] : P[s + 3];
			P[s + 4] = edge_on[ed] ? fr[ed] : P[s + 4];
		}
	}

	// scale, add, clip (vfgs_hw.c:263-267)
	// round(scale * P, shift) (vfgs_hw.c:263) = (scale * 2^(16-shift) * P + 2^15) >> 16 exactly; the LUT holds
	// scale * 2^(16-shift), so the shift is free: the pack below simply takes the high halves
	// Ranges, at the widest case -- 12 bit, where the stored shift is 4..9 (vfgs_hw.c:349,356-359: shift + 6 - bs) and an entry reaches 255 << 12:
	//   * entry: 255 << 12 = 1 044 480 < 2^23, so +entry and -entry fit the signed 24-bit operand of v_mad_i32_i24;
	//   * |P|: a pattern byte is at most 128, the overlap blend (w_cur + w_up <= 40, >> 5) at most (128 * 40 + 16) >> 5 = 160, the 3-tap
	//     edge filter on blended values at most (5 * 160 + 2) >> 2 = 200; 200 * 1 044 480 + 0x8000 = 208 928 768 < 2^31;
	//   * the grain that comes out of the high half is at most 208 928 768 >> 16 = 3187 in magnitude; clip2 caps the sample at 0x7000 = 28 672
	//     first, so the int16 sum lies in [-3188, 31 860]: inside int16 (at 10 bit the entry reaches 255 << 10 and the grain 797, at 8 bit
	//     255 << 8 and 199).
	// scaled grain of sample i, before the final >> 16: from the value itself where the edge filter may have changed it, straight
	// from the pattern byte (one-pattern form, no overlap blend) everywhere else
	auto edge_sample = [](int i) {
		if (M::PAIR) return i == 0 || i == NS - 1;
		for (int ed = 0; ed < M::NE; ed++)
			if (i == 4 * M::edge_quad(ed) + 3 || i == 4 * M::edge_quad(ed) + 4) return true;
		return false;
	};
	int G[NS];
#pragma unroll
	for (int i = 0; i < NS; i++)
	{
		// (8 bit only: +1..2 % there, 8 VGPRs fewer and no spill left in the all-one-pattern kernels; at 10 bit the same change
		// lets the compiler reach six waves per SIMD, which these kernels do not like: -1..-2.5 %, profiles/r04_ab5_sdwa_multiply.log)
		if (PK) G[i] = mad_i24(P[i], e[i], 1 << (pkshift - 1)) << (16 - pkshift);     // (overlap lines only; < 2^24: |P| <= 199, scale <= 255)
		else if (DEPTH == 8 && ONE && !OVERLAP && !edge_sample(i)) G[i] = mul_byte_i24(i % 4, pdw[i / 4], e[i]) + 0x8000;
		else G[i] = mad_i24(P[i], e[i], 0x8000);
	}
	auto clip2 = [&](uint32_t v, int g0, int g1) {
		const uint32_t gp = __builtin_amdgcn_perm((uint32_t)g1, (uint32_t)g0, 0x07060302);
		if (DEPTH > 8)  // a 16-bit container may hold anything: keep the add inside int16 (result is clipped anyway)
			v = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, v), __builtin_bit_cast(u16x2, 0x70007000u)));
		s16x2 s = __builtin_bit_cast(s16x2, v) + __builtin_bit_cast(s16x2, gp);
		s = __builtin_elementwise_max(s, __builtin_bit_cast(s16x2, lo2));
		s = __builtin_elementwise_min(s, __builtin_bit_cast(s16x2, hi2));
		return __builtin_bit_cast(uint32_t, s);
	};
	if (DEPTH > 8)
	{
#pragma unroll
		for (int d = 0; d < 4; d++)
			w[d] = clip2(w[d], G[2 * d], G[2 * d + 1]);
	}
	else
	{
#pragma unroll
		for (int d = 0; d < 4; d++)
		{
			const uint32_t v01 = __builtin_amdgcn_perm(0, w[d], 0x0c010c00), v23 = __builtin_amdgcn_perm(0, w[d], 0x0c030c02);
			const uint32_t s01 = clip2(v01, G[4 * d], G[4 * d + 1]);
			const uint32_t s23 = clip2(v23, G[4 * d + 2], G[4 * d + 3]);
			w[d] = __builtin_amdgcn_perm(s23, s01, 0x06040200);
		}
	}
}


// ---------------------------------------------------------------------------------------
// Luma / chroma mix of the look-up index (AFGS1 cb_mult / cb_luma_mult / cb_offset).
//
// One memory unit of a chroma row (c: 16 bytes) and the luma above it (l: 16 x SUBX bytes of luma row cy * suby) -> the unit's index
// dwords m, in the sample layout:  m = clip(((avgL * lm + C * cm) >> 6) + off, 0, 2^depth - 1), avgL = the rounded mean of the two luma
// samples over a horizontally subsampled chroma sample.  32-bit arithmetic per sample: L * lm + C * cm needs 8 + 8 + 1 bits at 8 bit and
// 16 + 8 + 1 with a 16-bit container that holds anything, so nothing is packed; both products fit the 24-bit multiplier
// (65535 x 128 < 2^23).  nv = index of the row's last luma sample (width - 1) relative to the unit's first: behind it the second sample
// of a pair is the row's last one (lw1), which only the lanes at a row's end see.
template <int DEPTH, int SUBX>
__device__ __forceinline__ void mix_index(const uint32_t (&c)[4], uint32_t (&l)[4 * SUBX], const int lm, const int cm, const int off,
                                          const int nv, const uint32_t lw1, uint32_t (&m)[4])
{
	constexpr int NS = DEPTH == 8 ? 16 : 8;
	constexpr int MAXV = (1 << DEPTH) - 1;
	if constexpr (SUBX == 2)
	{
		if (nv < 2 * NS - 1)
		{
#pragma unroll
			for (int j = 0; j < NS; j++)
			{
				if (2 * j + 1 <= nv) continue;
				if (DEPTH > 8) l[j] = (l[j] & 0xffffu) | (lw1 << 16);
				else l[j / 2] = (l[j / 2] & ~(0xff00u << (16 * (j % 2)))) | (lw1 << (16 * (j % 2) + 8));
			}
		}
	}
	auto one = [&](uint32_t L, uint32_t C) {
		const int v = ((__mul24((int)L, lm) + __mul24((int)C, cm)) >> 6) + off;
		return (uint32_t)min(max(v, 0), MAXV);
	};
#pragma unroll
	for (int d = 0; d < 4; d++)
	{
		if (DEPTH > 8)
		{
			uint32_t r[2];
#pragma unroll
			for (int h = 0; h < 2; h++)
			{
				const uint32_t C = h ? c[d] >> 16 : c[d] & 0xffffu;
				uint32_t L;
				if (SUBX == 2) { const uint32_t x = l[(2 * d + h) % (4 * SUBX)]; L = ((x & 0xffffu) + (x >> 16) + 1) >> 1; }
				else L = h ? l[d] >> 16 : l[d] & 0xffffu;
				r[h] = one(L, C);
			}
			m[d] = r[0] | (r[1] << 16);
		}
		else
		{
			uint32_t r[4];
#pragma unroll
			for (int i = 0; i < 4; i++)
			{
				const uint32_t C = (c[d] >> (8 * i)) & 0xffu;
				uint32_t L;
				if (SUBX == 2) { const uint32_t x = l[(2 * d + i / 2) % (4 * SUBX)] >> (16 * (i % 2)); L = ((x & 0xffu) + ((x >> 8) & 0xffu) + 1) >> 1; }
				else L = (l[d] >> (8 * i)) & 0xffu;
				r[i] = one(L, C);
			}
			m[d] = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
		}
	}
}

// ---------------------------------------------------------------------------------------
// memory helpers

template <int AUX>
__device__ __forceinline__ void load_seg(__amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff, uint32_t (&w)[4])
{
	const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, AUX);
	w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
}

// A buffer store of more than 64 bits reads its data registers AFTER it has issued; a VALU write to them in the next
// cycle changes what the last lanes (12..15 of every 16) store.  The compiler's hazard recognizer inserts the wait state
// only for stores WITHOUT a scalar offset register (the documented form of the hazard); on gfx950 the stores with one
// need it too (found the hard way: DESIGN.md 4 "store data hazard").  Two wait states after every such store.
__device__ __forceinline__ void store_data_hazard()
{
	__builtin_amdgcn_sched_barrier(0);     // nothing may move between the store and the wait states
	asm volatile("s_nop 1");
	__builtin_amdgcn_sched_barrier(0);
}

// one unit of the destination: 16 bytes, or 8 where a 10-bit source is narrowed to 8 bit (DW = 2)
template <int DW, int AUX>
__device__ __forceinline__ void store_unit(__amdgpu_buffer_rsrc_t rs, uint32_t voff, const uint32_t (&w)[DW])
{
	if constexpr (DW == 4)
	{
		const u32x4 t = {w[0], w[1], w[2], w[3]};
		__builtin_amdgcn_raw_buffer_store_b128(t, rs, voff, 0, AUX);
		store_data_hazard();
	}
	else
	{
		const u32x2 t = {w[0], w[1]};
		__builtin_amdgcn_raw_buffer_store_b64(t, rs, voff, 0, AUX);
	}
}

// register sets of a wave's ring for a plane of this depth and form (vfgs_layout.h VFGS_RING*)
template <int DEPTH, bool ONE>
constexpr int ring_depth() { return (DEPTH == 8 && ONE && kPk16) ? VFGS_RING_PK : ((DEPTH > 8 && ONE) ? VFGS_RING_ONE10 : VFGS_RING); }

// ---------------------------------------------------------------------------------------
// Row walk: one workgroup's share of one plane.
//
// tools/skeleton2.hip (profiles/r03_skeleton2_*.log) priced what round 2's tiled kernels paid besides their bytes: every
// vector-memory INSTRUCTION queues for the CU's saturated memory pipeline, and a 4 KiB tile cost 11 of them where 8 move
// data (narrow accesses at both tile edges), plus 8 LFSR loads per wave: 0.73 -> 0.67 of 8 TB/s.
// Here a wave owns whole ROWS instead of a tile of several rows:
//   * a workgroup = 4 waves = 4 x rw_rpw rows of ONE block row (wave w: rows w, w + 4, ...); a wave streams its row position
//     by position (64 aligned 16-byte units each) through a ring of four register sets -- the refill of a set is the position
//     four steps ahead, across row ends -- so a row costs one load and one store per KiB and nothing else;
//   * the block parameters of the row's blocks (this block row's LFSR registers and, for the workgroup that holds the overlap
//     lines, those of the block row above) are computed ONCE per workgroup, one or two blocks per thread, and kept in LDS
//     behind the table image; a lane reads its 1-3 entries per position;
//   * lanes compute the half-block shifted bytes: rotation by one lane with DPP wave_shr / wave_shl, the hand-over between
//     consecutive positions of a row with wave_ror / wave_rol (the previous position's lane 63 waits in lane 0 of a register
//     and enters as the `old` operand of the shift: no v_readlane, no scalar round trip); a position's units are stored one
//     step later, once lane 0 of the next position has delivered the last dwords of its lane 63;
//   * row bases and position offsets live in the buffer descriptor (base, num_records = bytes of the row left), so the
//     hardware range check covers every access of every lane: lanes behind the row's end load 0 and store nothing
//     (8-bit 4:2:x rows of an odd number of blocks end in HALF a unit: the check works per dword);
//   * rows of more than kTileBlocks blocks (WIDE kernels): the table holds one PART of
//     the row (kTileBlocks blocks) at a time; all waves walk part 0 of their row, the workgroup refills the table for part 1
//     between two barriers, and so on -- the ring of register sets simply runs on (the host gives such workgroups one row per wave);
//   * OUT8 (10- or 12-bit source, 8-bit destination, yuv.c:216-258): out8 = (v + 2) >> 2 (12 bit: (v + 8) >> 4) is applied to a lane's results, which
//     halves them (DW = 2 dwords per unit); everything behind the computation -- rotation back, stores, descriptors -- works
//     on those halves with the destination's own pitches.
//   * MIX (chroma planes of grain_mix_kernel): a position also loads the 16 x SUBX bytes of luma row cy * SUBY that lie over a
//     lane's chroma unit -- same descriptors-per-group scheme, so they are 16-byte coalesced and range-checked against the luma row, and
//     issued with the position's own sample loads: they are part of the ring, which is two sets deep here -- forms the index dwords in
//     the unit's layout (mix_index) and sends them through the same lane shift as the samples.
//   * SP (luma planes of grain_sp_kernel, 16-bit containers): the samples sit KernelArgs::sp_shift2 bits up in their containers; a position's
//     units are shifted down as they leave the ring and the results up before they go to memory (a packed 16-bit shift per dword each way).
//     SP with OUT8 (luma planes of grain_sp8_kernel): shifted down the same way, then narrowed like any OUT8 plane and not shifted up.
//     SP = 2 (luma planes of grain_p2sp_kernel / grain_p2sp8_kernel: a PLANAR source, a semi-planar destination): the source is read as it lies,
//     low-aligned -- nothing is shifted down -- the results go up or are narrowed as above, and the destination has a geometry of its own
//     (dpitch, drowbytes) at either container size.
//     SP = 3 (luma planes of grain_sp_kernel / grain_spml_kernel): SP = 1 whose destination may be a PLANAR picture, decided at RUN time by
//     KernelArgs::sp_kernel == 3 (vfgs_hip_add_grain_sp_frame_list_to_planar_dev) without a branch: the walk always stores through the
//     destination's own geometry -- for a surface the host passes the source's (dpitch == pitch, drowbytes == rowbytes) -- and the shift up
//     comes from a scalar that is 0 where the destination holds low-aligned samples.  (A second instantiation chosen per workgroup, as the UV
//     walk has it, was built and costs MORE registers: the scalars it spills take vector registers of the whole kernel, and the 8-bit
//     general-form kernels then spill two of those to scratch.)
//   * MODELS (grain_ml_kernel, and with SP the luma planes of grain_spml_kernel: a model per frame): the table image, the clip bounds and the packed form's shift are those of the
//     workgroup's FRAME -- FrameTable::model[f] points at a ModelRecord with the image behind it -- fetched with scalar loads (the pointer from
//     the kernel arguments, the record through it) in front of the image loads; everything they feed stays wave-uniform.  Without the flag
//     the values are the launch's, from KernelArgs, and nothing of this exists.
//     MODELS = 2 (both plane types of grain_mix_kernel without OUT8 and WIDE, the luma planes of grain_sp_mix_kernel): decided at RUN time by
//     KernelArgs::models_kernel, a wave-uniform branch around the scalar loads -- the same kernel serves the programmed mix (the launch's
//     values) and listed frames whose models carry a mix of their own (the frame's values; MIX: the mix words of its record too, not
//     KernelArgs::mix).  A value of its own so that the instantiations every other kernel uses stay what they were.
//     MODELS = 2 with OUT8 (every plane of grain_rw_kernel<.., OUT8, .., !WIDE, !PERSIST>, the luma planes of grain_sp8_kernel): the same
//     run-time decision for the narrowed destination -- the programmed _copy8 calls and the _models_copy8 lists share their kernels.
//     MODELS = 2 with SP = 2 (the luma planes of grain_p2sp_kernel / grain_p2sp8_kernel): the same run-time decision from a planar source onto a
//     surface -- the programmed _to_sp / _to_sp8 calls and the _models_to_sp / _models_to_sp8 lists share their kernels.
template <int DEPTH, int BW, int SUBX, int SUBY, int RS, int IMG_BYTES, bool ONE, int NEG, int NARROW, bool OUT8, bool WIDE, bool PERSIST, bool MIX = false, int SP = 0, int MODELS = 0>
__device__ __forceinline__ void run_plane_rw(const KernelArgs& a, const FrameTable& ft, const PlaneDesc& pd, uint8_t* lds, const int comp, const int f_in, const int r_in,
                                             const uint32_t img_off, const uint32_t bank_off, const uint32_t lut_off, const int lane, const int wave)
{
	constexpr int NS = DEPTH == 8 ? 16 : 8;
	constexpr int SZ = DEPTH > 8 ? 2 : 1;
	constexpr int SB = ONE ? ((DEPTH == 8 && kPk16) ? 2 : 1) : kSlots;     // bytes of a bank per sample position (vfgs_layout.h)
	using M = LaneMap<NS, BW>;
	constexpr int NR = M::NR;
	constexpr int RPB = 16 / SUBY;                       // rows of this plane per block row
	constexpr int NEF = M::PAIR ? 1 : M::NE;
	constexpr int K = M::SHIFT * SZ / 4;                 // dwords of a lane that lie in the memory unit before the lane's own
	constexpr int DW = OUT8 ? 2 : 4;                     // dwords of a unit in the destination ...
	constexpr int KD = OUT8 ? K / 2 : K;                 // ... and how many of a lane's result dwords belong to the unit before its own
	static_assert(!OUT8 || (DEPTH > 8 && K % 2 == 0), "the narrowed destination exists for 16-bit containers");
	constexpr int LDA = VFGS_LDAUX_ALIGNED, STA = VFGS_STAUX_ALIGNED;
	constexpr int LPB = M::PAIR ? 1 : M::BPL;            // blocks per lane step (PAIR: half a block, see idx0 below)
	constexpr int BPS = M::PAIR ? 32 : 64 * M::BPL;      // grain blocks a position advances by
	// positions per group = register sets of the ring = how many positions behind its load a position is stored (vfgs_layout.h)
	// (narrow one-pattern planes at 10 bit -- rows of one or two positions: the chroma of 1080p -- walk with a ring of their own depth: vfgs_layout.h)
	constexpr int NU = MIX ? 2 : ((DEPTH > 8 && ONE && NARROW != 0) ? VFGS_RING_NARROW10 : ring_depth<DEPTH, ONE>());
	constexpr int GPP = kTileBlocks / (NU * BPS);        // groups per part of a row (a part = kTileBlocks blocks = one parameter table)
	static_assert(GPP * NU * BPS == kTileBlocks, "a part is a whole number of groups");
	constexpr uint32_t PT_CUR = IMG_BYTES, PT_UP = IMG_BYTES + kParamTableBytes;
	static_assert(IMG_BYTES % 16 == 0, "table image in whole 16-byte units");
	static_assert(!(PERSIST && (WIDE || NARROW != 0)), "persistent workgroups walk ordinary rows");
	static_assert(!MIX || (ONE && NARROW == 0 && !PERSIST), "the mix exists for one-pattern chroma walked row by row");
	static_assert(!SP || (NARROW == 0 && !WIDE && !PERSIST && !MIX), "semi-planar frames: the plain luma walk (OUT8: of grain_sp8_kernel)");
	static_assert(!MODELS || (!WIDE && !PERSIST && (!MIX || MODELS == 2) && (SP != 2 || (MODELS == 2 && !MIX)) && (!OUT8 || (MODELS == 2 && !MIX))), "a model per frame: the plain walk (SP: the luma of grain_spml_kernel), one task per workgroup; under the mix, with the narrowed destination and from a planar source onto a surface: decided at run time");
	constexpr bool DGEO = OUT8 || SP == 2 || SP == 3;    // the destination has a geometry of its own
	const int pt = comp ? 1 : 0;
	auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };

	// One TASK = what a workgroup of the non-persistent launch does: the rows of one part of one block row of frame f.  A
	// persistent workgroup (PERSIST: general-form luma of small pictures, where the 36 KB table image is more than the 15-30 KB
	// of samples it serves) runs several tasks with ONE staging of the image: only the block parameters are per task (their
	// LFSR words and the task's first four positions are requested before the workgroup meets at the barrier that frees the
	// parameter table).
	// (run_uv_sp below restates the placement, the LFSR loads, the parameter-table fill and the group / descriptor logic of this lambda for the
	// interleaved UV plane of semi-planar frames: a fix here belongs there too)
	auto task = [&](const int f, const int r, const bool first_task) {
	// ---- the workgroup's place: block row of the stripe, part of it; the wave's rows -------------------------------
	const int split = r & (pd.rw_splits - 1);
	const int kbr = uni(r >> pd.rw_lsplits);             // block row inside the stripe
	const int Rabs = (a.y0 >> 4) + kbr;                  // absolute block row
	const int row_first = (a.y0 + SUBY - 1) / SUBY;      // first row of the stripe in this plane; the plane pointers address row y0 / SUBY
	const int prow0 = a.y0 / SUBY;
	const int alo = max(row_first, Rabs * RPB), ahi = min(row_first + pd.nrows, (Rabs + 1) * RPB);
	const int rpw = pd.rw_rpw;
#if VFGS_RW_CONSEC
	const int RSTR = 1;                                  // a wave's rows are consecutive (a contiguous stream where the rows are)
	const int base = uni(Rabs * RPB + split * (kWavesPerWG * rpw) + wave * rpw);     // my rows: base + RSTR * k, k in [k0, k1)
	int k0 = max(0, alo - base), k1 = min(rpw, max(0, ahi - base));
#else
	constexpr int RSTR = kWavesPerWG;                    // the waves of a workgroup walk down its rows side by side
	const int base = uni(Rabs * RPB + split * (kWavesPerWG * rpw) + wave);
	int k0 = (max(0, alo - base) + kWavesPerWG - 1) / kWavesPerWG, k1 = min(rpw, (max(0, ahi - base) + kWavesPerWG - 1) / kWavesPerWG);
#endif
	if (kbr >= a.nbrows || k1 < k0) k1 = k0;
	k0 = uni(k0); k1 = uni(k1);
	const bool wg_up = (Rabs > 0) && (split == 0);       // this workgroup holds the overlap lines of its block row (vfgs_hw.c:175,180)

	const int last = a.nblk - 1;
	const uint32_t cur_bit = a.cur_bit0 + (uint32_t)f * a.frame_bit_step + (uint32_t)(kbr * a.nblk);
	const uint32_t up_bit = (kbr > 0) ? cur_bit - (uint32_t)a.nblk : a.up_bit0 + (uint32_t)f * a.frame_bit_step;

	// ---- in flight together: the table image, the LFSR words of the row's blocks, my first four positions ----------
	// (in this order: a wave's loads return in issue order; fixed instruction stream)
	constexpr int STEP = kWavesPerWG * 64 * 16;
	constexpr int NIT = (IMG_BYTES + STEP - 1) / STEP;
	u32x4 tmp[NIT];
	// MODELS: my frame's model -- its record (constant address space: scalar loads) and the image behind it
	// (MODELS == 2: where the launch names no models these stay the launch's own values)
	const uint8_t* mtables = MODELS == 2 ? a.tables : nullptr;
	uint32_t mlo2 = MODELS == 2 ? a.lo2[pt] : 0, mhi2 = MODELS == 2 ? a.hi2[pt] : 0;
	int mpk_shift = MODELS == 2 ? a.pk_shift : 0;
	uint32_t mmix = 0;                    // MIX: my component's mix word of the record (model_mix_word)
	const bool per_model = MODELS == 2 ? a.models_kernel != 0 : MODELS != 0;
	if constexpr (MODELS != 0)
	{
		if (per_model)
		{
			typedef const uint32_t __attribute__((address_space(4)))* crec_t;
			const uint8_t* const mp = ft.model[f];
			const crec_t rec = (crec_t)(uintptr_t)mp;
			mlo2 = rec[pt]; mhi2 = rec[2 + pt];
			mpk_shift = (int)rec[4];
			if constexpr (MIX) mmix = rec[comp == 2 ? 7 : 6];
			mtables = mp + kModelRecordBytes;
		}
	}
	if (!PERSIST || first_task)
	{
		const __amdgpu_buffer_rsrc_t irs = make_rsrc((MODELS ? mtables : a.tables) + img_off, IMG_BYTES);
#pragma unroll
		for (int it = 0; it < NIT; it++)      // threads beyond the image re-read (and re-write) its last unit
			tmp[it] = __builtin_amdgcn_raw_buffer_load_b128(irs, min((uint32_t)(threadIdx.x * 16 + it * STEP), (uint32_t)(IMG_BYTES - 16)), 0, 0);
	}
	// parameter table of the part that begins at block B0: entry e = block B0 + e - 1 (clamped into the row); thread t fills
	// entries t, t + 256, ...
	constexpr int NPE = (kParamEntries + kWavesPerWG * 64 - 1) / (kWavesPerWG * 64);
	const __amdgpu_buffer_rsrc_t strs = make_rsrc((const uint8_t*)a.stream, a.stream_bytes);
	const __amdgpu_buffer_rsrc_t strs_up = make_rsrc((const uint8_t*)a.stream, wg_up ? a.stream_bytes : 0);
	auto param_loads = [&](const int B0, u32x2 (&wc)[NPE], u32x2 (&wu)[NPE]) {
#pragma unroll
		for (int i = 0; i < NPE; i++)
		{
			const int e = (int)threadIdx.x + i * kWavesPerWG * 64;
			const uint32_t blk = (uint32_t)min(max(B0 + e - 1, 0), last);
			const bool need = e < a.nblk - B0 + 4 && e < kParamEntries;
			wc[i] = __builtin_amdgcn_raw_buffer_load_b64(strs, need ? ((cur_bit + blk) >> 5) * 4 : kOOB, 0, 0);
			wu[i] = __builtin_amdgcn_raw_buffer_load_b64(strs_up, need ? ((up_bit + blk) >> 5) * 4 : kOOB, 0, 0);
		}
	};
	const int fsx = comp == 0 ? 0 : (comp == 1 ? 10 : 20);
	const int fsy = comp == 0 ? 14 : (comp == 1 ? 24 : 4);
	const int fsb = comp == 0 ? 31 : (comp == 1 ? 2 : 15);
	auto param_table = [&](const int B0, const u32x2 (&wc)[NPE], const u32x2 (&wu)[NPE]) {
#pragma unroll
		for (int i = 0; i < NPE; i++)
		{
			// (rows of up to 252 blocks -- 2160p and narrower -- need the first round only, 4320p two of the three: a wave-uniform
			// branch around arithmetic and LDS writes; the LFSR loads stay unconditional, switched off by their offsets, so
			// that the waits can still be counted)
			if (i > 0 && i * kWavesPerWG * 64 >= a.nblk - B0 + 4) break;
			const int e = (int)threadIdx.x + i * kWavesPerWG * 64;
			const uint32_t blk = (uint32_t)min(max(B0 + e - 1, 0), last);
			bool neg;
			const uint32_t vc = __builtin_amdgcn_alignbit(wc[i].y, wc[i].x, (cur_bit + blk) & 31);
			const uint32_t pc = (block_param<SUBX, SUBY, RS, SB>(vc, bank_off, fsx, fsy, fsb, &neg) + ((ONE && neg) ? (uint32_t)NEG : 0u)) | (neg ? 0x80000000u : 0u);
			const uint32_t vu = __builtin_amdgcn_alignbit(wu[i].y, wu[i].x, (up_bit + blk) & 31);
			const uint32_t pu = block_param<SUBX, SUBY, RS, SB>(vu, bank_off, fsx, fsy, fsb, &neg) | (neg ? 0x80000000u : 0u);
			if (e < kParamEntries)
			{
				*(uint32_t*)(lds + PT_CUR + e * 4) = pc;
				*(uint32_t*)(lds + PT_UP + e * 4) = pu;
			}
		}
	};
	u32x2 wc0[NPE], wu0[NPE];
	param_loads(0, wc0, wu0);
	// A row = rw_segs wave accesses ("positions": its units and the one behind them), walked in groups of four: the four
	// register sets.  One buffer descriptor serves a whole group: base = the first byte of the group, num_records = the
	// bytes the row has left from there (at most the group's 4 KiB), the position's 1 KiB step sits in the instruction's
	// immediate offset: the hardware range check switches off exactly the lanes behind the row's end -- and every lane of a
	// group that does not exist -- and no access of any lane can leave the row.  (Measured on gfx950: a scalar offset
	// operand IS part of what is checked against num_records, so the row offset has to go into the base.)
	const int tsegs = pd.rw_segs;
	const int ngroups = (tsegs + NU - 1) / NU;
	// (frames at a constant pitch, or a list of frames anywhere: their pointers sit in the kernel arguments, one scalar load)
	const uint8_t* sbase = a.listed ? ft.src[comp][f] : a.src[comp] + (uint64_t)f * pd.fpitch;
	uint8_t* dbase = a.listed ? ft.dst[comp][f] : a.dst[comp] + (uint64_t)f * pd.dfpitch;
	const uint32_t lane16 = (uint32_t)lane * 16;
	const uint32_t laned = (uint32_t)lane * (4 * DW);    // ... in the destination
	constexpr uint32_t UB = kMaxUnits * 16, UBD = kMaxUnits * 4 * DW;   // bytes of a position, source / destination
	constexpr uint32_t GB = NU * UB, GBD = NU * UBD;     // bytes of a group
	auto row_off = [&](int k) { return (uint32_t)((base + RSTR * k - prow0) * (int)pd.pitch); };
	// (only the narrowed destination has a geometry of its own: otherwise the host passes the source's, and saying so here
	// saves the scalar registers of a second set of row offsets)
	auto row_offd = [&](int k) { return DGEO ? (uint32_t)((base + RSTR * k - prow0) * (int)pd.dpitch) : row_off(k); };
	auto left = [&](int g) { const uint32_t o = (uint32_t)g * GB; return o < pd.rowbytes ? min(pd.rowbytes - o, GB) : 0u; };
	auto leftd = [&](int g) { const uint32_t o = (uint32_t)g * GBD, rb = DGEO ? pd.drowbytes : pd.rowbytes; return o < rb ? min(rb - o, GBD) : 0u; };
	uint32_t w[NU][4];
	// MIX: the luma over my chroma units (row cy * SUBY of the luma plane, SUBX units per chroma unit), in the ring with them
	constexpr int LQ = MIX ? SUBX : 1;
	const PlaneDesc& pl = a.pd[0];
	const uint8_t* lbase = MIX ? (a.listed ? ft.src[0][f] : a.src[0] + (uint64_t)f * pl.fpitch) : nullptr;
	auto lrow_off = [&](int k) { return (uint32_t)(((base + RSTR * k) * SUBY - a.y0) * (int)pl.pitch); };
	uint32_t lw[MIX ? NU : 1][4 * LQ];
	auto load_luma = [&](const __amdgpu_buffer_rsrc_t rs, const int u) {
#pragma unroll
		for (int i = 0; i < LQ; i++)
		{
			const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, lane16 * LQ + i * 16, 0, 0);
			lw[u][4 * i] = t.x; lw[u][4 * i + 1] = t.y; lw[u][4 * i + 2] = t.z; lw[u][4 * i + 3] = t.w;
		}
	};
	if constexpr (NARROW == 0)
	{
		const __amdgpu_buffer_rsrc_t rs0 = make_rsrc(sbase + (k0 < k1 ? row_off(k0) : 0u), k0 < k1 ? left(0) : 0u);
#pragma unroll
		for (int u = 0; u < NU; u++) load_seg<LDA>(rs0, lane16 + u * UB, 0, w[u]);
		if constexpr (MIX)
		{
#pragma unroll
			for (int u = 0; u < NU; u++)
			{
				// (a descriptor per position: the position's step is twice 1 KiB at 4:2:x and need not fit the immediate offset)
				const uint32_t o = (uint32_t)u * (UB * LQ);
				const bool on = k0 < k1 && o < pl.rowbytes;
				load_luma(make_rsrc(lbase + (on ? lrow_off(k0) + o : 0u), on ? min(pl.rowbytes - o, UB * LQ) : 0u), u);
			}
		}
	}
	else
	{
		// rows of NARROW positions: the four register sets hold 4 / NARROW consecutive rows of the wave
#pragma unroll
		for (int u = 0; u < NU; u++)
		{
			const int k = k0 + u / NARROW;
			const __amdgpu_buffer_rsrc_t rs0 = make_rsrc(sbase + (k < k1 ? row_off(k) : 0u), k < k1 ? pd.rowbytes : 0u);
			load_seg<LDA>(rs0, lane16 + (u % NARROW) * UB, 0, w[u]);
		}
	}
	if (!PERSIST || first_task)
	{
#pragma unroll
		for (int it = 0; it < NIT; it++)
			*(u32x4*)(lds + min((uint32_t)(threadIdx.x * 16 + it * STEP), (uint32_t)(IMG_BYTES - 16))) = tmp[it];
	}
	else
		__syncthreads();       // every wave is done with the previous task's parameter table

	// ---- block parameters of the row's first part (once per workgroup and task) --------------------------------------
	param_table(0, wc0, wu0);
	__syncthreads();
	// (WIDE is a kernel of its own: the part loop keeps the LFSR descriptors and a few more values alive through the walk, 5-7
	// VGPRs and a dozen spilled SGPRs that every picture would pay for -- measured with -Rpass-analysis=kernel-resource-usage)
	const int nparts = WIDE ? (a.nblk + kTileBlocks - 1) / kTileBlocks : 1;     // (workgroup-uniform: every wave meets the barriers below)
	static_assert(!(WIDE && NARROW != 0), "rows walked in parts are not narrow");
	if (k0 >= k1 && nparts == 1)
		return;

	// ---- per lane constants ------------------------------------------------------------------------------------------
	const uint32_t lutb = lut_off * 0x10001u;
	const uint32_t lo2 = MODELS ? mlo2 : a.lo2[pt], hi2 = MODELS ? mhi2 : a.hi2[pt];
	const bool first = M::PAIR && (lane & 1);                             // PAIR: odd lane positions hold the first half of a block
	const uint32_t pairoff = M::PAIR ? (first ? 0u : 8u * SB) : 0u;
	const uint32_t idx0 = (M::PAIR ? (uint32_t)(lane + 1) >> 1 : (uint32_t)lane * LPB) * 4;   // byte offset of my first entry in position 0 of a part
	const int cl = M::PAIR ? lane - 1 - (lane & 1) : lane * LPB - 1;       // PAIR: left unit of my lane pair; else: block of run 0 (both for position 0)
	constexpr int SSTEP = M::PAIR ? 64 : BPS;                              // what `cl` advances by per position
	// DPP moves by one lane; lanes without a source lane (lane 0 / lane 63) keep `old`; the rotations wrap around
	auto lane_up = [](uint32_t old, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xf, 0xf, false); };    // wave_shr:1: lane l <- lane l - 1
	auto lane_down = [](uint32_t old, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x130, 0xf, 0xf, false); };  // wave_shl:1: lane l <- lane l + 1
	auto rot_up = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x13c, 0xf, 0xf, false); };      // wave_ror:1: lane 0 <- lane 63
	auto rot_down = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x134, 0xf, 0xf, false); };    // wave_rol:1: lane 63 <- lane 0
	// a lane's results as they go to memory: the 4 dwords themselves, or narrowed to 8 bit (yuv_to_8bit, yuv.c:216-258:
	// out8 = (v + 2) >> 2 at 10 bit, in general (v + 2^(bs-1)) >> bs: (v + 8) >> 4 at 12 bit; both halves of a dword are <= (255 << bs) + 2^(bs-1)
	// behind the clip: no carry across them, and the result is at most 255)
	auto results = [](const uint32_t (&t)[4], uint32_t (&o)[DW]) {
		if constexpr (OUT8)
		{
			uint32_t n[4];
#pragma unroll
			for (int d = 0; d < 4; d++) n[d] = ((t[d] + (0x00010001u << (DEPTH - 9))) >> (DEPTH - 8)) & 0x00ff00ffu;
			o[0] = __builtin_amdgcn_perm(n[1], n[0], 0x06040200);
			o[1] = __builtin_amdgcn_perm(n[3], n[2], 0x06040200);
		}
		else
		{
#pragma unroll
			for (int d = 0; d < 4; d++) o[d] = t[d];
		}
	};

	// ---- the walk ----------------------------------------------------------------------------------------------------
	// SP = 3: what the results go up by -- nothing where the destination is a planar picture (KernelArgs::sp_kernel == 3)
	const uint32_t up2 = (SP == 3 && a.sp_kernel != 3) ? a.sp_shift2 : 0u;
	uint32_t carry[4] = {0, 0, 0, 0};      // in lane 0: the last K dwords of lane 63 of the previous position of the row
	uint32_t mcarry[4] = {0, 0, 0, 0};     // MIX: the same for the index dwords
	const int mixc = comp == 2 ? 1 : 0;
	// (a model per frame: the four values out of the frame's record, scalar bit-field extracts; KernelArgs::mix is not read)
	const bool rmix = MIX && MODELS == 2 && per_model;
	const int mix_lm = MIX ? (rmix ? model_mix_luma_mult(mmix) : a.mix[mixc][0]) : 0, mix_cm = MIX ? (rmix ? model_mix_chroma_mult(mmix) : a.mix[mixc][1]) : 0;
	const int mix_off = MIX ? (rmix ? model_mix_offset(mmix) : a.mix[mixc][2]) : 0;
	const bool mix_on = MIX && (rmix ? model_mix_active(mmix) != 0 : a.mix[mixc][3] != 0);      // (a component without a mix of its own keeps the sample as its index)
	uint32_t outp[DW] = {};                // the previous position's units: dwords KD.. of its lanes (the first DW - KD dwords of a unit)
	uint32_t tp[KD > 0 ? KD : 1] = {};     // ... and the first KD dwords its lanes computed: they belong one lane down
	__amdgpu_buffer_rsrc_t pdst = make_rsrc(dbase, 0);     // where the previous GROUP's last position goes
	if constexpr (NARROW != 0)
	{
		// Rows of one or two positions (chroma of 1080p 4:2:0 at 10 bit, of 2160p at 8 bit: 2 KiB and less).  Walked row by
		// row, half of the ring would stay empty and a wave would keep 2 KiB in flight where the chip needs 4: so a group is
		// 4 / NARROW consecutive rows of the wave.  Position q of the wave's sequence = row k0 + q / NARROW, position
		// q % NARROW of it; everything that depends on the row is wave-uniform data of the slot; the overlap lines are a
		// wave-uniform branch per slot (not two walks: a group may hold one of each kind).
		constexpr int P = NARROW, RPG = NU / P;
		const int ngr = (k1 - k0 + RPG - 1) / RPG;
		for (int G = 0; G < ngr; G++)
		{
			const int kg = k0 + G * RPG;
#pragma unroll
			for (int u = 0; u < NU; u++)
			{
				const int p = u % P;                                   // position inside the row (compile time after unrolling)
				const int k = kg + u / P;                              // the slot's row
				const bool valid = k < k1, nvalid = k + RPG < k1;      // wave-uniform
				const __amdgpu_buffer_rsrc_t nsrc = make_rsrc(sbase + (nvalid ? row_off(k + RPG) : 0u), nvalid ? pd.rowbytes : 0u);
				const __amdgpu_buffer_rsrc_t cdst = make_rsrc(dbase + (valid ? row_offd(k) : 0u), valid ? (OUT8 ? pd.drowbytes : pd.rowbytes) : 0u);
				uint32_t t[4];
#pragma unroll
				for (int d = 0; d < K; d++) t[d] = lane_up(p == 0 ? 0u : carry[d], w[u][4 - K + d]);
#pragma unroll
				for (int d = 0; d < K; d++) carry[d] = rot_up(w[u][4 - K + d]);
#pragma unroll
				for (int d = K; d < 4; d++) asm volatile("v_mov_b32 %0, %1" : "=v"(t[d]) : "v"(w[u][d - K]));
				load_seg<LDA>(nsrc, lane16 + p * UB, 0, w[u]);
				if (valid)
				{
					const int j = base + RSTR * k - Rabs * RPB;        // row inside the block row
					const int jrow = j * SUBY;
					const uint32_t rowoff = (uint32_t)j * RS, uprowoff = (uint32_t)(RPB + j) * RS;
					const int wc_ = jrow == 0 ? (SUBY > 1 ? 20 : 12) : 24, wu_ = jrow == 0 ? (SUBY > 1 ? 20 : 24) : 12;
					const uint8_t* pe = lds + idx0;
					bool edge_on[NEF];
					if (M::PAIR)
					{
						const int jl = cl + p * SSTEP;
						edge_on[0] = jl >= 0 && jl + 1 < 2 * a.nblk;
					}
					else
					{
#pragma unroll
						for (int ed = 0; ed < M::NE; ed++) edge_on[ed] = (cl + p * SSTEP + ed >= 0) && (cl + p * SSTEP + ed < last);
					}
					RunParam<NR> rp, up;
#pragma unroll
					for (int rr = 0; rr < NR; rr++) rp.pa[rr] = *(const uint32_t*)(pe + PT_CUR + (p * BPS + rr) * 4) + pairoff;
					if (Rabs > 0 && jrow <= 1)     // blends in the block above (vfgs_hw.c:173-188, 223-229)
					{
#pragma unroll
						for (int rr = 0; rr < NR; rr++) up.pa[rr] = *(const uint32_t*)(pe + PT_UP + (p * BPS + rr) * 4) + pairoff;
						grain_unit<DEPTH, BW, true, ONE, ONE && SUBX == 2, NEG>(lds, t, rp, up, lutb, rowoff, uprowoff, wc_, wu_, edge_on, first, lo2, hi2, MODELS ? mpk_shift : a.pk_shift, t);
					}
					else
					{
#pragma unroll
						for (int rr = 0; rr < NR; rr++) up.pa[rr] = 0u;
						grain_unit<DEPTH, BW, false, ONE, ONE && SUBX == 2, NEG>(lds, t, rp, up, lutb, rowoff, uprowoff, 0, 0, edge_on, first, lo2, hi2, MODELS ? mpk_shift : a.pk_shift, t);
					}
				}
				uint32_t o[DW];
				results(t, o);
				// the previous position (of this row, or the last one of the row before: `pdst` is its row) is complete
#pragma unroll
				for (int d = 0; d < KD; d++) outp[DW - KD + d] = lane_down(rot_down(o[d]), tp[d]);
				store_unit<DW, STA>(pdst, laned + ((p + P - 1) % P) * UBD, outp);
				pdst = cdst;
#pragma unroll
				for (int d = KD; d < DW; d++) outp[d - KD] = o[d];
#pragma unroll
				for (int d = 0; d < KD; d++) tp[d] = o[d];
#if VFGS_SCHED_FENCE
				__builtin_amdgcn_sched_barrier(0);
#endif
			}
		}
#pragma unroll
		for (int d = 0; d < KD; d++) outp[DW - KD + d] = lane_down(0u, tp[d]);
		store_unit<DW, STA>(pdst, laned + (P - 1) * UBD, outp);
		return;
	}
	// one row, groups [g_lo, g_hi) of it (a part); `overlap` is a type so that the walk of the (rare) overlap lines is code of
	// its own: the hot loop carries neither their arithmetic nor a branch around it
	auto walk_row = [&](auto overlap, const int k, const int g_lo, const int g_hi) {
		constexpr bool OV = decltype(overlap)::value;
		const int j = base + RSTR * k - Rabs * RPB;    // row inside the block row
		const int jrow = j * SUBY;
		const uint32_t rowoff = (uint32_t)j * RS, uprowoff = (uint32_t)(RPB + j) * RS;
		const int wc_ = jrow == 0 ? (SUBY > 1 ? 20 : 12) : 24, wu_ = jrow == 0 ? (SUBY > 1 ? 20 : 24) : 12;
		const uint32_t ro = row_off(k), rod = row_offd(k);
		// MIX: the row's last luma sample, the partner of every pair behind it (the lanes at the row's end only)
		uint32_t lw1 = 0;
		const uint32_t lro = MIX ? lrow_off(k) : 0u;
		if constexpr (MIX && SUBX == 2)
		{
			const __amdgpu_buffer_rsrc_t lrs = make_rsrc(lbase + lro, pl.rowbytes);
			const uint32_t at = (uint32_t)(a.mix_lw - 1) * SZ;
			lw1 = SZ == 2 ? (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(lrs, at, 0, 0) : (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(lrs, at, 0, 0);
		}
		for (int g = g_lo; g < g_hi; g++)
		{
			// the group after this one (this row's next, or the next row's first): what the four refills fetch
			const bool lastg = g + 1 == ngroups;
			const int ng = lastg ? 0 : g + 1;
			const bool nvalid = !lastg || k + 1 < k1;
			const uint32_t nso = nvalid ? (lastg ? row_off(k + 1) : ro) + (uint32_t)ng * GB : 0u;
			const __amdgpu_buffer_rsrc_t nsrc = make_rsrc(sbase + nso, nvalid ? left(ng) : 0u);
			const __amdgpu_buffer_rsrc_t cdst = make_rsrc(dbase + (rod + (uint32_t)g * GBD), leftd(g));
			const uint8_t* pe = lds + idx0 + (uint32_t)((g - g_lo) * NU * BPS * 4);    // (the table holds the part that begins at group g_lo)
			const int clg = cl + g * NU * SSTEP;
#pragma unroll
			for (int u = 0; u < NU; u++)
			{
				const bool firsts = u == 0 && g == 0;                    // first position of the row
				// assemble my 16 bytes: the last K dwords of the unit of the lane before me, the first 4 - K of mine
				uint32_t t[4];
				uint32_t ti[4] = {};
				if constexpr ((SP == 1 || SP == 3) && DEPTH > 8)
				{
#pragma unroll
					for (int d = 0; d < 4; d++) w[u][d] = pk_lshr_b16(a.sp_shift2, w[u][d]);
				}
				if constexpr (MIX)
				{
					// index dwords of my memory unit, then the same lane shift as the samples
					uint32_t mi[4];
					if (mix_on)
						mix_index<DEPTH, SUBX>(w[u], lw[u], mix_lm, mix_cm, mix_off, a.mix_lw - 1 - (((NU * g + u) * 64 + lane) * NS * SUBX), lw1, mi);
					else
					{
#pragma unroll
						for (int d = 0; d < 4; d++) mi[d] = w[u][d];
					}
#pragma unroll
					for (int d = 0; d < K; d++) ti[d] = lane_up(firsts ? 0u : mcarry[d], mi[4 - K + d]);
#pragma unroll
					for (int d = 0; d < K; d++) mcarry[d] = rot_up(mi[4 - K + d]);
#pragma unroll
					for (int d = K; d < 4; d++) ti[d] = mi[d - K];
				}
#pragma unroll
				for (int d = 0; d < K; d++) t[d] = lane_up(firsts ? 0u : carry[d], w[u][4 - K + d]);   // (in front of a row there is nothing)
#pragma unroll
				for (int d = 0; d < K; d++) carry[d] = rot_up(w[u][4 - K + d]);
				// (real copies: were t[] merely another name for these registers, the refill below would have to land somewhere
				// else and be copied back at the end of the loop -- behind a wait for all four refills)
#pragma unroll
				for (int d = K; d < 4; d++) asm volatile("v_mov_b32 %0, %1" : "=v"(t[d]) : "v"(w[u][d - K]));
				// the registers are free: refill them with the position four steps ahead
				load_seg<LDA>(nsrc, lane16 + u * UB, 0, w[u]);
				if constexpr (MIX)
				{
					const uint32_t o = (uint32_t)(ng * NU + u) * (UB * LQ);
					const bool on = nvalid && o < pl.rowbytes;
					load_luma(make_rsrc(lbase + (on ? (lastg ? lrow_off(k + 1) : lro) + o : 0u), on ? min(pl.rowbytes - o, UB * LQ) : 0u), u);
				}
				if (NU * g + u < tsegs)
				{
					bool edge_on[NEF];
					if (M::PAIR)
					{
						const int jl = clg + u * SSTEP;                    // left unit of this lane pair
						edge_on[0] = jl >= 0 && jl + 1 < 2 * a.nblk;
					}
					else
					{
#pragma unroll
						for (int ed = 0; ed < M::NE; ed++) edge_on[ed] = (clg + u * SSTEP + ed >= 0) && (clg + u * SSTEP + ed < last);
					}
					RunParam<NR> rp, up;
#pragma unroll
					for (int rr = 0; rr < NR; rr++) rp.pa[rr] = *(const uint32_t*)(pe + PT_CUR + (u * BPS + rr) * 4) + pairoff;
#pragma unroll
					for (int rr = 0; rr < NR; rr++) up.pa[rr] = OV ? *(const uint32_t*)(pe + PT_UP + (u * BPS + rr) * 4) + pairoff : 0u;
					if constexpr (MIX)
						grain_unit<DEPTH, BW, OV, ONE, ONE && SUBX == 2, NEG, true>(lds, t, rp, up, lutb, rowoff, uprowoff, OV ? wc_ : 0, OV ? wu_ : 0, edge_on, first, lo2, hi2, MODELS ? mpk_shift : a.pk_shift, ti);
					else
						grain_unit<DEPTH, BW, OV, ONE, ONE && SUBX == 2, NEG>(lds, t, rp, up, lutb, rowoff, uprowoff, OV ? wc_ : 0, OV ? wu_ : 0, edge_on, first, lo2, hi2, MODELS ? mpk_shift : a.pk_shift, t);
				}
				uint32_t o[DW];
				results(t, o);
				if constexpr (SP && DEPTH > 8 && !OUT8)     // (the narrowed destination holds plain bytes)
				{
#pragma unroll
					for (int d = 0; d < DW; d++) o[d] = pk_lshl_b16(SP == 3 ? up2 : a.sp_shift2, o[d]);
				}
				// the previous position's units are complete once the KD dwords its lanes computed have moved one lane down; its
				// lane 63 takes them from my lane 0 (the previous position of a row's first one is the last of another row:
				// its lane 63 lies behind that row's end and is never stored)
#pragma unroll
				for (int d = 0; d < KD; d++) outp[DW - KD + d] = lane_down(rot_down(o[d]), tp[d]);
				if (u == 0) store_unit<DW, STA>(pdst, laned + (NU - 1) * UBD, outp);
				else store_unit<DW, STA>(cdst, laned + (u - 1) * UBD, outp);
#pragma unroll
				for (int d = KD; d < DW; d++) outp[d - KD] = o[d];
#pragma unroll
				for (int d = 0; d < KD; d++) tp[d] = o[d];
#if VFGS_SCHED_FENCE
				__builtin_amdgcn_sched_barrier(0);
#endif
			}
			pdst = cdst;
		}
	};
	for (int h = 0;;)
	{
		// part h of my rows (all of them -- every group -- where the row's blocks fit one table: every BASELINE size)
		const int g_lo = h * GPP, g_hi = (h + 1 == nparts) ? ngroups : (h + 1) * GPP;
		for (int k = k0; k < k1; k++)
		{
			const int jrow = (base + RSTR * k - Rabs * RPB) * SUBY;
			if (Rabs > 0 && jrow <= 1) walk_row(std::true_type(), k, g_lo, g_hi);      // blends in the block above (vfgs_hw.c:173-188, 223-229)
			else walk_row(std::false_type(), k, g_lo, g_hi);
		}
		if (++h >= nparts) break;
		// the table of the next part: every wave is done reading this one; the LFSR words come out of L2 while the ring's
		// refills are in flight (wide pictures only: one row per wave, so the walk simply continues where it stopped)
		__syncthreads();
		u32x2 wcn[NPE], wun[NPE];
		param_loads(h * kTileBlocks, wcn, wun);
		param_table(h * kTileBlocks, wcn, wun);
		__syncthreads();
	}
	// the last position of my last row
#pragma unroll
	for (int d = 0; d < KD; d++) outp[DW - KD + d] = lane_down(0u, tp[d]);
	store_unit<DW, STA>(pdst, laned + (NU - 1) * UBD, outp);
	};     // task

	if constexpr (!PERSIST)
		task(f_in, r_in, true);
	else
	{
		// my tasks: t, t + P, t + 2 P, ... of the launch's nframes x pd.wgs luma tasks (frame-major: the persistent workgroups sweep
		// the frames in memory order together); the host passes P as (frames, tasks) so that nothing is divided here
		int f = f_in, r = r_in;
		for (bool first_task = true; f < a.nframes; first_task = false)
		{
			task(f, r, first_task);
			f += a.persist_step_f;
			r += a.persist_step_r;
			if (r >= pd.wgs) { r -= pd.wgs; f++; }
		}
	}
}

// Waves per SIMD the kernels are allocated for.  The 8-bit all-one-pattern kernels: SIX since round 6 -- the packed 16-bit form with a
// ring of two register sets needs 79 registers (round 5's form needed 97..100 and was held at five with one register spilled in the
// prologue, profiles/r03_ab22_lds_probes_and_occupancy.log), and six are worth 1.4 .. 3.4 % together with the shorter ring
// (profiles/r06_ab5_ring_depth_six_waves.log); rows walked in parts stay at four, the general-form kernels are held at four by their LDS
// image, the others by spills.
#ifndef VFGS_PK_WAVES
#define VFGS_PK_WAVES 6       // waves per SIMD of the 8-bit all-one-pattern kernels (packed 16-bit form with a ring of two: 79 VGPRs, no spill)
#endif
template <int DEPTH, bool ONEY, bool ONEC, bool WIDE>
constexpr int rw_waves_per_simd()
{
#ifdef VFGS_ONE10_WAVES      // developer A/B: the 10-bit all-one-pattern kernels at another occupancy
	if (DEPTH > 8 && ONEY && ONEC && !WIDE) return VFGS_ONE10_WAVES;
#endif
	return (DEPTH == 8 && ONEY && ONEC && !WIDE && VFGS_WG_PER_CU == 4) ? (kPk16 ? VFGS_PK_WAVES : 5) : (kWavesPerWG * VFGS_WG_PER_CU + 3) / 4;
}

// in place or out of place; workgroups numbered frame -> plane -> block row -> part of the block row
template <int DEPTH, int CSUBX, int CSUBY, bool OUT8, bool ONEY, bool ONEC, bool WIDE, bool PERSIST>
__global__ __launch_bounds__(kWavesPerWG * 64, (rw_waves_per_simd<DEPTH, ONEY, ONEC, WIDE>())) void grain_rw_kernel(const KernelArgs a, const FrameTable ft)
{
	constexpr ImageLayout L = image_layout(CSUBX, CSUBY, ONEY, ONEC, DEPTH == 8);
	// (unused LDS behind the tables holds a kernel at no more than its class's workgroups per CU: vfgs_layout.h lds_allocation)
	__shared__ __attribute__((aligned(16))) uint8_t lds[lds_allocation(DEPTH > 8, ONEY, ONEC, WIDE, L.lds_bytes + kParamBytes)];

	const int lane = threadIdx.x & 63;
	// wave-uniform by construction; telling the compiler keeps the decoding, row offsets and buffer descriptors in SGPRs
	// (otherwise every buffer instruction gets a waterfall loop)
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	// grid: x = (workgroup inside the frame, frame of a group of 2^lfronts frames), y = group of frames.  Large frames are swept
	// two at a time: the workgroups of frames 2m and 2m + 1 are dealt out alternately (measured: +1.6 % at 4320p, nothing at 2160p;
	// more than two, or smaller frames: a loss -- profiles/r03_ab18_frame_fronts_in_one_launch.log)
	// A model per frame with the narrowed destination (KernelArgs::models_kernel; vfgs_hip_add_grain_frame_list_models_copy8_dev):
	// the OUT8 kernels of ordinary rows without persistence take image, bounds and shift from the frame's model where the launch names
	// models, decided at run time (run_plane_rw MODELS = 2) -- no kernel of their own.  Every other instantiation is what it was.
	constexpr int PM = (OUT8 && !WIDE && !PERSIST) ? 2 : 0;
	int f, r;
	if constexpr (PERSIST)
	{
		// grid: x = [persistent luma workgroups | one workgroup per chroma task, frame-major]; one division per workgroup
		static_assert(!ONEY && !WIDE, "persistence exists for the general-form luma image");
		if ((int)blockIdx.x < a.persist_wgs)
		{
			f = (int)blockIdx.x / a.pd[0].wgs;
			r = (int)blockIdx.x - f * a.pd[0].wgs;
			run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, ONEY, L.y_neg, 0, OUT8, WIDE, true>(a, ft, a.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
			return;
		}
		const int x = (int)blockIdx.x - a.persist_wgs, per = 2 * a.pd[1].wgs;
		f = x / per;
		r = a.pd[0].wgs + (x - f * per);
	}
	else
	{
		// (the odd front of a pair runs one plane phase behind the even one -- chroma beside luma on every CU: vfgs_layout.h front_task, DESIGN.md 5.0 "a plane phase apart")
		const FrontTask t = front_task(blockIdx.x, blockIdx.y, a.lfronts, a.pd[0].wgs + 2 * a.pd[1].wgs, a.front_shift, a.front_plain_from);
		f = t.f;
		r = t.r;
	}
	if (f >= a.nframes) return;
	if (r < a.pd[0].wgs)
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, ONEY, L.y_neg, 0, OUT8, WIDE, false, false, 0, PM>(a, ft, a.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	else
	{
		r -= a.pd[0].wgs;
		const int comp = 1 + (r >= a.pd[1].wgs);
		if (comp == 2) r -= a.pd[1].wgs;
		// horizontally subsampled chroma rows of one or two positions (2 KiB and less: 1080p at 10 bit, 2160p at 8 bit): several rows per group
		if (!WIDE && CSUBX == 2 && a.pd[1].rw_segs == 2 && ring_depth<DEPTH, ONEC>() >= 2)      // (a ring of one set cannot hold two positions of a row)
			run_plane_rw<DEPTH, 16 / CSUBX, CSUBX, CSUBY, L.c_rs, L.c_bytes, ONEC, L.c_neg, WIDE ? 0 : 2, OUT8, WIDE, false, false, 0, PM>(a, ft, a.pd[1], lds, comp, f, r, L.c_off[comp - 1], L.c_bank, L.c_lut[comp - 1], lane, wave);
		else if (!WIDE && CSUBX == 2 && a.pd[1].rw_segs == 1)
			run_plane_rw<DEPTH, 16 / CSUBX, CSUBX, CSUBY, L.c_rs, L.c_bytes, ONEC, L.c_neg, WIDE ? 0 : 1, OUT8, WIDE, false, false, 0, PM>(a, ft, a.pd[1], lds, comp, f, r, L.c_off[comp - 1], L.c_bank, L.c_lut[comp - 1], lane, wave);
		else
			run_plane_rw<DEPTH, 16 / CSUBX, CSUBX, CSUBY, L.c_rs, L.c_bytes, ONEC, L.c_neg, 0, OUT8, WIDE, false, false, 0, PM>(a, ft, a.pd[1], lds, comp, f, r, L.c_off[comp - 1], L.c_bank, L.c_lut[comp - 1], lane, wave);
	}
}

// A MODEL PER FRAME (KernelArgs::models_kernel; vfgs_hip_add_grain_frame_list_models_dev): listed frames whose models share
// the form (ONEY, ONEC) of their table images and nothing else.  The grid, the workgroup numbering, the two frame fronts, the narrow chroma
// rows, the launch bounds and the LDS allocation of grain_rw_kernel<DEPTH, CSUBX, CSUBY, false, ONEY, ONEC, false, false>; a workgroup
// stages ITS frame's image and clips with ITS frame's bounds (run_plane_rw MODELS).  No persistent luma workgroups: a workgroup that keeps
// one staged image for several tasks would need them to be tasks of one model.
template <int DEPTH, int CSUBX, int CSUBY, bool ONEY, bool ONEC>
__global__ __launch_bounds__(kWavesPerWG * 64, (rw_waves_per_simd<DEPTH, ONEY, ONEC, false>())) void grain_ml_kernel(const KernelArgs a, const FrameTable ft)
{
	constexpr ImageLayout L = image_layout(CSUBX, CSUBY, ONEY, ONEC, DEPTH == 8);
	__shared__ __attribute__((aligned(16))) uint8_t lds[lds_allocation(DEPTH > 8, ONEY, ONEC, false, L.lds_bytes + kParamBytes)];

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = (int)(blockIdx.y << a.lfronts) + (int)(blockIdx.x & ((1u << a.lfronts) - 1));
	int r = (int)(blockIdx.x >> a.lfronts);
	if (f >= a.nframes) return;
	if (r < a.pd[0].wgs)
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, ONEY, L.y_neg, 0, false, false, false, false, 0, true>(a, ft, a.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	else
	{
		r -= a.pd[0].wgs;
		const int comp = 1 + (r >= a.pd[1].wgs);
		if (comp == 2) r -= a.pd[1].wgs;
		if (CSUBX == 2 && a.pd[1].rw_segs == 2 && ring_depth<DEPTH, ONEC>() >= 2)
			run_plane_rw<DEPTH, 16 / CSUBX, CSUBX, CSUBY, L.c_rs, L.c_bytes, ONEC, L.c_neg, 2, false, false, false, false, 0, true>(a, ft, a.pd[1], lds, comp, f, r, L.c_off[comp - 1], L.c_bank, L.c_lut[comp - 1], lane, wave);
		else if (CSUBX == 2 && a.pd[1].rw_segs == 1)
			run_plane_rw<DEPTH, 16 / CSUBX, CSUBX, CSUBY, L.c_rs, L.c_bytes, ONEC, L.c_neg, 1, false, false, false, false, 0, true>(a, ft, a.pd[1], lds, comp, f, r, L.c_off[comp - 1], L.c_bank, L.c_lut[comp - 1], lane, wave);
		else
			run_plane_rw<DEPTH, 16 / CSUBX, CSUBX, CSUBY, L.c_rs, L.c_bytes, ONEC, L.c_neg, 0, false, false, false, false, 0, true>(a, ft, a.pd[1], lds, comp, f, r, L.c_off[comp - 1], L.c_bank, L.c_lut[comp - 1], lane, wave);
	}
}

// The kernels of the luma / chroma mix (KernelArgs::mix_kernel): all-one-pattern images only (AFGS1), the grid and the
// workgroup numbering of grain_rw_kernel.  Luma workgroups are grain_rw_kernel's; chroma workgroups walk every row position by position
// (no narrow-row form) with the luma over it in their ring.  KernelArgs::mix_planes switches the workgroups of one plane type off: an
// in-place call is two launches on its stream, chroma first -- it reads luma as it is before this call -- then luma.  Four workgroups per
// CU at either depth (128 registers; the LDS allocation says the same).
template <int DEPTH, int CSUBX, int CSUBY, bool OUT8, bool WIDE>
__global__ __launch_bounds__(kWavesPerWG * 64, kMixWgPerCU) void grain_mix_kernel(const KernelArgs a, const FrameTable ft)
{
	constexpr ImageLayout L = image_layout(CSUBX, CSUBY, true, true, DEPTH == 8);
	__shared__ __attribute__((aligned(16))) uint8_t lds[mix_lds_allocation(L.lds_bytes + kParamBytes)];

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = (int)(blockIdx.y << a.lfronts) + (int)(blockIdx.x & ((1u << a.lfronts) - 1));
	int r = (int)(blockIdx.x >> a.lfronts);
	if (f >= a.nframes) return;
	// A model per frame (KernelArgs::models_kernel beside mix_kernel: listed frames whose models carry a mix): both walks take the
	// image, the bounds, the shift and the mix from the frame's model, decided at run time (run_plane_rw MODELS = 2).  Not for the narrowed
	// destination and not for rows walked in parts, which models do not have: those kernels are what they were.
	constexpr int PM = (!OUT8 && !WIDE) ? 2 : 0;
	if (r < a.pd[0].wgs)
	{
		if (a.mix_planes & 1) return;
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, true, L.y_neg, 0, OUT8, WIDE, false, false, 0, PM>(a, ft, a.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	}
	else
	{
		if (a.mix_planes & 2) return;
		// Cb and Cr of the same rows read the same luma: their workgroups are numbered eight of Cb, the same eight of Cr, ... -- next to each
		// other in time and (workgroups are dealt out to the eight XCDs in turn) on the same XCD, so that the second reader finds the luma in
		// that XCD's L2 (the luma loads are ordinary loads, not nontemporal ones like the sample loads)
		r -= a.pd[0].wgs;
		const int n = a.pd[1].wgs, full = n & ~7;
		int comp;
		if (r < 2 * full) { comp = 1 + ((r >> 3) & 1); r = ((r >> 4) << 3) | (r & 7); }
		else { r -= 2 * full; comp = 1 + (r >= n - full); r = full + (comp == 2 ? r - (n - full) : r); }
		run_plane_rw<DEPTH, 16 / CSUBX, CSUBX, CSUBY, L.c_rs, L.c_bytes, true, L.c_neg, 0, OUT8, WIDE, false, true, 0, PM>(a, ft, a.pd[1], lds, comp, f, r, L.c_off[comp - 1], L.c_bank, L.c_lut[comp - 1], lane, wave);
	}
}

// ---------------------------------------------------------------------------------------
// UV walk: semi-planar frames (NV12, NV16, P010, P210, P012; vfgs_hip_add_grain_sp_frame_list_dev).
//
// The chroma of such a frame is ONE plane of interleaved Cb/Cr pairs.  A UV workgroup takes the place of the row walk's Cb workgroup
// and its Cr workgroup: the same rows of one block row, a wave owns whole UV rows, and
//   * a lane's memory unit is 32 bytes (two 16-byte buffer loads, a wave access is 2 KiB), split in registers with v_perm_b32 into one
//     planar Cb unit and one planar Cr unit -- shifted down where the samples sit in the high bits of their containers -- each exactly
//     what a lane of the planar chroma walk holds: the lane shift (DPP), the hand-over between positions, the edge filter and grain_unit
//     run on them unchanged, once with Cb's block parameters and tables, once with Cr's; the two result units are shifted up,
//     interleaved again and stored as 32 bytes, one position behind their load like every unit of the row walk;
//   * the workgroup stages both components' tables (vfgs_layout.h "semi-planar"), and computes both components' block parameters from
//     ONE load of the block row's LFSR words: Cb and Cr take different bit fields of the same register (block_param);
//   * row ends are the buffer descriptor's range check, per dword: an 8-bit row of an odd number of blocks ends in half a 32-byte unit;
//   * rows are at most kTileBlocks blocks (the host refuses wider pictures): one parameter table per component and block row.
//
// MIX (UV workgroups of grain_sp_mix_kernel; DESIGN.md 4.7 "the mix on semi-planar frames"): a position also loads the 32 bytes of luma row
// cy * SUBY that lie over a lane's 32-byte UV unit -- at either container size the luma over a UV unit begins at the UV unit's own byte offset
// of its row -- as two 16-byte buffer loads through a descriptor of the LUMA row (range-checked against what that row has left), plain loads
// issued with the position's own: they are part of the ring.  ONE read of the luma serves both components: mix_index runs on the split Cb
// unit and on the split Cr unit with the same luma registers, each with its component's multipliers; the index dwords take the samples' lane
// shift and carry, and grain_unit's LUT gathers read them.
//
// PLANAR (UV workgroups of grain_p2sp_kernel / grain_p2sp8_kernel: a planar source, vfgs_hip_add_grain_frame_list_to_sp_dev): a position's load is one
// 16-byte buffer load from the Cb row and one from the Cr row, each through a descriptor of its own plane (FrameTable::src[1] / [2]; pd.pitch and
// pd.rowbytes describe ONE component's source row, the range check is per component row) -- the two planar units the split would have produced,
// low-aligned as they lie: no v_perm_b32, no shift down.  Everything behind the load is the walk above; the destination always has a geometry
// of its own (pd.dpitch; pd.drowbytes = ONE component's bytes of a destination row, the UV row holds twice as many).
//
// MODELS (UV workgroups of grain_spml_kernel: a model per frame): both components' tables, the chroma clip bounds and the packed
// form's shift are those of the workgroup's FRAME, as in run_plane_rw MODELS -- FrameTable::model[f] from the kernel arguments, the ModelRecord
// through it with scalar loads, in front of the table loads; everything they feed stays wave-uniform.  Without the flag nothing of this exists.
// MODELS = 2 (UV workgroups of grain_sp_mix_kernel): decided at run time by KernelArgs::models_kernel, as in run_plane_rw -- the frame's model
// then also supplies both components' mix (the two mix words of its record), and KernelArgs::mix is not read.
// MODELS = 2 with OUT8 (UV workgroups of grain_sp8_kernel): the same run-time decision without a mix; BOTH components of the 16-byte unit of
// Cb/Cr byte pairs are clipped with the frame's chroma bounds (lo2 / hi2 below are one pair for the two grain_unit calls of a position).
// MODELS = 2 with PLANAR (UV workgroups of grain_p2sp_kernel / grain_p2sp8_kernel): the same run-time decision; both components of a Cb/Cr pair
// take the frame's chroma bounds.
//
// TOPL, A PLANAR DESTINATION (UV workgroups of grain_sp_kernel / grain_spml_kernel -- neither MIX, OUT8 nor PLANAR -- where KernelArgs::sp_kernel == 3:
// vfgs_hip_add_grain_sp_frame_list_to_planar_dev): decided at RUN time by the kernel, ONCE per workgroup -- a wave-uniform branch between two
// instantiations of this function, so that the walk onto a surface keeps the instructions and the registers it had before there was a choice (one
// walk with the branch at the store spilled vector registers in the 8-bit general-form kernels, which sit at 126 of 128).  The walk is the one above
// up to the two planar result units; they are neither joined nor shifted up, and go as 16 bytes each to the Cb row and to the Cr row, through a
// descriptor per component (FrameTable::dst[1] / [2]; pd.dpitch and pd.drowbytes describe ONE component's destination row, the range check is per
// component row: an 8-bit row of an odd number of blocks ends in half a 16-byte unit and the 8 bytes behind it are never written).  The kernels with
// MIX, OUT8 or PLANAR hold nothing of this.
template <int DEPTH, int SUBY, int RS, int CIMG, int BANK, bool ONE, int NEG, bool MIX = false, bool OUT8 = false, bool PLANAR = false, int MODELS = 0, bool TOPL = false>
__device__ __forceinline__ void run_uv_sp(const KernelArgs& a, const FrameTable& ft, uint8_t* lds, const int f, const int r, const uint32_t img_off, const int lane, const int wave)
{
	constexpr int NS = DEPTH == 8 ? 16 : 8;
	constexpr int SZ = DEPTH > 8 ? 2 : 1;
	constexpr int SB = ONE ? ((DEPTH == 8 && kPk16) ? 2 : 1) : kSlots;
	constexpr int BW = 8;                                // chroma samples of a grain block (csubx == 2)
	using M = LaneMap<NS, BW>;
	static_assert(!M::PAIR, "a lane of a horizontally subsampled plane holds whole half blocks");
	constexpr int NR = M::NR, NE = M::NE;
	constexpr int RPB = 16 / SUBY;
	constexpr int K = M::SHIFT * SZ / 4;                 // dwords of a planar unit that belong to the lane before its own
	constexpr int BPS = 64 * M::BPL;                     // grain blocks a position advances by
	constexpr int NU = MIX ? kSpMixRing : kSpRing;
	static_assert(!MIX || ONE, "the mix exists for one-pattern chroma");
	constexpr int DW = OUT8 ? 2 : 4;                     // dwords of a component's planar unit in the destination ...
	constexpr int KD = OUT8 ? K / 2 : K;                 // ... and how many of them belong to the lane before its own
	static_assert(!OUT8 || (DEPTH > 8 && K % 2 == 0 && !MIX), "the narrowed destination exists for 16-bit containers, without the mix");
	static_assert(!PLANAR || !MIX, "a planar source has no mix form");
	static_assert(!MODELS || ((OUT8 || PLANAR) ? (MODELS == 2 && !MIX) : MIX == (MODELS == 2)), "a model per frame: the plain UV walk; under the mix, with the narrowed destination and from a planar source: decided at run time");
	constexpr bool DGEO = OUT8 || PLANAR;                // the destination has a geometry of its own
	static_assert(!TOPL || (!OUT8 && !PLANAR && !MIX), "planes out: the kernels of the plain UV walk alone");
	constexpr int LDA = VFGS_LDAUX_ALIGNED, STA = VFGS_STAUX_ALIGNED;
	constexpr int LUTB = 2 * 256 * 4;                    // a component's pair of tables (general form)
	constexpr int IMG = sp_uv_image_bytes(CIMG, LUTB, ONE);
	constexpr uint32_t BANK_OFF = ONE ? BANK : BANK + LUTB;     // of the bank behind a component's base (general form: behind BOTH pairs of tables)
	constexpr uint32_t PT = IMG;                         // parameter tables: component c, this block row at PT + 2 c tables, the row above one further
	static_assert(IMG % 16 == 0 && CIMG % 16 == 0, "table images in whole 16-byte units");
	static_assert(kTileBlocks % (NU * BPS) == 0 || NU * BPS > kTileBlocks, "positions of whole blocks");
	const PlaneDesc& pd = a.pd[1];
	auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };

	// ---- the workgroup's place (run_plane_rw "task") ----------------------------------------------------------------
	const int split = r & (pd.rw_splits - 1);
	const int kbr = uni(r >> pd.rw_lsplits);
	const int Rabs = (a.y0 >> 4) + kbr;
	const int row_first = (a.y0 + SUBY - 1) / SUBY;
	const int prow0 = a.y0 / SUBY;
	const int alo = max(row_first, Rabs * RPB), ahi = min(row_first + pd.nrows, (Rabs + 1) * RPB);
	const int rpw = pd.rw_rpw;
	constexpr int RSTR = kWavesPerWG;
	const int base = uni(Rabs * RPB + split * (kWavesPerWG * rpw) + wave);
	int k0 = (max(0, alo - base) + kWavesPerWG - 1) / kWavesPerWG, k1 = min(rpw, (max(0, ahi - base) + kWavesPerWG - 1) / kWavesPerWG);
	if (kbr >= a.nbrows || k1 < k0) k1 = k0;
	k0 = uni(k0); k1 = uni(k1);
	const bool wg_up = (Rabs > 0) && (split == 0);

	const int last = a.nblk - 1;
	const uint32_t cur_bit = a.cur_bit0 + (uint32_t)f * a.frame_bit_step + (uint32_t)(kbr * a.nblk);
	const uint32_t up_bit = (kbr > 0) ? cur_bit - (uint32_t)a.nblk : a.up_bit0 + (uint32_t)f * a.frame_bit_step;

	// ---- in flight together: the tables, the LFSR words of the row's blocks, my first positions ------------------------
	constexpr int STEP = kWavesPerWG * 64 * 16;
	constexpr int NIT = (IMG + STEP - 1) / STEP;
	u32x4 tmp[NIT];
	// MODELS: my frame's model -- its record (constant address space: scalar loads) and the image behind it
	// (MODELS == 2: where the launch names no models these stay the launch's own values)
	const uint8_t* mtables = MODELS == 2 ? a.tables : nullptr;
	uint32_t mlo2 = MODELS == 2 ? a.lo2[1] : 0, mhi2 = MODELS == 2 ? a.hi2[1] : 0;
	int mpk_shift = MODELS == 2 ? a.pk_shift : 0;
	uint32_t mmix[2] = {0, 0};            // MIX: Cb's and Cr's mix word of the record (model_mix_word)
	const bool per_model = MODELS == 2 ? a.models_kernel != 0 : MODELS != 0;
	if constexpr (MODELS != 0)
	{
		if (per_model)
		{
			typedef const uint32_t __attribute__((address_space(4)))* crec_t;
			const uint8_t* const mp = ft.model[f];
			const crec_t rec = (crec_t)(uintptr_t)mp;
			mlo2 = rec[1]; mhi2 = rec[3];
			mpk_shift = (int)rec[4];
			if constexpr (MIX) { mmix[0] = rec[6]; mmix[1] = rec[7]; }
			mtables = mp + kModelRecordBytes;
		}
	}
	{
		// (the device image holds [LUT Cb][bank][LUT Cr][bank]: one-pattern form -- both sub-images as they are; general form -- LDS offset o
		// comes from Cb's LUT, Cr's LUT, Cb's copy of the bank)
		const __amdgpu_buffer_rsrc_t irs = make_rsrc((MODELS ? mtables : a.tables) + img_off, 2 * CIMG);
#pragma unroll
		for (int it = 0; it < NIT; it++)
		{
			const uint32_t o = min((uint32_t)(threadIdx.x * 16 + it * STEP), (uint32_t)(IMG - 16));
			const uint32_t so = ONE ? o : (o < (uint32_t)LUTB ? o : (o < 2u * LUTB ? o - LUTB + CIMG : o - LUTB));
			tmp[it] = __builtin_amdgcn_raw_buffer_load_b128(irs, so, 0, 0);
		}
	}
	constexpr int NPE = (kParamEntries + kWavesPerWG * 64 - 1) / (kWavesPerWG * 64);
	const __amdgpu_buffer_rsrc_t strs = make_rsrc((const uint8_t*)a.stream, a.stream_bytes);
	const __amdgpu_buffer_rsrc_t strs_up = make_rsrc((const uint8_t*)a.stream, wg_up ? a.stream_bytes : 0);
	u32x2 wc[NPE], wu[NPE];
#pragma unroll
	for (int i = 0; i < NPE; i++)
	{
		const int e = (int)threadIdx.x + i * kWavesPerWG * 64;
		const uint32_t blk = (uint32_t)min(max(e - 1, 0), last);
		const bool need = e < a.nblk + 4 && e < kParamEntries;
		wc[i] = __builtin_amdgcn_raw_buffer_load_b64(strs, need ? ((cur_bit + blk) >> 5) * 4 : kOOB, 0, 0);
		wu[i] = __builtin_amdgcn_raw_buffer_load_b64(strs_up, need ? ((up_bit + blk) >> 5) * 4 : kOOB, 0, 0);
	}
	const int tsegs = pd.rw_segs;
	const int ngroups = (tsegs + NU - 1) / NU;
	const uint8_t* sbase = a.listed ? ft.src[1][f] : a.src[1] + (uint64_t)f * pd.fpitch;
	const uint8_t* sbase2 = PLANAR ? (a.listed ? ft.src[2][f] : a.src[2] + (uint64_t)f * pd.fpitch) : nullptr;     // PLANAR: the Cr plane (sbase: the Cb plane)
	uint8_t* dbase = a.listed ? ft.dst[1][f] : a.dst[1] + (uint64_t)f * pd.dfpitch;
	// TOPL: the destination is planar; dbase is its Cb plane and dbase2 its Cr plane (semi-planar frames are listed, always: launch_args_ok)
	uint8_t* dbase2 = TOPL ? ft.dst[2][f] : nullptr;
	const uint32_t lane32 = (uint32_t)lane * kSpUnitBytes;
	constexpr uint32_t UBI = kMaxUnits * kSpUnitBytes;   // bytes of a position of an interleaved row
	constexpr uint32_t UB = PLANAR ? kMaxUnits * 16 : UBI;     // bytes of a position of the source (PLANAR: of each component's row)
	constexpr uint32_t GB = NU * UB;                     // ... of a group
	auto row_off = [&](int k) { return (uint32_t)((base + RSTR * k - prow0) * (int)pd.pitch); };
	auto left = [&](int g) { const uint32_t o = (uint32_t)g * GB; return o < pd.rowbytes ? min(pd.rowbytes - o, GB) : 0u; };
	// (only the narrowed destination has a geometry of its own -- run_plane_rw: a lane's two 8-byte planar halves interleave into ONE 16-byte unit of
	// Cb/Cr byte pairs, a wave access is 1 KiB)
	constexpr uint32_t UBD = OUT8 ? kMaxUnits * 16 : UBI, GBD = NU * UBD;
	auto row_offd = [&](int k) { return (uint32_t)((base + RSTR * k - prow0) * (int)pd.dpitch); };
	auto leftd = [&](int g) { const uint32_t o = (uint32_t)g * GBD, rb = PLANAR ? 2 * pd.drowbytes : pd.drowbytes; return o < rb ? min(rb - o, GBD) : 0u; };
	// (TOPL: a position of ONE component's destination row is 1 KiB, a lane's unit 16 bytes)
	constexpr uint32_t UBP = kMaxUnits * 16, GBP = NU * UBP;
	auto leftp = [&](int g) { const uint32_t o = (uint32_t)g * GBP; return o < pd.drowbytes ? min(pd.drowbytes - o, GBP) : 0u; };
	uint32_t w[NU][8];
	// (rs2: PLANAR only -- the Cr row; w[u][0..3] is the Cb unit and w[u][4..7] the Cr unit)
	auto load_pos = [&](const __amdgpu_buffer_rsrc_t rs, const __amdgpu_buffer_rsrc_t rs2, const int u) {
		const u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rs, PLANAR ? (uint32_t)lane * 16 + u * UB : lane32 + u * UB, 0, LDA);
		const u32x4 hi = PLANAR ? __builtin_amdgcn_raw_buffer_load_b128(rs2, (uint32_t)lane * 16 + u * UB, 0, LDA)
		                        : __builtin_amdgcn_raw_buffer_load_b128(rs, lane32 + u * UB + 16, 0, LDA);
		w[u][0] = lo.x; w[u][1] = lo.y; w[u][2] = lo.z; w[u][3] = lo.w;
		w[u][4] = hi.x; w[u][5] = hi.y; w[u][6] = hi.z; w[u][7] = hi.w;
	};
	// MIX: the luma over my UV units (row cy * SUBY of the frame's luma plane, the same byte offset in its row), in the ring with them
	const PlaneDesc& pl = a.pd[0];
	const uint8_t* lbase = MIX ? ft.src[0][f] : nullptr;
	auto lrow_off = [&](int k) { return (uint32_t)((base + RSTR * k) * SUBY * (int)pl.pitch); };     // (whole frames: the plane pointer addresses line 0)
	// (a luma row of whole blocks has the bytes of a UV row of whole blocks -- launch_depth refuses anything else -- so left() is what it has left too)
	uint32_t lw[MIX ? NU : 1][8];
	auto load_luma = [&](const __amdgpu_buffer_rsrc_t rs, const int u) {
		const u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rs, lane32 + u * UB, 0, 0);
		const u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(rs, lane32 + u * UB + 16, 0, 0);
		lw[u][0] = lo.x; lw[u][1] = lo.y; lw[u][2] = lo.z; lw[u][3] = lo.w;
		lw[u][4] = hi.x; lw[u][5] = hi.y; lw[u][6] = hi.z; lw[u][7] = hi.w;
	};
	{
		const __amdgpu_buffer_rsrc_t rs0 = make_rsrc(sbase + (k0 < k1 ? row_off(k0) : 0u), k0 < k1 ? left(0) : 0u);
		const __amdgpu_buffer_rsrc_t rs02 = PLANAR ? make_rsrc(sbase2 + (k0 < k1 ? row_off(k0) : 0u), k0 < k1 ? left(0) : 0u) : rs0;
#pragma unroll
		for (int u = 0; u < NU; u++) load_pos(rs0, rs02, u);
		if constexpr (MIX)
		{
			const __amdgpu_buffer_rsrc_t ls0 = make_rsrc(lbase + (k0 < k1 ? lrow_off(k0) : 0u), k0 < k1 ? left(0) : 0u);
#pragma unroll
			for (int u = 0; u < NU; u++) load_luma(ls0, u);
		}
	}
#pragma unroll
	for (int it = 0; it < NIT; it++)
		*(u32x4*)(lds + min((uint32_t)(threadIdx.x * 16 + it * STEP), (uint32_t)(IMG - 16))) = tmp[it];

	// ---- block parameters of the row, both components (once per workgroup) ---------------------------------------------
#pragma unroll
	for (int i = 0; i < NPE; i++)
	{
		if (i > 0 && i * kWavesPerWG * 64 >= a.nblk + 4) break;
		const int e = (int)threadIdx.x + i * kWavesPerWG * 64;
		const uint32_t blk = (uint32_t)min(max(e - 1, 0), last);
		const uint32_t vc = __builtin_amdgcn_alignbit(wc[i].y, wc[i].x, (cur_bit + blk) & 31);
		const uint32_t vu = __builtin_amdgcn_alignbit(wu[i].y, wu[i].x, (up_bit + blk) & 31);
#pragma unroll
		for (int c = 0; c < 2; c++)
		{
			const int fsx = c ? 20 : 10, fsy = c ? 4 : 24, fsb = c ? 15 : 2;      // vfgs_hw.c:99-138, components 1 and 2
			bool neg;
			const uint32_t pc = (block_param<2, SUBY, RS, SB>(vc, BANK_OFF, fsx, fsy, fsb, &neg) + ((ONE && neg) ? (uint32_t)NEG : 0u)) | (neg ? 0x80000000u : 0u);
			const uint32_t pu = block_param<2, SUBY, RS, SB>(vu, BANK_OFF, fsx, fsy, fsb, &neg) | (neg ? 0x80000000u : 0u);
			if (e < kParamEntries)
			{
				*(uint32_t*)(lds + PT + (2 * c) * kParamTableBytes + e * 4) = pc;
				*(uint32_t*)(lds + PT + (2 * c + 1) * kParamTableBytes + e * 4) = pu;
			}
		}
	}
	__syncthreads();
	if (k0 >= k1)
		return;

	// ---- per lane constants ------------------------------------------------------------------------------------------
	const uint32_t lo2 = MODELS ? mlo2 : a.lo2[1], hi2 = MODELS ? mhi2 : a.hi2[1];
	const uint32_t idx0 = (uint32_t)lane * M::BPL * 4;
	const int cl = lane * M::BPL - 1;
	auto lane_up = [](uint32_t old, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xf, 0xf, false); };    // wave_shr:1
	auto lane_down = [](uint32_t old, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x130, 0xf, 0xf, false); };  // wave_shl:1
	auto rot_up = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x13c, 0xf, 0xf, false); };      // wave_ror:1
	auto rot_down = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x134, 0xf, 0xf, false); };    // wave_rol:1
	// byte selectors of the split (a dword pair of the UV row -> one dword of Cb, one of Cr) and of the interleave (one of each -> the pair)
	constexpr uint32_t SPLIT_CB = SZ == 2 ? 0x05040100u : 0x06040200u, SPLIT_CR = SZ == 2 ? 0x07060302u : 0x07050301u;
	constexpr uint32_t JOIN_LO = SZ == 2 ? 0x05040100u : 0x05010400u, JOIN_HI = SZ == 2 ? 0x07060302u : 0x07030602u;

	// ---- the walk ----------------------------------------------------------------------------------------------------
	uint32_t carry[2][K];                  // in lane 0: the last K dwords of lane 63 of the previous position of the row, per component
	uint32_t outp[2][DW] = {};             // the previous position's planar units: dwords KD.. of its lanes' results
	uint32_t tp[2][KD] = {};               // ... and the first KD dwords its lanes computed: they belong one lane down
	uint32_t mcarry[2][K];                 // MIX: the carry of the index dwords
#pragma unroll
	for (int c = 0; c < 2; c++)
#pragma unroll
		for (int d = 0; d < K; d++) carry[c][d] = mcarry[c][d] = 0;
	// MIX: per component { luma_mult, chroma_mult, offset, active } (a component without a mix of its own keeps the sample as its index)
	// (each value a scalar register of its own: the eight come out of ONE scalar load, and kept as its 8-register tuple they would be spilled as
	// one -- to a stack slot, the only scratch of the kernel; grain_sp_mix_kernel below says what guards this and what to do when it stops working)
	auto own = [](int v) { if constexpr (MIX) asm("" : "+s"(v)); return v; };
	// (a model per frame: the values out of the frame's record, scalar bit-field extracts; KernelArgs::mix is not read)
	const bool rmix = MIX && MODELS == 2 && per_model;
	auto pick = [&](const int c, const int i) {
		if (!rmix) return a.mix[c][i];
		return i == 0 ? model_mix_luma_mult(mmix[c]) : (i == 1 ? model_mix_chroma_mult(mmix[c]) : (i == 2 ? model_mix_offset(mmix[c]) : model_mix_active(mmix[c])));
	};
	const int mix_lm[2] = {MIX ? own(pick(0, 0)) : 0, MIX ? own(pick(1, 0)) : 0}, mix_cm[2] = {MIX ? own(pick(0, 1)) : 0, MIX ? own(pick(1, 1)) : 0};
	const int mix_off[2] = {MIX ? own(pick(0, 2)) : 0, MIX ? own(pick(1, 2)) : 0};
	const bool mix_on[2] = {MIX && own(pick(0, 3)) != 0, MIX && own(pick(1, 3)) != 0};
	__amdgpu_buffer_rsrc_t pdst = make_rsrc(dbase, 0);
	// TOPL: where the previous group's last position goes is kept as the Cb row's address and what ONE component's row has left there; the two
	// descriptors are made at the store, the Cr row's from the distance between the two planes.  (Four descriptors kept across the walk are
	// sixteen scalar registers; spilled scalars take a vector register of the whole kernel, and the 8-bit general-form kernels have none to give.)
	uint8_t* pptr = dbase;
	uint32_t plen = 0;
	const ptrdiff_t cr_from_cb = TOPL ? dbase2 - dbase : 0;
	// the previous position is complete: interleave its two planar units, shift them up, store 32 bytes
	// (store_planar, TOPL only: a planar destination takes the two units as they are, low-aligned, 16 bytes to the Cb row and 16 to the Cr row;
	// `off` counts bytes of the interleaved row, a component's row has half of them)
	auto store_planar = [&](uint8_t* const cb, const uint32_t len, const uint32_t off) {
		if constexpr (TOPL)
		{
			// The two asm statements below STEER the register allocator, they force nothing, and they are fitted to one compiler's allocator: their
			// only guard is tests/test_code_object_sp_to_planar_cpu.py (no scratch, no spilled vector register in the 48 kernels).  If a new ROCm
			// makes that test fail, this is the place to revisit -- and if the plain form (voff = lane * 16, outp[] as the stores' data) then fits,
			// take it.
			// (the lane's offset in a component's row is half its offset in the interleaved row: made here, not kept beside lane32)
			uint32_t voff;
			asm volatile("v_lshrrev_b32 %0, 1, %1" : "=v"(voff) : "v"(lane32));
			// (real copies, as the interleave makes them: were outp[] itself the store's data, each unit would have to sit in four consecutive
			// registers from one position to the next, apart from the results it is refilled from -- eight registers the 8-bit general-form
			// kernels do not have)
			uint32_t st[2][4];
#pragma unroll
			for (int q = 0; q < 8; q++) asm volatile("v_mov_b32 %0, %1" : "=v"(st[q / 4][q % 4]) : "v"(outp[q / 4][q % 4]));
			store_unit<4, STA>(make_rsrc(cb, len), voff + off / 2, st[0]);
			store_unit<4, STA>(make_rsrc(cb + cr_from_cb, len), voff + off / 2, st[1]);
		}
	};
	auto store_prev = [&](const __amdgpu_buffer_rsrc_t rs, const uint32_t off) {
		if constexpr (OUT8)
		{
			// (bytes: Cb0 Cr0 Cb1 Cr1 | Cb2 Cr2 Cb3 Cr3 out of one dword of each component; 16 bytes = the lane's eight pairs, one vector store)
			uint32_t s8[4];
#pragma unroll
			for (int j = 0; j < 2; j++)
			{
				s8[2 * j] = __builtin_amdgcn_perm(outp[1][j], outp[0][j], 0x05010400u);
				s8[2 * j + 1] = __builtin_amdgcn_perm(outp[1][j], outp[0][j], 0x07030602u);
			}
			store_unit<4, STA>(rs, (uint32_t)lane * 16 + off, s8);
		}
		else
		{
			uint32_t st[8];
#pragma unroll
			for (int j = 0; j < 4; j++)
			{
				st[2 * j] = __builtin_amdgcn_perm(outp[1][j], outp[0][j], JOIN_LO);
				st[2 * j + 1] = __builtin_amdgcn_perm(outp[1][j], outp[0][j], JOIN_HI);
			}
			if constexpr (DEPTH > 8)
			{
#pragma unroll
				for (int j = 0; j < 8; j++) st[j] = pk_lshl_b16(a.sp_shift2, st[j]);
			}
			const uint32_t s0[4] = {st[0], st[1], st[2], st[3]}, s1[4] = {st[4], st[5], st[6], st[7]};
			store_unit<4, STA>(rs, lane32 + off, s0);
			store_unit<4, STA>(rs, lane32 + off + 16, s1);
		}
	};
	// OUT8: a component's results narrowed to 8 bit with the depth's rounding, four dwords -> two (run_plane_rw `results`)
	auto narrow = [](const uint32_t (&t)[4], uint32_t (&o)[2]) {
		uint32_t n[4];
#pragma unroll
		for (int d = 0; d < 4; d++) n[d] = ((t[d] + (0x00010001u << (DEPTH > 8 ? DEPTH - 9 : 0))) >> (DEPTH > 8 ? DEPTH - 8 : 0)) & 0x00ff00ffu;
		o[0] = __builtin_amdgcn_perm(n[1], n[0], 0x06040200);
		o[1] = __builtin_amdgcn_perm(n[3], n[2], 0x06040200);
	};
	auto walk_row = [&](auto overlap, const int k) {
		constexpr bool OV = decltype(overlap)::value;
		constexpr bool TP = TOPL;
		const int j = base + RSTR * k - Rabs * RPB;    // row inside the block row
		const int jrow = j * SUBY;
		const uint32_t rowoff = (uint32_t)j * RS, uprowoff = (uint32_t)(RPB + j) * RS;
		const int wc_ = jrow == 0 ? (SUBY > 1 ? 20 : 12) : 24, wu_ = jrow == 0 ? (SUBY > 1 ? 20 : 24) : 12;
		const uint32_t ro = row_off(k);
		// MIX: the row's last luma sample, low-aligned: the partner of every pair behind it (the lanes at the row's end only)
		uint32_t lw1 = 0;
		const uint32_t lro = MIX ? lrow_off(k) : 0u;
		if constexpr (MIX)
		{
			const __amdgpu_buffer_rsrc_t lrs = make_rsrc(lbase + lro, pl.rowbytes);
			const uint32_t at = (uint32_t)(a.mix_lw - 1) * SZ;
			if constexpr (SZ == 2) lw1 = (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(lrs, at, 0, 0) >> (a.sp_shift2 & 0xffffu);
			else lw1 = (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(lrs, at, 0, 0);
		}
		for (int g = 0; g < ngroups; g++)
		{
			const bool lastg = g + 1 == ngroups;
			const int ng = lastg ? 0 : g + 1;
			const bool nvalid = !lastg || k + 1 < k1;
			const uint32_t nso = nvalid ? (lastg ? row_off(k + 1) : ro) + (uint32_t)ng * GB : 0u;
			const __amdgpu_buffer_rsrc_t nsrc = make_rsrc(sbase + nso, nvalid ? left(ng) : 0u);
			const __amdgpu_buffer_rsrc_t nsrc2 = PLANAR ? make_rsrc(sbase2 + nso, nvalid ? left(ng) : 0u) : nsrc;
			const __amdgpu_buffer_rsrc_t nlsrc = make_rsrc(lbase + (MIX && nvalid ? (lastg ? lrow_off(k + 1) : lro) + (uint32_t)ng * GB : 0u), MIX && nvalid ? left(ng) : 0u);
			// (TP: this group of the Cb row, and what ONE component's row has left from there; no descriptor is kept)
			uint8_t* const cptr = TP ? dbase + (row_offd(k) + (uint32_t)g * GBP) : nullptr;
			const uint32_t clen = TP ? leftp(g) : 0u;
			const __amdgpu_buffer_rsrc_t cdst = TP ? pdst
			                                  : (DGEO ? make_rsrc(dbase + (row_offd(k) + (uint32_t)g * GBD), leftd(g)) : make_rsrc(dbase + (ro + (uint32_t)g * GB), left(g)));
			const uint8_t* pe = lds + idx0 + (uint32_t)(g * NU * BPS * 4);
			const int clg = cl + g * NU * BPS;
#pragma unroll
			for (int u = 0; u < NU; u++)
			{
				const bool firsts = u == 0 && g == 0;
				// my 32 bytes as a planar Cb unit and a planar Cr unit, low-aligned samples
				uint32_t cw[2][4];
				if constexpr (PLANAR)
				{
					// (the units as they were loaded; real copies, as in run_plane_rw: the refill below lands in w[u] itself)
#pragma unroll
					for (int q = 0; q < 8; q++) asm volatile("v_mov_b32 %0, %1" : "=v"(cw[q / 4][q % 4]) : "v"(w[u][q]));
				}
				else
				{
#pragma unroll
					for (int q = 0; q < 4; q++)
					{
						cw[0][q] = __builtin_amdgcn_perm(w[u][2 * q + 1], w[u][2 * q], SPLIT_CB);
						cw[1][q] = __builtin_amdgcn_perm(w[u][2 * q + 1], w[u][2 * q], SPLIT_CR);
					}
				}
				if constexpr (DEPTH > 8 && !PLANAR)
				{
#pragma unroll
					for (int c = 0; c < 2; c++)
#pragma unroll
						for (int q = 0; q < 4; q++) cw[c][q] = pk_lshr_b16(a.sp_shift2, cw[c][q]);
				}
				// MIX: the index dwords of my two planar units from ONE copy of the luma over them
				uint32_t mi[2][4] = {};
				if constexpr (MIX)
				{
					uint32_t l[8];
#pragma unroll
					for (int q = 0; q < 8; q++) l[q] = DEPTH > 8 ? pk_lshr_b16(a.sp_shift2, lw[u][q]) : lw[u][q];
					const int nv = a.mix_lw - 1 - (((NU * g + u) * 64 + lane) * NS * 2);
#pragma unroll
					for (int c = 0; c < 2; c++)
					{
						if (mix_on[c])
							mix_index<DEPTH, 2>(cw[c], l, mix_lm[c], mix_cm[c], mix_off[c], nv, lw1, mi[c]);
						else
						{
#pragma unroll
							for (int d = 0; d < 4; d++) mi[c][d] = cw[c][d];
						}
					}
				}
				// the registers are free: refill them with the position NU steps ahead
				load_pos(nsrc, nsrc2, u);
				if constexpr (MIX) load_luma(nlsrc, u);
				const bool live = NU * g + u < tsegs;
				bool edge_on[NE];
#pragma unroll
				for (int ed = 0; ed < NE; ed++) edge_on[ed] = (clg + u * BPS + ed >= 0) && (clg + u * BPS + ed < last);
				uint32_t res[2][4];
				uint32_t res8[2][OUT8 ? 2 : 1];      // OUT8: the component's results narrowed
#pragma unroll
				for (int c = 0; c < 2; c++)
				{
					// the component's tables: one-pattern form -- a sub-image of its own; general form -- its pair of tables in front of the shared bank
					const uint8_t* cl_ = lds + ((ONE && c) ? CIMG : 0);
					const uint32_t lutb = (ONE ? 0u : (uint32_t)(c * LUTB)) * 0x10001u;
					uint32_t (&t)[4] = res[c];
#pragma unroll
					for (int d = 0; d < K; d++) t[d] = lane_up(firsts ? 0u : carry[c][d], cw[c][4 - K + d]);
#pragma unroll
					for (int d = 0; d < K; d++) carry[c][d] = rot_up(cw[c][4 - K + d]);
#pragma unroll
					for (int d = K; d < 4; d++) t[d] = cw[c][d - K];
					// (the index dwords: the same lane shift and carry as the samples)
					uint32_t ti[4] = {};
					if constexpr (MIX)
					{
#pragma unroll
						for (int d = 0; d < K; d++) ti[d] = lane_up(firsts ? 0u : mcarry[c][d], mi[c][4 - K + d]);
#pragma unroll
						for (int d = 0; d < K; d++) mcarry[c][d] = rot_up(mi[c][4 - K + d]);
#pragma unroll
						for (int d = K; d < 4; d++) ti[d] = mi[c][d - K];
					}
					if (live)
					{
						RunParam<NR> rp, up;
#pragma unroll
						for (int rr = 0; rr < NR; rr++) rp.pa[rr] = *(const uint32_t*)(pe + PT + (2 * c) * kParamTableBytes + (u * BPS + rr) * 4);
#pragma unroll
						for (int rr = 0; rr < NR; rr++) up.pa[rr] = OV ? *(const uint32_t*)(pe + PT + (2 * c + 1) * kParamTableBytes + (u * BPS + rr) * 4) : 0u;
						if constexpr (MIX)
							grain_unit<DEPTH, BW, OV, ONE, ONE, NEG, true>(cl_, t, rp, up, lutb, rowoff, uprowoff, OV ? wc_ : 0, OV ? wu_ : 0, edge_on, false, lo2, hi2, MODELS ? mpk_shift : a.pk_shift, ti);
						else
							grain_unit<DEPTH, BW, OV, ONE, ONE, NEG>(cl_, t, rp, up, lutb, rowoff, uprowoff, OV ? wc_ : 0, OV ? wu_ : 0, edge_on, false, lo2, hi2, MODELS ? mpk_shift : a.pk_shift, t);
					}
					if constexpr (OUT8)
					{
						narrow(t, res8[c]);
#pragma unroll
						for (int d = 0; d < KD; d++) outp[c][DW - KD + d] = lane_down(rot_down(res8[c][d]), tp[c][d]);
					}
					else
					{
#pragma unroll
						for (int d = 0; d < K; d++) outp[c][4 - K + d] = lane_down(rot_down(t[d]), tp[c][d]);
					}
				}
				if constexpr (TP)
				{
					if (u == 0) store_planar(pptr, plen, (NU - 1) * UBD);
					else store_planar(cptr, clen, (u - 1) * UBD);
				}
				else
				{
					if (u == 0) store_prev(pdst, (NU - 1) * UBD);
					else store_prev(cdst, (u - 1) * UBD);
				}
#pragma unroll
				for (int c = 0; c < 2; c++)
				{
					if constexpr (OUT8)
					{
#pragma unroll
						for (int d = KD; d < DW; d++) outp[c][d - KD] = res8[c][d];
#pragma unroll
						for (int d = 0; d < KD; d++) tp[c][d] = res8[c][d];
					}
					else
					{
#pragma unroll
						for (int d = K; d < 4; d++) outp[c][d - K] = res[c][d];
#pragma unroll
						for (int d = 0; d < K; d++) tp[c][d] = res[c][d];
					}
				}
#if VFGS_SCHED_FENCE
				__builtin_amdgcn_sched_barrier(0);
#endif
			}
			pdst = cdst;
			if constexpr (TP) { pptr = cptr; plen = clen; }
		}
	};
	for (int k = k0; k < k1; k++)
	{
		const int jrow = (base + RSTR * k - Rabs * RPB) * SUBY;
		if (Rabs > 0 && jrow <= 1) walk_row(std::true_type(), k);      // blends in the block above (vfgs_hw.c:173-188, 223-229)
		else walk_row(std::false_type(), k);
	}
	// the last position of my last row
#pragma unroll
	for (int c = 0; c < 2; c++)
#pragma unroll
		for (int d = 0; d < KD; d++) outp[c][DW - KD + d] = lane_down(0u, tp[c][d]);
	if constexpr (TOPL) store_planar(pptr, plen, (NU - 1) * UBD);
	else store_prev(pdst, (NU - 1) * UBD);
}

// The kernels of semi-planar frames (KernelArgs::sp_kernel): the grid and the workgroup numbering of grain_rw_kernel with ONE UV workgroup where
// that has a Cb and a Cr workgroup.  kSpWgPerCU (vfgs_layout.h) workgroups per CU in every form: a UV wave keeps two components' walks alive.
// KernelArgs::sp_kernel == 3 (vfgs_hip_add_grain_sp_frame_list_to_planar_dev): the same kernels store planar pictures, decided at run time: the luma
// walk without a branch (run_plane_rw SP = 3), the UV walk once per workgroup between two instantiations (run_uv_sp TOPL); grain_spml_kernel below
// likewise.  Guard of the registers this was fitted into: tests/test_code_object_sp_to_planar_cpu.py.
template <int DEPTH, int CSUBY, bool ONEY, bool ONEC>
__global__ __launch_bounds__(kWavesPerWG * 64, kSpWgPerCU) void grain_sp_kernel(const KernelArgs a, const FrameTable ft)
{
	constexpr ImageLayout L = image_layout(2, CSUBY, ONEY, ONEC, DEPTH == 8);
	__shared__ __attribute__((aligned(16))) uint8_t lds[sp_lds_allocation(sp_lds_need(L.y_bytes, L.c_bytes, L.lut_bytes, ONEC))];

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = (int)(blockIdx.y << a.lfronts) + (int)(blockIdx.x & ((1u << a.lfronts) - 1));
	const int r = (int)(blockIdx.x >> a.lfronts);
	if (f >= a.nframes) return;
	if (r < a.pd[0].wgs)
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, ONEY, L.y_neg, 0, false, false, false, false, 3>(a, ft, a.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	else if (a.sp_kernel == 3)      // planes out (run_uv_sp TOPL): one branch per workgroup
		run_uv_sp<DEPTH, CSUBY, L.c_rs, L.c_bytes, L.c_bank, ONEC, L.c_neg, false, false, false, 0, true>(a, ft, lds, f, r - a.pd[0].wgs, L.c_off[0], lane, wave);
	else
		run_uv_sp<DEPTH, CSUBY, L.c_rs, L.c_bytes, L.c_bank, ONEC, L.c_neg>(a, ft, lds, f, r - a.pd[0].wgs, L.c_off[0], lane, wave);
}

// Semi-planar frames with A MODEL PER FRAME (KernelArgs::sp_kernel AND models_kernel; vfgs_hip_add_grain_sp_frame_list_models_dev):
// grain_sp_kernel's grid, numbering, launch bounds and LDS allocation; listed frames whose models share the form (ONEY, ONEC) of their images
// and nothing else.  A workgroup, luma or UV, stages ITS frame's tables and clips with ITS frame's bounds (run_plane_rw / run_uv_sp MODELS).
template <int DEPTH, int CSUBY, bool ONEY, bool ONEC>
__global__ __launch_bounds__(kWavesPerWG * 64, kSpWgPerCU) void grain_spml_kernel(const KernelArgs a, const FrameTable ft)
{
	constexpr ImageLayout L = image_layout(2, CSUBY, ONEY, ONEC, DEPTH == 8);
	__shared__ __attribute__((aligned(16))) uint8_t lds[sp_lds_allocation(sp_lds_need(L.y_bytes, L.c_bytes, L.lut_bytes, ONEC))];

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = (int)(blockIdx.y << a.lfronts) + (int)(blockIdx.x & ((1u << a.lfronts) - 1));
	const int r = (int)(blockIdx.x >> a.lfronts);
	if (f >= a.nframes) return;
	if (r < a.pd[0].wgs)
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, ONEY, L.y_neg, 0, false, false, false, false, 3, true>(a, ft, a.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	else if (a.sp_kernel == 3)      // planes out (run_uv_sp TOPL): one branch per workgroup
		run_uv_sp<DEPTH, CSUBY, L.c_rs, L.c_bytes, L.c_bank, ONEC, L.c_neg, false, false, false, true, true>(a, ft, lds, f, r - a.pd[0].wgs, L.c_off[0], lane, wave);
	else
		run_uv_sp<DEPTH, CSUBY, L.c_rs, L.c_bytes, L.c_bank, ONEC, L.c_neg, false, false, false, true>(a, ft, lds, f, r - a.pd[0].wgs, L.c_off[0], lane, wave);
}

// The kernels of semi-planar frames with a narrowed destination (KernelArgs::sp_kernel AND out8: P010 / P210 / P012 in, NV12 / NV16 out;
// vfgs_hip_add_grain_sp_frame_list_copy8_dev): grain_sp_kernel's grid, numbering and residency.  Luma workgroups narrow their results like
// every OUT8 plane; a UV workgroup narrows each component's planar unit to 8 bytes, rotates the halves back and interleaves them into ONE 16-byte unit
// of Cb/Cr byte pairs.  The destination has a geometry of its own (PlaneDesc::dpitch, drowbytes: bytes); nothing is ever in place.
template <int DEPTH, int CSUBY, bool ONEY, bool ONEC>
__global__ __launch_bounds__(kWavesPerWG * 64, kSpWgPerCU) void grain_sp8_kernel(const KernelArgs a, const FrameTable ft)
{
	static_assert(DEPTH > 8, "the narrowed destination exists for 16-bit containers");
	constexpr ImageLayout L = image_layout(2, CSUBY, ONEY, ONEC, false);
	__shared__ __attribute__((aligned(16))) uint8_t lds[sp_lds_allocation(sp_lds_need(L.y_bytes, L.c_bytes, L.lut_bytes, ONEC))];

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = (int)(blockIdx.y << a.lfronts) + (int)(blockIdx.x & ((1u << a.lfronts) - 1));
	const int r = (int)(blockIdx.x >> a.lfronts);
	if (f >= a.nframes) return;
	// (a model per frame -- KernelArgs::models_kernel; vfgs_hip_add_grain_sp_frame_list_models_copy8_dev -- is decided at run time in both walks: MODELS = 2)
	if (r < a.pd[0].wgs)
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, ONEY, L.y_neg, 0, true, false, false, false, true, 2>(a, ft, a.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	else
		run_uv_sp<DEPTH, CSUBY, L.c_rs, L.c_bytes, L.c_bank, ONEC, L.c_neg, false, true, false, 2>(a, ft, lds, f, r - a.pd[0].wgs, L.c_off[0], lane, wave);
}

// The kernels of a PLANAR source with a semi-planar destination (KernelArgs::sp_kernel == 2; vfgs_hip_add_grain_frame_list_to_sp_dev):
// what a software decoder hands out (yuv420p, yuv420p10le, yuv422p10le ...) goes to the surface a display or a hardware encoder takes (NV12, P010 ...)
// in one pass.  grain_sp_kernel's grid, numbering, table staging and residency.  Luma workgroups read the low-aligned source as it lies and store
// the results shifted up by sp_shift2 at the destination's own pitch; a UV workgroup loads its Cb unit and its Cr unit from the two planar rows
// (run_uv_sp PLANAR) and stores them interleaved.  Nothing is ever in place.
template <int DEPTH, int CSUBY, bool ONEY, bool ONEC>
__global__ __launch_bounds__(kWavesPerWG * 64, kSpWgPerCU) void grain_p2sp_kernel(const KernelArgs a, const FrameTable ft)
{
	constexpr ImageLayout L = image_layout(2, CSUBY, ONEY, ONEC, DEPTH == 8);
	__shared__ __attribute__((aligned(16))) uint8_t lds[sp_lds_allocation(sp_lds_need(L.y_bytes, L.c_bytes, L.lut_bytes, ONEC))];

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = (int)(blockIdx.y << a.lfronts) + (int)(blockIdx.x & ((1u << a.lfronts) - 1));
	const int r = (int)(blockIdx.x >> a.lfronts);
	if (f >= a.nframes) return;
	// (the frames are listed, always -- launch_depth refuses anything else -- and saying so here takes the plane pointers of the arguments out of both
	// walks: kept, their 8-register tuple is live across the UV walk beside the second set of descriptors, gets a stack slot and with it scratch memory
	// for every dispatch; `b` is a copy in registers, never in memory.  Guard: tests/test_code_object_p2sp_cpu.py, private_segment_fixed_size == 0)
	KernelArgs b = a;
	b.listed = 1;
	// (a model per frame -- KernelArgs::models_kernel; vfgs_hip_add_grain_frame_list_models_to_sp_dev, DESIGN.md 4.8 -- is decided at run time in both walks:
	// MODELS = 2, a wave-uniform branch around the scalar loads of the frame's record; the guard above holds for it too)
	if (r < b.pd[0].wgs)
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, ONEY, L.y_neg, 0, false, false, false, false, 2, 2>(b, ft, b.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	else
		run_uv_sp<DEPTH, CSUBY, L.c_rs, L.c_bytes, L.c_bank, ONEC, L.c_neg, false, false, true, 2>(b, ft, lds, f, r - b.pd[0].wgs, L.c_off[0], lane, wave);
}

// ... with the narrowed 8-bit destination (KernelArgs::sp_kernel == 2 AND out8: planar 10 / 12 bit in, NV12 / NV16 out;
// vfgs_hip_add_grain_frame_list_to_sp8_dev): grain_sp8_kernel's stores behind the planar loads.
template <int DEPTH, int CSUBY, bool ONEY, bool ONEC>
__global__ __launch_bounds__(kWavesPerWG * 64, kSpWgPerCU) void grain_p2sp8_kernel(const KernelArgs a, const FrameTable ft)
{
	static_assert(DEPTH > 8, "the narrowed destination exists for 16-bit containers");
	constexpr ImageLayout L = image_layout(2, CSUBY, ONEY, ONEC, false);
	__shared__ __attribute__((aligned(16))) uint8_t lds[sp_lds_allocation(sp_lds_need(L.y_bytes, L.c_bytes, L.lut_bytes, ONEC))];

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = (int)(blockIdx.y << a.lfronts) + (int)(blockIdx.x & ((1u << a.lfronts) - 1));
	const int r = (int)(blockIdx.x >> a.lfronts);
	if (f >= a.nframes) return;
	KernelArgs b = a;
	b.listed = 1;      // (as in grain_p2sp_kernel; a model per frame, vfgs_hip_add_grain_frame_list_models_to_sp8_dev, likewise: MODELS = 2 in both walks)
	if (r < b.pd[0].wgs)
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, ONEY, L.y_neg, 0, true, false, false, false, 2, 2>(b, ft, b.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	else
		run_uv_sp<DEPTH, CSUBY, L.c_rs, L.c_bytes, L.c_bank, ONEC, L.c_neg, false, true, true, 2>(b, ft, lds, f, r - b.pd[0].wgs, L.c_off[0], lane, wave);
}

// The kernels of semi-planar frames under the luma / chroma mix (KernelArgs::sp_kernel AND mix_kernel): all-one-pattern images
// only, depths 8 and 10, the grid and the workgroup numbering of grain_sp_kernel.  Luma workgroups are grain_sp_kernel's; a UV workgroup holds
// the luma over its units in its ring and forms both components' index dwords from it.  KernelArgs::mix_planes switches the workgroups of one
// plane type off, as in grain_mix_kernel: a call whose destination luma shares bytes with its source luma is two launches on its stream, UV
// first.  kSpMixWgPerCU workgroups per CU: launch bounds and LDS allocation say the same (vfgs_layout.h).
template <int DEPTH, int CSUBY>
__global__ __launch_bounds__(kWavesPerWG * 64, kSpMixWgPerCU) void grain_sp_mix_kernel(const KernelArgs a, const FrameTable ft)
{
	constexpr ImageLayout L = image_layout(2, CSUBY, true, true, DEPTH == 8);
	__shared__ __attribute__((aligned(16))) uint8_t lds[sp_mix_lds_allocation(sp_lds_need(L.y_bytes, L.c_bytes, L.lut_bytes, true))];

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = (int)(blockIdx.y << a.lfronts) + (int)(blockIdx.x & ((1u << a.lfronts) - 1));
	const int r = (int)(blockIdx.x >> a.lfronts);
	const bool luma = r < a.pd[0].wgs;
	if (f >= a.nframes || (a.mix_planes & (luma ? 1 : 2))) return;
	// (these eight arguments arrive with ONE scalar load and both walks read them: each in a scalar register of its own from here on.  Kept as
	// the load's 8-register tuple across the UV walk, the register allocator gives the tuple a stack slot and then reloads it from the
	// arguments instead -- the slot stays in the kernel's frame, unused, and every dispatch would get scratch memory for it)
	// This steers the register allocator, it forces nothing, and it depends on the compiler: its ONLY guard is tests/test_code_object_sp_mix_cpu.py
	// (private_segment_fixed_size == 0).  If a new ROCm makes that test fail: compile with -Rpass-analysis=stack-frame-layout, which names the
	// size of the slot ("Type: Spill, Size: 32" is an 8-register tuple, 16 a 4-register one); find the scalar load of that width that is issued
	// twice from the same argument offset in the kernel's assembly (`b` below is a copy in registers, never in memory: it costs nothing); add the
	// fields at that offset to the list below -- or, if that no longer helps, lower the scalar pressure of the UV walk.  Never accept the scratch.
	KernelArgs b = a;
	auto own = [](auto& v) { asm("" : "+s"(v)); };
	own(b.cur_bit0); own(b.up_bit0); own(b.frame_bit_step); own(b.y0); own(b.nblk); own(b.nbrows); own(b.nframes); own(b.listed);
	// (the same for the four of the luma geometry that arrive with pd[0].wgs above)
	own(b.pd[0].nrows); own(b.pd[0].wgs); own(b.pd[0].rw_segs); own(b.pd[0].rw_rpw);
	// (a model per frame -- KernelArgs::models_kernel beside mix_kernel -- is decided at run time in both walks, as in grain_mix_kernel: MODELS = 2)
	if (luma)
		run_plane_rw<DEPTH, 16, 1, 1, L.y_rs, L.y_bytes, true, L.y_neg, 0, false, false, false, false, true, 2>(b, ft, b.pd[0], lds, 0, f, r, L.y_off, L.y_bank, 0, lane, wave);
	else
		run_uv_sp<DEPTH, CSUBY, L.c_rs, L.c_bytes, L.c_bank, true, L.c_neg, true, false, false, 2>(b, ft, lds, f, r - b.pd[0].wgs, L.c_off[0], lane, wave);
}

// ---------------------------------------------------------------------------------------
// host-side launcher (called from vfgs_host.cpp)

// What a launch's arguments must say for the kernel of key `k` (vfgs_layout.h KernelKey) to be the one that serves them; WHICH kernels exist
// is not decided here (kernel_exists, at the leaf of the dispatch below).  The host refuses all of this before it gets here.
static bool launch_args_ok(const KernelArgs& a, const FrameTable* list, const KernelKey& k)
{
	const Family f = k.family;
	// (the two families of the mix serve a model per frame too -- models that carry a mix -- with the kernels that decide it at run time: neither
	// the narrowed destination nor rows walked in parts)
	const bool mix_models = (f == Family::mix || f == Family::sp_mix) && a.models_kernel != 0;
	if (mix_models && (k.out8 || k.wide)) return false;
	// (so do the narrowed kernels of ordinary rows without persistence: grain_rw_kernel<.., out8, .., !wide, !persist> and grain_sp8_kernel)
	const bool out8_models = (f == Family::rw || f == Family::sp8) && a.models_kernel != 0;
	if (out8_models && !(k.out8 && !k.wide && !k.persist)) return false;
	// (and every kernel of a planar source with a semi-planar destination: listed frames with a 16-byte-aligned model image each, held to that below)
	const bool p2sp_models = (f == Family::p2sp || f == Family::p2sp8) && a.models_kernel != 0;
	// (a surface in, planes out: the kernels of sp / spml alone decide that at run time)
	const bool to_planar = a.sp_kernel == 3;
	if (to_planar && f != Family::sp && f != Family::spml) return false;
	const FamilyFields ff = family_fields(f, mix_models || out8_models || p2sp_models, to_planar);
	if (a.models_kernel != ff.models_kernel || a.mix_kernel != ff.mix_kernel || a.sp_kernel != ff.sp_kernel) return false;
	if (k.wide != (a.nblk > kTileBlocks)) return false;
	if (a.mix_kernel ? (a.mix_lw < 1 || a.mix_lw > a.nblk * kBlock) : a.mix_planes != 0) return false;
	if ((a.listed != 0) != (list != nullptr) || (list && a.nframes > kListFrames)) return false;
	// the phase between two frame fronts: grain_rw_kernel's alone, a rotation inside the frame's tasks
	if (a.front_shift != 0 && (f != Family::rw || k.persist || a.lfronts != 1 || a.front_shift < 0 || a.front_shift >= a.pd[0].wgs + 2 * a.pd[1].wgs)) return false;
	if (a.models_kernel)
	{
		// a model per frame: listed frames, every frame with a model image
		if (!list) return false;
		for (int i = 0; i < a.nframes; i++)
			if (!list->model[i] || ((uintptr_t)list->model[i] & 15)) return false;
	}
	if (family_semiplanar(f))
	{
		// listed whole frames; 16-bit containers: the samples sit the same number of bits up in both halves of a dword
		if (!list || a.y0 != 0) return false;
		if (k.depth == 8 ? a.sp_shift2 != 0 : (a.sp_shift2 >> 16) != (a.sp_shift2 & 0xffffu)) return false;
	}
	const bool planar_src = f == Family::p2sp || f == Family::p2sp8;
	if (planar_src || f == Family::sp8)
	{
		// a destination with a geometry of its own: its rows have the source rows' containers (narrowed: as bytes), in whole dwords; a planar
		// source: pd[1] holds ONE component's bytes of a source row and of a destination row, half a luma row's
		const uint32_t div = k.out8 ? 2 : 1;
		if (a.pd[1].drowbytes * div != a.pd[1].rowbytes || a.pd[0].drowbytes * div != a.pd[0].rowbytes) return false;
		if (planar_src && a.pd[0].rowbytes != 2 * a.pd[1].rowbytes) return false;
	}
	if (f == Family::sp_mix && a.pd[0].rowbytes != a.pd[1].rowbytes) return false;
	if (to_planar)
	{
		// a planar destination's own geometry: a luma row of the source's bytes, ONE component's half of a UV row's, pitches that hold them in
		// whole 16-byte units, three planes a frame
		if (a.pd[0].drowbytes != a.pd[0].rowbytes || 2 * a.pd[1].drowbytes != a.pd[1].rowbytes) return false;
		if (a.pd[0].dpitch < a.pd[0].drowbytes || a.pd[1].dpitch < a.pd[1].drowbytes || ((a.pd[0].dpitch | a.pd[1].dpitch) & 15)) return false;
		for (int i = 0; i < a.nframes; i++)
			if (!list->dst[0][i] || !list->dst[1][i] || !list->dst[2][i] || list->dst[1][i] == list->dst[2][i]) return false;
	}
	// (the luma walk of the two families always stores through the destination's geometry: for a surface it is the source's)
	else if ((f == Family::sp || f == Family::spml) && (a.pd[0].dpitch != a.pd[0].pitch || a.pd[0].drowbytes != a.pd[0].rowbytes)) return false;
	return true;
}

// grid: x = (workgroup inside the frame, frame of a group of 2^lfronts frames), y = group of frames; persist: a.persist_wgs luma workgroups
// share the launch's luma tasks and `grid` = persist_wgs + all chroma tasks, else `grid` = workgroups per frame
static dim3 grid_of(const KernelArgs& a, bool persist, int grid)
{
	return persist ? dim3((unsigned)grid) : dim3((unsigned)grid << a.lfronts, ((unsigned)a.nframes + (1u << a.lfronts) - 1) >> a.lfronts);
}

// The one kernel of a key, or none: the instantiations of a code object are the keys of its depth that kernel_exists() holds, no more, no fewer
// (tests/test_kernel_keys_cpu.py).
template <int D, int X, int Y, bool OUT8, bool ONEY, bool ONEC, bool WIDE, bool PERSIST, Family F>
static hipError_t launch_key(const KernelArgs& a, const FrameTable& ft, const dim3 g, hipStream_t stream)
{
	if constexpr (kernel_exists(KernelKey{D, X, Y, OUT8, ONEY, ONEC, WIDE, PERSIST, F}))
	{
		const dim3 b(kWavesPerWG * 64);
		if constexpr (F == Family::rw) hipLaunchKernelGGL((grain_rw_kernel<D, X, Y, OUT8, ONEY, ONEC, WIDE, PERSIST>), g, b, 0, stream, a, ft);
		else if constexpr (F == Family::ml) hipLaunchKernelGGL((grain_ml_kernel<D, X, Y, ONEY, ONEC>), g, b, 0, stream, a, ft);
		else if constexpr (F == Family::mix) hipLaunchKernelGGL((grain_mix_kernel<D, X, Y, OUT8, WIDE>), g, b, 0, stream, a, ft);
		else if constexpr (F == Family::sp) hipLaunchKernelGGL((grain_sp_kernel<D, Y, ONEY, ONEC>), g, b, 0, stream, a, ft);
		else if constexpr (F == Family::spml) hipLaunchKernelGGL((grain_spml_kernel<D, Y, ONEY, ONEC>), g, b, 0, stream, a, ft);
		else if constexpr (F == Family::sp8) hipLaunchKernelGGL((grain_sp8_kernel<D, Y, ONEY, ONEC>), g, b, 0, stream, a, ft);
		else if constexpr (F == Family::p2sp) hipLaunchKernelGGL((grain_p2sp_kernel<D, Y, ONEY, ONEC>), g, b, 0, stream, a, ft);
		else if constexpr (F == Family::p2sp8) hipLaunchKernelGGL((grain_p2sp8_kernel<D, Y, ONEY, ONEC>), g, b, 0, stream, a, ft);
		else hipLaunchKernelGGL((grain_sp_mix_kernel<D, Y>), g, b, 0, stream, a, ft);
		return hipGetLastError();
	}
	else
		return hipErrorInvalidValue;
}

// run-time selectors -> template arguments: fn(std::bool_constant<v>{}...) for the values `v...`, one branch each
template <bool... Bs, class Fn>
static hipError_t lift_bools(Fn&& fn) { return fn(std::bool_constant<Bs>{}...); }
template <bool... Bs, class Fn, class... Rest>
static hipError_t lift_bools(Fn&& fn, bool v, Rest... rest) { return v ? lift_bools<Bs..., true>(fn, rest...) : lift_bools<Bs..., false>(fn, rest...); }

template <class Fn>
static hipError_t lift_family(Family f, Fn&& fn)
{
	switch (f)
	{
	case Family::rw: return fn(std::integral_constant<Family, Family::rw>{});
	case Family::ml: return fn(std::integral_constant<Family, Family::ml>{});
	case Family::mix: return fn(std::integral_constant<Family, Family::mix>{});
	case Family::sp: return fn(std::integral_constant<Family, Family::sp>{});
	case Family::spml: return fn(std::integral_constant<Family, Family::spml>{});
	case Family::sp8: return fn(std::integral_constant<Family, Family::sp8>{});
	case Family::p2sp: return fn(std::integral_constant<Family, Family::p2sp>{});
	case Family::p2sp8: return fn(std::integral_constant<Family, Family::p2sp8>{});
	case Family::sp_mix: return fn(std::integral_constant<Family, Family::sp_mix>{});
	}
	return hipErrorInvalidValue;     // (not a Family)
}

// The product compiles this file THREE times (versatilefilmgrain_amd/build.py: -DVFGS_KERNEL_DEPTH=10, =8 and =12), side by side: one code object per
// sample depth; the 12-bit one holds the 10-bit one's row-walk kernels (same forms, same residency) and no mix kernels.  That halves the build (110 -> 60 s) and keeps the other depth's kernels off the device; it does NOT buy the
// start-up time round 5 hoped for: a code object's first launch costs 1.3 ms (profiles/r06_startup_probe_two_code_objects.jsonl), so the 15 ms
// of a process's first grain launch are the allocations and first transfers around it, not the 88 kernels.  Without the macro (the assembly
// listings) everything is one translation unit.
template <int D>
static hipError_t launch_depth(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream)
{
	if (k.depth != D || (k.csubx != 1 && k.csubx != 2) || (k.csuby != 1 && k.csuby != 2) || !launch_args_ok(a, list, k)) return hipErrorInvalidValue;
	static const FrameTable no_list{};
	const FrameTable& ft = list ? *list : no_list;
	const dim3 g = grid_of(a, k.persist, grid);
	return lift_family(k.family, [&](auto F) {
		return lift_bools([&](auto X2, auto Y2, auto OUT8, auto ONEY, auto ONEC, auto WIDE, auto PERSIST) {
			return launch_key<D, X2() ? 2 : 1, Y2() ? 2 : 1, OUT8(), ONEY(), ONEC(), WIDE(), PERSIST(), decltype(F)::value>(a, ft, g, stream);
		}, k.csubx == 2, k.csuby == 2, k.out8, k.oney, k.onec, k.wide, k.persist);
	});
}

#if !defined(VFGS_KERNEL_DEPTH) || VFGS_KERNEL_DEPTH == 8
hipError_t launch_grain_d8(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream) { return launch_depth<8>(a, list, k, grid, stream); }
#else
hipError_t launch_grain_d8(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream);
#endif

#if !defined(VFGS_KERNEL_DEPTH) || VFGS_KERNEL_DEPTH == 12
hipError_t launch_grain_d12(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream) { return launch_depth<12>(a, list, k, grid, stream); }
#else
hipError_t launch_grain_d12(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream);
#endif

#if !defined(VFGS_KERNEL_DEPTH) || VFGS_KERNEL_DEPTH == 10
hipError_t launch_grain(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream)
{
	if (k.depth == 10) return launch_depth<10>(a, list, k, grid, stream);
	if (k.depth == 8) return launch_grain_d8(a, list, k, grid, stream);
	return launch_grain_d12(a, list, k, grid, stream);
}

// the name of the kernel launch_grain() dispatches for a key, as the launch record states it (vfgs_hip_last_launch_info)
void name_launch(const KernelKey& k, char* out, size_t n) { kernel_name(k, out, n); }

ImageLayout layout_of(int csubx, int csuby, bool oney, bool onec, bool depth8) { return image_layout(csubx, csuby, oney, onec, depth8); }
#endif

}  // namespace vfgs
