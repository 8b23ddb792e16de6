// TEST INFRASTRUCTURE -- the product's host firmware (versatilefilmgrain_amd/csrc/vfgs_fw_host.cpp) under a recording hardware layer.
//
// vfgs_fw_host.cpp is a pure client of the hardware-layer interface (include/vfgs_hip.h).  This stand-alone program is linked with it and
// with the stubs below, which record what it calls: the nine setters, the jobs given to vfgs_hip_generate_patterns, and the chroma-mix
// calls.  No GPU, no reference.  tests/test_fw_host_records_cpu.py compiles and runs it.
//
//   fw_host_records <in> <out>
//   in  : per parameter set  u32 kind (0: fgs_sei, 1: fgs_afgs1), the C bytes of the structure
//   out : per parameter set  records in the layout of oracle/trace_shim.c -- u32 op, i32 a, i32 b, u32 nbytes, payload -- closed by op 199:
//           1..9  the setters, as trace_shim.c numbers them
//           100   one pattern job of a vfgs_hip_generate_patterns call: a = its position in the call, b = the call's job count,
//                 payload = the vfgs_hip_pattern_job
//           101   vfgs_hip_clear_chroma_mix
//           102   vfgs_hip_set_chroma_mix: a = component, payload = luma_mult, chroma_mult, offset (3 x i32)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/vfgs_hip.h"
#include "../../include/vfgs_hip_fw.h"

namespace {

FILE* g_out;

void rec(uint32_t op, int32_t a, int32_t b, const void* payload, uint32_t n)
{
	fwrite(&op, 4, 1, g_out);
	fwrite(&a, 4, 1, g_out);
	fwrite(&b, 4, 1, g_out);
	fwrite(&n, 4, 1, g_out);
	if (n) fwrite(payload, 1, n, g_out);
}

}  // namespace

extern "C" {

void vfgs_set_luma_pattern(int index, signed char* P)   { rec(1, index, 0, P, 4096); }
void vfgs_set_chroma_pattern(int index, signed char* P) { rec(2, index, 0, P, 4096); }
void vfgs_set_scale_lut(int c, unsigned char lut[])     { rec(3, c, 0, lut, 256); }
void vfgs_set_pattern_lut(int c, unsigned char lut[])   { rec(4, c, 0, lut, 256); }
void vfgs_set_seed(unsigned int seed)                   { rec(5, (int32_t)seed, 0, nullptr, 0); }
void vfgs_set_scale_shift(int shift)                    { rec(6, shift, 0, nullptr, 0); }
void vfgs_set_depth(int depth)                          { rec(7, depth, 0, nullptr, 0); }
void vfgs_set_legal_range(int legal)                    { rec(8, legal, 0, nullptr, 0); }
void vfgs_set_chroma_subsampling(int subx, int suby)    { rec(9, subx, suby, nullptr, 0); }

int vfgs_hip_generate_patterns(const vfgs_hip_pattern_job* jobs, int n)
{
	for (int i = 0; i < n; i++) rec(100, i, n, &jobs[i], sizeof jobs[i]);
	return 0;
}

void vfgs_hip_clear_chroma_mix(void) { rec(101, 0, 0, nullptr, 0); }

int vfgs_hip_set_chroma_mix(int c, int luma_mult, int chroma_mult, int offset)
{
	const int32_t v[3] = {luma_mult, chroma_mult, offset};
	rec(102, c, 0, v, sizeof v);
	return 0;
}

const char* vfgs_hip_last_error_string(void) { return ""; }

}  // extern "C"

int main(int argc, char** argv)
{
	if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
	FILE* in = fopen(argv[1], "rb");
	g_out = fopen(argv[2], "wb");
	if (!in || !g_out) { perror("fw_host_records"); return 2; }
	uint32_t kind;
	int n = 0;
	while (fread(&kind, 4, 1, in) == 1)
	{
		if (kind == 0)
		{
			std::vector<fgs_sei> s(1);
			if (fread(s.data(), sizeof(fgs_sei), 1, in) != 1) { fprintf(stderr, "set %d: short fgs_sei\n", n); return 2; }
			vfgs_init_sei(s.data());
		}
		else if (kind == 1)
		{
			fgs_afgs1 a;
			if (fread(&a, sizeof a, 1, in) != 1) { fprintf(stderr, "set %d: short fgs_afgs1\n", n); return 2; }
			vfgs_init_afgs1(&a);
		}
		else { fprintf(stderr, "set %d: kind %u\n", n, kind); return 2; }
		rec(199, n++, 0, nullptr, 0);
	}
	fclose(in);
	if (fclose(g_out)) { perror(argv[2]); return 2; }
	return 0;
}
