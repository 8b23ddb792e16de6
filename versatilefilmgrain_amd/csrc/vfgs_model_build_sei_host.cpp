// Firmware layer, host part: film grain models straight from FGC SEI messages (vfgs_hip_models_from_sei, include/vfgs_hip_fw.h).
//
// What vfgs_init_sei derives and hands to the hardware layer -- the lists of distinct patterns, their cut-offs or taps, scale and
// pattern LUTs, the shift -- goes into one job per message here (vfgs_fw_sei.h states the derivation for both), and the jobs of a call
// go to the model bookkeeping in vfgs_host.cpp (build_models_sei) together with the launcher of fw_sei_build_kernel, which that file
// does not name: this is the one host file that needs that entry of vfgs_fw_kernel.hip at link time.
// Where vfgs_init_sei aborts or reads past the message (a bitstream can carry it), this call refuses.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vfgs_hip.h"
#include "../../include/vfgs_hip_fw.h"
#include "vfgs_fw_sei.h"
#include "vfgs_model_build.h"

namespace {

const char* const kWho = "vfgs_hip_models_from_sei";

int refuse(int code, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	return vfgs::set_error(code, buf);
}

// what a message is refused for before anything is derived from it; 0, or the refusal (i: its index in the call, for the message)
int check_sei(const fgs_sei& m, unsigned i)
{
	for (int c = 0; c < 3; c++)
		if (m.comp_model_present_flag[c] && m.num_intensity_intervals[c] > 256)
			return refuse(42, "%s: message %u: component %d has %d intensity intervals (the message holds 256)", kWho, i, c, m.num_intensity_intervals[c]);
	if (m.model_id && (m.log2_scale_factor < 1 || m.log2_scale_factor > 15))
		return refuse(42, "%s: message %u: log2_scale_factor %d with the auto-regressive model (1..15)", kWho, i, m.log2_scale_factor);
	return 0;
}

// the slot a pattern LUT selects for every intensity, or -1 (uniform_slot of vfgs_host.cpp)
int uniform_slot(const uint8_t (&plut)[256])
{
	const int k = plut[0] >> 4;
	for (int i = 1; i < 256; i++)
		if ((plut[i] >> 4) != k) return -1;
	return k;
}

// one message -> the message side of its job, in vfgs_init_sei's order
void job_from_sei(const fgs_sei& m, vfgs::FwSeiJob& j)
{
	memset(&j, 0, sizeof j);
	vfgs::PatternList luma, chroma;
	if (m.comp_model_present_flag[0])
		vfgs::collect_patterns(&m, 0, luma);
	vfgs::sei_fill_luts(&m, luma, 0, j.slut[0], j.plut[0]);     // (slut[0] starts cleared)
	// Cb and Cr share one bank and one list (vfgs_fw.c:533-538)
	for (int c = 1; c < 3; c++)
		if (m.comp_model_present_flag[c])
			vfgs::collect_patterns(&m, c, chroma);
	// QUIRK: one scale table is cleared before Cb and NOT between Cb and Cr (vfgs_fw.c:530, :598-643)
	vfgs::sei_fill_luts(&m, chroma, 1, j.slut[1], j.plut[1]);
	memcpy(j.slut[2], j.slut[1], 256);
	vfgs::sei_fill_luts(&m, chroma, 2, j.slut[2], j.plut[2]);
	j.kind = m.model_id ? 1 : 0;
	j.ar_scale = m.log2_scale_factor;
	j.np_luma = luma.n;
	j.np_chroma = chroma.n;
	for (int pt = 0; pt < 2; pt++)
	{
		const vfgs::PatternList& pl = pt ? chroma : luma;
		for (int i = 0; i < pl.n; i++)
		{
			const int16_t* v = &m.comp_model_value[0][0][0] + pl.flat[i];
			int16_t* p = j.pat[8 * pt + i];
			if (j.kind) vfgs::sei_ar_taps(v, j.ar_scale, p);
			else { p[0] = v[1]; p[1] = v[2]; }
		}
	}
	for (int c = 0; c < 3; c++) j.slot[c] = uniform_slot(j.plut[c]);
	j.scale_shift = m.log2_scale_factor - (m.model_id ? 1 : 0);     // vfgs_fw.c:644: the argument of vfgs_set_scale_shift; build_models_sei checks and stores it
}

}  // namespace

extern "C" int vfgs_hip_models_from_sei(const fgs_sei* cfgs, unsigned n, vfgs_hip_model** out, void* stream)
{
	if (n == 0) return 0;
	if (!out) return refuse(41, "%s: null result pointer for %u models", kWho, n);
	for (unsigned i = 0; i < n; i++) out[i] = nullptr;
	if (!cfgs) return refuse(41, "%s: null messages for %u models", kWho, n);
	for (unsigned i = 0; i < n; i++)
		if (int e = check_sei(cfgs[i], i)) return e;
	std::vector<vfgs::FwSeiJob> jobs(n);
	for (unsigned i = 0; i < n; i++) job_from_sei(cfgs[i], jobs[i]);
	return vfgs::build_models_sei(kWho, jobs.data(), n, out, stream, &vfgs::launch_fw_sei_build);
}
