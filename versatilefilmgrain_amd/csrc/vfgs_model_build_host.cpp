// Firmware layer, host part: film grain models straight from AFGS1 parameter sets (vfgs_hip_models_from_afgs1, include/vfgs_hip_fw.h).
//
// What vfgs_init_afgs1 derives and hands to the hardware layer's setters -- scale LUTs, taps, shifts, range -- goes into one job per
// parameter set here, and the jobs of a call go to the model bookkeeping in vfgs_host.cpp (build_models) together with the launcher of
// fw_models_kernel, which that file does not name: this is the one host file that needs vfgs_fw_kernel.hip's new entry at link time.
// Where vfgs_init_afgs1 aborts on a parameter set (a bitstream can carry it), this call refuses.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vfgs_hip.h"
#include "../../include/vfgs_hip_fw.h"
#include "vfgs_fw_afgs1.h"
#include "vfgs_model_build.h"

namespace {

const char* const kWhoPlain = "vfgs_hip_models_from_afgs1";
const char* const kWhoMix = "vfgs_hip_models_from_afgs1_mix";

int refuse(int code, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	return vfgs::set_error(code, buf);
}

// one parameter set -> the parameter-set side of its job; 0, or the refusal (i: its index in the call, for the message)
// with_mix: the model carries the mix vfgs_init_afgs1 programs with the switch of vfgs_hip_afgs1_chroma_mix on (vfgs_fw_host.cpp), whatever
// the switch says
int job_from_afgs1(const fgs_afgs1& p, unsigned i, vfgs::FwModelJob& j, const bool with_mix)
{
	const char* const kWho = with_mix ? kWhoMix : kWhoPlain;
	memset(&j, 0, sizeof j);
	const int lag = p.ar_coeff_lag;
	if (lag < 1 || lag > 3)
		return refuse(42, "%s: parameter set %u: ar_coeff_lag %d, the reference supports 1..3 (vfgs_fw.c:438-459)", kWho, i, lag);
	if (p.num_y_points > 14 || p.num_cb_points > 10 || p.num_cr_points > 10)
		return refuse(42, "%s: parameter set %u: %d / %d / %d scaling points (at most 14 / 10 / 10)", kWho, i, p.num_y_points, p.num_cb_points, p.num_cr_points);
	if (p.ar_coeff_shift < 1 || p.ar_coeff_shift > 15)
		return refuse(42, "%s: parameter set %u: ar_coeff_shift %d outside 1..15", kWho, i, p.ar_coeff_shift);
	if (p.grain_scale_shift > 6)
		return refuse(42, "%s: parameter set %u: grain_scale_shift %d (at most 6)", kWho, i, p.grain_scale_shift);
	// chroma_scaling_from_luma: Cb and Cr take the luma function, and their own points are not looked at (vfgs_fw.c:676-682)
	if (!vfgs::afgs1_scaling_lut(j.slut[0], p.point_y_values, p.point_y_scaling, p.num_y_points))
		return refuse(42, "%s: parameter set %u: luma scaling points must be in increasing order (vfgs_fw.c:656)", kWho, i);
	if (p.chroma_scaling_from_luma)
	{
		memcpy(j.slut[1], j.slut[0], 256);
		memcpy(j.slut[2], j.slut[0], 256);
	}
	else if (!vfgs::afgs1_scaling_lut(j.slut[1], p.point_cb_values, p.point_cb_scaling, p.num_cb_points))
		return refuse(42, "%s: parameter set %u: Cb scaling points must be in increasing order (vfgs_fw.c:656)", kWho, i);
	else if (!vfgs::afgs1_scaling_lut(j.slut[2], p.point_cr_values, p.point_cr_scaling, p.num_cr_points))
		return refuse(42, "%s: parameter set %u: Cr scaling points must be in increasing order (vfgs_fw.c:656)", kWho, i);
	// QUIRK (vfgs_fw_host.cpp): all filters take 2*lag*(lag+1) taps; Cr's pattern LUT of 1 selects chroma slot 0, Cb's pattern, so
	// ar_coeffs_cr never reaches a picture and no Cr pattern is made
	vfgs::afgs1_taps(p.ar_coeffs_y, lag, j.coef[0]);
	vfgs::afgs1_taps(p.ar_coeffs_cb, lag, j.coef[1]);
	j.lag = lag;
	j.scale = p.ar_coeff_shift;
	j.shift = p.grain_scale_shift + 1;       // vfgs_fw.c:683-686
	j.scale_shift = p.grain_scaling - 6;     // the argument of vfgs_set_scale_shift; build_models checks and stores it for the programmed depth
	j.legal = p.clip_to_restricted_range != 0;
	// cb_mult and the other mix fields: vfgs_hip_models_from_afgs1 makes models without a mix, whatever vfgs_hip_afgs1_chroma_mix says;
	// grain_seed: the caller's (vfgs_hip_afgs1_seed)
	if (with_mix)
	{
		// what vfgs_init_afgs1 hands to vfgs_hip_set_chroma_mix, and what that setter would refuse (37 there)
		const bool cfl = p.chroma_scaling_from_luma != 0;
		const int v[2][3] = {{cfl ? 64 : p.cb_luma_mult - 128, cfl ? 0 : p.cb_mult - 128, cfl ? 0 : (int)p.cb_offset - 256},
		                     {cfl ? 64 : p.cr_luma_mult - 128, cfl ? 0 : p.cr_mult - 128, cfl ? 0 : (int)p.cr_offset - 256}};
		for (int c = 0; c < 2; c++)
		{
			if (v[c][0] < -128 || v[c][0] > 127 || v[c][1] < -128 || v[c][1] > 127 || v[c][2] < -256 || v[c][2] > 255)
				return refuse(42, "%s: parameter set %u: the mix of %s, %d, %d, %d, lies outside -128..127, -128..127, -256..255 (vfgs_hip_set_chroma_mix)", kWho, i,
				              c ? "Cr" : "Cb", v[c][0], v[c][1], v[c][2]);
			j.mix[c] = vfgs::model_mix_word(v[c][0], v[c][1], v[c][2], 1);     // (active: the setter's own rule -- a component that was set is)
		}
		j.mix_carried = 1;
	}
	return 0;
}

int models_from(const fgs_afgs1* cfgs, unsigned n, vfgs_hip_model** out, void* stream, const bool with_mix)
{
	const char* const kWho = with_mix ? kWhoMix : kWhoPlain;
	if (n == 0) return 0;
	if (!out) return refuse(41, "%s: null result pointer for %u models", kWho, n);
	for (unsigned i = 0; i < n; i++) out[i] = nullptr;
	if (!cfgs) return refuse(41, "%s: null parameter sets for %u models", kWho, n);
	std::vector<vfgs::FwModelJob> jobs(n);
	for (unsigned i = 0; i < n; i++)
		if (int e = job_from_afgs1(cfgs[i], i, jobs[i], with_mix)) return e;
	return vfgs::build_models(kWho, jobs.data(), n, out, stream, &vfgs::launch_fw_models);
}

}  // namespace

extern "C" int vfgs_hip_models_from_afgs1(const fgs_afgs1* cfgs, unsigned n, vfgs_hip_model** out, void* stream)
{
	return models_from(cfgs, n, out, stream, false);
}

extern "C" int vfgs_hip_models_from_afgs1_mix(const fgs_afgs1* cfgs, unsigned n, vfgs_hip_model** out, void* stream)
{
	return models_from(cfgs, n, out, stream, true);
}
