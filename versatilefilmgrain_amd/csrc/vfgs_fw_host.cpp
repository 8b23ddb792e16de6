// Firmware layer, host part: turns an FGC SEI message or an AFGS1 parameter set into what the
// hardware layer needs -- the two entry points of the reference's vfgs_fw.h:91-92.
//
// Only the small tables are computed here (scale / pattern LUTs, shifts, seed, the list of
// distinct patterns); the patterns themselves are generated on the GPU by
// vfgs_hip_generate_patterns (vfgs_fw_kernel.hip).  Like the reference's firmware this file is a
// pure client of the hardware-layer interface; the one thing it keeps is the switch of vfgs_hip_afgs1_chroma_mix.
//
// The derivations follow the reference line by line where the result depends on it, including
// its oddities (each is marked QUIRK), because parity is judged on the bytes the hardware layer
// ends up with (tests/golden/traces).
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vfgs_hip.h"
#include "../../include/vfgs_hip_fw.h"
#include "vfgs_fw_afgs1.h"
#include "vfgs_fw_sei.h"

namespace {

constexpr int kMaxPatterns = vfgs::kSeiMaxPatterns;

[[noreturn]] void fw_die(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	fprintf(stderr, "libvfgs_hip: fatal: ");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	abort();   // the reference asserts (vfgs_fw.c:459, :656)
}

// vfgs_hip_afgs1_chroma_mix: -1 = never called, the environment decides
std::atomic<int> g_afgs1_mix{-1};

bool afgs1_mix_on()
{
	static const bool env_on = [] { const char* e = getenv("VFGS_HIP_AFGS1_CHROMA_MIX"); return e && e[0] == '1'; }();
	const int v = g_afgs1_mix.load();
	return v < 0 ? env_on : v != 0;
}

void generate(const vfgs_hip_pattern_job* jobs, int n)
{
	if (n && vfgs_hip_generate_patterns(jobs, n))
		fw_die("pattern generation failed: %s", vfgs_hip_last_error_string());
}

// ---- SEI -------------------------------------------------------------------------------

// the list of distinct patterns, the tap matrix and the LUT fill: vfgs_fw_sei.h, shared with vfgs_hip_models_from_sei
using vfgs::PatternList;
using vfgs::collect_patterns;
using vfgs::sei_ar_taps;

void sei_jobs(const fgs_sei* cfg, const PatternList& pl, int chroma, vfgs_hip_pattern_job* jobs, int& n)
{
	for (int i = 0; i < pl.n; i++)
	{
		const int16_t* v = &cfg->comp_model_value[0][0][0] + pl.flat[i];
		vfgs_hip_pattern_job& j = jobs[n++];
		memset(&j, 0, sizeof j);
		j.chroma = chroma;
		j.index = i;
		j.seed_index = chroma;                 // vfgs_fw.c:369, :392, :606, :613
		if (cfg->model_id)
		{
			j.kind = 1;
			j.scale = cfg->log2_scale_factor;  // vfgs_fw.c:606: shift 1, scale log2_scale_factor
			j.shift = 1;
			sei_ar_taps(v, j.scale, j.coef);
		}
		else
		{
			j.kind = 0;
			j.fh = v[1];
			j.fv = v[2];
		}
	}
}

void sei_luts(const fgs_sei* cfg, const PatternList& pl, int c, unsigned char slut[256])
{
	unsigned char plut[256];
	vfgs::sei_fill_luts(cfg, pl, c, slut, plut);
	vfgs_set_scale_lut(c, slut);
	vfgs_set_pattern_lut(c, plut);
}

// ---- AFGS1 -----------------------------------------------------------------------------

// the scaling function and the tap order: vfgs_fw_afgs1.h, shared with vfgs_hip_models_from_afgs1 (which refuses where this aborts)
using vfgs::afgs1_taps;

void scaling_lut(unsigned char lut[256], const unsigned char* x, const unsigned char* y, int npoints)
{
	if (!vfgs::afgs1_scaling_lut(lut, x, y, npoints))
		fw_die("AFGS1 scaling points must be in increasing order (vfgs_fw.c:656)");
}

}  // namespace

extern "C" {

void vfgs_init_sei(fgs_sei* cfg)
{
	vfgs_hip_pattern_job jobs[2 * kMaxPatterns];
	int njobs = 0;
	PatternList luma, chroma;

	if (cfg->comp_model_present_flag[0])
		collect_patterns(cfg, 0, luma);
	sei_jobs(cfg, luma, 0, jobs, njobs);
	{
		unsigned char slut[256] = {0};
		sei_luts(cfg, luma, 0, slut);
	}
	// Cb and Cr share one bank and one list (vfgs_fw.c:533-538: the list is reset for c = 0 and 1 only)
	for (int c = 1; c < 3; c++)
		if (cfg->comp_model_present_flag[c])
			collect_patterns(cfg, c, chroma);
	sei_jobs(cfg, chroma, 1, jobs, njobs);
	{
		// QUIRK: one scale table is cleared before Cb and NOT between Cb and Cr (vfgs_fw.c:530,
		// :598-643), so Cr inherits Cb's scale wherever its own intervals leave a gap
		unsigned char slut[256] = {0};
		sei_luts(cfg, chroma, 1, slut);
		sei_luts(cfg, chroma, 2, slut);
	}
	generate(jobs, njobs);
	vfgs_set_scale_shift(cfg->log2_scale_factor - (cfg->model_id ? 1 : 0));   // vfgs_fw.c:644
	vfgs_hip_clear_chroma_mix();      // an SEI model indexes chroma by the chroma sample
}

void vfgs_hip_afgs1_chroma_mix(int enable)
{
	g_afgs1_mix.store(enable != 0);
}

unsigned int vfgs_hip_afgs1_seed(const fgs_afgs1* cfg)
{
	return cfg->grain_seed | ((uint32_t)cfg->grain_seed << 16);   // vfgs_fw.c:672
}

void vfgs_init_afgs1(fgs_afgs1* cfg)
{
	unsigned char lut[256];
	vfgs_hip_pattern_job jobs[3];
	const int lag = cfg->ar_coeff_lag;

	vfgs_set_seed(vfgs_hip_afgs1_seed(cfg));

	scaling_lut(lut, cfg->point_y_values, cfg->point_y_scaling, cfg->num_y_points);
	vfgs_set_scale_lut(0, lut);
	if (!cfg->chroma_scaling_from_luma)
		scaling_lut(lut, cfg->point_cb_values, cfg->point_cb_scaling, cfg->num_cb_points);
	vfgs_set_scale_lut(1, lut);
	if (!cfg->chroma_scaling_from_luma)
		scaling_lut(lut, cfg->point_cr_values, cfg->point_cr_scaling, cfg->num_cr_points);
	vfgs_set_scale_lut(2, lut);

	if (lag < 1 || lag > 3)
		fw_die("AFGS1 ar_coeff_lag %d: the reference supports 1..3 (vfgs_fw.c:438-459)", lag);
	// QUIRK: all three filters take 2*lag*(lag+1) taps (vfgs_fw.c:687-697); the extra chroma
	// coefficient (luma injection) is never used
	const int16_t* ar[3] = {cfg->ar_coeffs_y, cfg->ar_coeffs_cb, cfg->ar_coeffs_cr};
	for (int c = 0; c < 3; c++)
	{
		vfgs_hip_pattern_job& j = jobs[c];
		memset(&j, 0, sizeof j);
		j.kind = 1;
		j.chroma = c > 0;
		j.index = c == 2 ? 1 : 0;              // Cb -> chroma slot 0, Cr -> chroma slot 1
		j.seed_index = c;                      // vfgs_fw.c:689, :693, :697
		j.scale = cfg->ar_coeff_shift;
		j.shift = cfg->grain_scale_shift + 1;  // vfgs_fw.c:683-686
		afgs1_taps(ar[c], lag, j.coef);
	}
	generate(jobs, 3);

	memset(lut, 0, sizeof lut);
	vfgs_set_pattern_lut(0, lut);
	vfgs_set_pattern_lut(1, lut);
	// QUIRK: the reference fills Cr's pattern table with 1, and the hardware layer takes the slot
	// from bits 7:4 (vfgs_hw.c:212): Cr therefore uses chroma slot 0, Cb's pattern
	memset(lut, 1, sizeof lut);
	vfgs_set_pattern_lut(2, lut);

	vfgs_set_scale_shift(cfg->grain_scaling - 6);
	vfgs_set_legal_range(cfg->clip_to_restricted_range);

	// cb_mult / cb_luma_mult / cb_offset (and Cr's): parsed and dropped by the reference (vfgs_fw.c:706); with the switch of
	// vfgs_hip_afgs1_chroma_mix they become the hardware layer's luma / chroma mix, otherwise the index stays the chroma sample
	vfgs_hip_clear_chroma_mix();
	if (afgs1_mix_on())
	{
		const bool cfl = cfg->chroma_scaling_from_luma != 0;
		if (vfgs_hip_set_chroma_mix(1, cfl ? 64 : cfg->cb_luma_mult - 128, cfl ? 0 : cfg->cb_mult - 128, cfl ? 0 : (int)cfg->cb_offset - 256) ||
		    vfgs_hip_set_chroma_mix(2, cfl ? 64 : cfg->cr_luma_mult - 128, cfl ? 0 : cfg->cr_mult - 128, cfl ? 0 : (int)cfg->cr_offset - 256))
			fw_die("AFGS1 chroma mix: %s", vfgs_hip_last_error_string());
	}
}

}  // extern "C"
