// FGC SEI message -> the list of distinct patterns and the small tables, shared by the two host files of the firmware layer that read
// one: vfgs_fw_host.cpp (vfgs_init_sei programs the hardware layer with them) and vfgs_model_build_sei_host.cpp (vfgs_hip_models_from_sei
// puts them into the job table of fw_sei_build_kernel).  The derivations follow the reference line by line where the result depends on
// it, oddities included (each is marked QUIRK): this header is the one statement of them.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/vfgs_hip_fw.h"

namespace vfgs {

constexpr int kSeiMaxPatterns = 8;   // VFGS_MAX_PATTERNS, vfgs_hw.h:49

// The list of distinct patterns of one bank.  An entry is the position of an interval's model
// values in comp_model_value viewed as one flat int16 array (vfgs_fw.c:545: 6*(k + 256*c)).
struct PatternList {
	int n = 0;
	bool used[kSeiMaxPatterns] = {};
	int flat[kSeiMaxPatterns] = {};
	unsigned char lower[kSeiMaxPatterns] = {};   // lower intensity bound the entry was created from (sort key)
};

// Values 1..5 of an entry, i.e. everything but the scale factor (vfgs_fw.c:504-515).
// QUIRK: the reference initialises unused entries to ~0 and still compares against them; with
// its pointer arithmetic an unused entry reads elements -1+1 .. -1+5 of the flat array, that is
// the FIRST five numbers of the luma component's first interval.  Reproduced.
inline const int16_t* entry_tail(const fgs_sei* cfg, const PatternList& pl, int i)
{
	const int16_t* base = &cfg->comp_model_value[0][0][0];
	return pl.used[i] ? base + pl.flat[i] + 1 : base;
}

inline int find_pattern(const fgs_sei* cfg, const PatternList& pl, int flat)
{
	const int16_t* want = &cfg->comp_model_value[0][0][0] + flat + 1;
	for (int i = 0; i < kSeiMaxPatterns; i++)
		if (!memcmp(entry_tail(cfg, pl, i), want, (SEI_MAX_MODEL_VALUES - 1) * sizeof(int16_t)))
			return i;
	return kSeiMaxPatterns;
}

inline void collect_patterns(const fgs_sei* cfg, int c, PatternList& pl)
{
	// vfgs_fw.c:540-572: new parameter sets join the list, which stays sorted by the lower bound
	for (int k = 0; k < cfg->num_intensity_intervals[c]; k++)
	{
		const int flat = SEI_MAX_MODEL_VALUES * (k + 256 * c);
		if (find_pattern(cfg, pl, flat) != kSeiMaxPatterns || pl.n >= kSeiMaxPatterns)
			continue;
		const unsigned char a = cfg->intensity_interval_lower_bound[c][k];
		int at = pl.n;
		while (at > 0 && pl.lower[at - 1] > a)
		{
			pl.lower[at] = pl.lower[at - 1];
			pl.flat[at] = pl.flat[at - 1];
			at--;
		}
		pl.lower[at] = a;
		pl.flat[at] = flat;
		pl.used[pl.n] = true;   // entries 0..n are the used ones; the sort only moves values
		pl.n++;
	}
}

// SEI auto-regressive model: the six model values become a 4x7 tap matrix (vfgs_fw.c:427-436)
inline void sei_ar_taps(const int16_t* v, int scale, int16_t coef[28])
{
	memset(coef, 0, 28 * sizeof(int16_t));
	auto at = [&](int row, int col) -> int16_t& { return coef[row * 7 + col]; };
	at(3, 2) = v[1];                                           // left
	at(2, 3) = (int16_t)((v[1] * v[4]) >> scale);              // top
	at(2, 2) = at(2, 4) = (int16_t)((v[3] * v[4]) >> scale);   // top-left, top-right
	at(3, 1) = v[5];                                           // two to the left
	at(1, 3) = (int16_t)((int32_t)((uint32_t)v[5] * (uint32_t)v[4] * (uint32_t)v[4]) >> (2 * scale));   // two up
}

// Scale and pattern LUT of component c (vfgs_fw.c:598-643).  plut is written whole; slut only inside the component's intervals, so
// what the caller hands in shows through the gaps (vfgs_init_sei's QUIRK of Cb and Cr sharing one table).
inline void sei_fill_luts(const fgs_sei* cfg, const PatternList& pl, int c, unsigned char slut[256], unsigned char plut[256])
{
	if (!cfg->comp_model_present_flag[c])
	{
		memset(plut, 0, 256);
		return;
	}
	memset(plut, 255, 256);
	for (int k = 0; k < cfg->num_intensity_intervals[c]; k++)
	{
		const int a = cfg->intensity_interval_lower_bound[c][k];
		const int b = cfg->intensity_interval_upper_bound[c][k];
		const int i = find_pattern(cfg, pl, SEI_MAX_MODEL_VALUES * (k + 256 * c));
		for (int l = a; l <= b; l++)
		{
			slut[l] = (unsigned char)cfg->comp_model_value[c][k][0];
			if (i < kSeiMaxPatterns)
				plut[l] = (unsigned char)(i << 4);
		}
	}
	// intensities outside every interval repeat the pattern below them (vfgs_fw.c:625-633)
	unsigned char last = 0;
	for (int k = 0; k < 256; k++)
	{
		if (plut[k] == 255) plut[k] = last;
		else last = plut[k];
	}
}

}  // namespace vfgs
