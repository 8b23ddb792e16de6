// AFGS1 parameter set -> the small tables, shared by the two host files of the firmware layer that read one: vfgs_fw_host.cpp
// (vfgs_init_afgs1 programs the hardware layer with them) and vfgs_model_build_host.cpp (vfgs_hip_models_from_afgs1 puts them into
// the job table of fw_models_kernel).  The derivations follow the reference line by line, oddities included (vfgs_fw_host.cpp, QUIRK).
#pragma once
#include <stdint.h>
#include <string.h>

namespace vfgs {

// AFGS1 scaling function -> scale LUT: zero outside the points, between two points the rounded interpolation of
// vfgs_fw.c:649-661 (integer division that truncates towards zero, also for falling segments).  Segments are half-open
// [x[s], x[s+1]): the reference writes every segment including its end point and the next segment then rewrites that
// entry with its own start value -- the same bytes; only the last segment keeps its end point.
// false: the points are not in increasing order (the reference asserts, vfgs_fw.c:656); the LUT is then incomplete.
inline bool afgs1_scaling_lut(unsigned char lut[256], const unsigned char* x, const unsigned char* y, int npoints)
{
	memset(lut, 0, 256);
	for (int s = 0; s + 1 < npoints; s++)
	{
		const int x0 = x[s], span = x[s + 1] - x0, rise = (int)y[s + 1] - (int)y[s];
		if (span <= 0) return false;
		const int stop = x0 + span + (s + 2 == npoints ? 1 : 0);
		for (int t = x0; t < stop; t++)
			lut[t] = (unsigned char)(y[s] + (rise * (t - x0) + span / 2) / span);
	}
	return true;
}

// AV1 order of the causal neighbourhood -> 4x7 tap matrix (vfgs_fw.c:461-464)
inline void afgs1_taps(const int16_t* ar, int lag, int16_t coef[28])
{
	memset(coef, 0, 28 * sizeof(int16_t));
	int k = 0;
	for (int j = -lag; j <= 0; j++)
		for (int i = -lag; i <= lag && (i < 0 || j < 0); i++)
			coef[(3 + j) * 7 + 3 + i] = ar[k++];
}

}  // namespace vfgs
