// TEST INFRASTRUCTURE -- tests/test_kernel_keys_cpu.py.  Every key of vfgs_layout.h over the three depths, the four formats, all bools and all
// families: for those kernel_exists() holds, one line "<kernel_name> <kernel_lds_bytes>".
#include <cstdio>

#include "../../versatilefilmgrain_amd/csrc/vfgs_layout.h"

int main()
{
	using namespace vfgs;
	const int depths[] = {8, 10, 12}, formats[][2] = {{2, 2}, {2, 1}, {1, 1}, {1, 2}};
	for (int f = (int)Family::rw; f <= (int)Family::sp_mix; f++)
		for (int d : depths)
			for (auto& xy : formats)
				for (int b = 0; b < 32; b++)
				{
					const KernelKey k{d, xy[0], xy[1], (b & 1) != 0, (b & 2) != 0, (b & 4) != 0, (b & 8) != 0, (b & 16) != 0, (Family)f};
					if (!kernel_exists(k)) continue;
					char name[128];
					kernel_name(k, name, sizeof name);
					printf("%s %d\n", name, kernel_lds_bytes(k));
				}
	return 0;
}
