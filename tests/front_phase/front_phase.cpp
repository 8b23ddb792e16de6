// Stand-alone host program for tests/test_front_phase_cpu.py: the grid of a launch (vfgs_kernel.hip grid_of) decoded workgroup by workgroup
// with vfgs_layout.h front_task, the two phase fields from the host's rule (front_phase) or zero.
//
// usage: front_phase <luma workgroups> <workgroups of one chroma plane> <frames> <lfronts> <phase on: 0 | 1>
// prints "<shift> <plain_from> <grid x> <grid y>", then one line "<f> <r>" per workgroup, blockIdx.x fastest.
#include <stdio.h>
#include <stdlib.h>

#include "../../versatilefilmgrain_amd/csrc/vfgs_layout.h"

// (what the function is for: usable where a constant is asked for)
static_assert(vfgs::front_task(5, 3, 1, 6, 4, 4).f == 7 && vfgs::front_task(5, 3, 1, 6, 4, 4).r == 0, "odd front, rotated: task 2 + 4 wraps to 0");
static_assert(vfgs::front_task(5, 3, 1, 6, 4, 3).r == 2 && vfgs::front_task(4, 3, 1, 6, 4, 4).r == 2, "a plain group / the even front: today's decode");

int main(int argc, char** argv)
{
	if (argc != 6) return 2;
	const int wy = atoi(argv[1]), wc = atoi(argv[2]), nframes = atoi(argv[3]), lfronts = atoi(argv[4]), on = atoi(argv[5]);
	const int per_frame = wy + 2 * wc;
	const vfgs::FrontPhase fp = on ? vfgs::front_phase(lfronts, true, wy, wc, nframes) : vfgs::FrontPhase{0, 0};
	const unsigned gx = (unsigned)per_frame << lfronts, gy = ((unsigned)nframes + (1u << lfronts) - 1) >> lfronts;
	printf("%d %d %u %u\n", fp.shift, fp.plain_from, gx, gy);
	for (unsigned by = 0; by < gy; by++)
		for (unsigned bx = 0; bx < gx; bx++)
		{
			const vfgs::FrontTask t = vfgs::front_task(bx, by, lfronts, per_frame, fp.shift, fp.plain_from);
			printf("%d %d\n", t.f, t.r);
		}
	return 0;
}
