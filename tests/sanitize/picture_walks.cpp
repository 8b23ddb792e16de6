// TEST INFRASTRUCTURE.  The check of the checker for the shared semi-planar picture of walks.h (SpPic, DevSpPic, SpPool): one launch, and the
// first of the program, runs on an SpPool -- padded rows, an odd block count, a UV pitch of its own -- so a stub kernel that walks one row
// past a plane overflows a block that DevSpPic allocated and nothing else.  Every walk of tests/sanitize_semiplanar/sp_walks.cpp first asks
// planar_regs() for the registers to expect, whose scratch planes such a kernel overflows before it reaches a picture; the shared planar
// device frame needs no program of its own (the first launch of seeded_walks' `entries` runs on a DevFrame).
//
// usage: picture_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 5
#include "walks.h"

static void walk_sp_pool()
{
	program(10, 2, 2, true);
	SpPic f(200, 40, 2, 2, 16, 8);
	SpPool pool(f, 3);
	OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), nullptr, 3, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f));
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"sp_pool", walk_sp_pool},
	});
}
