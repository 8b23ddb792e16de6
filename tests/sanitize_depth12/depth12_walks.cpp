// TEST INFRASTRUCTURE.  The host layer of libvfgs_hip at sample depth 12 (vfgs_set_depth(12): bs = 4, uint16 containers), compiled with a
// sanitizer over tests/sanitize/hip_stub.cpp, as tests/sanitize/host_walks.cpp drives the rest of it: the setters and the export that
// answers which depths exist, device entries in place and out of place, parts, lists, an overlap region, rows walked in parts, line calls
// with the look-ahead, host stripes and frames on one and on two devices, depth switches in the middle of a process, the refusal of
// an active chroma mix.  The stub's "kernel" copies rows unchanged, so every walk also checks that what a call hands back is what went in.
// The stub refuses the narrowed destination and persistent luma workgroups at depths other than 10: the shapes here need neither
// (one-pattern models, or launches of few luma tasks); those two paths are the GPU suite's business (tests/test_gpu_depth12.py).
//
// usage: depth12_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 12
#include "../sanitize/walks.h"

static bool last_launch(int depth, unsigned long long* launches = nullptr, int* persistent = nullptr)
{
	vfgs_hip_launch_info li;
	if (vfgs_hip_last_launch_info(&li)) return false;
	if (launches) *launches = li.launches;
	if (persistent) *persistent = li.persistent_luma_workgroups;
	char want[32];
	snprintf(want, sizeof want, "stub<%d,", depth);
	return li.depth == depth && !strncmp(li.kernel, want, strlen(want));
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_setters_and_export()
{
	for (int d = -3; d < 40; d++) CHECK(vfgs_hip_supports_depth(d) == (d == 8 || d == 10 || d == 12));
	int p[8];
	for (int shift = 2; shift <= 7; shift++)
	{
		vfgs_hip_reset_state();
		vfgs_set_scale_shift(shift);
		vfgs_set_depth(12);
		vfgs_hip_get_params(p);
		CHECK(p[0] == shift + 2 && p[1] == 4);
		vfgs_set_depth(10);
		vfgs_hip_get_params(p);
		CHECK(p[0] == shift + 4 && p[1] == 2);
		vfgs_set_depth(12);
		vfgs_set_scale_shift(shift);
		vfgs_set_legal_range(1);
		vfgs_hip_get_params(p);
		CHECK(p[0] == shift + 2 && p[1] == 4 && p[2] == 16 && p[3] == 235 && p[4] == 16 && p[5] == 240);
		vfgs_set_depth(8);
		vfgs_hip_get_params(p);
		CHECK(p[0] == shift + 6 && p[1] == 0);
	}
	vfgs_set_depth(12);
	vfgs_hip_reset_state();
	vfgs_hip_get_params(p);
	CHECK(p[0] == 11 && p[1] == 0);
}

static void walk_device_entries()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	// width, height, subsampling, one-pattern model, shift (general-form luma: launches of few luma tasks -- no persistent workgroups)
	const int cases[][6] = {{1920, 270, 2, 2, 1, 5}, {520, 270, 2, 1, 0, 2}, {1042, 96, 1, 1, 1, 7}, {333, 80, 2, 2, 0, 5}, {8208, 48, 1, 1, 1, 2},
	                        {8400, 48, 2, 2, 0, 7}, {520, 270, 1, 2, 1, 5}, {16400, 32, 2, 1, 0, 5}};
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], sx = c[2], sy = c[3], nf = 3;
		program(12, sx, sy, c[4] != 0, c[5]);
		Frame f(w, h, 12, sx, sy);
		DevFrame d(f, nf);
		unsigned long long n0 = 0, n1 = 0;
		int pers = 0;
		OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, w, h, f.stride, f.cstride, st));
		CHECK(last_launch(12, &n0, &pers) && pers == 0);
		OK(vfgs_hip_add_grain_frames_dev(d.Y, d.U, d.V, w, h, f.stride, f.cstride, nf, d.ny, d.nc, st));
		CHECK(last_launch(12, &n1, &pers) && n1 == n0 + 1 && pers == 0);
		OK(vfgs_hip_add_grain_stripe_dev(d.Y + (size_t)22 * f.stride * f.sz, d.U + (size_t)(22 / sy) * f.cstride * f.sz, d.V + (size_t)(22 / sy) * f.cstride * f.sz, 22, w, 9,
		                                 f.stride, f.cstride, nullptr));
		OK(vfgs_hip_add_grain_frame_part_dev(d.Y + (size_t)16 * f.stride * f.sz, d.U + (size_t)(16 / sy) * f.cstride * f.sz, d.V + (size_t)(16 / sy) * f.cstride * f.sz, w, h, 16,
		                                     h - 16 - 3, f.stride, f.cstride, st));
		OK(vfgs_hip_add_grain_frames_part_dev(d.Y + (size_t)16 * f.stride * f.sz, d.U + (size_t)(16 / sy) * f.cstride * f.sz, d.V + (size_t)(16 / sy) * f.cstride * f.sz, w, h, 16,
		                                      16, f.stride, f.cstride, nf, d.ny, d.nc, st));
		{
			DevFrame o(d.ny * nf, d.nc * nf);
			OK(vfgs_hip_add_grain_copy_dev(d.Y, d.U, d.V, o.Y, o.U, o.V, w, h, 0, h, f.stride, f.cstride, nf, d.ny, d.nc, st));
			CHECK(last_launch(12));
			hipStreamSynchronize(st);
		}
		{
			std::vector<DevFrame*> fr;
			std::vector<vfgs_hip_frame_ptrs> list, dst;
			for (int i = 0; i < 6; i++) { fr.push_back(new DevFrame(f)); (i < 3 ? list : dst).push_back({fr.back()->Y, fr.back()->U, fr.back()->V}); }
			OK(vfgs_hip_add_grain_frame_list_dev(list.data(), 3, w, h, f.stride, f.cstride, st));
			OK(vfgs_hip_add_grain_frame_list_copy_dev(list.data(), dst.data(), 3, w, h, f.stride, f.cstride, st));
			OK(vfgs_hip_add_grain_frame_list_part_dev(list.data(), 3, w, h, 0, 32, f.stride, f.cstride, st));
			OK(vfgs_hip_overlap_begin(st));
			for (int i = 0; i < 3; i++) OK(vfgs_hip_add_grain_frame_dev(fr[i]->Y, fr[i]->U, fr[i]->V, w, h, f.stride, f.cstride, st));
			OK(vfgs_hip_overlap_end(st));
			hipStreamSynchronize(st);
			for (int i = 0; i < 3; i++) CHECK(fr[i]->holds(f));
			for (auto* p : fr) delete p;
		}
		hipStreamSynchronize(st);
		for (int i = 0; i < nf; i++) CHECK(d.holds(f, i));
		// the narrowed destination needs a 16-bit path: refused at depth 8 with error 16, before anything moves
		if (w == 333)
		{
			vfgs_set_depth(8);
			uint32_t s0[4], s1[4];
			vfgs_hip_get_seed_state(s0);
			CHECK(vfgs_hip_add_grain_copy8_dev(d.Y, d.U, d.V, d.Y, d.U, d.V, w, h, 0, h, f.stride, f.cstride, f.stride, f.cstride, 1, 0, 0, 0, 0, st) == 16);
			vfgs_hip_get_seed_state(s1);
			CHECK(!memcmp(s0, s1, sizeof s0));
		}
	}
	hipStreamDestroy(st);
}

static void walk_host_entries()
{
	const int cases[][4] = {{192, 144, 2, 2}, {200, 150, 1, 1}, {720, 576, 2, 2}, {346, 160, 2, 1}};
	for (const auto& c : cases)
	{
		program(12, c[2], c[3], c[0] != 720);
		vfgs_hip_line_lookahead(1);
		Frame f(c[0], c[1], 12, c[2], c[3]);
		const Frame before = f;
		OK(vfgs_hip_declare_frame(f.y(0), f.u(0), f.v(0), f.w, f.h, f.stride, f.cstride));
		for (int pass = 0; pass < 2; pass++)
			for (int y = 0; y < f.h; y++) vfgs_add_grain_line(f.y(y), f.u(y), f.v(y), y, f.w);
		OK(vfgs_hip_declare_frame(nullptr, nullptr, nullptr, 0, 0, 0, 0));
		CHECK(f.same(before) && last_launch(12));
		// a setter in the middle of a walk: the depth goes to 10 and back (what was computed ahead at 12 bit must not be served)
		for (int y = 0; y < f.h; y++)
		{
			if (y == 40) { vfgs_set_depth(10); vfgs_set_depth(12); }
			vfgs_add_grain_line(f.y(y), f.u(y), f.v(y), y, f.w);
		}
		CHECK(f.same(before));
		int y = 0;
		for (int hh : {6, 26, 32, 1, 15, 64}) { vfgs_add_grain_stripe(f.y(y), f.u(y), f.v(y), y, f.w, hh, f.stride, f.cstride); y += hh; }
		CHECK(f.same(before));
		std::vector<Frame> fr(4, f);
		std::vector<void*> Y, U, V;
		for (auto& x : fr) { Y.push_back(x.Y.data()); U.push_back(x.U.data()); V.push_back(x.V.data()); }
		OK(vfgs_hip_add_grain_frames_host(Y.data(), U.data(), V.data(), 4, f.w, f.h, f.stride, f.cstride));
		for (auto& x : fr) CHECK(x.same(before));
		// two devices (device 0 listed twice)
		const int two[2] = {0, 0}, one[1] = {0};
		OK(vfgs_hip_init_devices(two, 2));
		OK(vfgs_hip_add_grain_frames_host(Y.data(), U.data(), V.data(), 4, f.w, f.h, f.stride, f.cstride));
		vfgs_add_grain_stripe(f.y(0), f.u(0), f.v(0), 0, f.w, f.h, f.stride, f.cstride);
		for (auto& x : fr) CHECK(x.same(before));
		CHECK(f.same(before));
		OK(vfgs_hip_init_devices(one, 1));
	}
}

static void walk_depth_switches_two_threads()
{
	// 8 -> 12 -> 10 -> 12 with a frame at every depth, while another thread asks for the state
	std::thread other([] {
		int p[8];
		vfgs_hip_launch_info li;
		for (int i = 0; i < 300; i++) { vfgs_hip_get_params(p); (void)vfgs_hip_last_launch_info(&li); (void)vfgs_hip_supports_depth(i % 16); }
	});
	for (int round = 0; round < 3; round++)
		for (int depth : {8, 12, 10, 12})
		{
			program(depth, 2, 2, round != 1);
			Frame f(416, 96, depth, 2, 2);
			DevFrame d(f);
			OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr));
			CHECK(last_launch(depth) && d.holds(f));
			// the depth alone, tables kept: a new image (pre-shifted scales) for the next call
			if (depth == 10)
			{
				vfgs_set_depth(12);
				Frame g(416, 96, 12, 2, 2);
				DevFrame e(g);
				OK(vfgs_hip_add_grain_frame_dev(e.Y, e.U, e.V, g.w, g.h, g.stride, g.cstride, nullptr));
				CHECK(last_launch(12) && e.holds(g));
			}
		}
	other.join();
}

static void walk_mix_refused()
{
	// an active chroma mix while the depth is 12: error 38 from every processing call, nothing moves
	uint32_t s0[4], s1[4];
	unsigned long long n0 = 0, n1 = 0;
	program(12, 2, 2, true);
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	Frame f(512, 64, 12, 2, 2);
	DevFrame d(f);
	last_launch(12, &n0);
	vfgs_hip_get_seed_state(s0);
	CHECK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr) == 38 && vfgs_hip_last_error() == 38);
	CHECK(vfgs_hip_add_grain_stripe_dev(d.Y, d.U, d.V, 0, f.w, 16, f.stride, f.cstride, nullptr) == 38);
	CHECK(vfgs_hip_add_grain_frames_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, 1, 0, 0, nullptr) == 38);
	CHECK(vfgs_hip_add_grain_frame_part_dev(d.Y, d.U, d.V, f.w, f.h, 0, 32, f.stride, f.cstride, nullptr) == 38);
	CHECK(vfgs_hip_add_grain_copy_dev(d.Y, d.U, d.V, d.Y, d.U, d.V, f.w, f.h, 0, f.h, f.stride, f.cstride, 1, 0, 0, nullptr) == 38);
	vfgs_hip_frame_ptrs l = {d.Y, d.U, d.V};
	CHECK(vfgs_hip_add_grain_frame_list_dev(&l, 1, f.w, f.h, f.stride, f.cstride, nullptr) == 38);
	CHECK(vfgs_hip_add_grain_frame_list_part_dev(&l, 1, f.w, f.h, 0, 32, f.stride, f.cstride, nullptr) == 38);
	CHECK(vfgs_hip_add_grain_frame_list_copy_dev(&l, &l, 1, f.w, f.h, f.stride, f.cstride, nullptr) == 38);
	void *Y = f.Y.data(), *U = f.U.data(), *V = f.V.data();
	const Frame before = f;
	CHECK(vfgs_hip_add_grain_frames_host(&Y, &U, &V, 1, f.w, f.h, f.stride, f.cstride) == 38);
	vfgs_hip_get_seed_state(s1);
	last_launch(12, &n1);
	CHECK(!memcmp(s0, s1, sizeof s0) && n0 == n1 && d.holds(f) && f.same(before));
	// at depth 10 the same state is served by the kernels of the mix; cleared, depth 12 is the call of always
	vfgs_set_depth(10);
	OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr));
	vfgs_set_depth(12);
	vfgs_hip_clear_chroma_mix();
	OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr));
	CHECK(last_launch(12) && d.holds(f));
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"setters_and_export", walk_setters_and_export},
		{"device_entries", walk_device_entries},
		{"host_entries", walk_host_entries},
		{"depth_switches_two_threads", walk_depth_switches_two_threads},
		{"mix_refused", walk_mix_refused},
	});
}
