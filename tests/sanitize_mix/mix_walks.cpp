// TEST INFRASTRUCTURE.  The host layer of libvfgs_hip with a luma / chroma mix active (vfgs_hip_set_chroma_mix), compiled with a
// sanitizer over tests/sanitize/hip_stub.cpp, as tests/sanitize/host_walks.cpp drives the rest of it: set / get / clear and their
// refusals, device entries in place (two launches: chroma, then luma) and out of place, lists, the narrowed destination, line
// calls and host stripes and frames, the firmware switch from two threads, the refusals that must change nothing.  The stub's
// "kernel" copies rows unchanged, so every walk also checks that what a call hands back is what went in.
//
// usage: mix_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 7
#include "../sanitize/walks.h"

static bool last_kernel_is(const char* prefix, unsigned long long* launches = nullptr)
{
	vfgs_hip_launch_info li;
	if (vfgs_hip_last_launch_info(&li)) return false;
	if (launches) *launches = li.launches;
	return !strncmp(li.kernel, prefix, strlen(prefix));
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_set_get_clear()
{
	vfgs_hip_reset_state();
	int m[4] = {9, 9, 9, 9};
	OK(vfgs_hip_get_chroma_mix(1, m));
	CHECK(m[0] == 0 && m[1] == 0 && m[2] == 0 && m[3] == 0);
	OK(vfgs_hip_set_chroma_mix(1, -128, 127, -256));
	OK(vfgs_hip_set_chroma_mix(2, 127, -128, 255));
	OK(vfgs_hip_get_chroma_mix(2, m));
	CHECK(m[0] == 127 && m[1] == -128 && m[2] == 255 && m[3] == 1);
	CHECK(vfgs_hip_set_chroma_mix(0, 0, 64, 0) == 37 && vfgs_hip_set_chroma_mix(3, 0, 64, 0) == 37);
	CHECK(vfgs_hip_set_chroma_mix(1, 128, 0, 0) == 37 && vfgs_hip_set_chroma_mix(1, 0, -129, 0) == 37 && vfgs_hip_set_chroma_mix(1, 0, 0, 256) == 37);
	CHECK(vfgs_hip_get_chroma_mix(1, nullptr) == 37 && vfgs_hip_last_error() == 37);
	OK(vfgs_hip_get_chroma_mix(1, m));
	CHECK(m[0] == -128 && m[1] == 127 && m[2] == -256 && m[3] == 1);
	vfgs_hip_clear_chroma_mix();
	OK(vfgs_hip_get_chroma_mix(1, m));
	CHECK(m[3] == 0);
	OK(vfgs_hip_set_chroma_mix(2, 1, 2, 3));
	vfgs_hip_reset_state();
	OK(vfgs_hip_get_chroma_mix(2, m));
	CHECK(m[0] == 0 && m[3] == 0);
}

static void walk_device_entries()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	const int cases[][5] = {{1920, 270, 10, 2, 2}, {520, 270, 10, 2, 1}, {1042, 96, 8, 1, 1}, {333, 80, 8, 2, 2}, {8208, 48, 10, 1, 1}, {8400, 48, 8, 2, 2}, {520, 270, 10, 1, 2}};
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], depth = c[2], sx = c[3], sy = c[4], nf = 3;
		program(depth, sx, sy, true);
		OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
		if (w != 520) OK(vfgs_hip_set_chroma_mix(2, 64, 119, -238));      // (one component alone as well)
		Frame f(w, h, depth, sx, sy);
		DevFrame d(f, nf);
		unsigned long long n0 = 0, n1 = 0;
		OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, w, h, f.stride, f.cstride, st));
		CHECK(last_kernel_is("grain_mix_kernel<", &n0));
		// in place: chroma in a launch of its own in front of luma's
		OK(vfgs_hip_add_grain_frames_dev(d.Y, d.U, d.V, w, h, f.stride, f.cstride, nf, d.ny, d.nc, st));
		CHECK(last_kernel_is("grain_mix_kernel<", &n1) && n1 == n0 + 2);
		OK(vfgs_hip_add_grain_stripe_dev(d.Y + (size_t)22 * f.stride * f.sz, d.U + (size_t)(22 / sy) * f.cstride * f.sz, d.V + (size_t)(22 / sy) * f.cstride * f.sz, 22, w, 21,
		                                 f.stride, f.cstride, nullptr));
		OK(vfgs_hip_add_grain_frame_part_dev(d.Y + (size_t)16 * f.stride * f.sz, d.U + (size_t)(16 / sy) * f.cstride * f.sz, d.V + (size_t)(16 / sy) * f.cstride * f.sz, w, h, 16,
		                                     h - 16 - 3, f.stride, f.cstride, st));
		// out of place: one launch
		{
			DevFrame o(d.ny * nf, d.nc * nf);
			OK(vfgs_hip_add_grain_copy_dev(d.Y, d.U, d.V, o.Y, o.U, o.V, w, h, 0, h, f.stride, f.cstride, nf, d.ny, d.nc, st));
			CHECK(last_kernel_is("grain_mix_kernel<", &n0));
			if (depth == 10)
			{
				DevFrame o8((size_t)f.stride * h * nf, (size_t)f.cstride * f.ch * nf);
				OK(vfgs_hip_add_grain_copy8_dev(d.Y, d.U, d.V, o8.Y, o8.U, o8.V, w, h, 0, h, f.stride, f.cstride, f.stride, f.cstride, nf, d.ny, d.nc, (size_t)f.stride * h,
				                                (size_t)f.cstride * f.ch, st));
				CHECK(last_kernel_is("grain_mix_kernel<", &n1) && n1 == n0 + 1);
			}
			hipStreamSynchronize(st);
			for (int i = 0; i < nf; i++) CHECK(DevFrame(f).holds(f));
		}
		// frames anywhere, in place and out of place
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
			for (auto* p : fr) { CHECK(p->holds(f)); delete p; }
		}
		hipStreamSynchronize(st);
		for (int i = 0; i < nf; i++) CHECK(d.holds(f, i));
		// and without the mix: the kernels of always
		vfgs_hip_clear_chroma_mix();
		OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, w, h, f.stride, f.cstride, st));
		CHECK(last_kernel_is("stub<"));
		hipStreamSynchronize(st);
	}
	hipStreamDestroy(st);
}

static void walk_host_entries()
{
	const int cases[][5] = {{192, 144, 10, 2, 2}, {200, 150, 8, 1, 1}, {720, 576, 8, 2, 2}};
	for (const auto& c : cases)
	{
		program(c[2], c[3], c[4], true);
		OK(vfgs_hip_set_chroma_mix(1, 64, 0, 0));
		OK(vfgs_hip_set_chroma_mix(2, 64, 0, 0));
		vfgs_hip_line_lookahead(1);
		Frame f(c[0], c[1], c[2], c[3], c[4]);
		const Frame before = f;
		for (int pass = 0; pass < 2; pass++)      // (a second walk through the same buffer is where the look-ahead would start to work ahead)
			for (int y = 0; y < f.h; y++) vfgs_add_grain_line(f.y(y), f.u(y), f.v(y), y, f.w);
		CHECK(last_kernel_is("grain_mix_kernel<"));
		int y = 0;
		for (int hh : {6, 26, 32, 1, 15, 64}) { vfgs_add_grain_stripe(f.y(y), f.u(y), f.v(y), y, f.w, hh, f.stride, f.cstride); y += hh; }
		CHECK(f.same(before));
		std::vector<Frame> fr(4, f);
		std::vector<void*> Y, U, V;
		for (auto& x : fr) { Y.push_back(x.Y.data()); U.push_back(x.U.data()); V.push_back(x.V.data()); }
		OK(vfgs_hip_add_grain_frames_host(Y.data(), U.data(), V.data(), 4, f.w, f.h, f.stride, f.cstride));
		for (auto& x : fr) CHECK(x.same(before));
		// the mix cleared in the middle of a walk: the look-ahead is back and must not serve anything computed before
		vfgs_hip_clear_chroma_mix();
		for (int pass = 0; pass < 2; pass++)
			for (int yy = 0; yy < f.h; yy++) vfgs_add_grain_line(f.y(yy), f.u(yy), f.v(yy), yy, f.w);
		CHECK(f.same(before) && last_kernel_is("stub<"));
	}
}

static void walk_firmware_switch_from_two_threads()
{
	vfgs_hip_reset_state();
	fgs_afgs1 a;
	memset(&a, 0, sizeof a);
	a.grain_seed = 77; a.num_y_points = 2; a.point_y_values[1] = 255; a.point_y_scaling[0] = 20; a.point_y_scaling[1] = 60;
	a.num_cb_points = 2; a.point_cb_values[1] = 255; a.point_cb_scaling[1] = 40; a.num_cr_points = 2; a.point_cr_values[1] = 255; a.point_cr_scaling[1] = 40;
	a.grain_scaling = 10; a.ar_coeff_lag = 2; a.ar_coeff_shift = 7;
	a.cb_mult = 247; a.cb_luma_mult = 192; a.cb_offset = 18; a.cr_mult = 229; a.cr_luma_mult = 192; a.cr_offset = 54;
	std::thread other([] {
		int m[4];
		for (int i = 0; i < 200; i++) { vfgs_hip_afgs1_chroma_mix(i & 1); (void)vfgs_hip_get_chroma_mix(1 + (i & 1), m); }
		vfgs_hip_afgs1_chroma_mix(1);
	});
	for (int i = 0; i < 20; i++) vfgs_init_afgs1(&a);
	other.join();
	vfgs_init_afgs1(&a);
	int m[4];
	OK(vfgs_hip_get_chroma_mix(1, m));
	CHECK(m[0] == 64 && m[1] == 119 && m[2] == -238 && m[3] == 1);
	OK(vfgs_hip_get_chroma_mix(2, m));
	CHECK(m[0] == 64 && m[1] == 101 && m[2] == -202 && m[3] == 1);
	Frame f(320, 64, 8, 2, 2);
	const Frame before = f;
	for (int y = 0; y < f.h; y++) vfgs_add_grain_line(f.y(y), f.u(y), f.v(y), y, f.w);
	CHECK(f.same(before) && last_kernel_is("grain_mix_kernel<8,2,2,"));
	a.chroma_scaling_from_luma = 1;
	vfgs_init_afgs1(&a);
	OK(vfgs_hip_get_chroma_mix(2, m));
	CHECK(m[0] == 64 && m[1] == 0 && m[2] == 0 && m[3] == 1);
	vfgs_hip_afgs1_chroma_mix(0);
	vfgs_init_afgs1(&a);
	OK(vfgs_hip_get_chroma_mix(1, m));
	CHECK(m[3] == 0);
}

static void walk_refusals()
{
	// a model that needs a general-form bank; rows walked in parts at 4:2:2; several devices: error 38, nothing moves
	uint32_t s0[4], s1[4];
	unsigned long long n0 = 0, n1 = 0;
	{
		program(10, 2, 2, false);
		OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
		Frame f(512, 64, 10, 2, 2);
		DevFrame d(f);
		last_kernel_is("", &n0);
		vfgs_hip_get_seed_state(s0);
		CHECK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr) == 38 && vfgs_hip_last_error() == 38);
		CHECK(vfgs_hip_add_grain_copy_dev(d.Y, d.U, d.V, d.Y, d.U, d.V, f.w, f.h, 0, f.h, f.stride, f.cstride, 1, 0, 0, nullptr) == 38);
		vfgs_hip_frame_ptrs l = {d.Y, d.U, d.V};
		CHECK(vfgs_hip_add_grain_frame_list_dev(&l, 1, f.w, f.h, f.stride, f.cstride, nullptr) == 38);
		void *Y = f.Y.data(), *U = f.U.data(), *V = f.V.data();
		const Frame before = f;
		CHECK(vfgs_hip_add_grain_frames_host(&Y, &U, &V, 1, f.w, f.h, f.stride, f.cstride) == 38);
		vfgs_hip_get_seed_state(s1);
		last_kernel_is("", &n1);
		CHECK(!memcmp(s0, s1, sizeof s0) && n0 == n1 && d.holds(f) && f.same(before));
		vfgs_hip_clear_chroma_mix();
		OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr));
	}
	{
		program(10, 2, 1, true);
		OK(vfgs_hip_set_chroma_mix(2, 32, 32, 0));
		Frame f(8400, 32, 10, 2, 1);
		DevFrame d(f);
		vfgs_hip_get_seed_state(s0);
		CHECK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr) == 38);
		vfgs_hip_get_seed_state(s1);
		CHECK(!memcmp(s0, s1, sizeof s0) && d.holds(f));
	}
	{
		program(8, 2, 2, true);
		OK(vfgs_hip_set_chroma_mix(1, 64, 0, 0));
		const int two[2] = {0, 1}, one[1] = {0};
		OK(vfgs_hip_init_devices(two, 2));
		Frame f(1280, 720, 8, 2, 2);
		const Frame before = f;
		void *Y = f.Y.data(), *U = f.U.data(), *V = f.V.data();
		vfgs_hip_get_seed_state(s0);
		CHECK(vfgs_hip_add_grain_frames_host(&Y, &U, &V, 1, f.w, f.h, f.stride, f.cstride) == 38);
		vfgs_hip_get_seed_state(s1);
		CHECK(!memcmp(s0, s1, sizeof s0) && f.same(before));
		// the device-pointer entries stay on the primary device and work
		DevFrame d(f);
		OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr));
		OK(vfgs_hip_init_devices(one, 1));
		OK(vfgs_hip_add_grain_frames_host(&Y, &U, &V, 1, f.w, f.h, f.stride, f.cstride));
		CHECK(f.same(before));
	}
	vfgs_hip_clear_chroma_mix();
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"set_get_clear", walk_set_get_clear},
		{"device_entries", walk_device_entries},
		{"host_entries", walk_host_entries},
		{"firmware_switch_two_threads", walk_firmware_switch_from_two_threads},
		{"refusals", walk_refusals},
	});
}
