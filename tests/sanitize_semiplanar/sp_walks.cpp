// TEST INFRASTRUCTURE.  Semi-planar frames (include/vfgs_hip.h: vfgs_hip_add_grain_sp_frame_list_dev) in the host layer of libvfgs_hip,
// compiled with a sanitizer over tests/sanitize/hip_stub.cpp, as tests/sanitize_seeded/seeded_walks.cpp drives the seeded lists: in place,
// out of place, with and without seeds, both sample shifts, odd block counts, more frames than a launch holds, an overlap region, every
// refusal, two threads calling at once.  The stub's "kernel" copies rows unchanged and touches exactly the bytes the real one addresses --
// for these launches the UV plane's whole-block rows, through components 1 and 2 alike -- so planes allocated exactly as large as the
// contract says make every wrong extent or pitch a sanitizer report.  The seed registers are compared with those of the planar list calls
// on planar frames of the same size, through the same library.  Values are the GPU suite's business (tests/test_gpu_semiplanar.py).
//
// usage: sp_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 77
#include "../sanitize/walks.h"

using Pic = SpPic;
using Pool = SpPool;

static bool sp_kernel_named(const vfgs_hip_launch_info& li)
{
	return !strncmp(li.kernel, "grain_sp_kernel<", 16) && li.listed == 1 && li.persistent_luma_workgroups == 0;     // (the host formats the name itself)
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_entries()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	// width, height, depth, csuby, one-pattern model, sample shift, row padding in containers: odd block counts (13, 33, 65, 129), a single
	// block row, the widest row, both shifts, every depth
	const int cases[][7] = {{200, 150, 10, 2, 1, 6, 0}, {520, 70, 8, 2, 0, 0, 16}, {1032, 33, 10, 1, 0, 0, 8}, {1042, 96, 12, 1, 1, 4, 0}, {8192, 17, 10, 2, 0, 6, 0},
	                        {2056, 16, 8, 1, 1, 0, 0}, {136, 40, 12, 2, 0, 0, 24}};
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], depth = c[2], sy = c[3], shift = c[5], n = 5;
		program(depth, 2, sy, c[4] != 0);
		Pic f(w, h, sy, depth > 8 ? 2 : 1, c[6], c[6]);
		const std::vector<uint32_t> seeds = seeds_of(n);
		// in place, one seed sequence
		vfgs_set_seed(99);
		const Regs want_plain = planar_regs(f, n, nullptr);
		Pool pool(f, n), out(f, n);
		vfgs_set_seed(99);
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), nullptr, n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_plain);
		vfgs_hip_launch_info li;
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && sp_kernel_named(li) && li.nframes == n && li.in_place == 1 && li.depth == depth);
		// in place, a seed per picture
		const Regs want_seeded = planar_regs(f, n, seeds.data());
		vfgs_set_seed(7);
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_seeded);
		// out of place, seeded and not; one pair in place
		auto dst = out.list;
		dst[3] = pool.list[3];
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), dst.data(), seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_seeded);
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && li.in_place == 0);
		vfgs_set_seed(99);
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), dst.data(), nullptr, n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_plain);
		hipStreamSynchronize(st);
		CHECK(pool.all_hold(f) && out.all_hold(f));
	}
	hipStreamDestroy(st);
}

static void walk_seventy_frames()
{
	program(10, 2, 2, true);
	Pic f(264, 40, 2, 2);
	const std::vector<uint32_t> seeds = seeds_of(70);
	const Regs want = planar_regs(f, 70, seeds.data());
	Pool pool(f, 70);
	vfgs_hip_launch_info a, b;
	CHECK(vfgs_hip_last_launch_info(&a) == 0);
	OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), seeds.data(), 70, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 3 && b.nframes == 6 && b.listed == 1);
	CHECK(Regs() == want);
	vfgs_set_seed(5);
	const Regs want2 = planar_regs(f, 70, nullptr);
	vfgs_set_seed(5);
	CHECK(vfgs_hip_last_launch_info(&a) == 0);
	OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), nullptr, 70, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 3 && b.nframes == 6);
	CHECK(Regs() == want2);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f));
}

static void walk_overlap_region()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	program(10, 2, 2, true);
	Pic f(520, 70, 2, 2);
	const std::vector<uint32_t> sb = seeds_of(3);
	vfgs_set_seed(3);
	planar_regs(f, 4, nullptr);
	const Regs want = planar_regs(f, 3, sb.data());
	Pool a(f, 4), b(f, 3);
	vfgs_set_seed(3);
	OK(vfgs_hip_overlap_begin(st));
	OK(vfgs_hip_add_grain_sp_frame_list_dev(a.list.data(), a.list.data(), nullptr, 4, f.w, f.h, f.stride, f.uv_stride, 6, st));
	OK(vfgs_hip_add_grain_sp_frame_list_dev(b.list.data(), b.list.data(), sb.data(), 3, f.w, f.h, f.stride, f.uv_stride, 6, st));
	OK(vfgs_hip_add_grain_sp_frame_list_dev(a.list.data(), a.list.data(), sb.data(), 3, f.w, f.h, f.stride, f.uv_stride, 6, st));
	OK(vfgs_hip_overlap_end(st));
	CHECK(Regs() == want);
	hipStreamSynchronize(st);
	CHECK(a.all_hold(f) && b.all_hold(f));
	hipStreamDestroy(st);
}

static void walk_refusals()
{
	program(10, 2, 2, false);
	Pic f(520, 70, 2, 2);
	Pool pool(f, 3), other(f, 3);
	const std::vector<uint32_t> seeds = seeds_of(3);
	const Regs before;
	vfgs_hip_launch_info a, b;
	const bool had = vfgs_hip_last_launch_info(&a) == 0;
	const unsigned w = f.w, h = f.h, s = f.stride, u = f.uv_stride;
	auto call = [&](const vfgs_hip_sp_frame* src, const vfgs_hip_sp_frame* dst, unsigned ww = 520, unsigned ss = 0, unsigned uu = 0, unsigned shift = 6) {
		const int rc = vfgs_hip_add_grain_sp_frame_list_dev(src, dst, seeds.data(), 3, ww, h, ss ? ss : s, uu ? uu : u, shift, nullptr);
		CHECK(rc == vfgs_hip_last_error());
		return rc;
	};
	auto L = pool.list, D = other.list;
	(void)w;
	CHECK(call(nullptr, L.data()) == 18 && call(L.data(), nullptr) == 18);
	L[1].UV = nullptr;
	CHECK(call(L.data(), L.data()) == 18);
	L = pool.list; L[1].Y = nullptr;
	CHECK(call(L.data(), L.data()) == 18);
	L = pool.list; L[1].UV = (uint8_t*)L[1].UV + 8;
	CHECK(call(L.data(), L.data()) == 7);
	L = pool.list; D[2].Y = (uint8_t*)D[2].Y + 4;
	CHECK(call(L.data(), D.data()) == 7);
	D = other.list;
	CHECK(call(L.data(), L.data(), 520, 512) == 6 && call(L.data(), L.data(), 520, 0, 512) == 6);
	CHECK(call(L.data(), L.data(), 520, s + 4) == 8 && call(L.data(), L.data(), 520, 0, u + 4) == 8);
	CHECK(call(L.data(), L.data(), 100) == 5);
	L[2] = L[0];
	CHECK(call(L.data(), L.data()) == 18);                   // a destination listed twice
	L = pool.list; D[1].UV = D[0].Y;
	CHECK(call(L.data(), D.data()) == 18);                   // a UV plane that is another frame's Y
	D = other.list; D[1].UV = (uint8_t*)D[0].Y + 2048;
	CHECK(call(L.data(), D.data()) == 18);                   // ... that overlaps it
	D = other.list; D[1].UV = L[2].UV;
	CHECK(call(L.data(), D.data()) == 18);                   // a source plane of frame 2 is frame 1's destination
	D = other.list;
	// what this call alone refuses
	CHECK(call(L.data(), L.data(), 520, 0, 0, 4) == 40 && call(L.data(), L.data(), 520, 0, 0, 16) == 40);
	CHECK(call(L.data(), L.data(), 8208, 8208, 8208) == 40);
	vfgs_set_depth(8);
	CHECK(call(L.data(), L.data(), 520, 0, 0, 8) == 40 && call(L.data(), L.data(), 520, 0, 0, 6) == 40);
	vfgs_set_depth(10);
	vfgs_set_chroma_subsampling(1, 1);
	CHECK(call(L.data(), L.data()) == 40);
	vfgs_set_chroma_subsampling(1, 2);
	CHECK(call(L.data(), L.data()) == 40);
	vfgs_set_chroma_subsampling(2, 2);
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	CHECK(call(L.data(), L.data()) == 40);
	vfgs_hip_clear_chroma_mix();
	unsigned char lut[256];
	memset(lut, 0x90, sizeof lut);                 // slot 9: undefined in the reference
	vfgs_set_pattern_lut(1, lut);
	CHECK(call(L.data(), L.data()) == 4);
	for (int i = 0; i < 256; i++) lut[i] = (unsigned char)((i >> 5) << 4);
	vfgs_set_pattern_lut(1, lut);
	OK(vfgs_hip_add_grain_sp_frame_list_dev(L.data(), L.data(), seeds.data(), 0, w, h, s, u, 6, nullptr));
	OK(vfgs_hip_add_grain_sp_frame_list_dev(nullptr, nullptr, nullptr, 0, 100, h, 0, 0, 99, nullptr));
	CHECK(Regs() == before);
	CHECK((vfgs_hip_last_launch_info(&b) == 0) == had && (!had || a.launches == b.launches));
	// the same list is served afterwards
	const Regs want = planar_regs(f, 3, seeds.data());
	vfgs_set_seed(1);
	OK(vfgs_hip_add_grain_sp_frame_list_dev(L.data(), L.data(), seeds.data(), 3, w, h, s, u, 6, nullptr));
	CHECK(Regs() == want);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f) && other.all_hold(f));
}

static void walk_two_threads()
{
	// two threads, a pool and a stream each, calling at once: the library serialises them; with a seed per picture the order does not
	// show in the registers a thread's last call leaves only if both end on the same seed
	program(10, 2, 2, true);
	Pic f(520, 70, 2, 2);
	const std::vector<uint32_t> seeds = seeds_of(6);
	const Regs want = planar_regs(f, 6, seeds.data());
	Pool pa(f, 6), pb(f, 6);
	void* st[2] = {nullptr, nullptr};
	hipStreamCreateWithFlags(&st[0], 1);
	hipStreamCreateWithFlags(&st[1], 1);
	int rc[2] = {0, 0};
	auto work = [&](int t, Pool* p) {
		for (int k = 0; k < 8 && !rc[t]; k++)
			rc[t] = vfgs_hip_add_grain_sp_frame_list_dev(p->list.data(), p->list.data(), seeds.data(), 6, f.w, f.h, f.stride, f.uv_stride, 6, st[t]);
	};
	std::thread ta(work, 0, &pa), tb(work, 1, &pb);
	ta.join(); tb.join();
	CHECK(rc[0] == 0 && rc[1] == 0);
	CHECK(Regs() == want);
	hipStreamSynchronize(st[0]);
	hipStreamSynchronize(st[1]);
	CHECK(pa.all_hold(f) && pb.all_hold(f));
	hipStreamDestroy(st[0]);
	hipStreamDestroy(st[1]);
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"entries", walk_entries},
		{"seventy_frames", walk_seventy_frames},
		{"overlap_region", walk_overlap_region},
		{"refusals", walk_refusals},
		{"two_threads", walk_two_threads},
	});
}
