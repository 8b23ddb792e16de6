// TEST INFRASTRUCTURE.  The frame lists with a seed per picture (include/vfgs_hip.h: vfgs_hip_add_grain_frame_list_seeded_*) in the host
// layer of libvfgs_hip, compiled with a sanitizer over tests/sanitize/hip_stub.cpp, as tests/sanitize/host_walks.cpp drives the rest of it:
// whole lists, parts, out of place, the narrowed destination, more frames than a launch holds, images of many calls queued on two streams
// (slots of the images' ring reused), an overlap region, seeded calls between vfgs_set_seed and unseeded batches, the refusals, and two
// devices with a host-memory call behind a seeded list.  The stub's "kernel" copies rows unchanged and aborts when a launch addresses LFSR
// bits behind the image it was handed; the seed registers are compared with those of the contract's loop
// (vfgs_set_seed(seeds[f]); vfgs_hip_add_grain_frame_dev(frame f)) run through the same library.  Values are the GPU suite's business.
//
// usage: seeded_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 34
#include "../sanitize/walks.h"

using Pool = FramePool;

static std::vector<vfgs_hip_frame_ptrs> at_line(const Pool& pool, const Frame& f, int y)
{
	std::vector<vfgs_hip_frame_ptrs> l;
	for (const auto& d : pool.fr)
		l.push_back({d->Y + (size_t)y * f.stride * f.sz, d->U + (size_t)(y / f.sy) * f.cstride * f.sz, d->V + (size_t)(y / f.sy) * f.cstride * f.sz});
	return l;
}

// the registers the contract's loop leaves, through the single-frame entry point of the same library
static Regs loop_regs(const Frame& f, const std::vector<uint32_t>& seeds)
{
	DevFrame d(f);
	for (uint32_t s : seeds)
	{
		vfgs_set_seed(s);
		OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr));
	}
	hipDeviceSynchronize();
	return Regs();
}

static uint64_t stat(int i)
{
	uint64_t st[4];
	vfgs_hip_get_seeded_stream_stats(st);
	return st[i];
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_entries()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	// width, height, depth, subsampling, one-pattern model (general-form luma at depth 10: launches of few luma tasks)
	const int cases[][6] = {{200, 150, 10, 2, 2, 1}, {520, 70, 8, 2, 2, 0}, {333, 80, 10, 1, 1, 1}, {1042, 96, 12, 2, 1, 1}, {8400, 48, 10, 2, 2, 0}, {346, 160, 8, 1, 2, 1}};
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], depth = c[2], sx = c[3], sy = c[4], n = 5;
		program(depth, sx, sy, c[5] != 0);
		Frame f(w, h, depth, sx, sy);
		const std::vector<uint32_t> seeds = seeds_of(n);
		const Regs want = loop_regs(f, seeds);
		Pool pool(f, n), out(f, n);
		vfgs_set_seed(99);
		OK(vfgs_hip_add_grain_frame_list_seeded_dev(pool.list.data(), seeds.data(), n, w, h, f.stride, f.cstride, st));
		CHECK(Regs() == want && stat(3) == 1);
		// parts: the first block rows, a part below line 0 whose last block row is partial, the tail; each leaves the registers of whole frames
		const int parts[][2] = {{0, 32}, {16, h - 16 - 3}, {32, h - 32}};
		for (const auto& p : parts)
		{
			vfgs_set_seed(7);
			const auto l = at_line(pool, f, p[0]);
			OK(vfgs_hip_add_grain_frame_list_seeded_part_dev(l.data(), seeds.data(), n, w, h, p[0], p[1], f.stride, f.cstride, st));
			CHECK(Regs() == want);
		}
		OK(vfgs_hip_add_grain_frame_list_seeded_copy_dev(pool.list.data(), out.list.data(), seeds.data(), n, w, h, f.stride, f.cstride, st));
		CHECK(Regs() == want);
		if (depth == 10)
		{
			std::vector<std::unique_ptr<DevFrame>> d8;
			std::vector<vfgs_hip_frame_ptrs> l8;
			for (int i = 0; i < n; i++) { d8.emplace_back(new DevFrame((size_t)f.stride * h, (size_t)f.cstride * f.ch)); l8.push_back({d8.back()->Y, d8.back()->U, d8.back()->V}); }
			OK(vfgs_hip_add_grain_frame_list_seeded_copy8_dev(pool.list.data(), l8.data(), seeds.data(), n, w, h, f.stride, f.cstride, f.stride, f.cstride, st));
			CHECK(Regs() == want);
			hipStreamSynchronize(st);
		}
		// a list without seeds continues the last picture's stream
		OK(vfgs_hip_add_grain_frame_list_dev(pool.list.data(), 2, w, h, f.stride, f.cstride, st));
		CHECK(stat(3) == 0);
		hipStreamSynchronize(st);
		CHECK(pool.all_hold(f) && out.all_hold(f));
	}
	hipStreamDestroy(st);
}

static void walk_seventy_frames()
{
	program(10, 2, 2, true);
	Frame f(200, 150, 10, 2, 2);
	const std::vector<uint32_t> seeds = seeds_of(70);
	const Regs want = loop_regs(f, seeds);
	Pool pool(f, 70);
	const uint64_t built = stat(0);
	vfgs_hip_launch_info a, b;
	CHECK(vfgs_hip_last_launch_info(&a) == 0);
	OK(vfgs_hip_add_grain_frame_list_seeded_dev(pool.list.data(), seeds.data(), 70, f.w, f.h, f.stride, f.cstride, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 3 && b.nframes == 6 && b.listed == 1);
	CHECK(Regs() == want && stat(0) - built == 3 && stat(1) == 6 * 9);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f));
}

static void walk_slot_reuse()
{
	// every image in a slot of its own: twelve calls queued on two streams turn the ring of four over three times while nothing has run
	setenv("VFGS_HIP_SEEDED_SLOT_KB", "0", 1);
	void* st[2] = {nullptr, nullptr};
	hipStreamCreateWithFlags(&st[0], 1);
	hipStreamCreateWithFlags(&st[1], 1);
	program(10, 2, 2, false);
	Frame f(200, 150, 10, 2, 2);
	std::vector<std::unique_ptr<Pool>> pools;
	std::vector<uint32_t> last;
	const uint64_t built = stat(0);
	for (int c = 0; c < 12; c++)
	{
		const int n = 1 + c % 4 * 3;      // (images of different sizes: slots grow)
		pools.emplace_back(new Pool(f, n));
		last = seeds_of(n);
		OK(vfgs_hip_add_grain_frame_list_seeded_dev(pools.back()->list.data(), last.data(), n, f.w, f.h, f.stride, f.cstride, st[c & 1]));
	}
	CHECK(stat(0) - built == 12);
	// the default again: the images of the next calls share a slot
	unsetenv("VFGS_HIP_SEEDED_SLOT_KB");
	for (int c = 0; c < 12; c++)
		OK(vfgs_hip_add_grain_frame_list_seeded_dev(pools[c]->list.data(), last.data(), 1, f.w, f.h, f.stride, f.cstride, st[c & 1]));
	hipStreamSynchronize(st[0]);
	hipStreamSynchronize(st[1]);
	for (const auto& p : pools) CHECK(p->all_hold(f));
	const Regs got;
	CHECK(got == loop_regs(f, {last[0]}));
	hipStreamDestroy(st[0]);
	hipStreamDestroy(st[1]);
}

static void walk_overlap_region()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	program(10, 2, 2, true);
	Frame f(520, 70, 10, 2, 2);
	const std::vector<uint32_t> sa = seeds_of(4), sb = seeds_of(3);
	std::vector<uint32_t> all = sa;
	all.insert(all.end(), sb.begin(), sb.end());
	const Regs want = loop_regs(f, all);
	Pool a(f, 4), b(f, 3);
	DevFrame d(f);
	vfgs_set_seed(3);
	OK(vfgs_hip_overlap_begin(st));
	OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, st));
	OK(vfgs_hip_add_grain_frame_list_seeded_dev(a.list.data(), sa.data(), 4, f.w, f.h, f.stride, f.cstride, st));
	OK(vfgs_hip_add_grain_frame_list_seeded_dev(b.list.data(), sb.data(), 3, f.w, f.h, f.stride, f.cstride, st));
	OK(vfgs_hip_overlap_end(st));
	CHECK(Regs() == want);
	OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, st));
	hipStreamSynchronize(st);
	CHECK(a.all_hold(f) && b.all_hold(f) && d.holds(f));
	hipStreamDestroy(st);
}

static void walk_interleaved()
{
	// seeded lists between vfgs_set_seed, single frames and unseeded batches of stripes (the stream of jumps, whose chain a new seed ends)
	program(10, 2, 2, true);
	Frame f(1920, 272, 10, 2, 2);
	Pool pool(f, 8);
	const auto part = at_line(pool, f, 64);
	for (int round = 0; round < 3; round++)
	{
		const std::vector<uint32_t> seeds = seeds_of(8);
		OK(vfgs_hip_add_grain_frame_list_seeded_dev(pool.list.data(), seeds.data(), 8, f.w, f.h, f.stride, f.cstride, nullptr));
		const Regs a;
		for (int k = 0; k < 3; k++) OK(vfgs_hip_add_grain_frame_list_part_dev(part.data(), 8, f.w, f.h, 64, 32, f.stride, f.cstride, nullptr));
		OK(vfgs_hip_add_grain_frame_list_seeded_part_dev(part.data(), seeds.data(), 8, f.w, f.h, 64, 32, f.stride, f.cstride, nullptr));
		CHECK(Regs() == a);
		vfgs_set_seed(round);
		OK(vfgs_hip_add_grain_frame_dev(pool.fr[0]->Y, pool.fr[0]->U, pool.fr[0]->V, f.w, f.h, f.stride, f.cstride, nullptr));
		OK(vfgs_hip_add_grain_frame_list_seeded_dev(pool.list.data(), seeds.data(), 1, f.w, f.h, f.stride, f.cstride, nullptr));
		OK(vfgs_hip_add_grain_frame_list_dev(pool.list.data(), 8, f.w, f.h, f.stride, f.cstride, nullptr));
	}
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f));
}

static void walk_refusals()
{
	program(10, 2, 2, false);
	Frame f(520, 70, 10, 2, 2);
	Pool pool(f, 3);
	const std::vector<uint32_t> seeds = seeds_of(3);
	const Regs before;
	const uint64_t built = stat(0);
	vfgs_hip_launch_info a, b;
	const bool had = vfgs_hip_last_launch_info(&a) == 0;
	auto L = pool.list;
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), nullptr, 3, f.w, f.h, f.stride, f.cstride, nullptr) == 39 && vfgs_hip_last_error() == 39);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_part_dev(L.data(), nullptr, 3, f.w, f.h, 16, 16, f.stride, f.cstride, nullptr) == 39);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_copy_dev(L.data(), L.data(), nullptr, 3, f.w, f.h, f.stride, f.cstride, nullptr) == 39);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_copy8_dev(L.data(), L.data(), nullptr, 3, f.w, f.h, f.stride, f.cstride, f.stride, f.cstride, nullptr) == 39);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(nullptr, seeds.data(), 3, f.w, f.h, f.stride, f.cstride, nullptr) == 18);
	L[2] = L[0];
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 3, f.w, f.h, f.stride, f.cstride, nullptr) == 18);
	L = pool.list; L[1].U = nullptr;
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 3, f.w, f.h, f.stride, f.cstride, nullptr) == 18);
	L = pool.list; L[1].Y = (uint8_t*)L[1].Y + 8;
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 3, f.w, f.h, f.stride, f.cstride, nullptr) == 7);
	L = pool.list;
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 3, f.w, f.h, 512, f.cstride, nullptr) == 6);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_part_dev(L.data(), seeds.data(), 3, f.w, f.h, 24, 16, f.stride, f.cstride, nullptr) == 11);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_part_dev(L.data(), seeds.data(), 3, f.w, f.h, 16, 0xFFFFFFFFu, f.stride, f.cstride, nullptr) == 12);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 3, 100, f.h, f.stride, f.cstride, nullptr) == 5);
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));     // a general-form model
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 3, f.w, f.h, f.stride, f.cstride, nullptr) == 38);
	vfgs_hip_clear_chroma_mix();
	vfgs_set_depth(8);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_copy8_dev(L.data(), L.data(), seeds.data(), 3, f.w, f.h, f.stride, f.cstride, f.stride, f.cstride, nullptr) == 16);
	vfgs_set_depth(10);
	unsigned char lut[256];
	memset(lut, 0x90, sizeof lut);                 // slot 9: undefined in the reference
	vfgs_set_pattern_lut(1, lut);
	CHECK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 3, f.w, f.h, f.stride, f.cstride, nullptr) == 4);
	memset(lut, 0x10, sizeof lut);
	vfgs_set_pattern_lut(1, lut);
	OK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 0, f.w, f.h, f.stride, f.cstride, nullptr));
	OK(vfgs_hip_add_grain_frame_list_seeded_dev(nullptr, nullptr, 0, f.w, f.h, f.stride, f.cstride, nullptr));
	CHECK(Regs() == before && stat(0) == built);
	CHECK((vfgs_hip_last_launch_info(&b) == 0) == had && (!had || a.launches == b.launches));
	// the same list is served afterwards
	const Regs want = loop_regs(f, seeds);
	vfgs_set_seed(1);
	OK(vfgs_hip_add_grain_frame_list_seeded_dev(L.data(), seeds.data(), 3, f.w, f.h, f.stride, f.cstride, nullptr));
	CHECK(Regs() == want);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f));
}

static void walk_two_devices()
{
	// a host-memory call behind a seeded list, split over two devices (device 0 listed twice): the replica takes over the list's last seed
	program(10, 2, 2, true);
	Frame f(416, 240, 10, 2, 2);
	const Frame before = f;
	const std::vector<uint32_t> seeds = seeds_of(4);
	Pool pool(f, 4);
	std::vector<Frame> fr(3, f);
	std::vector<void*> Y, U, V;
	for (auto& x : fr) { Y.push_back(x.Y.data()); U.push_back(x.U.data()); V.push_back(x.V.data()); }
	Regs got[2];
	for (int ndev = 1; ndev <= 2; ndev++)
	{
		const int devs[2] = {0, 0};
		OK(vfgs_hip_init_devices(devs, ndev));
		vfgs_set_seed(5);
		OK(vfgs_hip_add_grain_frames_host(Y.data(), U.data(), V.data(), 3, f.w, f.h, f.stride, f.cstride));
		OK(vfgs_hip_add_grain_frame_list_seeded_dev(pool.list.data(), seeds.data(), 4, f.w, f.h, f.stride, f.cstride, nullptr));
		OK(vfgs_hip_add_grain_frames_host(Y.data(), U.data(), V.data(), 3, f.w, f.h, f.stride, f.cstride));
		vfgs_add_grain_stripe(fr[0].Y.data(), fr[0].U.data(), fr[0].V.data(), 0, f.w, f.h, f.stride, f.cstride);
		got[ndev - 1] = Regs();
	}
	CHECK(got[0] == got[1]);
	for (auto& x : fr) CHECK(x.Y == before.Y && x.U == before.U && x.V == before.V);
	const int one[1] = {0};
	OK(vfgs_hip_init_devices(one, 1));
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f));
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"entries", walk_entries},
		{"seventy_frames", walk_seventy_frames},
		{"slot_reuse", walk_slot_reuse},
		{"overlap_region", walk_overlap_region},
		{"interleaved", walk_interleaved},
		{"refusals", walk_refusals},
		{"two_devices", walk_two_devices},
	});
}
