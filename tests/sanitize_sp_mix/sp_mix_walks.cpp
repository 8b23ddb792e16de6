// TEST INFRASTRUCTURE.  Semi-planar frames under an active luma / chroma mix (include/vfgs_hip.h: vfgs_hip_add_grain_sp_frame_list_dev with
// vfgs_hip_set_chroma_mix) in the host layer of libvfgs_hip, compiled with a sanitizer over tests/sanitize/hip_stub.cpp, as
// tests/sanitize_semiplanar/sp_walks.cpp drives the call without a mix: a one-pattern model with a mix in place (two launches counted) and
// out of place (one launch), seeded and unseeded, 35 frames; the registers of the planar copy list under the same mix; planes allocated
// exactly as large as the contract says; a general-form model and depth 12 under a mix refused with 40 and nothing changed; two threads.
// The stub's "kernel" copies rows unchanged and touches exactly the bytes the real one addresses.  Values are the GPU suite's business
// (tests/test_gpu_semiplanar_mix.py).
//
// usage: sp_mix_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 177
#include "../sanitize/walks.h"

using Pic = SpPic;
using Pool = SpPool;

// a model, then the mix: Cb alone, Cr alone or both (bit 0 / bit 1 of `mix`)
static void program_mix(int depth, int sy, bool one_pattern, int mix)
{
	Model m{depth, 2, sy, one_pattern, one_pattern};
	m.mix = mix;
	program(m);
}

static bool sp_mix_kernel_named(const vfgs_hip_launch_info& li, int depth, int sy)
{
	char want[64];
	snprintf(want, sizeof want, "grain_sp_mix_kernel<%d,%d>", depth, sy);
	return !strcmp(li.kernel, want) && li.listed == 1 && li.one_y == 1 && li.one_c == 1 && li.persistent_luma_workgroups == 0 &&
	       li.lds_bytes_per_workgroup == 53248;     // (the host formats the name itself)
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_entries()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	// width, height, depth, csuby, mix (1 Cb, 2 Cr, 3 both), sample shift, row padding in containers: odd block counts, an odd width, a single
	// block row, the widest row, both shifts, both depths, both formats
	const int cases[][7] = {{200, 150, 10, 2, 3, 6, 0}, {520, 70, 8, 2, 1, 0, 16}, {1032, 33, 10, 1, 2, 0, 8}, {333, 17, 8, 1, 3, 0, 0}, {8192, 17, 10, 2, 3, 6, 0},
	                        {2056, 16, 8, 2, 2, 0, 0}, {136, 41, 10, 1, 1, 6, 24}};
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], depth = c[2], sy = c[3], shift = c[5], n = 5;
		program_mix(depth, sy, true, c[4]);
		Pic f(w, h, sy, depth > 8 ? 2 : 1, c[6], c[6]);
		const std::vector<uint32_t> seeds = seeds_of(n);
		vfgs_set_seed(99);
		const Regs want_plain = planar_regs(f, n, nullptr, PLANAR_LIST_COPY);
		const Regs want_seeded = planar_regs(f, n, seeds.data(), PLANAR_LIST_COPY);
		Pool pool(f, n), out(f, n);
		vfgs_hip_launch_info li;
		// in place, one seed sequence: UV first, then luma
		vfgs_set_seed(99);
		unsigned long long n0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), nullptr, n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_plain);
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && sp_mix_kernel_named(li, depth, sy) && li.launches - n0 == 2 && li.nframes == n && li.in_place == 1 && li.depth == depth);
		// in place, a seed per picture
		vfgs_set_seed(7);
		n0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_seeded && launches() - n0 == 2);
		// out of place, seeded and not: one launch
		n0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), out.list.data(), seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_seeded);
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && sp_mix_kernel_named(li, depth, sy) && li.launches - n0 == 1 && li.in_place == 0);
		vfgs_set_seed(99);
		n0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), out.list.data(), nullptr, n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_plain && launches() - n0 == 1);
		// one pair in place, and destination Y == source Y with UV elsewhere: luma is a hazard, two launches
		auto dst = out.list;
		dst[3] = pool.list[3];
		n0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), dst.data(), seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_seeded && launches() - n0 == 2);
		dst = out.list;
		for (int i = 0; i < n; i++) dst[i].Y = pool.list[i].Y;
		n0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), dst.data(), seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_seeded && launches() - n0 == 2);
		hipStreamSynchronize(st);
		CHECK(pool.all_hold(f) && out.all_hold(f));
		// after the mix is cleared the launch is the one of always
		vfgs_hip_clear_chroma_mix();
		n0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), nullptr, n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && !strncmp(li.kernel, "grain_sp_kernel<", 16) && li.launches - n0 == 1);
		hipStreamSynchronize(st);
	}
	hipStreamDestroy(st);
}

static void walk_thirty_five_frames()
{
	program_mix(10, 2, true, 3);
	Pic f(264, 40, 2, 2);
	const std::vector<uint32_t> seeds = seeds_of(35);
	const Regs want = planar_regs(f, 35, seeds.data(), PLANAR_LIST_COPY);
	Pool pool(f, 35), out(f, 35);
	vfgs_hip_launch_info b;
	unsigned long long n0 = launches();
	OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), seeds.data(), 35, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - n0 == 4 && b.nframes == 3 && b.listed == 1);     // 32 + 3 frames, two launches each
	CHECK(Regs() == want);
	vfgs_set_seed(5);
	const Regs want2 = planar_regs(f, 35, nullptr, PLANAR_LIST_COPY);
	vfgs_set_seed(5);
	n0 = launches();
	OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), out.list.data(), nullptr, 35, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - n0 == 2 && b.nframes == 3);                      // out of place: one each
	CHECK(Regs() == want2);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f) && out.all_hold(f));
}

static void walk_overlap_region()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	program_mix(8, 2, true, 3);
	Pic f(520, 70, 2, 1);
	const std::vector<uint32_t> sb = seeds_of(3);
	vfgs_set_seed(3);
	planar_regs(f, 4, nullptr, PLANAR_LIST_COPY);
	const Regs want = planar_regs(f, 3, sb.data(), PLANAR_LIST_COPY);
	Pool a(f, 4), b(f, 3);
	vfgs_set_seed(3);
	OK(vfgs_hip_overlap_begin(st));
	OK(vfgs_hip_add_grain_sp_frame_list_dev(a.list.data(), a.list.data(), nullptr, 4, f.w, f.h, f.stride, f.uv_stride, 0, st));
	OK(vfgs_hip_add_grain_sp_frame_list_dev(b.list.data(), b.list.data(), sb.data(), 3, f.w, f.h, f.stride, f.uv_stride, 0, st));
	OK(vfgs_hip_overlap_end(st));
	CHECK(Regs() == want);
	hipStreamSynchronize(st);
	CHECK(a.all_hold(f) && b.all_hold(f));
	hipStreamDestroy(st);
}

static void walk_refusals()
{
	Pic f(520, 70, 2, 2);
	const std::vector<uint32_t> seeds = seeds_of(3);
	auto refused = [&](Pool& pool, unsigned shift, const char* cause) {
		const Regs before;
		const unsigned long long n0 = launches();
		for (const uint32_t* sd : {seeds.data(), (const uint32_t*)nullptr})
		{
			const int rc = vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), sd, 3, f.w, f.h, f.stride, f.uv_stride, shift, nullptr);
			CHECK(rc == 40 && rc == vfgs_hip_last_error());
			CHECK(strstr(vfgs_hip_last_error_string(), "chroma mix") && strstr(vfgs_hip_last_error_string(), cause));
		}
		CHECK(Regs() == before && launches() == n0);
		hipDeviceSynchronize();
		CHECK(pool.all_hold(f));
	};
	// a general-form model under a mix
	program_mix(10, 2, false, 1);
	{
		Pool pool(f, 3);
		refused(pool, 6, "general-form");
		// ... the planar call refuses the same case with its own code
		const size_t cs = (size_t)f.nblk * 16;
		uint8_t *y, *u, *v;
		hipMalloc((void**)&y, (size_t)f.h * cs * 2); hipMalloc((void**)&u, f.crows * cs * 2); hipMalloc((void**)&v, f.crows * cs * 2);
		vfgs_hip_frame_ptrs p{y, u, v};
		CHECK(vfgs_hip_add_grain_frame_list_dev(&p, 1, f.w, f.h, f.nblk * 16, (unsigned)cs, nullptr) == 38);
		hipFree(y); hipFree(u); hipFree(v);
		// the same list is served once the mix is off
		vfgs_hip_clear_chroma_mix();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), seeds.data(), 3, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));
		hipDeviceSynchronize();
	}
	// depth 12 under a mix (P012: shift 4)
	program_mix(12, 2, true, 3);
	{
		Pool pool(f, 3);
		refused(pool, 4, "depth is 12");
		refused(pool, 0, "depth is 12");
		// ... and at depth 10 the same model and list are served
		vfgs_set_depth(10);
		const Regs want = planar_regs(f, 3, seeds.data(), PLANAR_LIST_COPY);
		vfgs_set_seed(1);
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), seeds.data(), 3, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));
		CHECK(Regs() == want);
		hipDeviceSynchronize();
		CHECK(pool.all_hold(f));
		// several devices set: the call is a device-pointer call, stays on the primary device and honours the mix there
		const int two[2] = {0, 1}, one[1] = {0};
		OK(vfgs_hip_init_devices(two, 2));
		const unsigned long long n0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), seeds.data(), 3, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));
		vfgs_hip_launch_info li;
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && sp_mix_kernel_named(li, 10, 2) && li.launches - n0 == 2 && Regs() == want);
		hipDeviceSynchronize();
		OK(vfgs_hip_init_devices(one, 1));
	}
}

static void walk_two_threads()
{
	// two threads, a pool and a stream each, calling at once: the library serialises them; with a seed per picture the order does not
	// show in the registers a thread's last call leaves only if both end on the same seed.  One thread in place, one out of place.
	program_mix(10, 2, true, 3);
	Pic f(520, 70, 2, 2);
	const std::vector<uint32_t> seeds = seeds_of(6);
	const Regs want = planar_regs(f, 6, seeds.data(), PLANAR_LIST_COPY);
	Pool pa(f, 6), pb(f, 6), pc(f, 6);
	void* st[2] = {nullptr, nullptr};
	hipStreamCreateWithFlags(&st[0], 1);
	hipStreamCreateWithFlags(&st[1], 1);
	int rc[2] = {0, 0};
	auto work = [&](int t, Pool* s, Pool* d) {
		for (int k = 0; k < 8 && !rc[t]; k++)
			rc[t] = vfgs_hip_add_grain_sp_frame_list_dev(s->list.data(), d->list.data(), seeds.data(), 6, f.w, f.h, f.stride, f.uv_stride, 6, st[t]);
	};
	std::thread ta(work, 0, &pa, &pa), tb(work, 1, &pb, &pc);
	ta.join(); tb.join();
	CHECK(rc[0] == 0 && rc[1] == 0);
	CHECK(Regs() == want);
	hipStreamSynchronize(st[0]);
	hipStreamSynchronize(st[1]);
	CHECK(pa.all_hold(f) && pb.all_hold(f) && pc.all_hold(f));
	hipStreamDestroy(st[0]);
	hipStreamDestroy(st[1]);
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"entries", walk_entries},
		{"thirty_five_frames", walk_thirty_five_frames},
		{"overlap_region", walk_overlap_region},
		{"refusals", walk_refusals},
		{"two_threads", walk_two_threads},
	});
}
