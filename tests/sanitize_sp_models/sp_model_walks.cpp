// TEST INFRASTRUCTURE.  Semi-planar frames with a model per picture (include/vfgs_hip.h: vfgs_hip_add_grain_sp_frame_list_models_dev) in the
// host layer of libvfgs_hip, compiled with a sanitizer over tests/sanitize/hip_stub.cpp, as tests/sanitize_models/model_walks.cpp drives the
// planar call and tests/sanitize_semiplanar/sp_walks.cpp the plain semi-planar one: in place and out of place, seeded and not, a change of
// form in the middle of a list, lists longer than a launch holds, release while everything is queued, two host threads calling on two
// streams, every refusal with nothing changed.  Planes are allocated exactly as large as the contract says, so a wrong extent or pitch is a
// sanitizer report.
//
// What the stub CANNOT prove: its "kernel" copies rows unchanged and reads KernelArgs::tables only -- frame 0's table image -- not the images
// of the other frames of a launch (FrameTable::model[]), which the stub (unchanged, and older than the field) does not know.  So the walks
// themselves read every model's device bytes -- record and image, the length vfgs_hip_model_info reports -- once everything queued has run:
// bytes that were freed or handed to another capture while a queued launch could still read them are a sanitizer report there or in the
// stub's queue.  The handle is opaque; the host layer keeps the device pointer as the structure's first member for exactly this read.
// Values are the GPU suite's business (tests/test_gpu_sp_model_list.py); the seed registers are compared with those of the planar list
// calls on planar frames of the same size, through the same library.
//
// usage: sp_model_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 53
#include "../sanitize/walks.h"

using Pic = SpPic;
using Pool = SpPool;

static bool spml_named(const vfgs_hip_launch_info& li)
{
	return !strncmp(li.kernel, "grain_spml_kernel<", 18) && li.listed == 1 && li.persistent_luma_workgroups == 0;     // (the host formats the name itself)
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

// in place and out of place, seeded and not: every depth, both chroma formats, both sample shifts, odd block counts, padded rows
static void walk_entries()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	// width, height, depth, csuby, one-pattern models, sample shift, row padding in containers
	const int cases[][7] = {{200, 150, 10, 2, 1, 6, 0}, {520, 70, 8, 2, 0, 0, 16}, {1032, 33, 10, 1, 0, 0, 8}, {1042, 96, 12, 1, 1, 4, 0}, {8192, 17, 10, 2, 0, 6, 0},
	                        {2056, 16, 8, 1, 1, 0, 0}, {136, 40, 12, 2, 0, 0, 24}};
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], depth = c[2], sy = c[3], shift = c[5], n = 5;
		program(depth, 2, sy, c[4] != 0, 4, 1);
		vfgs_hip_model* a = capture(st);
		program(depth, 2, sy, c[4] != 0);
		vfgs_hip_model* b = capture(st);
		const vfgs_hip_model* ms[5] = {a, b, b, a, b};
		Pic f(w, h, sy, depth > 8 ? 2 : 1, c[6], c[6]);
		const std::vector<uint32_t> seeds = seeds_of(n);
		vfgs_set_seed(99);
		const Regs want_plain = planar_regs(f, n, nullptr);
		Pool pool(f, n), out(f, n);
		vfgs_set_seed(99);
		unsigned long long l0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), pool.list.data(), ms, nullptr, n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_plain);
		vfgs_hip_launch_info li;
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && spml_named(li) && li.launches - l0 == 1 && li.nframes == n && li.in_place == 1 && li.depth == depth);
		CHECK(li.one_y == c[4] && li.one_c == c[4]);
		// out of place, a seed per picture; one pair in place
		const Regs want_seeded = planar_regs(f, n, seeds.data());
		auto dst = out.list;
		dst[3] = pool.list[3];
		OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), dst.data(), ms, seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(Regs() == want_seeded);
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && spml_named(li) && li.in_place == 0);
		// in place with seeds, out of place without
		OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), pool.list.data(), ms, seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), out.list.data(), ms, nullptr, n, w, h, f.stride, f.uv_stride, shift, st));
		// the programmed state is the caller's: a plain semi-planar call behind it
		OK(vfgs_hip_add_grain_sp_frame_list_dev(pool.list.data(), pool.list.data(), nullptr, 2, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && !strncmp(li.kernel, "grain_sp_kernel<", 16));
		hipStreamSynchronize(st);
		CHECK(pool.all_hold(f) && out.all_hold(f));
		touch_model(a); touch_model(b);
		vfgs_hip_model_release(a); vfgs_hip_model_release(b);
	}
	hipStreamDestroy(st);
}

// a change of form in the middle of a list, and more frames than a launch holds
static void walk_form_changes()
{
	const int cases[][4] = {{200, 150, 10, 2}, {520, 70, 8, 2}, {1042, 48, 12, 1}};
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], depth = c[2], sy = c[3], n = 70, shift = depth > 8 ? 16 - depth : 0;
		Pic f(w, h, sy, depth > 8 ? 2 : 1);
		program(depth, 2, sy, false);
		vfgs_hip_model* g = capture(st);           // general form
		program(depth, 2, sy, true, 4, 1);
		vfgs_hip_model* o1 = capture(st);          // one-pattern form
		program(depth, 2, sy, true);
		vfgs_hip_model* o2 = capture(st);
		// 3 of g, 40 alternating o1 / o2 (one form: 32 + 8), 2 of g, 25 of o1: launches 3, 32, 8, 2, 25
		std::vector<const vfgs_hip_model*> ms;
		for (int i = 0; i < 3; i++) ms.push_back(g);
		for (int i = 0; i < 40; i++) ms.push_back(i & 1 ? o1 : o2);
		for (int i = 0; i < 2; i++) ms.push_back(g);
		for (int i = 0; i < 25; i++) ms.push_back(o1);
		const std::vector<uint32_t> seeds = seeds_of(n);
		vfgs_set_seed(77);
		const Regs want_plain = planar_regs(f, n, nullptr);
		const Regs want_seeded = planar_regs(f, n, seeds.data());
		Pool pool(f, n), out(f, n);
		vfgs_set_seed(77);
		unsigned long long l0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), pool.list.data(), ms.data(), nullptr, n, w, h, f.stride, f.uv_stride, shift, st));
		vfgs_hip_launch_info li;
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && spml_named(li) && li.launches - l0 == 5 && li.nframes == 25 && li.one_y == 1 && li.one_c == 1);
		CHECK(Regs() == want_plain);
		l0 = launches();
		OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), out.list.data(), ms.data(), seeds.data(), n, w, h, f.stride, f.uv_stride, shift, st));
		CHECK(launches() - l0 == 5 && Regs() == want_seeded);
		hipStreamSynchronize(st);
		CHECK(pool.all_hold(f) && out.all_hold(f));
		for (const vfgs_hip_model* m : {g, o1, o2}) touch_model(m);
		vfgs_hip_model_release(g); vfgs_hip_model_release(o1); vfgs_hip_model_release(o2);
	}
	hipStreamDestroy(st);
}

// captured on one stream, used on another, released with everything still queued; captures in between; an overlap region
static void walk_release_while_queued()
{
	void *sa = nullptr, *sb = nullptr;
	hipStreamCreateWithFlags(&sa, 1);
	hipStreamCreateWithFlags(&sb, 1);
	Pic f(520, 70, 2, 2);
	program(10, 2, 2, true);
	vfgs_hip_model* a = capture(sa);
	vfgs_hip_model* a2 = capture(sa);
	program(10, 2, 2, true, 4, 1);
	vfgs_hip_model* b = capture(sb);
	Pool pool(f, 6);
	const vfgs_hip_model* ms[6] = {a, b, a2, b, a, b};
	// released BEFORE use: refused, nothing changed
	vfgs_hip_model_release(a2);
	const Regs r0;
	CHECK(vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), pool.list.data(), ms, nullptr, 6, f.w, f.h, f.stride, f.uv_stride, 6, sb) == 41);
	CHECK(Regs() == r0);
	ms[2] = a;
	OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), pool.list.data(), ms, nullptr, 6, f.w, f.h, f.stride, f.uv_stride, 6, sb));
	vfgs_hip_model_release(a);                     // right after the call returns
	vfgs_hip_model_release(a);                     // twice: no-op
	// captures in between take other buffers (or buffers whose readers are done): a dozen, each released at once
	for (int i = 0; i < 12; i++)
	{
		vfgs_hip_model* t = capture(i & 1 ? sa : sb);
		touch_model(t);
		vfgs_hip_model_release(t);
	}
	hipStreamSynchronize(sb);
	CHECK(pool.all_hold(f));
	touch_model(b);
	// two calls inside an overlap region, a release inside it
	program(10, 2, 2, false);
	vfgs_hip_model* c = capture(sa);
	vfgs_set_seed(3);
	const Regs want = planar_regs(f, 7, nullptr);
	Pool pa(f, 4), pb(f, 3);
	const vfgs_hip_model* ma[4] = {b, b, c, b};
	const vfgs_hip_model* mb[3] = {c, b, b};
	vfgs_set_seed(3);
	OK(vfgs_hip_overlap_begin(sa));
	OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pa.list.data(), pa.list.data(), ma, nullptr, 4, f.w, f.h, f.stride, f.uv_stride, 6, sa));
	OK(vfgs_hip_add_grain_sp_frame_list_models_dev(pb.list.data(), pb.list.data(), mb, nullptr, 3, f.w, f.h, f.stride, f.uv_stride, 6, sa));
	vfgs_hip_model_release(b);                     // inside the region, with both calls queued on its internal streams
	OK(vfgs_hip_overlap_end(sa));
	CHECK(Regs() == want);
	hipStreamSynchronize(sa);
	CHECK(pa.all_hold(f) && pb.all_hold(f));
	touch_model(c);
	vfgs_hip_model_release(c);
	hipStreamDestroy(sa);
	hipStreamDestroy(sb);
}

// two host threads calling on two streams with the same models, a third capturing and releasing
static void walk_threads()
{
	Pic f(520, 70, 2, 2);
	program(10, 2, 2, true);
	vfgs_hip_model* a = capture(nullptr);
	vfgs_hip_model* b = capture(nullptr);
	hipDeviceSynchronize();
	const vfgs_hip_model* ms[6] = {a, b, b, a, b, a};
	auto caller = [&](int k) {
		void* st = nullptr;
		hipStreamCreateWithFlags(&st, 1);
		Pool pool(f, 6), out(f, 6);
		for (int i = 0; i < 30; i++)
		{
			const std::vector<uint32_t> seeds = {1u + i, 2u, 3u + k, 4u, 5u, 6u};
			const bool oop = (i + k) & 2;
			const int rc = vfgs_hip_add_grain_sp_frame_list_models_dev(pool.list.data(), oop ? out.list.data() : pool.list.data(), ms, (i & 1) ? seeds.data() : nullptr, 6,
			                                                           f.w, f.h, f.stride, f.uv_stride, 6, st);
			if (rc) g_fail++;
			if (i % 7 == k) hipStreamSynchronize(st);
		}
		hipStreamSynchronize(st);
		if (!pool.all_hold(f) || !out.all_hold(f)) g_fail++;
		hipStreamDestroy(st);
	};
	std::atomic<bool> stop{false};
	auto capturer = [&] {
		void* st = nullptr;
		hipStreamCreateWithFlags(&st, 1);
		for (int i = 0; i < 40 && !stop; i++)
		{
			vfgs_hip_model* m = nullptr;
			if (vfgs_hip_model_capture(&m, st) || !m) { g_fail++; break; }
			if (i % 3 == 0) hipStreamSynchronize(st);
			vfgs_hip_model_release(m);
		}
		hipStreamSynchronize(st);
		hipStreamDestroy(st);
	};
	std::thread t1(caller, 0), t2(caller, 1), t3(capturer);
	t1.join(); t2.join();
	stop = true;
	t3.join();
	hipDeviceSynchronize();
	touch_model(a); touch_model(b);
	vfgs_hip_model_release(a);
	vfgs_hip_model_release(b);
}

static void walk_refusals()
{
	Pic f(520, 70, 2, 2);
	program(8, 2, 2, true);
	vfgs_hip_model* m8 = capture(nullptr);
	program(10, 2, 1, true);
	vfgs_hip_model* m422 = capture(nullptr);
	program(10, 2, 2, true);
	vfgs_hip_model* gone = capture(nullptr);
	vfgs_hip_model_release(gone);
	vfgs_hip_model* a = capture(nullptr);
	program(10, 2, 2, false);
	vfgs_hip_model* b = capture(nullptr);
	Pool pool(f, 3), other(f, 3);
	const std::vector<uint32_t> seeds = seeds_of(3);
	const Regs want = planar_regs(f, 3, seeds.data());
	vfgs_set_seed(5);
	const Regs before;
	const unsigned long long l0 = launches();
	auto L = pool.list;
	const vfgs_hip_model* ok[3] = {a, b, a};
	auto call = [&](const vfgs_hip_sp_frame* s, const vfgs_hip_sp_frame* d, const vfgs_hip_model* const* ms, unsigned w = 520, unsigned stride = 0, unsigned uvs = 0,
	                unsigned shift = 6) {
		return vfgs_hip_add_grain_sp_frame_list_models_dev(s, d, ms, seeds.data(), 3, w, f.h, stride ? stride : (unsigned)f.stride, uvs ? uvs : (unsigned)f.uv_stride, shift, nullptr);
	};
	// 41, each cause
	CHECK(call(L.data(), L.data(), nullptr) == 41 && vfgs_hip_last_error() == 41);
	{ const vfgs_hip_model* ms[3] = {a, nullptr, a}; CHECK(call(L.data(), L.data(), ms) == 41); }
	{ const vfgs_hip_model* ms[3] = {a, b, gone}; CHECK(call(L.data(), L.data(), ms) == 41); }
	{ const vfgs_hip_model* ms[3] = {a, m8, a}; CHECK(call(L.data(), L.data(), ms) == 41 && strstr(vfgs_hip_last_error_string(), "depth 8")); }
	{ const vfgs_hip_model* ms[3] = {m422, b, a}; CHECK(call(L.data(), L.data(), ms) == 41 && strstr(vfgs_hip_last_error_string(), "2,1")); }
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	CHECK(call(L.data(), L.data(), ok) == 41 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
	vfgs_hip_clear_chroma_mix();
	// 40, each cause
	CHECK(call(L.data(), L.data(), ok, 520, 0, 0, 4) == 40 && strstr(vfgs_hip_last_error_string(), "sample_shift 4"));
	{
		// (planes of that width: the list checks, which come first, find nothing)
		Pic wide(8208, 17, 2, 2);
		Pool wp(wide, 3);
		CHECK(vfgs_hip_add_grain_sp_frame_list_models_dev(wp.list.data(), wp.list.data(), ok, seeds.data(), 3, 8208, 17, wide.stride, wide.uv_stride, 6, nullptr) == 40 &&
		      strstr(vfgs_hip_last_error_string(), "8208"));
	}
	vfgs_set_chroma_subsampling(1, 2);             // (4:4:0: the chroma rows of the planes as allocated -- the list checks come first)
	CHECK(call(L.data(), L.data(), ok) == 40 && strstr(vfgs_hip_last_error_string(), "csubx 1"));
	vfgs_set_chroma_subsampling(2, 2);
	vfgs_set_depth(8);
	CHECK(call(L.data(), L.data(), ok) == 40 && strstr(vfgs_hip_last_error_string(), "sample_shift 6 at depth 8"));
	vfgs_set_depth(10);
	// what the semi-planar list refuses, with its codes
	CHECK(call(nullptr, L.data(), ok) == 18 && call(L.data(), nullptr, ok) == 18);
	L[2] = L[0];
	CHECK(call(L.data(), L.data(), ok) == 18);
	L = pool.list; L[1].UV = nullptr;
	CHECK(call(L.data(), L.data(), ok) == 18);
	L = pool.list; L[1].Y = (uint8_t*)L[1].Y + 8;
	CHECK(call(L.data(), L.data(), ok) == 7);
	L = pool.list;
	{ auto D = L; std::swap(D[0], D[1]); CHECK(call(L.data(), D.data(), ok) == 18); }
	{ auto D = other.list; D[1].UV = D[0].Y; CHECK(call(L.data(), D.data(), ok) == 18); }      // a UV plane that is another frame's Y
	CHECK(call(L.data(), L.data(), ok, 520, 512) == 6);
	CHECK(call(L.data(), L.data(), ok, 520, 0, 512) == 6);
	CHECK(call(L.data(), L.data(), ok, 520, f.stride + 4) == 8);
	CHECK(call(L.data(), L.data(), ok, 100) == 5);
	// the list checks come first, then 40, then 41
	CHECK(call(L.data(), L.data(), nullptr, 100) == 5 && call(L.data(), L.data(), nullptr, 520, 0, 0, 4) == 40);
	// the programmed state's own troubles are not the models': an undefined pattern-LUT entry
	unsigned char lut[256];
	memset(lut, 0x90, sizeof lut);
	vfgs_set_pattern_lut(1, lut);
	OK(vfgs_hip_add_grain_sp_frame_list_models_dev(L.data(), L.data(), ok, nullptr, 0, f.w, f.h, f.stride, f.uv_stride, 6, nullptr));      // an empty list is no call at all
	OK(vfgs_hip_add_grain_sp_frame_list_models_dev(nullptr, nullptr, nullptr, nullptr, 0, 100, f.h, 0, 0, 99, nullptr));
	CHECK(Regs() == before && launches() == l0);
	OK(call(L.data(), L.data(), ok));              // (with the undefined LUT entry still programmed)
	CHECK(Regs() == want);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f) && other.all_hold(f));
	for (const vfgs_hip_model* m : {a, b, m8, m422}) touch_model(m);
	// a, b, m8, m422 stay live: vfgs_hip_shutdown at the end of main releases what is left (the leak check says whether it did)
}

int main(int argc, char** argv)
{
	// run_walks shuts down with live models (walk_refusals leaves four)
	return run_walks(argc, argv, {
		{"entries", walk_entries},
		{"form_changes", walk_form_changes},
		{"release_while_queued", walk_release_while_queued},
		{"threads", walk_threads},
		{"refusals", walk_refusals},
	});
}
