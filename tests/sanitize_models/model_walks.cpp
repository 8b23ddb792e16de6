// TEST INFRASTRUCTURE.  Models as device objects (include/vfgs_hip.h: vfgs_hip_model_capture / _release / _info,
// vfgs_hip_add_grain_frame_list_models_dev) in the host layer of libvfgs_hip, compiled with a sanitizer over tests/sanitize/hip_stub.cpp, as
// tests/sanitize_seeded/seeded_walks.cpp drives the seeded lists: capture / use / release in every order, lists whose models change form and
// that are longer than a launch holds, planes allocated exactly to contract size, every refusal with nothing changed, and two threads that
// capture and release while a third calls.
//
// What the stub CANNOT prove: its "kernel" reads KernelArgs::tables only -- the first frame's table image -- not the images of the other
// frames of a launch (FrameTable::model[]), which the stub (unchanged, and older than the field) does not know.  So the walks themselves read
// every model's device bytes -- record and image, the length vfgs_hip_model_info reports -- once everything queued has run: bytes that were
// freed or handed to another capture while a queued launch could still read them are a sanitizer report there or in the stub's queue.  The
// handle is opaque; the host layer keeps the device pointer as the structure's first member for exactly this read.  Values are the GPU
// suite's business (tests/test_gpu_model_list.py); the seed registers are compared with those of the contract's loop through the same library.
//
// usage: model_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 41
#include "../sanitize/walks.h"

using Pool = FramePool;

// the registers the contract's loop leaves -- they depend on the seeds and the geometry, not on the model -- through the plain entries
static Regs loop_regs(const Frame& f, int n, const std::vector<uint32_t>* seeds)
{
	DevFrame d(f);
	for (int i = 0; i < n; i++)
	{
		if (seeds) vfgs_set_seed((*seeds)[i]);
		OK(vfgs_hip_add_grain_frame_dev(d.Y, d.U, d.V, f.w, f.h, f.stride, f.cstride, nullptr));
	}
	hipDeviceSynchronize();
	return Regs();
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_orders()
{
	void *sa = nullptr, *sb = nullptr;
	hipStreamCreateWithFlags(&sa, 1);
	hipStreamCreateWithFlags(&sb, 1);
	Frame f(520, 70, 10, 2, 2);
	program(10, 2, 2, true);
	vfgs_hip_model* a = capture(sa);
	vfgs_hip_model* a2 = capture(sa);              // the same state twice: two models
	CHECK(a != a2);
	program(10, 2, 2, true, 4, 1);
	vfgs_hip_model* b = capture(sb);
	int ia[8], ib[8];
	OK(vfgs_hip_model_info(a, ia)); OK(vfgs_hip_model_info(b, ib));
	CHECK(ia[0] == 10 && ia[1] == 2 && ia[2] == 2 && ia[3] == 1 && ia[4] == 1 && ia[6] == 0 && ib[6] == 1 && ib[5] == ia[5] - 1 && ia[7] == ib[7]);
	Pool pool(f, 6);
	const vfgs_hip_model* ms[6] = {a, b, a2, b, a, b};
	// released BEFORE use: refused, nothing changed
	vfgs_hip_model_release(a2);
	const Regs r0;
	CHECK(vfgs_hip_add_grain_frame_list_models_dev(pool.list.data(), pool.list.data(), ms, nullptr, 6, f.w, f.h, f.stride, f.cstride, sb) == 41);
	CHECK(Regs() == r0);
	ms[2] = a;
	// captured on sa and sb, used on sb; released right after the call returns, with everything still queued
	OK(vfgs_hip_add_grain_frame_list_models_dev(pool.list.data(), pool.list.data(), ms, nullptr, 6, f.w, f.h, f.stride, f.cstride, sb));
	vfgs_hip_model_release(a);
	vfgs_hip_model_release(a);                     // twice: no-op
	vfgs_hip_model_release(nullptr);
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
	// use after the other stream's capture, in place and out of place, seeded
	Pool out(f, 3);
	const vfgs_hip_model* m3[3] = {b, b, b};
	const std::vector<uint32_t> seeds = seeds_of(3);
	OK(vfgs_hip_add_grain_frame_list_models_dev(pool.list.data(), out.list.data(), m3, seeds.data(), 3, f.w, f.h, f.stride, f.cstride, sa));
	hipStreamSynchronize(sa);
	CHECK(out.all_hold(f));
	touch_model(b);
	vfgs_hip_model_release(b);
	hipStreamDestroy(sa);
	hipStreamDestroy(sb);
}

static void walk_lists()
{
	// width, height, depth, subsampling
	const int cases[][5] = {{200, 150, 10, 2, 2}, {520, 70, 8, 2, 2}, {333, 80, 10, 1, 1}, {1042, 96, 12, 2, 1}, {346, 160, 8, 1, 2}};
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], depth = c[2], sx = c[3], sy = c[4], n = 70;
		Frame f(w, h, depth, sx, sy);
		program(depth, sx, sy, false);
		vfgs_hip_model* g = capture(st);           // general form
		program(depth, sx, sy, true, 4, 1);
		vfgs_hip_model* o1 = capture(st);          // one-pattern form
		program(depth, sx, sy, true);
		vfgs_hip_model* o2 = capture(st);
		// 3 of g, 40 alternating o1 / o2 (one form: 32 + 8), 2 of g, 25 of o1: launches 3, 32, 8, 2, 25
		std::vector<const vfgs_hip_model*> ms;
		for (int i = 0; i < 3; i++) ms.push_back(g);
		for (int i = 0; i < 40; i++) ms.push_back(i & 1 ? o1 : o2);
		for (int i = 0; i < 2; i++) ms.push_back(g);
		for (int i = 0; i < 25; i++) ms.push_back(o1);
		const std::vector<uint32_t> seeds = seeds_of(n);
		vfgs_set_seed(77);
		const Regs want_plain = loop_regs(f, n, nullptr);
		const Regs want_seeded = loop_regs(f, n, &seeds);
		Pool pool(f, n), out(f, n);
		vfgs_set_seed(77);
		unsigned long long l0 = launches();
		OK(vfgs_hip_add_grain_frame_list_models_dev(pool.list.data(), pool.list.data(), ms.data(), nullptr, n, w, h, f.stride, f.cstride, st));
		vfgs_hip_launch_info li;
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && li.launches - l0 == 5 && li.nframes == 25 && li.listed == 1 && li.one_y == 1 && li.one_c == 1);
		CHECK(Regs() == want_plain);
		l0 = launches();
		OK(vfgs_hip_add_grain_frame_list_models_dev(pool.list.data(), out.list.data(), ms.data(), seeds.data(), n, w, h, f.stride, f.cstride, st));
		CHECK(launches() - l0 == 5 && Regs() == want_seeded);
		// the programmed state is the caller's: a plain call behind it
		OK(vfgs_hip_add_grain_frame_list_dev(pool.list.data(), 2, w, h, f.stride, f.cstride, st));
		hipStreamSynchronize(st);
		CHECK(pool.all_hold(f) && out.all_hold(f));
		for (const vfgs_hip_model* m : {g, o1, o2}) touch_model(m);
		vfgs_hip_model_release(g); vfgs_hip_model_release(o1); vfgs_hip_model_release(o2);
	}
	hipStreamDestroy(st);
}

static void walk_overlap_region()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	Frame f(520, 70, 10, 2, 2);
	program(10, 2, 2, true);
	vfgs_hip_model* a = capture(st);
	program(10, 2, 2, false);
	vfgs_hip_model* b = capture(st);
	vfgs_set_seed(3);
	const Regs want = loop_regs(f, 7, nullptr);
	Pool pa(f, 4), pb(f, 3);
	const vfgs_hip_model* ma[4] = {a, a, b, a};
	const vfgs_hip_model* mb[3] = {b, a, a};
	vfgs_set_seed(3);
	OK(vfgs_hip_overlap_begin(st));
	OK(vfgs_hip_add_grain_frame_list_models_dev(pa.list.data(), pa.list.data(), ma, nullptr, 4, f.w, f.h, f.stride, f.cstride, st));
	OK(vfgs_hip_add_grain_frame_list_models_dev(pb.list.data(), pb.list.data(), mb, nullptr, 3, f.w, f.h, f.stride, f.cstride, st));
	vfgs_hip_model_release(a);                     // inside the region, with both calls queued on its internal streams
	OK(vfgs_hip_overlap_end(st));
	CHECK(Regs() == want);
	hipStreamSynchronize(st);
	CHECK(pa.all_hold(f) && pb.all_hold(f));
	touch_model(b);
	vfgs_hip_model_release(b);
	hipStreamDestroy(st);
}

static void walk_refusals()
{
	Frame f(520, 70, 10, 2, 2);
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
	Pool pool(f, 3);
	const std::vector<uint32_t> seeds = seeds_of(3);
	const Regs want = loop_regs(f, 3, &seeds);     // (now: the plain entries will refuse the state this walk programs further down)
	vfgs_set_seed(5);
	const Regs before;
	const unsigned long long l0 = launches();
	auto L = pool.list;
	const vfgs_hip_model* ok[3] = {a, b, a};
	auto call = [&](const vfgs_hip_frame_ptrs* s, const vfgs_hip_frame_ptrs* d, const vfgs_hip_model* const* ms, unsigned w = 520, unsigned stride = 0) {
		return vfgs_hip_add_grain_frame_list_models_dev(s, d, ms, seeds.data(), 3, w, f.h, stride ? stride : (unsigned)f.stride, f.cstride, nullptr);
	};
	// 41, each cause
	CHECK(call(L.data(), L.data(), nullptr) == 41 && vfgs_hip_last_error() == 41);
	{ const vfgs_hip_model* ms[3] = {a, nullptr, a}; CHECK(call(L.data(), L.data(), ms) == 41); }
	{ const vfgs_hip_model* ms[3] = {a, b, gone}; CHECK(call(L.data(), L.data(), ms) == 41); }
	{ const vfgs_hip_model* ms[3] = {a, m8, a}; CHECK(call(L.data(), L.data(), ms) == 41 && strstr(vfgs_hip_last_error_string(), "depth 8")); }
	{ const vfgs_hip_model* ms[3] = {m422, b, a}; CHECK(call(L.data(), L.data(), ms) == 41 && strstr(vfgs_hip_last_error_string(), "2,1")); }
	CHECK(vfgs_hip_add_grain_frame_list_models_dev(L.data(), L.data(), ok, seeds.data(), 3, 8200, f.h, 8256, 4128, nullptr) == 41 && strstr(vfgs_hip_last_error_string(), "8200"));
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	CHECK(call(L.data(), L.data(), ok) == 41 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
	vfgs_hip_clear_chroma_mix();
	int info[8];
	CHECK(vfgs_hip_model_info(gone, info) == 41 && vfgs_hip_model_info(nullptr, info) == 41 && vfgs_hip_model_info(a, nullptr) == 41);
	CHECK(vfgs_hip_model_capture(nullptr, nullptr) == 41);
	// what the list calls refuse
	CHECK(call(nullptr, L.data(), ok) == 18 && call(L.data(), nullptr, ok) == 18);
	L[2] = L[0];
	CHECK(call(L.data(), L.data(), ok) == 18);
	L = pool.list; L[1].U = nullptr;
	CHECK(call(L.data(), L.data(), ok) == 18);
	L = pool.list; L[1].Y = (uint8_t*)L[1].Y + 8;
	CHECK(call(L.data(), L.data(), ok) == 7);
	L = pool.list;
	{ auto D = L; std::swap(D[0], D[1]); CHECK(call(L.data(), D.data(), ok) == 18); }
	CHECK(call(L.data(), L.data(), ok, 520, 512) == 6);
	CHECK(call(L.data(), L.data(), ok, 100) == 5);
	// the programmed state's own troubles are not the models': an undefined pattern-LUT entry refuses capture (4), a call with models captured before is served
	unsigned char lut[256];
	memset(lut, 0x90, sizeof lut);
	vfgs_set_pattern_lut(1, lut);
	vfgs_hip_model* none = (vfgs_hip_model*)1;
	CHECK(vfgs_hip_model_capture(&none, nullptr) == 4 && none == nullptr);
	OK(vfgs_hip_add_grain_frame_list_models_dev(L.data(), L.data(), ok, nullptr, 0, f.w, f.h, f.stride, f.cstride, nullptr));      // an empty list is no call at all
	OK(vfgs_hip_add_grain_frame_list_models_dev(nullptr, nullptr, nullptr, nullptr, 0, f.w, f.h, f.stride, f.cstride, nullptr));
	CHECK(Regs() == before && launches() == l0);
	OK(call(L.data(), L.data(), ok));              // (with the undefined LUT entry still programmed)
	CHECK(Regs() == want);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f));
	for (const vfgs_hip_model* m : {a, b, m8, m422}) touch_model(m);
	// a, b, m8, m422 stay live: vfgs_hip_shutdown at the end of main releases what is left (the leak check says whether it did)
}

static void walk_threads()
{
	// two threads capture, read and release models of the state programmed here while a third calls with models captured before
	Frame f(520, 70, 10, 2, 2);
	program(10, 2, 2, true);
	vfgs_hip_model* a = capture(nullptr);
	vfgs_hip_model* b = capture(nullptr);
	std::atomic<bool> stop{false};
	auto capturer = [&](int k) {
		void* st = nullptr;
		hipStreamCreateWithFlags(&st, 1);
		for (int i = 0; i < 40 && !stop; i++)
		{
			vfgs_hip_model* m = nullptr;
			if (vfgs_hip_model_capture(&m, st) || !m) { g_fail++; break; }
			int info[8];
			if (vfgs_hip_model_info(m, info) || info[0] != 10) g_fail++;
			if ((i + k) % 3 == 0) hipStreamSynchronize(st);
			vfgs_hip_model_release(m);
		}
		hipStreamSynchronize(st);
		hipStreamDestroy(st);
	};
	Pool pool(f, 6);
	const vfgs_hip_model* ms[6] = {a, b, b, a, b, a};
	std::thread t1(capturer, 0), t2(capturer, 1);
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	for (int i = 0; i < 30; i++)
	{
		const std::vector<uint32_t> seeds = seeds_of(6);
		OK(vfgs_hip_add_grain_frame_list_models_dev(pool.list.data(), pool.list.data(), ms, (i & 1) ? seeds.data() : nullptr, 6, f.w, f.h, f.stride, f.cstride, st));
		if (i % 7 == 0) hipStreamSynchronize(st);
	}
	stop = true;
	t1.join(); t2.join();
	hipStreamSynchronize(st);
	CHECK(pool.all_hold(f));
	touch_model(a); touch_model(b);
	vfgs_hip_model_release(a);
	vfgs_hip_model_release(b);
	hipStreamDestroy(st);
}

int main(int argc, char** argv)
{
	// run_walks shuts down with live models (walk_refusals leaves four)
	return run_walks(argc, argv, {
		{"orders", walk_orders},
		{"lists", walk_lists},
		{"overlap_region", walk_overlap_region},
		{"refusals", walk_refusals},
		{"threads", walk_threads},
	});
}
