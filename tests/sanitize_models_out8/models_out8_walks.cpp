// TEST INFRASTRUCTURE.  A model per picture with the narrowed 8-bit destination (include/vfgs_hip.h:
// vfgs_hip_add_grain_frame_list_models_copy8_dev, vfgs_hip_add_grain_sp_frame_list_models_copy8_dev) in the host layer of libvfgs_hip,
// compiled with a sanitizer over the unchanged tests/sanitize/hip_stub.cpp, as tests/sanitize_sp_models/sp_model_walks.cpp drives the call
// it extends: lists whose models change form (five launches out of 70 frames), seeded and not, release right after the call with
// everything queued, every refusal with nothing changed (a plane that reaches the 2 GiB window, 15, included).  Planes are allocated exactly as large as the contracts say -- sources in 16-bit
// containers, destinations in bytes with pitches of their own -- so a wrong extent or pitch is a sanitizer report.
//
// What the stub proves here: its "kernel" narrows every source row into the destination row the launch names ((v + 2) >> 2, a grain of
// zero) with the launch's own PlaneDesc, so the walks compare every destination byte -- the written region against the narrowed source,
// everything else against the fill.  The stub serves the narrowed destination at depth 10 only; depth 12 is the GPU suite's.
// What it cannot prove: it reads KernelArgs::tables only, frame 0's image, not FrameTable::model[] -- the walks read every model's device
// bytes themselves once everything queued has run, as the walks of the calls with models do.  Values are the GPU suite's business
// (tests/test_gpu_model_list_out8.py, tests/test_gpu_sp_model_list_out8.py); the seed registers are compared with those of the planar
// list calls on planar frames of the same size, through the same library.
//
// usage: models_out8_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 59
#include "../sanitize/walks.h"

// The geometry of one call, planar or semi-planar (sp: U is the plane of Cb/Cr pairs, V unused): sources of 10-bit samples in 16-bit
// containers, destinations of bytes; every plane (rows - 1) pitches and one row of whole blocks.
struct Geo {
	bool sp;
	int w, h, sx, sy, nblk, crows;
	unsigned stride, cstride, dstride, dcstride;      // samples / samples / bytes / bytes
	size_t yrow, crow;                                 // containers of a row of whole blocks, luma / one chroma plane
	Geo(bool sp_, int w_, int h_, int sx_, int sy_, int pad, int dpad) : sp(sp_), w(w_), h(h_), sx(sx_), sy(sy_)
	{
		nblk = (w + 15) / 16;
		crows = (h + sy - 1) / sy;
		yrow = (size_t)nblk * 16;
		crow = sp ? yrow : yrow / sx;
		stride = (unsigned)yrow + pad; cstride = (unsigned)crow + pad;
		dstride = (unsigned)yrow + dpad; dcstride = ((unsigned)crow + 2 * dpad + 15) & ~15u;      // (bytes: multiples of 16)
	}
	size_t ysize(bool d) const { return (size_t)(h - 1) * (d ? dstride : stride) + yrow; }
	size_t csize(bool d) const { return (size_t)(crows - 1) * (d ? dcstride : cstride) + crow; }
	int nplanes() const { return sp ? 2 : 3; }
};

struct Planes {
	std::vector<uint8_t> p[3];
};

static Planes source_of(const Geo& g)
{
	Planes s;
	s.p[0].resize(g.ysize(false) * 2);
	for (int c = 1; c < g.nplanes(); c++) s.p[c].resize(g.csize(false) * 2);
	for (auto& v : s.p)
		for (size_t i = 0; i < v.size(); i += 2) { const unsigned x = rnd() & 0x3ff; v[i] = (uint8_t)x; v[i + 1] = (uint8_t)(x >> 8); }
	return s;
}

static const uint8_t kFill = 0xa5;

// what the stub leaves in a destination: the whole blocks of every row narrowed, everything else the fill
static Planes expected_of(const Geo& g, const Planes& s)
{
	Planes d;
	for (int c = 0; c < g.nplanes(); c++)
	{
		const size_t rows = c ? g.crows : g.h, rowb = c ? g.crow : g.yrow, sp = c ? g.cstride : g.stride, dp = c ? g.dcstride : g.dstride;
		d.p[c].assign(c ? g.csize(true) : g.ysize(true), kFill);
		const uint16_t* src = (const uint16_t*)s.p[c].data();
		for (size_t r = 0; r < rows; r++)
			for (size_t i = 0; i < rowb; i++) d.p[c][r * dp + i] = (uint8_t)((src[r * sp + i] + 2) >> 2);
	}
	return d;
}

struct DevPlanes {
	uint8_t* p[3] = {nullptr, nullptr, nullptr};
	size_t n[3] = {0, 0, 0};
	explicit DevPlanes(const Planes& h)
	{
		for (int c = 0; c < 3; c++)
			if (!h.p[c].empty()) { n[c] = h.p[c].size(); hipMalloc((void**)&p[c], n[c]); hipMemcpy(p[c], h.p[c].data(), n[c], 1); }
	}
	~DevPlanes() { for (auto* q : p) if (q) hipFree(q); }
	DevPlanes(const DevPlanes&) = delete;
	bool holds(const Planes& h) const
	{
		for (int c = 0; c < 3; c++)
		{
			std::vector<uint8_t> b(n[c]);
			if (n[c]) hipMemcpy(b.data(), p[c], n[c], 2);
			if (b != h.p[c]) return false;
		}
		return true;
	}
};

struct Pool {
	std::vector<std::unique_ptr<DevPlanes>> fr;
	std::vector<vfgs_hip_frame_ptrs> list;
	std::vector<vfgs_hip_sp_frame> sp_list;
	Pool(const Planes& h, int n)
	{
		for (int i = 0; i < n; i++)
		{
			fr.emplace_back(new DevPlanes(h));
			list.push_back({fr.back()->p[0], fr.back()->p[1], fr.back()->p[2]});
			sp_list.push_back({fr.back()->p[0], fr.back()->p[1]});
		}
	}
	bool all_hold(const Planes& h) const
	{
		for (const auto& d : fr) if (!d->holds(h)) return false;
		return true;
	}
};

static Planes filled_like(const Geo& g)
{
	Planes d;
	d.p[0].assign(g.ysize(true), kFill);
	for (int c = 1; c < g.nplanes(); c++) d.p[c].assign(g.csize(true), kFill);
	return d;
}

// the registers the contract's loop leaves -- they depend on the seeds and the geometry, not on the model or the destination -- through the
// planar list calls on planar pictures of the same size
static Regs planar_regs(const Geo& g, int n, const uint32_t* seeds) { return planar_regs(g.w, g.h, g.crows, 2, n, seeds); }

// the entry of the geometry's kind
static int call(const Geo& g, const Pool& src, const Pool& dst, const vfgs_hip_model* const* ms, const uint32_t* seeds, unsigned n, void* st, unsigned shift = 0)
{
	if (g.sp)
		return vfgs_hip_add_grain_sp_frame_list_models_copy8_dev(src.sp_list.data(), dst.sp_list.data(), ms, seeds, n, g.w, g.h, g.stride, g.cstride, g.dstride, g.dcstride, shift, st);
	return vfgs_hip_add_grain_frame_list_models_copy8_dev(src.list.data(), dst.list.data(), ms, seeds, n, g.w, g.h, g.stride, g.cstride, g.dstride, g.dcstride, st);
}

// (the model of the launch names the kernels of the row walk its own way: tests/sanitize/hip_stub.cpp name_launch)
static bool named(const Geo& g, const vfgs_hip_launch_info& li, int oney, int onec)
{
	char want[96];
	if (g.sp) snprintf(want, sizeof want, "grain_sp8_kernel<10,%d,%s,%s>", g.sy, oney ? "true" : "false", onec ? "true" : "false");
	else snprintf(want, sizeof want, "stub<10,%d,%d,1,%d,%d,0,0>", g.sx, g.sy, oney, onec);
	return !strcmp(li.kernel, want) && li.listed == 1 && li.out8 == 1 && li.in_place == 0 && li.persistent_luma_workgroups == 0 && li.depth == 10;
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

// 70 frames whose models change form: 3 general, 40 alternating between two one-pattern models (32 + 8), 2 general, 25 one-pattern
static void walk_runs_across_forms()
{
	// semi-planar, width, height, csubx, csuby, source padding (containers), destination padding (bytes)
	const int cases[][7] = {{0, 200, 40, 2, 2, 0, 16}, {0, 264, 33, 1, 1, 8, 0}, {0, 136, 48, 1, 2, 0, 32}, {1, 200, 40, 2, 2, 8, 16}, {1, 1042, 17, 2, 1, 0, 0}};
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	for (const auto& c : cases)
	{
		const Geo g(c[0] != 0, c[1], c[2], c[3], c[4], c[5], c[6]);
		const int n = 70;
		program(10, g.sx, g.sy, false);
		vfgs_hip_model* gen = capture(st);
		program(10, g.sx, g.sy, true, 4, 1);
		vfgs_hip_model* o1 = capture(st);
		program(10, g.sx, g.sy, true);
		vfgs_hip_model* o2 = capture(st);
		std::vector<const vfgs_hip_model*> ms;
		for (int i = 0; i < 3; i++) ms.push_back(gen);
		for (int i = 0; i < 40; i++) ms.push_back(i & 1 ? o1 : o2);
		for (int i = 0; i < 2; i++) ms.push_back(gen);
		for (int i = 0; i < 25; i++) ms.push_back(o1);
		const std::vector<uint32_t> seeds = seeds_of(n);
		vfgs_set_seed(77);
		const Regs want_plain = planar_regs(g, n, nullptr);
		const Regs want_seeded = planar_regs(g, n, seeds.data());
		const Planes s = source_of(g), fill = filled_like(g), want = expected_of(g, s);
		Pool src(s, n), dst(fill, n), dst2(fill, n);
		vfgs_set_seed(77);
		unsigned long long l0 = launches();
		OK(call(g, src, dst, ms.data(), nullptr, n, st, g.sp ? 6 : 0));
		vfgs_hip_launch_info li;
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && named(g, li, 1, 1) && li.launches - l0 == 5 && li.nframes == 25);
		CHECK(Regs() == want_plain);
		l0 = launches();
		OK(call(g, src, dst2, ms.data(), seeds.data(), n, st, 0));
		CHECK(launches() - l0 == 5 && Regs() == want_seeded);
		// the programmed state is the caller's: the programmed list behind it, the model programmed last
		if (!g.sp) OK(vfgs_hip_add_grain_frame_list_copy8_dev(src.list.data(), dst.list.data(), 2, g.w, g.h, g.stride, g.cstride, g.dstride, g.dcstride, st));
		else OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(src.sp_list.data(), dst.sp_list.data(), nullptr, 2, g.w, g.h, g.stride, g.cstride, g.dstride, g.dcstride, 0, st));
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && named(g, li, 1, 1) && li.nframes == 2);
		hipStreamSynchronize(st);
		CHECK(src.all_hold(s) && dst.all_hold(want) && dst2.all_hold(want));      // (the stub's kernel does not look at sample_shift)
		for (const vfgs_hip_model* m : {gen, o1, o2}) touch_model(m);
		vfgs_hip_model_release(gen); vfgs_hip_model_release(o1); vfgs_hip_model_release(o2);
	}
	hipStreamDestroy(st);
}

// captured on one stream, used on another, released right after the call with everything queued; captures in between; an overlap region
static void walk_release_right_after_the_call()
{
	void *sa = nullptr, *sb = nullptr;
	hipStreamCreateWithFlags(&sa, 1);
	hipStreamCreateWithFlags(&sb, 1);
	for (int sp = 0; sp < 2; sp++)
	{
		const Geo g(sp != 0, 520, 70, 2, 2, 0, 16);
		program(10, 2, 2, true);
		vfgs_hip_model* a = capture(sa);
		program(10, 2, 2, true, 4, 1);
		vfgs_hip_model* b = capture(sb);
		const Planes s = source_of(g), fill = filled_like(g), want = expected_of(g, s);
		Pool src(s, 6), dst(fill, 6);
		const vfgs_hip_model* ms[6] = {a, b, a, b, a, b};
		OK(call(g, src, dst, ms, nullptr, 6, sb));
		vfgs_hip_model_release(a);                     // right after the call returns
		vfgs_hip_model_release(a);                     // twice: no-op
		const Regs r0;
		CHECK(call(g, src, dst, ms, nullptr, 6, sb) == 41 && Regs() == r0);      // a released entry: refused, nothing changed
		for (int i = 0; i < 12; i++)
		{
			vfgs_hip_model* t = capture(i & 1 ? sa : sb);
			touch_model(t);
			vfgs_hip_model_release(t);
		}
		hipStreamSynchronize(sb);
		CHECK(src.all_hold(s) && dst.all_hold(want));
		touch_model(b);
		// two calls inside an overlap region, a release inside it
		program(10, 2, 2, false);
		vfgs_hip_model* c = capture(sa);
		vfgs_set_seed(3);
		const Regs regs = planar_regs(g, 7, nullptr);
		Pool sa4(s, 4), sb3(s, 3), da(fill, 4), db(fill, 3);
		const vfgs_hip_model* ma[4] = {b, b, c, b};
		const vfgs_hip_model* mb[3] = {c, b, b};
		vfgs_set_seed(3);
		OK(vfgs_hip_overlap_begin(sa));
		OK(call(g, sa4, da, ma, nullptr, 4, sa));
		OK(call(g, sb3, db, mb, nullptr, 3, sa));
		vfgs_hip_model_release(b);                     // inside the region, with both calls queued on its internal streams
		OK(vfgs_hip_overlap_end(sa));
		CHECK(Regs() == regs);
		hipStreamSynchronize(sa);
		CHECK(da.all_hold(want) && db.all_hold(want) && sa4.all_hold(s) && sb3.all_hold(s));
		touch_model(c);
		vfgs_hip_model_release(c);
	}
	hipStreamDestroy(sa);
	hipStreamDestroy(sb);
}

static void walk_refusals()
{
	for (int sp = 0; sp < 2; sp++)
	{
		const Geo g(sp != 0, 544, 70, 2, 2, 0, 16);      // (34 blocks: the planes' pitches are multiples of 16 bytes at depth 8 as well)
		program(8, 2, 2, true);
		vfgs_hip_model* m8 = capture(nullptr);
		program(10, 2, 1, true);
		vfgs_hip_model* m422 = capture(nullptr);
		program(10, 2, 2, true);
		vfgs_hip_model* gone = capture(nullptr);
		vfgs_hip_model_release(gone);
		vfgs_hip_model* a = capture(nullptr);
		OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
		vfgs_hip_model* mixed = nullptr;
		OK(vfgs_hip_model_capture_mix(&mixed, nullptr));
		vfgs_hip_clear_chroma_mix();
		program(10, 2, 2, false);
		vfgs_hip_model* b = capture(nullptr);
		const Planes s = source_of(g), fill = filled_like(g), want = expected_of(g, s);
		Pool src(s, 3), dst(fill, 3);
		const std::vector<uint32_t> seeds = seeds_of(3);
		const Regs regs = planar_regs(g, 3, seeds.data());
		vfgs_set_seed(5);
		const Regs before;
		const unsigned long long l0 = launches();
		uint64_t b0[8], b1[8];
		vfgs_hip_get_model_build_stats(b0);
		const vfgs_hip_model* ok[3] = {a, b, a};
		auto with = [&](const vfgs_hip_model* const* ms, unsigned shift = 0) { return call(g, src, dst, ms, seeds.data(), 3, nullptr, shift); };
		// 41, each cause
		CHECK(with(nullptr) == 41 && vfgs_hip_last_error() == 41);
		{ const vfgs_hip_model* ms[3] = {a, nullptr, a}; CHECK(with(ms) == 41); }
		{ const vfgs_hip_model* ms[3] = {a, b, gone}; CHECK(with(ms) == 41); }
		{ const vfgs_hip_model* ms[3] = {a, m8, a}; CHECK(with(ms) == 41 && strstr(vfgs_hip_last_error_string(), "depth 8")); }
		{ const vfgs_hip_model* ms[3] = {m422, b, a}; CHECK(with(ms) == 41 && strstr(vfgs_hip_last_error_string(), "2,1")); }
		{ const vfgs_hip_model* ms[3] = {a, b, mixed}; CHECK(with(ms) == 41 && strstr(vfgs_hip_last_error_string(), "chroma mix") && strstr(vfgs_hip_last_error_string(), "frame 2")); }
		OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
		CHECK(with(ok) == 41 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
		vfgs_hip_clear_chroma_mix();
		// 40 before 41 (semi-planar), 16 before both, the list checks before everything
		if (g.sp) CHECK(with(nullptr, 4) == 40 && strstr(vfgs_hip_last_error_string(), "sample_shift 4"));
		vfgs_set_depth(8);
		CHECK(with(nullptr, g.sp ? 6 : 0) == 16);
		vfgs_set_depth(10);
		{
			Geo t = g; t.dstride = 512;
			CHECK(call(t, src, dst, nullptr, seeds.data(), 3, nullptr) == 6);
			t = g; t.dcstride += 8;
			CHECK(call(t, src, dst, nullptr, seeds.data(), 3, nullptr) == 8);
			t = g; t.w = 100;
			CHECK(call(t, src, dst, nullptr, seeds.data(), 3, nullptr, 4) == 5);
		}
		// 15: ONE picture whose luma plane reaches the 2 GiB buffer window (1864136 rows x 576 containers x 2 bytes; refused before anything is
		// touched: its planes are addresses, 8 GiB apart) -- behind the list checks, in front of the destination's pitches, 16, 40 and 41
		{
			auto far = [](uintptr_t k) { return (void*)(k << 33); };
			const vfgs_hip_frame_ptrs bs = {far(1), far(2), far(3)}, bd = {far(4), far(5), far(6)};
			const vfgs_hip_sp_frame bss = {far(1), far(2)}, bsd = {far(4), far(5)};
			const unsigned rows = 1864136;
			if (g.sp)
			{
				CHECK(vfgs_hip_add_grain_sp_frame_list_models_copy8_dev(&bss, &bsd, nullptr, seeds.data(), 1, 520, rows, 576, 576, 512, 528, 4, nullptr) == 15);
				CHECK(vfgs_hip_add_grain_sp_frame_list_models_copy8_dev(&bss, &bss, ok, seeds.data(), 1, 520, rows, 576, 576, 528, 528, 6, nullptr) == 18);
			}
			else
			{
				CHECK(vfgs_hip_add_grain_frame_list_models_copy8_dev(&bs, &bd, nullptr, seeds.data(), 1, 520, rows, 576, 320, 512, 272, nullptr) == 15);
				CHECK(vfgs_hip_add_grain_frame_list_models_copy8_dev(&bs, &bd, ok, seeds.data(), 1, 520, rows - 1, 576, 320, 512, 272, nullptr) == 6);
			}
			CHECK(strstr(vfgs_hip_last_error_string(), g.sp ? "shares bytes" : "destination stride") != nullptr);
		}
		// planes that share bytes: a destination listed twice; semi-planar: a destination that is its own source
		{
			Pool d2(fill, 3);
			d2.list[2] = d2.list[0]; d2.sp_list[2] = d2.sp_list[0];
			CHECK(call(g, src, d2, ok, seeds.data(), 3, nullptr) == 18);
			if (g.sp) CHECK(call(g, src, src, ok, seeds.data(), 3, nullptr) == 18 && strstr(vfgs_hip_last_error_string(), "shares bytes"));
		}
		// the programmed state's own troubles are not the models': an undefined pattern-LUT entry
		unsigned char lut[256];
		memset(lut, 0x90, sizeof lut);
		vfgs_set_pattern_lut(1, lut);
		OK(call(g, src, dst, ok, nullptr, 0, nullptr));      // an empty list is no call at all
		vfgs_hip_get_model_build_stats(b1);
		CHECK(Regs() == before && launches() == l0 && !memcmp(b0, b1, sizeof b0));
		hipDeviceSynchronize();
		CHECK(src.all_hold(s) && dst.all_hold(fill));
		OK(with(ok));                                        // (with the undefined LUT entry still programmed)
		CHECK(Regs() == regs);
		hipDeviceSynchronize();
		CHECK(src.all_hold(s) && dst.all_hold(want));
		for (const vfgs_hip_model* m : {a, b, m8, m422, mixed}) touch_model(m);
		// the models stay live: vfgs_hip_shutdown at the end of main releases what is left (the leak check says whether it did)
	}
}

int main(int argc, char** argv)
{
	// run_walks shuts down with live models (walk_refusals leaves ten)
	return run_walks(argc, argv, {
		{"runs_across_forms", walk_runs_across_forms},
		{"release_right_after_the_call", walk_release_right_after_the_call},
		{"refusals", walk_refusals},
	});
}
