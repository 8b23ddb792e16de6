// TEST INFRASTRUCTURE.  A model per picture from planar pictures onto semi-planar surfaces (include/vfgs_hip.h:
// vfgs_hip_add_grain_frame_list_models_to_sp_dev and vfgs_hip_add_grain_frame_list_models_to_sp8_dev) in the host layer of libvfgs_hip,
// compiled with a sanitizer over the unchanged tests/sanitize/hip_stub.cpp, as tests/sanitize_p2sp/p2sp_walks.cpp drives the programmed
// calls they extend and tests/sanitize_models_out8/models_out8_walks.cpp the narrowed lists with models: lists whose models change form
// (five launches out of 70 frames), seeded and not, what the launcher is handed for every run, every refusal in the header's order with
// nothing changed, a released model, and two threads calling at once.  Every plane is allocated exactly as large as the contract says:
// (rows - 1) pitches and one row of whole blocks, a planar chroma row of 8 containers per block, a UV row of 16.
//
// The model of the HIP runtime is compiled INTO this translation unit, unchanged, with its launcher of the grain kernels under another
// name, as in tests/sanitize_model_mix/model_mix_walks.cpp: vfgs::launch_grain below stands where vfgs_kernel.hip's does, holds every
// launch of the two families to what launch_args_ok holds it to -- family_fields() of the key with models where models_kernel is set:
// sp_kernel == 2, and with models listed frames with a 16-byte-aligned model image each -- records what it was handed, and passes the
// launch on to the model.
//
// What the model of the launch moves (see the head of tests/sanitize_p2sp/p2sp_walks.cpp, whose `modelled` is restated here): the narrowed
// form at the destination's own pitches, luma rows and ONE component's share of a UV row; the form in the depth's container at the SOURCE's
// pitches, so these walks keep stride <= dst_stride and cstride <= dst_uv_stride and prove the three source planes' extents only.  It reads
// KernelArgs::tables -- frame 0's image -- not FrameTable::model[]: the walks read every model's device bytes themselves once everything
// queued has run.  The narrowed destination is served at depth 10 only.  Values are the GPU suite's business (tests/test_gpu_models_to_sp.py).
//
// usage: models_to_sp_walks [walk ...]     (no argument: all of them)
#define launch_grain stub_launch_grain
#include "../sanitize/hip_stub.cpp"
#undef launch_grain

#include <hip/hip_runtime.h>

#include <type_traits>

#define WALKS_SEED 2718
#define WALKS_HAVE_HIP_RUNTIME_H
#include "../sanitize/walks.h"

// what the launcher was handed: the last launch, and how many launches of the two families with and without models
struct Handed { vfgs::Family family; int models_kernel, mix_kernel, sp_kernel, listed, nframes; bool out8; };
static Handed g_handed;      // (written under the library's lock; the walk with two threads reads it after the join)
static std::atomic<uint64_t> g_with_models{0}, g_programmed{0};

namespace vfgs {
hipError_t launch_grain(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream)
{
	const bool p2sp = k.family == Family::p2sp || k.family == Family::p2sp8;
	if (p2sp)
	{
		const FamilyFields ff = family_fields(k.family, a.models_kernel != 0);
		bool ok = a.models_kernel == ff.models_kernel && a.mix_kernel == 0 && ff.mix_kernel == 0 && a.sp_kernel == 2 && ff.sp_kernel == 2 && kernel_exists(k) &&
		          k.out8 == (k.family == Family::p2sp8) && list && a.listed == 1 && a.y0 == 0;
		for (int i = 0; ok && a.models_kernel && i < a.nframes; i++) ok = list->model[i] && !((uintptr_t)list->model[i] & 15);
		// (the launch's own image is frame 0's, behind its record)
		if (ok && a.models_kernel) ok = a.tables == list->model[0] + kModelRecordBytes;
		if (!ok)
		{
			fprintf(stderr, "FAILED launcher: family %d with models_kernel %d, mix_kernel %d, sp_kernel %d, out8 %d is not a launch the real launcher takes\n",
			        (int)k.family, a.models_kernel, a.mix_kernel, a.sp_kernel, (int)k.out8);
			g_fail++;
			return hipErrorInvalidValue;
		}
		(a.models_kernel ? g_with_models : g_programmed)++;
	}
	g_handed = Handed{k.family, a.models_kernel, a.mix_kernel, a.sp_kernel, a.listed, a.nframes, k.out8};
	return stub_launch_grain(a, list, k, grid, stream);
}
}  // namespace vfgs

static bool handed(bool out8, int models_kernel, int nframes)
{
	return g_handed.family == (out8 ? vfgs::Family::p2sp8 : vfgs::Family::p2sp) && g_handed.models_kernel == models_kernel && g_handed.mix_kernel == 0 &&
	       g_handed.sp_kernel == 2 && g_handed.listed == 1 && g_handed.out8 == out8 && g_handed.nframes == nframes;
}

// the two entry points exist with these C types
using to_sp_fn = int (*)(const vfgs_hip_frame_ptrs*, const vfgs_hip_sp_frame*, const vfgs_hip_model* const*, const uint32_t*, unsigned, unsigned, unsigned, unsigned,
                         unsigned, unsigned, unsigned, unsigned, void*);
using to_sp8_fn = int (*)(const vfgs_hip_frame_ptrs*, const vfgs_hip_sp_frame*, const vfgs_hip_model* const*, const uint32_t*, unsigned, unsigned, unsigned, unsigned,
                          unsigned, unsigned, unsigned, void*);
static_assert(std::is_same<decltype(&vfgs_hip_add_grain_frame_list_models_to_sp_dev), to_sp_fn>::value, "vfgs_hip_add_grain_frame_list_models_to_sp_dev");
static_assert(std::is_same<decltype(&vfgs_hip_add_grain_frame_list_models_to_sp8_dev), to_sp8_fn>::value, "vfgs_hip_add_grain_frame_list_models_to_sp8_dev");
static_assert(sizeof(vfgs::KernelArgs) == 312 && offsetof(vfgs::FrameTable, model) == 6 * 8 * vfgs::kListFrames, "what the kernels of before load has not moved");
static_assert(vfgs::family_fields(vfgs::Family::p2sp, true).models_kernel == 1 && vfgs::family_fields(vfgs::Family::p2sp8, true).models_kernel == 1 &&
              vfgs::family_fields(vfgs::Family::p2sp).models_kernel == 0 && vfgs::family_fields(vfgs::Family::p2sp8, true).sp_kernel == 2, "the two families decide at run time");

// a picture of `sz`-byte containers, its planes exactly as large as the contract says.  planar: Y, U, V (C[0], C[1]), a chroma row of 8
// containers per block; else Y and UV (C[0]), a UV row of 16.  pad / cpad: containers a row pitch exceeds the whole blocks by
struct Pic {
	int w, h, sy, sz, nblk, stride, cstride, crows;
	bool planar;
	std::vector<uint8_t> Y, C[2];
	Pic(bool planar_, int w_, int h_, int sy_, int sz_, int pad = 0, int cpad = 0) : w(w_), h(h_), sy(sy_), sz(sz_), planar(planar_)
	{
		nblk = (w + 15) / 16;
		stride = nblk * 16 + pad;
		cstride = nblk * (planar ? 8 : 16) + cpad;
		crows = (h + sy - 1) / sy;
		Y.resize(((size_t)(h - 1) * stride + nblk * 16) * sz);
		C[0].resize(((size_t)(crows - 1) * cstride + nblk * (planar ? 8 : 16)) * sz);
		if (planar) C[1].resize(C[0].size());
		for (auto* p : {&Y, &C[0], &C[1]})
			for (auto& b : *p) b = (uint8_t)rnd();
	}
};

struct DevPic {
	uint8_t* p[3] = {nullptr, nullptr, nullptr};
	size_t n[3];
	explicit DevPic(const Pic& f) : n{f.Y.size(), f.C[0].size(), f.C[1].size()}
	{
		const std::vector<uint8_t>* v[3] = {&f.Y, &f.C[0], &f.C[1]};
		for (int i = 0; i < 3; i++)
			if (n[i]) { hipMalloc((void**)&p[i], n[i]); to_device(p[i], v[i]->data(), n[i]); }
	}
	~DevPic() { for (auto* q : p) if (q) hipFree(q); }
	DevPic(const DevPic&) = delete;
	bool holds(const Pic& f) const
	{
		const std::vector<uint8_t>* v[3] = {&f.Y, &f.C[0], &f.C[1]};
		for (int i = 0; i < 3; i++)
		{
			std::vector<uint8_t> got(n[i]);
			if (n[i]) to_host(got.data(), p[i], n[i]);
			if (got != *v[i]) return false;
		}
		return true;
	}
	vfgs_hip_frame_ptrs planes() const { return {p[0], p[1], p[2]}; }
	vfgs_hip_sp_frame surface() const { return {p[0], p[1]}; }
};

template <class Ptrs>
struct PicPool {
	std::vector<std::unique_ptr<DevPic>> fr;
	std::vector<Ptrs> list;
	PicPool(const Pic& f, int n)
	{
		for (int i = 0; i < n; i++)
		{
			fr.emplace_back(new DevPic(f));
			if constexpr (std::is_same<Ptrs, vfgs_hip_frame_ptrs>::value) list.push_back(fr.back()->planes());
			else list.push_back(fr.back()->surface());
		}
	}
	bool all_hold(const Pic& f) const
	{
		for (const auto& d : fr) if (!d->holds(f)) return false;
		return true;
	}
};
using SrcPool = PicPool<vfgs_hip_frame_ptrs>;
using DstPool = PicPool<vfgs_hip_sp_frame>;

// what the model's launch leaves in a destination that held `fill` (tests/sanitize_p2sp/p2sp_walks.cpp `modelled`)
static Pic modelled(const Pic& src, const Pic& fill, bool out8)
{
	Pic out = fill;
	if (out8)
	{
		const uint16_t *sy = (const uint16_t*)src.Y.data(), *sv = (const uint16_t*)src.C[1].data();
		for (int r = 0; r < src.h; r++)
			for (int i = 0; i < src.nblk * 16; i++) out.Y[(size_t)r * fill.stride + i] = (uint8_t)((sy[(size_t)r * src.stride + i] + 2) >> 2);
		for (int r = 0; r < src.crows; r++)
			for (int i = 0; i < src.nblk * 8; i++) out.C[0][(size_t)r * fill.cstride + i] = (uint8_t)((sv[(size_t)r * src.cstride + i] + 2) >> 2);
		return out;
	}
	const size_t sz = src.sz;
	for (int r = 0; r < src.h; r++) memcpy(&out.Y[(size_t)r * src.stride * sz], &src.Y[(size_t)r * src.stride * sz], src.nblk * 16 * sz);
	for (int r = 0; r < src.crows; r++) memcpy(&out.C[0][(size_t)r * src.cstride * sz], &src.C[1][(size_t)r * src.cstride * sz], src.nblk * 8 * sz);
	return out;
}

// the registers the contract's loop leaves -- they depend on the seeds and the geometry, not on the model or the destination: those of the
// planar copy list (seeded or not) on the same sources, through the same library
static Regs planar_regs(const Pic& f, int n, const uint32_t* seeds)
{
	SrcPool s(f, n), d(f, n);
	if (seeds) OK(vfgs_hip_add_grain_frame_list_seeded_copy_dev(s.list.data(), d.list.data(), seeds, n, f.w, f.h, f.stride, f.cstride, nullptr));
	else OK(vfgs_hip_add_grain_frame_list_copy_dev(s.list.data(), d.list.data(), n, f.w, f.h, f.stride, f.cstride, nullptr));
	hipDeviceSynchronize();
	return Regs();
}

static bool named(const vfgs_hip_launch_info& li, bool out8, int depth, int sy, int oney, int onec)
{
	char want[96];
	snprintf(want, sizeof want, "%s<%d,%d,%s,%s>", out8 ? "grain_p2sp8_kernel" : "grain_p2sp_kernel", depth, sy, oney ? "true" : "false", onec ? "true" : "false");
	return !strcmp(li.kernel, want) && li.out8 == (out8 ? 1 : 0) && li.listed == 1 && li.in_place == 0 && li.persistent_luma_workgroups == 0 && li.depth == depth;
}

static int call(bool out8, const SrcPool& s, const DstPool& d, const vfgs_hip_model* const* ms, const uint32_t* seeds, unsigned n, const Pic& f, const Pic& fill,
                unsigned shift, void* st)
{
	if (out8) return vfgs_hip_add_grain_frame_list_models_to_sp8_dev(s.list.data(), d.list.data(), ms, seeds, n, f.w, f.h, f.stride, f.cstride, fill.stride, fill.cstride, st);
	return vfgs_hip_add_grain_frame_list_models_to_sp_dev(s.list.data(), d.list.data(), ms, seeds, n, f.w, f.h, f.stride, f.cstride, fill.stride, fill.cstride, shift, st);
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

// 70 frames whose models change form: 3 general, 40 alternating between two one-pattern models (32 + 8), 2 general, 25 one-pattern
static void walk_runs_across_forms()
{
	// depth, out8, width, height, csuby, sample shift, source padding of Y / of a chroma row, destination padding of Y / UV (containers)
	const int cases[][10] = {{10, 0, 200, 40, 2, 6, 0, 0, 0, 0}, {8, 0, 264, 33, 2, 0, 16, 8, 16, 32}, {12, 0, 136, 48, 1, 4, 8, 8, 16, 48},
	                         {10, 1, 200, 40, 2, 0, 16, 8, 32, 16}, {10, 1, 1042, 17, 1, 0, 0, 0, 16, 0}};
	hipStream_t st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	for (const auto& c : cases)
	{
		const int depth = c[0], w = c[2], h = c[3], sy = c[4], n = 70;
		const bool out8 = c[1] != 0;
		const unsigned shift = (unsigned)c[5];
		program(depth, 2, sy, false);
		vfgs_hip_model* gen = capture(st);
		program(depth, 2, sy, true, 4, 1);
		vfgs_hip_model* o1 = capture(st);
		program(depth, 2, sy, true);
		vfgs_hip_model* o2 = capture(st);
		std::vector<const vfgs_hip_model*> ms;
		for (int i = 0; i < 3; i++) ms.push_back(gen);
		for (int i = 0; i < 40; i++) ms.push_back(i & 1 ? o1 : o2);
		for (int i = 0; i < 2; i++) ms.push_back(gen);
		for (int i = 0; i < 25; i++) ms.push_back(o1);
		const std::vector<uint32_t> seeds = seeds_of(n);
		Pic f(true, w, h, sy, depth > 8 ? 2 : 1, c[6], c[7]), fill(false, w, h, sy, (depth > 8 && !out8) ? 2 : 1, c[8], c[9]);
		const Pic want = modelled(f, fill, out8);
		vfgs_set_seed(77);
		const Regs want_plain = planar_regs(f, n, nullptr);
		const Regs want_seeded = planar_regs(f, n, seeds.data());
		SrcPool src(f, n);
		DstPool dst(fill, n), dst2(fill, n);
		vfgs_set_seed(77);
		unsigned long long l0 = launches();
		uint64_t m0 = g_with_models, p0 = g_programmed;
		OK(call(out8, src, dst, ms.data(), nullptr, n, f, fill, shift, st));
		vfgs_hip_launch_info li;
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && named(li, out8, depth, sy, 1, 1) && li.launches - l0 == 5 && li.nframes == 25);
		CHECK(handed(out8, 1, 25) && g_with_models - m0 == 5 && g_programmed == p0);
		CHECK(Regs() == want_plain);
		l0 = launches();
		OK(call(out8, src, dst2, ms.data(), seeds.data(), n, f, fill, shift, st));
		CHECK(launches() - l0 == 5 && Regs() == want_seeded && g_with_models - m0 == 10);
		// a list that ends on the general form: the last run is its kernel's
		OK(call(out8, src, dst2, ms.data(), seeds.data(), 45, f, fill, shift, st));
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && named(li, out8, depth, sy, 0, 0) && li.nframes == 2 && handed(out8, 1, 2));
		// the programmed state is the caller's: the programmed call behind it, the model programmed last, without models_kernel
		if (out8) OK(vfgs_hip_add_grain_frame_list_to_sp8_dev(src.list.data(), dst.list.data(), nullptr, 2, w, h, f.stride, f.cstride, fill.stride, fill.cstride, st));
		else OK(vfgs_hip_add_grain_frame_list_to_sp_dev(src.list.data(), dst.list.data(), nullptr, 2, w, h, f.stride, f.cstride, fill.stride, fill.cstride, shift, st));
		CHECK(vfgs_hip_last_launch_info(&li) == 0 && named(li, out8, depth, sy, 1, 1) && li.nframes == 2 && handed(out8, 0, 2) && g_programmed - p0 == 1);
		hipStreamSynchronize(st);
		CHECK(src.all_hold(f) && dst.all_hold(want) && dst2.all_hold(want));
		for (const vfgs_hip_model* m : {gen, o1, o2}) touch_model(m);
		vfgs_hip_model_release(gen); vfgs_hip_model_release(o1); vfgs_hip_model_release(o2);
	}
	hipStreamDestroy(st);
}

// captured on one stream, used on another, released right after the call with everything queued; an overlap region
static void walk_release_right_after_the_call()
{
	hipStream_t sa = nullptr, sb = nullptr;
	hipStreamCreateWithFlags(&sa, 1);
	hipStreamCreateWithFlags(&sb, 1);
	for (int out8 = 0; out8 < 2; out8++)
	{
		program(10, 2, 2, true);
		vfgs_hip_model* a = capture(sa);
		program(10, 2, 2, true, 4, 1);
		vfgs_hip_model* b = capture(sb);
		Pic f(true, 520, 70, 2, 2), fill(false, 520, 70, 2, out8 ? 1 : 2, 16, 32);
		const Pic want = modelled(f, fill, out8 != 0);
		const unsigned shift = out8 ? 0 : 6;
		SrcPool src(f, 6);
		DstPool dst(fill, 6);
		const vfgs_hip_model* ms[6] = {a, b, a, b, a, b};
		OK(call(out8 != 0, src, dst, ms, nullptr, 6, f, fill, shift, sb));
		vfgs_hip_model_release(a);                     // right after the call returns
		vfgs_hip_model_release(a);                     // twice: no-op
		const Regs r0;
		const unsigned long long l0 = launches();
		CHECK(call(out8 != 0, src, dst, ms, nullptr, 6, f, fill, shift, sb) == 41 && strstr(vfgs_hip_last_error_string(), "frame 0 is not a live model"));
		CHECK(Regs() == r0 && launches() == l0);       // a released entry: refused, nothing changed
		for (int i = 0; i < 12; i++)
		{
			vfgs_hip_model* t = capture(i & 1 ? sa : sb);
			touch_model(t);
			vfgs_hip_model_release(t);
		}
		hipStreamSynchronize(sb);
		CHECK(src.all_hold(f) && dst.all_hold(want));
		touch_model(b);
		// two calls inside an overlap region, a release inside it
		program(10, 2, 2, false);
		vfgs_hip_model* c = capture(sa);
		vfgs_set_seed(3);
		const Regs regs = planar_regs(f, 7, nullptr);
		SrcPool sa4(f, 4), sb3(f, 3);
		DstPool da(fill, 4), db(fill, 3);
		const vfgs_hip_model* ma[4] = {b, b, c, b};
		const vfgs_hip_model* mb[3] = {c, b, b};
		vfgs_set_seed(3);
		OK(vfgs_hip_overlap_begin(sa));
		OK(call(out8 != 0, sa4, da, ma, nullptr, 4, f, fill, shift, sa));
		OK(call(out8 != 0, sb3, db, mb, nullptr, 3, f, fill, shift, sa));
		vfgs_hip_model_release(b);                     // inside the region, with both calls queued on its internal streams
		OK(vfgs_hip_overlap_end(sa));
		CHECK(Regs() == regs && handed(out8 != 0, 1, 2));
		hipStreamSynchronize(sa);
		CHECK(da.all_hold(want) && db.all_hold(want) && sa4.all_hold(f) && sb3.all_hold(f));
		touch_model(c);
		vfgs_hip_model_release(c);
	}
	hipStreamDestroy(sa);
	hipStreamDestroy(sb);
}

// every refusal with its code, in the order the header states: 40, 16, 18 (a null list), 6 / 8 (the destination's pitches), the list checks
// (18, 7, 5 / 6 / 8), 15, then 41
static void walk_refusals()
{
	for (int out8 = 0; out8 < 2; out8++)
	{
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
		Pic f(true, 520, 70, 2, 2, 0, 0), fill(false, 520, 70, 2, out8 ? 1 : 2, 16, 32);
		const Pic want = modelled(f, fill, out8 != 0);
		SrcPool src(f, 3);
		DstPool dst(fill, 3);
		const std::vector<uint32_t> seeds = seeds_of(3);
		const Regs regs = planar_regs(f, 3, seeds.data());
		vfgs_set_seed(5);
		const Regs before;
		const unsigned long long l0 = launches();
		const uint64_t m0 = g_with_models;
		const Stats b0;
		const vfgs_hip_model* ok[3] = {a, b, a};
		const unsigned h = f.h, s = f.stride, u = f.cstride, ds = fill.stride, du = fill.cstride, good = out8 ? 0 : 6;
		// (0: the good value)
		auto raw = [&](const vfgs_hip_frame_ptrs* S, const vfgs_hip_sp_frame* D, const vfgs_hip_model* const* ms, unsigned ww = 520, unsigned ss = 0, unsigned uu = 0,
		               unsigned shift = 99, unsigned dss = 0, unsigned duu = 0, unsigned hh = 0) {
			if (shift == 99) shift = good;
			const int rc = out8 ? vfgs_hip_add_grain_frame_list_models_to_sp8_dev(S, D, ms, seeds.data(), 3, ww, hh ? hh : h, ss ? ss : s, uu ? uu : u, dss ? dss : ds, duu ? duu : du, nullptr)
			                    : vfgs_hip_add_grain_frame_list_models_to_sp_dev(S, D, ms, seeds.data(), 3, ww, hh ? hh : h, ss ? ss : s, uu ? uu : u, dss ? dss : ds, duu ? duu : du, shift, nullptr);
			CHECK(rc == 0 || rc == vfgs_hip_last_error());
			return rc;
		};
		auto L = src.list;
		auto D = dst.list;
		auto with = [&](const vfgs_hip_model* const* ms) { return raw(L.data(), D.data(), ms); };
		// 41, each cause
		CHECK(with(nullptr) == 41 && strstr(vfgs_hip_last_error_string(), "null list of models"));
		{ const vfgs_hip_model* ms[3] = {a, nullptr, a}; CHECK(with(ms) == 41 && strstr(vfgs_hip_last_error_string(), "frame 1 is null")); }
		{ const vfgs_hip_model* ms[3] = {a, b, gone}; CHECK(with(ms) == 41 && strstr(vfgs_hip_last_error_string(), "frame 2 is not a live model")); }
		{ const vfgs_hip_model* ms[3] = {a, m8, a}; CHECK(with(ms) == 41 && strstr(vfgs_hip_last_error_string(), "depth 8")); }
		{ const vfgs_hip_model* ms[3] = {m422, b, a}; CHECK(with(ms) == 41 && strstr(vfgs_hip_last_error_string(), "2,1")); }
		{ const vfgs_hip_model* ms[3] = {a, b, mixed}; CHECK(with(ms) == 41 && strstr(vfgs_hip_last_error_string(), "chroma mix") && strstr(vfgs_hip_last_error_string(), "frame 2")); }
		OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
		CHECK(with(ok) == 41 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
		// (the programmed calls keep their own refusal under a programmed mix: 40)
		if (out8) CHECK(vfgs_hip_add_grain_frame_list_to_sp8_dev(L.data(), D.data(), seeds.data(), 3, 520, h, s, u, ds, du, nullptr) == 40);
		else CHECK(vfgs_hip_add_grain_frame_list_to_sp_dev(L.data(), D.data(), seeds.data(), 3, 520, h, s, u, ds, du, 6, nullptr) == 40);
		vfgs_hip_clear_chroma_mix();
		// the order.  40 in front of everything: a bad shift, a width walked in parts, csubx 1 -- with null lists, null models, bad pitches
		if (!out8) CHECK(raw(nullptr, nullptr, nullptr, 520, 0, 0, 4, 8, 8) == 40 && strstr(vfgs_hip_last_error_string(), "sample_shift 4"));
		CHECK(raw(nullptr, D.data(), nullptr, 8208, 8208, 4104, 99, 8208, 8208) == 40 && strstr(vfgs_hip_last_error_string(), "width 8208"));
		vfgs_set_chroma_subsampling(1, 1);
		CHECK(raw(nullptr, nullptr, nullptr) == 40 && strstr(vfgs_hip_last_error_string(), "csubx 1"));
		vfgs_set_chroma_subsampling(2, 2);
		// 16 (the narrowed call at depth 8) behind 40, in front of the null list; the call in the depth's container has no such refusal
		vfgs_set_depth(8);
		if (out8) CHECK(raw(nullptr, nullptr, nullptr) == 16);
		else CHECK(raw(nullptr, nullptr, nullptr, 520, 0, 0, 6) == 40 && raw(nullptr, nullptr, nullptr, 520, 0, 0, 0) == 18);
		vfgs_set_depth(10);
		// 18 for a null list in front of the destination's pitches; 6 / 8 for those in front of the list checks
		CHECK(raw(nullptr, D.data(), nullptr, 520, 0, 0, 99, 512) == 18 && raw(L.data(), nullptr, nullptr, 520, 0, 0, 99, 0, ds + 4) == 18);
		L[1].U = (uint8_t*)L[1].U + 8;                  // (a misaligned source plane: 7, one of the list checks)
		CHECK(raw(L.data(), D.data(), nullptr) == 7);
		CHECK(raw(L.data(), D.data(), nullptr, 520, 0, 0, 99, 512) == 6 && raw(L.data(), D.data(), nullptr, 520, 0, 0, 99, 0, 264) == 6);
		CHECK(raw(L.data(), D.data(), nullptr, 520, 0, 0, 99, ds + 4) == 8 && raw(L.data(), D.data(), nullptr, 520, 0, 0, 99, 0, du + 4) == 8);
		L = src.list;
		// the list checks in front of 41: null planes, misaligned planes, the source's geometry, planes that share bytes
		L[1].V = nullptr;
		CHECK(raw(L.data(), D.data(), nullptr) == 18);
		L = src.list; D[2].UV = nullptr;
		CHECK(raw(L.data(), D.data(), nullptr) == 18);
		D = dst.list; D[2].Y = (uint8_t*)D[2].Y + 4;
		CHECK(raw(L.data(), D.data(), nullptr) == 7);
		D = dst.list;
		CHECK(raw(L.data(), D.data(), nullptr, 100) == 5);
		CHECK(raw(L.data(), D.data(), nullptr, 520, 512) == 6 && raw(L.data(), D.data(), nullptr, 520, 0, 256) == 6);
		CHECK(raw(L.data(), D.data(), nullptr, 520, s + 4) == 8 && raw(L.data(), D.data(), nullptr, 520, 0, u + 4) == 8);
		D[2] = D[0];
		CHECK(raw(L.data(), D.data(), nullptr) == 18 && strstr(vfgs_hip_last_error_string(), "listed twice"));
		D = dst.list; D[1].Y = L[1].Y;
		CHECK(raw(L.data(), D.data(), ok) == 18);      // its own frame's source luma: no in-place form
		D = dst.list; D[0].UV = (uint8_t*)L[2].V + 1024;
		CHECK(raw(L.data(), D.data(), ok) == 18);      // inside another frame's source Cr
		D = dst.list;
		// 15: ONE picture whose luma plane reaches the 2 GiB buffer window (1864136 rows x 576 samples x 2 bytes; refused before anything is
		// touched: its planes are addresses, 8 GiB apart) -- behind the list checks, in front of 41; one row fewer and the null models are named
		{
			auto far = [](uintptr_t k) { return (void*)(k << 33); };
			const vfgs_hip_frame_ptrs bs = {far(1), far(2), far(3)};
			const vfgs_hip_sp_frame bd = {far(4), far(5)};
			auto big = [&](unsigned rows) {
				return out8 ? vfgs_hip_add_grain_frame_list_models_to_sp8_dev(&bs, &bd, nullptr, seeds.data(), 1, 520, rows, 576, 288, 528, 544, nullptr)
				            : vfgs_hip_add_grain_frame_list_models_to_sp_dev(&bs, &bd, nullptr, seeds.data(), 1, 520, rows, 576, 288, 528, 544, 6, nullptr);
			};
			CHECK(big(1864136) == 15 && strstr(vfgs_hip_last_error_string(), "2 GiB"));
			CHECK(big(1864135) == 41);
		}
		// the programmed state's own troubles are not the models': an undefined pattern-LUT entry
		unsigned char lut[256];
		memset(lut, 0x90, sizeof lut);
		vfgs_set_pattern_lut(1, lut);
		// an empty list is no call at all, whatever else it says
		if (out8) OK(vfgs_hip_add_grain_frame_list_models_to_sp8_dev(nullptr, nullptr, nullptr, nullptr, 0, 100, 70, 0, 0, 0, 0, nullptr));
		else OK(vfgs_hip_add_grain_frame_list_models_to_sp_dev(nullptr, nullptr, nullptr, nullptr, 0, 100, 70, 0, 0, 0, 0, 99, nullptr));
		CHECK(Regs() == before && launches() == l0 && g_with_models == m0 && Stats() == b0);
		hipDeviceSynchronize();
		CHECK(src.all_hold(f) && dst.all_hold(fill));
		// the same lists are served afterwards (with the undefined LUT entry still programmed): A | B | A, three runs
		OK(with(ok));
		CHECK(Regs() == regs && launches() - l0 == 3 && g_with_models - m0 == 3 && handed(out8 != 0, 1, 1));
		hipDeviceSynchronize();
		CHECK(src.all_hold(f) && dst.all_hold(want));
		for (const vfgs_hip_model* m : {a, b, m8, m422, mixed}) touch_model(m);
		// the models stay live: vfgs_hip_shutdown at the end of main releases what is left (the leak check says whether it did)
	}
}

static void walk_two_threads()
{
	// two threads, pools, models' lists and a stream each, calling at once: the library serialises them; with a seed per picture the registers a
	// thread's last call leaves do not show the order as long as both end on the same seed
	program(10, 2, 2, true);
	vfgs_hip_model* a = capture(nullptr);
	program(10, 2, 2, true, 4, 1);
	vfgs_hip_model* b = capture(nullptr);
	Pic f(true, 520, 70, 2, 2), fill(false, 520, 70, 2, 2, 16, 0), fill8(false, 520, 70, 2, 1, 0, 16);
	const std::vector<uint32_t> seeds = seeds_of(6);
	const Regs want = planar_regs(f, 6, seeds.data());
	SrcPool sa(f, 6), sb(f, 6);
	DstPool da(fill, 6), db(fill8, 6);
	const vfgs_hip_model* ma[6] = {a, b, a, b, b, a};
	const vfgs_hip_model* mb[6] = {b, b, a, a, b, a};
	hipStream_t st[2] = {nullptr, nullptr};
	hipStreamCreateWithFlags(&st[0], 1);
	hipStreamCreateWithFlags(&st[1], 1);
	const uint64_t m0 = g_with_models;
	int rc[2] = {0, 0};
	auto work = [&](int t) {
		for (int k = 0; k < 8 && !rc[t]; k++)
			rc[t] = t ? call(true, sb, db, mb, seeds.data(), 6, f, fill8, 0, st[1]) : call(false, sa, da, ma, seeds.data(), 6, f, fill, 6, st[0]);
	};
	std::thread ta(work, 0), tb(work, 1);
	ta.join(); tb.join();
	CHECK(rc[0] == 0 && rc[1] == 0);
	CHECK(Regs() == want && g_with_models - m0 == 16);      // (both models are of one form: a launch per call)
	hipStreamSynchronize(st[0]);
	hipStreamSynchronize(st[1]);
	CHECK(sa.all_hold(f) && sb.all_hold(f) && da.all_hold(modelled(f, fill, false)) && db.all_hold(modelled(f, fill8, true)));
	touch_model(a); touch_model(b);
	vfgs_hip_model_release(a); vfgs_hip_model_release(b);
	hipStreamDestroy(st[0]);
	hipStreamDestroy(st[1]);
}

int main(int argc, char** argv)
{
	// run_walks shuts down with live models (walk_refusals leaves ten)
	return run_walks(argc, argv, {
		{"runs_across_forms", walk_runs_across_forms},
		{"release_right_after_the_call", walk_release_right_after_the_call},
		{"refusals", walk_refusals},
		{"two_threads", walk_two_threads},
	});
}
