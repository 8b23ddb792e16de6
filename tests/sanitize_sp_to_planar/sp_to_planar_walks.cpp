// TEST INFRASTRUCTURE.  Semi-planar surfaces in, planar pictures out (include/vfgs_hip.h: vfgs_hip_add_grain_sp_frame_list_to_planar_dev and
// vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev) in the host layer of libvfgs_hip, compiled with a sanitizer over the unchanged
// tests/sanitize/hip_stub.cpp, as tests/sanitize_models_to_sp/models_to_sp_walks.cpp drives the opposite direction: both entry points with
// and without seeds, odd block counts, every depth, 35 frames (a second launch), models that change form (a launch per run), an overlap
// region, every refusal with nothing changed, and two threads calling at once.  Every plane is allocated exactly as large as the contract
// says: (rows - 1) pitches and one row of whole blocks, a UV row of 16 containers per block, a planar chroma row of 8.
//
// The model of the HIP runtime is compiled INTO this translation unit, unchanged, with its launcher of the grain kernels under another
// name: vfgs::launch_grain below stands where vfgs_kernel.hip's does.  A launch with KernelArgs::sp_kernel == 3 is held to what
// launch_args_ok holds it to -- families sp and spml only, family_fields() of the key with its third argument, listed whole frames, three
// destination planes per frame, pd[1].drowbytes ONE component's half of the UV row -- and is then MODELLED HERE, because the model's row
// copy knows no planar destination: "grain" of zero, every luma container >> shift to the destination's luma row at ITS pitch, the even
// containers of a UV row >> shift to the Cb row and the odd ones to the Cr row at THEIR pitch, exactly drowbytes bytes a row -- so the
// extents and pitches of all five planes are proven by the sanitizer, and what lands in the destinations is compared byte for byte
// (`modelled` restates it), pad bytes included.  Every other launch is passed on to the model.  Values are the GPU suite's business
// (tests/test_gpu_sp_to_planar.py).
//
// usage: sp_to_planar_walks [walk ...]     (no argument: all of them)
#define launch_grain stub_launch_grain
#include "../sanitize/hip_stub.cpp"
#undef launch_grain

#include <hip/hip_runtime.h>

#include <type_traits>

#define WALKS_SEED 1357
#define WALKS_HAVE_HIP_RUNTIME_H
#include "../sanitize/walks.h"

// what the launcher was handed: the last launch, and how many launches onto planes
struct Handed { vfgs::Family family; int models_kernel, mix_kernel, sp_kernel, listed, nframes; bool out8; };
static Handed g_handed;      // (written under the library's lock; the walk with two threads reads it after the join)
static std::atomic<uint64_t> g_to_planar{0};

namespace vfgs {
hipError_t launch_grain(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream)
{
	g_handed = Handed{k.family, a.models_kernel, a.mix_kernel, a.sp_kernel, a.listed, a.nframes, k.out8};
	if (a.sp_kernel != 3)
	{
		// (the existing launches say what they said: the two-argument family_fields() still answers for them)
		if ((k.family == Family::sp || k.family == Family::spml) && family_fields(k.family).sp_kernel != a.sp_kernel) { fprintf(stderr, "FAILED launcher: sp_kernel %d\n", a.sp_kernel); g_fail++; }
		return stub_launch_grain(a, list, k, grid, stream);
	}
	const FamilyFields ff = family_fields(k.family, false, true);
	const int sz = k.depth > 8 ? 2 : 1;
	bool ok = (k.family == Family::sp || k.family == Family::spml) && ff.sp_kernel == 3 && a.models_kernel == ff.models_kernel && a.mix_kernel == 0 && kernel_exists(k) &&
	          !k.out8 && list && a.listed == 1 && a.y0 == 0 && a.nframes <= kListFrames && grid > 0 && a.nblk <= kTileBlocks &&
	          a.pd[0].rowbytes == (uint32_t)(a.nblk * 16 * sz) && a.pd[1].rowbytes == a.pd[0].rowbytes && a.pd[0].drowbytes == a.pd[0].rowbytes &&
	          2 * a.pd[1].drowbytes == a.pd[1].rowbytes && a.pd[0].dpitch >= a.pd[0].drowbytes && a.pd[1].dpitch >= a.pd[1].drowbytes &&
	          !((a.pd[0].dpitch | a.pd[1].dpitch) & 15) && (k.depth == 8 ? a.sp_shift2 == 0 : (a.sp_shift2 >> 16) == (a.sp_shift2 & 0xffffu));
	for (int i = 0; ok && i < a.nframes; i++)
	{
		ok = list->src[1][i] == list->src[2][i] && list->dst[0][i] && list->dst[1][i] && list->dst[2][i] && list->dst[1][i] != list->dst[2][i];
		if (ok && a.models_kernel) ok = list->model[i] && !((uintptr_t)list->model[i] & 15);
	}
	if (ok && a.models_kernel) ok = a.tables == list->model[0] + kModelRecordBytes;
	if (!ok)
	{
		fprintf(stderr, "FAILED launcher: family %d with models_kernel %d, mix_kernel %d, sp_kernel %d, out8 %d is not a launch the real launcher takes\n",
		        (int)k.family, a.models_kernel, a.mix_kernel, a.sp_kernel, (int)k.out8);
		g_fail++;
		return hipErrorInvalidValue;
	}
	g_to_planar++;
	const KernelArgs c = a;
	const FrameTable ft = *list;
	const int depth = k.depth, csuby = k.csuby;
	const bool oney = k.oney, onec = k.onec;
	std::lock_guard<std::recursive_mutex> g(g_mu);
	g_stats_deferred++;
	enqueue(stream, [=] {
		const ImageLayout L = image_layout(2, csuby, oney, onec, depth == 8);
		touch(c.tables, (size_t)L.bytes);
		touch(c.stream, c.stream_bytes);
		const unsigned shift = c.sp_shift2 & 0xffffu;
		for (int f = 0; f < c.nframes; f++)
		{
			for (int r = 0; r < c.pd[0].nrows; r++)
			{
				const uint8_t* s = ft.src[0][f] + (size_t)r * c.pd[0].pitch;
				uint8_t* d = ft.dst[0][f] + (size_t)r * c.pd[0].dpitch;
				for (uint32_t i = 0; i < c.pd[0].drowbytes / sz; i++)
				{
					if (sz == 2) ((uint16_t*)d)[i] = (uint16_t)(((const uint16_t*)s)[i] >> shift);
					else d[i] = s[i];
				}
			}
			for (int r = 0; r < c.pd[1].nrows; r++)
			{
				const uint8_t* s = ft.src[1][f] + (size_t)r * c.pd[1].pitch;
				uint8_t* u = ft.dst[1][f] + (size_t)r * c.pd[1].dpitch;
				uint8_t* v = ft.dst[2][f] + (size_t)r * c.pd[1].dpitch;
				for (uint32_t i = 0; i < c.pd[1].drowbytes / sz; i++)
				{
					if (sz == 2)
					{
						((uint16_t*)u)[i] = (uint16_t)(((const uint16_t*)s)[2 * i] >> shift);
						((uint16_t*)v)[i] = (uint16_t)(((const uint16_t*)s)[2 * i + 1] >> shift);
					}
					else { u[i] = s[2 * i]; v[i] = s[2 * i + 1]; }
				}
			}
		}
	});
	return hipSuccess;
}
}  // namespace vfgs

static bool handed(bool models, int nframes)
{
	return g_handed.family == (models ? vfgs::Family::spml : vfgs::Family::sp) && g_handed.models_kernel == (models ? 1 : 0) && g_handed.mix_kernel == 0 &&
	       g_handed.sp_kernel == 3 && g_handed.listed == 1 && !g_handed.out8 && g_handed.nframes == nframes;
}

// the two entry points exist with these C types; the kernel arguments have not moved; the existing callers of family_fields() get what they got
using to_planar_fn = int (*)(const vfgs_hip_sp_frame*, const vfgs_hip_frame_ptrs*, const uint32_t*, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned,
                             unsigned, void*);
using models_to_planar_fn = int (*)(const vfgs_hip_sp_frame*, const vfgs_hip_frame_ptrs*, const vfgs_hip_model* const*, const uint32_t*, unsigned, unsigned, unsigned,
                                    unsigned, unsigned, unsigned, unsigned, unsigned, void*);
static_assert(std::is_same<decltype(&vfgs_hip_add_grain_sp_frame_list_to_planar_dev), to_planar_fn>::value, "vfgs_hip_add_grain_sp_frame_list_to_planar_dev");
static_assert(std::is_same<decltype(&vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev), models_to_planar_fn>::value, "vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev");
static_assert(sizeof(vfgs::KernelArgs) == 312 && offsetof(vfgs::FrameTable, model) == 6 * 8 * vfgs::kListFrames, "what the kernels of before load has not moved");
static_assert(vfgs::family_fields(vfgs::Family::sp).sp_kernel == 1 && vfgs::family_fields(vfgs::Family::spml, false).sp_kernel == 1 &&
              vfgs::family_fields(vfgs::Family::sp, false, true).sp_kernel == 3 && vfgs::family_fields(vfgs::Family::spml, false, true).sp_kernel == 3 &&
              vfgs::family_fields(vfgs::Family::spml, false, true).models_kernel == 1 && vfgs::family_fields(vfgs::Family::sp8, false, true).sp_kernel == 1 &&
              vfgs::family_fields(vfgs::Family::p2sp, false, true).sp_kernel == 2 && vfgs::family_fields(vfgs::Family::sp_mix, false, true).sp_kernel == 1 &&
              vfgs::family_fields(vfgs::Family::rw, false, true).sp_kernel == 0, "planes out: the families sp and spml alone");

// a planar destination of `sz`-byte samples, its planes exactly as large as the contract says; pad / cpad: samples a row pitch exceeds the
// whole blocks by (an 8-bit chroma row of an odd number of blocks: a pitch of whole 16-byte units has 8 pad bytes)
struct PlPic {
	int w, h, sy, sz, nblk, stride, cstride, crows;
	std::vector<uint8_t> P[3];
	PlPic(int w_, int h_, int sy_, int sz_, int pad = 0, int cpad = 0) : w(w_), h(h_), sy(sy_), sz(sz_)
	{
		nblk = (w + 15) / 16;
		stride = nblk * 16 + pad;
		cstride = (nblk * 8 * sz + 15) / 16 * 16 / sz + cpad;
		crows = (h + sy - 1) / sy;
		P[0].resize(((size_t)(h - 1) * stride + nblk * 16) * sz);
		P[1].resize(((size_t)(crows - 1) * cstride + nblk * 8) * sz);
		P[2].resize(P[1].size());
		for (auto& p : P)
			for (auto& b : p) b = (uint8_t)rnd();
	}
};

struct DevPl {
	uint8_t* p[3] = {nullptr, nullptr, nullptr};
	size_t n[3];
	explicit DevPl(const PlPic& f) : n{f.P[0].size(), f.P[1].size(), f.P[2].size()}
	{
		for (int i = 0; i < 3; i++) { hipMalloc((void**)&p[i], n[i]); to_device(p[i], f.P[i].data(), n[i]); }
	}
	~DevPl() { for (auto* q : p) hipFree(q); }
	DevPl(const DevPl&) = delete;
	vfgs_hip_frame_ptrs ptrs() const { return {p[0], p[1], p[2]}; }
	bool holds(const PlPic& f) const
	{
		for (int i = 0; i < 3; i++)
		{
			std::vector<uint8_t> got(n[i]);
			to_host(got.data(), p[i], n[i]);
			if (got != f.P[i]) return false;
		}
		return true;
	}
};
using PlPool = PoolOf<PlPic, DevPl, vfgs_hip_frame_ptrs>;

// what the launch modelled above leaves in a destination that held `fill`
static PlPic modelled(const SpPic& s, const PlPic& fill, unsigned shift)
{
	PlPic out = fill;
	const int sz = s.sz;
	auto get = [&](const std::vector<uint8_t>& p, size_t i) { return sz == 2 ? (unsigned)(p[2 * i] | p[2 * i + 1] << 8) >> shift : (unsigned)p[i]; };
	auto put = [&](std::vector<uint8_t>& p, size_t i, unsigned v) { if (sz == 2) { p[2 * i] = (uint8_t)v; p[2 * i + 1] = (uint8_t)(v >> 8); } else p[i] = (uint8_t)v; };
	for (int r = 0; r < s.h; r++)
		for (int i = 0; i < s.nblk * 16; i++) put(out.P[0], (size_t)r * fill.stride + i, get(s.Y, (size_t)r * s.stride + i));
	for (int r = 0; r < s.crows; r++)
		for (int i = 0; i < s.nblk * 8; i++)
		{
			put(out.P[1], (size_t)r * fill.cstride + i, get(s.UV, (size_t)r * s.uv_stride + 2 * i));
			put(out.P[2], (size_t)r * fill.cstride + i, get(s.UV, (size_t)r * s.uv_stride + 2 * i + 1));
		}
	return out;
}

// the registers the contract names: those of the semi-planar call (with models: of the call with models) out of place on the same sources
static Regs sp_regs(const SpPic& f, int n, const uint32_t* seeds, unsigned shift, const vfgs_hip_model* const* models = nullptr)
{
	SpPool s(f, n), d(f, n);
	if (models) OK(vfgs_hip_add_grain_sp_frame_list_models_dev(s.list.data(), d.list.data(), models, seeds, n, f.w, f.h, f.stride, f.uv_stride, shift, nullptr));
	else OK(vfgs_hip_add_grain_sp_frame_list_dev(s.list.data(), d.list.data(), seeds, n, f.w, f.h, f.stride, f.uv_stride, shift, nullptr));
	hipDeviceSynchronize();
	return Regs();
}

static bool named(const vfgs_hip_launch_info& li, bool models, int depth)
{
	const char* want = models ? "grain_spml_kernel<" : "grain_sp_kernel<";
	return !strncmp(li.kernel, want, strlen(want)) && li.out8 == 0 && li.listed == 1 && li.in_place == 0 && li.persistent_luma_workgroups == 0 && li.depth == depth;
}

static int to_planar(const SpPool& s, const PlPool& d, const vfgs_hip_model* const* models, const uint32_t* seeds, int n, const SpPic& f, const PlPic& fill, unsigned shift, void* st)
{
	if (models)
		return vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev(s.list.data(), d.list.data(), models, seeds, n, f.w, f.h, f.stride, f.uv_stride, fill.stride, fill.cstride, shift, st);
	return vfgs_hip_add_grain_sp_frame_list_to_planar_dev(s.list.data(), d.list.data(), seeds, n, f.w, f.h, f.stride, f.uv_stride, fill.stride, fill.cstride, shift, st);
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_both_entry_points()
{
	hipStream_t st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	// depth, width, height, csuby, one-pattern model, sample shift, source padding of Y / UV, destination padding of Y / of a chroma row
	// (containers / samples): odd block counts (9, 13, 21, 65), a single block row, the widest row, every depth, pitches below the source's
	const int cases[][10] = {{10, 200, 150, 2, 1, 6, 0, 0, 0, 0},  {10, 520, 39, 2, 0, 0, 32, 16, 16, 8}, {8, 328, 39, 2, 0, 0, 16, 48, 0, 0},  {8, 136, 33, 1, 1, 0, 0, 0, 16, 16},
	                         {12, 1032, 33, 1, 0, 4, 8, 8, 0, 24}, {8, 1040, 96, 2, 1, 0, 0, 0, 16, 0},   {10, 8192, 17, 2, 0, 6, 0, 0, 0, 8}, {12, 328, 40, 2, 1, 0, 64, 0, 0, 0}};
	for (const auto& c : cases)
	{
		const int depth = c[0], w = c[1], h = c[2], sy = c[3], n = 5, sz = depth > 8 ? 2 : 1;
		const unsigned shift = (unsigned)c[5];
		SpPic f(w, h, sy, sz, c[6], c[7]);
		PlPic fill(w, h, sy, sz, c[8], c[9]);
		const PlPic want = modelled(f, fill, shift);
		const std::vector<uint32_t> seeds = seeds_of(n);
		for (int with_models = 0; with_models < 2; with_models++)
		{
			program(depth, 2, sy, c[4] != 0);
			std::vector<const vfgs_hip_model*> models;
			if (with_models)
			{
				vfgs_hip_model* m = capture(st);
				models.assign(n, m);
			}
			const vfgs_hip_model* const* mp = with_models ? models.data() : nullptr;
			vfgs_set_seed(99);
			const Regs want_plain = sp_regs(f, n, nullptr, shift, mp);
			const Regs want_seeded = sp_regs(f, n, seeds.data(), shift, mp);
			SpPool src(f, n);
			vfgs_hip_launch_info a, b;
			{
				// one seed sequence
				PlPool dst(fill, n);
				vfgs_set_seed(99);
				CHECK(vfgs_hip_last_launch_info(&a) == 0);
				const uint64_t n0 = g_to_planar;
				OK(to_planar(src, dst, mp, nullptr, n, f, fill, shift, st));
				CHECK(Regs() == want_plain);
				CHECK(vfgs_hip_last_launch_info(&b) == 0 && named(b, with_models != 0, depth) && b.nframes == n && b.launches - a.launches == 1);
				CHECK(handed(with_models != 0, n) && g_to_planar - n0 == 1);
				hipStreamSynchronize(st);
				CHECK(dst.all_hold(want) && src.all_hold(f));
			}
			{
				// a seed per picture
				PlPool dst(fill, n);
				vfgs_set_seed(7);
				OK(to_planar(src, dst, mp, seeds.data(), n, f, fill, shift, st));
				CHECK(Regs() == want_seeded);
				CHECK(vfgs_hip_last_launch_info(&b) == 0 && named(b, with_models != 0, depth) && handed(with_models != 0, n));
				hipStreamSynchronize(st);
				CHECK(dst.all_hold(want) && src.all_hold(f));
			}
			if (with_models) { touch_model(models[0]); vfgs_hip_model_release(const_cast<vfgs_hip_model*>(models[0])); }
		}
	}
	hipStreamDestroy(st);
}

static void walk_thirty_five_frames()
{
	program(10, 2, 2, true);
	SpPic f(264, 40, 2, 2, 16, 0);
	PlPic fill(264, 40, 2, 2, 0, 8);
	const PlPic want = modelled(f, fill, 6);
	const std::vector<uint32_t> seeds = seeds_of(35);
	const Regs want_seeded = sp_regs(f, 35, seeds.data(), 6);
	SpPool src(f, 35);
	PlPool dst(fill, 35);
	vfgs_hip_launch_info a, b;
	CHECK(vfgs_hip_last_launch_info(&a) == 0);
	OK(to_planar(src, dst, nullptr, seeds.data(), 35, f, fill, 6, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 2 && b.nframes == 3 && named(b, false, 10) && handed(false, 3));
	CHECK(Regs() == want_seeded);
	vfgs_set_seed(5);
	const Regs want_plain = sp_regs(f, 35, nullptr, 6);
	vfgs_set_seed(5);
	CHECK(vfgs_hip_last_launch_info(&a) == 0);
	OK(to_planar(src, dst, nullptr, nullptr, 35, f, fill, 6, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 2 && b.nframes == 3);
	CHECK(Regs() == want_plain);
	hipDeviceSynchronize();
	CHECK(src.all_hold(f) && dst.all_hold(want));
}

static void walk_models_change_form()
{
	// A A B B B A: models of two forms, a launch per run; the programmed state is what it was
	hipStream_t st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	program(10, 2, 1, true);
	vfgs_hip_model* A = capture(st);
	program(10, 2, 1, false);
	vfgs_hip_model* B = capture(st);
	const vfgs_hip_model* models[6] = {A, A, B, B, B, A};
	SpPic f(328, 39, 1, 2, 0, 16);
	PlPic fill(328, 39, 1, 2, 16, 0);
	const std::vector<uint32_t> seeds = seeds_of(6);
	const Regs want = sp_regs(f, 6, seeds.data(), 6, models);
	int before[8], after[8];
	vfgs_hip_get_params(before);
	SpPool src(f, 6);
	PlPool dst(fill, 6);
	vfgs_hip_launch_info a, b;
	CHECK(vfgs_hip_last_launch_info(&a) == 0);
	const uint64_t n0 = g_to_planar;
	OK(to_planar(src, dst, models, seeds.data(), 6, f, fill, 6, st));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 3 && b.nframes == 1 && named(b, true, 10) && handed(true, 1) && g_to_planar - n0 == 3);
	CHECK(Regs() == want);
	vfgs_hip_get_params(after);
	CHECK(!memcmp(before, after, sizeof before));
	hipStreamSynchronize(st);
	CHECK(src.all_hold(f) && dst.all_hold(modelled(f, fill, 6)));
	// a released model is refused, nothing changed
	const Regs regs;
	vfgs_hip_model_release(B);
	PlPool again(fill, 6);
	CHECK(to_planar(src, again, models, seeds.data(), 6, f, fill, 6, st) == 41);
	CHECK(Regs() == regs && again.all_hold(fill));
	// a model that CARRIES a mix and a model of another chroma format are the models' to refuse (41), each named, nothing changed
	{
		program(Model{10, 2, 1, true, true, 5, 0, 1});
		vfgs_hip_model* M = nullptr;
		OK(vfgs_hip_model_capture_mix(&M, st));
		program(10, 2, 2, true);
		vfgs_hip_model* F = capture(st);
		program(10, 2, 1, true);          // (4:2:2 again, no mix programmed)
		int mix[4] = {0, 0, 0, 0};
		OK(vfgs_hip_model_chroma_mix(M, 1, mix));
		CHECK(mix[3] == 1);
		const Regs r0;
		const unsigned long long l0 = launches();
		const vfgs_hip_model* with_mix[6] = {A, A, A, M, A, A};
		CHECK(to_planar(src, again, with_mix, seeds.data(), 6, f, fill, 6, st) == 41 && strstr(vfgs_hip_last_error_string(), "carries a chroma mix"));
		CHECK(to_planar(src, again, with_mix, nullptr, 6, f, fill, 6, st) == 41);
		const vfgs_hip_model* other[6] = {A, F, A, A, A, A};
		CHECK(to_planar(src, again, other, seeds.data(), 6, f, fill, 6, st) == 41 && strstr(vfgs_hip_last_error_string(), "chroma subsampling 2,2"));
		CHECK(Regs() == r0 && launches() == l0);
		hipStreamSynchronize(st);
		CHECK(again.all_hold(fill) && src.all_hold(f));
		vfgs_hip_model_release(M);
		vfgs_hip_model_release(F);
	}
	vfgs_hip_model_release(A);
	hipStreamDestroy(st);
}

static void walk_overlap_region()
{
	hipStream_t st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	program(10, 2, 2, true);
	SpPic f(520, 70, 2, 2);
	PlPic fill(520, 70, 2, 2, 0, 16);
	const PlPic want6 = modelled(f, fill, 6), want0 = modelled(f, fill, 0);
	const std::vector<uint32_t> sb = seeds_of(3);
	vfgs_set_seed(3);
	sp_regs(f, 4, nullptr, 6);
	const Regs regs = sp_regs(f, 3, sb.data(), 0);
	SpPool a(f, 4), b(f, 3);
	PlPool da(fill, 4), db(fill, 3);
	vfgs_set_seed(3);
	OK(vfgs_hip_overlap_begin(st));
	OK(to_planar(a, da, nullptr, nullptr, 4, f, fill, 6, st));
	OK(to_planar(b, db, nullptr, sb.data(), 3, f, fill, 0, st));
	OK(vfgs_hip_overlap_end(st));
	CHECK(Regs() == regs);
	hipStreamSynchronize(st);
	CHECK(a.all_hold(f) && b.all_hold(f) && da.all_hold(want6) && db.all_hold(want0));
	hipStreamDestroy(st);
}

static void walk_refusals()
{
	program(10, 2, 2, false);
	SpPic f(520, 70, 2, 2, 0, 0);
	PlPic fill(520, 70, 2, 2, 16, 8);
	SpPool pool(f, 3);
	PlPool other(fill, 3);
	const std::vector<uint32_t> seeds = seeds_of(3);
	vfgs_hip_launch_info a, b;
	const unsigned h = f.h, s = f.stride, u = f.uv_stride, ds = fill.stride, du = fill.cstride;
	auto call = [&](const vfgs_hip_sp_frame* src, const vfgs_hip_frame_ptrs* dst, unsigned ww = 520, unsigned ss = 0, unsigned uu = 0, unsigned shift = 6, unsigned dss = 0, unsigned duu = 0) {
		const int rc = vfgs_hip_add_grain_sp_frame_list_to_planar_dev(src, dst, seeds.data(), 3, ww, h, ss ? ss : s, uu ? uu : u, dss ? dss : ds, duu ? duu : du, shift, nullptr);
		CHECK(rc == 0 || rc == vfgs_hip_last_error());     // (a served call leaves the last error alone)
		return rc;
	};
	auto L = pool.list;
	auto D = other.list;
	const Regs before;
	const bool had = vfgs_hip_last_launch_info(&a) == 0;
	// null lists and planes
	CHECK(call(nullptr, D.data()) == 18 && call(L.data(), nullptr) == 18);
	L[1].UV = nullptr;
	CHECK(call(L.data(), D.data()) == 18);
	L = pool.list; D[1].Y = nullptr;
	CHECK(call(L.data(), D.data()) == 18);
	D = other.list; D[2].V = nullptr;
	CHECK(call(L.data(), D.data()) == 18);
	// misaligned pointers, source and destination
	D = other.list; L[1].UV = (uint8_t*)L[1].UV + 8;
	CHECK(call(L.data(), D.data()) == 7);
	L = pool.list; D[2].U = (uint8_t*)D[2].U + 4;
	CHECK(call(L.data(), D.data()) == 7);
	D = other.list; D[2].V = (uint8_t*)D[2].V + 8;
	CHECK(call(L.data(), D.data()) == 7);
	D = other.list;
	// the source's geometry, with the semi-planar call's codes
	CHECK(call(L.data(), D.data(), 520, 512) == 6 && call(L.data(), D.data(), 520, 0, 512) == 6);
	CHECK(call(L.data(), D.data(), 520, s + 4) == 8 && call(L.data(), D.data(), 520, 0, u + 4) == 8);
	CHECK(call(L.data(), D.data(), 100) == 5);
	// the destination's pitches: ONE component's row is half as many samples as the luma row
	CHECK(call(L.data(), D.data(), 520, 0, 0, 6, 512) == 6 && call(L.data(), D.data(), 520, 0, 0, 6, 0, 256) == 6);
	CHECK(call(L.data(), D.data(), 520, 0, 0, 6, ds + 4) == 8 && call(L.data(), D.data(), 520, 0, 0, 6, 0, du + 4) == 8);
	// what the call alone refuses: error 40, the cause in the message
	CHECK(call(L.data(), D.data(), 520, 0, 0, 4) == 40 && strstr(vfgs_hip_last_error_string(), "sample_shift"));
	CHECK(call(L.data(), D.data(), 520, 0, 0, 16) == 40);
	CHECK(call(L.data(), D.data(), 8208, 8208, 8208, 6, 8208, 4104) == 40 && strstr(vfgs_hip_last_error_string(), "width 8208"));
	// destinations that share bytes; a destination that shares bytes with a source plane, of its own frame and of another: no in-place form
	D[2] = D[0];
	CHECK(call(L.data(), D.data()) == 18);
	D = other.list; D[1].V = D[1].U;
	CHECK(call(L.data(), D.data()) == 18);
	D = other.list; D[1].V = (uint8_t*)D[0].Y + 1024;
	CHECK(call(L.data(), D.data()) == 18);
	D = other.list; D[1].Y = L[1].Y;
	CHECK(call(L.data(), D.data()) == 18);                   // its own frame's source luma
	D = other.list; D[1].U = L[1].UV;
	CHECK(call(L.data(), D.data()) == 18);                   // its own frame's source UV
	D = other.list; D[0].V = (uint8_t*)L[2].UV + 4096;
	CHECK(call(L.data(), D.data()) == 18);                   // inside another frame's source UV
	D = other.list;
	// depth 8, another chroma format, the mix
	vfgs_set_depth(8);
	CHECK(call(L.data(), D.data()) == 40);
	vfgs_set_depth(10);
	vfgs_set_chroma_subsampling(1, 1);
	CHECK(call(L.data(), D.data()) == 40 && strstr(vfgs_hip_last_error_string(), "csubx"));
	vfgs_set_chroma_subsampling(2, 2);
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	CHECK(call(L.data(), D.data()) == 40 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
	{
		const vfgs_hip_model* none[3] = {nullptr, nullptr, nullptr};
		CHECK(vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev(L.data(), D.data(), none, seeds.data(), 3, 520, h, s, u, ds, du, 6, nullptr) == 41);
	}
	vfgs_hip_clear_chroma_mix();
	// an empty list is no call at all
	OK(vfgs_hip_add_grain_sp_frame_list_to_planar_dev(L.data(), D.data(), seeds.data(), 0, 520, h, s, u, ds, du, 6, nullptr));
	CHECK(Regs() == before);
	CHECK((vfgs_hip_last_launch_info(&b) == 0) == had && (!had || a.launches == b.launches));
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f) && other.all_hold(fill));
	// the destination's extents at its OWN pitches decide: one arena, the planes back to back at the smallest extents are served; a Cb plane
	// that begins one unit inside the luma plane is refused
	{
		const size_t yb = fill.P[0].size(), cb = fill.P[1].size();
		const size_t ya = (yb + 15) & ~(size_t)15, ca = (cb + 15) & ~(size_t)15;
		uint8_t* arena = nullptr;
		hipMalloc((void**)&arena, ya + ca + cb);
		PlPool extra(fill, 3);
		auto E = extra.list;
		E[1].Y = arena; E[1].U = arena + ya - 16; E[1].V = arena + ya + ca;
		CHECK(call(L.data(), E.data()) == 18);
		E[1].U = arena + ya;
		CHECK(call(L.data(), E.data()) == 0);
		hipDeviceSynchronize();
		hipFree(arena);
		program(10, 2, 2, false);
	}
	// the same lists are served afterwards
	const Regs want = sp_regs(f, 3, seeds.data(), 6);
	vfgs_set_seed(1);
	CHECK(call(L.data(), D.data()) == 0);
	CHECK(Regs() == want);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f) && other.all_hold(modelled(f, fill, 6)));
}

static void walk_two_threads()
{
	// two threads, pools and a stream each, calling at once: the library serialises them; with a seed per picture the registers a thread's
	// last call leaves do not show the order as long as both end on the same seed
	hipStream_t st[2] = {nullptr, nullptr};
	hipStreamCreateWithFlags(&st[0], 1);
	hipStreamCreateWithFlags(&st[1], 1);
	program(10, 2, 2, true);
	vfgs_hip_model* m = capture(st[0]);
	std::vector<const vfgs_hip_model*> models(6, m);
	SpPic f(520, 70, 2, 2);
	PlPic fill(520, 70, 2, 2, 16, 0), fill2(520, 70, 2, 2, 0, 8);
	const std::vector<uint32_t> seeds = seeds_of(6);
	const Regs want = sp_regs(f, 6, seeds.data(), 6);
	SpPool sa(f, 6), sb(f, 6);
	PlPool da(fill, 6), db(fill2, 6);
	int rc[2] = {0, 0};
	auto work = [&](int t) {
		for (int k = 0; k < 8 && !rc[t]; k++)
			rc[t] = t ? to_planar(sb, db, models.data(), seeds.data(), 6, f, fill2, 6, st[1]) : to_planar(sa, da, nullptr, seeds.data(), 6, f, fill, 6, st[0]);
	};
	std::thread ta(work, 0), tb(work, 1);
	ta.join(); tb.join();
	CHECK(rc[0] == 0 && rc[1] == 0);
	CHECK(Regs() == want);
	hipStreamSynchronize(st[0]);
	hipStreamSynchronize(st[1]);
	CHECK(sa.all_hold(f) && sb.all_hold(f) && da.all_hold(modelled(f, fill, 6)) && db.all_hold(modelled(f, fill2, 6)));
	vfgs_hip_model_release(m);
	hipStreamDestroy(st[0]);
	hipStreamDestroy(st[1]);
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"both_entry_points", walk_both_entry_points},
		{"thirty_five_frames", walk_thirty_five_frames},
		{"models_change_form", walk_models_change_form},
		{"overlap_region", walk_overlap_region},
		{"refusals", walk_refusals},
		{"two_threads", walk_two_threads},
	});
}
