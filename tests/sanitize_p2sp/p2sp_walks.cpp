// TEST INFRASTRUCTURE.  Planar frames in, semi-planar surfaces out (include/vfgs_hip.h: vfgs_hip_add_grain_frame_list_to_sp_dev and
// vfgs_hip_add_grain_frame_list_to_sp8_dev) in the host layer of libvfgs_hip, compiled with a sanitizer over the unchanged
// tests/sanitize/hip_stub.cpp, as tests/sanitize_sp_out8/sp_out8_walks.cpp drives the call beside it: both entry points with and without
// seeds, odd block counts, 35 frames (a second launch), an overlap region, every refusal -- a destination aliased with a source included --
// and two threads calling at once.  Every plane is allocated exactly as large as the contract says: (rows - 1) pitches and one row of whole
// blocks, a planar chroma row of 8 containers per block, a UV row of 16.
//
// What the model of the launch (hip_stub.cpp launch_grain, unchanged) proves here and what it does not.  It copies, per component, the
// rows of PlaneDesc::rowbytes bytes from FrameTable::src[c] to FrameTable::dst[c]:
//   * the narrowed form (out8): rows of PlaneDesc::drowbytes bytes at PlaneDesc::dpitch -- the destination's own pitch.  The source planes'
//     extents and pitches, the destination luma plane's extent and pitch and the pitch of the destination UV plane are all proven; of a UV row
//     the model writes ONE component's share (8 bytes per block, Cb's then Cr's over it), so the second half of the last UV row is not proven
//     to be inside the plane;
//   * the form in the depth's container: the model has no destination pitch of its own there -- it writes a destination row at the
//     SOURCE's pitch -- so these walks keep stride <= dst_stride and cstride <= dst_uv_stride (what the model writes then lies inside the
//     destination planes) and prove the extents and pitches of the three SOURCE planes only; the destination's extents at its own pitches
//     are not proven by the model.  They are what the host's own overlap rule works with, which the refusals walk exercises at the byte
//     (a destination plane that ends exactly where another begins is served, one byte further it is refused), and what the GPU suite
//     compares, padding included (tests/test_gpu_planar_to_sp.py).
// What the model leaves in the destinations is compared (`modelled` restates it), and everything else must keep its bytes.  The seed registers
// are compared with those of the planar copy lists on the same sources, through the same library.  Values are the GPU suite's business.
//
// usage: p2sp_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 4242
#include "../sanitize/walks.h"

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
	bool operator==(const Pic& o) const { return Y == o.Y && C[0] == o.C[0] && C[1] == o.C[1]; }
};

struct DevPic {
	uint8_t* p[3] = {nullptr, nullptr, nullptr};
	size_t n[3];
	explicit DevPic(const Pic& f) : n{f.Y.size(), f.C[0].size(), f.C[1].size()}
	{
		const std::vector<uint8_t>* v[3] = {&f.Y, &f.C[0], &f.C[1]};
		for (int i = 0; i < 3; i++)
			if (n[i]) { hipMalloc((void**)&p[i], n[i]); hipMemcpy(p[i], v[i]->data(), n[i], 1); }
	}
	~DevPic() { for (auto* q : p) if (q) hipFree(q); }
	DevPic(const DevPic&) = delete;
	bool holds(const Pic& f) const
	{
		const std::vector<uint8_t>* v[3] = {&f.Y, &f.C[0], &f.C[1]};
		for (int i = 0; i < 3; i++)
		{
			std::vector<uint8_t> got(n[i]);
			if (n[i]) hipMemcpy(got.data(), p[i], n[i], 2);
			if (got != *v[i]) return false;
		}
		return true;
	}
};

struct SrcPool {
	std::vector<std::unique_ptr<DevPic>> fr;
	std::vector<vfgs_hip_frame_ptrs> list;
	SrcPool(const Pic& f, int n)
	{
		for (int i = 0; i < n; i++) { fr.emplace_back(new DevPic(f)); list.push_back({fr.back()->p[0], fr.back()->p[1], fr.back()->p[2]}); }
	}
	bool all_hold(const Pic& f) const
	{
		for (const auto& d : fr) if (!d->holds(f)) return false;
		return true;
	}
};

struct DstPool {
	std::vector<std::unique_ptr<DevPic>> fr;
	std::vector<vfgs_hip_sp_frame> list;
	DstPool(const Pic& f, int n)
	{
		for (int i = 0; i < n; i++) { fr.emplace_back(new DevPic(f)); list.push_back({fr.back()->p[0], fr.back()->p[1]}); }
	}
	bool all_hold(const Pic& f) const
	{
		for (const auto& d : fr) if (!d->holds(f)) return false;
		return true;
	}
};

// what the model's launch leaves in a destination that held `fill` (see the head of this file): out8 -- at the destination's pitches, the
// luma row narrowed as it lies and Cr's narrowed row over the first half of the UV row; else -- at the SOURCE's pitches, the luma row and
// Cr's row as they lie
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

// the registers the contract names: those of the planar copy list (seeded or not) on the same sources, into planar destinations of their own
static Regs planar_regs(const Pic& f, int n, const uint32_t* seeds)
{
	SrcPool s(f, n), d(f, n);
	if (seeds) OK(vfgs_hip_add_grain_frame_list_seeded_copy_dev(s.list.data(), d.list.data(), seeds, n, f.w, f.h, f.stride, f.cstride, nullptr));
	else OK(vfgs_hip_add_grain_frame_list_copy_dev(s.list.data(), d.list.data(), n, f.w, f.h, f.stride, f.cstride, nullptr));
	hipDeviceSynchronize();
	return Regs();
}

static bool p2sp_launch(const vfgs_hip_launch_info& li, bool out8, int depth)
{
	const char* want = out8 ? "grain_p2sp8_kernel<" : "grain_p2sp_kernel<";
	return !strncmp(li.kernel, want, strlen(want)) && li.out8 == (out8 ? 1 : 0) && li.listed == 1 && li.in_place == 0 && li.persistent_luma_workgroups == 0 && li.depth == depth;
}

static int to_sp(bool out8, const SrcPool& s, const DstPool& d, const uint32_t* seeds, int n, const Pic& f, const Pic& fill, unsigned shift, void* st)
{
	if (out8) return vfgs_hip_add_grain_frame_list_to_sp8_dev(s.list.data(), d.list.data(), seeds, n, f.w, f.h, f.stride, f.cstride, fill.stride, fill.cstride, st);
	return vfgs_hip_add_grain_frame_list_to_sp_dev(s.list.data(), d.list.data(), seeds, n, f.w, f.h, f.stride, f.cstride, fill.stride, fill.cstride, shift, st);
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_both_entry_points()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	// depth, out8, width, height, csuby, one-pattern model, sample shift, source padding of Y / of a chroma row, destination padding of Y / UV
	// (containers; the destination's never below the source's where the model writes at the source's pitch): odd block counts (13, 17, 33,
	// 65), a single block row, the widest row, every depth
	const int cases[][11] = {{10, 0, 200, 150, 2, 1, 6, 0, 0, 0, 0},   {10, 0, 520, 70, 2, 0, 0, 16, 8, 32, 16},  {8, 0, 264, 40, 2, 0, 0, 16, 8, 16, 32},
	                         {12, 0, 1032, 33, 1, 0, 4, 8, 8, 16, 48}, {8, 0, 1042, 96, 1, 1, 0, 0, 0, 16, 0},    {10, 0, 8192, 17, 2, 0, 6, 0, 0, 0, 8},
	                         {10, 1, 200, 150, 2, 1, 0, 0, 0, 0, 0},   {10, 1, 520, 70, 2, 0, 0, 16, 8, 32, 16},  {10, 1, 1032, 33, 1, 0, 0, 8, 24, 16, 48},
	                         {10, 1, 8192, 17, 2, 0, 0, 0, 0, 16, 0},  {10, 1, 264, 40, 1, 1, 0, 24, 0, 0, 32}};
	for (const auto& c : cases)
	{
		const int depth = c[0], w = c[2], h = c[3], sy = c[4], n = 5;
		const bool out8 = c[1] != 0;
		const unsigned shift = (unsigned)c[6];
		program(depth, 2, sy, c[5] != 0);
		Pic f(true, w, h, sy, depth > 8 ? 2 : 1, c[7], c[8]), fill(false, w, h, sy, (depth > 8 && !out8) ? 2 : 1, c[9], c[10]);
		const Pic want = modelled(f, fill, out8);
		const std::vector<uint32_t> seeds = seeds_of(n);
		vfgs_set_seed(99);
		const Regs want_plain = planar_regs(f, n, nullptr);
		const Regs want_seeded = planar_regs(f, n, seeds.data());
		SrcPool src(f, n);
		vfgs_hip_launch_info a, b;
		{
			// one seed sequence
			DstPool dst(fill, n);
			vfgs_set_seed(99);
			CHECK(vfgs_hip_last_launch_info(&a) == 0);
			OK(to_sp(out8, src, dst, nullptr, n, f, fill, shift, st));
			CHECK(Regs() == want_plain);
			CHECK(vfgs_hip_last_launch_info(&b) == 0 && p2sp_launch(b, out8, depth) && b.nframes == n && b.launches - a.launches == 1);
			hipStreamSynchronize(st);
			CHECK(dst.all_hold(want) && src.all_hold(f));
		}
		{
			// a seed per picture
			DstPool dst(fill, n);
			vfgs_set_seed(7);
			OK(to_sp(out8, src, dst, seeds.data(), n, f, fill, shift, st));
			CHECK(Regs() == want_seeded);
			CHECK(vfgs_hip_last_launch_info(&b) == 0 && p2sp_launch(b, out8, depth));
			hipStreamSynchronize(st);
			CHECK(dst.all_hold(want) && src.all_hold(f));
		}
	}
	hipStreamDestroy(st);
}

static void walk_thirty_five_frames()
{
	for (int out8 = 0; out8 < 2; out8++)
	{
		program(10, 2, 2, true);
		Pic f(true, 264, 40, 2, 2), fill(false, 264, 40, 2, out8 ? 1 : 2, 16, 32);
		const Pic want = modelled(f, fill, out8 != 0);
		const std::vector<uint32_t> seeds = seeds_of(35);
		const Regs want_seeded = planar_regs(f, 35, seeds.data());
		SrcPool src(f, 35);
		DstPool dst(fill, 35);
		vfgs_hip_launch_info a, b;
		CHECK(vfgs_hip_last_launch_info(&a) == 0);
		OK(to_sp(out8 != 0, src, dst, seeds.data(), 35, f, fill, out8 ? 0 : 6, nullptr));
		CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 2 && b.nframes == 3 && p2sp_launch(b, out8 != 0, 10));
		CHECK(Regs() == want_seeded);
		vfgs_set_seed(5);
		const Regs want_plain = planar_regs(f, 35, nullptr);
		vfgs_set_seed(5);
		CHECK(vfgs_hip_last_launch_info(&a) == 0);
		OK(to_sp(out8 != 0, src, dst, nullptr, 35, f, fill, out8 ? 0 : 6, nullptr));
		CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 2 && b.nframes == 3);
		CHECK(Regs() == want_plain);
		hipDeviceSynchronize();
		CHECK(src.all_hold(f) && dst.all_hold(want));
	}
}

static void walk_overlap_region()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	program(10, 2, 2, true);
	Pic f(true, 520, 70, 2, 2), fill(false, 520, 70, 2, 2, 0, 16), fill8(false, 520, 70, 2, 1, 16, 0);
	const Pic want = modelled(f, fill, false), want8 = modelled(f, fill8, true);
	const std::vector<uint32_t> sb = seeds_of(3);
	vfgs_set_seed(3);
	planar_regs(f, 4, nullptr);
	planar_regs(f, 3, sb.data());
	const Regs regs = planar_regs(f, 3, sb.data());
	SrcPool a(f, 4), b(f, 3);
	DstPool da(fill, 4), db(fill8, 3), dc(fill, 3);
	vfgs_set_seed(3);
	OK(vfgs_hip_overlap_begin(st));
	OK(to_sp(false, a, da, nullptr, 4, f, fill, 6, st));
	OK(to_sp(true, b, db, sb.data(), 3, f, fill8, 0, st));
	OK(to_sp(false, b, dc, sb.data(), 3, f, fill, 0, st));
	OK(vfgs_hip_overlap_end(st));
	CHECK(Regs() == regs);
	hipStreamSynchronize(st);
	CHECK(a.all_hold(f) && b.all_hold(f) && da.all_hold(want) && db.all_hold(want8) && dc.all_hold(want));
	hipStreamDestroy(st);
}

static void walk_refusals()
{
	for (int out8 = 0; out8 < 2; out8++)
	{
		program(10, 2, 2, false);
		Pic f(true, 520, 70, 2, 2, 0, 0), fill(false, 520, 70, 2, out8 ? 1 : 2, 16, 32);
		SrcPool pool(f, 3);
		DstPool other(fill, 3);
		const std::vector<uint32_t> seeds = seeds_of(3);
		vfgs_hip_launch_info a, b;
		const unsigned h = f.h, s = f.stride, u = f.cstride, ds = fill.stride, du = fill.cstride;
		const unsigned good_shift = out8 ? 0 : 6;
		auto call = [&](const vfgs_hip_frame_ptrs* src, const vfgs_hip_sp_frame* dst, unsigned ww = 520, unsigned ss = 0, unsigned uu = 0, unsigned shift = 99, unsigned dss = 0,
		                unsigned duu = 0) {
			if (shift == 99) shift = good_shift;
			const int rc = out8 ? vfgs_hip_add_grain_frame_list_to_sp8_dev(src, dst, seeds.data(), 3, ww, h, ss ? ss : s, uu ? uu : u, dss ? dss : ds, duu ? duu : du, nullptr)
			                    : vfgs_hip_add_grain_frame_list_to_sp_dev(src, dst, seeds.data(), 3, ww, h, ss ? ss : s, uu ? uu : u, dss ? dss : ds, duu ? duu : du, shift, nullptr);
			CHECK(rc == 0 || rc == vfgs_hip_last_error());     // (a served call leaves the last error alone)
			return rc;
		};
		auto L = pool.list;
		auto D = other.list;
		// null lists and planes
		CHECK(call(nullptr, D.data()) == 18 && call(L.data(), nullptr) == 18);
		L[1].V = nullptr;
		CHECK(call(L.data(), D.data()) == 18);
		L = pool.list; D[1].Y = nullptr;
		CHECK(call(L.data(), D.data()) == 18);
		D = other.list; D[2].UV = nullptr;
		CHECK(call(L.data(), D.data()) == 18);
		// misaligned pointers, source and destination
		D = other.list; L[1].U = (uint8_t*)L[1].U + 8;
		CHECK(call(L.data(), D.data()) == 7);
		L = pool.list; D[2].Y = (uint8_t*)D[2].Y + 4;
		CHECK(call(L.data(), D.data()) == 7);
		D = other.list; D[2].UV = (uint8_t*)D[2].UV + 8;
		CHECK(call(L.data(), D.data()) == 7);
		D = other.list;
		// the source's geometry, with the planar list's codes
		CHECK(call(L.data(), D.data(), 520, 512) == 6 && call(L.data(), D.data(), 520, 0, 256) == 6);
		CHECK(call(L.data(), D.data(), 520, s + 4) == 8 && call(L.data(), D.data(), 520, 0, u + 4) == 8);
		CHECK(call(L.data(), D.data(), 100) == 5);
		// the destination's pitches: a UV row is as many containers as the luma row
		CHECK(call(L.data(), D.data(), 520, 0, 0, 99, 512) == 6 && call(L.data(), D.data(), 520, 0, 0, 99, 0, 512) == 6 && call(L.data(), D.data(), 520, 0, 0, 99, 0, 264) == 6);
		CHECK(call(L.data(), D.data(), 520, 0, 0, 99, ds + 4) == 8 && call(L.data(), D.data(), 520, 0, 0, 99, 0, du + 4) == 8);
		// what the call alone refuses: error 40, the cause in the message
		if (!out8)
		{
			CHECK(call(L.data(), D.data(), 520, 0, 0, 4) == 40 && strstr(vfgs_hip_last_error_string(), "sample_shift"));
			CHECK(call(L.data(), D.data(), 520, 0, 0, 16) == 40);
		}
		CHECK(call(L.data(), D.data(), 8208, 8208, 4104, 99, 8208, 8208) == 40 && strstr(vfgs_hip_last_error_string(), "width 8208"));
		// destinations that share bytes; a destination that shares bytes with a source plane, of its own frame and of another: no in-place form
		D[2] = D[0];
		CHECK(call(L.data(), D.data()) == 18);
		D = other.list; D[1].UV = (uint8_t*)D[0].Y + 1024;
		CHECK(call(L.data(), D.data()) == 18);
		D = other.list; D[1].Y = L[1].Y;
		CHECK(call(L.data(), D.data()) == 18);                   // its own frame's source luma
		D = other.list; D[1].UV = L[1].U;
		CHECK(call(L.data(), D.data()) == 18);                   // its own frame's source Cb
		D = other.list; D[1].UV = L[1].V;
		CHECK(call(L.data(), D.data()) == 18);                   // its own frame's source Cr
		D = other.list; D[0].UV = (uint8_t*)L[2].Y + 4096;
		CHECK(call(L.data(), D.data()) == 18);                   // inside another frame's source luma
		D = other.list; D[0].Y = (uint8_t*)L[2].V + 1024;
		CHECK(call(L.data(), D.data()) == 18);                   // inside another frame's source Cr
		D = other.list;
		// the destination's extents at its OWN pitches decide (the model of the launch does not prove them): one arena, the UV plane directly
		// behind the luma plane's last whole block is served -- below; one container earlier it is refused
		{
			const size_t ybytes = fill.Y.size(), cbytes = fill.C[0].size();
			CHECK(ybytes % 16 == 0);
			uint8_t* arena = nullptr;
			hipMalloc((void**)&arena, ybytes + cbytes);
			DstPool extra(fill, 3);
			auto E = extra.list;
			E[1].Y = arena; E[1].UV = arena + ybytes - 16;
			CHECK(call(L.data(), E.data()) == 18);
			E[1].UV = arena + ybytes;
			CHECK(call(L.data(), E.data()) == 0);
			hipDeviceSynchronize();
			hipFree(arena);
			program(10, 2, 2, false);
		}
		const Regs before;
		const bool had = vfgs_hip_last_launch_info(&a) == 0;
		// depth 8, another chroma format, the mix
		vfgs_set_depth(8);
		if (out8) CHECK(call(L.data(), D.data()) == 16);
		else CHECK(call(L.data(), D.data(), 520, 0, 0, 6) == 40);
		vfgs_set_depth(10);
		vfgs_set_chroma_subsampling(1, 1);
		CHECK(call(L.data(), D.data()) == 40 && strstr(vfgs_hip_last_error_string(), "csubx"));
		vfgs_set_chroma_subsampling(2, 2);
		OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
		CHECK(call(L.data(), D.data()) == 40 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
		vfgs_hip_clear_chroma_mix();
		// an empty list is no call at all
		if (out8) OK(vfgs_hip_add_grain_frame_list_to_sp8_dev(L.data(), D.data(), seeds.data(), 0, 520, h, s, u, ds, du, nullptr));
		else OK(vfgs_hip_add_grain_frame_list_to_sp_dev(L.data(), D.data(), seeds.data(), 0, 520, h, s, u, ds, du, 6, nullptr));
		CHECK(Regs() == before);
		CHECK((vfgs_hip_last_launch_info(&b) == 0) == had && (!had || a.launches == b.launches));
		hipDeviceSynchronize();
		CHECK(pool.all_hold(f) && other.all_hold(fill));
		// the same lists are served afterwards
		const Regs want = planar_regs(f, 3, seeds.data());
		vfgs_set_seed(1);
		CHECK(call(L.data(), D.data()) == 0);
		CHECK(Regs() == want);
		hipDeviceSynchronize();
		CHECK(pool.all_hold(f) && other.all_hold(modelled(f, fill, out8 != 0)));
	}
}

static void walk_two_threads()
{
	// two threads, pools and a stream each, calling at once: the library serialises them; with a seed per picture the registers a thread's
	// last call leaves do not show the order as long as both end on the same seed
	program(10, 2, 2, true);
	Pic f(true, 520, 70, 2, 2), fill(false, 520, 70, 2, 2, 16, 0), fill8(false, 520, 70, 2, 1, 0, 16);
	const std::vector<uint32_t> seeds = seeds_of(6);
	const Regs want = planar_regs(f, 6, seeds.data());
	SrcPool sa(f, 6), sb(f, 6);
	DstPool da(fill, 6), db(fill8, 6);
	void* st[2] = {nullptr, nullptr};
	hipStreamCreateWithFlags(&st[0], 1);
	hipStreamCreateWithFlags(&st[1], 1);
	int rc[2] = {0, 0};
	auto work = [&](int t) {
		for (int k = 0; k < 8 && !rc[t]; k++)
			rc[t] = t ? to_sp(true, sb, db, seeds.data(), 6, f, fill8, 0, st[1]) : to_sp(false, sa, da, seeds.data(), 6, f, fill, 6, st[0]);
	};
	std::thread ta(work, 0), tb(work, 1);
	ta.join(); tb.join();
	CHECK(rc[0] == 0 && rc[1] == 0);
	CHECK(Regs() == want);
	hipStreamSynchronize(st[0]);
	hipStreamSynchronize(st[1]);
	CHECK(sa.all_hold(f) && sb.all_hold(f) && da.all_hold(modelled(f, fill, false)) && db.all_hold(modelled(f, fill8, true)));
	hipStreamDestroy(st[0]);
	hipStreamDestroy(st[1]);
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"both_entry_points", walk_both_entry_points},
		{"thirty_five_frames", walk_thirty_five_frames},
		{"overlap_region", walk_overlap_region},
		{"refusals", walk_refusals},
		{"two_threads", walk_two_threads},
	});
}
