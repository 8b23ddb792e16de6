// TEST INFRASTRUCTURE.  The prelude of every stand-alone walk program that drives the host layer of libvfgs_hip over tests/sanitize/hip_stub.cpp
// (tests/sanitize*/*.cpp, built by tests/sanitize_build.py): the declarations of the runtime model, CHECK / OK and the failure counter, the LCG,
// program() for a model, the seed registers, one planar and one semi-planar picture with their device copies and pools, the registers of the
// planar list calls on frames of the same size, the helpers around models that several programs share, and run_walks(), the main() of a program.
// What is particular to one program -- its expectation of what a launch leaves, its kernel-name predicates, its stand-in launchers -- stays there.
//
// A program sets its LCG seed and includes this file:
//     #define WALKS_SEED 34
//     #include "../sanitize/walks.h"
// then defines its walk_*() functions and ends with
//     int main(int argc, char** argv) { return run_walks(argc, argv, {{"entries", walk_entries}, ...}); }
// A program that brings the runtime's own header (<hip/hip_runtime.h>, for a stand-in launcher) includes it first and defines
// WALKS_HAVE_HIP_RUNTIME_H, so that the model's functions are not declared a second time.
#pragma once
#ifndef WALKS_SEED
#error "define WALKS_SEED, the program's LCG seed, before including walks.h"
#endif

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vfgs_hip.h"
#include "../../include/vfgs_hip_fw.h"

extern "C" void vfgs_stub_stats(uint64_t out[3]);
extern "C" void vfgs_stub_fail_pinned_allocs(int n);
#ifndef WALKS_HAVE_HIP_RUNTIME_H
extern "C" int hipMalloc(void** p, size_t n);
extern "C" int hipFree(void* p);
extern "C" int hipMemcpy(void* d, const void* s, size_t n, int kind);
extern "C" int hipStreamCreateWithFlags(void** s, unsigned flags);
extern "C" int hipStreamDestroy(void* s);
extern "C" int hipStreamSynchronize(void* s);
extern "C" int hipDeviceSynchronize(void);
enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
#endif

static std::atomic<int> g_fail{0};      // (walks call from several threads)
#define CHECK(c)                                                                     \
	do {                                                                             \
		if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
	} while (0)
#define OK(call)                                                                                                    \
	do {                                                                                                            \
		const int rc_ = (call);                                                                                     \
		if (rc_) { fprintf(stderr, "FAILED %s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, vfgs_hip_last_error_string()); g_fail++; } \
	} while (0)

static uint32_t g_lcg = WALKS_SEED;
static uint32_t lcg_step(uint32_t x) { return x * 1664525u + 1013904223u; }      // (a thread of a walk keeps a state of its own)
static uint32_t rnd() { g_lcg = lcg_step(g_lcg); return g_lcg >> 8; }
static uint32_t rnd32() { return rnd() << 8 ^ rnd(); }

// a seed per picture; the two registers that step oddly lead every list long enough to hold them
static std::vector<uint32_t> seeds_of(int n)
{
	std::vector<uint32_t> s(n);
	for (auto& v : s) v = rnd32();
	if (n > 2) { s[0] = 0; s[1] = 0x80000000u; }
	return s;
}

// ---- the programmed model ---------------------------------------------------------------------------------------------------

// eight random patterns for luma and chroma alike, then per component a random scale LUT and a pattern LUT that names one slot (one_*) or
// eight; mix: a luma / chroma mix for Cb (bit 0) and Cr (bit 1).  (callers hold no lock: a walk with several threads programs before it starts them)
struct Model {
	int depth, sx, sy;
	bool one_luma, one_chroma;
	int shift = 5, legal = 0, mix = 0;
	unsigned seed = 4711;
};

static void program(const Model& m)
{
	vfgs_hip_reset_state();
	vfgs_set_depth(m.depth);
	vfgs_set_chroma_subsampling(m.sx, m.sy);
	signed char P[4096];
	for (int k = 0; k < 8; k++)
	{
		for (int i = 0; i < 4096; i++) P[i] = (signed char)((int)(rnd() % 255) - 127);
		vfgs_set_luma_pattern(k, P);
		vfgs_set_chroma_pattern(k, P);
	}
	unsigned char lut[256];
	for (int c = 0; c < 3; c++)
	{
		for (int i = 0; i < 256; i++) lut[i] = (unsigned char)(rnd() % 200);
		vfgs_set_scale_lut(c, lut);
		const bool one = c == 0 ? m.one_luma : m.one_chroma;
		for (int i = 0; i < 256; i++) lut[i] = (unsigned char)(one ? 0x10 : ((i >> 5) << 4));
		vfgs_set_pattern_lut(c, lut);
	}
	vfgs_set_scale_shift(m.shift);
	vfgs_set_legal_range(m.legal);
	vfgs_set_seed(m.seed);
	if (m.mix & 1) OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	if (m.mix & 2) OK(vfgs_hip_set_chroma_mix(2, 64, 101, -202));
}

// the usual call: one form for every component
static void program(int depth, int sx, int sy, bool one_pattern, int shift = 5, int legal = 0)
{
	program(Model{depth, sx, sy, one_pattern, one_pattern, shift, legal});
}

struct Regs {
	uint32_t r[4];
	Regs() { vfgs_hip_get_seed_state(r); }
	bool operator==(const Regs& o) const { return !memcmp(r, o.r, sizeof r); }
};

static unsigned long long launches()
{
	vfgs_hip_launch_info li;
	return vfgs_hip_last_launch_info(&li) == 0 ? li.launches : 0;
}

// ---- pictures -----------------------------------------------------------------------------------------------------------------

static void to_device(void* d, const void* s, size_t n) { (void)hipMemcpy(d, s, n, hipMemcpyHostToDevice); }
static void to_host(void* d, const void* s, size_t n) { (void)hipMemcpy(d, s, n, hipMemcpyDeviceToHost); }

// one planar picture in ordinary host memory, the reference's geometry (yuv.c:54-87) unless a row pitch is given: one allocation per plane,
// so that a byte written past a plane's end is a heap overflow and not a neighbour's sample
struct Frame {
	int w, h, depth, sx, sy, stride, cstride, cw, ch, sz;
	std::vector<uint8_t> Y, U, V;
	Frame(int w_, int h_, int depth_, int sx_, int sy_, int stride_ = 0) : w(w_), h(h_), depth(depth_), sx(sx_), sy(sy_)
	{
		sz = depth > 8 ? 2 : 1;
		stride = stride_ ? stride_ : ((w % 64) ? (w + 64) & ~63 : w);
		cstride = stride / sx;
		cw = w / sx; ch = (h + sy - 1) / sy;
		Y.resize((size_t)stride * h * sz); U.resize((size_t)cstride * ch * sz); V.resize((size_t)cstride * ch * sz);
		fill();
	}
	void fill()
	{
		for (auto* p : {&Y, &U, &V})
			for (size_t i = 0; i < p->size(); i += sz)
			{
				const uint32_t v = rnd() & ((1u << depth) - 1);
				(*p)[i] = (uint8_t)v;
				if (sz == 2) (*p)[i + 1] = (uint8_t)(v >> 8);
			}
	}
	uint8_t* y(int line) { return Y.data() + (size_t)line * stride * sz; }
	uint8_t* u(int line) { return U.data() + (size_t)(line / sy) * cstride * sz; }
	uint8_t* v(int line) { return V.data() + (size_t)(line / sy) * cstride * sz; }
	bool same(const Frame& o) const { return Y == o.Y && U == o.U && V == o.V; }
};

// nframes copies of a Frame at a frame pitch of ny / nc bytes, or bare planes of ny and nc bytes: exactly as large as the planes, a byte too
// many is a heap overflow
struct DevFrame {
	uint8_t *Y = nullptr, *U = nullptr, *V = nullptr;
	size_t ny, nc;
	explicit DevFrame(const Frame& f, int nframes = 1) : DevFrame(f.Y.size() * nframes, f.U.size() * nframes)
	{
		ny = f.Y.size(); nc = f.U.size();
		for (int i = 0; i < nframes; i++) { to_device(Y + i * ny, f.Y.data(), ny); to_device(U + i * nc, f.U.data(), nc); to_device(V + i * nc, f.V.data(), nc); }
	}
	DevFrame(size_t ny_, size_t nc_) : ny(ny_), nc(nc_) { hipMalloc((void**)&Y, ny); hipMalloc((void**)&U, nc); hipMalloc((void**)&V, nc); }
	~DevFrame() { hipFree(Y); hipFree(U); hipFree(V); }
	DevFrame(const DevFrame&) = delete;
	vfgs_hip_frame_ptrs ptrs() const { return {Y, U, V}; }
	bool holds(const Frame& f, int i = 0) const
	{
		std::vector<uint8_t> y(ny), u(nc), v(nc);
		to_host(y.data(), Y + i * ny, ny); to_host(u.data(), U + i * nc, nc); to_host(v.data(), V + i * nc, nc);
		return y == f.Y && u == f.U && v == f.V;
	}
};

// a semi-planar picture of sz-byte containers, its planes exactly as large as the contract says: (rows - 1) pitches and one row of whole
// blocks; pad / uv_pad: containers a row pitch exceeds the whole blocks by
struct SpPic {
	int w, h, sy, sz, nblk, stride, uv_stride, crows;
	std::vector<uint8_t> Y, UV;
	SpPic(int w_, int h_, int sy_, int sz_, int pad = 0, int uv_pad = 0) : w(w_), h(h_), sy(sy_), sz(sz_)
	{
		nblk = (w + 15) / 16;
		stride = nblk * 16 + pad;
		uv_stride = nblk * 16 + uv_pad;
		crows = (h + sy - 1) / sy;
		Y.resize(((size_t)(h - 1) * stride + nblk * 16) * sz);
		UV.resize(((size_t)(crows - 1) * uv_stride + nblk * 16) * sz);
		for (auto* p : {&Y, &UV})
			for (auto& b : *p) b = (uint8_t)rnd();
	}
};

struct DevSpPic {
	uint8_t *Y = nullptr, *UV = nullptr;
	size_t ny, nc;
	explicit DevSpPic(const SpPic& f) : ny(f.Y.size()), nc(f.UV.size())
	{
		hipMalloc((void**)&Y, ny); hipMalloc((void**)&UV, nc);
		to_device(Y, f.Y.data(), ny); to_device(UV, f.UV.data(), nc);
	}
	~DevSpPic() { hipFree(Y); hipFree(UV); }
	DevSpPic(const DevSpPic&) = delete;
	vfgs_hip_sp_frame ptrs() const { return {Y, UV}; }
	bool holds(const SpPic& f) const
	{
		std::vector<uint8_t> y(ny), c(nc);
		to_host(y.data(), Y, ny); to_host(c.data(), UV, nc);
		return y == f.Y && c == f.UV;
	}
};

// n device copies of one picture and the list a call takes
template <class Host, class Dev, class Ptrs>
struct PoolOf {
	std::vector<std::unique_ptr<Dev>> fr;
	std::vector<Ptrs> list;
	PoolOf(const Host& f, int n)
	{
		for (int i = 0; i < n; i++) { fr.emplace_back(new Dev(f)); list.push_back(fr.back()->ptrs()); }
	}
	bool all_hold(const Host& f) const
	{
		for (const auto& d : fr) if (!d->holds(f)) return false;
		return true;
	}
};
using FramePool = PoolOf<Frame, DevFrame, vfgs_hip_frame_ptrs>;
using SpPool = PoolOf<SpPic, DevSpPic, vfgs_hip_sp_frame>;

// n frames of device planes without a host copy, the reference's geometry (a UV plane as wide as luma's), planar and semi-planar lists
struct BarePlanes {
	int w, h, stride, cstride, ch;
	std::vector<uint8_t*> dev;
	std::vector<vfgs_hip_frame_ptrs> list;
	std::vector<vfgs_hip_sp_frame> sp_list;
	BarePlanes(int n, int w_, int h_, int depth, int sx, int sy, bool semiplanar) : w(w_), h(h_)
	{
		const int sz = depth > 8 ? 2 : 1;
		stride = (w % 64) ? (w + 64) & ~63 : w;
		cstride = semiplanar ? stride : stride / sx;
		ch = (h + sy - 1) / sy;
		for (int i = 0; i < n; i++)
		{
			uint8_t *Y = nullptr, *U = nullptr, *V = nullptr;
			hipMalloc((void**)&Y, (size_t)stride * h * sz);
			hipMalloc((void**)&U, (size_t)cstride * ch * sz);
			dev.push_back(Y); dev.push_back(U);
			if (semiplanar) { sp_list.push_back({Y, U}); continue; }
			hipMalloc((void**)&V, (size_t)cstride * ch * sz);
			dev.push_back(V);
			list.push_back({Y, U, V});
		}
	}
	~BarePlanes() { for (uint8_t* p : dev) hipFree(p); }
	BarePlanes(const BarePlanes&) = delete;
};

// ---- the registers the contract names -------------------------------------------------------------------------------------------

// the seed registers a planar list call (seeded or not) leaves on n planar pictures of w x h in sz-byte containers, rows of whole blocks
// (a planar chroma row pitch of whole 16-byte units at any block count): in place, into destinations of their own, or into 8-bit ones
enum PlanarEntry { PLANAR_LIST, PLANAR_LIST_COPY, PLANAR_LIST_COPY8 };

static Regs planar_regs(int w, int h, int crows, int sz, int n, const uint32_t* seeds, PlanarEntry e = PLANAR_LIST)
{
	const unsigned row = (unsigned)((w + 15) / 16 * 16);
	std::vector<uint8_t*> mem;
	std::vector<vfgs_hip_frame_ptrs> s, d;
	for (int i = 0; i < (e == PLANAR_LIST ? n : 2 * n); i++)
	{
		const size_t c = i < n ? sz : (e == PLANAR_LIST_COPY8 ? 1 : sz);      // the container of a source, of a destination
		uint8_t* p[3];
		for (int k = 0; k < 3; k++)
		{
			const size_t bytes = (size_t)(k ? crows : h) * row * c;
			hipMalloc((void**)&p[k], bytes);
			memset(p[k], 0x55, bytes);
		}
		mem.insert(mem.end(), p, p + 3);
		(i < n ? s : d).push_back({p[0], p[1], p[2]});
	}
	switch (e)
	{
	case PLANAR_LIST:
		if (seeds) OK(vfgs_hip_add_grain_frame_list_seeded_dev(s.data(), seeds, n, w, h, row, row, nullptr));
		else OK(vfgs_hip_add_grain_frame_list_dev(s.data(), n, w, h, row, row, nullptr));
		break;
	case PLANAR_LIST_COPY:
		if (seeds) OK(vfgs_hip_add_grain_frame_list_seeded_copy_dev(s.data(), d.data(), seeds, n, w, h, row, row, nullptr));
		else OK(vfgs_hip_add_grain_frame_list_copy_dev(s.data(), d.data(), n, w, h, row, row, nullptr));
		break;
	case PLANAR_LIST_COPY8:
		if (seeds) OK(vfgs_hip_add_grain_frame_list_seeded_copy8_dev(s.data(), d.data(), seeds, n, w, h, row, row, row, row, nullptr));
		else OK(vfgs_hip_add_grain_frame_list_copy8_dev(s.data(), d.data(), n, w, h, row, row, row, row, nullptr));
		break;
	}
	hipDeviceSynchronize();
	for (auto* p : mem) hipFree(p);
	return Regs();
}

static Regs planar_regs(const SpPic& f, int n, const uint32_t* seeds, PlanarEntry e = PLANAR_LIST)
{
	return planar_regs(f.w, f.h, f.crows, f.sz, n, seeds, e);
}

// ---- models -------------------------------------------------------------------------------------------------------------------

static void set_format(int depth, int sx, int sy, int legal = 0)
{
	vfgs_hip_reset_state();
	vfgs_set_depth(depth);
	vfgs_set_chroma_subsampling(sx, sy);
	vfgs_set_legal_range(legal);
}

static vfgs_hip_model* capture(void* stream)
{
	vfgs_hip_model* m = nullptr;
	OK(vfgs_hip_model_capture(&m, stream));
	CHECK(m != nullptr);
	return m;
}

// what the stub's kernel does not read: the model's device bytes, all of them (the device pointer is the handle's first member)
static void touch_model(const vfgs_hip_model* m)
{
	int info[8];
	OK(vfgs_hip_model_info(m, info));
	const uint8_t* dev;
	memcpy(&dev, m, sizeof dev);
	std::vector<uint8_t> b((size_t)info[7]);
	to_host(b.data(), dev, b.size());
	unsigned x = 0;
	for (uint8_t v : b) x += v;
	CHECK(info[7] > 4096 && x != 0);
}

// every byte of a built model through the public read-back, into a buffer of exactly its size; lo: the marker of the stand-in that wrote it
static void touch_image(const vfgs_hip_model* m, int lo = 0x40)
{
	int info[8];
	OK(vfgs_hip_model_info(m, info));
	std::vector<uint8_t> b((size_t)info[7]);
	size_t bytes = 0;
	OK(vfgs_hip_model_image(m, b.data(), b.size(), &bytes));
	CHECK(bytes == b.size() && bytes > 4096);
	int32_t pk = 0;
	memcpy(&pk, b.data() + 16, 4);
	CHECK(pk == info[5] && b[32] >= lo && b[32] < lo + 0x20 && b[bytes - 1] == b[32]);      // the record's shift; the stand-in's marker from end to end
}

struct Stats {
	uint64_t v[8];
	Stats() { vfgs_hip_get_model_build_stats(v); }
	bool operator==(const Stats& o) const { return !memcmp(v, o.v, sizeof v); }
};

// ---- main() -------------------------------------------------------------------------------------------------------------------

struct Walk {
	const char* name;
	void (*fn)();
};

// the walks named on the command line (none: all of them), a line " ok " / "FAILED" for each -- tests/sanitize_build.py counts them -- with
// whatever the program appends to it; the exit status says whether any CHECK failed
static int run_walks(int argc, char** argv, std::initializer_list<Walk> walks, std::string (*more)() = nullptr)
{
	for (const auto& w : walks)
	{
		bool want = argc < 2;
		for (int i = 1; i < argc; i++) want = want || !strcmp(argv[i], w.name);
		if (!want) continue;
		const int before = g_fail;
		w.fn();
		printf("%-28s %s%s\n", w.name, g_fail == before ? " ok " : "FAILED", more ? more().c_str() : "");
		fflush(stdout);
	}
	vfgs_hip_shutdown();
	return g_fail ? 1 : 0;
}
