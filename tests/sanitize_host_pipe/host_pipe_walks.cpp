// TEST INFRASTRUCTURE.  Pictures in host memory as a stream (include/vfgs_hip.h: vfgs_hip_host_pipe_open / _submit / _wait / _close) in the
// host layer of libvfgs_hip, compiled with a sanitizer over the unchanged tests/sanitize/hip_stub.cpp: a steady stream with a model and a
// seed per picture through reused slots, a submitting and a waiting thread on one pipe, refusals in mid-stream, close with pictures in
// flight, vfgs_hip_shutdown with an open pipe and the stale handle behind it.  Host planes are allocated exactly as large as the contract
// says -- (rows - 1) pitches and one row of whole blocks, pinned or pageable -- so a wrong extent, pitch or slot is a sanitizer report.
//
// What the stub proves here: its "kernel" moves every source row to the destination row the launch names (a grain of zero; narrowed,
// (v + 2) >> 2, with the 8-bit destination, which it serves at depth 10), and its copies run only when something waits for them.  So a
// destination holds the source's whole blocks (narrowed) and its fill everywhere else exactly when upload, launch and download of that
// picture went through the right slot at the right pitches, and not before its ticket was waited for.  Values are the GPU suite's business
// (tests/test_gpu_host_pipe.py); the seed registers are compared with those of the planar list calls on device frames of the same size.
//
// What the model cannot show by itself: its event wait never sleeps -- it runs what the event depends on, on the calling thread -- so a
// vfgs_hip_host_pipe_wait that kept the library's lock while "asleep" would go unnoticed.  This program is therefore linked with
// -Wl,--wrap=hipEventSynchronize (tests/test_sanitize_host_pipe_cpu.py): the host layer's event waits pass through the wrapper below, which
// for a thread that has set a gate sleeps until ANOTHER thread's submit has returned, and only then lets the model's wait run.  A wait that
// holds the lock across that sleep keeps the submit out: the gate gives up after twenty seconds and the walk fails.
//
// usage: host_pipe_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 61
#include <chrono>

#include "../sanitize/walks.h"

struct Gate {
	const std::atomic<uint64_t>* issued;      // tickets another thread's submits have returned
	uint64_t need;                            // the sleeper wakes when that many are out
	std::atomic<uint64_t>* asleep;            // told the ticket the sleeper sleeps on: the other thread submits only then
	uint64_t ticket;
};
static thread_local const Gate* t_gate = nullptr;
static std::atomic<bool> g_gate_gave_up{false};

extern "C" int __real_hipEventSynchronize(void* event);
extern "C" int __wrap_hipEventSynchronize(void* event)
{
	if (const Gate* g = t_gate)
	{
		const auto t0 = std::chrono::steady_clock::now();
		g->asleep->store(g->ticket);
		while (g->issued->load() < g->need && !g_gate_gave_up)
		{
			if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20))
			{
				fprintf(stderr, "FAILED: no submit returned while another thread slept in vfgs_hip_host_pipe_wait: the wait holds the library's lock\n");
				g_fail++;
				g_gate_gave_up = true;
			}
			std::this_thread::sleep_for(std::chrono::microseconds(50));
		}
	}
	return __real_hipEventSynchronize(event);
}

static const uint8_t kFill = 0xa5;

// one picture's three planes in host memory, pinned (vfgs_hip_host_alloc) or pageable: `str` / `cstr` containers a row, `sz` bytes each
struct HostPic {
	bool pinned;
	uint8_t* p[3] = {nullptr, nullptr, nullptr};
	size_t n[3] = {0, 0, 0};
	HostPic(bool pinned_, int h, int crows, size_t str, size_t cstr, size_t yrow, size_t crow, int sz) : pinned(pinned_)
	{
		n[0] = ((size_t)(h - 1) * str + yrow) * sz;
		n[1] = n[2] = ((size_t)(crows - 1) * cstr + crow) * sz;
		for (int c = 0; c < 3; c++)
		{
			p[c] = pinned ? (uint8_t*)vfgs_hip_host_alloc(n[c]) : (uint8_t*)malloc(n[c]);
			CHECK(p[c] != nullptr);
		}
	}
	~HostPic() { for (auto* q : p) { if (pinned) vfgs_hip_host_free(q); else free(q); } }
	HostPic(const HostPic&) = delete;
	vfgs_hip_frame_ptrs ptrs() const { return {p[0], p[1], p[2]}; }
	void fill(uint8_t v) { for (int c = 0; c < 3; c++) memset(p[c], v, n[c]); }
	void random(int depth)
	{
		for (int c = 0; c < 3; c++)
			for (size_t i = 0; i < n[c]; i += depth > 8 ? 2 : 1)
			{
				const uint32_t v = rnd() & ((1u << depth) - 1);
				p[c][i] = (uint8_t)v;
				if (depth > 8) p[c][i + 1] = (uint8_t)(v >> 8);
			}
	}
	std::vector<uint8_t> bytes() const
	{
		std::vector<uint8_t> b;
		for (int c = 0; c < 3; c++) b.insert(b.end(), p[c], p[c] + n[c]);
		return b;
	}
};

// the geometry of a pipe: sources of `depth`-bit samples, destinations of the same samples or (dst8) of bytes
struct Geo {
	int w, h, depth, sx, sy, sz, dsz, nblk, crows;
	unsigned stride, cstride, dstride, dcstride;
	size_t yrow, crow;
	bool dst, dst8;
	Geo(int w_, int h_, int depth_, int sx_, int sy_, int pad, int dpad, bool dst_, bool dst8_) : w(w_), h(h_), depth(depth_), sx(sx_), sy(sy_), dst(dst_), dst8(dst8_)
	{
		sz = depth > 8 ? 2 : 1; dsz = dst8 ? 1 : sz;
		nblk = (w + 15) / 16; crows = (h + sy - 1) / sy;
		yrow = (size_t)nblk * 16; crow = yrow / sx;
		stride = (unsigned)yrow + pad; cstride = ((unsigned)crow + pad + 15) & ~15u;
		dstride = dst ? (unsigned)yrow + dpad : 0; dcstride = dst ? ((unsigned)crow + 2 * dpad + 15) & ~15u : 0;
	}
	vfgs_hip_host_pipe_desc desc(unsigned slots) const { return {(unsigned)w, (unsigned)h, stride, cstride, dstride, dcstride, dst8 ? 1 : 0, slots}; }
	std::unique_ptr<HostPic> source(bool pinned) const
	{
		std::unique_ptr<HostPic> s(new HostPic(pinned, h, crows, stride, cstride, yrow, crow, sz));
		s->random(depth);
		return s;
	}
	std::unique_ptr<HostPic> destination(bool pinned) const
	{
		std::unique_ptr<HostPic> d(new HostPic(pinned, h, crows, dstride, dcstride, yrow, crow, dsz));
		d->fill(kFill);
		return d;
	}
	// what the stub leaves in a destination of source `s`: the whole blocks of every row (narrowed), the fill everywhere else
	std::vector<uint8_t> expected(const HostPic& s) const
	{
		std::vector<uint8_t> out;
		for (int c = 0; c < 3; c++)
		{
			const size_t rows = c ? crows : h, row = c ? crow : yrow, sp = c ? cstride : stride, dp = c ? dcstride : dstride;
			std::vector<uint8_t> d(((rows - 1) * dp + row) * dsz, kFill);
			for (size_t r = 0; r < rows; r++)
				for (size_t i = 0; i < row; i++)
				{
					if (!dst8) { memcpy(&d[(r * dp + i) * sz], s.p[c] + (r * sp + i) * sz, sz); continue; }
					uint16_t v;
					memcpy(&v, s.p[c] + (r * sp + i) * 2, 2);
					d[r * dp + i] = (uint8_t)((v + 2) >> 2);
				}
			out.insert(out.end(), d.begin(), d.end());
		}
		return out;
	}
};

static vfgs_hip_host_pipe* open_pipe(const Geo& g, unsigned slots)
{
	const vfgs_hip_host_pipe_desc d = g.desc(slots);
	vfgs_hip_host_pipe* p = nullptr;
	OK(vfgs_hip_host_pipe_open(&d, &p));
	CHECK(p != nullptr);
	return p;
}

// the registers one picture of the geometry leaves behind the registers of now, through the planar list calls on device frames
static Regs regs_after(const Geo& g, const uint32_t* seed) { return planar_regs(g.w, g.h, g.crows, g.sz, 1, seed); }

static bool recorded(const Geo& g, bool model, int oney, int onec)
{
	vfgs_hip_launch_info li;
	if (vfgs_hip_last_launch_info(&li)) return false;
	char want[96];
	if (model && !g.dst8) snprintf(want, sizeof want, "grain_ml_kernel<%d,%d,%d,%s,%s>", g.depth, g.sx, g.sy, oney ? "true" : "false", onec ? "true" : "false");
	else snprintf(want, sizeof want, "stub<%d,%d,%d,%d,%d,%d,0,0>", g.depth, g.sx, g.sy, g.dst8 ? 1 : 0, oney, onec);
	if (strcmp(li.kernel, want)) fprintf(stderr, "kernel %s, expected %s\n", li.kernel, want);
	return !strcmp(li.kernel, want) && li.internal == 1 && li.listed == 1 && li.nframes == 1 && li.out8 == (g.dst8 ? 1 : 0) && li.in_place == (g.dst ? 0 : 1);
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

// eight pictures through three slots (two of them through two), models alternating between a general-form and a one-pattern one, a seed per
// picture; then the programmed state and the running seed sequence; pinned and pageable memory; in place, a destination, an 8-bit one
static void walk_steady_stream()
{
	// width, height, depth, csubx, csuby, source padding, destination padding, destination, dst8
	const int cases[][9] = {{200, 40, 10, 2, 2, 8, 16, 1, 1}, {264, 33, 8, 1, 1, 0, 0, 1, 0}, {136, 48, 10, 1, 2, 16, 32, 1, 0},
	                        {200, 40, 10, 2, 2, 8, 0, 0, 0}, {1000, 17, 12, 1, 2, 0, 16, 1, 0}};
	for (const auto& c : cases)
		for (int pinned = 0; pinned < 2; pinned++)
		{
			const Geo g(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7] != 0, c[8] != 0);
			const int n = 8;
			program(g.depth, g.sx, g.sy, false);
			vfgs_hip_model* gen = capture(nullptr);
			program(g.depth, g.sx, g.sy, true, 4, 1);
			vfgs_hip_model* one = capture(nullptr);
			const std::vector<uint32_t> seeds = seeds_of(n);
			std::vector<Regs> want;
			for (int i = 0; i < n; i++) want.push_back(regs_after(g, &seeds[i]));
			vfgs_set_seed(77);
			std::vector<Regs> want_plain;
			for (int i = 0; i < n; i++) want_plain.push_back(regs_after(g, nullptr));
			std::vector<std::unique_ptr<HostPic>> src, dst, before;
			for (int i = 0; i < 2 * n; i++)
			{
				src.push_back(g.source(pinned != 0));
				if (g.dst) dst.push_back(g.destination(pinned != 0));
			}
			std::vector<std::vector<uint8_t>> orig;
			for (auto& s : src) orig.push_back(s->bytes());
			vfgs_hip_host_pipe* p = open_pipe(g, pinned ? 0 : 2);
			int params[8], params2[8];
			vfgs_hip_get_params(params);
			std::vector<uint64_t> tickets(2 * n);
			for (int i = 0; i < n; i++)
			{
				const vfgs_hip_frame_ptrs s = src[i]->ptrs(), d = g.dst ? dst[i]->ptrs() : s;
				OK(vfgs_hip_host_pipe_submit(p, &s, g.dst ? &d : nullptr, i & 1 ? one : gen, &seeds[i], &tickets[i]));
				CHECK(tickets[i] == (uint64_t)i + 1 && Regs() == want[i] && recorded(g, true, i & 1, i & 1));
			}
			vfgs_hip_model_release(gen);      // with pictures of both models in flight
			vfgs_hip_model_release(one);
			// the programmed state (one-pattern, programmed last) and the running seed sequence, behind them in the same ring
			vfgs_set_seed(77);
			for (int i = n; i < 2 * n; i++)
			{
				const vfgs_hip_frame_ptrs s = src[i]->ptrs(), d = g.dst ? dst[i]->ptrs() : s;
				OK(vfgs_hip_host_pipe_submit(p, &s, g.dst ? &d : nullptr, nullptr, nullptr, &tickets[i]));
				CHECK(tickets[i] == (uint64_t)i + 1 && Regs() == want_plain[i - n] && recorded(g, false, 1, 1));
			}
			vfgs_hip_get_params(params2);
			CHECK(!memcmp(params, params2, sizeof params));
			OK(vfgs_hip_host_pipe_wait(p, tickets[2 * n - 1]));      // the last one: every earlier one is home too
			OK(vfgs_hip_host_pipe_wait(p, tickets[3]));              // again: home is home
			for (int i = 0; i < 2 * n; i++)
			{
				CHECK(src[i]->bytes() == orig[i]);                   // (in place: the stub's grain is zero)
				if (g.dst) CHECK(dst[i]->bytes() == g.expected(*src[i]));
			}
			OK(vfgs_hip_host_pipe_close(p));
		}
}

// one thread submits, another waits for every ticket as it is issued -- and sleeps in that wait until the NEXT submit has returned (the
// gate above): wait sleeps without the library's lock (the ThreadSanitizer's walk)
static void walk_two_threads()
{
	const Geo g(200, 40, 10, 2, 2, 8, 16, true, true);
	const int n = 24;
	program(10, 2, 2, true);
	vfgs_hip_model* m = capture(nullptr);
	const std::vector<uint32_t> seeds = seeds_of(n);
	std::vector<std::unique_ptr<HostPic>> src, dst;
	for (int i = 0; i < n; i++) { src.push_back(g.source(true)); dst.push_back(g.destination(true)); }
	vfgs_hip_host_pipe* p = open_pipe(g, 3);
	std::atomic<uint64_t> issued{0}, asleep{0};
	std::atomic<int> waited{0};
	std::thread waiter([&] {
		for (uint64_t t = 1; t <= (uint64_t)n; t++)
		{
			while (issued.load() < t) std::this_thread::yield();
			const Gate gate{&issued, std::min<uint64_t>(t + 1, n), &asleep, t};
			t_gate = &gate;
			OK(vfgs_hip_host_pipe_wait(p, t));
			t_gate = nullptr;
			CHECK(dst[t - 1]->bytes() == g.expected(*src[t - 1]));      // home means home, while the other thread goes on submitting
			waited++;
		}
	});
	for (int i = 0; i < n; i++)
	{
		const vfgs_hip_frame_ptrs s = src[i]->ptrs(), d = dst[i]->ptrs();
		uint64_t t = 0;
		// picture i + 1 is submitted while the other thread sleeps in its wait for picture i (twenty seconds for it to get there)
		const auto t0 = std::chrono::steady_clock::now();
		while (asleep.load() < (uint64_t)i && !g_gate_gave_up && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(20)) std::this_thread::yield();
		CHECK(asleep.load() >= (uint64_t)i || g_gate_gave_up);
		OK(vfgs_hip_host_pipe_submit(p, &s, &d, i % 3 ? m : nullptr, &seeds[i], &t));
		CHECK(t == (uint64_t)i + 1);
		issued.store(t);
	}
	waiter.join();
	CHECK(waited == n);
	OK(vfgs_hip_host_pipe_close(p));
	vfgs_hip_model_release(m);
}

// every refusal between two good pictures: nothing queued, no ticket, no register moved, the next submit gets the next ticket
static void walk_refusals_in_mid_stream()
{
	const Geo g(200, 40, 10, 2, 2, 8, 16, true, true), gi(200, 40, 10, 2, 2, 8, 0, false, false);
	program(8, 2, 2, true);
	vfgs_hip_model* m8 = capture(nullptr);
	program(10, 2, 2, true);
	vfgs_hip_model* gone = capture(nullptr);
	vfgs_hip_model_release(gone);
	vfgs_hip_model* a = capture(nullptr);
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	vfgs_hip_model* mixed = nullptr;
	OK(vfgs_hip_model_capture_mix(&mixed, nullptr));
	vfgs_hip_clear_chroma_mix();
	vfgs_set_seed(9);
	// open
	{
		vfgs_hip_host_pipe* q = (vfgs_hip_host_pipe*)16;
		vfgs_hip_host_pipe_desc d = g.desc(3);
		CHECK(vfgs_hip_host_pipe_open(nullptr, &q) == 43 && q == nullptr);
		CHECK(vfgs_hip_host_pipe_open(&d, nullptr) == 43);
		d.slots = 1; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 43 && strstr(vfgs_hip_last_error_string(), "slots"));
		d.slots = 9; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 43);
		d = g.desc(3); d.dst_stride = d.dst_cstride = 0; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 43 && vfgs_hip_last_error() == 43);
		d = g.desc(3); d.width = 100; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 5 && strstr(vfgs_hip_last_error_string(), "vfgs_hip_host_pipe_open: "));
		d = g.desc(3); d.width = 32000; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 17);
		d = g.desc(3); d.stride = 192; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 6);
		d = g.desc(3); d.cstride += 4; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 8);
		d = g.desc(3); d.dst_stride = 192; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 6);
		d = g.desc(3); d.dst_cstride += 8; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 8);
		d = g.desc(3); d.height = 1864136 * 3; CHECK(vfgs_hip_host_pipe_open(&d, &q) == 15);
		vfgs_set_depth(8);
		d = g.desc(3); d.stride = 224;      // (rows of whole 16-byte units at depth 8 too)
		CHECK(vfgs_hip_host_pipe_open(&d, &q) == 16 && q == nullptr);
		d = g.desc(3);
		vfgs_set_depth(10);
		const int two[2] = {0, 1};
		OK(vfgs_hip_init_devices(two, 2));
		CHECK(vfgs_hip_host_pipe_open(&d, &q) == 43 && strstr(vfgs_hip_last_error_string(), "devices"));
		OK(vfgs_hip_init_devices(two, 1));
	}
	vfgs_hip_host_pipe* p = open_pipe(g, 3);
	vfgs_hip_host_pipe* pi = open_pipe(gi, 2);
	std::vector<std::unique_ptr<HostPic>> src, dst;
	for (int i = 0; i < 3; i++) { src.push_back(g.source(true)); dst.push_back(g.destination(true)); }
	const uint32_t seed = 4242;
	uint64_t t = 0;
	const vfgs_hip_frame_ptrs s0 = src[0]->ptrs(), d0 = dst[0]->ptrs(), s1 = src[1]->ptrs(), d1 = dst[1]->ptrs(), s2 = src[2]->ptrs();
	OK(vfgs_hip_host_pipe_submit(p, &s0, &d0, a, &seed, &t));
	CHECK(t == 1);
	const Regs before;
	const unsigned long long l0 = launches();
	t = 99;
	// (a refused submit queues nothing: the model of the runtime sees no operation)
	auto on = [&](vfgs_hip_host_pipe* q, const vfgs_hip_frame_ptrs* s, const vfgs_hip_frame_ptrs* d, const vfgs_hip_model* m, const uint32_t* sd) {
		uint64_t st0[3], st1[3];
		vfgs_stub_stats(st0);
		const int rc = vfgs_hip_host_pipe_submit(q, s, d, m, sd, &t);
		vfgs_stub_stats(st1);
		CHECK(rc == 0 || st0[0] == st1[0]);
		return rc;
	};
	auto sub = [&](const vfgs_hip_frame_ptrs* s, const vfgs_hip_frame_ptrs* d, const vfgs_hip_model* m) { return on(p, s, d, m, &seed); };
	CHECK(vfgs_hip_host_pipe_submit(nullptr, &s1, &d1, a, &seed, &t) == 43);
	CHECK(sub(nullptr, &d1, a) == 43);
	CHECK(vfgs_hip_host_pipe_submit(p, &s1, &d1, a, &seed, nullptr) == 43);
	CHECK(vfgs_hip_host_pipe_submit((vfgs_hip_host_pipe*)&t, &s1, &d1, a, &seed, &t) == 43);      // never a pipe: not dereferenced
	CHECK(sub(&s1, nullptr, a) == 43 && strstr(vfgs_hip_last_error_string(), "destination"));
	CHECK(on(pi, &s2, &d1, nullptr, nullptr) == 43 && strstr(vfgs_hip_last_error_string(), "in place"));
	CHECK(vfgs_hip_host_pipe_wait(p, 2) == 43 && vfgs_hip_host_pipe_wait(p, 0) == 43 && vfgs_hip_host_pipe_wait(nullptr, 1) == 43);
	{ vfgs_hip_frame_ptrs x = s1; x.U = nullptr; CHECK(sub(&x, &d1, a) == 18 && strstr(vfgs_hip_last_error_string(), "vfgs_hip_host_pipe_submit: ")); }
	{ vfgs_hip_frame_ptrs x = d1; x.V = x.U; CHECK(sub(&s1, &x, a) == 18); }
	{ vfgs_hip_frame_ptrs x = d1; x.Y = s1.Y; CHECK(sub(&s1, &x, a) == 18 && strstr(vfgs_hip_last_error_string(), "shares bytes")); }
	CHECK(sub(&s1, &d1, gone) == 41 && sub(&s1, &d1, m8) == 41 && strstr(vfgs_hip_last_error_string(), "depth 8"));
	CHECK(sub(&s1, &d1, mixed) == 41 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	CHECK(sub(&s1, &d1, a) == 41 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
	vfgs_hip_clear_chroma_mix();
	vfgs_set_depth(12);
	CHECK(sub(&s1, &d1, a) == 43 && strstr(vfgs_hip_last_error_string(), "depth 12"));
	vfgs_set_depth(10);
	vfgs_set_chroma_subsampling(2, 1);
	CHECK(sub(&s1, &d1, a) == 43);
	vfgs_set_chroma_subsampling(2, 2);
	OK(vfgs_hip_overlap_begin(nullptr));
	CHECK(sub(&s1, &d1, a) == 43 && strstr(vfgs_hip_last_error_string(), "overlap"));
	OK(vfgs_hip_overlap_end(nullptr));
	{
		const int two[2] = {0, 1};
		OK(vfgs_hip_init_devices(two, 2));
		CHECK(sub(&s1, &d1, a) == 43);
		OK(vfgs_hip_init_devices(two, 1));
	}
	// the programmed state of a submit without a model: an undefined pattern-LUT entry (4); a general-form model under a programmed mix (38,
	// in place: the mix has no narrowed form).  (9, a scale shift out of range, is behind them in the device call; no setter programs one)
	unsigned char lut[256], keep[256];
	OK(vfgs_hip_get_luts(1, nullptr, keep));
	memset(lut, 0x90, sizeof lut);
	vfgs_set_pattern_lut(1, lut);
	CHECK(sub(&s1, &d1, nullptr) == 4);
	vfgs_set_pattern_lut(1, keep);
	for (int i = 0; i < 256; i++) lut[i] = (unsigned char)((i >> 5) << 4);
	vfgs_set_pattern_lut(0, lut);
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	CHECK(on(pi, &s2, nullptr, nullptr, nullptr) == 38);
	vfgs_hip_clear_chroma_mix();
	CHECK(t == 99 && Regs() == before && launches() == l0);
	OK(sub(&s1, &d1, a));
	CHECK(t == 2);
	OK(vfgs_hip_host_pipe_submit(pi, &s2, nullptr, nullptr, nullptr, &t));
	CHECK(t == 1);
	OK(vfgs_hip_host_pipe_wait(p, 2));
	CHECK(dst[0]->bytes() == g.expected(*src[0]) && dst[1]->bytes() == g.expected(*src[1]));
	OK(vfgs_hip_host_pipe_close(pi));      // (drains: s2 may go)
	OK(vfgs_hip_host_pipe_close(p));
	CHECK(vfgs_hip_host_pipe_close(p) == 43 && vfgs_hip_host_pipe_wait(p, 1) == 43 && sub(&s1, &d1, a) == 43);
	for (vfgs_hip_model* m : {m8, a, mixed}) vfgs_hip_model_release(m);
}

// seven pictures through two slots, never waited for: close brings them home
static void walk_close_with_pictures_in_flight()
{
	for (int pinned = 0; pinned < 2; pinned++)
	{
		const Geo g(264, 33, 8, 1, 1, 0, 16, true, false);
		const int n = 7;
		program(8, 1, 1, false);
		vfgs_hip_model* m = capture(nullptr);
		std::vector<std::unique_ptr<HostPic>> src, dst;
		for (int i = 0; i < n; i++) { src.push_back(g.source(pinned != 0)); dst.push_back(g.destination(pinned != 0)); }
		vfgs_hip_host_pipe* p = open_pipe(g, 2);
		for (int i = 0; i < n; i++)
		{
			const vfgs_hip_frame_ptrs s = src[i]->ptrs(), d = dst[i]->ptrs();
			const uint32_t seed = 1000 + i;
			uint64_t t = 0;
			OK(vfgs_hip_host_pipe_submit(p, &s, &d, m, &seed, &t));
			CHECK(t == (uint64_t)i + 1);
		}
		vfgs_hip_model_release(m);
		OK(vfgs_hip_host_pipe_close(p));
		for (int i = 0; i < n; i++) CHECK(dst[i]->bytes() == g.expected(*src[i]));
	}
}

// vfgs_hip_shutdown drains and closes an open pipe; its handle is stale behind it and refused without being looked at; a new pipe works
static void walk_shutdown_with_an_open_pipe()
{
	const Geo g(200, 40, 10, 2, 2, 0, 16, true, false);
	program(10, 2, 2, true);
	std::vector<std::unique_ptr<HostPic>> src, dst;
	// (pageable: pinned memory is the device's and goes with the shutdown)
	for (int i = 0; i < 3; i++) { src.push_back(g.source(false)); dst.push_back(g.destination(false)); }
	vfgs_hip_host_pipe* p = open_pipe(g, 3);
	vfgs_hip_host_pipe* idle = open_pipe(g, 8);
	uint64_t t = 0;
	for (int i = 0; i < 2; i++)
	{
		const vfgs_hip_frame_ptrs s = src[i]->ptrs(), d = dst[i]->ptrs();
		OK(vfgs_hip_host_pipe_submit(p, &s, &d, nullptr, nullptr, &t));
	}
	vfgs_hip_shutdown();
	for (int i = 0; i < 2; i++) CHECK(dst[i]->bytes() == g.expected(*src[i]));
	const vfgs_hip_frame_ptrs s = src[2]->ptrs(), d = dst[2]->ptrs();
	CHECK(vfgs_hip_host_pipe_submit(p, &s, &d, nullptr, nullptr, &t) == 43 && vfgs_hip_host_pipe_wait(p, 1) == 43 && vfgs_hip_host_pipe_close(p) == 43);
	CHECK(vfgs_hip_host_pipe_close(idle) == 43);
	vfgs_hip_host_pipe* q = open_pipe(g, 0);      // the library initialises again
	OK(vfgs_hip_host_pipe_submit(q, &s, &d, nullptr, nullptr, &t));
	CHECK(t == 1);
	OK(vfgs_hip_host_pipe_wait(q, 1));
	CHECK(dst[2]->bytes() == g.expected(*src[2]));
	// (q stays open: run_walks shuts down with it)
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"steady_stream", walk_steady_stream},
		{"two_threads", walk_two_threads},
		{"refusals_in_mid_stream", walk_refusals_in_mid_stream},
		{"close_with_pictures_in_flight", walk_close_with_pictures_in_flight},
		{"shutdown_with_an_open_pipe", walk_shutdown_with_an_open_pipe},
	});
}
