// TEST INFRASTRUCTURE.  Models built from AFGS1 parameter sets (include/vfgs_hip_fw.h: vfgs_hip_models_from_afgs1; include/vfgs_hip.h:
// vfgs_hip_model_image, vfgs_hip_get_model_build_stats) in the host layer of libvfgs_hip, compiled with a sanitizer over the unchanged
// tests/sanitize/hip_stub.cpp, as tests/sanitize_sp_models/sp_model_walks.cpp drives the captured models: chunks and slabs of every size,
// release in every order, use in both list calls with a model per picture, every refusal with nothing changed, shutdown with live models,
// the read-back with a short buffer, and a thread that builds and releases while another makes list calls.
//
// The stub knows nothing of fw_models_kernel, and the host layer does not name its launcher (the entry point hands it down), so this file
// brings its OWN stand-in for vfgs::launch_fw_models below: it reads the job table the host queued and writes exactly the bytes the kernel
// addresses -- every model's 32-byte record and the image_layout() bytes behind it -- so a slab that is too small, a wrong offset or a
// table that was not copied is a sanitizer report or a failed check.  The stand-in has no access to the stub's queue: it waits for the
// stream (which runs the queued copy of the job table) and then writes at once; the list launches that READ the models stay deferred, so
// a slab handed on or freed while a queued launch could still read it is seen there.  Values are the GPU suite's business
// (tests/test_gpu_models_from_afgs1.py).
//
// usage: model_build_walks [walk ...]     (no argument: all of them)
#include <hip/hip_runtime.h>

#include <algorithm>

#define WALKS_SEED 43
#define WALKS_HAVE_HIP_RUNTIME_H
#include "../sanitize/walks.h"
#include "../../versatilefilmgrain_amd/csrc/vfgs_model_build.h"

using Planes = BarePlanes;

static std::atomic<uint64_t> g_standin_launches{0}, g_standin_models{0};

namespace vfgs {
hipError_t launch_fw_models(const FwConstants* k, const FwModelJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream)
{
	if (n <= 0 || n > kFwModelChunk || !k || !jobs) return hipErrorInvalidValue;
	(void)hipStreamSynchronize(stream);      // the job table's copy has run
	unsigned char x = 0;
	for (size_t i = 0; i < sizeof(FwConstants); i += 64) x ^= ((const unsigned char*)k)[i];
	const uint8_t* prev_end = (const uint8_t*)(jobs + kFwModelChunk);       // the models lie behind the table, in order, without overlap
	for (int i = 0; i < n; i++)
	{
		const FwModelJob j = jobs[i];
		const ImageLayout L = image_layout(csubx, csuby, j.one_y != 0, j.one_c != 0, depth8 != 0);
		if (((uintptr_t)j.dst & 15) || j.dst < prev_end || j.lag < 1 || j.lag > 3 || j.scale < 1 || j.scale > 15 || j.shift < 1 || j.shift > 7)
		{
			fprintf(stderr, "FAILED stand-in: job %d of %d is not what the kernel may be given\n", i, n);
			g_fail++;
			return hipErrorInvalidValue;
		}
		memcpy(j.dst, &j.rec, kModelRecordBytes);
		memset(j.dst + kModelRecordBytes, 0x40 + (i & 31) + (x & 0), (size_t)L.bytes);
		prev_end = j.dst + kModelRecordBytes + L.bytes;
	}
	g_standin_launches++;
	g_standin_models += (uint64_t)n;
	return hipSuccess;
}
}  // namespace vfgs

// a valid parameter set; `hot`: a luma scaling point of 255 at grain_scaling 11 -- the general form at 8 bit
static fgs_afgs1 make_set(bool hot = false)
{
	fgs_afgs1 a;
	memset(&a, 0, sizeof a);
	a.grain_seed = (uint16_t)rnd();
	a.num_y_points = (uint8_t)(2 + rnd() % 13);
	for (int k = 0; k < a.num_y_points; k++) { a.point_y_values[k] = (uint8_t)(k * 18 + rnd() % 18); a.point_y_scaling[k] = (uint8_t)(rnd() % 200); }
	if (hot) a.point_y_scaling[1] = 255;
	a.num_cb_points = (uint8_t)(rnd() % 11);
	a.num_cr_points = (uint8_t)(rnd() % 11);
	for (int k = 0; k < 10; k++)
	{
		a.point_cb_values[k] = (uint8_t)(k * 25 + rnd() % 25); a.point_cb_scaling[k] = (uint8_t)(rnd() % 200);
		a.point_cr_values[k] = (uint8_t)(k * 25 + rnd() % 25); a.point_cr_scaling[k] = (uint8_t)(rnd() % 200);
	}
	a.chroma_scaling_from_luma = (uint8_t)(rnd() & 1);
	a.grain_scaling = hot ? 11 : (uint8_t)(8 + rnd() % 4);
	a.ar_coeff_lag = (uint8_t)(1 + rnd() % 3);
	for (int k = 0; k < 24; k++) a.ar_coeffs_y[k] = (int16_t)((int)(rnd() % 256) - 128);
	for (int k = 0; k < 25; k++) { a.ar_coeffs_cb[k] = (int16_t)((int)(rnd() % 256) - 128); a.ar_coeffs_cr[k] = (int16_t)((int)(rnd() % 256) - 128); }
	a.ar_coeff_shift = (uint8_t)(6 + rnd() % 4);
	a.grain_scale_shift = (uint8_t)(rnd() % 4);
	a.clip_to_restricted_range = (uint8_t)(rnd() & 1);
	return a;
}

static std::vector<fgs_afgs1> make_sets(unsigned n, bool some_hot = false)
{
	std::vector<fgs_afgs1> v;
	for (unsigned i = 0; i < n; i++) v.push_back(make_set(some_hot && i % 3 == 0));
	return v;
}

static std::vector<vfgs_hip_model*> build(const std::vector<fgs_afgs1>& sets, void* stream)
{
	std::vector<vfgs_hip_model*> out(sets.size(), (vfgs_hip_model*)0x10);
	OK(vfgs_hip_models_from_afgs1(sets.data(), (unsigned)sets.size(), out.data(), stream));
	for (vfgs_hip_model* m : out) CHECK(m != nullptr && m != (vfgs_hip_model*)0x10);
	return out;
}

static void list_call(const std::vector<vfgs_hip_model*>& models, const std::vector<fgs_afgs1>& sets, int depth, int sx, int sy, void* stream)
{
	const int n = (int)models.size();
	Planes p(n, 264, 40, depth, sx, sy, false);
	std::vector<uint32_t> seeds;
	for (const fgs_afgs1& a : sets) seeds.push_back(vfgs_hip_afgs1_seed(&a));
	OK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), models.data(), seeds.data(), (unsigned)n, 264, 40, p.stride, p.cstride, stream));
	hipStreamSynchronize((hipStream_t)stream);
}

// ---- walks ----------------------------------------------------------------------------------------------------------------------------

static void walk_sizes()
{
	hipStream_t s = nullptr;
	hipStreamCreateWithFlags(&s, 0);
	const int geo[][3] = {{10, 2, 2}, {8, 1, 1}, {12, 2, 1}, {8, 1, 2}};
	for (const auto& g : geo)
		for (unsigned n : {1u, (unsigned)vfgs::kFwModelChunk + 1, 70u})
		{
			set_format(g[0], g[1], g[2]);
			const auto sets = make_sets(n, g[0] == 8);
			const Stats s0;
			const uint64_t l0 = g_standin_launches;
			const auto models = build(sets, s);
			const Stats s1;
			const uint64_t chunks = (n + vfgs::kFwModelChunk - 1) / vfgs::kFwModelChunk;
			CHECK(s1.v[0] == s0.v[0] + 1 && s1.v[1] == s0.v[1] + n && s1.v[2] == s0.v[2] + chunks && s1.v[3] == s0.v[3] + chunks && s1.v[6] == vfgs::kFwModelChunk);
			CHECK(g_standin_launches == l0 + chunks);
			bool general = false;
			for (unsigned i = 0; i < n; i++)
			{
				int info[8];
				OK(vfgs_hip_model_info(models[i], info));
				CHECK(info[0] == g[0] && info[1] == g[1] && info[2] == g[2] && info[5] == sets[i].grain_scaling - (g[0] - 8) && info[6] == (sets[i].clip_to_restricted_range != 0));
				general = general || !info[3];
				touch_image(models[i]);
			}
			CHECK(general == (g[0] == 8));        // the hot sets fall back to the general form at 8 bit only
			list_call(models, sets, g[0], g[1], g[2], s);
			for (vfgs_hip_model* m : models) vfgs_hip_model_release(m);
		}
	hipStreamDestroy(s);
}

static void walk_release_orders()
{
	hipStream_t s = nullptr, s2 = nullptr;
	hipStreamCreateWithFlags(&s, 0);
	hipStreamCreateWithFlags(&s2, 0);
	set_format(10, 2, 2);
	const unsigned n = vfgs::kFwModelChunk + 1;
	const auto sets = make_sets(n);
	for (int round = 0; round < 4; round++)
	{
		auto models = build(sets, s);
		// partial, shuffled release: every other model goes, in a shuffled order; the others serve a launch on ANOTHER stream that is still
		// queued when they go too
		std::vector<unsigned> order;
		for (unsigned i = 0; i < n; i++) order.push_back(i);
		for (unsigned i = n - 1; i > 0; i--) std::swap(order[i], order[rnd() % (i + 1)]);
		std::vector<vfgs_hip_model*> keep;
		std::vector<fgs_afgs1> keep_sets;
		for (unsigned i : order)
			if (i & 1) vfgs_hip_model_release(models[i]);
			else { keep.push_back(models[i]); keep_sets.push_back(sets[i]); }
		for (unsigned i : order)
			if (i & 1) { int info[8]; CHECK(vfgs_hip_model_info(models[i], info) == 41); }
		Planes p((int)keep.size(), 264, 40, 10, 2, 2, false);
		std::vector<uint32_t> seeds(keep.size(), 77u);
		OK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), keep.data(), seeds.data(), (unsigned)keep.size(), 264, 40, p.stride, p.cstride, s2));
		for (vfgs_hip_model* m : keep) vfgs_hip_model_release(m);      // the launch is queued, not run
		vfgs_hip_model_release(keep[0]);                              // released before: no-op
		vfgs_hip_model_release(nullptr);
		// the next build takes the slabs that were just left -- after their readers -- or new ones; either way the queued launch reads live bytes
		auto again = build(sets, s);
		for (vfgs_hip_model* m : again) touch_image(m);
		hipStreamSynchronize(s2);
		for (vfgs_hip_model* m : again) vfgs_hip_model_release(m);
	}
	// steady state: build / use / release, no allocation and no free after the first cycle
	uint64_t mark[2] = {0, 0};
	for (int cycle = 0; cycle < 4; cycle++)
	{
		const auto chunk = make_sets(vfgs::kFwModelChunk);
		auto models = build(chunk, s);
		list_call(models, chunk, 10, 2, 2, s);
		for (vfgs_hip_model* m : models) vfgs_hip_model_release(m);
		const Stats st;
		if (cycle == 0) { mark[0] = st.v[4]; mark[1] = st.v[5]; }
		CHECK(st.v[4] == mark[0] && st.v[5] == mark[1]);
	}
	hipStreamDestroy(s);
	hipStreamDestroy(s2);
}

static void walk_both_list_calls()
{
	hipStream_t s = nullptr;
	hipStreamCreateWithFlags(&s, 0);
	for (int depth : {8, 10, 12})
		for (int sy : {2, 1})
		{
			set_format(depth, 2, sy);
			const auto sets = make_sets(7, depth == 8);
			auto models = build(sets, s);
			list_call(models, sets, depth, 2, sy, nullptr);            // (another stream than the build's: waits by event)
			const unsigned shift = depth == 8 ? 0 : 16 - depth;
			Planes p(7, 264, 40, depth, 2, sy, true);
			std::vector<uint32_t> seeds;
			for (const fgs_afgs1& a : sets) seeds.push_back(vfgs_hip_afgs1_seed(&a));
			OK(vfgs_hip_add_grain_sp_frame_list_models_dev(p.sp_list.data(), p.sp_list.data(), models.data(), seeds.data(), 7, 264, 40, p.stride, p.cstride, shift, s));
			OK(vfgs_hip_add_grain_sp_frame_list_models_dev(p.sp_list.data(), p.sp_list.data(), models.data(), nullptr, 7, 264, 40, p.stride, p.cstride, shift, s));
			hipStreamSynchronize(s);
			// inside an overlap region the build takes the region's stream
			OK(vfgs_hip_overlap_begin(s));
			auto more = build(sets, s);
			OK(vfgs_hip_add_grain_sp_frame_list_models_dev(p.sp_list.data(), p.sp_list.data(), more.data(), seeds.data(), 7, 264, 40, p.stride, p.cstride, shift, s));
			OK(vfgs_hip_overlap_end(s));
			hipStreamSynchronize(s);
			for (vfgs_hip_model* m : more) { touch_image(m); vfgs_hip_model_release(m); }
			for (vfgs_hip_model* m : models) vfgs_hip_model_release(m);
		}
	hipStreamDestroy(s);
}

static void refused(std::vector<fgs_afgs1> sets, unsigned at, int code, const char* what)
{
	std::vector<vfgs_hip_model*> out(sets.size(), (vfgs_hip_model*)0x10);
	const Stats s0;
	const Regs r0;
	const uint64_t l0 = g_standin_launches;
	const int rc = vfgs_hip_models_from_afgs1(sets.data(), (unsigned)sets.size(), out.data(), nullptr);
	char idx[32];
	snprintf(idx, sizeof idx, "parameter set %u:", at);
	if (rc != code || !strstr(vfgs_hip_last_error_string(), idx))
	{
		fprintf(stderr, "FAILED refusal %s at %u: %d (%s), expected %d\n", what, at, rc, vfgs_hip_last_error_string(), code);
		g_fail++;
	}
	for (vfgs_hip_model* m : out) CHECK(m == nullptr);
	CHECK(Stats() == s0 && Regs() == r0 && g_standin_launches == l0);
}

static void walk_refusals()
{
	set_format(8, 2, 2);
	vfgs_set_seed(5);
	for (unsigned at : {0u, 4u})
	{
		auto base = make_sets(5);
		for (auto& a : base) a.chroma_scaling_from_luma = 0;
		auto v = base; v[at].ar_coeff_lag = 0; refused(v, at, 42, "lag 0");
		v = base; v[at].ar_coeff_lag = 4; refused(v, at, 42, "lag 4");
		v = base; v[at].num_y_points = 15; refused(v, at, 42, "15 luma points");
		v = base; v[at].num_cb_points = 11; refused(v, at, 42, "11 Cb points");
		v = base; v[at].num_cr_points = 255; refused(v, at, 42, "255 Cr points");
		v = base; v[at].num_y_points = 3; v[at].point_y_values[2] = v[at].point_y_values[1]; refused(v, at, 42, "equal luma points");
		v = base; v[at].num_cb_points = 2; v[at].point_cb_values[0] = 9; v[at].point_cb_values[1] = 8; refused(v, at, 42, "falling Cb points");
		v = base; v[at].num_cr_points = 2; v[at].point_cr_values[0] = 9; v[at].point_cr_values[1] = 9; refused(v, at, 42, "equal Cr points");
		v = base; v[at].ar_coeff_shift = 0; refused(v, at, 42, "ar_coeff_shift 0");
		v = base; v[at].ar_coeff_shift = 16; refused(v, at, 42, "ar_coeff_shift 16");
		v = base; v[at].grain_scale_shift = 7; refused(v, at, 42, "grain_scale_shift 7");
		v = base; v[at].grain_scaling = 7; refused(v, at, 9, "grain_scaling 7");
		v = base; v[at].grain_scaling = 14; refused(v, at, 9, "grain_scaling 14");
		// not refused: chroma points out of order that chroma_scaling_from_luma leaves unused
		v = base; v[at].chroma_scaling_from_luma = 1; v[at].num_cb_points = 2; v[at].point_cb_values[0] = 9; v[at].point_cb_values[1] = 8;
		for (vfgs_hip_model* m : build(v, nullptr)) vfgs_hip_model_release(m);
	}
	const auto sets = make_sets(2);
	vfgs_hip_model* out[2] = {(vfgs_hip_model*)0x10, (vfgs_hip_model*)0x10};
	const Stats s0;
	CHECK(vfgs_hip_models_from_afgs1(sets.data(), 2, nullptr, nullptr) == 41);
	CHECK(vfgs_hip_models_from_afgs1(nullptr, 2, out, nullptr) == 41 && !out[0] && !out[1]);
	out[0] = out[1] = (vfgs_hip_model*)0x10;
	CHECK(vfgs_hip_models_from_afgs1(sets.data(), 0, out, nullptr) == 0 && out[0] == (vfgs_hip_model*)0x10);      // n == 0: no call at all
	CHECK(vfgs_hip_models_from_afgs1(nullptr, 0, nullptr, nullptr) == 0);
	CHECK(Stats() == s0);
}

static void walk_shutdown_and_short_buffer()
{
	set_format(10, 2, 2);
	const auto sets = make_sets(vfgs::kFwModelChunk + 3);
	auto models = build(sets, nullptr);
	// the read-back: a dead handle, a short buffer, no buffer, an exact one
	int info[8];
	OK(vfgs_hip_model_info(models[1], info));
	std::vector<uint8_t> b((size_t)info[7] - 1);
	size_t need = 0;
	CHECK(vfgs_hip_model_image(models[1], b.data(), b.size(), &need) == 6 && need == (size_t)info[7]);
	need = 0;
	CHECK(vfgs_hip_model_image(models[1], nullptr, 0, &need) == 6 && need == (size_t)info[7]);
	CHECK(vfgs_hip_model_image(models[1], b.data(), b.size(), nullptr) == 6);
	CHECK(vfgs_hip_model_image(nullptr, b.data(), b.size(), &need) == 41);
	touch_image(models[1]);
	vfgs_hip_model_release(models[0]);
	CHECK(vfgs_hip_model_image(models[0], b.data(), b.size(), &need) == 41);
	// shutdown with live models (and a slab that is partly released): everything goes, the handles are dead, nothing leaks
	vfgs_hip_shutdown();
	CHECK(vfgs_hip_model_info(models[2], info) == 41);
	for (vfgs_hip_model* m : models) vfgs_hip_model_release(m);
	// ... and the library starts again
	set_format(8, 2, 2);
	auto again = build(make_sets(3, true), nullptr);
	for (vfgs_hip_model* m : again) { touch_image(m); vfgs_hip_model_release(m); }
	vfgs_hip_shutdown();
}

static void walk_threads()
{
	set_format(10, 2, 2);
	const auto mine = make_sets(5);
	auto models = build(mine, nullptr);
	std::atomic<bool> stop{false};
	std::thread builder([&] {
		hipStream_t s = nullptr;
		hipStreamCreateWithFlags(&s, 0);
		uint32_t lcg = 7;
		while (!stop)
		{
			lcg = lcg_step(lcg);
			std::vector<fgs_afgs1> sets(1 + (lcg >> 8) % 40, mine[(lcg >> 16) % 5]);
			std::vector<vfgs_hip_model*> out(sets.size());
			if (vfgs_hip_models_from_afgs1(sets.data(), (unsigned)sets.size(), out.data(), s)) { g_fail++; break; }
			for (size_t i = out.size(); i-- > 0;) vfgs_hip_model_release(out[i]);
		}
		hipStreamDestroy(s);
	});
	hipStream_t s = nullptr;
	hipStreamCreateWithFlags(&s, 0);
	for (int i = 0; i < 30; i++)
	{
		Planes p(5, 264, 40, 10, 2, 2, false);
		std::vector<uint32_t> seeds(5, (uint32_t)i);
		OK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), models.data(), seeds.data(), 5, 264, 40, p.stride, p.cstride, s));
		hipStreamSynchronize(s);
	}
	stop = true;
	builder.join();
	for (vfgs_hip_model* m : models) { touch_image(m); vfgs_hip_model_release(m); }
	hipStreamDestroy(s);
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"sizes", walk_sizes},
		{"release_orders", walk_release_orders},
		{"both_list_calls", walk_both_list_calls},
		{"refusals", walk_refusals},
		{"threads", walk_threads},
		{"shutdown_and_short_buffer", walk_shutdown_and_short_buffer},
	});
}
