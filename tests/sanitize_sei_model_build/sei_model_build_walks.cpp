// TEST INFRASTRUCTURE.  Models built from FGC SEI messages (include/vfgs_hip_fw.h: vfgs_hip_models_from_sei) in the host layer of
// libvfgs_hip, compiled with a sanitizer over the unchanged tests/sanitize/hip_stub.cpp, as tests/sanitize_model_build/model_build_walks.cpp
// drives the models built from AFGS1 parameter sets: chunks and slabs of every size, release in every order, use in both list calls with a
// model per picture, every refusal with nothing changed, shutdown with live models, the read-back with a short buffer, SEI and AFGS1 builds
// alternating on the slab pool (their job tables differ in size: a slab is reused only where its staging buffer suffices too), and threads
// that build and release while another makes list calls.
//
// The stub knows nothing of fw_sei_build_kernel or fw_models_kernel, and the host layer names neither launcher (the entry points hand
// them down), so this file brings its OWN stand-ins for both: each reads the job table the host queued and writes exactly the bytes the
// kernel addresses -- every model's 32-byte record and the image_layout() bytes behind it -- so a slab that is too small, a staging buffer
// that is too short for the table, a wrong offset or a table that was not copied is a sanitizer report or a failed check.  Values are the
// GPU suite's business (tests/test_gpu_models_from_sei.py).
//
// usage: sei_model_build_walks [walk ...]     (no argument: all of them)
#include <hip/hip_runtime.h>

#include <algorithm>

#define WALKS_SEED 43
#define WALKS_HAVE_HIP_RUNTIME_H
#include "../sanitize/walks.h"
#include "../../versatilefilmgrain_amd/csrc/vfgs_model_build.h"

using Planes = BarePlanes;

static std::atomic<uint64_t> g_standin_launches{0}, g_standin_models{0};

namespace vfgs {
template <class Job, class Valid>
static hipError_t standin(const FwConstants* k, const Job* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream, int marker, Valid valid)
{
	if (n <= 0 || n > kFwModelChunk || !k || !jobs) return hipErrorInvalidValue;
	(void)hipStreamSynchronize(stream);      // the job table's copy has run
	unsigned char x = 0;
	for (size_t i = 0; i < sizeof(FwConstants); i += 64) x ^= ((const unsigned char*)k)[i];
	const uint8_t* prev_end = (const uint8_t*)(jobs + kFwModelChunk);       // the models lie behind the table, in order, without overlap
	for (int i = 0; i < n; i++)
	{
		const Job j = jobs[i];
		const ImageLayout L = image_layout(csubx, csuby, j.one_y != 0, j.one_c != 0, depth8 != 0);
		if (((uintptr_t)j.dst & 15) || j.dst < prev_end || !valid(j))
		{
			fprintf(stderr, "FAILED stand-in: job %d of %d is not what the kernel may be given\n", i, n);
			g_fail++;
			return hipErrorInvalidValue;
		}
		memcpy(j.dst, &j.rec, kModelRecordBytes);
		memset(j.dst + kModelRecordBytes, marker + (i & 31) + (x & 0), (size_t)L.bytes);
		prev_end = j.dst + kModelRecordBytes + L.bytes;
	}
	g_standin_launches++;
	g_standin_models += (uint64_t)n;
	return hipSuccess;
}

hipError_t launch_fw_sei_build(const FwConstants* k, const FwSeiJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream)
{
	return standin(k, jobs, n, csubx, csuby, depth8, stream, 0x40, [](const FwSeiJob& j) {
		bool ok = (j.kind == 0 || j.kind == 1) && j.np_luma >= 0 && j.np_luma <= 8 && j.np_chroma >= 0 && j.np_chroma <= 8 && (!j.kind || (j.ar_scale >= 1 && j.ar_scale <= 15));
		for (int c = 0; c < 3; c++) ok = ok && j.slot[c] >= -1 && j.slot[c] < 8;
		ok = ok && (!j.one_y || j.slot[0] >= 0) && (!j.one_c || (j.slot[1] >= 0 && j.slot[2] >= 0));
		return ok;
	});
}

hipError_t launch_fw_models(const FwConstants* k, const FwModelJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream)
{
	return standin(k, jobs, n, csubx, csuby, depth8, stream, 0x80,
	               [](const FwModelJob& j) { return j.lag >= 1 && j.lag <= 3 && j.scale >= 1 && j.scale <= 15 && j.shift >= 1 && j.shift <= 7; });
}
}  // namespace vfgs

// a valid message: either kind, 1..12 intervals per component (more than 8 distinct parameter sets happen), chroma components absent at
// times; `hot`: one interval per component with a scale of 255 at a stored shift of 11+ -- the general form at 8 bit, one-pattern above
static fgs_sei make_sei(bool hot = false)
{
	fgs_sei m;
	memset(&m, 0, sizeof m);
	const bool ar = !hot && (rnd() & 1);
	m.model_id = ar ? (uint8_t)(1 + rnd() % 3) : 0;
	m.log2_scale_factor = hot ? 6 : (uint8_t)((ar ? 3 : 2) + rnd() % 6);
	for (int c = 0; c < 3; c++)
	{
		m.comp_model_present_flag[c] = (uint8_t)(c == 0 || hot || rnd() % 4 != 0);
		const int n = hot ? 1 : 1 + (int)(rnd() % 12);
		m.num_intensity_intervals[c] = (uint16_t)n;
		m.num_model_values[c] = ar ? 6 : 3;
		for (int k = 0; k < n; k++)
		{
			m.intensity_interval_lower_bound[c][k] = (uint8_t)(hot ? 0 : k * 20 + rnd() % 10);
			m.intensity_interval_upper_bound[c][k] = (uint8_t)(hot ? 255 : k * 20 + 10 + rnd() % 10);
			int16_t* v = m.comp_model_value[c][k];
			v[0] = (int16_t)(hot ? 255 : rnd() % 200);
			if (ar) { v[1] = (int16_t)((int)(rnd() % 201) - 100); v[3] = (int16_t)((int)(rnd() % 121) - 60); v[4] = (int16_t)(rnd() % (1u << m.log2_scale_factor)); v[5] = (int16_t)((int)(rnd() % 81) - 40); }
			else { v[1] = (int16_t)(rnd() % 16); v[2] = (int16_t)(rnd() % 16); }
		}
	}
	return m;
}

static std::vector<fgs_sei> make_seis(unsigned n, bool some_hot = false)
{
	std::vector<fgs_sei> v;
	for (unsigned i = 0; i < n; i++) v.push_back(make_sei(some_hot && i % 3 == 0));
	return v;
}

static fgs_afgs1 make_afgs1()
{
	fgs_afgs1 a;
	memset(&a, 0, sizeof a);
	a.grain_seed = (uint16_t)rnd();
	a.num_y_points = 2;
	a.point_y_values[1] = 255; a.point_y_scaling[0] = (uint8_t)(rnd() % 200); a.point_y_scaling[1] = (uint8_t)(rnd() % 200);
	a.chroma_scaling_from_luma = 1;
	a.grain_scaling = (uint8_t)(8 + rnd() % 4);
	a.ar_coeff_lag = (uint8_t)(1 + rnd() % 3);
	for (int k = 0; k < 24; k++) a.ar_coeffs_y[k] = (int16_t)((int)(rnd() % 256) - 128);
	a.ar_coeff_shift = 7;
	return a;
}

static std::vector<vfgs_hip_model*> build(const std::vector<fgs_sei>& msgs, void* stream)
{
	std::vector<vfgs_hip_model*> out(msgs.size(), (vfgs_hip_model*)0x10);
	OK(vfgs_hip_models_from_sei(msgs.data(), (unsigned)msgs.size(), out.data(), stream));
	for (vfgs_hip_model* m : out) CHECK(m != nullptr && m != (vfgs_hip_model*)0x10);
	return out;
}

static std::vector<vfgs_hip_model*> build_afgs1(const std::vector<fgs_afgs1>& sets, void* stream)
{
	std::vector<vfgs_hip_model*> out(sets.size(), (vfgs_hip_model*)0x10);
	OK(vfgs_hip_models_from_afgs1(sets.data(), (unsigned)sets.size(), out.data(), stream));
	for (vfgs_hip_model* m : out) CHECK(m != nullptr && m != (vfgs_hip_model*)0x10);
	return out;
}

static void list_call(const std::vector<vfgs_hip_model*>& models, int depth, int sx, int sy, void* stream)
{
	const int n = (int)models.size();
	Planes p(n, 264, 40, depth, sx, sy, false);
	std::vector<uint32_t> seeds;
	for (int i = 0; i < n; i++) seeds.push_back(rnd());
	OK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), models.data(), seeds.data(), (unsigned)n, 264, 40, p.stride, p.cstride, stream));
	hipStreamSynchronize((hipStream_t)stream);
}

// ---- walks ----------------------------------------------------------------------------------------------------------------------------

static void walk_sizes()
{
	hipStream_t s = nullptr;
	hipStreamCreateWithFlags(&s, 0);
	const int geo[][4] = {{10, 2, 2, 0}, {8, 1, 1, 1}, {12, 2, 1, 1}, {8, 1, 2, 0}};
	for (const auto& g : geo)
		for (unsigned n : {1u, 32u, 33u, 100u})
		{
			set_format(g[0], g[1], g[2], g[3]);
			const auto msgs = make_seis(n, true);
			const Stats s0;
			const uint64_t l0 = g_standin_launches;
			const auto models = build(msgs, s);
			const Stats s1;
			const uint64_t chunks = (n + vfgs::kFwModelChunk - 1) / vfgs::kFwModelChunk;
			CHECK(s1.v[0] == s0.v[0] + 1 && s1.v[1] == s0.v[1] + n && s1.v[2] == s0.v[2] + chunks && s1.v[3] == s0.v[3] + chunks && s1.v[6] == vfgs::kFwModelChunk);
			CHECK(g_standin_launches == l0 + chunks);
			for (unsigned i = 0; i < n; i++)
			{
				int info[8];
				OK(vfgs_hip_model_info(models[i], info));
				const int arg = msgs[i].log2_scale_factor - (msgs[i].model_id ? 1 : 0);
				CHECK(info[0] == g[0] && info[1] == g[1] && info[2] == g[2] && info[5] == arg + 6 - (g[0] - 8) && info[6] == g[3]);
				if (i % 3 == 0) CHECK(info[3] == (g[0] != 8) && info[4] == (g[0] != 8));        // the hot messages: uniform everywhere, general at 8 bit only
				touch_image(models[i]);
			}
			list_call(models, g[0], g[1], g[2], s);
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
	const auto msgs = make_seis(n);
	for (int round = 0; round < 4; round++)
	{
		auto models = build(msgs, s);
		// partial, shuffled release: every other model goes, in a shuffled order; the others serve a launch on ANOTHER stream that is still
		// queued when they go too
		std::vector<unsigned> order;
		for (unsigned i = 0; i < n; i++) order.push_back(i);
		for (unsigned i = n - 1; i > 0; i--) std::swap(order[i], order[rnd() % (i + 1)]);
		std::vector<vfgs_hip_model*> keep;
		for (unsigned i : order)
			if (i & 1) vfgs_hip_model_release(models[i]);
			else keep.push_back(models[i]);
		for (unsigned i : order)
			if (i & 1) { int info[8]; CHECK(vfgs_hip_model_info(models[i], info) == 41); }
		Planes p((int)keep.size(), 264, 40, 10, 2, 2, false);
		std::vector<uint32_t> seeds(keep.size(), 77u);
		OK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), keep.data(), seeds.data(), (unsigned)keep.size(), 264, 40, p.stride, p.cstride, s2));
		for (vfgs_hip_model* m : keep) vfgs_hip_model_release(m);      // the launch is queued, not run
		vfgs_hip_model_release(keep[0]);                              // released before: no-op
		vfgs_hip_model_release(nullptr);
		// the next build takes the slabs that were just left -- after their readers -- or new ones; either way the queued launch reads live bytes
		auto again = build(msgs, s);
		for (vfgs_hip_model* m : again) touch_image(m);
		hipStreamSynchronize(s2);
		for (vfgs_hip_model* m : again) vfgs_hip_model_release(m);
	}
	// steady state: build / use / release, no allocation and no free after the first cycle
	uint64_t mark[2] = {0, 0};
	for (int cycle = 0; cycle < 4; cycle++)
	{
		auto models = build(make_seis(vfgs::kFwModelChunk), s);
		list_call(models, 10, 2, 2, s);
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
			const auto msgs = make_seis(7, true);
			auto models = build(msgs, s);
			list_call(models, depth, 2, sy, nullptr);            // (another stream than the build's: waits by event)
			const unsigned shift = depth == 8 ? 0 : 16 - depth;
			Planes p(7, 264, 40, depth, 2, sy, true);
			std::vector<uint32_t> seeds(7, 5u);
			OK(vfgs_hip_add_grain_sp_frame_list_models_dev(p.sp_list.data(), p.sp_list.data(), models.data(), seeds.data(), 7, 264, 40, p.stride, p.cstride, shift, s));
			OK(vfgs_hip_add_grain_sp_frame_list_models_dev(p.sp_list.data(), p.sp_list.data(), models.data(), nullptr, 7, 264, 40, p.stride, p.cstride, shift, s));
			hipStreamSynchronize(s);
			// inside an overlap region the build takes the region's stream
			OK(vfgs_hip_overlap_begin(s));
			auto more = build(msgs, s);
			OK(vfgs_hip_add_grain_sp_frame_list_models_dev(p.sp_list.data(), p.sp_list.data(), more.data(), seeds.data(), 7, 264, 40, p.stride, p.cstride, shift, s));
			OK(vfgs_hip_overlap_end(s));
			hipStreamSynchronize(s);
			for (vfgs_hip_model* m : more) { touch_image(m); vfgs_hip_model_release(m); }
			for (vfgs_hip_model* m : models) vfgs_hip_model_release(m);
		}
	hipStreamDestroy(s);
}

static void refused(std::vector<fgs_sei> msgs, unsigned at, int code, const char* what)
{
	std::vector<vfgs_hip_model*> out(msgs.size(), (vfgs_hip_model*)0x10);
	const Stats s0;
	const Regs r0;
	const uint64_t l0 = g_standin_launches;
	const int rc = vfgs_hip_models_from_sei(msgs.data(), (unsigned)msgs.size(), out.data(), nullptr);
	char idx[32];
	snprintf(idx, sizeof idx, "message %u:", at);
	if (rc != code || !strstr(vfgs_hip_last_error_string(), idx) || !strstr(vfgs_hip_last_error_string(), "vfgs_hip_models_from_sei"))
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
		auto base = make_seis(5);
		for (auto& m : base) { m.model_id = 0; m.log2_scale_factor = 5; for (int c = 0; c < 3; c++) m.comp_model_present_flag[c] = 1; }
		auto v = base; v[at].num_intensity_intervals[0] = 257; refused(v, at, 42, "257 luma intervals");
		v = base; v[at].num_intensity_intervals[1] = 300; refused(v, at, 42, "300 Cb intervals");
		v = base; v[at].num_intensity_intervals[2] = 65535; refused(v, at, 42, "65535 Cr intervals");
		v = base; v[at].model_id = 1; v[at].log2_scale_factor = 0; refused(v, at, 42, "AR, log2_scale_factor 0");
		v = base; v[at].model_id = 7; v[at].log2_scale_factor = 16; refused(v, at, 42, "AR, log2_scale_factor 16");
		v = base; v[at].log2_scale_factor = 1; refused(v, at, 9, "FF, log2_scale_factor 1");
		v = base; v[at].log2_scale_factor = 8; refused(v, at, 9, "FF, log2_scale_factor 8");
		v = base; v[at].model_id = 1; v[at].log2_scale_factor = 2; refused(v, at, 9, "AR, log2_scale_factor 2");
		v = base; v[at].model_id = 1; v[at].log2_scale_factor = 9; refused(v, at, 9, "AR, log2_scale_factor 9");
		// all messages are examined for 42 first, then for 9
		v = base; v[0].log2_scale_factor = 8; v[4].num_intensity_intervals[0] = 257; refused(v, 4, 42, "42 before 9");
		// not refused: too many intervals in a component that is absent, 256 intervals
		v = base; v[at].comp_model_present_flag[2] = 0; v[at].num_intensity_intervals[2] = 999; v[at].num_intensity_intervals[0] = 256;
		for (vfgs_hip_model* m : build(v, nullptr)) vfgs_hip_model_release(m);
	}
	const auto msgs = make_seis(2);
	vfgs_hip_model* out[2] = {(vfgs_hip_model*)0x10, (vfgs_hip_model*)0x10};
	const Stats s0;
	CHECK(vfgs_hip_models_from_sei(msgs.data(), 2, nullptr, nullptr) == 41);
	CHECK(vfgs_hip_models_from_sei(nullptr, 2, out, nullptr) == 41 && !out[0] && !out[1]);
	out[0] = out[1] = (vfgs_hip_model*)0x10;
	CHECK(vfgs_hip_models_from_sei(msgs.data(), 0, out, nullptr) == 0 && out[0] == (vfgs_hip_model*)0x10);      // n == 0: no call at all
	CHECK(vfgs_hip_models_from_sei(nullptr, 0, nullptr, nullptr) == 0);
	CHECK(Stats() == s0);
}

static void walk_shutdown_and_short_buffer()
{
	set_format(10, 2, 2);
	auto models = build(make_seis(vfgs::kFwModelChunk + 3), nullptr);
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
	auto again = build(make_seis(3, true), nullptr);
	for (vfgs_hip_model* m : again) { touch_image(m); vfgs_hip_model_release(m); }
	vfgs_hip_shutdown();
}

// the two builders take turns on the pool: a slab left by an AFGS1 build has a staging buffer too short for an SEI job table (the
// stand-ins read the whole table the host copied from it: too short a buffer is a heap overflow report), and the other way round it serves
static void walk_alternating_pool()
{
	hipStream_t s = nullptr;
	hipStreamCreateWithFlags(&s, 0);
	static_assert(sizeof(vfgs::FwSeiJob) > sizeof(vfgs::FwModelJob), "the walk is about the larger table meeting the smaller staging buffer");
	for (int depth : {8, 10})
	{
		set_format(depth, 2, 2);
		for (int round = 0; round < 6; round++)
		{
			std::vector<fgs_afgs1> sets;
			for (unsigned i = 0; i < (round & 1 ? 32u : 5u); i++) sets.push_back(make_afgs1());
			auto a = build_afgs1(sets, s);
			for (vfgs_hip_model* m : a) touch_image(m, 0x80);
			if (round % 3 != 2) for (vfgs_hip_model* m : a) vfgs_hip_model_release(m);      // an idle AFGS1 slab in front of the SEI build
			auto b = build(make_seis(round & 2 ? 32 : 9, true), s);
			for (vfgs_hip_model* m : b) touch_image(m);
			if (round % 3 == 2) { for (vfgs_hip_model* m : a) touch_image(m, 0x80); for (vfgs_hip_model* m : a) vfgs_hip_model_release(m); }
			std::vector<vfgs_hip_model*> both(b);
			list_call(both, depth, 2, 2, s);
			for (vfgs_hip_model* m : b) vfgs_hip_model_release(m);      // an idle SEI slab in front of the next AFGS1 build
		}
	}
	hipStreamDestroy(s);
}

static void walk_threads()
{
	set_format(10, 2, 2);
	const auto mine = make_seis(5);
	auto models = build(mine, nullptr);
	std::atomic<bool> stop{false};
	const fgs_afgs1 a = make_afgs1();
	auto builder = [&](uint32_t lcg, bool afgs1_too) {
		hipStream_t s = nullptr;
		hipStreamCreateWithFlags(&s, 0);
		while (!stop)
		{
			lcg = lcg_step(lcg);
			const unsigned n = 1 + (lcg >> 8) % 40;
			std::vector<vfgs_hip_model*> out(n);
			if (afgs1_too && (lcg >> 20 & 1))
			{
				std::vector<fgs_afgs1> sets(n, a);
				if (vfgs_hip_models_from_afgs1(sets.data(), n, out.data(), s)) { g_fail++; break; }
			}
			else
			{
				std::vector<fgs_sei> msgs(n, mine[(lcg >> 16) % 5]);
				if (vfgs_hip_models_from_sei(msgs.data(), n, out.data(), s)) { g_fail++; break; }
			}
			for (size_t i = out.size(); i-- > 0;) vfgs_hip_model_release(out[i]);
		}
		hipStreamDestroy(s);
	};
	std::thread t1(builder, 7u, false), t2(builder, 11u, true);
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
	t1.join();
	t2.join();
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
		{"alternating_pool", walk_alternating_pool},
		{"threads", walk_threads},
		{"shutdown_and_short_buffer", walk_shutdown_and_short_buffer},
	});
}
