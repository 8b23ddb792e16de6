// TEST INFRASTRUCTURE.  Models that carry a chroma mix (include/vfgs_hip_fw.h: vfgs_hip_models_from_afgs1_mix; include/vfgs_hip.h:
// vfgs_hip_model_capture_mix, vfgs_hip_model_chroma_mix, the two list calls with a model per picture) in the host layer of libvfgs_hip,
// compiled with a sanitizer over the unchanged tests/sanitize/hip_stub.cpp, as tests/sanitize_model_build/model_build_walks.cpp drives the
// models without one: the three entry points with their C types, the host side of the record (what the job table hands the kernel, what the
// read-back and vfgs_hip_model_chroma_mix return), the splitting of a list into runs with the kernel each run is given, and every refusal
// with nothing changed.  The stand-in for vfgs::launch_fw_models below writes what the kernel writes: the job's 32-byte record and the
// image_layout() bytes behind it.  Values are the GPU suite's business (tests/test_gpu_model_list_mix.py).
//
// The model of the HIP runtime is compiled INTO this translation unit, unchanged, with its launcher of the grain kernels under another
// name: vfgs::launch_grain below stands where vfgs_kernel.hip's does, holds every launch to the agreement that one holds it to -- the key's
// family against KernelArgs::models_kernel / mix_kernel / sp_kernel through family_fields(), a model per frame never with a narrowed
// destination or rows walked in parts -- records what it was handed, and passes the launch on to the model.
//
// usage: model_mix_walks [walk ...]     (no argument: all of them)
#define launch_grain stub_launch_grain
#include "../sanitize/hip_stub.cpp"
#undef launch_grain

#include <hip/hip_runtime.h>

#include <type_traits>

#define WALKS_SEED 17
#define WALKS_HAVE_HIP_RUNTIME_H
#include "../sanitize/walks.h"
#include "../../versatilefilmgrain_amd/csrc/vfgs_model_build.h"

using Planes = BarePlanes;

static std::atomic<uint64_t> g_standin_launches{0};

namespace vfgs {
hipError_t launch_fw_models(const FwConstants* k, const FwModelJob* jobs, int n, int csubx, int csuby, int depth8, hipStream_t stream)
{
	if (n <= 0 || n > kFwModelChunk || !k || !jobs) return hipErrorInvalidValue;
	(void)hipStreamSynchronize(stream);      // the job table's copy has run
	for (int i = 0; i < n; i++)
	{
		const FwModelJob j = jobs[i];
		const ImageLayout L = image_layout(csubx, csuby, j.one_y != 0, j.one_c != 0, depth8 != 0);
		// (a job that carries a mix says so in its record, and only then)
		if (((uintptr_t)j.dst & 15) || (j.mix_carried != 0) != ((j.rec.mix_flags & 1u) != 0) || (!j.mix_carried && (j.rec.mix[0] | j.rec.mix[1])))
		{
			fprintf(stderr, "FAILED stand-in: job %d of %d is not what the kernel may be given\n", i, n);
			g_fail++;
			return hipErrorInvalidValue;
		}
		memcpy(j.dst, &j.rec, kModelRecordBytes);
		memset(j.dst + kModelRecordBytes, 0x40 + (i & 31), (size_t)L.bytes);
	}
	g_standin_launches++;
	return hipSuccess;
}
}  // namespace vfgs

// what the launcher was handed: the last launch, and how many launches of each kind
struct Handed { vfgs::Family family; int models_kernel, mix_kernel, sp_kernel, listed, nframes; bool out8, wide; };
static Handed g_handed;
static std::atomic<uint64_t> g_mix_with_models{0}, g_mix_programmed{0}, g_without_mix{0};

namespace vfgs {
hipError_t launch_grain(const KernelArgs& a, const FrameTable* list, const KernelKey& k, int grid, hipStream_t stream)
{
	const bool mixf = k.family == Family::mix || k.family == Family::sp_mix, mix_models = mixf && a.models_kernel != 0;
	const FamilyFields ff = family_fields(k.family, mix_models);
	bool ok = a.models_kernel == ff.models_kernel && a.mix_kernel == ff.mix_kernel && a.sp_kernel == ff.sp_kernel && !(mix_models && (k.out8 || k.wide));
	if (mixf) ok = ok && kernel_exists(k);
	if (a.models_kernel)      // a model per frame: listed frames, every frame with a model image
	{
		ok = ok && list && a.listed == 1;
		for (int i = 0; ok && i < a.nframes; i++) ok = list->model[i] && !((uintptr_t)list->model[i] & 15);
	}
	if (!ok)
	{
		fprintf(stderr, "FAILED launcher: family %d with models_kernel %d, mix_kernel %d, sp_kernel %d, out8 %d, wide %d is not a launch the real launcher takes\n",
		        (int)k.family, a.models_kernel, a.mix_kernel, a.sp_kernel, (int)k.out8, (int)k.wide);
		g_fail++;
		return hipErrorInvalidValue;
	}
	g_handed = Handed{k.family, a.models_kernel, a.mix_kernel, a.sp_kernel, a.listed, a.nframes, k.out8, k.wide};
	(mix_models ? g_mix_with_models : mixf ? g_mix_programmed : g_without_mix)++;
	return stub_launch_grain(a, list, k, grid, stream);
}
}  // namespace vfgs

static bool handed(vfgs::Family f, int models_kernel, int mix_kernel)
{
	return g_handed.family == f && g_handed.models_kernel == models_kernel && g_handed.mix_kernel == mix_kernel && g_handed.listed == 1 && !g_handed.out8 && !g_handed.wide;
}

// the three entry points exist with these C types
static_assert(std::is_same<decltype(&vfgs_hip_models_from_afgs1_mix), int (*)(const fgs_afgs1*, unsigned, vfgs_hip_model**, void*)>::value, "vfgs_hip_models_from_afgs1_mix");
static_assert(std::is_same<decltype(&vfgs_hip_model_capture_mix), int (*)(vfgs_hip_model**, void*)>::value, "vfgs_hip_model_capture_mix");
static_assert(std::is_same<decltype(&vfgs_hip_model_chroma_mix), int (*)(const vfgs_hip_model*, int, int*)>::value, "vfgs_hip_model_chroma_mix");
static_assert(sizeof(vfgs::ModelRecord) == 32 && offsetof(vfgs::ModelRecord, mix_flags) == 20 && offsetof(vfgs::ModelRecord, mix) == 24, "the record's mix words");
static_assert(sizeof(vfgs::KernelArgs) == 312 && offsetof(vfgs::FrameTable, model) == 6 * 8 * vfgs::kListFrames, "what the kernels of before load has not moved");

// a valid parameter set whose image is all-one-pattern at every depth; the mix fields as given
static fgs_afgs1 make_set(int cb_mult, int cb_luma, int cb_off, int cr_mult, int cr_luma, int cr_off, bool cfl = false, bool hot = false)
{
	fgs_afgs1 a;
	memset(&a, 0, sizeof a);
	a.grain_seed = (uint16_t)rnd();
	a.num_y_points = 3;
	for (int k = 0; k < 3; k++) { a.point_y_values[k] = (uint8_t)(k * 60 + 10); a.point_y_scaling[k] = (uint8_t)(40 + rnd() % 60); }
	if (hot) a.point_y_scaling[1] = 255;
	a.num_cb_points = a.num_cr_points = 2;
	for (int k = 0; k < 2; k++) { a.point_cb_values[k] = a.point_cr_values[k] = (uint8_t)(k * 100 + 20); a.point_cb_scaling[k] = a.point_cr_scaling[k] = (uint8_t)(30 + rnd() % 50); }
	a.chroma_scaling_from_luma = cfl;
	a.grain_scaling = hot ? 11 : 9;
	a.ar_coeff_lag = 2;
	for (int k = 0; k < 24; k++) a.ar_coeffs_y[k] = (int16_t)((int)(rnd() % 64) - 32);
	for (int k = 0; k < 25; k++) a.ar_coeffs_cb[k] = a.ar_coeffs_cr[k] = (int16_t)((int)(rnd() % 64) - 32);
	a.ar_coeff_shift = 7;
	a.cb_mult = (uint8_t)cb_mult; a.cb_luma_mult = (uint8_t)cb_luma; a.cb_offset = (uint16_t)cb_off;
	a.cr_mult = (uint8_t)cr_mult; a.cr_luma_mult = (uint8_t)cr_luma; a.cr_offset = (uint16_t)cr_off;
	return a;
}

struct Snapshot {      // what no call here may change
	int mix[2][4];
	uint32_t regs[4];
	int params[8];
	Snapshot()
	{
		vfgs_hip_get_chroma_mix(1, mix[0]); vfgs_hip_get_chroma_mix(2, mix[1]);
		vfgs_hip_get_seed_state(regs);
		vfgs_hip_get_params(params);
	}
	bool same_but_regs(const Snapshot& o) const { return !memcmp(mix, o.mix, sizeof mix) && !memcmp(params, o.params, sizeof params); }
	bool operator==(const Snapshot& o) const { return same_but_regs(o) && !memcmp(regs, o.regs, sizeof regs); }
};

static std::vector<uint8_t> image_of(const vfgs_hip_model* m)
{
	int info[8];
	OK(vfgs_hip_model_info(m, info));
	std::vector<uint8_t> b((size_t)info[7]);
	size_t bytes = 0;
	OK(vfgs_hip_model_image(m, b.data(), b.size(), &bytes));
	CHECK(bytes == b.size());
	return b;
}

static bool mix_is(const vfgs_hip_model* m, int c, int lm, int cm, int off, int active)
{
	int v[4] = {9, 9, 9, 9};
	OK(vfgs_hip_model_chroma_mix(m, c, v));
	return v[0] == lm && v[1] == cm && v[2] == off && v[3] == active;
}

static bool last_kernel_begins(const char* name)
{
	vfgs_hip_launch_info li;
	return !vfgs_hip_last_launch_info(&li) && !strncmp(li.kernel, name, strlen(name)) && li.listed == 1;
}

// ---- walks ----------------------------------------------------------------------------------------------------------------------------

// the record: what the job table hands the kernel comes back through the read-back and through vfgs_hip_model_chroma_mix, at 8 and 10 bit
static void walk_record()
{
	for (int depth : {8, 10})
	{
		set_format(depth, 2, 2);
		vfgs_hip_set_chroma_mix(2, 5, 6, 7);      // a programmed mix and the switch: neither is looked at, neither changes
		vfgs_hip_afgs1_chroma_mix(0);
		const std::vector<fgs_afgs1> sets = {make_set(247, 192, 18, 229, 182, 54), make_set(128, 192, 256, 128, 192, 256), make_set(1, 2, 3, 4, 5, 6, true),
		                                     make_set(0, 255, 511, 255, 0, 0)};
		std::vector<vfgs_hip_model*> m(sets.size()), p(sets.size());
		const Snapshot s0;
		OK(vfgs_hip_models_from_afgs1_mix(sets.data(), (unsigned)sets.size(), m.data(), nullptr));
		OK(vfgs_hip_models_from_afgs1(sets.data(), (unsigned)sets.size(), p.data(), nullptr));
		CHECK(Snapshot() == s0);
		CHECK(mix_is(m[0], 1, 64, 119, -238, 1) && mix_is(m[0], 2, 54, 101, -202, 1));
		CHECK(mix_is(m[1], 1, 64, 0, 0, 1) && mix_is(m[1], 2, 64, 0, 0, 1));
		CHECK(mix_is(m[2], 1, 64, 0, 0, 1) && mix_is(m[2], 2, 64, 0, 0, 1));      // chroma_scaling_from_luma
		CHECK(mix_is(m[3], 1, 127, -128, 255, 1) && mix_is(m[3], 2, -128, 127, -256, 1));      // the ends of every field
		const int bs = depth - 8;
		for (size_t i = 0; i < sets.size(); i++)
		{
			const std::vector<uint8_t> a = image_of(m[i]), b = image_of(p[i]);
			vfgs::ModelRecord ra, rb;
			memcpy(&ra, a.data(), sizeof ra); memcpy(&rb, b.data(), sizeof rb);
			CHECK(a.size() == b.size() && !memcmp(a.data(), b.data(), 20));
			CHECK(rb.mix_flags == 0 && rb.mix[0] == 0 && rb.mix[1] == 0 && mix_is(p[i], 1, 0, 0, 0, 0) && mix_is(p[i], 2, 0, 0, 0, 0));
			CHECK(ra.mix_flags == 1);
			for (int c = 0; c < 2; c++)
			{
				int v[4];
				OK(vfgs_hip_model_chroma_mix(m[i], c + 1, v));
				CHECK(ra.mix[c] == vfgs::model_mix_word(v[0], v[1], v[2] * (1 << bs), v[3]));
				CHECK(vfgs::model_mix_luma_mult(ra.mix[c]) == v[0] && vfgs::model_mix_chroma_mult(ra.mix[c]) == v[1] && vfgs::model_mix_offset(ra.mix[c]) == v[2] * (1 << bs) && vfgs::model_mix_active(ra.mix[c]) == 1);
			}
		}
		// capture: drops the mix; capture_mix: carries the one that is active now, per component
		vfgs_hip_model *c0 = nullptr, *c1 = nullptr, *c2 = nullptr;
		unsigned char lut[256];
		memset(lut, 0, sizeof lut);
		for (int c = 0; c < 3; c++) { vfgs_set_pattern_lut(c, lut); vfgs_set_scale_lut(c, lut); }
		const Snapshot s1;
		OK(vfgs_hip_model_capture(&c0, nullptr));
		OK(vfgs_hip_model_capture_mix(&c1, nullptr));
		CHECK(Snapshot() == s1);
		CHECK(mix_is(c0, 1, 0, 0, 0, 0) && mix_is(c0, 2, 0, 0, 0, 0) && mix_is(c1, 1, 0, 0, 0, 0) && mix_is(c1, 2, 5, 6, 7, 1));
		vfgs_hip_clear_chroma_mix();
		OK(vfgs_hip_model_capture_mix(&c2, nullptr));
		CHECK(image_of(c2) == image_of(c0) && image_of(c1) != image_of(c0));
		int v[4];
		CHECK(vfgs_hip_model_chroma_mix(c1, 0, v) == 37 && vfgs_hip_model_chroma_mix(c1, 3, v) == 37 && vfgs_hip_model_chroma_mix(nullptr, 1, v) == 41);
		vfgs_hip_model_release(c1);
		CHECK(vfgs_hip_model_chroma_mix(c1, 1, v) == 41);
		vfgs_hip_model_release(c0); vfgs_hip_model_release(c2);
		for (vfgs_hip_model* x : m) vfgs_hip_model_release(x);
		for (vfgs_hip_model* x : p) vfgs_hip_model_release(x);
	}
}

// runs: at most 32 consecutive frames whose models share (one_y, one_c, carries a mix); the kernel of each run; in place under a mix: two launches
static void walk_runs()
{
	hipStream_t s = nullptr;
	hipStreamCreateWithFlags(&s, 0);
	for (int depth : {8, 10})
		for (int sy : {2, 1})
		{
			set_format(depth, 2, sy);
			const std::vector<fgs_afgs1> sets = {make_set(247, 192, 18, 229, 182, 54), make_set(128, 192, 256, 128, 192, 256)};
			vfgs_hip_model *mm[2], *pl[1];
			OK(vfgs_hip_models_from_afgs1_mix(sets.data(), 2, mm, s));
			OK(vfgs_hip_models_from_afgs1(sets.data(), 1, pl, s));
			const vfgs_hip_model* abacb[5] = {mm[0], mm[1], mm[0], pl[0], mm[1]};
			const uint32_t seeds[5] = {1, 2, 3, 4, 5};
			const unsigned shift = depth == 8 ? 0 : 6;
			for (int in_place = 0; in_place < 2; in_place++)
			{
				Planes src(5, 264, 40, depth, 2, sy, false), dst(5, 264, 40, depth, 2, sy, false);
				const Snapshot s0;
				unsigned long long n0 = launches();
				uint64_t m0 = g_mix_with_models, p0 = g_mix_programmed, w0 = g_without_mix;
				OK(vfgs_hip_add_grain_frame_list_models_dev(src.list.data(), in_place ? src.list.data() : dst.list.data(), abacb, seeds, 5, 264, 40, src.stride, src.cstride, s));
				CHECK(launches() - n0 == (in_place ? 5u : 3u));      // [A B A] [C] [B]: a run under a mix over shared luma bytes is two launches
				CHECK(last_kernel_begins("grain_mix_kernel<") && Snapshot().same_but_regs(s0));
				// the launcher was handed the key of the mix family WITH models_kernel set for the runs with a mix, grain_ml_kernel's for [C]
				CHECK(handed(vfgs::Family::mix, 1, 1) && g_handed.sp_kernel == 0 && g_handed.nframes == 1);
				CHECK(g_mix_with_models - m0 == (in_place ? 4u : 2u) && g_mix_programmed == p0 && g_without_mix - w0 == 1);
				Planes ssp(5, 264, 40, depth, 2, sy, true), dsp(5, 264, 40, depth, 2, sy, true);
				n0 = launches();
				m0 = g_mix_with_models; w0 = g_without_mix;
				OK(vfgs_hip_add_grain_sp_frame_list_models_dev(ssp.sp_list.data(), in_place ? ssp.sp_list.data() : dsp.sp_list.data(), abacb, nullptr, 5, 264, 40, ssp.stride, ssp.cstride, shift, s));
				CHECK(launches() - n0 == (in_place ? 5u : 3u));
				CHECK(last_kernel_begins("grain_sp_mix_kernel<") && Snapshot().same_but_regs(s0));
				CHECK(handed(vfgs::Family::sp_mix, 1, 1) && g_handed.sp_kernel == 1 && g_handed.nframes == 1);
				CHECK(g_mix_with_models - m0 == (in_place ? 4u : 2u) && g_mix_programmed == p0 && g_without_mix - w0 == 1);
				// the run without a mix keeps its kernels
				n0 = launches();
				OK(vfgs_hip_add_grain_frame_list_models_dev(src.list.data(), src.list.data(), abacb + 3, seeds, 1, 264, 40, src.stride, src.cstride, s));
				CHECK(launches() - n0 == 1 && last_kernel_begins("grain_ml_kernel<") && handed(vfgs::Family::ml, 1, 0));
				OK(vfgs_hip_add_grain_sp_frame_list_models_dev(ssp.sp_list.data(), ssp.sp_list.data(), abacb + 3, nullptr, 1, 264, 40, ssp.stride, ssp.cstride, shift, s));
				CHECK(last_kernel_begins("grain_spml_kernel<") && handed(vfgs::Family::spml, 1, 0));
				hipStreamSynchronize(s);
			}
			// 34 frames, the values of the mix alternating: 32 + 2
			{
				Planes src(34, 136, 32, depth, 2, sy, false), dst(34, 136, 32, depth, 2, sy, false);
				std::vector<const vfgs_hip_model*> ms;
				std::vector<uint32_t> sd;
				for (int i = 0; i < 34; i++) { ms.push_back(mm[i & 1]); sd.push_back(100u + i); }
				const unsigned long long n0 = launches();
				OK(vfgs_hip_add_grain_frame_list_models_dev(src.list.data(), dst.list.data(), ms.data(), sd.data(), 34, 136, 32, src.stride, src.cstride, s));
				vfgs_hip_launch_info li;
				CHECK(launches() - n0 == 2 && !vfgs_hip_last_launch_info(&li) && li.nframes == 2);
				hipStreamSynchronize(s);
			}
			vfgs_hip_model_release(mm[0]); vfgs_hip_model_release(mm[1]); vfgs_hip_model_release(pl[0]);
		}
	hipStreamDestroy(s);
}

static void refused_build(std::vector<fgs_afgs1> sets, unsigned at, int code)
{
	std::vector<vfgs_hip_model*> out(sets.size(), (vfgs_hip_model*)0x10);
	const Snapshot s0;
	uint64_t st0[8], st1[8];
	vfgs_hip_get_model_build_stats(st0);
	const uint64_t l0 = g_standin_launches;
	const int rc = vfgs_hip_models_from_afgs1_mix(sets.data(), (unsigned)sets.size(), out.data(), nullptr);
	char idx[32];
	snprintf(idx, sizeof idx, "parameter set %u:", at);
	if (rc != code || !strstr(vfgs_hip_last_error_string(), idx))
	{
		fprintf(stderr, "FAILED refusal at %u: %d (%s), expected %d\n", at, rc, vfgs_hip_last_error_string(), code);
		g_fail++;
	}
	for (vfgs_hip_model* m : out) CHECK(m == nullptr);
	vfgs_hip_get_model_build_stats(st1);
	CHECK(Snapshot() == s0 && !memcmp(st0, st1, sizeof st0) && g_standin_launches == l0);
}

static void walk_refusals()
{
	const fgs_afgs1 good = make_set(247, 192, 18, 229, 182, 54);
	// 42: a mix field the setter would refuse, and everything vfgs_hip_models_from_afgs1 refuses; 9 as there
	set_format(10, 2, 2);
	for (unsigned at : {0u, 2u})
	{
		std::vector<fgs_afgs1> v(3, good);
		v[at].cb_offset = 512; refused_build(v, at, 42);
		v.assign(3, good); v[at].cr_offset = 65535; refused_build(v, at, 42);
		v.assign(3, good); v[at].ar_coeff_lag = 0; refused_build(v, at, 42);
		v.assign(3, good); v[at].grain_scaling = 14; refused_build(v, at, 9);
		// (not refused: the same offset with chroma_scaling_from_luma, which does not look at it)
		v.assign(3, good); v[at].cb_offset = 512; v[at].chroma_scaling_from_luma = 1;
		std::vector<vfgs_hip_model*> out(3);
		OK(vfgs_hip_models_from_afgs1_mix(v.data(), 3, out.data(), nullptr));
		for (vfgs_hip_model* m : out) vfgs_hip_model_release(m);
	}
	vfgs_hip_model* out2[2] = {(vfgs_hip_model*)0x10, (vfgs_hip_model*)0x10};
	CHECK(vfgs_hip_models_from_afgs1_mix(&good, 1, nullptr, nullptr) == 41 && vfgs_hip_models_from_afgs1_mix(nullptr, 2, out2, nullptr) == 41 && !out2[0] && !out2[1]);
	CHECK(vfgs_hip_models_from_afgs1_mix(nullptr, 0, nullptr, nullptr) == 0);
	// 38: depth 12; an 8-bit set that falls back to the general form
	set_format(12, 2, 2);
	refused_build(std::vector<fgs_afgs1>(2, good), 0, 38);
	set_format(8, 2, 2);
	{
		std::vector<fgs_afgs1> v(3, good);
		v[1] = make_set(247, 192, 18, 229, 182, 54, false, true);
		refused_build(v, 1, 38);
		vfgs_hip_model* m = nullptr;
		OK(vfgs_hip_models_from_afgs1(&v[1], 1, &m, nullptr));      // (without a mix the general form is served)
		int info[8];
		OK(vfgs_hip_model_info(m, info));
		CHECK(info[3] == 0);
		vfgs_hip_model_release(m);
	}
	// capture_mix: 38 at depth 12 and for a general-form bank, under an active mix only; capture is unchanged
	unsigned char lut[256];
	memset(lut, 0, sizeof lut);
	for (int general = 0; general < 2; general++)
	{
		set_format(general ? 10 : 12, 2, 2);
		for (int c = 0; c < 3; c++) { vfgs_set_scale_lut(c, lut); vfgs_set_pattern_lut(c, lut); }
		if (general)
		{
			unsigned char two[256];
			for (int i = 0; i < 256; i++) two[i] = (unsigned char)((i & 1) << 4);      // two slots: no one-pattern form
			vfgs_set_pattern_lut(0, two);
		}
		vfgs_hip_model *m = (vfgs_hip_model*)0x10, *n = nullptr;
		OK(vfgs_hip_model_capture_mix(&m, nullptr));      // no mix active: capture's result
		vfgs_hip_model_release(m);
		vfgs_hip_set_chroma_mix(1, 10, 20, 30);
		const Snapshot s0;
		m = (vfgs_hip_model*)0x10;
		CHECK(vfgs_hip_model_capture_mix(&m, nullptr) == 38 && m == nullptr && Snapshot() == s0);
		OK(vfgs_hip_model_capture(&n, nullptr));
		vfgs_hip_model_release(n);
	}
	CHECK(vfgs_hip_model_capture_mix(nullptr, nullptr) == 41);
	// the list calls: a PROGRAMMED mix is refused with 41 as before, and so is a model (with a mix) of another depth or chroma format
	set_format(10, 2, 2);
	vfgs_hip_model* m = nullptr;
	OK(vfgs_hip_models_from_afgs1_mix(&good, 1, &m, nullptr));
	const vfgs_hip_model* ms[1] = {m};
	Planes p(1, 264, 40, 10, 2, 2, false), q(1, 264, 40, 10, 2, 2, true);
	vfgs_hip_set_chroma_mix(1, 1, 2, 3);
	const unsigned long long n0 = launches();
	CHECK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), ms, nullptr, 1, 264, 40, p.stride, p.cstride, nullptr) == 41);
	CHECK(vfgs_hip_add_grain_sp_frame_list_models_dev(q.sp_list.data(), q.sp_list.data(), ms, nullptr, 1, 264, 40, q.stride, q.cstride, 6, nullptr) == 41);
	vfgs_hip_clear_chroma_mix();
	vfgs_set_depth(8);
	CHECK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), ms, nullptr, 1, 264, 40, p.stride, p.cstride, nullptr) == 41);
	vfgs_set_depth(10);
	vfgs_set_chroma_subsampling(2, 1);      // ... and of another chroma format
	CHECK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), ms, nullptr, 1, 264, 40, p.stride, p.cstride, nullptr) == 41);
	CHECK(vfgs_hip_add_grain_sp_frame_list_models_dev(q.sp_list.data(), q.sp_list.data(), ms, nullptr, 1, 264, 40, q.stride, q.cstride, 6, nullptr) == 41);
	vfgs_set_chroma_subsampling(2, 2);
	CHECK(launches() == n0);
	OK(vfgs_hip_add_grain_frame_list_models_dev(p.list.data(), p.list.data(), ms, nullptr, 1, 264, 40, p.stride, p.cstride, nullptr));
	hipStreamSynchronize(nullptr);
	vfgs_hip_model_release(m);
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"record", walk_record},
		{"runs", walk_runs},
		{"refusals", walk_refusals},
	});
}
