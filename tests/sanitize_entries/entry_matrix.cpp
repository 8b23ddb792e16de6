// TEST INFRASTRUCTURE.  A characterisation of the device-pointer entries of libvfgs_hip (include/vfgs_hip.h: every vfgs_hip_add_grain_*_dev)
// as the host layer answers them over tests/sanitize/hip_stub.cpp: one text line per call -- entry, case, return code, last error code and
// text, the launch record of an accepted call that launched, the four seed registers and the [3] flag of the stripe- and seeded-stream statistics behind
// EVERY call (a refused call changes nothing: its line shows the registers of the line before it, or of a fresh vfgs_set_seed(4711)).
// tests/test_entry_matrix_cpu.py compares the output byte for byte with tests/golden/entry_matrix.txt, which was recorded once and is not
// regenerated when the host layer is reshaped: return codes, texts, which of two refusals wins, the launch record and the registers stay.
//
// The output holds no pointers, addresses or times.  A HIP error's text carries the expression and source line that met it
// ("expr -> text (file:line)"); of such a text only the runtime's part is printed.  The stub knows fewer kernels than the launcher (no
// narrowed destination and no persistent workgroups at 12 bit): such a call is recorded with the stub's refusal, registers moved and all.
// Values are the GPU suite's business; addresses are the sanitizer walks' (planes here are allocated generously).
#define WALKS_SEED 7
#include "../sanitize/walks.h"

static vfgs_hip_model* capture()
{
	vfgs_hip_model* m = nullptr;
	if (vfgs_hip_model_capture(&m, nullptr) || !m) printf("CAPTURE FAILED: %s\n", vfgs_hip_last_error_string());
	return m;
}

// n frames of three planes at one frame pitch, every plane with room for `rows` rows of `stride` 16-bit containers (a UV plane is "U")
struct Set {
	uint8_t* p[3];
	uint64_t pitch;
	std::vector<vfgs_hip_frame_ptrs> list;
	Set(unsigned n, unsigned stride, unsigned rows) : pitch((uint64_t)rows * stride * 2)
	{
		for (auto& q : p) hipMalloc((void**)&q, (size_t)(n * pitch));
		for (unsigned f = 0; f < n; f++) list.push_back({p[0] + f * pitch, p[1] + f * pitch, p[2] + f * pitch});
	}
	~Set() { for (auto* q : p) hipFree(q); }
	Set(const Set&) = delete;
};

enum Entry { STRIPE, FRAME, FRAME_PART, FRAMES, FRAMES_PART, COPY, COPY8, LIST, LIST_PART, LIST_COPY, LIST_COPY8, SEEDED, SEEDED_PART, SEEDED_COPY,
             SEEDED_COPY8, MODELS, SP, SP_MODELS, SP_COPY8, TO_SP, TO_SP8, NENTRIES };
static const char* const kNames[NENTRIES] = {"stripe", "frame", "frame_part", "frames", "frames_part", "copy", "copy8", "frame_list", "frame_list_part",
                                             "frame_list_copy", "frame_list_copy8", "frame_list_seeded", "frame_list_seeded_part", "frame_list_seeded_copy",
                                             "frame_list_seeded_copy8", "frame_list_models", "sp_frame_list", "sp_frame_list_models", "sp_frame_list_copy8",
                                             "frame_list_to_sp", "frame_list_to_sp8"};
static bool takes_dst(Entry e) { return e == COPY || e == COPY8 || e == LIST_COPY || e == LIST_COPY8 || e == SEEDED_COPY || e == SEEDED_COPY8 || e >= MODELS; }
static bool is_list(Entry e) { return e >= LIST; }
static bool narrows(Entry e) { return e == COPY8 || e == LIST_COPY8 || e == SEEDED_COPY8 || e == SP_COPY8 || e == TO_SP8; }
static bool must_copy(Entry e) { return e == SP_COPY8 || e == TO_SP || e == TO_SP8; }
static bool semiplanar(Entry e) { return e >= SP; }

struct Args {
	unsigned n = 2, w = 0, h = 0, py = 0, ph = 0, stride = 0, cstride = 0, dstride = 0, dcstride = 0, shift = 0;
	uint64_t yp = 0, cp = 0, dyp = 0, dcp = 0;
	std::vector<vfgs_hip_frame_ptrs> src, dst;
	bool copy = false, null_src = false, null_dst = false;
	std::vector<uint32_t> seeds;                 // (empty: none)
	std::vector<const vfgs_hip_model*> models;
	bool null_models = false;
	void* stream = nullptr;
};

static int call(Entry e, const Args& a)
{
	const bool copy = a.copy && takes_dst(e);
	const vfgs_hip_frame_ptrs* S = a.null_src ? nullptr : a.src.data();
	const vfgs_hip_frame_ptrs* D = a.null_dst ? nullptr : (copy ? a.dst.data() : S);
	const vfgs_hip_frame_ptrs s0 = a.src[0], d0 = copy ? a.dst[0] : a.src[0];
	const uint32_t* seeds = a.seeds.empty() ? nullptr : a.seeds.data();
	const vfgs_hip_model* const* ms = a.null_models ? nullptr : a.models.data();
	std::vector<vfgs_hip_sp_frame> ss, sd;
	for (unsigned f = 0; f < a.src.size(); f++) ss.push_back({a.src[f].Y, a.src[f].U});
	for (unsigned f = 0; f < a.dst.size(); f++) sd.push_back({a.dst[f].Y, a.dst[f].U});
	const vfgs_hip_sp_frame* SS = a.null_src ? nullptr : ss.data();
	const vfgs_hip_sp_frame* SD = a.null_dst ? nullptr : (copy ? sd.data() : SS);
	switch (e)
	{
	case STRIPE: return vfgs_hip_add_grain_stripe_dev(s0.Y, s0.U, s0.V, a.py, a.w, a.ph, a.stride, a.cstride, a.stream);
	case FRAME: return vfgs_hip_add_grain_frame_dev(s0.Y, s0.U, s0.V, a.w, a.h, a.stride, a.cstride, a.stream);
	case FRAME_PART: return vfgs_hip_add_grain_frame_part_dev(s0.Y, s0.U, s0.V, a.w, a.h, a.py, a.ph, a.stride, a.cstride, a.stream);
	case FRAMES: return vfgs_hip_add_grain_frames_dev(s0.Y, s0.U, s0.V, a.w, a.h, a.stride, a.cstride, a.n, a.yp, a.cp, a.stream);
	case FRAMES_PART: return vfgs_hip_add_grain_frames_part_dev(s0.Y, s0.U, s0.V, a.w, a.h, a.py, a.ph, a.stride, a.cstride, a.n, a.yp, a.cp, a.stream);
	case COPY: return vfgs_hip_add_grain_copy_dev(s0.Y, s0.U, s0.V, d0.Y, d0.U, d0.V, a.w, a.h, a.py, a.ph, a.stride, a.cstride, a.n, a.yp, a.cp, a.stream);
	case COPY8:
		return vfgs_hip_add_grain_copy8_dev(s0.Y, s0.U, s0.V, d0.Y, d0.U, d0.V, a.w, a.h, a.py, a.ph, a.stride, a.cstride, a.dstride, a.dcstride, a.n, a.yp, a.cp, a.dyp,
		                                    a.dcp, a.stream);
	case LIST: return vfgs_hip_add_grain_frame_list_dev(S, a.n, a.w, a.h, a.stride, a.cstride, a.stream);
	case LIST_PART: return vfgs_hip_add_grain_frame_list_part_dev(S, a.n, a.w, a.h, a.py, a.ph, a.stride, a.cstride, a.stream);
	case LIST_COPY: return vfgs_hip_add_grain_frame_list_copy_dev(S, D, a.n, a.w, a.h, a.stride, a.cstride, a.stream);
	case LIST_COPY8: return vfgs_hip_add_grain_frame_list_copy8_dev(S, D, a.n, a.w, a.h, a.stride, a.cstride, a.dstride, a.dcstride, a.stream);
	case SEEDED: return vfgs_hip_add_grain_frame_list_seeded_dev(S, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.stream);
	case SEEDED_PART: return vfgs_hip_add_grain_frame_list_seeded_part_dev(S, seeds, a.n, a.w, a.h, a.py, a.ph, a.stride, a.cstride, a.stream);
	case SEEDED_COPY: return vfgs_hip_add_grain_frame_list_seeded_copy_dev(S, D, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.stream);
	case SEEDED_COPY8: return vfgs_hip_add_grain_frame_list_seeded_copy8_dev(S, D, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.dstride, a.dcstride, a.stream);
	case MODELS: return vfgs_hip_add_grain_frame_list_models_dev(S, D, ms, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.stream);
	case SP: return vfgs_hip_add_grain_sp_frame_list_dev(SS, SD, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.shift, a.stream);
	case SP_MODELS: return vfgs_hip_add_grain_sp_frame_list_models_dev(SS, SD, ms, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.shift, a.stream);
	case SP_COPY8: return vfgs_hip_add_grain_sp_frame_list_copy8_dev(SS, SD, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.dstride, a.dcstride, a.shift, a.stream);
	case TO_SP: return vfgs_hip_add_grain_frame_list_to_sp_dev(S, SD, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.dstride, a.dcstride, a.shift, a.stream);
	case TO_SP8: return vfgs_hip_add_grain_frame_list_to_sp8_dev(S, SD, seeds, a.n, a.w, a.h, a.stride, a.cstride, a.dstride, a.dcstride, a.stream);
	default: return -1;
	}
}

static void report(Entry e, const std::string& label, int rc)
{
	std::string msg = rc ? vfgs_hip_last_error_string() : "";
	if (msg.find(".cpp:") != std::string::npos)      // a HIP error: "expr -> text (file:line)"
	{
		const size_t a = msg.find(" -> "), b = msg.rfind(" (");
		msg = "hip: " + msg.substr(a + 4, b - a - 4);
	}
	printf("%s | %s | rc=%d err=%d \"%s\"", kNames[e], label.c_str(), rc, rc ? vfgs_hip_last_error() : 0, msg.c_str());
	static unsigned long long launches = 0;
	vfgs_hip_launch_info li;
	if (rc == 0 && (vfgs_hip_last_launch_info(&li) != 0 || li.launches == launches)) printf(" | no launch");
	else if (rc == 0 && (launches = li.launches))
		printf(" | %s depth=%d %d,%d out8=%d one=%d,%d in_place=%d nframes=%d wgs=%d fronts=%d rpw=%d,%d pos=%d,%d parts=%d persist=%d waves=%d lds=%d launches=%llu "
		       "listed=%d internal=%d",
		       li.kernel, li.depth, li.csubx, li.csuby, li.out8, li.one_y, li.one_c, li.in_place, li.nframes, li.workgroups_per_frame, li.frames_per_front, li.rows_per_wave[0],
		       li.rows_per_wave[1], li.positions_per_row[0], li.positions_per_row[1], li.parts_per_row, li.persistent_luma_workgroups, li.waves_per_workgroup,
		       li.lds_bytes_per_workgroup, li.launches, li.listed, li.internal);
	uint32_t r[4];
	uint64_t st[4], sd[4];
	vfgs_hip_get_seed_state(r);
	vfgs_hip_get_stripe_stream_stats(st);
	vfgs_hip_get_seeded_stream_stats(sd);
	printf(" | seed=%08x,%08x,%08x,%08x stripe=%d seeded=%d\n", r[0], r[1], r[2], r[3], (int)st[3], (int)sd[3]);
}

struct Shape { int depth, sx, sy; unsigned w, h; bool one; };

// the call every case starts from: whole frames of the shape, rows of whole blocks, planes of the sets
static Args base(const Shape& s, const Set& A, const Set& B, unsigned n)
{
	Args a;
	a.n = n; a.w = s.w; a.h = s.h; a.ph = s.h;
	a.stride = a.cstride = a.dstride = a.dcstride = (s.w + 15) / 16 * 16;
	a.yp = a.cp = a.dyp = a.dcp = A.pitch;
	a.src.assign(A.list.begin(), A.list.begin() + n);
	a.dst.assign(B.list.begin(), B.list.begin() + n);
	a.shift = s.depth > 8 ? 16 - s.depth : 0;
	return a;
}

static std::string describe(const Shape& s, const Args& a, const char* more = "")
{
	char b[200];
	snprintf(b, sizeof b, "d%d %d,%d %s w%u h%u n%u part %u+%u%s%s%s", s.depth, s.sx, s.sy, s.one ? "one" : "gen", a.w, a.h, a.n, a.py, a.ph, a.copy ? " copy" : "",
	         a.seeds.empty() ? "" : " seeds", more);
	return b;
}

static std::vector<uint32_t> matrix_seeds(unsigned n)
{
	std::vector<uint32_t> s(n);
	for (unsigned i = 0; i < n; i++) s[i] = i == 0 ? 0 : (i == 1 ? 0x80000000u : 1234567u * i + 89);
	return s;
}

// ---- accepted calls: every entry over the shapes -------------------------------------------------------------------------------

static void matrix()
{
	const Shape shapes[] = {{8, 2, 2, 136, 17, false},   {10, 2, 2, 144, 48, false}, {10, 2, 1, 8208, 33, true}, {12, 1, 1, 136, 48, true},
	                        {8, 1, 2, 144, 33, true},    {12, 2, 2, 8208, 17, false}, {12, 2, 1, 144, 17, true},  {10, 2, 2, 8192, 33, true}};
	for (const Shape& s : shapes)
	{
		program(s.depth, s.sx, s.sy, true);
		vfgs_hip_model* mo = capture();
		program(s.depth, s.sx, s.sy, false);
		vfgs_hip_model* mg = capture();
		program(s.depth, s.sx, s.sy, s.one);
		const unsigned nmax = s.w <= 144 ? 33 : 3, stride = (s.w + 15) / 16 * 16;
		Set A(nmax, stride, s.h), B(nmax, stride, s.h);
		auto go = [&](Entry e, Args a, const char* more = "") {
			if (narrows(e) && s.depth == 8) return;
			if (semiplanar(e) && (s.sx != 2 || s.w > 8192)) return;
			if (e == MODELS && s.w > 8192) return;
			if (must_copy(e)) a.copy = true;
			if (!takes_dst(e)) a.copy = false;
			report(e, describe(s, a, more), call(e, a));
		};
		// parts of frames (the entries with frames at a pitch and the lists take turns over the parts)
		int turn = 0;
		for (unsigned py : {0u, 16u})
			for (unsigned ph : {0u, 1u, 17u})
			{
				if (py + ph > s.h) continue;
				Args a = base(s, A, B, 1);
				a.py = py; a.ph = ph;
				go(STRIPE, a);
				go(FRAME_PART, a);
				a = base(s, A, B, 2);
				a.py = py; a.ph = ph; a.copy = true;
				go(turn & 1 ? LIST_PART : FRAMES_PART, a);
				go(turn++ & 1 ? COPY8 : COPY, a);
				a = base(s, A, B, 3);
				a.py = py; a.ph = ph;
				a.seeds = matrix_seeds(3);
				go(SEEDED_PART, a);
			}
		// whole frames, in place and copied, with and without a seed per frame, a model per frame: every entry at some frame count
		go(FRAME, base(s, A, B, 1));
		for (unsigned n : {1u, 2u, 3u, 33u})
		{
			if (n > nmax) continue;
			Args a = base(s, A, B, n), c = a, sd = a, sc = a;     // in place, copied, seeded in place, seeded and copied
			c.copy = sc.copy = true;
			sd.seeds = sc.seeds = matrix_seeds(n);
			go(FRAMES, a);
			go(LIST, a);
			go(SEEDED, sd);
			if (n == 1) { go(COPY, c); go(COPY8, c); go(SP, sd); go(TO_SP, c); }
			if (n == 2) { go(LIST_COPY, c); go(LIST_COPY8, c); go(SP, a); go(SP_COPY8, sc); go(TO_SP8, c); }
			if (n == 3) { go(SEEDED_COPY, sc); go(SEEDED_COPY8, sc); go(SP, sc); go(SP_COPY8, c); go(TO_SP, sc); go(TO_SP8, sc); }
			if (n == 33) { go(LIST_COPY, a); go(SEEDED_COPY, sd); go(COPY, a); go(SP, c); }
			// models: one form, then a list whose form changes inside it (and, at 33 frames, a run longer than a launch holds)
			for (int mixed = 0; mixed < 2; mixed++)
			{
				Args m = (int)(n & 1) != mixed ? sc : a;
				for (unsigned i = 0; i < n; i++) m.models.push_back(!mixed ? (s.one ? mo : mg) : ((i % 3 == 1 && i < 6) ? mo : mg));
				go(MODELS, m, mixed ? " mixed forms" : " one form");
				go(SP_MODELS, m, mixed ? " mixed forms" : " one form");
			}
		}
		hipDeviceSynchronize();
		vfgs_hip_model_release(mo);
		vfgs_hip_model_release(mg);
	}
}

// ---- a chroma mix set and cleared; persistent workgroups; two fronts; an overlap region ------------------------------------------

static void modes()
{
	for (int depth : {8, 10})
	{
		const Shape s{depth, 2, 2, 144, 48, true};
		program(depth, 2, 2, true);
		Set A(3, 144, 48), B(3, 144, 48);
		for (int on = 1; on >= 0; on--)
		{
			if (on) { vfgs_hip_set_chroma_mix(1, 32, 32, 0); vfgs_hip_set_chroma_mix(2, -20, 100, 3); }
			else vfgs_hip_clear_chroma_mix();
			const char* more = on ? " mix" : " mix cleared";
			for (Entry e : {FRAME, FRAMES, COPY, COPY8, LIST, LIST_COPY, LIST_COPY8, SEEDED, SP, SP_COPY8, TO_SP})
				for (int copy = 0; copy < 2; copy++)
				{
					if ((narrows(e) && depth == 8) || (copy && !takes_dst(e)) || (!copy && must_copy(e))) continue;
					Args a = base(s, A, B, e == FRAME ? 1 : 3);
					a.copy = copy != 0;
					if (e == SEEDED) a.seeds = matrix_seeds(3);
					report(e, describe(s, a, more), call(e, a));
				}
		}
	}
	{
		// general-form luma of small 10-bit pictures, enough tasks for persistent workgroups: 600 frames at pitch 0 (the same planes)
		const Shape s{10, 2, 2, 144, 48, false};
		program(10, 2, 2, false);
		Set A(1, 144, 48), B(1, 144, 48);
		Args a = base(s, A, B, 1);
		a.n = 600; a.yp = a.cp = a.dyp = a.dcp = 0;
		report(FRAMES, describe(s, a, " pitch 0"), call(FRAMES, a));
		a.n = 65536;
		report(FRAMES, describe(s, a, " pitch 0"), call(FRAMES, a));
	}
	{
		// rows far apart: a stripe of 64 MiB and more per frame pair is swept on two fronts -- but not inside an overlap region
		const Shape s{10, 2, 2, 144, 48, true};
		program(10, 2, 2, true);
		const unsigned stride = 0x70000;
		Set A(1, stride, 48), B(1, 144, 48), C(3, 144, 48), D(3, 144, 48);
		void* st = nullptr;
		hipStreamCreateWithFlags(&st, 1);
		Args a = base(s, A, B, 1);
		a.n = 2; a.stride = a.cstride = stride; a.yp = a.cp = 0; a.stream = st;
		Args b = base(s, C, D, 3);
		b.stream = st;
		report(FRAMES, describe(s, a, " stride 0x70000 pitch 0"), call(FRAMES, a));
		printf("overlap_begin %d\n", vfgs_hip_overlap_begin(st));
		report(FRAMES, describe(s, a, " stride 0x70000 pitch 0, in a region"), call(FRAMES, a));
		report(LIST, describe(s, b, " in a region"), call(LIST, b));
		b.copy = true;
		report(SP, describe(s, b, " in a region"), call(SP, b));
		report(FRAME, describe(s, b, " in a region"), call(FRAME, b));
		printf("overlap_end %d\n", vfgs_hip_overlap_end(st));
		report(LIST, describe(s, b, " behind the region"), call(LIST, b));
		hipDeviceSynchronize();
		hipStreamDestroy(st);
	}
}

// ---- refusals: each one an entry can raise, alone and together with the one behind it in that entry's order ---------------------

enum Fault { PARTY, PARTH, FPITCH, NOSEEDS, NULLSRC, NULLDST, NULLPLANE, NARROW, TOOWIDE, STRIDE, ALIGN, ROWPITCH, DALIGN, UVSTRIDE, TWICE, SHARED, DEPTH8, DSTRIDE,
             DROWPITCH, DFPITCH, BADLUT, TWOGIB, MIXON, MIXGEN, MIX12, CSUBX, SSHIFT, SPWIDE, NOMODELS, NULLMODEL, GONEMODEL, DEPTHMODEL, NFAULTS };
static const char* const kFaults[NFAULTS] = {"part_y 8", "part past the frame", "frame pitch + 8", "no seeds", "null source list", "null destination list", "null plane",
                                             "width 100", "width 31760", "stride 128", "plane + 8", "stride + 4", "destination plane + 8", "uv_stride 80",
                                             "a destination twice", "source of 0 is destination of 1", "depth 8", "destination stride 128", "destination stride + 4",
                                             "destination frame pitch + 8", "undefined pattern slot", "rows of 256 MiB", "mix", "mix, general form", "mix, depth 12",
                                             "csubx 1", "sample_shift 5", "width 8208", "null models", "null model", "released model", "model of depth 8"};

static vfgs_hip_model *g_live, *g_gone, *g_m8;

static void apply(Fault f, Entry e, Args& a)
{
	unsigned char lut[256];
	switch (f)
	{
	case PARTY: a.py = 8; break;
	case PARTH: a.ph = a.h + 1; break;
	case FPITCH: a.yp += 8; break;
	case NOSEEDS: a.seeds.clear(); break;
	case NULLSRC: a.null_src = true; break;
	case NULLDST: a.null_dst = true; break;
	case NULLPLANE: a.src[1].U = nullptr; break;
	case NARROW: a.w = 100; break;
	case TOOWIDE: a.w = a.stride = a.cstride = a.dstride = a.dcstride = 31760; break;
	case STRIDE: a.stride = 128; break;
	case ALIGN: a.src[0].Y = (uint8_t*)a.src[0].Y + 8; break;
	case ROWPITCH: a.stride += 4; break;
	case DALIGN: a.dst[0].Y = (uint8_t*)a.dst[0].Y + 8; break;
	case UVSTRIDE: a.cstride = 80; break;
	case TWICE: (a.copy ? a.dst : a.src)[1] = (a.copy ? a.dst : a.src)[0]; break;
	case SHARED: a.dst[1].Y = a.src[0].Y; break;
	case DEPTH8: vfgs_set_depth(8); a.shift = 0; break;
	case DSTRIDE: a.dstride = 128; break;
	case DROWPITCH: a.dstride += 4; break;
	case DFPITCH: a.dyp += 8; break;
	case BADLUT: memset(lut, 0x90, sizeof lut); vfgs_set_pattern_lut(1, lut); break;
	case TWOGIB:      // (one frame, planes at made-up addresses far apart: the call is refused before anything is read)
		a.stride = a.cstride = a.dstride = a.dcstride = 0x8000000; a.n = 1;
		a.src[0] = {(void*)(1ull << 40), (void*)(2ull << 40), (void*)(3ull << 40)};
		a.dst[0] = {(void*)(4ull << 40), (void*)(5ull << 40), (void*)(6ull << 40)};
		break;
	case MIXON: vfgs_hip_set_chroma_mix(1, 32, 32, 0); break;
	case MIXGEN: program(10, 2, 2, false); vfgs_hip_set_chroma_mix(1, 32, 32, 0); break;
	case MIX12: program(12, 2, 2, true); vfgs_hip_set_chroma_mix(1, 32, 32, 0); a.shift = 4; break;
	case CSUBX: vfgs_set_chroma_subsampling(1, 2); break;
	case SSHIFT: a.shift = 5; break;
	case SPWIDE:      // (planes at made-up addresses, as above: no entry that is asked for this takes rows walked in parts)
		a.w = a.stride = a.cstride = a.dstride = a.dcstride = 8208; a.n = 1;
		a.src[0] = {(void*)(1ull << 40), (void*)(2ull << 40), (void*)(3ull << 40)};
		a.dst[0] = {(void*)(4ull << 40), (void*)(5ull << 40), (void*)(6ull << 40)};
		break;
	case NOMODELS: a.null_models = true; break;
	case NULLMODEL: a.models[1] = nullptr; break;
	case GONEMODEL: a.models[2] = g_gone; break;
	case DEPTHMODEL: a.models[0] = g_m8; break;
	default: break;
	}
	(void)e;
}

static void refusals()
{
	const Shape s{10, 2, 2, 144, 48, true};
	program(8, 2, 2, true);
	g_m8 = capture();
	program(10, 2, 2, true);
	g_gone = capture();
	vfgs_hip_model_release(g_gone);
	g_live = capture();
	Set A(3, 144, 48), B(3, 144, 48);
	const std::vector<Fault> geometry = {NARROW, TOOWIDE, STRIDE, ALIGN, ROWPITCH}, tail = {BADLUT, TWOGIB, MIXGEN}, sp40 = {CSUBX, SSHIFT, SPWIDE};
	const std::vector<Fault> models41 = {NOMODELS, NULLMODEL, GONEMODEL, DEPTHMODEL};
	for (int ei = 0; ei < NENTRIES; ei++)
	{
		const Entry e = (Entry)ei;
		const bool parts = e == FRAME_PART || e == FRAMES_PART || e == COPY || e == COPY8 || e == LIST_PART || e == SEEDED_PART;
		const bool seeded = e >= SEEDED && e <= SEEDED_COPY8, pitches = e == FRAMES || e == FRAMES_PART || e == COPY || e == COPY8;
		// the order in which the entry refuses
		std::vector<Fault> order;
		auto add = [&](const std::vector<Fault>& v) { order.insert(order.end(), v.begin(), v.end()); };
		const std::vector<Fault> dst8 = {DSTRIDE, DROWPITCH};
		std::vector<Fault> lists = {NULLSRC};
		if (takes_dst(e)) lists.push_back(NULLDST);
		std::vector<Fault> sweep = {NULLPLANE, NARROW, TOOWIDE, STRIDE, ALIGN, ROWPITCH};
		if (takes_dst(e)) sweep.push_back(DALIGN);
		if (e == SP || e == SP_MODELS || e == SP_COPY8) sweep.push_back(UVSTRIDE);
		sweep.push_back(TWICE);
		if (takes_dst(e)) sweep.push_back(SHARED);
		if (parts) add({PARTY, PARTH});
		if (pitches) add({FPITCH});
		if (!is_list(e))
		{
			add(geometry);
			if (e == COPY) add({DALIGN});
			if (e == COPY8) add({DEPTH8, DSTRIDE, DROWPITCH, DFPITCH});
			add(tail);
		}
		else if (e == MODELS) { add(models41); add({SPWIDE, MIXON}); add(lists); add(sweep); add({TWOGIB}); }
		else if (e == SP) { add(sp40); add({MIX12}); add(lists); add(sweep); add(tail); }
		else if (e == SP_MODELS) { add(lists); add(sweep); add(sp40); add(models41); add({MIXON, TWOGIB}); }
		else if (e == SP_COPY8) { add(sp40); add({DEPTH8, MIXON}); add(lists); add(dst8); add(sweep); add({BADLUT, TWOGIB}); }
		else if (e == TO_SP || e == TO_SP8)
		{
			add({CSUBX});
			if (e == TO_SP) add({SSHIFT});
			add({SPWIDE});
			if (e == TO_SP8) add({DEPTH8});
			add({MIXON}); add(lists); add(dst8); add(sweep); add({BADLUT, TWOGIB});
		}
		else
		{
			if (seeded) add({NOSEEDS});
			add(lists); add(sweep);
			if (narrows(e)) add({DEPTH8, DSTRIDE, DROWPITCH});
			add(tail);
		}
		for (size_t i = 0; i < order.size(); i++)
			for (int together = 0; together < 2; together++)
			{
				if (together && i + 1 == order.size()) continue;
				program(10, 2, 2, true);
				Args a = base(s, A, B, 3);
				a.copy = takes_dst(e);
				if (parts) { a.py = 16; a.ph = 17; }
				if (seeded || e >= MODELS) a.seeds = matrix_seeds(3);
				if (e == MODELS || e == SP_MODELS) a.models.assign(3, g_live);
				if (together) apply(order[i + 1], e, a);      // (the earlier one is applied last: where both change one argument, it wins)
				apply(order[i], e, a);
				report(e, std::string(kFaults[order[i]]) + (together ? std::string(" + ") + kFaults[order[i + 1]] : ""), call(e, a));
			}
		// no frames: no call at all in the lists, whatever else is wrong; the plane calls check first
		for (Fault f : {NFAULTS, NARROW})
		{
			program(10, 2, 2, true);
			Args a = base(s, A, B, 3);
			a.n = 0;
			a.copy = takes_dst(e);
			if (e == MODELS || e == SP_MODELS) a.null_models = true;
			apply(f, e, a);
			report(e, std::string("no frames") + (f == NFAULTS ? "" : std::string(" + ") + kFaults[f]), call(e, a));
		}
	}
	hipDeviceSynchronize();
	vfgs_hip_model_release(g_live);
	vfgs_hip_model_release(g_m8);
}

int main()
{
	matrix();
	modes();
	refusals();
	hipDeviceSynchronize();
	vfgs_hip_shutdown();
	return 0;
}
