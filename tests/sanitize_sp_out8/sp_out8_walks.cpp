// TEST INFRASTRUCTURE.  Semi-planar frames with the narrowed 8-bit destination (include/vfgs_hip.h: vfgs_hip_add_grain_sp_frame_list_copy8_dev)
// in the host layer of libvfgs_hip, compiled with a sanitizer over the unchanged tests/sanitize/hip_stub.cpp, as
// tests/sanitize_semiplanar/sp_walks.cpp drives the call it extends: out of place with and without seeds, both sample shifts, odd block
// counts, destination pitches larger than the rows and different for Y and UV, more frames than a launch holds, an overlap region, every
// refusal.  Depth 10 only: the model of the launch refuses narrowed launches at any other depth.  The model's "kernel" touches exactly the
// bytes the real one addresses -- the UV plane's whole-block rows of BYTES through components 1 and 2 alike, at the destination's own pitch
// -- so planes allocated exactly as large as the contract says make every wrong extent or pitch a sanitizer report; what it writes, the
// source container narrowed as it lies, is compared too, and the destination's padding must keep its bytes.  The seed registers are
// compared with those of the planar _copy8 list calls on planar frames of the same size, through the same library.  Values are the GPU
// suite's business (tests/test_gpu_semiplanar_out8.py).
//
// usage: sp_out8_walks [walk ...]     (no argument: all of them)
#define WALKS_SEED 99
#include "../sanitize/walks.h"

using Pic = SpPic;
using Pool = SpPool;

// what the model's launch leaves in a destination that held `fill`: in every row of the picture the whole blocks' bytes are the source's
// containers narrowed as they lie, (c + 2) >> 2; everything else is the fill's
static Pic modelled(const Pic& src, const Pic& fill)
{
	Pic out = fill;
	const uint16_t *sy = (const uint16_t*)src.Y.data(), *suv = (const uint16_t*)src.UV.data();
	for (int r = 0; r < src.h; r++)
		for (int i = 0; i < src.nblk * 16; i++) out.Y[(size_t)r * fill.stride + i] = (uint8_t)((sy[(size_t)r * src.stride + i] + 2) >> 2);
	for (int r = 0; r < src.crows; r++)
		for (int i = 0; i < src.nblk * 16; i++) out.UV[(size_t)r * fill.uv_stride + i] = (uint8_t)((suv[(size_t)r * src.uv_stride + i] + 2) >> 2);
	return out;
}

static bool sp8_launch(const vfgs_hip_launch_info& li)
{
	return !strncmp(li.kernel, "grain_sp8_kernel<10,", 20) && li.out8 == 1 && li.listed == 1 && li.in_place == 0 && li.persistent_luma_workgroups == 0 && li.depth == 10;
}

// ---- walks ---------------------------------------------------------------------------------------------------------------

static void walk_out_of_place()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	// width, height, csuby, one-pattern model, sample shift, source row padding (containers), destination padding of Y, of UV (bytes): odd
	// block counts (13, 33, 65, 129), a single block row, the widest row, both shifts
	const int cases[][8] = {{200, 150, 2, 1, 6, 0, 0, 0}, {520, 70, 2, 0, 0, 16, 32, 16}, {1032, 33, 1, 0, 0, 8, 16, 48}, {1042, 96, 1, 1, 6, 0, 0, 16},
	                        {8192, 17, 2, 0, 6, 0, 16, 0}, {2056, 16, 1, 1, 0, 0, 64, 32}, {136, 40, 2, 0, 6, 24, 16, 32}};
	for (const auto& c : cases)
	{
		const int w = c[0], h = c[1], sy = c[2], shift = c[4], n = 5;
		program(10, 2, sy, c[3] != 0);
		Pic f(w, h, sy, 2, c[5], c[5]), fill(w, h, sy, 1, c[6], c[7]);
		const Pic want = modelled(f, fill);
		const std::vector<uint32_t> seeds = seeds_of(n);
		vfgs_set_seed(99);
		const Regs want_plain = planar_regs(f, n, nullptr, PLANAR_LIST_COPY8);
		const Regs want_seeded = planar_regs(f, n, seeds.data(), PLANAR_LIST_COPY8);
		Pool src(f, n);
		vfgs_hip_launch_info a, b;
		{
			// one seed sequence
			Pool dst(fill, n);
			vfgs_set_seed(99);
			CHECK(vfgs_hip_last_launch_info(&a) == 0);
			OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(src.list.data(), dst.list.data(), nullptr, n, w, h, f.stride, f.uv_stride, fill.stride, fill.uv_stride, shift, st));
			CHECK(Regs() == want_plain);
			CHECK(vfgs_hip_last_launch_info(&b) == 0 && sp8_launch(b) && b.nframes == n && b.launches - a.launches == 1);
			hipStreamSynchronize(st);
			CHECK(dst.all_hold(want) && src.all_hold(f));
		}
		{
			// a seed per picture
			Pool dst(fill, n);
			vfgs_set_seed(7);
			OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(src.list.data(), dst.list.data(), seeds.data(), n, w, h, f.stride, f.uv_stride, fill.stride, fill.uv_stride, shift, st));
			CHECK(Regs() == want_seeded);
			CHECK(vfgs_hip_last_launch_info(&b) == 0 && sp8_launch(b));
			hipStreamSynchronize(st);
			CHECK(dst.all_hold(want) && src.all_hold(f));
		}
	}
	hipStreamDestroy(st);
}

static void walk_thirty_three_frames()
{
	program(10, 2, 2, true);
	Pic f(136, 16, 2, 2), fill(136, 16, 2, 1, 16, 32);
	const Pic want = modelled(f, fill);
	const std::vector<uint32_t> seeds = seeds_of(33);
	const Regs want_seeded = planar_regs(f, 33, seeds.data(), PLANAR_LIST_COPY8);
	Pool src(f, 33), dst(fill, 33);
	vfgs_hip_launch_info a, b;
	CHECK(vfgs_hip_last_launch_info(&a) == 0);
	OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(src.list.data(), dst.list.data(), seeds.data(), 33, f.w, f.h, f.stride, f.uv_stride, fill.stride, fill.uv_stride, 6, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 2 && b.nframes == 1 && sp8_launch(b));
	CHECK(Regs() == want_seeded);
	vfgs_set_seed(5);
	const Regs want_plain = planar_regs(f, 33, nullptr, PLANAR_LIST_COPY8);
	vfgs_set_seed(5);
	CHECK(vfgs_hip_last_launch_info(&a) == 0);
	OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(src.list.data(), dst.list.data(), nullptr, 33, f.w, f.h, f.stride, f.uv_stride, fill.stride, fill.uv_stride, 6, nullptr));
	CHECK(vfgs_hip_last_launch_info(&b) == 0 && b.launches - a.launches == 2 && b.nframes == 1);
	CHECK(Regs() == want_plain);
	hipDeviceSynchronize();
	CHECK(src.all_hold(f) && dst.all_hold(want));
}

static void walk_overlap_region()
{
	void* st = nullptr;
	hipStreamCreateWithFlags(&st, 1);
	program(10, 2, 2, true);
	Pic f(520, 70, 2, 2), fill(520, 70, 2, 1, 0, 16);
	const Pic want = modelled(f, fill);
	const std::vector<uint32_t> sb = seeds_of(3);
	vfgs_set_seed(3);
	planar_regs(f, 4, nullptr, PLANAR_LIST_COPY8);
	const Regs regs = planar_regs(f, 3, sb.data(), PLANAR_LIST_COPY8);
	Pool a(f, 4), b(f, 3), da(fill, 4), db(fill, 3);
	vfgs_set_seed(3);
	OK(vfgs_hip_overlap_begin(st));
	OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(a.list.data(), da.list.data(), nullptr, 4, f.w, f.h, f.stride, f.uv_stride, fill.stride, fill.uv_stride, 6, st));
	OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(b.list.data(), db.list.data(), sb.data(), 3, f.w, f.h, f.stride, f.uv_stride, fill.stride, fill.uv_stride, 6, st));
	OK(vfgs_hip_add_grain_sp_frame_list_dev(a.list.data(), a.list.data(), sb.data(), 3, f.w, f.h, f.stride, f.uv_stride, 6, st));      // (the existing call beside it)
	OK(vfgs_hip_overlap_end(st));
	CHECK(Regs() == regs);
	hipStreamSynchronize(st);
	CHECK(a.all_hold(f) && b.all_hold(f) && da.all_hold(want) && db.all_hold(want));
	hipStreamDestroy(st);
}

static void walk_refusals()
{
	program(10, 2, 2, false);
	Pic f(520, 70, 2, 2), fill(520, 70, 2, 1, 16, 32);
	Pool pool(f, 3), other(fill, 3);
	const std::vector<uint32_t> seeds = seeds_of(3);
	const Regs before;
	vfgs_hip_launch_info a, b;
	const bool had = vfgs_hip_last_launch_info(&a) == 0;
	const unsigned h = f.h, s = f.stride, u = f.uv_stride, ds = fill.stride, du = fill.uv_stride;
	auto call = [&](const vfgs_hip_sp_frame* src, const vfgs_hip_sp_frame* dst, unsigned ww = 520, unsigned ss = 0, unsigned uu = 0, unsigned shift = 6, unsigned dss = 0,
	                unsigned duu = 0) {
		const int rc = vfgs_hip_add_grain_sp_frame_list_copy8_dev(src, dst, seeds.data(), 3, ww, h, ss ? ss : s, uu ? uu : u, dss ? dss : ds, duu ? duu : du, shift, nullptr);
		CHECK(rc == vfgs_hip_last_error());
		return rc;
	};
	auto L = pool.list, D = other.list;
	// everything the semi-planar call refuses
	CHECK(call(nullptr, D.data()) == 18 && call(L.data(), nullptr) == 18);
	L[1].UV = nullptr;
	CHECK(call(L.data(), D.data()) == 18);
	L = pool.list; D[1].Y = nullptr;
	CHECK(call(L.data(), D.data()) == 18);
	D = other.list; L[1].UV = (uint8_t*)L[1].UV + 8;
	CHECK(call(L.data(), D.data()) == 7);
	L = pool.list; D[2].Y = (uint8_t*)D[2].Y + 4;
	CHECK(call(L.data(), D.data()) == 7);
	D = other.list; D[2].UV = (uint8_t*)D[2].UV + 8;
	CHECK(call(L.data(), D.data()) == 7);
	D = other.list;
	CHECK(call(L.data(), D.data(), 520, 512) == 6 && call(L.data(), D.data(), 520, 0, 512) == 6);
	CHECK(call(L.data(), D.data(), 520, s + 4) == 8 && call(L.data(), D.data(), 520, 0, u + 4) == 8);
	CHECK(call(L.data(), D.data(), 100) == 5);
	CHECK(call(L.data(), D.data(), 520, 0, 0, 4) == 40 && call(L.data(), D.data(), 520, 0, 0, 16) == 40);
	CHECK(call(L.data(), D.data(), 8208, 8208, 8208, 6, 8208, 8208) == 40);
	// the destination's pitches, with the planar _copy8 list's codes: a UV row of bytes is as long as the luma row
	CHECK(call(L.data(), D.data(), 520, 0, 0, 6, 512) == 6 && call(L.data(), D.data(), 520, 0, 0, 6, 0, 512) == 6 && call(L.data(), D.data(), 520, 0, 0, 6, 0, 264) == 6);
	CHECK(call(L.data(), D.data(), 520, 0, 0, 6, ds + 8) == 8 && call(L.data(), D.data(), 520, 0, 0, 6, 0, du + 8) == 8);
	// destinations that share bytes; a destination that shares bytes with a source plane, of its own frame and of another: no in-place form
	D[2] = D[0];
	CHECK(call(L.data(), D.data()) == 18);
	D = other.list; D[1].UV = (uint8_t*)D[0].Y + 1024;
	CHECK(call(L.data(), D.data()) == 18);
	D = other.list; D[1].Y = L[1].Y;
	CHECK(call(L.data(), D.data()) == 18);                   // its own frame's source luma
	D = other.list; D[1].UV = L[1].UV;
	CHECK(call(L.data(), D.data()) == 18);                   // its own frame's source UV
	D = other.list; D[0].UV = (uint8_t*)L[2].Y + 4096;
	CHECK(call(L.data(), D.data()) == 18);                   // inside another frame's source luma
	CHECK(call(L.data(), L.data()) == 18);                   // the source list itself
	D = other.list;
	// depth 8, another chroma format, the mix
	vfgs_set_depth(8);
	CHECK(call(L.data(), D.data(), 520, 0, 0, 0) == 16 && call(L.data(), D.data(), 520, 0, 0, 6) == 40);
	vfgs_set_depth(10);
	vfgs_set_chroma_subsampling(1, 1);
	CHECK(call(L.data(), D.data()) == 40);
	vfgs_set_chroma_subsampling(2, 2);
	OK(vfgs_hip_set_chroma_mix(1, 32, 32, 0));
	CHECK(call(L.data(), D.data()) == 40 && strstr(vfgs_hip_last_error_string(), "chroma mix"));
	vfgs_hip_clear_chroma_mix();
	OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(L.data(), D.data(), seeds.data(), 0, 520, h, s, u, ds, du, 6, nullptr));      // an empty list is no call at all
	CHECK(Regs() == before);
	CHECK((vfgs_hip_last_launch_info(&b) == 0) == had && (!had || a.launches == b.launches));
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f) && other.all_hold(fill));
	// the same lists are served afterwards
	const Regs want = planar_regs(f, 3, seeds.data(), PLANAR_LIST_COPY8);
	vfgs_set_seed(1);
	OK(vfgs_hip_add_grain_sp_frame_list_copy8_dev(L.data(), D.data(), seeds.data(), 3, 520, h, s, u, ds, du, 6, nullptr));
	CHECK(Regs() == want);
	hipDeviceSynchronize();
	CHECK(pool.all_hold(f) && other.all_hold(modelled(f, fill)));
}

int main(int argc, char** argv)
{
	return run_walks(argc, argv, {
		{"out_of_place", walk_out_of_place},
		{"thirty_three_frames", walk_thirty_three_frames},
		{"overlap_region", walk_overlap_region},
		{"refusals", walk_refusals},
	});
}
