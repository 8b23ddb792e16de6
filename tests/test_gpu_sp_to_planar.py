"""GPU (MI355X): vfgs_hip_add_grain_sp_frame_list_to_planar_dev and _models_to_planar_dev -- semi-planar surfaces in (NV12 / NV16 / P010 /
P210 / P012), planar pictures out -- against the oracle, through the C ABI, bit for bit: every byte of the three destination planes of every
frame, padding included, every container of the sources (unchanged), and the four seed registers.

The cases and their expectation are tests/sp_to_planar_cases.py's (the existing semi-planar helpers' results, taken apart and shifted
down; checked on the oracle alone by tests/test_sp_to_planar_cases_cpu.py).  Three frames a case, heights 33 and 39, rows of 9, 21, 65, 129,
257 and 512 blocks: the smallest shapes at which this walk can go wrong (the case table says why each is there).  Frames are separate
allocations listed out of address order unless a test says otherwise; destinations are pre-filled with garbage."""
import numpy as np
import pytest

import layout_arena as LA
import model_list_util as U
import semiplanar_util as SP
import sp_model_list_util as SU
import sp_to_planar_cases as C
import vfgs_testlib as T
from gpu_util import stream_ptr
from test_gpu_semiplanar import DevSP, assert_equal, scattered

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


class DevPlanes:
    """a planar destination (sp_to_planar_cases.Planes) resident on the GPU, an allocation per plane"""

    def __init__(self, p):
        import torch
        self.p = p
        self.t = [torch.from_numpy(a.view(np.uint8).copy()).cuda() for _, a in p.planes()]

    def ptrs(self):
        return tuple(t.data_ptr() for t in self.t)

    def download(self):
        import torch
        torch.cuda.synchronize()
        return C.Planes(*[t.cpu().numpy().view(a.dtype) for t, (_, a) in zip(self.t, self.p.planes())])


def destinations(fills, seed=0):
    order = np.random.default_rng(1000 + seed).permutation(len(fills))
    dst = [None] * len(fills)
    for i in order:
        dst[i] = DevPlanes(fills[i])
    return dst


def assert_planes(got, want, what=""):
    for (role, a), (_, b) in zip(got.planes(), want.planes()):
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            at = tuple(bad[0])
            raise AssertionError(f"{what} plane {role}: {len(bad)} samples differ, first at {at}: got {a[at]:#x}, want {b[at]:#x}; last at {tuple(bad[-1])}")


def launches(hip):
    return U.launches(hip)


class Setup:
    """the library programmed for a case (with models: the models captured, the library left programmed with the last one)"""

    def __init__(self, hip, case):
        self.hip, self.case = hip, case
        self.depth, self.sy = C.geometry(case)
        self.handles, self.forms = None, None
        if case.models:
            self.recs = [C.records_of(m) for m in case.models]
            self.handles = U.capture_all(hip, self.recs, stream_ptr())
            self.forms = [(i["one_y"], i["one_c"]) for i in (hip.model_info(m) for m in self.handles)]
        else:
            U.program(hip, C.records_of(case.program))

    def release(self):
        for m in self.handles or []:
            self.hip.model_release(m)

    def call(self, src, dst, geo, seeds=None, pick=None, shift=None, stream=None):
        """src / dst: lists of plane addresses; geo: (width, height, stride, uv_stride, dst_stride, dst_cstride)"""
        st = stream_ptr() if stream is None else stream
        shift = self.case.shift if shift is None else shift
        if self.handles:
            self.hip.add_grain_sp_frame_list_models_to_planar_dev(src, dst, [self.handles[k] for k in (pick or C.pick_of(self.case))[:len(src)]], seeds, *geo, shift, st)
        else:
            self.hip.add_grain_sp_frame_list_to_planar_dev(src, dst, seeds, *geo, shift, st)

    def assert_launch(self, info, n0, pick=None):
        case = self.case
        assert info["listed"] == 1 and info["in_place"] == 0 and info["out8"] == 0 and info["depth"] == self.depth, info
        assert info["lds_bytes_per_workgroup"] == 40960, info
        if self.handles:
            pick = pick or C.pick_of(case)
            runs = U.runs_of(self.forms, pick)
            assert info["launches"] - n0 == len(runs) and info["nframes"] == runs[-1], (info, runs)
            assert info["kernel"] == T.kernel_name("grain_spml_kernel", self.depth, self.sy, *self.forms[pick[-1]]), info
        else:
            assert info["launches"] - n0 == 1 and info["nframes"] == C.NFRAMES, info
            # (the form is the program's, from the table: not read back from the record it is compared with)
            assert info["kernel"] == T.kernel_name("grain_sp_kernel", self.depth, self.sy, *C.FORM_OF[case.program]), info
            assert (info["one_y"], info["one_c"]) == C.FORM_OF[case.program], info


def geo_of(f0, fill):
    return (f0.width, f0.height, f0.stride, f0.uv_stride, fill.stride, fill.cstride)


def programmed_state(hip):
    return (hip.params(), [hip.luts(c) for c in range(3)], hip.chroma_mix(1), hip.chroma_mix(2))


def run_case(hip, case, shuffle=0, stream=None):
    s = Setup(hip, case)
    try:
        frames = C.sources(case)
        fills = [C.fill_for(f, 7 + i, case.pad, case.cpad) for i, f in enumerate(frames)]
        want, regs = C.expected(case, frames, fills)
        src, dst = scattered(frames, shuffle), destinations(fills, shuffle)
        before = programmed_state(hip)
        n0 = launches(hip)
        s.call([d.ptrs() for d in src], [d.ptrs() for d in dst], geo_of(frames[0], fills[0]), C.seeds_of(case), stream=stream)
        for i, (sd, dd, f, w) in enumerate(zip(src, dst, frames, want)):
            assert_planes(dd.download(), w, f"{case.id} destination {i}")       # what is written, and every other byte as it was
            assert_equal(sd.download(), f, f"{case.id} source {i}")
        assert hip.seed_state() == regs
        info = hip.last_launch_info()
        s.assert_launch(info, n0)
        if case.models:
            assert programmed_state(hip) == before
            assert s.forms[0] == s.forms[1] != s.forms[2], s.forms
        return info
    finally:
        s.release()


# ---- the case table ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_case(hip, case):
    info = run_case(hip, case, shuffle=len(case.id))
    sz = 2 if C.geometry(case)[0] > 8 else 1
    units = (case.blocks * 16 * sz + 31) // 32               # 32-byte units of a UV row
    assert info["positions_per_row"][1] == (units + 64) // 64, info
    assert bool(hip.seeded_stream_stats()["last_launch_used_it"]) == case.seeded


def test_the_table_of_forms_is_the_plain_semi_planar_calls(hip):
    """sp_to_planar_cases.FORM_OF, which pins the kernel every case without models must name, against the existing call on the same programs"""
    for prog, form in C.FORM_OF.items():
        rec = C.records_of(prog)
        depth, _, sy = T.trace_geometry(rec)
        U.program(hip, rec)
        d = DevSP(SP.garbage_sp_frame(136, 33, depth, sy, 0, 5))
        hip.add_grain_sp_frame_list_dev([d.ptrs()], None, None, 136, 33, d.sp.stride, d.sp.uv_stride, 0, stream_ptr())
        info = hip.last_launch_info()
        assert (info["one_y"], info["one_c"]) == form and info["kernel"] == T.kernel_name("grain_sp_kernel", depth, sy, *form), (prog, info)


def test_all_four_forms(hip):
    seen = {}
    for c in C.CASES:
        if c.id.startswith("form-") and not c.seeded:
            info = run_case(hip, c)
            seen[(info["one_y"], info["one_c"])] = info["kernel"]
    assert set(seen) == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen
    assert all(k.startswith("grain_sp_kernel<") for k in seen.values()), seen


# ---- memory as a caller hands it over -----------------------------------------------------------------------------------------------

def arena_case(case, index):
    """sources and destinations in ONE allocation: the planes of each side back to back, bases 16-aligned and never 256-aligned, the
    smallest pitches, exactly the addressed rows, random guards"""
    depth, sy = C.geometry(case)
    sz = 2 if depth > 8 else 1
    frames = C.sources(case)
    rows, crows, cols = C.written(frames[0])
    nblk = cols // 16
    py, pc = LA.min_pitch(nblk, sz), LA.min_pitch(nblk, sz, 2)
    src, dst = [], []
    for f in range(C.NFRAMES):
        src += [LA.Want(f"src.f{f}.Y", "Y", "src", f, py, rows, nblk * 16 * sz, sz, 0), LA.Want(f"src.f{f}.UV", "UV", "src", f, py, crows, nblk * 16 * sz, sz, 0)]
        dst += [LA.Want(f"dst.f{f}.Y", "Y", "dst", f, py, rows, nblk * 16 * sz, sz, 0)]
        dst += [LA.Want(f"dst.f{f}.{r}", r, "dst", f, pc, crows, nblk * 8 * sz, sz, 0) for r in ("U", "V")]
    arena = LA.Arena([src, dst], index, 4242 + index)
    for f, sp in enumerate(frames):
        arena.put(arena.plane("src", f, "Y"), sp.Y)
        arena.put(arena.plane("src", f, "UV"), sp.UV)
    # the sources as the arena holds them: tight pitches (the rows of the picture, their whole blocks)
    tight = []
    # (as arrays of the test library's geometry: the luma rows rounded up to 16, zeros behind the rows the arena holds -- never addressed)
    h2 = (frames[0].height + 15) & ~15
    for f, sp in enumerate(frames):
        Y, UV = np.zeros((h2, py // sz), sp.dtype), np.zeros((h2 // sy, py // sz), sp.dtype)
        Y[:rows] = np.ascontiguousarray(arena.rows(arena.plane("src", f, "Y"))).view(sp.dtype)
        UV[:crows] = np.ascontiguousarray(arena.rows(arena.plane("src", f, "UV"))).view(sp.dtype)
        tight.append(SP.SPFrame(sp.width, sp.height, depth, sy, py // sz, py // sz, case.shift, Y, UV))
    return arena, tight, (py // sz, pc // sz)


@pytest.mark.parametrize("cid", ["nv12-21", "p010-65", "p012-129", "models-10_422-seeded"])
def test_arena(hip, cid):
    """one case per depth (and one with a model per picture): the WHOLE allocation is compared -- guards, pad bytes, the sources"""
    import torch
    case = next(c for c in C.CASES if c.id == cid)
    arena, tight, (dstride, dcstride) = arena_case(case, C.CASES.index(case))
    want_sp, regs = C.expected_sp(case, tight)
    want = arena.buf.copy()
    for f, w in enumerate(want_sp):
        d = SP.to_planar(w)
        for role, a in (("Y", d.Y), ("U", d.U), ("V", d.V)):
            arena.put(arena.plane("dst", f, role), a, want)
    assert np.count_nonzero(want != arena.buf) * 4 >= np.count_nonzero(arena.region_mask())      # (a quarter of the region's bytes change)
    s = Setup(hip, case)
    try:
        dev = torch.from_numpy(arena.buf.copy()).cuda()
        base = dev.data_ptr()
        at = lambda side, f, role: base + arena.plane(side, f, role).off
        src = [(at("src", f, "Y"), at("src", f, "UV")) for f in range(C.NFRAMES)]
        dst = [(at("dst", f, "Y"), at("dst", f, "U"), at("dst", f, "V")) for f in range(C.NFRAMES)]
        # (16-byte bases; where a side's planes begin is never 256-aligned, the planes behind lie back to back)
        assert all(p % 16 == 0 for fr in src + dst for p in fr) and src[0][0] % 256 != 0 and dst[0][0] % 256 != 0
        f0 = tight[0]
        n0 = launches(hip)
        s.call(src, dst, (f0.width, f0.height, f0.stride, f0.uv_stride, dstride, dcstride), C.seeds_of(case))
        torch.cuda.synchronize()
        LA.compare(arena, dev.cpu().numpy(), want, what=cid)
        assert hip.seed_state() == regs
        s.assert_launch(hip.last_launch_info(), n0)
    finally:
        s.release()


# ---- neighbours, streams ------------------------------------------------------------------------------------------------------------

def test_neighbours_unharmed(hip):
    """KernelArgs::sp_kernel gained a value: the plain semi-planar call, in place and out of place, and the models call run once each
    behind a _to_planar call on the same stream; each is bit-exact and reports its own kernel"""
    case = next(c for c in C.CASES if c.id == "models-10_420-sequence")
    run_case(hip, next(c for c in C.CASES if c.id == "p010-65"))
    assert hip.last_launch_info()["kernel"].startswith("grain_sp_kernel<")
    s = Setup(hip, case)
    try:
        depth, sy, W, H = s.depth, s.sy, 1032, 39
        ora = U.oracle_programmed(s.recs[-1])
        # the new call with models in front
        frames = C.sources(case)
        fills = [C.fill_for(f, 70 + i) for i, f in enumerate(frames)]
        want, regs = C.expected(case, frames, fills, ora)
        src, dst = scattered(frames, 1), destinations(fills, 1)
        s.call([d.ptrs() for d in src], [d.ptrs() for d in dst], geo_of(frames[0], fills[0]))
        for dd, w in zip(dst, want):
            assert_planes(dd.download(), w, "to planar")
        assert hip.seed_state() == regs == ora.seed_state()
        # the plain semi-planar call in place: the library is still programmed with the last model captured (the models call left the programmed
        # state alone), so an oracle programmed the same way, both from one seed
        ora = U.oracle_programmed(s.recs[-1])
        hip.set_seed(77); ora.set_seed(77)
        mk = lambda n, seed: [SP.garbage_sp_frame(W, H, depth, sy, 6, seed + i) for i in range(n)]
        fr = mk(3, 200)
        w1 = SP.expected(ora, fr, None, 6)
        dev = scattered(fr, 2)
        hip.add_grain_sp_frame_list_dev([d.ptrs() for d in dev], None, None, W, H, fr[0].stride, fr[0].uv_stride, 6, stream_ptr())
        for d, w in zip(dev, w1):
            assert_equal(d.download(), w, "in place")
        info = hip.last_launch_info()
        assert hip.seed_state() == ora.seed_state() and info["kernel"].startswith("grain_sp_kernel<") and info["in_place"] == 1, info
        # ... out of place: the written containers keep their shift, the padding its bytes
        fr = mk(3, 300)
        w2 = SP.expected(ora, fr, [4, 5, 6], 6)
        fill = SP.garbage_sp_frame(W, H, depth, sy, 6, 999)
        sdev, ddev = scattered(fr, 3), [DevSP(fill) for _ in fr]
        hip.add_grain_sp_frame_list_dev([d.ptrs() for d in sdev], [d.ptrs() for d in ddev], [4, 5, 6], W, H, fr[0].stride, fr[0].uv_stride, 6, stream_ptr())
        rows, crows, cols = SP.written_region(fr[0])
        for sd, dd, w, f in zip(sdev, ddev, w2, fr):
            e = fill.copy()
            e.Y[:rows, :cols] = w.Y[:rows, :cols]
            e.UV[:crows, :cols] = w.UV[:crows, :cols]
            assert_equal(dd.download(), e, "out of place")
            assert_equal(sd.download(), f, "source")
        info = hip.last_launch_info()
        assert hip.seed_state() == ora.seed_state() and info["kernel"].startswith("grain_sp_kernel<") and info["in_place"] == 0, info
        # the semi-planar call with models, in place
        fr = mk(3, 400)
        pick = [1, 0, 1]
        w3, regs3 = SU.expect_unseeded(ora, s.recs, pick, fr, 6)
        dev = scattered(fr, 4)
        hip.add_grain_sp_frame_list_models_dev([d.ptrs() for d in dev], None, [s.handles[k] for k in pick], None, W, H, fr[0].stride, fr[0].uv_stride, 6, stream_ptr())
        for d, w in zip(dev, w3):
            assert_equal(d.download(), w, "models")
        assert hip.seed_state() == regs3
        assert hip.last_launch_info()["kernel"] == T.kernel_name("grain_spml_kernel", depth, sy, *s.forms[1])
    finally:
        s.release()


def test_two_calls_inside_an_overlap_region(hip):
    a = next(c for c in C.CASES if c.id == "p010-21")
    s = Setup(hip, a)
    ora = U.oracle_programmed(C.records_of(a.program))
    fa = C.sources(a)
    fb = [SP.garbage_sp_frame(fa[0].width, fa[0].height, s.depth, s.sy, a.shift, 60 + i) for i in range(2)]
    fills = [C.fill_for(f, 80 + i, 16, 16) for i, f in enumerate(fa + fb)]
    seeds = [11, 22]
    wa = SP.expected(ora, fa, None, a.shift)
    wb = SP.expected(ora, fb, seeds, a.shift)
    want = [C.paste(w, f) for w, f in zip(wa + wb, fills)]
    sa, sb, dst = scattered(fa, 8), scattered(fb, 9), destinations(fills, 8)
    geo = geo_of(fa[0], fills[0])
    st = stream_ptr()
    hip.overlap_begin(st)
    s.call([d.ptrs() for d in sa], [d.ptrs() for d in dst[:3]], geo, None, stream=st)
    s.call([d.ptrs() for d in sb], [d.ptrs() for d in dst[3:]], geo, seeds, stream=st)
    hip.overlap_end(st)
    for i, (d, w) in enumerate(zip(dst, want)):
        assert_planes(d.download(), w, f"frame {i}")
    assert hip.seed_state() == ora.seed_state()


# ---- refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ["p010-21", "models-10_420-seeded"], ids=["programmed", "models"])
def test_refusals_change_nothing(hip, cid):
    """every refusal of the contract with its code and its cause; then the registers, `launches` and every byte of every plane are compared;
    then the same lists are served"""
    import torch
    from versatilefilmgrain_amd.hw import VfgsHipError
    case = next(c for c in C.CASES if c.id == cid)
    s = Setup(hip, case)
    try:
        models = s.handles is not None
        frames = C.sources(case)
        fills = [C.fill_for(f, 7 + i, 16, 16) for i, f in enumerate(frames)]
        f0, fill = frames[0], fills[0]
        src, dst = scattered(frames), destinations(fills)
        geo = geo_of(f0, fill)
        good = case.shift
        seeds = [1, 2, 3]
        carries_mix = other_format = None
        if models:
            # (made in front of everything that is compared: a model that carries a mix -- the library is programmed with the last model of the
            # case, all-one-pattern -- and a model of another chroma format, 4:2:2 beside the programmed 4:2:0)
            assert s.forms[2] == (1, 1) and s.sy == 2
            hip.set_chroma_mix(1, 32, 32, 0)
            carries_mix = hip.model_capture_mix(stream_ptr())
            hip.clear_chroma_mix()
            assert hip.model_chroma_mix(carries_mix, 1)[3] == 1
            other_format = U.capture_all(hip, [C.records_of("fgs_sei_10_422")], stream_ptr())[0]
            U.program(hip, s.recs[-1])
        st0, n0 = hip.seed_state(), launches(hip)
        sp, dp = [d.ptrs() for d in src], [d.ptrs() for d in dst]

        def unchanged(what):
            assert hip.seed_state() == st0 and launches(hip) == n0, what
            for i, (sd_, dd, f, w) in enumerate(zip(src, dst, frames, fills)):
                assert_planes(dd.download(), w, f"{what}: destination {i}")
                assert_equal(sd_.download(), f, f"{what}: source {i}")

        def refused(code, s_=sp, d=dp, sd=seeds, g=geo, shift=good, match=None):
            with pytest.raises(VfgsHipError, match=match or f"error {code}:"):
                s.call(s_, d, g, None if sd is None else sd[:len(s_)], shift=shift)
            assert hip.lib.vfgs_hip_last_error() == code
            unchanged(f"after the refusal {code} ({match})")      # after EACH refusal: the registers, `launches`, every byte of every plane

        def with_geo(**kw):
            names = ("width", "height", "stride", "uv_stride", "dst_stride", "dst_cstride")
            return tuple(kw.get(n, v) for n, v in zip(names, geo))

        # what the semi-planar calls refuse with error 40, the cause named
        for subx, suby in ((1, 1), (1, 2)):
            hip.set_chroma_subsampling(subx, suby)
            try:
                refused(40, match="csubx 1")
            finally:
                hip.set_chroma_subsampling(2, s.sy)
        refused(40, shift=4, match="sample_shift 4 at depth 10")
        refused(40, shift=10, match="sample_shift")
        refused(40, g=(8208, f0.height, 8256, 8256, 8256, 4160), match="width 8208")
        hip.set_depth(8)
        try:
            refused(40, shift=6, match="sample_shift 6 at depth 8")
        finally:
            hip.set_depth(10)
        try:
            hip.set_chroma_mix(1, 32, 32, 0)
            refused(41 if models else 40, match="chroma mix")
            refused(41 if models else 40, sd=None, match="chroma mix")
        finally:
            hip.clear_chroma_mix()
        # null list or plane
        arr_s, arr_d = hip.sp_frame_list(sp), hip.frame_list(dp)
        if models:
            fn = hip.lib.vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev
            marr = (__import__("ctypes").c_void_p * 3)(*[s.handles[k] for k in C.pick_of(case)])
            assert fn(None, arr_d, marr, None, 3, *geo, good, stream_ptr()) == 18
            assert fn(arr_s, None, marr, None, 3, *geo, good, stream_ptr()) == 18
            assert fn(arr_s, arr_d, None, None, 3, *geo, good, stream_ptr()) == 41
        else:
            fn = hip.lib.vfgs_hip_add_grain_sp_frame_list_to_planar_dev
            assert fn(None, arr_d, None, 3, *geo, good, stream_ptr()) == 18
            assert fn(arr_s, None, None, 3, *geo, good, stream_ptr()) == 18
        refused(18, s_=[sp[0], (sp[1][0], 0), sp[2]], match="null plane")
        refused(18, s_=[sp[0], (0, sp[1][1]), sp[2]], match="null plane")
        for k in range(3):
            refused(18, d=[dp[0], tuple(0 if i == k else p for i, p in enumerate(dp[1])), dp[2]], match="null plane")
        # misaligned source, misaligned destination
        refused(7, s_=[sp[0], (sp[1][0], sp[1][1] + 8), sp[2]])
        for k in range(3):
            refused(7, d=[dp[0], tuple(p + 8 if i == k else p for i, p in enumerate(dp[1])), dp[2]])
        # geometry of the source, with the semi-planar call's codes
        refused(6, g=with_geo(stride=320))
        refused(6, g=with_geo(uv_stride=320))
        refused(8, g=with_geo(stride=f0.stride + 4))
        refused(8, g=with_geo(uv_stride=f0.uv_stride + 4))
        refused(5, g=with_geo(width=100))
        # the destination's pitches: ONE component's row is half as many samples as the luma row
        refused(6, g=with_geo(dst_stride=320))
        refused(6, g=with_geo(dst_cstride=160))
        refused(8, g=with_geo(dst_stride=fill.stride + 4))
        refused(8, g=with_geo(dst_cstride=fill.cstride + 4))
        # destination planes that share bytes; a destination plane that shares bytes with ANY source plane: there is no in-place form
        refused(18, d=[dp[0], dp[1], dp[0]], match="listed twice")
        refused(18, d=[dp[0], (dp[1][0], dp[1][1], dp[1][1]), dp[2]], match="listed twice")
        refused(18, d=[dp[0], (dp[1][0], dp[1][1], dp[0][0] + 1024), dp[2]], match="overlap")
        refused(18, d=[dp[0], (sp[1][0], dp[1][1], dp[1][2]), dp[2]], match="shares bytes")
        refused(18, d=[dp[0], (dp[1][0], sp[2][1], dp[1][2]), dp[2]], match="shares bytes")
        refused(18, d=[dp[0], (dp[1][0], dp[1][1], sp[0][1] + 2048), dp[2]], match="shares bytes")
        if models:
            # a released model in the list
            gone = hip.model_capture(stream_ptr())
            hip.model_release(gone)
            keep, s.handles[0] = s.handles[0], gone
            try:
                refused(41, match="not a live model")
            finally:
                s.handles[0] = keep
            # a model that CARRIES a mix (the mix stays with the calls that honour it), a model of another chroma format than the programmed one
            for bad, why in ((carries_mix, "carries a chroma mix"), (other_format, "captured at depth 10, chroma subsampling 2,1")):
                keep, s.handles[2] = s.handles[2], bad
                try:
                    refused(41, match=why)
                    refused(41, sd=None, match=why)
                finally:
                    s.handles[2] = keep
            hip.model_release(carries_mix)
            hip.model_release(other_format)
        s.call([], [], geo, None)           # an empty list is no call at all
        unchanged("after the refusals")
        # ... and the same lists are served afterwards
        case3 = case._replace(seeded=True)
        if models:
            want_sp, regs = SU.expect_seeded(s.recs, C.pick_of(case), frames, seeds, good)
        else:
            ora = U.oracle_programmed(C.records_of(case.program))
            want_sp = SP.expected(ora, frames, seeds, good)
            regs = ora.seed_state()
        s.call(sp, dp, geo, seeds)
        for dd, w, f in zip(dst, want_sp, fills):
            assert_planes(dd.download(), C.paste(w, f), "served afterwards")
        assert hip.seed_state() == regs
    finally:
        s.release()
    del torch
