"""GPU (MI355X): vfgs_hip_add_grain_sp_frame_list_dev under an active luma / chroma mix (vfgs_hip_set_chroma_mix; AFGS1 cb_mult /
cb_luma_mult / cb_offset) -- NV12 / NV16 / P010 / P210 -- through the C ABI, bit for bit against tests/semiplanar_mix_util.py: the
unchanged oracle on the index frame of D(src), its grain moved onto the real chroma, interleaved and shifted back; every container of
both planes of every frame, padding included, and the four seed registers.

Every input is built by `case(key)` below, which also names the number of chroma samples the derivation may leave out (0 for content in
0.3 .. 0.7 of the range; 3 % -- the planar tests' figure -- for full-range content and for the saturating mix, see SAT).
tests/test_semiplanar_mix_util_cpu.py runs the oracle alone over every case and asserts that cap; here it is asserted again in front
of every comparison.

Shapes are the smallest that reach each mechanism: a UV position is 2 KiB -- 1024 luma samples of a row at 16-bit containers, 2048 at
8 bit -- and the ring of the kernels holds two of them.
"""
import numpy as np
import pytest

import chroma_mix_util as X
import model_programs as MP
import semiplanar_mix_util as M
import semiplanar_util as SP
import vfgs_testlib as T

pytestmark = pytest.mark.gpu

BOTH = ((32, 32, 0), (32, 32, 0))
CORPUS = ((64, 119, -238), (64, 101, -202))
CORPUS_RANGE = dict(lo=0.4, hi=0.6, clo=0.4, chi=0.5)        # keeps the corpus mix inside 0.2 .. 0.8 (test_gpu_chroma_mix.py content_range)
# A mix that saturates: m = L + C - 80 << bs.  On content uniform in 0.3 .. 0.7 of the range m exceeds the range where L + C > 1.3125, a
# triangle of (1.4 - 1.3125)^2 / 2 over the square of 0.4^2: 2.4 % of the samples; there the index is clipped to 2^depth - 1, the oracle's
# output on the index frame mostly sits on a bound and the derivation leaves the sample out.  Cap: the 3 % of the full-range tests.
SAT = ((64, 64, -80), (64, 64, -80))
# The corpus models scale the grain to zero at both ends of the intensity range: there a clipped index gives no grain, the oracle's output on the
# index frame IS the bound, and every saturated sample leaves the comparison -- SAT above runs the clamp but does not pin it.  Two generated
# full-range one-pattern programs (tests/model_programs.py) have scales at the ends: with the index clipped to 2^depth - 1 ("hi") or to 0 ("lo") the
# output leaves the bound wherever the grain points inwards.  A block's sign is random, so that is about half of the saturated samples, less
# those whose grain rounds to zero: the test asks for an eighth.  Cap of the derivation: the 3 % of the full-range tests.
CLAMP_NAMES = {8: "one_cb_cr_differ_8_420", 10: "m128_outside_window_10_422"}
CLAMP_MIXES = {"hi": ((64, 64, -80), (64, 64, -80)), "lo": ((64, 64, -176), (64, 64, -176))}
P8_422 = "one_same_slot_8_422"                               # a one-pattern program at 8 bit 4:2:2 (tests/model_programs.py)
NAMES = {"8/420": "fgs_afgs1_test1_8_420", "10/420": "fgs_afgs1_test1_10_420", "10/422": "fgs_afgs1_test3_10_422", "8/422": P8_422}

HEIGHTS = [16, 17, 33, 70]
WIDTHS8 = [136, 333, 2040, 2048, 2056, 4104, 8192]
WIDTHS10 = [136, 345, 1016, 1024, 1032, 2056, 8192]
GEOMETRY = [("8/420", w, HEIGHTS[i % 4]) for i, w in enumerate(WIDTHS8)] + [("10/420", w, HEIGHTS[(i + 1) % 4]) for i, w in enumerate(WIDTHS10)] + \
           [("8/422", w, HEIGHTS[(i + 2) % 4]) for i, w in enumerate(WIDTHS8[1::3])] + [("10/422", w, HEIGHTS[(i + 3) % 4]) for i, w in enumerate(WIDTHS10[1::3])]
MIXES = {"both": BOTH, "corpus": CORPUS, "cb_only": ((32, 32, 0), None), "cr_only": (None, (64, 0, 0)), "saturating": SAT}


def records_of(name):
    return T.load_trace(name) if name.startswith("fgs_") else MP.program(name)


def case(key):
    """-> dict(name, mixes, frames, seeds, shift, cap): the input of one GPU comparison"""
    kind = key[0]
    seeds, shift, cap = None, 0, 0
    if kind == "class":                 # every kernel instantiation: 3 frames of 1032 x 90 (a ragged last block row)
        name, mixes = NAMES[key[1]], BOTH
        dims, n, seed, rng = (1032, 90), 3, 10, {}
    elif kind == "mix":                 # every mix at both depths, P010 high-aligned at 10 bit
        name, mixes = NAMES[key[2]], MIXES[key[1]]
        dims, n, seed = (520, 70), 2, 20
        rng = CORPUS_RANGE if key[1] == "corpus" else {}
        shift = 6 if key[2].startswith("10") else 0
        cap = 3 if key[1] == "saturating" else 0
    elif kind == "clamp":               # CLAMP_NAMES above
        name, mixes = CLAMP_NAMES[key[2]], CLAMP_MIXES[key[1]]
        dims, n, seed, rng, cap = (520, 70), 2, 20, {}, 3
        shift = 6 if key[2] == 10 else 0
    elif kind == "geometry":
        name, mixes = NAMES[key[1]], BOTH
        dims, n, seed, rng = (key[2], key[3]), 2, key[2] + key[3], {}
    elif kind == "high":                # P010 / P210, random low bits
        name, mixes = NAMES[key[1]], CORPUS if key[1] == "10/420" else BOTH
        dims, n, seed, shift = (1032, 90), 2, 40, 6
        rng = CORPUS_RANGE if key[1] == "10/420" else {}
    elif kind == "place":
        name, mixes = NAMES[key[1]], BOTH
        dims, n, seed, rng = (2056, 70), 3, 50, {}
        shift = 6 if key[1].startswith("10") else 0
        seeds = [7, 0x80000000, 7]
    elif kind == "many":                # 35 frames = launches of 32 + 3
        name, mixes = NAMES["8/420"], BOTH
        dims, n, seed, rng = (264, 40), 35, 700, {}
        seeds = [int(s) for s in np.random.default_rng(3).integers(0, 1 << 32, 35)] if key[1] else None
    elif kind == "region":
        name, mixes = NAMES["10/420"], BOTH
        dims, n, seed, rng, shift = (520, 70), key[1], 80 + key[1], {}, 6
        seeds = [11, 22, 33] if key[1] == 3 else None
    elif kind == "fronts":              # three P010 frames of 8192 x 1366: 2 x (Y + UV) >= 64 MiB (test_gpu_semiplanar.py test_two_frame_fronts)
        name, mixes = NAMES["10/420"], BOTH
        dims, n, seed, rng, shift = (8192, key[1]), key[2], 60, {}, 6
    elif kind == "sequence":
        name, mixes = NAMES["10/420"], BOTH
        dims, n, seed, rng, shift = (520, 70), key[1], 100 * key[1], {}, key[2]
        seeds = key[3]
    elif kind == "firmware":
        name, mixes = NAMES[key[1]], CORPUS
        dims, n, seed, rng = (520, 70), 2, 8, CORPUS_RANGE
        shift = 6 if key[1].startswith("10") else 0
    elif kind == "full":                # full-range content
        name, mixes = NAMES[key[1]], BOTH
        dims, n, seed, rng, cap = (520, 70), 3, 90, dict(lo=0.0, hi=1.0), 3
    elif kind == "neutral":             # content over the whole in-range span
        name, mixes = NAMES[key[1]], (X.NEUTRAL, X.NEUTRAL)
        dims, n, seed, rng = (1032, 90), 2, 4, dict(lo=0.0, hi=1.0)
    else:
        raise KeyError(key)
    rec = records_of(name)
    depth, sx, sy = T.trace_geometry(rec)
    assert sx == 2
    frames = M.ranged_sp_frames(*dims, depth, sy, shift, n, seed, **rng)
    return dict(name=name, rec=rec, mixes=mixes, frames=frames, seeds=seeds, shift=shift, depth=depth, suby=sy,
                cap=cap * M.chroma_samples(frames) // 100)


CASE_KEYS = [("class", k) for k in NAMES] + [("mix", m, d) for m in MIXES for d in ("8/420", "10/420")] + \
            [("geometry", g, w, h) for g, w, h in GEOMETRY] + [("high", "10/420"), ("high", "10/422")] + \
            [("place", "8/420"), ("place", "10/422")] + [("many", False), ("many", True)] + [("region", 4), ("region", 3)] + \
            [("fronts", 1366, 3), ("fronts", 1360, 2)] + [("sequence", 5, 6, None), ("sequence", 1, 0, None), ("sequence", 4, 6, (5, 0, 0xC0FFEE, 5))] + \
            [("firmware", "10/420"), ("firmware", "8/420")] + [("full", "8/420"), ("full", "10/420")] + \
            [("clamp", e, d) for e in CLAMP_MIXES for d in CLAMP_NAMES]
# (the "neutral" cases are compared byte for byte with the mix switched off, not through the derivation: they have no cap)


# ---- the GPU side -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


def program(hip, c, mixes="case"):
    """-> an oracle in the same programmed state"""
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, c["rec"])
    for k, m in enumerate(c["mixes"] if mixes == "case" else mixes, 1):
        if m is not None:
            hip.set_chroma_mix(k, *m)
    ora = T.OracleHW()
    T.replay(ora, c["rec"])
    return ora


def expect(ora, c):
    res, excluded = M.expected(ora, c["rec"], c["frames"], c["seeds"], c["shift"], c["mixes"])
    print(f"excluded by the derivation: {excluded} of {M.chroma_samples(c['frames'])} chroma samples (cap {c['cap']})")
    assert excluded <= c["cap"], (excluded, c["cap"])
    return res


def launches(hip):
    return (hip.last_launch_info() or {"launches": 0})["launches"]


def kernel_name(c):
    return T.kernel_name("grain_sp_mix_kernel", c["depth"], c["suby"])


def check(devs, res, what=""):
    for i, (d, (want, mask)) in enumerate(zip(devs, res)):
        n = M.mismatches(d.download(), want, mask)
        assert n == 0, f"{what} frame {i}: {n} containers differ from the expectation"


def call(hip, c, src, dst=None, stream=None):
    from gpu_util import stream_ptr
    f0 = c["frames"][0]
    hip.add_grain_sp_frame_list_dev([d.ptrs() for d in src], None if dst is None else [d.ptrs() for d in dst], c["seeds"], f0.width, f0.height,
                                    f0.stride, f0.uv_stride, c["shift"], stream_ptr() if stream is None else stream)


def run_in_place(hip, key, shuffle=0, ora=None, c=None):
    """program (unless an oracle comes along: the sequence goes on), expect, call in place, compare everything"""
    from test_gpu_semiplanar import scattered
    c = c or case(key)
    if ora is None:
        ora = program(hip, c)
    res = expect(ora, c)
    devs = scattered(c["frames"], shuffle)
    call(hip, c, devs)
    check(devs, res, str(key))
    assert hip.seed_state() == ora.seed_state()
    return c, devs, res, ora


@pytest.mark.parametrize("fmt", list(NAMES))
def test_every_kernel_instantiation(hip, fmt):
    n0 = launches(hip)
    c, *_ = run_in_place(hip, ("class", fmt))
    info = hip.last_launch_info()
    assert info["kernel"] == kernel_name(c) and info["one_y"] == 1 and info["one_c"] == 1, info
    assert info["launches"] - n0 == 2 and info["nframes"] == 3 and info["listed"] == 1 and info["in_place"] == 1, info     # in place: UV, then luma
    assert info["lds_bytes_per_workgroup"] == 53248, info


@pytest.mark.parametrize("fmt", ["8/420", "10/420"])
@pytest.mark.parametrize("mix", list(MIXES))
def test_mixes(hip, mix, fmt):
    c, *_ = run_in_place(hip, ("mix", mix, fmt), shuffle=1)
    assert hip.last_launch_info()["kernel"] == kernel_name(c)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("end", ["hi", "lo"])
def test_the_clamp_of_the_index_is_compared(hip, end, depth):
    """CLAMP_NAMES / CLAMP_MIXES: a share of the samples whose index is clipped to an end of the range stays in the comparison"""
    c, devs, res, _ = run_in_place(hip, ("clamp", end, depth), shuffle=1)
    sat, compared = M.saturated_samples(c["frames"], c["mixes"], [m for _, m in res])
    print(f"saturated index samples: {sat}, of them compared: {compared}")
    assert sat > 0 and compared >= sat // 8, (sat, compared)
    assert hip.last_launch_info()["kernel"] == kernel_name(c)


@pytest.mark.parametrize("fmt,width,height", GEOMETRY)
def test_row_geometry(hip, fmt, width, height):
    c, *_ = run_in_place(hip, ("geometry", fmt, width, height), shuffle=2)
    info = hip.last_launch_info()
    unit_samples = 64 * 32 // (2 if c["depth"] > 8 else 1)     # containers of a UV position
    nblk = (width + 15) // 16
    assert info["kernel"] == kernel_name(c) and info["positions_per_row"][1] == (-(-nblk * 16 // (unit_samples // 64)) + 64) // 64, info


def test_geometry_covers_every_width_and_height():
    assert {w for g, w, _ in GEOMETRY if g == "8/420"} == set(WIDTHS8) and {w for g, w, _ in GEOMETRY if g == "10/420"} == set(WIDTHS10)
    assert {h for _, _, h in GEOMETRY} == set(HEIGHTS) and {g for g, _, _ in GEOMETRY} == set(NAMES)


@pytest.mark.parametrize("fmt", ["10/420", "10/422"])
def test_high_aligned_samples(hip, fmt):
    """P010 / P210: random low bits in Y and UV give what zero low bits give; the written containers' low bits are zero"""
    from test_gpu_semiplanar import scattered
    c, devs, res, _ = run_in_place(hip, ("high", fmt), shuffle=1)
    frames = c["frames"]
    assert any((f.Y & 63).any() for f in frames) and any((f.UV & 63).any() for f in frames)
    rows, crows, cols = SP.written_region(frames[0])
    got = [d.download() for d in devs]
    for g in got:
        assert not (g.Y[:rows, :cols] & 63).any() and not (g.UV[:crows, :cols] & 63).any()
    clean = []
    for f in frames:
        z = f.copy()
        z.Y &= 0xffc0
        z.UV &= 0xffc0
        clean.append(z)
    c2 = dict(c, frames=clean)
    program(hip, c2)
    devs2 = scattered(clean, 2)
    call(hip, c2, devs2)
    for a, b in zip(got, [d.download() for d in devs2]):
        assert np.array_equal(a.Y[:rows, :cols], b.Y[:rows, :cols]) and np.array_equal(a.UV[:crows, :cols], b.UV[:crows, :cols])


@pytest.mark.parametrize("fmt", ["8/420", "10/422"])
def test_placement(hip, fmt):
    """in place (two launches) == out of place (one launch) == destination Y the source Y with UV elsewhere (two launches), byte for byte in
    what is written; sources of out-of-place planes stay, destination padding is never written; a seed per picture"""
    from test_gpu_semiplanar import DevSP, scattered
    c, devs, res, ora = run_in_place(hip, ("place", fmt))
    inplace = [d.download() for d in devs]
    frames = c["frames"]
    f0 = frames[0]
    rows, crows, cols = SP.written_region(f0)
    fill = M.ranged_sp_frames(f0.width, f0.height, c["depth"], c["suby"], c["shift"], 1, 999)[0]

    def filled(want):
        e = fill.copy()
        e.Y[:rows, :cols] = want.Y[:rows, :cols]
        e.UV[:crows, :cols] = want.UV[:crows, :cols]
        return e

    # out of place
    program(hip, c)
    src, dst = scattered(frames, 6), [DevSP(fill) for _ in frames]
    n0 = launches(hip)
    call(hip, c, src, dst)
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 1 and info["in_place"] == 0 and info["kernel"] == kernel_name(c), info
    check(dst, [(filled(w), m) for w, m in res], "out of place")
    for s, f in zip(src, frames):
        assert s.download().equal_all(f), "the source of an out-of-place call changed"
    for d, g in zip(dst, inplace):
        o = d.download()
        assert np.array_equal(o.Y[:rows, :cols], g.Y[:rows, :cols]) and np.array_equal(o.UV[:crows, :cols], g.UV[:crows, :cols])
    assert hip.seed_state() == ora.seed_state()
    # destination Y == source Y, UV elsewhere: luma is still a hazard
    program(hip, c)
    src = scattered(frames, 7)
    dst = []
    for s in src:
        d = DevSP(fill)
        d.Y = s.Y
        dst.append(d)
    n0 = launches(hip)
    call(hip, c, src, dst)
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 2 and info["kernel"] == kernel_name(c), info
    for i, (s, d, f, (w, m)) in enumerate(zip(src, dst, frames, res)):
        e = filled(w)
        e.Y[...] = w.Y                      # (the luma plane is the source's own: its padding too)
        assert M.mismatches(d.download(), e, m) == 0, f"partially in place, frame {i}"
        assert np.array_equal(s.download().UV, f.UV), "the UV source of a partially in-place call changed"
    assert hip.seed_state() == ora.seed_state()


@pytest.mark.parametrize("seeded", [False, True])
def test_more_frames_than_one_launch_holds(hip, seeded):
    """35 frames = launches of 32 + 3, each UV first, then luma"""
    n0 = launches(hip)
    c, *_ = run_in_place(hip, ("many", seeded), shuffle=3)
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 4 and info["nframes"] == 3 and info["kernel"] == kernel_name(c), info
    assert hip.seeded_stream_stats()["last_launch_used_it"] == seeded


def test_two_calls_inside_an_overlap_region(hip):
    from gpu_util import stream_ptr
    from test_gpu_semiplanar import scattered
    a, b = case(("region", 4)), case(("region", 3))
    ora = program(hip, a)
    ra, rb = expect(ora, a), expect(ora, b)
    da, db = scattered(a["frames"], 8), scattered(b["frames"], 9)
    st = stream_ptr()
    hip.overlap_begin(st)
    call(hip, a, da, stream=st)
    call(hip, b, db, stream=st)
    hip.overlap_end(st)
    check(da, ra, "first call")
    check(db, rb, "second call")
    assert hip.seed_state() == ora.seed_state()


def test_two_frame_fronts(hip):
    c, *_ = run_in_place(hip, ("fronts", 1366, 3), shuffle=5)
    info = hip.last_launch_info()
    assert info["frames_per_front"] == 2 and info["nframes"] == 3 and info["kernel"] == kernel_name(c), info
    run_in_place(hip, ("fronts", 1360, 2))
    assert hip.last_launch_info()["frames_per_front"] == 1


@pytest.mark.parametrize("fmt", ["8/420", "10/420"])
def test_neutral_mix_equals_mix_off_and_clear_and_reset_bring_todays_kernel_back(hip, fmt):
    from test_gpu_semiplanar import scattered
    c = case(("neutral", fmt))
    out = {}
    for tag in ("off", "neutral", "clear", "reset"):
        program(hip, c, (None, None) if tag == "off" else c["mixes"])
        if tag == "clear":
            hip.clear_chroma_mix()
        if tag == "reset":
            hip.lib.vfgs_hip_reset_state()
            T.replay(hip, c["rec"])
        devs = scattered(c["frames"], 4)
        n0 = launches(hip)
        call(hip, c, devs)
        info = hip.last_launch_info()
        out[tag] = [d.download() for d in devs], hip.seed_state(), info["kernel"], info["launches"] - n0
    assert out["neutral"][2] == kernel_name(c) and out["neutral"][3] == 2
    for tag in ("off", "clear", "reset"):
        assert out[tag][2].startswith("grain_sp_kernel<") and out[tag][3] == 1, out[tag][2:]
        assert all(a.equal_all(b) for a, b in zip(out[tag][0], out["neutral"][0])) and out[tag][1] == out["neutral"][1], tag
    ora = T.OracleHW()
    T.replay(ora, c["rec"])
    for g, w in zip(out["off"][0], SP.expected(ora, c["frames"], None, 0)):
        assert g.equal_all(w)


def test_one_seed_sequence_across_entry_points(hip):
    """a planar frame under the mix, a semi-planar list without seeds, a planar list under the mix, vfgs_set_seed + a semi-planar list of one,
    a seeded semi-planar list, a planar frame: the registers equal the oracle's after each step"""
    from gpu_util import DevFrame, stream_ptr
    c0 = case(("sequence", 5, 6, None))
    ora = program(hip, c0)
    rec, depth, sy = c0["rec"], c0["depth"], c0["suby"]
    legal = X.legal_range(rec)
    W, H = 520, 70

    def planar(n, seed):
        fr = X.ranged_frames(W, H, depth, 2, sy, n, seed)
        dev = [DevFrame(f) for f in fr]
        if n == 1:
            hip.add_grain_frame_dev(*dev[0].ptrs(), W, H, fr[0].stride, fr[0].cstride, stream_ptr())
        else:
            hip.add_grain_frame_list_dev([d.ptrs() for d in dev], W, H, fr[0].stride, fr[0].cstride, stream_ptr())
        assert hip.last_launch_info()["kernel"].startswith("grain_mix_kernel<")
        for d, f in zip(dev, fr):
            fi = X.index_frame(f, BOTH)
            o = fi.copy()
            ora.add_grain_frame(o)
            want, masks, ex = X.expect_from(f, fi, o, legal)
            assert ex == 0 and X.mismatches(d.download(), want, masks) == 0
        assert hip.seed_state() == ora.seed_state()

    planar(1, 1)
    run_in_place(hip, None, shuffle=1, ora=ora, c=c0)
    assert not hip.seeded_stream_stats()["last_launch_used_it"]
    planar(3, 2)
    hip.set_seed(777); ora.set_seed(777)
    run_in_place(hip, None, ora=ora, c=case(("sequence", 1, 0, None)))
    run_in_place(hip, None, shuffle=3, ora=ora, c=case(("sequence", 4, 6, (5, 0, 0xC0FFEE, 5))))
    planar(1, 3)


@pytest.mark.parametrize("fmt", ["10/420", "8/420"])
def test_firmware_path_programs_the_mix_the_call_uses(hip, fmt):
    """vfgs_init_afgs1 with the chroma mix switched on programs the corpus mix; a semi-planar call then uses it"""
    from test_gpu_chroma_mix import firmware_program
    from test_gpu_semiplanar import scattered
    from versatilefilmgrain_amd import fw
    c = case(("firmware", fmt))
    try:
        fw.afgs1_chroma_mix(True)
        firmware_program(hip, c["name"])
        assert (hip.chroma_mix(1), hip.chroma_mix(2)) == (CORPUS[0] + (1,), CORPUS[1] + (1,))
        ora = T.OracleHW()
        T.replay(ora, c["rec"])
        res = expect(ora, c)
        devs = scattered(c["frames"], 2)
        call(hip, c, devs)
        check(devs, res)
        assert hip.seed_state() == ora.seed_state() and hip.last_launch_info()["kernel"] == kernel_name(c)
    finally:
        fw.afgs1_chroma_mix(False)


@pytest.mark.parametrize("fmt", ["8/420", "10/420"])
def test_full_range_content(hip, fmt):
    """the derivation may leave out at most 3 % of the chroma samples (asserted on the oracle, here and on the CPU)"""
    run_in_place(hip, ("full", fmt))


def test_refusals_under_a_mix_change_nothing(hip):
    """a general-form model under a mix: 40; depth 12 under a mix: 40; the cause in the message; registers, launch count and bytes as they
    were; then the same list is served"""
    from gpu_util import stream_ptr
    from test_gpu_semiplanar import scattered
    from versatilefilmgrain_amd.hw import VfgsHipError
    c = case(("mix", "both", "10/420"))
    frames, seeds = c["frames"], [1, 2]
    f0 = frames[0]
    geo = (f0.width, f0.height, f0.stride, f0.uv_stride)
    devs = scattered(frames)
    ptrs = [d.ptrs() for d in devs]
    st = stream_ptr()

    def refused(match, sd, shift):
        st0, n0 = hip.seed_state(), launches(hip)
        with pytest.raises(VfgsHipError, match=match):
            hip.add_grain_sp_frame_list_dev(ptrs, None, sd, *geo, shift, st)
        assert hip.lib.vfgs_hip_last_error() == 40
        assert hip.seed_state() == st0 and launches(hip) == n0

    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, T.load_trace("fgs_sei_10_420"))       # eight luma patterns: a general-form bank
    hip.set_chroma_mix(1, 32, 32, 0)
    for sd in (seeds, None):
        refused("error 40:.*chroma mix.*general-form", sd, 6)
    program(hip, c)
    hip.set_depth(12)
    for sd in (seeds, None):
        refused("error 40:.*chroma mix.*depth is 12", sd, 4)
    for d, f in zip(devs, frames):
        assert d.download().equal_all(f)
    c = dict(c, seeds=seeds)
    ora = program(hip, c)
    res = expect(ora, c)
    call(hip, c, devs)
    check(devs, res)
    assert hip.seed_state() == ora.seed_state()
