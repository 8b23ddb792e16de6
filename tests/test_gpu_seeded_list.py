"""GPU (MI355X): vfgs_hip_add_grain_frame_list_seeded_* -- a list of frames with a seed per picture in ONE launch -- against the
oracle, through the C ABI, bit for bit (every sample of every plane, padding included, and the four seed registers).

The contract (include/vfgs_hip.h): samples and registers are those of `vfgs_set_seed(seeds[f]); vfgs_hip_add_grain_frame_dev(frame f)`
for every f in list order, so the ground truth everywhere is the oracle run as that loop.  Every frame is an allocation of its own,
listed out of address order (the helpers of tests/test_gpu_frame_list.py).  The kernels are the unseeded lists' -- what differs is
where a frame's LFSR windows lie in the image the launch reads -- so the cases reach every kernel class that computes a stream
position: general and one-pattern forms at every depth, persistent luma workgroups, rows walked in parts, two frame fronts, the
narrowed destination, the kernels of the chroma mix, parts that begin below line 0."""
import numpy as np
import pytest

import vfgs_testlib as T
from gpu_util import DevFrame, stream_ptr
from test_gpu_frame_list import FORMATS, garbage_frame, program, scattered

pytestmark = pytest.mark.gpu

SEVEN = [0, 0x80000000, 0xFFFFFFFF, 12345, 12345, 0x5eed1e55, 0x0badf00d]     # (the first two both load register 0; a repeated neighbour)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.lib.vfgs_hip_reset_state()


def fresh_seeds(n, seed):
    return [int(s) for s in np.random.default_rng(seed).integers(0, 1 << 32, n)]


def oracle_loop(ora, frames, seeds):
    """the contract's loop on copies of the frames"""
    want = [f.copy() for f in frames]
    for w, s in zip(want, seeds):
        ora.set_seed(s)
        ora.add_grain_frame(w)
    return want


def launches(hip):
    return (hip.last_launch_info() or {"launches": 0})["launches"]


def run_seeded(hip, ora, frames, seeds, shuffle=0, stream=None):
    """frames through the seeded list entry (in place) vs the oracle's loop; returns the device frames"""
    want = oracle_loop(ora, frames, seeds)
    dev = scattered(frames, shuffle)
    f0 = frames[0]
    hip.add_grain_frame_list_seeded_dev([d.ptrs() for d in dev], seeds, f0.width, f0.height, f0.stride, f0.cstride, stream_ptr() if stream is None else stream)
    for i, (d, w) in enumerate(zip(dev, want)):
        assert d.download().equal_all(w), i
    assert hip.seed_state() == ora.seed_state()
    assert hip.seeded_stream_stats()["last_launch_used_it"]
    return dev


@pytest.mark.parametrize("name", FORMATS + ["fgs_sei_10_420@depth12"])
def test_every_format(hip, name):
    if name.endswith("@depth12"):
        import test_gpu_depth12 as D
        rec = D.records12(name.split("@")[0])
        D.program(hip, rec)
        ora, (depth, sx, sy) = D.oracle_for(rec), T.trace_geometry(rec)
        assert depth == 12
    else:
        ora, (depth, sx, sy) = program(hip, name)
    frames = [garbage_frame(1032, 90, depth, sx, sy, 10 + i) for i in range(7)]
    n0, built0 = launches(hip), hip.seeded_stream_stats()["images_built"]
    run_seeded(hip, ora, frames, SEVEN)
    info, st = hip.last_launch_info(), hip.seeded_stream_stats()
    assert info["launches"] - n0 == 1 and info["nframes"] == 7 and info["listed"] == 1 and info["in_place"] == 1 and info["depth"] == depth, info
    # 65 blocks x 6 block rows: ceil((32 + 65 + 390 + 64) / 32) + 1 words per frame
    assert st["images_built"] - built0 == 1 and st["image_words"] == 7 * 19 and st["last_launch_used_it"], st


def test_one_seed_sequence_across_entry_points(hip):
    """unseeded frame, seeded list, unseeded list (continues the last picture's stream), vfgs_set_seed + frame, seeded list of one, a frame in two
    stripes, seeded list"""
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    W, H = 520, 70
    mk = lambda n, s: [garbage_frame(W, H, depth, sx, sy, s + i) for i in range(n)]

    def one_frame(s, stripes=False):
        f = mk(1, s)[0]
        w = f.copy(); ora.add_grain_frame(w)
        d = DevFrame(f)
        if stripes:
            hip.add_grain_stripe_dev(*d.ptrs(0), 0, W, 32, f.stride, f.cstride, stream_ptr())
            hip.add_grain_stripe_dev(*d.ptrs(32), 32, W, H - 32, f.stride, f.cstride, stream_ptr())
        else:
            hip.add_grain_frame_dev(*d.ptrs(), W, H, f.stride, f.cstride, stream_ptr())
        assert d.download().equal_all(w)
        assert hip.seed_state() == ora.seed_state()

    one_frame(0)
    run_seeded(hip, ora, mk(5, 100), fresh_seeds(5, 1), shuffle=1)
    fr = mk(3, 200)
    want = [f.copy() for f in fr]
    for w in want:
        ora.add_grain_frame(w)
    dev = scattered(fr, 2)
    hip.add_grain_frame_list_dev([d.ptrs() for d in dev], W, H, fr[0].stride, fr[0].cstride, stream_ptr())
    for d, w in zip(dev, want):
        assert d.download().equal_all(w)
    assert hip.seed_state() == ora.seed_state() and not hip.seeded_stream_stats()["last_launch_used_it"]
    hip.set_seed(777); ora.set_seed(777)
    one_frame(300)
    run_seeded(hip, ora, mk(1, 400), [0xC0FFEE])
    one_frame(500, stripes=True)
    run_seeded(hip, ora, mk(4, 600), fresh_seeds(4, 2), shuffle=3)


def test_more_frames_than_one_launch_holds(hip):
    """70 frames = launches of 32 + 32 + 6, each with its slice of the seeds"""
    ora, (depth, sx, sy) = program(hip, "fgs_afgs1_test1_8_420")
    frames = [garbage_frame(264, 40, depth, sx, sy, 700 + i) for i in range(70)]
    n0 = launches(hip)
    run_seeded(hip, ora, frames, fresh_seeds(70, 3), shuffle=3)
    info = hip.last_launch_info()
    assert info["launches"] - n0 == 3 and info["nframes"] == 6 and info["listed"] == 1, info


def test_persistent_luma_workgroups(hip):
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    frames = [garbage_frame(256, 1100, depth, sx, sy, 900 + i) for i in range(32)]
    run_seeded(hip, ora, frames, fresh_seeds(32, 4), shuffle=4)
    info = hip.last_launch_info()
    assert info["persistent_luma_workgroups"] > 0 and info["nframes"] == 32, info


@pytest.mark.parametrize("name", ["fgs_afgs1_test1_8_420", "fgs_sei_10_420"])
def test_rows_walked_in_parts(hip, name):
    ora, (depth, sx, sy) = program(hip, name)
    frames = [garbage_frame(8200, 40, depth, sx, sy, 20 + i) for i in range(3)]
    run_seeded(hip, ora, frames, fresh_seeds(3, 5), shuffle=5)
    assert hip.last_launch_info()["parts_per_row"] == 2


def test_two_frame_fronts(hip):
    """4320p, an odd count: frames 2m and 2m + 1 are swept together, each at its own seed's stream"""
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    frames = [garbage_frame(7680, 4320, depth, sx, sy, 50 + i) for i in range(3)]
    run_seeded(hip, ora, frames, fresh_seeds(3, 6), shuffle=5)
    info = hip.last_launch_info()
    assert info["frames_per_front"] == 2 and info["listed"] == 1, info


@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_8_420", "fgs_sei_10_444"])
def test_stripe_split(hip, name):
    """Three ranks' parts of every listed frame, each from a freshly programmed state with the same seeds: the parts together are the whole
    frames, and every rank leaves the registers of whole frames (a part that begins below line 0 reads the row above it too)"""
    ora, (depth, sx, sy) = program(hip, name)
    W, H = 1032, 150
    frames = [garbage_frame(W, H, depth, sx, sy, 40 + i) for i in range(5)]
    seeds = fresh_seeds(5, 7)
    want = oracle_loop(ora, frames, seeds)
    dev = scattered(frames, 12)
    f0 = frames[0]
    states = []
    for py, ph in ((0, 32), (32, 48), (80, 70)):
        program(hip, name)
        hip.add_grain_frame_list_seeded_part_dev([d.ptrs(py) for d in dev], seeds, W, H, py, ph, f0.stride, f0.cstride, stream_ptr())
        states.append(hip.seed_state())
    assert states[0] == states[1] == states[2] == ora.seed_state()
    for i, (d, w) in enumerate(zip(dev, want)):
        assert d.download().equal_all(w), i


@pytest.mark.parametrize("name", ["fgs_sei_10_420", "fgs_afgs1_test1_8_444"])
def test_out_of_place(hip, name):
    """src[f] -> dst[f]; one pair in place; the sources stay as they were"""
    ora, (depth, sx, sy) = program(hip, name)
    frames = [garbage_frame(1032, 90, depth, sx, sy, 30 + i) for i in range(6)]
    seeds = fresh_seeds(6, 8)
    want = oracle_loop(ora, frames, seeds)
    src = scattered(frames, 6)
    blank = T.Frame(1032, 90, depth, sx, sy)
    dst = [DevFrame(blank) for _ in frames]
    dst[2] = src[2]
    f0 = frames[0]
    hip.add_grain_frame_list_seeded_copy_dev([d.ptrs() for d in src], [d.ptrs() for d in dst], seeds, f0.width, f0.height, f0.stride, f0.cstride, stream_ptr())
    cy = (f0.width + 15) // 16 * 16
    for i, (s, d, w, f) in enumerate(zip(src, dst, want, frames)):
        g = d.download()
        if i == 2:
            assert g.equal_all(w)
            continue
        assert np.array_equal(g.Y[:90, :cy], w.Y[:90, :cy]) and np.array_equal(g.U[:90 // sy, :cy // sx], w.U[:90 // sy, :cy // sx]) and np.array_equal(g.V[:90 // sy, :cy // sx], w.V[:90 // sy, :cy // sx]), i
        assert not g.Y[:, cy:].any() and not g.Y[90:].any()          # the destination's padding is never written
        assert s.download().equal_all(f), i
    assert hip.seed_state() == ora.seed_state()
    assert hip.last_launch_info()["in_place"] == 0


def test_8bit_output(hip):
    import torch
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    W, H = 1032, 70
    frames = [garbage_frame(W, H, depth, sx, sy, 60 + i) for i in range(5)]
    for f in frames:
        for p in f.planes():
            np.minimum(p, 0xfffd, out=p)
    seeds = fresh_seeds(5, 9)
    want = oracle_loop(ora, frames, seeds)
    src = scattered(frames, 7)
    f8 = T.Frame(W, H, 8, sx, sy)
    dst = [tuple(torch.full(p.shape, 0x5a, dtype=torch.uint8, device="cuda") for p in f8.planes()) for _ in frames]
    f0 = frames[0]
    hip.add_grain_frame_list_seeded_copy8_dev([d.ptrs() for d in src], [tuple(t.data_ptr() for t in d) for d in dst], seeds, W, H, f0.stride, f0.cstride,
                                              f8.stride, f8.cstride, stream_ptr())
    torch.cuda.synchronize()
    nblk = (W + 15) // 16
    for i, (w, d) in enumerate(zip(want, dst)):
        for got, w16, rows, cols in ((d[0], w.Y, H, nblk * 16), (d[1], w.U, H // sy, nblk * 16 // sx), (d[2], w.V, H // sy, nblk * 16 // sx)):
            g = got.cpu().numpy()
            exp = ((w16[:rows, :cols].astype(np.int32) + 2) >> 2).astype(np.uint8)
            assert np.array_equal(g[:rows, :cols], exp), i
            assert (g[rows:] == 0x5a).all() and (g[:, cols:] == 0x5a).all(), i
    assert hip.seed_state() == ora.seed_state()
    info = hip.last_launch_info()
    assert info["out8"] == 1 and info["listed"] == 1


def test_two_seeded_lists_inside_an_overlap_region(hip):
    ora, (depth, sx, sy) = program(hip, "fgs_sei_ar_test1_10_420")
    a = [garbage_frame(520, 70, depth, sx, sy, 80 + i) for i in range(4)]
    b = [garbage_frame(520, 70, depth, sx, sy, 90 + i) for i in range(3)]
    seeds = fresh_seeds(7, 10)
    want = oracle_loop(ora, a + b, seeds)
    da, db = scattered(a, 8), scattered(b, 9)
    st = stream_ptr()
    hip.overlap_begin(st)
    hip.add_grain_frame_list_seeded_dev([d.ptrs() for d in da], seeds[:4], 520, 70, a[0].stride, a[0].cstride, st)
    hip.add_grain_frame_list_seeded_dev([d.ptrs() for d in db], seeds[4:], 520, 70, a[0].stride, a[0].cstride, st)
    hip.overlap_end(st)
    for i, (d, w) in enumerate(zip(da + db, want)):
        assert d.download().equal_all(w), i
    assert hip.seed_state() == ora.seed_state()


def test_more_calls_in_flight_than_the_ring_has_slots(hip, monkeypatch):
    """Behind one launch of three 4320p frames, nine seeded lists on two streams with nothing synchronised in between, every image in a
    slot of its own (VFGS_HIP_SEEDED_SLOT_KB=0): the ring of four turns over twice while the first images still wait for their kernels,
    and no slot may be overwritten before they have run"""
    import torch
    monkeypatch.setenv("VFGS_HIP_SEEDED_SLOT_KB", "0")
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    big = [garbage_frame(7680, 4320, depth, sx, sy, 150 + i) for i in range(3)]
    small = [[garbage_frame(520, 70, depth, sx, sy, 1000 + 10 * c + i) for i in range(3)] for c in range(9)]
    seeds = [fresh_seeds(3, 20 + c) for c in range(9)]
    want_big = [f.copy() for f in big]
    for w in want_big:
        ora.add_grain_frame(w)
    want = [oracle_loop(ora, fr, s) for fr, s in zip(small, seeds)]
    dbig = scattered(big, 1)
    dev = [scattered(fr, c) for c, fr in enumerate(small)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    st0 = hip.seeded_stream_stats()
    hip.add_grain_frame_list_dev([d.ptrs() for d in dbig], 7680, 4320, big[0].stride, big[0].cstride, streams[0].cuda_stream)
    for c in range(9):
        f0 = small[c][0]
        hip.add_grain_frame_list_seeded_dev([d.ptrs() for d in dev[c]], seeds[c], 520, 70, f0.stride, f0.cstride, streams[c & 1].cuda_stream)
    st1 = hip.seeded_stream_stats()
    torch.cuda.synchronize()
    print("seeded stream stats:", st0, "->", st1)
    assert st1["images_built"] - st0["images_built"] == 9
    for i, (d, w) in enumerate(zip(dbig, want_big)):
        assert d.download().equal_all(w), i
    for c in range(9):
        for i, (d, w) in enumerate(zip(dev[c], want[c])):
            assert d.download().equal_all(w), (c, i)
    assert hip.seed_state() == ora.seed_state()


def test_chroma_mix_active(hip):
    """fgs_afgs1_test1_10_420 with a mix on Cb and on Cr, in place (two launches that read one image): against the model of
    tests/chroma_mix_util.py -- the unchanged oracle on the index frames -- run with the per-frame seeds"""
    import chroma_mix_util as X
    name, mixes = "fgs_afgs1_test1_10_420", ((64, 119, -238), (64, 101, -202))
    rec = T.load_trace(name)
    depth, sx, sy = T.trace_geometry(rec)
    frames = X.ranged_frames(1032, 90, depth, sx, sy, 5, 11, lo=0.4, hi=0.6, clo=0.4, chi=0.5)
    seeds = fresh_seeds(5, 12)
    ora = T.OracleHW()
    T.replay(ora, rec)
    res, excluded = [], 0
    for f, s in zip(frames, seeds):
        fi = X.index_frame(f, mixes)
        out = fi.copy()
        ora.set_seed(s)
        ora.add_grain_frame(out)
        want, masks, ex = X.expect_from(f, fi, out, X.legal_range(rec))
        res.append((want, masks))
        excluded += ex
    assert excluded == 0
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, rec)
    try:
        for c, m in enumerate(mixes, 1):
            hip.set_chroma_mix(c, *m)
        dev = scattered(frames, 13)
        n0 = launches(hip)
        hip.add_grain_frame_list_seeded_dev([d.ptrs() for d in dev], seeds, 1032, 90, frames[0].stride, frames[0].cstride, stream_ptr())
        for i, (d, (want, masks)) in enumerate(zip(dev, res)):
            assert X.mismatches(d.download(), want, masks) == 0, i
        assert hip.seed_state() == ora.seed_state()
        info = hip.last_launch_info()
        assert info["kernel"].startswith("grain_mix_kernel<10,2,2,") and info["launches"] - n0 == 2 and info["nframes"] == 5, info
        assert hip.seeded_stream_stats()["last_launch_used_it"]
    finally:
        hip.clear_chroma_mix()


def test_refusals_change_nothing(hip):
    """... in particular they do not reseed"""
    from versatilefilmgrain_amd.hw import VfgsHipError
    ora, (depth, sx, sy) = program(hip, "fgs_sei_10_420")
    frames = [garbage_frame(520, 70, depth, sx, sy, i) for i in range(3)]
    dev = scattered(frames)
    f0 = frames[0]
    geo = (f0.width, f0.height, f0.stride, f0.cstride, stream_ptr())
    seeds = fresh_seeds(3, 14)
    st0 = hip.seed_state()
    ptrs = [d.ptrs() for d in dev]
    with pytest.raises(VfgsHipError, match="error 39"):
        hip.add_grain_frame_list_seeded_dev(ptrs, None, *geo)
    with pytest.raises(VfgsHipError, match="error 39"):
        hip.add_grain_frame_list_seeded_copy_dev(ptrs, ptrs, None, *geo)
    with pytest.raises(VfgsHipError, match="listed twice"):
        hip.add_grain_frame_list_seeded_dev([ptrs[0], ptrs[1], ptrs[0]], seeds, *geo)
    with pytest.raises(VfgsHipError, match="null plane"):
        hip.add_grain_frame_list_seeded_dev([ptrs[0], (ptrs[1][0], 0, ptrs[1][2])], seeds[:2], *geo)
    with pytest.raises(VfgsHipError, match="16-byte aligned"):
        hip.add_grain_frame_list_seeded_dev([ptrs[0], (ptrs[1][0] + 8, ptrs[1][1], ptrs[1][2])], seeds[:2], *geo)
    with pytest.raises(VfgsHipError, match="multiple of 16"):
        hip.add_grain_frame_list_seeded_part_dev([d.ptrs(24) for d in dev], seeds, f0.width, f0.height, 24, 16, f0.stride, f0.cstride, stream_ptr())
    with pytest.raises(VfgsHipError, match="error 16"):     # the narrowed destination of an 8-bit path
        hip.set_depth(8)
        try:
            hip.add_grain_frame_list_seeded_copy8_dev(ptrs, ptrs, seeds, f0.width, f0.height, f0.stride, f0.cstride, f0.stride, f0.cstride, stream_ptr())
        finally:
            hip.set_depth(10)
    try:
        hip.set_chroma_mix(1, 32, 32, 0)      # the default SEI model selects its patterns by intensity: a general-form bank
        with pytest.raises(VfgsHipError, match="error 38"):
            hip.add_grain_frame_list_seeded_dev(ptrs, seeds, *geo)
    finally:
        hip.clear_chroma_mix()
    hip.add_grain_frame_list_seeded_dev([], [], *geo)          # an empty list is no call at all ...
    hip.add_grain_frame_list_seeded_dev([], None, *geo)        # ... with or without seeds
    assert hip.seed_state() == st0
    for d, f in zip(dev, frames):
        assert d.download().equal_all(f)
    # ... and the same list is served afterwards
    want = oracle_loop(ora, frames, seeds)
    hip.add_grain_frame_list_seeded_dev(ptrs, seeds, *geo)
    for d, w in zip(dev, want):
        assert d.download().equal_all(w)
    assert hip.seed_state() == ora.seed_state()
