"""CPU: the streams of a frame list with a seed per picture (vfgs_host.cpp: SeededStream; include/vfgs_hip.h:
vfgs_hip_add_grain_frame_list_seeded_*).  vfgs_hip_seed_segments hands out exactly what the library uploads for such a launch: segment f
is the stream of the register seeds[f] << 1 (vfgs_hw.c:339-344) from first_bit on.  Checked against the reference's register step
(vfgs_hw.c:74-79) stepped literally, against the generator of the stripe batches (vfgs_hip_lfsr_segments, itself checked in
tests/test_lfsr_jump_cpu.py), and -- the seed registers the entry points leave -- through the host layer over the HIP runtime model of
tests/sanitize (no GPU) against the oracle run as the contract's loop: set_seed(seeds[f]); add_grain_frame(frame f)."""
import ctypes as C
import subprocess
import sys
import time

import numpy as np
import pytest

import vfgs_testlib as T
from versatilefilmgrain_amd import fw, hw

SEEDS = [0, 1, 0x80000000, 0xFFFFFFFF, 12345, 0xdeadbeef]


@pytest.fixture(scope="module")
def hip():
    return hw.VfgsHip()


def layout(width, part_y, part_h):
    """(first_bit, seg_words) of a launch over lines [part_y, part_y + part_h), as include/vfgs_hip.h states them"""
    nblk, b = (width + 15) // 16, part_y >> 4
    nbr = ((part_y + part_h - 1) >> 4) - b + 1
    return max(b - 1, 0) * nblk, (32 + nblk + nbr * nblk + 64 + 31) // 32 + 1


def test_segments_equal_the_literal_register_steps(hip):
    """vfgs_hw.c:74-79 stepped one by one from seed << 1: 2,000 steps, every word of every segment"""
    step = T.oracle_lib().vfgs_oracle_lfsr_step
    for first, nw in ((0, 62), (7, 40), (415, 49), (1968, 1)):
        got = hip.seed_segments(SEEDS, first, nw)
        for f, seed in enumerate(SEEDS):
            r, at = (seed << 1) & 0xFFFFFFFF, 0
            for k in range(nw):
                while at < first + 32 * k:
                    r = step(r)
                    at += 1
                assert at <= 2000
                assert got[f][k] == r, (hex(seed), first, k)


@pytest.mark.parametrize("width,height,part_y,part_h", [(1920, 1080, 0, 1080), (7680, 4320, 0, 4320), (1920, 1080, 34 * 16, 200), (7680, 4320, 34 * 16, 544)])
def test_segments_equal_the_generator_of_the_stripe_batches(hip, width, height, part_y, part_h):
    first, nw = layout(width, part_y, part_h)
    seeds = SEEDS + [int(s) for s in np.random.default_rng(3).integers(0, 1 << 32, 4)]
    got = hip.seed_segments(seeds, first, nw)
    out = (C.c_uint32 * nw)()
    for f, seed in enumerate(seeds):
        assert hip.lib.vfgs_hip_lfsr_segments((seed << 1) & 0xFFFFFFFF, first, 1, 1, nw, out) == 0
        assert got[f] == list(out), hex(seed)


def test_a_distant_first_bit_is_one_jump(hip):
    """first_bit = 2^40 would be hours of stepping; and the jump composes: 2^40 + 64 is word 2 of the segment at 2^40"""
    t0 = time.perf_counter()
    a = hip.seed_segments([12345, 0xFFFFFFFF], 1 << 40, 40)
    dt = time.perf_counter() - t0
    assert dt < 1.0, dt
    b = hip.seed_segments([12345, 0xFFFFFFFF], (1 << 40) + 64, 38)
    assert a[0][2:] == b[0] and a[1][2:] == b[1]
    assert a[0] != a[1] and any(a[0])


def test_refusals(hip):
    seeds, out = (C.c_uint32 * 2)(1, 2), (C.c_uint32 * 16)()
    f = hip.lib.vfgs_hip_seed_segments
    assert f(None, 2, 0, 8, out) != 0
    assert f(seeds, 2, 0, 8, None) != 0
    assert f(seeds, 0, 0, 8, out) != 0
    assert f(seeds, 2, 0, 0, out) != 0
    assert f(seeds, 2, 0, 8, out) == 0


def test_afgs1_seed_is_the_register_the_firmware_loads(hip):
    """vfgs_fw.c:672: grain_seed | grain_seed << 16 goes to vfgs_set_seed, which loads it << 1 (vfgs_hw.c:343)"""
    _, cfgs = T.load_fwcfg("fgs_afgs1_test1_10_420")
    cfg = [fw.struct_from_bytes(k, raw) for k, raw in cfgs if k == 1][0]
    assert cfg.grain_seed != 0
    hip.lib.vfgs_hip_reset_state()
    try:
        fw.init_afgs1(cfg)
        s = fw.afgs1_seed(cfg)
        assert s == (cfg.grain_seed | cfg.grain_seed << 16)
        assert hip.seed_state() == ((s << 1) & 0xFFFFFFFF,) * 4
        cfg.grain_seed = 0xFFFF
        assert fw.afgs1_seed(cfg) == 0xFFFFFFFF
    finally:
        hip.lib.vfgs_hip_reset_state()


MODEL_DRIVER = r"""
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
vp, u = C.c_void_p, C.c_uint
class P(C.Structure):
    _fields_ = [("Y", vp), ("U", vp), ("V", vp)]
fp, sp = C.POINTER(P), C.POINTER(C.c_uint32)
lib.vfgs_hip_add_grain_frame_list_seeded_dev.argtypes = [fp, sp, u, u, u, u, u, vp]
lib.vfgs_hip_add_grain_frame_list_seeded_part_dev.argtypes = [fp, sp, u, u, u, u, u, u, u, vp]
lib.vfgs_hip_add_grain_frame_list_seeded_copy_dev.argtypes = [fp, fp, sp, u, u, u, u, u, vp]
lib.vfgs_hip_add_grain_frame_list_dev.argtypes = [fp, u, u, u, u, u, vp]
lib.vfgs_hip_add_grain_frame_dev.argtypes = [vp, vp, vp, u, u, u, u, vp]
lib.vfgs_hip_get_seeded_stream_stats.argtypes = [C.POINTER(C.c_uint64)]
lib.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
W, H, S = 200, 150, 256
lib.vfgs_set_depth(10); lib.vfgs_set_chroma_subsampling(2, 2); lib.vfgs_set_scale_shift(5); lib.vfgs_set_seed(4711)
def frames(n):
    arr = (P * n)()
    for k in range(n):
        for name, size in (("Y", S * 160 * 2), ("U", S // 2 * 80 * 2), ("V", S // 2 * 80 * 2)):
            p = vp(); lib.hipMalloc(C.byref(p), size); setattr(arr[k], name, p.value)
    return arr
def state():
    out = (C.c_uint32 * 4)(); lib.vfgs_hip_get_seed_state(out); return list(out)
def seeds(n, base):
    return (C.c_uint32 * n)(*[(base * 2654435761 + 977 * k * k) & 0xFFFFFFFF for k in range(n)])
log = []
pool = frames(70)
s5, s70, s3 = seeds(5, 1), seeds(70, 2), seeds(3, 3)
assert lib.vfgs_hip_add_grain_frame_list_seeded_dev(pool, s5, 5, W, H, S, S // 2, None) == 0
log.append(("list", list(s5), state()))
before = state()
assert lib.vfgs_hip_add_grain_frame_list_seeded_dev(pool, None, 5, W, H, S, S // 2, None) == 39
dup = (P * 2)(pool[0], pool[0])
assert lib.vfgs_hip_add_grain_frame_list_seeded_dev(dup, s5, 2, W, H, S, S // 2, None) == 18
assert lib.vfgs_hip_add_grain_frame_list_seeded_part_dev(pool, s5, 5, W, H, 8, 32, S, S // 2, None) == 11
assert lib.vfgs_hip_add_grain_frame_list_seeded_dev(pool, s5, 0, W, H, S, S // 2, None) == 0
assert lib.vfgs_hip_add_grain_frame_list_seeded_dev(pool, None, 0, W, H, S, S // 2, None) == 0
assert state() == before, "a refused call moved the registers"
part = (P * 3)()
for k in range(3):
    part[k].Y, part[k].U, part[k].V = pool[k].Y + 48 * S * 2, pool[k].U + 24 * (S // 2) * 2, pool[k].V + 24 * (S // 2) * 2
assert lib.vfgs_hip_add_grain_frame_list_seeded_part_dev(part, s3, 3, W, H, 48, 70, S, S // 2, None) == 0
log.append(("part", list(s3), state()))
assert lib.vfgs_hip_add_grain_frame_list_seeded_dev(pool, s70, 70, W, H, S, S // 2, None) == 0
log.append(("list", list(s70), state()))
st = (C.c_uint64 * 4)(); lib.vfgs_hip_get_seeded_stream_stats(st)
assert st[0] == 1 + 1 + 3 and st[3] == 1 and st[1] == 6 * 9, list(st)     # (32 + 32 + 6 frames; 6 segments of 9 words)
assert lib.vfgs_hip_add_grain_frame_list_dev(pool, 3, W, H, S, S // 2, None) == 0
log.append(("unseeded", 3, state()))
lib.vfgs_hip_get_seeded_stream_stats(st)
assert st[3] == 0
assert lib.vfgs_hip_add_grain_frame_list_seeded_copy_dev(pool, (P * 2)(pool[10], pool[11]), s5, 2, W, H, S, S // 2, None) == 0
log.append(("list", list(s5)[:2], state()))
assert lib.vfgs_hip_add_grain_frame_dev(pool[0].Y, pool[0].U, pool[0].V, W, H, S, S // 2, None) == 0
log.append(("unseeded", 1, state()))
lib.hipDeviceSynchronize()
lib.vfgs_hip_shutdown()
print("LOG", json.dumps(log))
"""


def test_seed_registers_of_the_entry_points_over_the_runtime_model(tmp_path):
    """seeded lists of 200 x 150 (whole, a part, 70 frames = three launches, out of place), refused calls in between, unseeded calls that
    continue the last picture's stream: vfgs_hip_get_seed_state against the oracle's after the contract's loop, every time"""
    import json
    import sanitize_build as S
    if not S.HAVE_TOOLS:
        pytest.skip("needs g++ and the HIP headers")
    so = S.build(tmp_path, "libvfgs_host_model.so", S.OPTIMISED, [], shared=True)
    r = subprocess.run([sys.executable, "-c", MODEL_DRIVER, str(so)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    log = json.loads(r.stdout.split("LOG", 1)[1])
    ora = T.OracleHW()
    ora.set_depth(10); ora.set_chroma_subsampling(2, 2); ora.set_scale_shift(5); ora.set_seed(4711)
    scratch = T.Frame(200, 150, 10, 2, 2)
    assert len(log) == 6
    for i, (kind, arg, got) in enumerate(log):
        if kind == "unseeded":
            for _ in range(arg):
                ora.add_grain_frame(scratch)
        else:     # (a part leaves the registers of whole frames)
            for s in arg:
                ora.set_seed(s)
                ora.add_grain_frame(scratch)
        assert tuple(got) == ora.seed_state(), (i, kind)
