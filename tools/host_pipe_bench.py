#!/usr/bin/env python3
"""Developer tool: what the host-memory pipe (vfgs_hip_host_pipe_*) buys a decoder whose pictures arrive in host memory one at a time, each
with its own AFGS1 parameter set and seed, on one MI355X, in one command.  Writes one JSON document (default profiles/host_pipe.json).

Workloads: 32 pictures of 1920x1080 and of 3840x2160, 10-bit 4:2:0, in pinned host memory (every plane an allocation of its own, pitches =
the rows, content uniform in 0.3 .. 0.7 of the range), 32 distinct AFGS1 parameter sets (the sixteen recorded 10-bit 4:2:0 ones of
tests/golden/fwcfg, each once as recorded and once with another seed and a changed luma scaling function), each picture with the seed of
its set.  Legs alternated, `--rounds` rounds; a window is `passes` passes over the 32 pictures behind one warm-up pass, timed by the host
clock around work that ends with every picture in host memory; building and releasing the 32 models is inside the window.

  a   the pipe, in place: vfgs_hip_models_from_afgs1 (32 models), 32 submits, the wait for the last ticket, 32 releases
  a8  the pipe with the narrowed 8-bit destination (dst8), the same otherwise
  b   what a caller can do without the pipe: the 32 models, then per picture three synchronous 2-D uploads, a one-picture
      vfgs_hip_add_grain_frame_list_models_dev, a stream synchronise, three synchronous 2-D downloads; 32 releases
  c   the link-rate yardstick: vfgs_hip_add_grain_frames_host over the 32 pictures with ONE programmed model (no model is built)
  c_this  leg c on THIS build: the old call shares its three streams with the pipes now, so parent and this build are alternated over it

b and c run on the PARENT commit's library where --parent-lib names it (a state of its own in the same process, the same buffers): the
yardsticks are then not the code under test.  Picture 0 of legs a and b is compared byte for byte first (`same_picture`)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402

AFGS1_10_420 = ["fgs_afgs1_test%s_10_420" % k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, "1_tbl")]
WORKLOADS = [(1920, 1080, 96), (3840, 2160, 32)]      # width, height, passes of a window (half a second and more)
NF = 32
H2D, D2H = 1, 2


class Baseline:
    """the library legs b and c run on: the setters a recorded program needs, the models from parameter sets, the one-picture list call with
    a model and the pipelined host call"""

    def __init__(self, lib, hw, fw):
        self.lib = lib
        vp, u, i = C.c_void_p, C.c_uint, C.c_int
        fp, u32p = C.POINTER(hw.FramePtrs), C.POINTER(C.c_uint32)
        for n, a in (("vfgs_set_luma_pattern", [i, vp]), ("vfgs_set_chroma_pattern", [i, vp]), ("vfgs_set_scale_lut", [i, vp]), ("vfgs_set_pattern_lut", [i, vp]),
                     ("vfgs_set_seed", [u]), ("vfgs_set_scale_shift", [i]), ("vfgs_set_depth", [i]), ("vfgs_set_legal_range", [i]),
                     ("vfgs_set_chroma_subsampling", [i, i]), ("vfgs_hip_init", [i]),
                     ("vfgs_hip_models_from_afgs1", [vp, u, C.POINTER(vp), vp]), ("vfgs_hip_model_release", [vp]),
                     ("vfgs_hip_add_grain_frame_list_models_dev", [fp, fp, C.POINTER(vp), u32p, u, u, u, u, u, vp]),
                     ("vfgs_hip_add_grain_frames_host", [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), u, u, u, u, u])):
            getattr(lib, n).argtypes = a
        lib.vfgs_hip_model_release.restype = None
        lib.vfgs_hip_last_error_string.restype = C.c_char_p
        lib.vfgs_hip_reset_state.restype = None
        assert lib.vfgs_hip_init(0) == 0
        b = hw._b
        self.set_luma_pattern = lambda k, P: lib.vfgs_set_luma_pattern(k, b(P))
        self.set_chroma_pattern = lambda k, P: lib.vfgs_set_chroma_pattern(k, b(P))
        self.set_scale_lut = lambda c, l: lib.vfgs_set_scale_lut(c, b(l))
        self.set_pattern_lut = lambda c, l: lib.vfgs_set_pattern_lut(c, b(l))
        self.set_seed = lambda s: lib.vfgs_set_seed(s & 0xFFFFFFFF)
        self.set_scale_shift, self.set_depth, self.set_legal_range = lib.vfgs_set_scale_shift, lib.vfgs_set_depth, lib.vfgs_set_legal_range
        self.set_chroma_subsampling = lib.vfgs_set_chroma_subsampling

    def ck(self, rc):
        assert rc == 0, self.lib.vfgs_hip_last_error_string()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libvfgs_hip.so of the parent commit: legs b and c run on it (without it: on this build)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "host_pipe.json"))
    ap.add_argument("--trace", action="store_true", help="for a run under a tracer: 3840x2160 only, legs a and c, one round of four passes each, no JSON document")
    args = ap.parse_args()
    import torch
    import vfgs_testlib as T
    from versatilefilmgrain_amd import fw, hw
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.trace or args.rounds >= 5, "at least five rounds of each leg"
    hip = hw.VfgsHip(device=0)
    rt = C.CDLL(hw.hip_runtimes_mapped()[0])
    rt.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    rt.hipStreamSynchronize.argtypes = [C.c_void_p]
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    base = Baseline(C.CDLL(str(args.parent_lib)), hw, fw) if args.parent_lib else Baseline(hip.lib, hw, fw)
    rec = T.load_trace("fgs_afgs1_test1_10_420")      # depth, format, range -- and leg c's ONE programmed model
    for b in (hip, base):
        b.lib.vfgs_hip_reset_state()
        T.replay(b, rec)

    afgs1 = []
    for i in range(NF):
        kind, raw = T.load_fwcfg(AFGS1_10_420[i % 16])[1][-1]
        assert kind == 1
        a = fw.struct_from_bytes(1, raw)
        if i >= 16:     # the second model of a parameter set: another seed, another luma scaling function
            a.grain_seed = (a.grain_seed + 257 * (i - 15)) & 0xffff
            for k in range(a.num_y_points):
                a.point_y_scaling[k] = max(1, a.point_y_scaling[k] - 1 - (i & 3))
        afgs1.append(a)
    assert len({bytes(a) for a in afgs1}) == NF
    seeds = [fw.afgs1_seed(a) for a in afgs1]
    cfg_arr = (fw.FgsAfgs1 * NF)(*afgs1)
    seed_arr = [(C.c_uint32 * 1)(s) for s in seeds]

    out = {"what": "pictures in host memory, a model and a seed per picture (tools/host_pipe_bench.py): legs alternated in one command on one MI355X, "
                   "%d rounds, a window = a warm-up pass and then the listed passes over 32 pictures in pinned memory, host clock around work that ends "
                   "with every picture in host memory; building and releasing the 32 models is inside the window (legs a, a8, b)" % args.rounds,
           "device": hip.device_info(), "baseline_library": "the parent commit's" if args.parent_lib else "this build's",
           "legs": {"a": "the pipe, in place", "a8": "the pipe, dst8", "b": "per picture: 3 synchronous 2-D uploads, a one-picture list call with its model, 3 downloads",
                    "c": "vfgs_hip_add_grain_frames_host, ONE programmed model", "c_this": "leg c on this build (c: the baseline library)"}, "workloads": {}}
    rng = np.random.default_rng(1)
    keep = []

    def pinned(shape, dtype, fill=None):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = hip.host_alloc(n)
        keep.append(p)
        v = np.frombuffer((C.c_char * n).from_address(p), dtype=dtype).reshape(shape)
        if fill is not None:
            v[...] = fill
        return v

    for w, h, passes in ([(3840, 2160, 4)] if args.trace else WORKLOADS):
        shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
        content = [rng.integers(int(0.3 * 1024), int(0.7 * 1024), s, dtype=np.int32).astype(np.uint16) for s in shapes]
        src = [[pinned(s, np.uint16, c) for s, c in zip(shapes, content)] for _ in range(NF)]
        dst8 = [[pinned(s, np.uint8, 0x5a) for s in shapes] for _ in range(NF)]
        sp = [tuple(p.ctypes.data for p in f) for f in src]
        dp = [tuple(p.ctypes.data for p in f) for f in dst8]
        dev = [torch.empty(s, dtype=torch.int16, device="cuda") for s in shapes]
        dev_list = hw.VfgsHip.frame_list([tuple(t.data_ptr() for t in dev)])
        arrs = [(C.c_void_p * NF)(*[f[i].ctypes.data for f in src]) for i in range(3)]
        picture_bytes = sum(a * b for a, b in shapes) * 2

        kernels = {}

        def restore():
            for f in src:
                for p, c in zip(f, content):
                    p[...] = c

        def leg_pipe(pipe, dst):
            ms = hip.models_from_afgs1(afgs1, st)
            t = 0
            for k in range(NF):
                t = pipe.submit(sp[k], dst[k] if dst else None, ms[k], seeds[k])
            kernels["a8" if dst else "a"] = hip.last_launch_info()["kernel"]
            for m in ms:
                hip.model_release(m)      # (as soon as the submits have returned)
            pipe.wait(t)

        def leg_b():
            ms = (C.c_void_p * NF)()
            base.ck(base.lib.vfgs_hip_models_from_afgs1(cfg_arr, NF, ms, st))
            for k in range(NF):
                for i, (rows, cols) in enumerate(shapes):
                    assert rt.hipMemcpy2D(dev[i].data_ptr(), cols * 2, sp[k][i], cols * 2, cols * 2, rows, H2D) == 0
                one = (C.c_void_p * 1)(ms[k])
                base.ck(base.lib.vfgs_hip_add_grain_frame_list_models_dev(dev_list, dev_list, one, seed_arr[k], 1, w, h, w, w // 2, st))
                assert rt.hipStreamSynchronize(st) == 0
                for i, (rows, cols) in enumerate(shapes):
                    assert rt.hipMemcpy2D(sp[k][i], cols * 2, dev[i].data_ptr(), cols * 2, cols * 2, rows, D2H) == 0
            for m in ms:
                base.lib.vfgs_hip_model_release(m)

        def leg_c():
            base.ck(base.lib.vfgs_hip_add_grain_frames_host(arrs[0], arrs[1], arrs[2], NF, w, h, w, w // 2))

        def leg_c_this():
            hip._ck(hip.lib.vfgs_hip_add_grain_frames_host(arrs[0], arrs[1], arrs[2], NF, w, h, w, w // 2))

        with hip.host_pipe(w, h, w, w // 2) as pa, hip.host_pipe(w, h, w, w // 2, w, w // 2, True) as pa8:
            legs = {"a": lambda: leg_pipe(pa, None), "a8": lambda: leg_pipe(pa8, dp), "b": leg_b, "c": leg_c, "c_this": leg_c_this}
            if args.trace:
                for name in ("a", "c"):
                    legs[name]()
                    t0 = time.perf_counter()
                    for _p in range(passes):
                        legs[name]()
                    print("traced leg", name, round((time.perf_counter() - t0) * 1e3 / (passes * NF), 4), "ms per picture", flush=True)
                return 0
            # the same picture through a and b
            legs["a"]()
            got = [p.copy() for p in src[0]]
            restore()
            legs["b"]()
            same = all(np.array_equal(x, y) for x, y in zip(got, src[0])) and not np.array_equal(got[0], content[0])
            restore()
            ms_pp = {k: [] for k in legs}
            window_s = {k: [] for k in legs}
            for _ in range(args.rounds):
                for name, fn in legs.items():      # (alternated: every round runs every leg)
                    fn()      # warm-up: every shape of the window
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _p in range(passes):
                        fn()
                    dt = time.perf_counter() - t0      # (every leg ends with its last picture in host memory)
                    ms_pp[name].append(round(dt * 1e3 / (passes * NF), 4))
                    window_s[name].append(round(dt, 3))
                    restore()
        med = {k: statistics.median(v) for k, v in ms_pp.items()}
        e = {"pictures": NF, "passes_per_window": passes, "picture_bytes": picture_bytes, "same_picture": bool(same), "kernels_of_the_pipe": kernels,
             "window_seconds": {k: [min(v), max(v)] for k, v in window_s.items()},
             "ms_per_picture_rounds": ms_pp, "ms_per_picture": {k: round(v, 4) for k, v in med.items()},
             "GBps_each_way_a": round(picture_bytes / med["a"] / 1e6, 2),
             "a_rounds_all_below_b_rounds": bool(max(ms_pp["a"]) < min(ms_pp["b"])), "b_over_a": round(med["b"] / med["a"], 3),
             "a_over_c": round(med["a"] / med["c"], 3), "a_median_above_c_slowest_round": bool(med["a"] > max(ms_pp["c"])),
             "a8_over_a": round(med["a8"] / med["a"], 3),
             "old_call_this_over_parent": round(med["c_this"] / med["c"], 4), "old_call_parent_min_max": [min(ms_pp["c"]), max(ms_pp["c"])],
             "old_call_this_median_within_parent_spread": bool(min(ms_pp["c"]) <= med["c_this"] <= max(ms_pp["c"]))}
        out["workloads"]["%dx%d 10-bit 4:2:0 x%d" % (w, h, NF)] = e
        print(w, h, json.dumps(e), flush=True)
        del src, dst8, dev
        for p in keep:
            hip.host_free(p)
        keep.clear()
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
