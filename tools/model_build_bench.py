#!/usr/bin/env python3
"""Developer tool: what it costs to MAKE film grain models from AFGS1 parameter sets, on one MI355X, in one command.

Legs, alternated in one process, `--rounds` rounds after a warm-up; a host clock (perf_counter) around work that ends in a stream
synchronise, `--reps` repetitions per round and leg; 32 DISTINCT parameter sets (a recorded one with the AR coefficients and the seed
varied per picture, so that no pattern request repeats the previous one and skips its generation):
  a  today's loop: vfgs_init_afgs1 + vfgs_hip_model_capture per set (32 sets, then the synchronise)
  b  vfgs_hip_models_from_afgs1, n = 32
  c  vfgs_hip_models_from_afgs1, n = 1
  d  end to end at 1920x1080 P010 x 32, one model per picture (the 10-bit 4:2:0 configuration only):
       d_build    b + vfgs_hip_add_grain_sp_frame_list_models_dev + release of the 32
       d_capture  a + the same list call + release
       d_reprogram  vfgs_init_afgs1 + vfgs_hip_add_grain_sp_frame_list_dev on ONE surface per launch, 32 times
Reports microseconds per model (per picture for d) as median (min .. max) over the rounds, and the bookkeeping counters.
Writes one JSON document (default profiles/model_build.json)."""
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
import torch  # noqa: E402
import vfgs_testlib as T  # noqa: E402
from versatilefilmgrain_amd import fw, hw  # noqa: E402

N = 32
CONFIGS = [  # name, recorded parameter set, depth, csubx, csuby, ar_coeff_lag, end-to-end leg
    ("10-bit 4:2:0 lag 3", "fgs_afgs1_test3_10_420", 10, 2, 2, 3, True),
    ("8-bit 4:4:4 lag 2", "fgs_afgs1_test1_8_444", 8, 1, 1, 2, False),
]


def distinct_sets(name, lag):
    kind, raw = T.load_fwcfg(name)[1][-1]
    assert kind == 1
    arr = (fw.FgsAfgs1 * N)()
    for i in range(N):
        a = fw.struct_from_bytes(1, raw)
        assert a.ar_coeff_lag == lag, (name, a.ar_coeff_lag)
        a.grain_seed = (a.grain_seed + 977 * i) & 0xFFFF
        for k in range(2 * lag * (lag + 1)):
            a.ar_coeffs_y[k] = max(-128, min(127, a.ar_coeffs_y[k] + ((i * 7 + k * 3) % 9) - 4))
            a.ar_coeffs_cb[k] = max(-128, min(127, a.ar_coeffs_cb[k] + ((i * 5 + k) % 7) - 3))
        arr[i] = a
    assert len({bytes(arr[i]) for i in range(N)}) == N
    return arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "model_build.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    fw._lib()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    out = {"what": "making film grain models from %d distinct AFGS1 parameter sets: legs alternated in one process on one MI355X, %d rounds of %d "
                   "repetitions after %d warm-up repetitions, host clock around work that ends in a stream synchronise, microseconds per model "
                   "(legs d: per picture) (tools/model_build_bench.py)" % (N, args.rounds, args.reps, args.warmup),
           "legs": {"a": "vfgs_init_afgs1 + vfgs_hip_model_capture per set", "b": "vfgs_hip_models_from_afgs1, n = 32",
                    "c": "vfgs_hip_models_from_afgs1, n = 1",
                    "d_build": "b + vfgs_hip_add_grain_sp_frame_list_models_dev on 32 P010 surfaces of 1920x1080 + release",
                    "d_capture": "a + the same list call + release",
                    "d_reprogram": "vfgs_init_afgs1 + vfgs_hip_add_grain_sp_frame_list_dev on one surface per launch, 32 times"},
           "device": hip.device_info(), "configurations": {}}
    for name, cfg, depth, sx, sy, lag, end_to_end in CONFIGS:
        lib.vfgs_hip_reset_state()
        hip.set_depth(depth)
        hip.set_chroma_subsampling(sx, sy)
        fw.afgs1_chroma_mix(False)
        sets = distinct_sets(cfg, lag)
        ptrs = [C.pointer(sets[i]) for i in range(N)]
        seeds = (C.c_uint32 * N)(*[fw.afgs1_seed(sets[i]) for i in range(N)])
        handles = (C.c_void_p * N)()
        one = (C.c_void_p * 1)()

        def ck(rc):
            assert rc == 0, lib.vfgs_hip_last_error_string()

        def release():
            for i in range(N):
                lib.vfgs_hip_model_release(handles[i])

        def make_a():
            m = C.c_void_p()
            for i in range(N):
                lib.vfgs_init_afgs1(ptrs[i])
                ck(lib.vfgs_hip_model_capture(C.byref(m), sp))
                handles[i] = m.value

        def make_b():
            ck(lib.vfgs_hip_models_from_afgs1(sets, N, handles, sp))

        def leg_a():
            make_a()
            stream.synchronize()
            t = time.perf_counter()
            release()
            return t, N

        def leg_b():
            make_b()
            stream.synchronize()
            t = time.perf_counter()
            release()
            return t, N

        state = {"k": 0}

        def leg_c():
            state["k"] += 1
            ck(lib.vfgs_hip_models_from_afgs1(ptrs[state["k"] % N], 1, one, sp))
            stream.synchronize()
            t = time.perf_counter()
            lib.vfgs_hip_model_release(one[0])
            return t, 1

        legs = {"a": leg_a, "b": leg_b, "c": leg_c}
        if end_to_end:
            w, h = 1920, 1080
            shift = 16 - depth
            keep = [[torch.randint(0, 1 << depth, (rows, w), dtype=torch.int16, device="cuda") << shift for rows in (h, h // sy)] for _ in range(N)]
            surfaces = hip.sp_frame_list([tuple(p.data_ptr() for p in planes) for planes in keep])
            singles = [hip.sp_frame_list([tuple(p.data_ptr() for p in planes)]) for planes in keep]
            torch.cuda.synchronize()

            def listed():
                ck(lib.vfgs_hip_add_grain_sp_frame_list_models_dev(surfaces, surfaces, handles, seeds, N, w, h, w, w, shift, sp))
                release()
                stream.synchronize()
                return time.perf_counter(), N

            def leg_d_build():
                make_b()
                return listed()

            def leg_d_capture():
                make_a()
                return listed()

            def leg_d_reprogram():
                for i in range(N):
                    lib.vfgs_init_afgs1(ptrs[i])         # (programs the picture's seed too)
                    ck(lib.vfgs_hip_add_grain_sp_frame_list_dev(singles[i], singles[i], None, 1, w, h, w, w, shift, sp))
                stream.synchronize()
                return time.perf_counter(), N

            legs.update({"d_build": leg_d_build, "d_capture": leg_d_capture, "d_reprogram": leg_d_reprogram})

        def measure(leg, reps):
            total, count = 0.0, 0
            for _ in range(reps):
                t0 = time.perf_counter()
                t1, n = leg()
                total += t1 - t0
                count += n
            return total * 1e6 / count

        us = {k: [] for k in legs}
        for k, leg in legs.items():
            measure(leg, args.warmup)
        stats0 = hip.model_build_stats()
        for _ in range(args.rounds):
            for k, leg in legs.items():
                us[k].append(round(measure(leg, args.reps), 3))
        stats1 = hip.model_build_stats()
        r = {"us_per_model": us,
             "median_min_max": {k: [statistics.median(v), min(v), max(v)] for k, v in us.items()},
             "b_range_entirely_below_a_range": max(us["b"]) < min(us["a"]),
             "build_stats_before_the_rounds": stats0, "build_stats_after_the_rounds": stats1}
        if end_to_end:
            r["d_build_range_entirely_below_d_capture_range"] = max(us["d_build"]) < min(us["d_capture"])
            r["d_build_range_entirely_below_d_reprogram_range"] = max(us["d_build"]) < min(us["d_reprogram"])
            del keep, surfaces, singles
            torch.cuda.empty_cache()
        out["configurations"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    lib.vfgs_hip_reset_state()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
