#!/usr/bin/env python3
"""Developer tool: what it costs to MAKE film grain models from FGC SEI messages, on one MI355X, in one command.

Legs, alternated in one process, `--rounds` rounds after a warm-up; a host clock (perf_counter) around work that ends in a stream
synchronise, `--reps` repetitions per round and leg; 32 DISTINCT messages per configuration (a recorded one with the cut-offs or the
auto-regressive coefficients varied per message, so that no pattern request repeats the previous one and skips its generation):
  a  today's loop: vfgs_init_sei + vfgs_hip_model_capture per message (32 messages, then the synchronise)
  b  vfgs_hip_models_from_sei, n = 32
  c  vfgs_hip_models_from_sei, n = 1
  d  end to end at 1920x1080 P010 x 32, one model per picture (the 10-bit configurations):
       d_build      b + vfgs_hip_add_grain_sp_frame_list_models_dev + release of the 32
       d_capture    a + the same list call + release
       d_reprogram  vfgs_init_sei + vfgs_hip_add_grain_sp_frame_list_dev on ONE surface per launch, 32 times
Reports microseconds per model (per picture for d) as median (min .. max) over the rounds, and the bookkeeping counters.
Writes one JSON document (default profiles/sei_model_build.json)."""
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


def recorded(name):
    kind, raw = T.load_fwcfg(name)[1][-1]
    assert kind == 0
    return fw.struct_from_bytes(0, raw)


def default_ff(i):
    """the CLI default (8 luma patterns), every cut-off moved by the message's index"""
    s = recorded("default_10_420")
    assert s.model_id == 0
    for c in range(3):
        for k in range(s.num_intensity_intervals[c]):
            v = s.comp_model_value[c][k]
            v[1] = 2 + (v[1] + i + k) % 13
            v[2] = 2 + (v[2] + 5 * i + i // 13 + k) % 13
    return s


def chroma_ff(i):
    """the 8-bit default with three patterns in Cb and three others in Cr"""
    s = recorded("default_8_420")
    assert s.model_id == 0
    for c in (1, 2):
        s.comp_model_present_flag[c] = 1
        s.num_intensity_intervals[c] = 3
        s.num_model_values[c] = 3
        for k, (lo, hi) in enumerate(((0, 80), (81, 170), (171, 255))):
            s.intensity_interval_lower_bound[c][k] = lo
            s.intensity_interval_upper_bound[c][k] = hi
            v = s.comp_model_value[c][k]
            v[0] = 40 + 20 * k + 7 * c
            v[1] = 2 + (i + 3 * k + 5 * c) % 13
            v[2] = 2 + (5 * i + i // 13 + k + c) % 13
    for k in range(s.num_intensity_intervals[0]):
        s.comp_model_value[0][k][1] = 2 + (s.comp_model_value[0][k][1] + i) % 13
        s.comp_model_value[0][k][2] = 2 + (s.comp_model_value[0][k][2] + 5 * i + i // 13) % 13
    return s


def ar(i):
    """the recorded auto-regressive message, its coefficients moved by the message's index"""
    s = recorded("fgs_sei_ar_test1_10_420")
    assert s.model_id == 1
    for c in range(3):
        for k in range(s.num_intensity_intervals[c]):
            v = s.comp_model_value[c][k]
            v[1] = max(-100, min(100, v[1] + (i * 7 + k) % 11 - 5))
            v[3] = max(-60, min(60, v[3] + (i * 5 + c) % 9 - 4))
            v[5] = max(-40, min(40, v[5] + (i * 3) % 7 - 3))
    return s


CONFIGS = [  # name, message i of the set, depth, end-to-end legs
    ("10-bit 4:2:0 frequency filtered, the CLI default (8 luma patterns)", default_ff, 10, True),
    ("8-bit 4:2:0 frequency filtered, 8 luma and 6 chroma patterns", chroma_ff, 8, False),
    ("10-bit 4:2:0 auto-regressive", ar, 10, True),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sei_model_build.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    fw._lib()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    out = {"what": "making film grain models from %d distinct FGC SEI messages: legs alternated in one process on one MI355X, %d rounds of %d "
                   "repetitions after %d warm-up repetitions, host clock around work that ends in a stream synchronise, microseconds per model "
                   "(legs d: per picture) (tools/sei_model_build_bench.py)" % (N, args.rounds, args.reps, args.warmup),
           "legs": {"a": "vfgs_init_sei + vfgs_hip_model_capture per message", "b": "vfgs_hip_models_from_sei, n = 32",
                    "c": "vfgs_hip_models_from_sei, n = 1",
                    "d_build": "b + vfgs_hip_add_grain_sp_frame_list_models_dev on 32 P010 surfaces of 1920x1080 + release",
                    "d_capture": "a + the same list call + release",
                    "d_reprogram": "vfgs_init_sei + vfgs_hip_add_grain_sp_frame_list_dev on one surface per launch, 32 times"},
           "device": hip.device_info(), "configurations": {}}
    for name, message, depth, end_to_end in CONFIGS:
        lib.vfgs_hip_reset_state()
        hip.set_depth(depth)
        hip.set_chroma_subsampling(2, 2)
        msgs = (fw.FgsSei * N)(*[message(i) for i in range(N)])
        assert len({bytes(msgs[i]) for i in range(N)}) == N
        ptrs = [C.pointer(msgs[i]) for i in range(N)]
        seeds = (C.c_uint32 * N)(*[1000 + 77 * i for i in range(N)])
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
                lib.vfgs_init_sei(ptrs[i])
                ck(lib.vfgs_hip_model_capture(C.byref(m), sp))
                handles[i] = m.value

        def make_b():
            ck(lib.vfgs_hip_models_from_sei(msgs, N, handles, sp))

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
            ck(lib.vfgs_hip_models_from_sei(ptrs[state["k"] % N], 1, one, sp))
            stream.synchronize()
            t = time.perf_counter()
            lib.vfgs_hip_model_release(one[0])
            return t, 1

        legs = {"a": leg_a, "b": leg_b, "c": leg_c}
        if end_to_end:
            w, h = 1920, 1080
            shift = 16 - depth
            keep = [[torch.randint(0, 1 << depth, (rows, w), dtype=torch.int16, device="cuda") << shift for rows in (h, h // 2)] for _ in range(N)]
            surfaces = hip.sp_frame_list([tuple(p.data_ptr() for p in planes) for planes in keep])
            singles = [hip.sp_frame_list([tuple(p.data_ptr() for p in planes)]) for planes in keep]
            one_seed = [(C.c_uint32 * 1)(seeds[i]) for i in range(N)]
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
                    lib.vfgs_init_sei(ptrs[i])
                    ck(lib.vfgs_hip_add_grain_sp_frame_list_dev(singles[i], singles[i], one_seed[i], 1, w, h, w, w, shift, sp))
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
