#!/usr/bin/env python3
"""Developer tool: what a seed per picture costs a frame-list launch, on one MI355X, in one command.

Legs, alternated, `--rounds` rounds, HIP-event windows of `--window` launches after a warm-up, in place, every frame an allocation of
its own, fresh random seeds per call:
  a  vfgs_hip_add_grain_frame_list_dev            the unseeded list (the yardstick: its code path is untouched by the seeds)
  b  vfgs_hip_add_grain_frame_list_seeded_dev     the seeded list
  c  vfgs_set_seed + vfgs_hip_add_grain_frame_dev per frame: the only way to a seed per picture without it
  d  leg b inside an overlap region (vfgs_hip_overlap_begin / _end around the window)
Also: the host time of a seeded call (the image is built and queued inside it), the bytes of its image, the host waits for a slot.
Prints one JSON document (profiles/per_picture_seeds.json is one, with what was measured beside it added by hand)."""
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
import torch  # noqa: E402
import vfgs_testlib as T  # noqa: E402
from versatilefilmgrain_amd import hw  # noqa: E402

SHAPES = [  # name, width, height, trace, frames per launch
    ("1920x1080 10-bit 4:2:0 fgs_sei x32", 1920, 1080, "fgs_sei_10_420", 32),
    ("3840x2160 10-bit 4:2:0 fgs_afgs1_test1 x16", 3840, 2160, "fgs_afgs1_test1_10_420", 16),
    ("7680x4320 10-bit 4:2:0 fgs_sei x8", 7680, 4320, "fgs_sei_10_420", 8),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pool-mb", type=int, default=1600, help="bytes of frames cycled through per shape (beyond the last-level cache)")
    ap.add_argument("--shapes", default="0,1,2")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    out = {"what": "frame lists with a seed per picture: legs alternated in one command on one MI355X, %d rounds, HIP-event windows of %d launches "
                   "after %d warm-up launches, in place, every frame an allocation of its own, uniform random content, fresh random seeds per "
                   "call (tools/seeded_list_bench.py)" % (args.rounds, args.window, args.warmup),
           "legs": {"a": "vfgs_hip_add_grain_frame_list_dev", "b": "vfgs_hip_add_grain_frame_list_seeded_dev",
                    "c": "vfgs_set_seed + vfgs_hip_add_grain_frame_dev per frame", "d": "leg b inside an overlap region"},
           "device": hip.device_info(), "shapes": {}}
    rng = np.random.default_rng(1)
    for si in [int(x) for x in args.shapes.split(",")]:
        name, w, h, trace, nf = SHAPES[si]
        lib.vfgs_hip_reset_state()
        rec = T.load_trace(trace)
        T.replay(hip, rec)
        depth, sx, sy = T.trace_geometry(rec)
        assert depth == 10
        frame_bytes = (w * h + 2 * (w // sx) * (h // sy)) * 2
        nsets = max(2, -(-args.pool_mb * (1 << 20) // (frame_bytes * nf)))
        keep, sets, singles = [], [], []
        for _ in range(nsets):
            ptrs = []
            for _ in range(nf):
                planes = [torch.randint(0, 1 << 10, (rows, cols), dtype=torch.int16, device="cuda") for rows, cols in ((h, w), (h // sy, w // sx), (h // sy, w // sx))]
                keep.append(planes)
                ptrs.append(tuple(p.data_ptr() for p in planes))
            order = rng.permutation(nf)          # list order is not address order
            ptrs = [ptrs[i] for i in order]
            sets.append(hip.frame_list(ptrs))
            singles.append(ptrs)
        torch.cuda.synchronize()
        ncalls = args.warmup + args.window
        seed_arrays = lambda: [(C.c_uint32 * nf)(*[int(s) for s in rng.integers(0, 1 << 32, nf)]) for _ in range(ncalls)]
        cw = w // sx

        def leg_a(k, seeds):
            return lib.vfgs_hip_add_grain_frame_list_dev(sets[k % nsets], nf, w, h, w, cw, sp)

        def leg_b(k, seeds):
            return lib.vfgs_hip_add_grain_frame_list_seeded_dev(sets[k % nsets], seeds[k], nf, w, h, w, cw, sp)

        def leg_c(k, seeds):
            rc = 0
            for (y, u, v), s in zip(singles[k % nsets], seeds[k]):
                lib.vfgs_set_seed(s)
                rc |= lib.vfgs_hip_add_grain_frame_dev(y, u, v, w, h, w, cw, sp)
            return rc

        def window(leg, region=False):
            seeds = seed_arrays()
            host = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for k in range(args.warmup):
                assert leg(k, seeds) == 0, lib.vfgs_hip_last_error_string()
            stream.synchronize()
            e0.record(stream)
            if region:
                hip.overlap_begin(sp)
            for k in range(args.warmup, ncalls):
                t0 = time.perf_counter()
                rc = leg(k, seeds)
                host.append((time.perf_counter() - t0) * 1e6)
                assert rc == 0, lib.vfgs_hip_last_error_string()
            if region:
                hip.overlap_end(sp)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / (args.window * nf), host, hip.last_launch_info()["kernel"]

        us = {k: [] for k in "abcd"}
        host_b, host_a, kernels = [], [], {}
        waits0 = hip.seeded_stream_stats()["host_waits"]
        for _ in range(args.rounds):
            for key, leg, region in (("a", leg_a, False), ("b", leg_b, False), ("c", leg_c, False), ("d", leg_b, True)):
                t, host, kern = window(leg, region)
                us[key].append(round(t, 3))
                kernels[key] = kern
                if key == "b":
                    host_b += host
                if key == "a":
                    host_a += host
        st = hip.seeded_stream_stats()
        med = {k: statistics.median(v) for k, v in us.items()}
        rngs = {k: [min(v), max(v)] for k, v in us.items()}
        pixels_bytes = frame_bytes * 2      # every sample read once and written once
        r = {"us_per_frame": us, "kernel": kernels, "median": {k: round(v, 3) for k, v in med.items()}, "min_max": rngs,
             "fraction_of_8TBs_peak_at_median": {k: round(pixels_bytes / (med[k] * 1e-6) / 8e12, 3) for k in med},
             "b_over_a_ratio_of_medians": round(med["b"] / med["a"], 4), "c_over_b_ratio_of_medians": round(med["c"] / med["b"], 4),
             "d_over_b_ratio_of_medians": round(med["d"] / med["b"], 4),
             "b_inside_a_spread": rngs["a"][0] <= med["b"] <= rngs["a"][1],
             "b_spread_entirely_below_c_spread": rngs["b"][1] < rngs["c"][0],
             "host_us_per_call": {"seeded_list_median": round(statistics.median(host_b), 2), "seeded_list_p99": round(float(np.percentile(host_b, 99)), 2),
                                  "seeded_list_max": round(max(host_b), 2), "unseeded_list_median": round(statistics.median(host_a), 2)},
             "image_bytes": int(st["image_words"]) * 4, "slot_waits_in_this_shape": int(st["host_waits"] - waits0),
             "frame_sets_cycled": nsets}
        out["shapes"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        del keep, sets, singles
        torch.cuda.empty_cache()
    lib.vfgs_hip_reset_state()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
