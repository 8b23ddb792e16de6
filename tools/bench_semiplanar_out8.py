#!/usr/bin/env python3
"""Developer tool: semi-planar frames with the narrowed 8-bit destination (vfgs_hip_add_grain_sp_frame_list_copy8_dev, P010 -> NV12)
against the planar _copy8 list and against what a caller with decoder surfaces does without it, on one MI355X, in one process.

Paths, alternated, the whole comparison repeated `--rounds` times, device events around `--window` launches after a warm-up of every path
(vfgs_hip_timer_begin / _end), out of place, every plane an allocation of its own, uniform random content:
  a  vfgs_hip_add_grain_sp_frame_list_copy8_dev, P010 -> NV12
  b  vfgs_hip_add_grain_frame_list_copy8_dev on the planar twins (the yardstick: kernels this work does not touch)
  c  what a caller does today: vfgs_hip_add_grain_sp_frame_list_dev out of place into a P010 scratch surface, then torch passes on the same
     stream that shift, round and cast both planes to NV12 (per plane: >> 6, + 2, >> 2 into a 16-bit scratch plane, and the cast copy)
Workloads: P010 fgs_sei 10-bit 4:2:0 at the project's list shapes.  Every workload has a parity check of its own against the oracle (paths
a and c on one frame, bit for bit); a failure withholds the numbers.
Writes one JSON document (default profiles/semiplanar_out8.json): per-frame times of every round, the spread of b across its rounds (highest
minus lowest over the median), whether a lies inside it, fractions of the 8 TB/s peak on the algorithmic bytes (one 16-bit read + one 8-bit
write of every sample, the same for a and b)."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import semiplanar_out8_util as SP8  # noqa: E402
import semiplanar_util as SP  # noqa: E402
import vfgs_testlib as T  # noqa: E402
from versatilefilmgrain_amd import hw  # noqa: E402

PEAK = 8e12
SIZES = [("1920x1080 x32", 1920, 1080, 32), ("3840x2160 x16", 3840, 2160, 16), ("7680x4320 x8", 7680, 4320, 8)]
TRACE, DEPTH, SHIFT = "fgs_sei_10_420", 10, 6


class Pictures:
    """n P010 pictures, their planar twins, the NV12 / planar 8-bit destinations and path c's scratch on the device"""

    def __init__(self, w, h, n, rng):
        self.w, self.h, self.n = w, h, n
        f = T.Frame(w, h, DEPTH, 2, 2)
        self.stride, self.cstride, self.uv_stride = f.stride, f.cstride, 2 * f.cstride
        rows, crows = f.Y.shape[0], f.U.shape[0]

        def planes(r, cols, sh):
            # (one random plane of each kind, a device copy per picture: separate allocations; int16: torch shifts, the bits are the containers')
            a = (rng.integers(0, 1 << DEPTH, (r, cols), dtype=np.uint32) << sh).astype(np.uint16)
            t = torch.from_numpy(a.view(np.int16)).cuda()
            return [t.clone() for _ in range(n)]

        def bytes_(r, cols):
            return [torch.full((r, cols), 0x5a, dtype=torch.uint8, device="cuda") for _ in range(n)]

        self.Y, self.UV = planes(rows, self.stride, SHIFT), planes(crows, self.uv_stride, SHIFT)
        self.pY, self.pU, self.pV = planes(rows, self.stride, 0), planes(crows, self.cstride, 0), planes(crows, self.cstride, 0)
        self.dY, self.dUV = bytes_(rows, self.stride), bytes_(crows, self.uv_stride)                       # NV12, pitches in bytes
        self.qY, self.qU, self.qV = bytes_(rows, self.stride), bytes_(crows, self.cstride), bytes_(crows, self.cstride)
        self.sY, self.sUV = [torch.empty_like(t) for t in self.Y], [torch.empty_like(t) for t in self.UV]  # path c: the P010 scratch surfaces
        self.tY, self.tUV = torch.empty_like(self.Y[0]), torch.empty_like(self.UV[0])                     # ... and one 16-bit plane of each kind
        L = hw.VfgsHip
        self.src = L.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(self.Y, self.UV)])
        self.dst = L.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(self.dY, self.dUV)])
        self.scr = L.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(self.sY, self.sUV)])
        self.psrc = L.frame_list([(y.data_ptr(), u.data_ptr(), v.data_ptr()) for y, u, v in zip(self.pY, self.pU, self.pV)])
        self.pdst = L.frame_list([(y.data_ptr(), u.data_ptr(), v.data_ptr()) for y, u, v in zip(self.qY, self.qU, self.qV)])

    def path_a(self, hip, st):
        hip.add_grain_sp_frame_list_copy8_dev(self.src, self.dst, None, self.w, self.h, self.stride, self.uv_stride, self.stride, self.uv_stride, SHIFT, st)

    def path_b(self, hip, st):
        hip.add_grain_frame_list_copy8_dev(self.psrc, self.pdst, self.w, self.h, self.stride, self.cstride, self.stride, self.cstride, st)

    def path_c(self, hip, st):
        hip.add_grain_sp_frame_list_dev(self.src, self.scr, None, self.w, self.h, self.stride, self.uv_stride, SHIFT, st)
        # (arithmetic shifts of the int16 containers: a sample of 512 and more comes out 256 too low, which the cast to uint8 drops)
        for s, t, d in [(s, self.tY, d) for s, d in zip(self.sY, self.dY)] + [(s, self.tUV, d) for s, d in zip(self.sUV, self.dUV)]:
            torch.bitwise_right_shift(s, SHIFT, out=t)
            t.add_(2)
            t.bitwise_right_shift_(2)
            d.copy_(t)

    def source(self, i):
        torch.cuda.synchronize()
        return SP.SPFrame(self.w, self.h, DEPTH, 2, self.stride, self.uv_stride, SHIFT,
                          self.Y[i].cpu().numpy().view(np.uint16).copy(), self.UV[i].cpu().numpy().view(np.uint16).copy())

    def destination(self, i):
        torch.cuda.synchronize()
        return SP.SPFrame(self.w, self.h, 8, 2, self.stride, self.uv_stride, 0, self.dY[i].cpu().numpy().copy(), self.dUV[i].cpu().numpy().copy())


def parity(hip, rec, pics, st):
    """paths a and c from the same seed: frame 0's destination against the oracle, bit for bit, where the call writes"""
    ok = True
    for path in (pics.path_a, pics.path_c):
        ora = T.OracleHW()
        T.replay(ora, rec)
        hip.set_seed(4711); ora.set_seed(4711)
        src = pics.source(0)
        for t in pics.dY + pics.dUV:
            t.fill_(0x5a)
        want = SP8.expected8(ora, [src], None, SHIFT, pics.destination(0))[0]
        path(hip, st)
        got = pics.destination(0)
        rows, crows, cols = SP.written_region(src)
        ok = ok and np.array_equal(got.Y[:rows, :cols], want.Y[:rows, :cols]) and np.array_equal(got.UV[:crows, :cols], want.UV[:crows, :cols])
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="0,1,2")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "semiplanar_out8.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.rounds >= 5, "the comparison is repeated at least five times"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    rng = np.random.default_rng(1)
    out = {"what": "semi-planar frames with the narrowed 8-bit destination (P010 -> NV12): paths alternated in one process on one MI355X, %d rounds, "
                   "device-event windows of %d launches after %d warm-up launches of every path, out of place, every plane an allocation of its own, "
                   "uniform random content (tools/bench_semiplanar_out8.py)" % (args.rounds, args.window, args.warmup),
           "paths": {"a": "vfgs_hip_add_grain_sp_frame_list_copy8_dev", "b": "vfgs_hip_add_grain_frame_list_copy8_dev on the planar twins",
                     "c": "vfgs_hip_add_grain_sp_frame_list_dev out of place into a P010 scratch surface, then torch passes that shift, round and "
                          "cast both planes to NV12"},
           "peak_bytes_per_s": PEAK, "device": hip.device_info(), "workloads": {}}
    failed = False
    with torch.cuda.stream(stream):
        for si in [int(x) for x in args.sizes.split(",")]:
            sname, w, h, nf = SIZES[si]
            lib.vfgs_hip_reset_state()
            rec = T.load_trace(TRACE)
            T.replay(hip, rec)
            pics = Pictures(w, h, nf, rng)
            name = f"{sname} P010 fgs_sei 10-bit 4:2:0"
            if not parity(hip, rec, pics, st):
                out["workloads"][name] = {"parity": False, "note": "parity against the oracle failed: numbers withheld"}
                failed = True
                continue
            paths = {"a": pics.path_a, "b": pics.path_b, "c": pics.path_c}
            for p in paths.values():
                for _ in range(args.warmup):
                    p(hip, st)
            torch.cuda.synchronize()
            us = {k: [] for k in paths}
            for _ in range(args.rounds):
                for k, p in paths.items():
                    ms = C.c_float()
                    hip._ck(lib.vfgs_hip_timer_begin(st))
                    for _ in range(args.window):
                        p(hip, st)
                    hip._ck(lib.vfgs_hip_timer_end(st, C.byref(ms)))
                    us[k].append(ms.value * 1e3 / args.window / nf)
            pics.path_a(hip, st)
            info = hip.last_launch_info()
            alg = 3 * (w * h + 2 * (w // 2) * (h // 2))
            med = {k: statistics.median(v) for k, v in us.items()}
            spread = (max(us["b"]) - min(us["b"])) / med["b"]
            e = {"parity": True, "frames_per_launch": nf, "kernel_a": info["kernel"], "algorithmic_bytes_per_frame": alg,
                 "us_per_frame": {k: round(med[k], 3) for k in med},
                 "us_per_frame_rounds": {k: [round(x, 3) for x in v] for k, v in us.items()},
                 "b_spread_pct": round(100 * spread, 2),
                 "fraction_of_peak": {k: round(alg / (med[k] * 1e-6) / PEAK, 4) for k in ("a", "b")},
                 "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4),
                 "a_inside_b_spread": bool(abs(med["a"] / med["b"] - 1) <= spread),
                 "every_round_of_a_faster_than_every_round_of_c": bool(max(us["a"]) < min(us["c"]))}
            out["workloads"][name] = e
            print(name, json.dumps(e["us_per_frame"]), "b spread %", e["b_spread_pct"], "a/b", e["a_over_b"], "a/c", e["a_over_c"], flush=True)
            del pics
            torch.cuda.empty_cache()
    out["condition_a_faster_than_c_everywhere"] = (not failed) and all(e.get("every_round_of_a_faster_than_every_round_of_c") for e in out["workloads"].values())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out, "condition:", out["condition_a_faster_than_c_everywhere"])
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
