#!/usr/bin/env python3
"""Developer tool: semi-planar frames (vfgs_hip_add_grain_sp_frame_list_dev) against the planar list and against what a caller with
decoder surfaces does without it, on one MI355X, in one process.

Paths, alternated, the whole comparison repeated `--rounds` times, device events around `--window` launches after a warm-up of every
shape (vfgs_hip_timer_begin / _end), in place, every plane an allocation of its own, uniform random content:
  a  vfgs_hip_add_grain_sp_frame_list_dev on the semi-planar pictures
  b  vfgs_hip_add_grain_frame_list_dev on their planar twins (the yardstick: kernels this work does not touch)
  c  what a caller does today: de-interleave the UV plane into scratch planes (and shift every plane down where the samples sit in the high
     bits), b on the scratch planes, interleave (and shift) back -- plain torch copies on the same stream
Workloads: the project's list shapes, each as P010 (fgs_sei 10-bit, shift 6) and as NV12 (fgs_afgs1_test1 8-bit).  Every workload has a
parity check of its own against the oracle (paths a and c on one frame, bit for bit); a failure withholds the numbers.
Writes one JSON document (default profiles/semiplanar.json): per-frame times, the spread of b across its repeats, fractions of the 8 TB/s
peak on the algorithmic bytes (one read + one write of every sample, the same for a and b)."""
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
import semiplanar_util as SP  # noqa: E402
import vfgs_testlib as T  # noqa: E402
from versatilefilmgrain_amd import hw  # noqa: E402

PEAK = 8e12
SIZES = [("1920x1080 x32", 1920, 1080, 32), ("3840x2160 x16", 3840, 2160, 16), ("7680x4320 x8", 7680, 4320, 8)]
FORMS = [("P010 fgs_sei 10-bit 4:2:0", "fgs_sei_10_420", 6), ("NV12 fgs_afgs1_test1 8-bit 4:2:0", "fgs_afgs1_test1_8_420", 0)]


class Pictures:
    """n semi-planar pictures and their planar twins + scratch planes on the device"""

    def __init__(self, w, h, depth, shift, n, rng):
        self.w, self.h, self.depth, self.shift, self.n = w, h, depth, shift, n
        f = T.Frame(w, h, depth, 2, 2)
        self.stride, self.cstride, self.uv_stride = f.stride, f.cstride, 2 * f.cstride
        self.dt = torch.int16 if depth > 8 else torch.uint8      # (int16: torch shifts; the bits are the containers')
        npdt = np.uint16 if depth > 8 else np.uint8

        def planes(rows, cols, sh):
            # (one random plane of each kind, a device copy per picture: separate allocations, seconds of host time saved)
            a = (rng.integers(0, 1 << depth, (rows, cols), dtype=np.uint32) << sh).astype(npdt)
            t = torch.from_numpy(a.view(np.int16) if depth > 8 else a).cuda()
            return [t.clone() for _ in range(n)]

        self.Y = planes(f.Y.shape[0], self.stride, shift)
        self.UV = planes(f.U.shape[0], self.uv_stride, shift)
        self.pY = planes(f.Y.shape[0], self.stride, 0)
        self.pU = planes(f.U.shape[0], self.cstride, 0)
        self.pV = planes(f.U.shape[0], self.cstride, 0)
        self.sU = [torch.empty_like(t) for t in self.pU]
        self.sV = [torch.empty_like(t) for t in self.pV]
        self.sp_list = hw.VfgsHip.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(self.Y, self.UV)])
        self.pl_list = hw.VfgsHip.frame_list([(y.data_ptr(), u.data_ptr(), v.data_ptr()) for y, u, v in zip(self.pY, self.pU, self.pV)])
        self.sc_list = hw.VfgsHip.frame_list([(y.data_ptr(), u.data_ptr(), v.data_ptr()) for y, u, v in zip(self.Y, self.sU, self.sV)])
        self.mask = (1 << depth) - 1

    def path_a(self, hip, st):
        hip.add_grain_sp_frame_list_dev(self.sp_list, None, None, self.w, self.h, self.stride, self.uv_stride, self.shift, st)

    def path_b(self, hip, st):
        hip.add_grain_frame_list_dev(self.pl_list, self.w, self.h, self.stride, self.cstride, st)

    def path_c(self, hip, st):
        sh = self.shift
        for y, uv, u, v in zip(self.Y, self.UV, self.sU, self.sV):
            if sh:
                torch.bitwise_right_shift(uv[:, 0::2], sh, out=u); u.bitwise_and_(self.mask)
                torch.bitwise_right_shift(uv[:, 1::2], sh, out=v); v.bitwise_and_(self.mask)
                y.bitwise_right_shift_(sh); y.bitwise_and_(self.mask)
            else:
                u.copy_(uv[:, 0::2]); v.copy_(uv[:, 1::2])
        hip.add_grain_frame_list_dev(self.sc_list, self.w, self.h, self.stride, self.cstride, st)
        for y, uv, u, v in zip(self.Y, self.UV, self.sU, self.sV):
            if sh:
                torch.bitwise_left_shift(u, sh, out=uv[:, 0::2])
                torch.bitwise_left_shift(v, sh, out=uv[:, 1::2])
                y.bitwise_left_shift_(sh)
            else:
                uv[:, 0::2].copy_(u); uv[:, 1::2].copy_(v)

    def sp_frame(self, i):
        npdt = np.uint16 if self.depth > 8 else np.uint8
        torch.cuda.synchronize()
        return SP.SPFrame(self.w, self.h, self.depth, 2, self.stride, self.uv_stride, self.shift,
                          self.Y[i].cpu().numpy().view(npdt).copy(), self.UV[i].cpu().numpy().view(npdt).copy())


def parity(hip, rec, pics, st):
    """paths a and c on the pictures as they are, from the same seed: frame 0 against the oracle, bit for bit"""
    ok = True
    for path in (pics.path_a, pics.path_c):
        ora = T.OracleHW()
        T.replay(ora, rec)
        hip.set_seed(4711); ora.set_seed(4711)
        src = [pics.sp_frame(0)]
        want = SP.expected(ora, src, None, pics.shift)[0]
        path(hip, st)
        got = pics.sp_frame(0)
        rows, crows, cols = SP.written_region(want)
        ok = ok and np.array_equal(got.Y[:rows, :cols], want.Y[:rows, :cols]) and np.array_equal(got.UV[:crows, :cols], want.UV[:crows, :cols])
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="0,1,2")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "semiplanar.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.rounds >= 5, "the comparison is repeated at least five times"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    rng = np.random.default_rng(1)
    out = {"what": "semi-planar frames: paths alternated in one process on one MI355X, %d rounds, device-event windows of %d launches after %d "
                   "warm-up launches of every path, in place, every plane an allocation of its own, uniform random content "
                   "(tools/bench_semiplanar.py)" % (args.rounds, args.window, args.warmup),
           "paths": {"a": "vfgs_hip_add_grain_sp_frame_list_dev", "b": "vfgs_hip_add_grain_frame_list_dev on the planar twins",
                     "c": "de-interleave (and shift) into scratch planes with torch copies, path b's call, interleave (and shift) back"},
           "peak_bytes_per_s": PEAK, "device": hip.device_info(), "workloads": {}}
    failed = False
    with torch.cuda.stream(stream):
        for si in [int(x) for x in args.sizes.split(",")]:
            sname, w, h, nf = SIZES[si]
            for fname, trace, shift in FORMS:
                lib.vfgs_hip_reset_state()
                rec = T.load_trace(trace)
                T.replay(hip, rec)
                depth = T.trace_geometry(rec)[0]
                pics = Pictures(w, h, depth, shift, nf, rng)
                name = f"{sname} {fname}"
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
                info = None
                pics.path_a(hip, st)
                info = hip.last_launch_info()
                sz = 2 if depth > 8 else 1
                alg = 2 * sz * (w * h + 2 * (w // 2) * (h // 2))
                med = {k: statistics.median(v) for k, v in us.items()}
                e = {"parity": True, "frames_per_launch": nf, "kernel_a": info["kernel"], "algorithmic_bytes_per_frame": alg,
                     "us_per_frame": {k: round(med[k], 3) for k in med},
                     "us_per_frame_rounds": {k: [round(x, 3) for x in v] for k, v in us.items()},
                     "b_spread_pct": round(100 * (max(us["b"]) - min(us["b"])) / med["b"], 2),
                     "fraction_of_peak": {k: round(alg / (med[k] * 1e-6) / PEAK, 4) for k in ("a", "b")},
                     "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4),
                     "a_faster_than_c": bool(max(us["a"]) < min(us["c"]))}
                out["workloads"][name] = e
                print(name, json.dumps(e["us_per_frame"]), "b spread %", e["b_spread_pct"], "a/b", e["a_over_b"], "a/c", e["a_over_c"], flush=True)
                del pics
                torch.cuda.empty_cache()
    out["condition_a_faster_than_c_everywhere"] = (not failed) and all(e.get("a_faster_than_c") for e in out["workloads"].values())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out, "condition:", out["condition_a_faster_than_c_everywhere"])
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
