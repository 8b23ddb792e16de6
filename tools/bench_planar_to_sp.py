#!/usr/bin/env python3
"""Developer tool: planar frames in, semi-planar surfaces out (vfgs_hip_add_grain_frame_list_to_sp_dev / _to_sp8_dev: yuv420p10le -> P010 or
NV12, yuv420p -> NV12) against what a caller does without them and against the existing semi-planar calls, on one MI355X, in one process.

Paths, alternated, the whole comparison repeated `--rounds` times, device events around `--window` launches after a warm-up of every path
(vfgs_hip_timer_begin / _end), out of place, every plane an allocation of its own, uniform random content:
  a  the new call
  b  what a caller does today: vfgs_hip_add_grain_frame_list_copy_dev (narrowed: _copy8_dev) into planar scratch, then torch passes on the
     same stream that shift the luma up into the surface and interleave (and shift) Cb and Cr into its UV plane
  c  the existing semi-planar call out of place on the semi-planar twins of the same pictures (vfgs_hip_add_grain_sp_frame_list_dev;
     narrowed: _sp_frame_list_copy8_dev): exactly the bytes of a, so the yardstick for the kernel
Workloads: fgs_sei 10-bit 4:2:0 to P010 and, narrowed, to NV12 at the project's list shapes, and one 8-bit NV12 case.  Every workload has a
parity check of its own against the oracle (paths a and b on one frame, bit for bit); a failure withholds the numbers.
Writes one JSON document (default profiles/planar_to_semiplanar.json): per-frame times of every round, a / b, a / c beside the spread of c
across its rounds (highest minus lowest over the median), fractions of the 8 TB/s peak on the algorithmic bytes (one read and one write of
every sample in its container)."""
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
import planar_to_sp_util as P2  # noqa: E402
import semiplanar_util as SP  # noqa: E402
import vfgs_testlib as T  # noqa: E402
from versatilefilmgrain_amd import hw  # noqa: E402

PEAK = 8e12
SIZES = {"1080p": (1920, 1080, 32), "2160p": (3840, 2160, 16), "4320p": (7680, 4320, 8)}
# name, trace, depth, narrowed, sample shift, sizes
WORKLOADS = [("10-bit 4:2:0 fgs_sei to P010", "fgs_sei_10_420", 10, False, 6, ("1080p", "2160p", "4320p")),
             ("10-bit 4:2:0 fgs_sei to NV12 (narrowed)", "fgs_sei_10_420", 10, True, 0, ("1080p", "2160p", "4320p")),
             ("8-bit 4:2:0 fgs_sei to NV12", "fgs_sei_8_420", 8, False, 0, ("2160p",))]


class Pictures:
    """n planar pictures, their semi-planar twins (path c), the destination surfaces and path b's planar scratch, all on the device"""

    def __init__(self, w, h, n, depth, out8, shift, rng):
        self.w, self.h, self.n, self.depth, self.out8, self.shift = w, h, n, depth, out8, shift
        f = T.Frame(w, h, depth, 2, 2)
        self.stride, self.cstride, self.uv_stride = f.stride, f.cstride, 2 * f.cstride
        rows, crows = f.Y.shape[0], f.U.shape[0]
        sdt, snp = (torch.int16, np.uint16) if depth > 8 else (torch.uint8, np.uint8)      # (int16: torch shifts; the bits are the containers')
        ddt = torch.uint8 if (out8 or depth == 8) else torch.int16

        def src_planes(r, cols):
            a = rng.integers(0, 1 << depth, (r, cols), dtype=np.uint32).astype(snp)
            t = torch.from_numpy(a.view(np.int16) if depth > 8 else a).cuda()
            return [t.clone() for _ in range(n)]

        def dst_planes(r, cols, dt=ddt):
            return [torch.full((r, cols), 0x5a, dtype=dt, device="cuda") for _ in range(n)]

        self.pY, self.pU, self.pV = src_planes(rows, self.stride), src_planes(crows, self.cstride), src_planes(crows, self.cstride)
        # the semi-planar twins of the same pictures, high-aligned where the destination is (path c reads what path a would write without grain)
        tw = shift if not out8 else 6
        self.tw_shift = tw if depth > 8 else 0
        self.tY = [torch.bitwise_left_shift(y, self.tw_shift) if self.tw_shift else y.clone() for y in self.pY]
        self.tUV = []
        for u, v in zip(self.pU, self.pV):
            uv = torch.stack((u, v), dim=2).reshape(crows, self.uv_stride)
            self.tUV.append(torch.bitwise_left_shift(uv, self.tw_shift) if self.tw_shift else uv.contiguous())
        self.dY, self.dUV = dst_planes(rows, self.stride), dst_planes(crows, self.uv_stride)                 # the surfaces
        qdt = torch.uint8 if out8 else sdt
        self.qY, self.qU, self.qV = dst_planes(rows, self.stride, qdt), dst_planes(crows, self.cstride, qdt), dst_planes(crows, self.cstride, qdt)
        L = hw.VfgsHip
        self.psrc = L.frame_list([(y.data_ptr(), u.data_ptr(), v.data_ptr()) for y, u, v in zip(self.pY, self.pU, self.pV)])
        self.pscr = L.frame_list([(y.data_ptr(), u.data_ptr(), v.data_ptr()) for y, u, v in zip(self.qY, self.qU, self.qV)])
        self.tsrc = L.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(self.tY, self.tUV)])
        self.dst = L.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(self.dY, self.dUV)])

    def path_a(self, hip, st):
        if self.out8:
            hip.add_grain_frame_list_to_sp8_dev(self.psrc, self.dst, None, self.w, self.h, self.stride, self.cstride, self.stride, self.uv_stride, st)
        else:
            hip.add_grain_frame_list_to_sp_dev(self.psrc, self.dst, None, self.w, self.h, self.stride, self.cstride, self.stride, self.uv_stride, self.shift, st)

    def path_b(self, hip, st):
        if self.out8:
            hip.add_grain_frame_list_copy8_dev(self.psrc, self.pscr, self.w, self.h, self.stride, self.cstride, self.stride, self.cstride, st)
        else:
            hip.add_grain_frame_list_copy_dev(self.psrc, self.pscr, self.w, self.h, self.stride, self.cstride, st)
        sh = 0 if self.out8 else self.shift
        for qy, qu, qv, dy, duv in zip(self.qY, self.qU, self.qV, self.dY, self.dUV):
            pairs = duv.view(duv.shape[0], self.cstride, 2)
            if sh:
                torch.bitwise_left_shift(qy, sh, out=dy)
                torch.bitwise_left_shift(qu, sh, out=pairs[:, :, 0])
                torch.bitwise_left_shift(qv, sh, out=pairs[:, :, 1])
            else:
                dy.copy_(qy)
                pairs[:, :, 0].copy_(qu)
                pairs[:, :, 1].copy_(qv)

    def path_c(self, hip, st):
        if self.out8:
            hip.add_grain_sp_frame_list_copy8_dev(self.tsrc, self.dst, None, self.w, self.h, self.stride, self.uv_stride, self.stride, self.uv_stride, self.tw_shift, st)
        else:
            hip.add_grain_sp_frame_list_dev(self.tsrc, self.dst, None, self.w, self.h, self.stride, self.uv_stride, self.tw_shift, st)

    def source(self, i):
        torch.cuda.synchronize()
        f = T.Frame(self.w, self.h, self.depth, 2, 2)
        for p, t in zip(f.planes(), (self.pY[i], self.pU[i], self.pV[i])):
            p[...] = t.cpu().numpy().view(f.dtype)
        return f

    def destination(self, i):
        torch.cuda.synchronize()
        dt = np.uint8 if (self.out8 or self.depth == 8) else np.uint16
        return SP.SPFrame(self.w, self.h, 8 if self.out8 else self.depth, 2, self.stride, self.uv_stride, 0 if self.out8 else self.shift,
                          self.dY[i].cpu().numpy().view(dt).copy(), self.dUV[i].cpu().numpy().view(dt).copy())


def parity(hip, rec, pics, st):
    """paths a and b from the same seed: frame 0's surface against the oracle, bit for bit, where the call writes"""
    ok = True
    for path in (pics.path_a, pics.path_b):
        ora = T.OracleHW()
        T.replay(ora, rec)
        hip.set_seed(4711); ora.set_seed(4711)
        src = pics.source(0)
        for t in pics.dY + pics.dUV:
            t.fill_(0x5a)
        fill = pics.destination(0)
        want = (P2.expected8(ora, [src], None, fill) if pics.out8 else P2.expected(ora, [src], None, pics.shift, fill))[0]
        path(hip, st)
        got = pics.destination(0)
        rows, crows, cols = SP.written_region(fill)
        ok = ok and np.array_equal(got.Y[:rows, :cols], want.Y[:rows, :cols]) and np.array_equal(got.UV[:crows, :cols], want.UV[:crows, :cols])
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="0,1,2")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "planar_to_semiplanar.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.rounds >= 5, "the comparison is repeated at least five times"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    rng = np.random.default_rng(1)
    out = {"what": "planar frames in, semi-planar surfaces out: paths alternated in one process on one MI355X, %d rounds, device-event windows of %d "
                   "launches after %d warm-up launches of every path, out of place, every plane an allocation of its own, uniform random content "
                   "(tools/bench_planar_to_sp.py)" % (args.rounds, args.window, args.warmup),
           "paths": {"a": "vfgs_hip_add_grain_frame_list_to_sp_dev (narrowed: _to_sp8_dev)",
                     "b": "vfgs_hip_add_grain_frame_list_copy_dev (narrowed: _copy8_dev) into planar scratch, then torch passes that shift and interleave into the surface",
                     "c": "vfgs_hip_add_grain_sp_frame_list_dev (narrowed: _sp_frame_list_copy8_dev) out of place on the semi-planar twins: the bytes of a"},
           "peak_bytes_per_s": PEAK, "device": hip.device_info(), "workloads": {}}
    failed = False
    with torch.cuda.stream(stream):
        for wi in [int(x) for x in args.workloads.split(",")]:
            wname, trace, depth, out8, shift, sizes = WORKLOADS[wi]
            for sname in sizes:
                w, h, nf = SIZES[sname]
                lib.vfgs_hip_reset_state()
                rec = T.load_trace(trace)
                T.replay(hip, rec)
                pics = Pictures(w, h, nf, depth, out8, shift, rng)
                name = f"{w}x{h} x{nf} {wname}"
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
                kern = {}
                for _ in range(args.rounds):
                    for k, p in paths.items():
                        ms = C.c_float()
                        hip._ck(lib.vfgs_hip_timer_begin(st))
                        for _ in range(args.window):
                            p(hip, st)
                        hip._ck(lib.vfgs_hip_timer_end(st, C.byref(ms)))
                        us[k].append(ms.value * 1e3 / args.window / nf)
                        kern[k] = hip.last_launch_info()["kernel"]
                sz_in, sz_out = (2 if depth > 8 else 1), (1 if (out8 or depth == 8) else 2)
                alg = (sz_in + sz_out) * (w * h + 2 * (w // 2) * (h // 2))
                med = {k: statistics.median(v) for k, v in us.items()}
                spread = (max(us["c"]) - min(us["c"])) / med["c"]
                e = {"parity": True, "frames_per_launch": nf, "kernels": kern, "algorithmic_bytes_per_frame": alg,
                     "us_per_frame": {k: round(med[k], 3) for k in med},
                     "us_per_frame_rounds": {k: [round(x, 3) for x in v] for k, v in us.items()},
                     "c_spread_pct": round(100 * spread, 2),
                     "fraction_of_peak": {k: round(alg / (med[k] * 1e-6) / PEAK, 4) for k in ("a", "c")},
                     "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4),
                     "a_inside_c_spread": bool(abs(med["a"] / med["c"] - 1) <= spread),
                     "every_round_of_a_faster_than_every_round_of_b": bool(max(us["a"]) < min(us["b"]))}
                out["workloads"][name] = e
                print(name, json.dumps(e["us_per_frame"]), "c spread %", e["c_spread_pct"], "a/b", e["a_over_b"], "a/c", e["a_over_c"], flush=True)
                del pics
                torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
