#!/usr/bin/env python3
"""Developer tool: semi-planar surfaces in, planar pictures out (vfgs_hip_add_grain_sp_frame_list_to_planar_dev: P010 -> yuv420p10le,
NV12 -> yuv420p) against what a caller does without it, and what the run-time decision costs the calls whose kernels it lives in, on one
MI355X, in one command.

Part (a), legs alternated, the whole comparison repeated `--rounds` times, device-event windows of `--window` launches after a warm-up of
every leg, out of place, every plane an allocation of its own, uniform random content:
  a  the new call
  b  what a caller does today, three passes: vfgs_hip_add_grain_sp_frame_list_dev out of place into a scratch surface, then torch passes on
     the same stream that de-interleave (Y copied, Cb and Cr split into their planes), then torch passes that shift the three planes down
     (at depth 8 there is nothing to shift: two passes)
  c  the plain out-of-place semi-planar call alone: the bytes of a, so the yardstick for the kernel
Criterion: the whole spread of a lies below the whole spread of b on every shape; a / c is reported, not gated.  Leg a has a parity check
against the oracle on one frame, bit for bit; a failure withholds the numbers.

Part (b), with --parent-lib (the parent commit's libvfgs_hip.so, loaded beside this one: a state of its own): the two existing calls whose
48 kernels gained the decision -- vfgs_hip_add_grain_sp_frame_list_dev and _sp_frame_list_models_dev, in place -- through the parent's
library (P, Pm) and through this one (T, Tm), alternated, over the shapes of tools/sp_model_list_bench.py.  Criterion: this build's median
is no slower than the parent's slowest round.

Writes one JSON document (default profiles/sp_to_planar.json)."""
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
SIZES = {"1080p": (1920, 1080, 32), "2160p": (3840, 2160, 16), "4320p": (7680, 4320, 8)}
# name, trace, depth, sample shift of the source
WORKLOADS = [("P010 to yuv420p10le, fgs_sei", "fgs_sei_10_420", 10, 6), ("NV12 to yuv420p, fgs_sei", "fgs_sei_8_420", 8, 0)]
# part (b): name, width, height, trace, frames per launch: the shapes of tools/sp_model_list_bench.py (profiles/sp_model_list.json), then those
# workloads of tools/bench_semiplanar.py (profiles/semiplanar.json) that are not among them
EXISTING = [("1920x1080 P010 fgs_sei x32", 1920, 1080, "fgs_sei_10_420", 32), ("3840x2160 P010 fgs_afgs1_test1 x16", 3840, 2160, "fgs_afgs1_test1_10_420", 16),
            ("7680x4320 P010 fgs_sei x8", 7680, 4320, "fgs_sei_10_420", 8), ("3840x2160 NV12 fgs_afgs1_test1 x8", 3840, 2160, "fgs_afgs1_test1_8_420", 8),
            ("3840x2160 P010 fgs_sei x16", 3840, 2160, "fgs_sei_10_420", 16), ("1920x1080 NV12 fgs_afgs1_test1 x32", 1920, 1080, "fgs_afgs1_test1_8_420", 32),
            ("3840x2160 NV12 fgs_afgs1_test1 x16", 3840, 2160, "fgs_afgs1_test1_8_420", 16), ("7680x4320 NV12 fgs_afgs1_test1 x8", 7680, 4320, "fgs_afgs1_test1_8_420", 8)]


class Pictures:
    """n semi-planar pictures, the planar destinations, and leg b's scratch surfaces, all on the device"""

    def __init__(self, w, h, n, depth, shift, rng):
        self.w, self.h, self.n, self.depth, self.shift = w, h, n, depth, shift
        f = T.Frame(w, h, depth, 2, 2)
        self.stride, self.cstride, self.uv_stride = f.stride, f.cstride, 2 * f.cstride
        rows, crows = f.Y.shape[0], f.U.shape[0]
        dt, npdt = (torch.int16, np.uint16) if depth > 8 else (torch.uint8, np.uint8)      # (int16: torch shifts; the bits are the containers')

        def src(r, cols):
            a = (rng.integers(0, 1 << depth, (r, cols), dtype=np.uint32) << shift).astype(npdt)
            t = torch.from_numpy(a.view(np.int16) if depth > 8 else a).cuda()
            return [t.clone() for _ in range(n)]

        def dst(r, cols):
            return [torch.full((r, cols), 0x5a, dtype=dt, device="cuda") for _ in range(n)]

        self.sY, self.sUV = src(rows, self.stride), src(crows, self.uv_stride)
        self.qY, self.qUV = dst(rows, self.stride), dst(crows, self.uv_stride)                      # leg b's scratch surfaces, leg c's destinations
        self.dY, self.dU, self.dV = dst(rows, self.stride), dst(crows, self.cstride), dst(crows, self.cstride)
        L = hw.VfgsHip
        self.src = L.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(self.sY, self.sUV)])
        self.scr = L.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(self.qY, self.qUV)])
        self.dst = L.frame_list([(y.data_ptr(), u.data_ptr(), v.data_ptr()) for y, u, v in zip(self.dY, self.dU, self.dV)])

    def leg_a(self, hip, st):
        hip.add_grain_sp_frame_list_to_planar_dev(self.src, self.dst, None, self.w, self.h, self.stride, self.uv_stride, self.stride, self.cstride, self.shift, st)

    def leg_c(self, hip, st):
        hip.add_grain_sp_frame_list_dev(self.src, self.scr, None, self.w, self.h, self.stride, self.uv_stride, self.shift, st)

    def leg_b(self, hip, st):
        self.leg_c(hip, st)
        for qy, quv, dy, du, dv in zip(self.qY, self.qUV, self.dY, self.dU, self.dV):
            pairs = quv.view(quv.shape[0], self.cstride, 2)
            dy.copy_(qy)
            du.copy_(pairs[:, :, 0])
            dv.copy_(pairs[:, :, 1])
        if self.shift:
            # (an arithmetic shift of int16: the bytes moved are those of the logical one, which is what is timed; leg b has no parity check)
            for p in self.dY + self.dU + self.dV:
                p.bitwise_right_shift_(self.shift)

    def parity(self, hip, rec, st):
        """leg a on frame 0 against the oracle, bit for bit, where the call writes"""
        ora = T.OracleHW()
        T.replay(ora, rec)
        hip.set_seed(4711); ora.set_seed(4711)
        torch.cuda.synchronize()
        npdt = np.uint16 if self.depth > 8 else np.uint8
        sp = SP.SPFrame(self.w, self.h, self.depth, 2, self.stride, self.uv_stride, self.shift, self.sY[0].cpu().numpy().view(npdt).copy(), self.sUV[0].cpu().numpy().view(npdt).copy())
        want = SP.to_planar(SP.expected(ora, [sp], None, self.shift)[0])
        self.leg_a(hip, st)
        torch.cuda.synchronize()
        rows, crows, cols = SP.written_region(sp)
        got = [t.cpu().numpy().view(npdt) for t in (self.dY[0], self.dU[0], self.dV[0])]
        return bool(np.array_equal(got[0][:rows, :cols], want.Y[:rows, :cols]) and np.array_equal(got[1][:crows, :cols // 2], want.U[:crows, :cols // 2]) and
                    np.array_equal(got[2][:crows, :cols // 2], want.V[:crows, :cols // 2]))


class ParentLib:
    """the entry points part (b) needs, from another build of the library loaded beside this one (a state of its own)"""

    def __init__(self, path):
        self.lib = C.CDLL(str(path))
        vp, u, i = C.c_void_p, C.c_uint, C.c_int
        spf = C.POINTER(hw.SpFrame)
        for n, a in (("vfgs_set_luma_pattern", [i, vp]), ("vfgs_set_chroma_pattern", [i, vp]), ("vfgs_set_scale_lut", [i, vp]), ("vfgs_set_pattern_lut", [i, vp]),
                     ("vfgs_set_seed", [u]), ("vfgs_set_scale_shift", [i]), ("vfgs_set_depth", [i]), ("vfgs_set_legal_range", [i]),
                     ("vfgs_set_chroma_subsampling", [i, i]), ("vfgs_hip_init", [i]), ("vfgs_hip_model_capture", [C.POINTER(vp), vp]), ("vfgs_hip_model_release", [vp]),
                     ("vfgs_hip_add_grain_sp_frame_list_dev", [spf, spf, C.POINTER(C.c_uint32), u, u, u, u, u, u, vp]),
                     ("vfgs_hip_add_grain_sp_frame_list_models_dev", [spf, spf, C.POINTER(vp), C.POINTER(C.c_uint32), u, u, u, u, u, u, vp]),
                     ("vfgs_hip_last_launch_info", [C.POINTER(hw.LaunchInfo)])):
            getattr(self.lib, n).argtypes = a
        self.lib.vfgs_hip_last_error_string.restype = C.c_char_p
        self.lib.vfgs_hip_reset_state.argtypes = []
        assert self.lib.vfgs_hip_init(0) == 0
        b = hw._b
        self.set_luma_pattern = lambda k, P: self.lib.vfgs_set_luma_pattern(k, b(P))
        self.set_chroma_pattern = lambda k, P: self.lib.vfgs_set_chroma_pattern(k, b(P))
        self.set_scale_lut = lambda c, l: self.lib.vfgs_set_scale_lut(c, b(l))
        self.set_pattern_lut = lambda c, l: self.lib.vfgs_set_pattern_lut(c, b(l))
        self.set_seed = lambda s: self.lib.vfgs_set_seed(s & 0xFFFFFFFF)
        self.set_scale_shift = self.lib.vfgs_set_scale_shift
        self.set_depth = self.lib.vfgs_set_depth
        self.set_legal_range = self.lib.vfgs_set_legal_range
        self.set_chroma_subsampling = self.lib.vfgs_set_chroma_subsampling

    def kernel(self):
        li = hw.LaunchInfo()
        return li.kernel.decode() if self.lib.vfgs_hip_last_launch_info(C.byref(li)) == 0 else None


def part_a(hip, args, stream, out):
    lib, st = hip.lib, stream.cuda_stream
    rng = np.random.default_rng(1)
    failed = False
    for wname, trace, depth, shift in WORKLOADS:
        for sname in args.sizes.split(","):
            w, h, nf = SIZES[sname]
            lib.vfgs_hip_reset_state()
            rec = T.load_trace(trace)
            T.replay(hip, rec)
            pics = Pictures(w, h, nf, depth, shift, rng)
            name = f"{w}x{h} x{nf} {wname}"
            if not pics.parity(hip, rec, st):
                out["feature"][name] = {"parity": False, "note": "parity against the oracle failed: numbers withheld"}
                failed = True
                continue
            legs = {"a": pics.leg_a, "b": pics.leg_b, "c": pics.leg_c}
            for p in legs.values():
                for _ in range(args.warmup):
                    p(hip, st)
            torch.cuda.synchronize()
            us, kern = {k: [] for k in legs}, {}
            for _ in range(args.rounds):
                for k, p in legs.items():
                    ms = C.c_float()
                    hip._ck(lib.vfgs_hip_timer_begin(st))
                    for _ in range(args.window):
                        p(hip, st)
                    hip._ck(lib.vfgs_hip_timer_end(st, C.byref(ms)))
                    us[k].append(round(ms.value * 1e3 / args.window / nf, 3))
                    kern[k] = hip.last_launch_info()["kernel"]
            sz = 2 if depth > 8 else 1
            alg = 2 * sz * (w * h + 2 * (w // 2) * (h // 2))
            med = {k: statistics.median(v) for k, v in us.items()}
            e = {"parity": True, "frames_per_launch": nf, "kernels": kern, "algorithmic_bytes_per_frame": alg,
                 "us_per_frame_median": {k: round(med[k], 3) for k in med}, "us_per_frame_min_max": {k: [min(v), max(v)] for k, v in us.items()},
                 "us_per_frame_rounds": us, "fraction_of_peak": {k: round(alg / (med[k] * 1e-6) / PEAK, 4) for k in ("a", "c")},
                 "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4),
                 "whole_spread_of_a_below_whole_spread_of_b": bool(max(us["a"]) < min(us["b"]))}
            out["feature"][name] = e
            print(name, json.dumps(e["us_per_frame_median"]), "a/b", e["a_over_b"], "a/c", e["a_over_c"], e["whole_spread_of_a_below_whole_spread_of_b"], flush=True)
            del pics
            torch.cuda.empty_cache()
    out["criterion_a_met"] = (not failed) and all(e.get("whole_spread_of_a_below_whole_spread_of_b") for e in out["feature"].values())


def part_b(hip, parent, args, stream, out):
    lib, st = hip.lib, stream.cuda_stream
    rng = np.random.default_rng(2)
    for name, w, h, trace, nf in EXISTING:
        rec = T.load_trace(trace)
        depth, sx, sy = T.trace_geometry(rec)
        lib.vfgs_hip_reset_state(); parent.lib.vfgs_hip_reset_state()
        T.replay(hip, rec); T.replay(parent, rec)
        m_t = hip.model_capture(st)
        m_p = C.c_void_p()
        assert parent.lib.vfgs_hip_model_capture(C.byref(m_p), st) == 0
        shift = 16 - depth if depth > 8 else 0
        sz = 2 if depth > 8 else 1
        frame_bytes = (w * h + w * (h // sy)) * sz
        nsets = max(2, -(-args.pool_mb * (1 << 20) // (frame_bytes * nf)))
        dt, top = (torch.int16, 1 << 10) if depth > 8 else (torch.uint8, 256)
        keep, sets = [], []
        for _ in range(nsets):
            ptrs = []
            for _ in range(nf):
                planes = [torch.randint(0, top, (rows, w), dtype=dt, device="cuda") << shift for rows in (h, h // sy)]
                keep.append(planes)
                ptrs.append(tuple(p.data_ptr() for p in planes))
            sets.append(hip.sp_frame_list([ptrs[i] for i in rng.permutation(nf)]))
        torch.cuda.synchronize()
        mt = (C.c_void_p * nf)(*([m_t] * nf))
        mp = (C.c_void_p * nf)(*([m_p.value] * nf))
        legs = {
            "P": lambda k: parent.lib.vfgs_hip_add_grain_sp_frame_list_dev(sets[k % nsets], sets[k % nsets], None, nf, w, h, w, w, shift, st),
            "T": lambda k: lib.vfgs_hip_add_grain_sp_frame_list_dev(sets[k % nsets], sets[k % nsets], None, nf, w, h, w, w, shift, st),
            "Pm": lambda k: parent.lib.vfgs_hip_add_grain_sp_frame_list_models_dev(sets[k % nsets], sets[k % nsets], mp, None, nf, w, h, w, w, shift, st),
            "Tm": lambda k: lib.vfgs_hip_add_grain_sp_frame_list_models_dev(sets[k % nsets], sets[k % nsets], mt, None, nf, w, h, w, w, shift, st),
        }

        def window(leg):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for k in range(args.warmup):
                assert leg(k) == 0
            stream.synchronize()
            e0.record(stream)
            for k in range(args.warmup, args.warmup + args.window_b):
                assert leg(k) == 0
            e1.record(stream)
            e1.synchronize()
            return round(e0.elapsed_time(e1) * 1e3 / (args.window_b * nf), 3)

        us = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                us[k].append(window(leg))
        med = {k: statistics.median(v) for k, v in us.items()}
        r = {"us_per_frame_rounds": us, "median": {k: round(v, 3) for k, v in med.items()}, "min_max": {k: [min(v), max(v)] for k, v in us.items()},
             "kernels": {"P": parent.kernel(), "T": hip.last_launch_info()["kernel"]}, "frame_sets_cycled": nsets,
             "T_over_P_ratio_of_medians": round(med["T"] / med["P"], 4), "Tm_over_Pm_ratio_of_medians": round(med["Tm"] / med["Pm"], 4),
             "T_median_within_parents_slowest_round": bool(med["T"] <= max(us["P"])), "Tm_median_within_parents_slowest_round": bool(med["Tm"] <= max(us["Pm"]))}
        out["existing_calls"][name] = r
        print(name, json.dumps(r["median"]), "T/P", r["T_over_P_ratio_of_medians"], "Tm/Pm", r["Tm_over_Pm_ratio_of_medians"], flush=True)
        hip.model_release(m_t)
        parent.lib.vfgs_hip_model_release(m_p)
        del keep, sets
        torch.cuda.empty_cache()
    out["criterion_b_met"] = all(r["T_median_within_parents_slowest_round"] and r["Tm_median_within_parents_slowest_round"] for r in out["existing_calls"].values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--window-b", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1080p,2160p,4320p")
    ap.add_argument("--pool-mb", type=int, default=1600, help="part (b): bytes of frames cycled through per shape (beyond the last-level cache)")
    ap.add_argument("--parent-lib", default=None, help="libvfgs_hip.so of the parent commit: part (b) is measured with it, and left out without it")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sp_to_planar.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.rounds >= 5, "the comparison is repeated at least five times"
    hip = hw.VfgsHip(device=0)
    stream = torch.cuda.Stream()
    out = {"what": "semi-planar surfaces in, planar pictures out: legs alternated in one command on one MI355X, %d rounds, device-event windows of %d launches "
                   "(existing calls: %d) after %d warm-up launches of every leg, uniform random content (tools/bench_sp_to_planar.py)" % (args.rounds, args.window, args.window_b, args.warmup),
           "legs": {"a": "vfgs_hip_add_grain_sp_frame_list_to_planar_dev",
                    "b": "vfgs_hip_add_grain_sp_frame_list_dev out of place into a scratch surface, torch passes that de-interleave, torch passes that shift down",
                    "c": "vfgs_hip_add_grain_sp_frame_list_dev out of place alone: the bytes of a",
                    "P / T": "vfgs_hip_add_grain_sp_frame_list_dev in place, the parent commit's library / this library",
                    "Pm / Tm": "vfgs_hip_add_grain_sp_frame_list_models_dev in place, one model on every frame, the parent commit's library / this library"},
           "peak_bytes_per_s": PEAK, "device": hip.device_info(), "feature": {}, "existing_calls": {}}
    with torch.cuda.stream(stream):
        part_a(hip, args, stream, out)
        if args.parent_lib:
            part_b(hip, ParentLib(args.parent_lib), args, stream, out)
    hip.lib.vfgs_hip_reset_state()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out, "criterion (a):", out.get("criterion_a_met"), "criterion (b):", out.get("criterion_b_met"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
