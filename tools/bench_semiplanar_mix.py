#!/usr/bin/env python3
"""Developer tool: semi-planar frames under an active luma / chroma mix (vfgs_hip_add_grain_sp_frame_list_dev + vfgs_hip_set_chroma_mix)
against the planar kernels of the mix and against what a caller with decoder surfaces had to do without it, on one MI355X, in one process.

Paths, alternated, the whole comparison repeated `--rounds` times, device events around `--window` launches after a warm-up of every
path (vfgs_hip_timer_begin / _end), every plane an allocation of its own, content uniform in 0.3 .. 0.7 of the range, mix (32, 32, 0) on
both components, each workload in place and out of place:
  a  the semi-planar call under the mix (grain_sp_mix_kernel)
  b  vfgs_hip_add_grain_frame_list_dev / _copy_dev under the same mix on the planar twins (grain_mix_kernel: the yardstick, untouched)
  c  what a caller did before: de-interleave the UV plane into scratch planes (and shift every plane down where the samples sit in the high
     bits), b's in-place call on the scratch planes, interleave (and shift) back into the destination -- plain torch copies on the same stream
  d  the semi-planar call with the mix off (grain_sp_kernel): the same bytes but for the luma a UV workgroup reads, 7N / 6N at 4:2:0
Workloads: the project's list shapes, fgs_afgs1_test1 as NV12 (8 bit) and as P010 (10 bit, shift 6).  Every workload has a parity check of
its own (path a on one frame against tests/semiplanar_mix_util.py, bit for bit, no sample excluded); a failure withholds the numbers.
Writes one JSON document (default profiles/semiplanar_mix.json).

--merge-only adds what is measured outside this process to that document, without a GPU:
  --objdump-json  the comparison of `llvm-objdump -d` of the untouched kernel families with the parent build's (`existing_kernels_objdump`)
  --bench-py-jsonl  lines {"tree": "parent" | "this", "result": <bench.py's JSON line>} of alternated bench.py runs (`bench_py`: the headline value
                  of every run, this tree's median, the parent's range and whether the median lies inside it)"""
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
import semiplanar_mix_util as M  # noqa: E402
import semiplanar_util as SP  # noqa: E402
import vfgs_testlib as T  # noqa: E402
from versatilefilmgrain_amd import hw  # noqa: E402

PEAK = 8e12
MIX = (32, 32, 0)
SIZES = [("1920x1080 x32", 1920, 1080, 32), ("3840x2160 x16", 3840, 2160, 16), ("7680x4320 x8", 7680, 4320, 8)]
FORMS = [("NV12 fgs_afgs1_test1 8-bit 4:2:0", "fgs_afgs1_test1_8_420", 0), ("P010 fgs_afgs1_test1 10-bit 4:2:0", "fgs_afgs1_test1_10_420", 6)]


class Pictures:
    """n semi-planar pictures, destinations, planar twins and scratch planes on the device"""

    def __init__(self, w, h, depth, shift, n, rng, in_place):
        self.w, self.h, self.depth, self.shift, self.n, self.in_place = w, h, depth, shift, n, in_place
        f = T.Frame(w, h, depth, 2, 2)
        self.stride, self.cstride, self.uv_stride = f.stride, f.cstride, 2 * f.cstride
        npdt = np.uint16 if depth > 8 else np.uint8
        lo, hi = int(0.3 * (1 << depth)), int(0.7 * (1 << depth))

        def planes(rows, cols, sh):
            # (one random plane of each kind, a device copy per picture: separate allocations)
            a = (rng.integers(lo, hi, (rows, cols), dtype=np.uint32) << sh).astype(npdt)
            t = torch.from_numpy(a.view(np.int16) if depth > 8 else a).cuda()
            return [t.clone() for _ in range(n)]

        rows, crows = f.Y.shape[0], f.U.shape[0]
        self.Y, self.UV = planes(rows, self.stride, shift), planes(crows, self.uv_stride, shift)
        self.pY, self.pU, self.pV = planes(rows, self.stride, 0), planes(crows, self.cstride, 0), planes(crows, self.cstride, 0)
        self.sY = [torch.empty_like(t) for t in self.Y] if (shift or not in_place) else self.Y      # (c's scratch luma: the source must stay)
        self.sU, self.sV = [torch.empty_like(t) for t in self.pU], [torch.empty_like(t) for t in self.pV]
        if in_place:
            self.dY, self.dUV, self.qY, self.qU, self.qV = self.Y, self.UV, self.pY, self.pU, self.pV
        else:
            self.dY, self.dUV = [torch.empty_like(t) for t in self.Y], [torch.empty_like(t) for t in self.UV]
            self.qY, self.qU, self.qV = ([torch.empty_like(t) for t in p] for p in (self.pY, self.pU, self.pV))
        sp = lambda ys, uvs: hw.VfgsHip.sp_frame_list([(y.data_ptr(), uv.data_ptr()) for y, uv in zip(ys, uvs)])
        pl = lambda ys, us, vs: hw.VfgsHip.frame_list([(y.data_ptr(), u.data_ptr(), v.data_ptr()) for y, u, v in zip(ys, us, vs)])
        self.sp_src, self.sp_dst = sp(self.Y, self.UV), sp(self.dY, self.dUV)
        self.pl_src, self.pl_dst = pl(self.pY, self.pU, self.pV), pl(self.qY, self.qU, self.qV)
        self.sc_list = pl(self.sY, self.sU, self.sV)
        self.mask = (1 << depth) - 1

    def sp_call(self, hip, st):
        hip.add_grain_sp_frame_list_dev(self.sp_src, None if self.in_place else self.sp_dst, None, self.w, self.h, self.stride, self.uv_stride, self.shift, st)

    def path_a(self, hip, st):
        self.sp_call(hip, st)

    def path_b(self, hip, st):
        if self.in_place:
            hip.add_grain_frame_list_dev(self.pl_src, self.w, self.h, self.stride, self.cstride, st)
        else:
            hip.add_grain_frame_list_copy_dev(self.pl_src, self.pl_dst, self.w, self.h, self.stride, self.cstride, st)

    def path_c(self, hip, st):
        sh = self.shift
        for y, uv, sy, u, v in zip(self.Y, self.UV, self.sY, self.sU, self.sV):
            if sh:
                torch.bitwise_right_shift(uv[:, 0::2], sh, out=u); u.bitwise_and_(self.mask)
                torch.bitwise_right_shift(uv[:, 1::2], sh, out=v); v.bitwise_and_(self.mask)
                torch.bitwise_right_shift(y, sh, out=sy); sy.bitwise_and_(self.mask)
            else:
                u.copy_(uv[:, 0::2]); v.copy_(uv[:, 1::2])
                if sy is not y:
                    sy.copy_(y)
        hip.add_grain_frame_list_dev(self.sc_list, self.w, self.h, self.stride, self.cstride, st)
        for dy, duv, sy, u, v in zip(self.dY, self.dUV, self.sY, self.sU, self.sV):
            if sh:
                torch.bitwise_left_shift(u, sh, out=duv[:, 0::2])
                torch.bitwise_left_shift(v, sh, out=duv[:, 1::2])
                torch.bitwise_left_shift(sy, sh, out=dy)
            else:
                duv[:, 0::2].copy_(u); duv[:, 1::2].copy_(v)
                if dy is not sy:
                    dy.copy_(sy)

    def frame(self, ys, uvs, i):
        npdt = np.uint16 if self.depth > 8 else np.uint8
        torch.cuda.synchronize()
        return SP.SPFrame(self.w, self.h, self.depth, 2, self.stride, self.uv_stride, self.shift,
                          ys[i].cpu().numpy().view(npdt).copy(), uvs[i].cpu().numpy().view(npdt).copy())


def set_mix(hip, on):
    hip.clear_chroma_mix()
    if on:
        hip.set_chroma_mix(1, *MIX)
        hip.set_chroma_mix(2, *MIX)


def parity(hip, rec, pics, st):
    """path a on the pictures as they are, from a known seed: frame 0 against the derivation on the oracle, bit for bit"""
    ora = T.OracleHW()
    T.replay(ora, rec)
    hip.set_seed(4711); ora.set_seed(4711)
    src = pics.frame(pics.Y, pics.UV, 0)
    (want, mask), excluded = (lambda r: (r[0][0], r[1]))(M.expected(ora, rec, [src], None, pics.shift, (MIX, MIX)))
    pics.path_a(hip, st)
    got = pics.frame(pics.dY, pics.dUV, 0)
    rows, crows, cols = SP.written_region(want)
    return bool(excluded == 0 and np.array_equal(got.Y[:rows, :cols], want.Y[:rows, :cols]) and np.array_equal(got.UV[:crows, :cols], want.UV[:crows, :cols]))


def merge(args):
    out = json.loads(Path(args.out).read_text())
    if args.objdump_json:
        out["existing_kernels_objdump"] = json.loads(Path(args.objdump_json).read_text())
    if args.bench_py_jsonl:
        runs = {"parent": [], "this": []}
        for line in Path(args.bench_py_jsonl).read_text().splitlines():
            if line.strip():
                r = json.loads(line)
                runs[r["tree"]].append(r["result"])
        key = args.bench_py_key
        p, t = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
        assert len(p) >= 3 and len(t) >= 3, "three runs of each tree"
        out["bench_py"] = {"what": "bench.py --gpus 1, the parent's tree and this tree alternated", "metric": key, "unit": runs["this"][0].get("unit"),
                           "parent": p, "this": t, "this_median": statistics.median(t), "parent_range": [min(p), max(p)],
                           "this_median_inside_parent_range": bool(min(p) <= statistics.median(t) <= max(p)),
                           "this_median_not_below_parent_range": bool(statistics.median(t) >= min(p))}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("merged into", args.out)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-only", action="store_true")
    ap.add_argument("--objdump-json")
    ap.add_argument("--bench-py-jsonl")
    ap.add_argument("--bench-py-key", default="value")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="0,1,2")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "semiplanar_mix.json"))
    args = ap.parse_args()
    if args.merge_only:
        return merge(args)
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.rounds >= 5, "the comparison is repeated at least five times"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    rng = np.random.default_rng(1)
    out = {"what": "semi-planar frames under the luma / chroma mix (32, 32, 0): paths alternated in one process on one MI355X, %d rounds, device-event "
                   "windows of %d launches after %d warm-up launches of every path, every plane an allocation of its own, content uniform in 0.3 .. 0.7 "
                   "of the range (tools/bench_semiplanar_mix.py)" % (args.rounds, args.window, args.warmup),
           "paths": {"a": "vfgs_hip_add_grain_sp_frame_list_dev under the mix", "b": "vfgs_hip_add_grain_frame_list_dev / _copy_dev under the mix on the planar twins",
                     "c": "de-interleave (and shift) into scratch planes with torch copies, path b's in-place call on them, interleave (and shift) into the destination",
                     "d": "vfgs_hip_add_grain_sp_frame_list_dev with the mix off"},
           "traffic_ratio_a_over_d_if_the_luma_read_is_shared": round(7 / 6, 4),
           "peak_bytes_per_s": PEAK, "device": hip.device_info(), "workloads": {}}
    failed = False
    with torch.cuda.stream(stream):
        for si in [int(x) for x in args.sizes.split(",")]:
            sname, w, h, nf = SIZES[si]
            for fname, trace, shift in FORMS:
                for in_place in (True, False):
                    lib.vfgs_hip_reset_state()
                    rec = T.load_trace(trace)
                    T.replay(hip, rec)
                    depth = T.trace_geometry(rec)[0]
                    pics = Pictures(w, h, depth, shift, nf, rng, in_place)
                    name = f"{sname} {fname} {'in place' if in_place else 'out of place'}"
                    set_mix(hip, True)
                    if not parity(hip, rec, pics, st):
                        out["workloads"][name] = {"parity": False, "note": "parity against the oracle failed: numbers withheld"}
                        failed = True
                        continue
                    paths = {"a": (pics.path_a, True), "b": (pics.path_b, True), "c": (pics.path_c, True), "d": (pics.sp_call, False)}
                    kernels, launches = {}, {}
                    for k, (p, mix) in paths.items():
                        set_mix(hip, mix)
                        n0 = (hip.last_launch_info() or {"launches": 0})["launches"]
                        for _ in range(args.warmup):
                            p(hip, st)
                        info = hip.last_launch_info()
                        kernels[k], launches[k] = info["kernel"], (info["launches"] - n0) // args.warmup
                    torch.cuda.synchronize()
                    us = {k: [] for k in paths}
                    for _ in range(args.rounds):
                        for k, (p, mix) in paths.items():
                            set_mix(hip, mix)
                            ms = C.c_float()
                            hip._ck(lib.vfgs_hip_timer_begin(st))
                            for _ in range(args.window):
                                p(hip, st)
                            hip._ck(lib.vfgs_hip_timer_end(st, C.byref(ms)))
                            us[k].append(ms.value * 1e3 / args.window / nf)
                    sz = 2 if depth > 8 else 1
                    alg = 2 * sz * (w * h + 2 * (w // 2) * (h // 2))
                    med = {k: statistics.median(v) for k, v in us.items()}
                    spread = 100 * (max(us["b"]) - min(us["b"])) / med["b"]
                    e = {"parity": True, "frames_per_launch": nf, "kernels": kernels, "launches_per_call": launches, "algorithmic_bytes_per_frame": alg,
                         "us_per_frame": {k: round(med[k], 3) for k in med},
                         "us_per_frame_rounds": {k: [round(x, 3) for x in v] for k, v in us.items()},
                         "b_spread_pct": round(spread, 2),
                         "fraction_of_peak": {k: round(alg / (med[k] * 1e-6) / PEAK, 4) for k in ("a", "b", "d")},
                         "a_over_b": round(med["a"] / med["b"], 4), "a_inside_b_spread": bool(abs(med["a"] / med["b"] - 1) * 100 <= spread),
                         "a_over_c": round(med["a"] / med["c"], 4), "a_over_d": round(med["a"] / med["d"], 4),
                         "a_faster_than_c": bool(max(us["a"]) < min(us["c"]))}
                    out["workloads"][name] = e
                    print(name, json.dumps(e["us_per_frame"]), "b spread %", e["b_spread_pct"], "a/b", e["a_over_b"], "a/c", e["a_over_c"], "a/d", e["a_over_d"], flush=True)
                    del pics
                    torch.cuda.empty_cache()
    out["condition_a_faster_than_c_everywhere"] = (not failed) and all(e.get("a_faster_than_c") for e in out["workloads"].values())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out, "condition:", out["condition_a_faster_than_c_everywhere"])
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
