#!/usr/bin/env python3
"""Developer tool: what a chroma mix per model buys, and what teaching the two mix kernel families to read it costs the programmed mix, on
one MI355X, in one command.  Writes one JSON document (default profiles/model_mix_list.json).

buys -- 1920x1080 10-bit 4:2:0 x 32 planar and 1920x1080 P010 x 32, in place, 32 DISTINCT AFGS1 parameter sets (the sixteen recorded
10-bit 4:2:0 ones of tests/golden/fwcfg, each with two mixes), every plane an allocation of its own, content uniform in 0.3 .. 0.7 of the
range; legs alternated, `--rounds` rounds, device-event windows of `--window` passes over the 32 pictures after a warm-up:
  new  vfgs_hip_models_from_afgs1_mix (32 models: one copy, one launch) + the list call with a model per picture + releasing the models,
       ALL inside the window: what a player pays per group of 32 pictures
  old  the only shape that worked before: vfgs_hip_afgs1_chroma_mix(1), then per picture vfgs_init_afgs1 and a one-frame list call
  Picture 0 of the two legs is compared byte for byte first (`same_picture`).

costs -- the PROGRAMMED mix (vfgs_hip_set_chroma_mix (32, 32, 0) on both components), whose kernels this change edits: the workloads of
profiles/chroma_mix.json (grain_mix_kernel, list calls of 8 frames) and of profiles/semiplanar_mix.json's path a (grain_sp_mix_kernel),
in place and out of place.  Needs --parent-lib, the parent commit's libvfgs_hip.so loaded beside this one (a state of its own, the same
buffers, the same stream): rounds alternate parent / this, at least five.  Per workload: the rounds, the medians, their ratio, the parent's
round-to-round spread and whether this build's median lies within it (`this_median_within_parent_spread`).

--merge-only --resources-json F adds the kernels' resource notes (`kernel_resources`) to the document without a GPU."""
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

MIX = (32, 32, 0)
AFGS1_10_420 = ["fgs_afgs1_test%s_10_420" % k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, "1_tbl")]
# the programmed-mix workloads: name, trace, width, height, frames per launch, semi-planar sample shift (None: planar)
COST = [("7680x4320 10-bit 4:2:0 fgs_afgs1_test1 planar x8", "fgs_afgs1_test1_10_420", 7680, 4320, 8, None),
        ("3840x2160 8-bit 4:4:4 fgs_afgs1_test1 planar x8", "fgs_afgs1_test1_8_444", 3840, 2160, 8, None)]
COST += [("%dx%d %s fgs_afgs1_test1 x%d" % (w, h, n, nf), t, w, h, nf, sh) for w, h, nf in ((1920, 1080, 32), (3840, 2160, 16), (7680, 4320, 8))
         for n, t, sh in (("NV12", "fgs_afgs1_test1_8_420", 0), ("P010", "fgs_afgs1_test1_10_420", 6))]


def merge(args):
    out = json.loads(Path(args.out).read_text())
    out["kernel_resources"] = json.loads(Path(args.resources_json).read_text())
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("merged into", args.out)
    return 0


class Build:
    """one build of the library: the setters a recorded program needs, the mix and the list calls of the programmed-mix legs"""

    def __init__(self, lib, hw):
        self.lib, self.hw = lib, hw
        vp, u, i = C.c_void_p, C.c_uint, C.c_int
        fp, spf, u32p = C.POINTER(hw.FramePtrs), C.POINTER(hw.SpFrame), C.POINTER(C.c_uint32)
        for n, a in (("vfgs_set_luma_pattern", [i, vp]), ("vfgs_set_chroma_pattern", [i, vp]), ("vfgs_set_scale_lut", [i, vp]), ("vfgs_set_pattern_lut", [i, vp]),
                     ("vfgs_set_seed", [u]), ("vfgs_set_scale_shift", [i]), ("vfgs_set_depth", [i]), ("vfgs_set_legal_range", [i]),
                     ("vfgs_set_chroma_subsampling", [i, i]), ("vfgs_hip_init", [i]), ("vfgs_hip_set_chroma_mix", [i, i, i, i]),
                     ("vfgs_hip_add_grain_frame_list_dev", [fp, u, u, u, u, u, vp]), ("vfgs_hip_add_grain_frame_list_copy_dev", [fp, fp, u, u, u, u, u, vp]),
                     ("vfgs_hip_add_grain_sp_frame_list_dev", [spf, spf, u32p, u, u, u, u, u, u, vp]), ("vfgs_hip_last_launch_info", [C.POINTER(hw.LaunchInfo)])):
            getattr(lib, n).argtypes = a
        lib.vfgs_hip_last_error_string.restype = C.c_char_p
        lib.vfgs_hip_reset_state.restype = None
        lib.vfgs_hip_clear_chroma_mix.restype = None
        assert lib.vfgs_hip_init(0) == 0
        b = hw._b
        self.set_luma_pattern = lambda k, P: lib.vfgs_set_luma_pattern(k, b(P))
        self.set_chroma_pattern = lambda k, P: lib.vfgs_set_chroma_pattern(k, b(P))
        self.set_scale_lut = lambda c, l: lib.vfgs_set_scale_lut(c, b(l))
        self.set_pattern_lut = lambda c, l: lib.vfgs_set_pattern_lut(c, b(l))
        self.set_seed = lambda s: lib.vfgs_set_seed(s & 0xFFFFFFFF)
        self.set_scale_shift, self.set_depth, self.set_legal_range = lib.vfgs_set_scale_shift, lib.vfgs_set_depth, lib.vfgs_set_legal_range
        self.set_chroma_subsampling = lib.vfgs_set_chroma_subsampling

    def program(self, T, rec):
        self.lib.vfgs_hip_reset_state()
        T.replay(self, rec)
        self.lib.vfgs_hip_clear_chroma_mix()
        for c in (1, 2):
            assert self.lib.vfgs_hip_set_chroma_mix(c, *MIX) == 0, self.lib.vfgs_hip_last_error_string()

    def kernel(self):
        li = self.hw.LaunchInfo()
        return li.kernel.decode() if self.lib.vfgs_hip_last_launch_info(C.byref(li)) == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-only", action="store_true")
    ap.add_argument("--resources-json")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libvfgs_hip.so of the parent commit, for the `costs` part (left out without it)")
    ap.add_argument("--skip-buys", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "model_mix_list.json"))
    args = ap.parse_args()
    if args.merge_only:
        return merge(args)
    import torch
    import vfgs_testlib as T
    from versatilefilmgrain_amd import fw, hw
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.rounds >= 5, "at least five rounds of each leg"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    rng = np.random.default_rng(1)
    out = {"what": "a chroma mix per model (tools/model_mix_list_bench.py): legs alternated in one command on one MI355X, %d rounds, device-event windows "
                   "of %d passes after %d warm-up passes, every plane an allocation of its own, content uniform in 0.3 .. 0.7 of the range"
                   % (args.rounds, args.window, args.warmup), "device": hip.device_info()}

    def planes(n, rows, cols, depth, shift):
        lo, hi = int(0.3 * (1 << depth)), int(0.7 * (1 << depth))
        a = (rng.integers(lo, hi, (rows, cols), dtype=np.uint32) << shift).astype(np.uint16 if depth > 8 else np.uint8)
        t = torch.from_numpy(a.view(np.int16) if depth > 8 else a).cuda()
        return [t.clone() for _ in range(n)]

    def timed(fn, n_warm, n_win, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(n_warm):
            fn()
        stream.synchronize()
        e0.record(stream)
        for _ in range(n_win):
            fn()
        e1.record(stream)
        e1.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / (n_win * per), 3)

    # ---- what it buys
    if not args.skip_buys:
        buys = {}
        w, h, nf, depth = 1920, 1080, 32, 10
        rec = T.load_trace(AFGS1_10_420[0])
        cfgs = []
        for i in range(nf):
            kind, raw = T.load_fwcfg(AFGS1_10_420[i % 16])[1][-1]
            assert kind == 1
            a = fw.struct_from_bytes(1, raw)
            if i >= 16:     # the second mix of a parameter set: distinct from every recorded one (128 / 192 / 256 and the .tbl's)
                a.cb_mult, a.cb_luma_mult, a.cb_offset = 128 + 2 * (i - 15), 192 - (i - 15), 256 - (i - 15)
                a.cr_mult, a.cr_luma_mult, a.cr_offset = 128 + (i - 15), 192 - 2 * (i - 15), 256 + (i - 15)
            cfgs.append(a)
        assert len({bytes(a) for a in cfgs}) == nf
        seeds = [fw.afgs1_seed(a) for a in cfgs]
        for name, shift in (("1920x1080 10-bit 4:2:0 planar x32", None), ("1920x1080 P010 x32", 6)):
            lib.vfgs_hip_reset_state()
            T.replay(hip, rec)
            if shift is None:
                Y, U, V = planes(nf, h, w, depth, 0), planes(nf, h // 2, w // 2, depth, 0), planes(nf, h // 2, w // 2, depth, 0)
                ptrs = [tuple(p.data_ptr() for p in f) for f in zip(Y, U, V)]
                flist, ones = hip.frame_list(ptrs), [hip.frame_list([p]) for p in ptrs]
                many = lambda ms: hip.add_grain_frame_list_models_dev(flist, None, ms, seeds, w, h, w, w // 2, st)
                one = lambda k: hip.add_grain_frame_list_dev(ones[k], w, h, w, w // 2, st)
                probe = (Y[0], U[0], V[0])
            else:
                Y, UV = planes(nf, h, w, depth, shift), planes(nf, h // 2, w, depth, shift)
                ptrs = [tuple(p.data_ptr() for p in f) for f in zip(Y, UV)]
                flist, ones = hip.sp_frame_list(ptrs), [hip.sp_frame_list([p]) for p in ptrs]
                many = lambda ms: hip.add_grain_sp_frame_list_models_dev(flist, None, ms, seeds, w, h, w, w, shift, st)
                one = lambda k: hip.add_grain_sp_frame_list_dev(ones[k], None, None, w, h, w, w, shift, st)
                probe = (Y[0], UV[0])
            info = {}

            def leg_new():
                fw.afgs1_chroma_mix(False)
                hip.clear_chroma_mix()
                ms = hip.models_from_afgs1_mix(cfgs, st)
                n0 = hip.last_launch_info()["launches"] if hip.last_launch_info() else 0
                many(ms)
                li = hip.last_launch_info()
                info["new"] = {"kernel": li["kernel"], "grain_launches_per_32_pictures": li["launches"] - n0}
                for m in ms:
                    hip.model_release(m)

            def leg_old():
                fw.afgs1_chroma_mix(True)
                for k in range(nf):
                    fw.init(cfgs[k])
                    one(k)
                info["old"] = {"kernel": hip.last_launch_info()["kernel"], "grain_launches_per_32_pictures": nf}

            # picture 0, from the same content, through both legs
            keep = [p.clone() for p in probe]
            leg_new()
            stream.synchronize()
            got_new = [p.clone() for p in probe]
            for p, k in zip(probe, keep):
                p.copy_(k)
            torch.cuda.synchronize()
            leg_old()
            stream.synchronize()
            same = all(bool(torch.equal(a, b)) for a, b in zip(got_new, probe)) and not all(bool(torch.equal(a, b)) for a, b in zip(keep, probe))
            us = {"new": [], "old": []}
            for _ in range(args.rounds):
                us["new"].append(timed(leg_new, args.warmup, args.window, nf))
                us["old"].append(timed(leg_old, max(1, args.warmup // 4), max(2, args.window // 4), nf))
            med = {k: statistics.median(v) for k, v in us.items()}
            buys[name] = {"same_picture": same, "distinct_parameter_sets": nf, "legs": info, "us_per_picture_rounds": us,
                          "us_per_picture": {k: round(v, 3) for k, v in med.items()}, "old_over_new": round(med["old"] / med["new"], 2),
                          "new_rounds_all_below_old_rounds": max(us["new"]) < min(us["old"])}
            print(name, json.dumps(buys[name]), flush=True)
            fw.afgs1_chroma_mix(False)
            hip.clear_chroma_mix()
            del Y, flist, ones, ptrs, probe, keep, got_new
            torch.cuda.empty_cache()
        out["buys"] = {"legs": {"new": "vfgs_hip_models_from_afgs1_mix + the list call with a model per picture + vfgs_hip_model_release, all inside the window",
                                "old": "vfgs_hip_afgs1_chroma_mix(1); per picture vfgs_init_afgs1 + a one-frame list call"}, "workloads": buys}

    # ---- what it must not cost
    if args.parent_lib:
        builds = {"parent": Build(C.CDLL(str(args.parent_lib)), hw), "this": Build(lib, hw)}
        cost = {}
        for name, trace, w, h, nf, shift in COST:
            rec = T.load_trace(trace)
            depth, sx, sy = T.trace_geometry(rec)
            for b in builds.values():
                b.program(T, rec)
            for in_place in (True, False):
                if shift is None:
                    Y, U, V = planes(nf, h, w, depth, 0), planes(nf, h // sy, w // sx, depth, 0), planes(nf, h // sy, w // sx, depth, 0)
                    src = hw.VfgsHip.frame_list([tuple(p.data_ptr() for p in f) for f in zip(Y, U, V)])
                    dd = None if in_place else [[torch.empty_like(t) for t in p] for p in (Y, U, V)]
                    dst = None if in_place else hw.VfgsHip.frame_list([tuple(p.data_ptr() for p in f) for f in zip(*dd)])
                    if in_place:
                        call = lambda L: L.vfgs_hip_add_grain_frame_list_dev(src, nf, w, h, w, w // sx, st)
                    else:
                        call = lambda L: L.vfgs_hip_add_grain_frame_list_copy_dev(src, dst, nf, w, h, w, w // sx, st)
                else:
                    Y, UV = planes(nf, h, w, depth, shift), planes(nf, h // sy, w, depth, shift)
                    src = hw.VfgsHip.sp_frame_list([tuple(p.data_ptr() for p in f) for f in zip(Y, UV)])
                    dd = None if in_place else [[torch.empty_like(t) for t in p] for p in (Y, UV)]
                    dst = src if in_place else hw.VfgsHip.sp_frame_list([tuple(p.data_ptr() for p in f) for f in zip(*dd)])
                    call = lambda L: L.vfgs_hip_add_grain_sp_frame_list_dev(src, dst, None, nf, w, h, w, w, shift, st)
                us, kernels = {k: [] for k in builds}, {}
                for _ in range(args.rounds):
                    for k, b in builds.items():
                        def fn(b=b):
                            assert call(b.lib) == 0, b.lib.vfgs_hip_last_error_string()
                        us[k].append(timed(fn, args.warmup, args.window, nf))
                        kernels[k] = b.kernel()
                med = {k: statistics.median(v) for k, v in us.items()}
                p = us["parent"]
                e = {"kernel": kernels, "frames_per_launch": nf, "us_per_frame_rounds": us, "us_per_frame": {k: round(v, 3) for k, v in med.items()},
                     "this_over_parent": round(med["this"] / med["parent"], 4), "parent_min_max": [min(p), max(p)],
                     "parent_spread_pct": round(100 * (max(p) - min(p)) / med["parent"], 2),
                     "this_median_within_parent_spread": bool(min(p) <= med["this"] <= max(p)), "this_median_not_above_parent_max": bool(med["this"] <= max(p))}
                cost[name + (" in place" if in_place else " out of place")] = e
                print(name, "in place" if in_place else "out of place", json.dumps(e), flush=True)
                del Y, src, dst, dd
                torch.cuda.empty_cache()
        for b in builds.values():
            b.lib.vfgs_hip_clear_chroma_mix()
            b.lib.vfgs_hip_reset_state()
        out["costs"] = {"what": "the programmed mix %s on both components, the parent commit's library and this one alternated on the same buffers" % (MIX,),
                        "workloads": cost, "every_median_within_parent_spread": all(e["this_median_within_parent_spread"] for e in cost.values()),
                        "no_median_above_parent_max": all(e["this_median_not_above_parent_max"] for e in cost.values())}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
