#!/usr/bin/env python3
"""Developer tool: what a model per picture from planar pictures onto semi-planar surfaces buys, and what teaching the to-surface kernels to
read a model per frame costs the programmed _to_sp / _to_sp8 callers, on one MI355X, in one command.  Writes one JSON document (default
profiles/models_to_sp.json).

buys -- 1920x1080 10-bit 4:2:0 x 32, planar -> P010 and planar -> NV12, 32 distinct AFGS1 parameter sets (the sixteen recorded 10-bit 4:2:0
ones of tests/golden/fwcfg, each once as recorded and once with another seed and a changed luma scaling function), each with its seed,
every plane an allocation of its own, content uniform in 0.3 .. 0.7 of the range; legs alternated, `--rounds` rounds, device-event windows
of `--window` passes over the 32 pictures after a warm-up:
  new  vfgs_hip_models_from_afgs1 (32 models) + the _models_to_sp / _models_to_sp8 call + releasing the models, ALL inside the window
  old  the only shape that worked before: per picture vfgs_init_afgs1 + vfgs_set_seed and a one-picture _to_sp / _to_sp8 call -- on the
       PARENT commit's library where --parent-lib names it (a state of its own, the same buffers, the same stream), else on this one
  Picture 0 of the two legs is compared byte for byte first (`same_picture`).

costs -- the PROGRAMMED _to_sp / _to_sp8 calls, whose kernels this change edits, on the workloads of profiles/planar_to_semiplanar.json
(fgs_sei: 10 bit to P010 and to NV12 at 1080p x 32, 2160p x 16, 4320p x 8; 8 bit to NV12 at 2160p x 16).  Needs --parent-lib: rounds
alternate parent / this, at least five.  Per workload: the rounds, the medians, their ratio, the parent's own min .. max and whether this
build's median lies within it.

same_model -- the new calls with ONE model on all 32 frames against the programmed call of the same model, this build, alternated: what
the run-time decision and the scalar loads of the record cost a launch."""
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

AFGS1_10_420 = ["fgs_afgs1_test%s_10_420" % k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, "1_tbl")]
SIZES = [(1920, 1080, 32), (3840, 2160, 16), (7680, 4320, 8)]
# the programmed workloads: name, trace, depth, width, height, frames per launch, narrowed, sample shift
COST = [("%dx%d x%d 10-bit 4:2:0 fgs_sei to P010" % (w, h, nf), "fgs_sei_10_420", 10, w, h, nf, False, 6) for w, h, nf in SIZES]
COST += [("%dx%d x%d 10-bit 4:2:0 fgs_sei to NV12 (narrowed)" % (w, h, nf), "fgs_sei_10_420", 10, w, h, nf, True, 0) for w, h, nf in SIZES]
COST += [("3840x2160 x16 8-bit 4:2:0 fgs_sei to NV12", "fgs_sei_8_420", 8, 3840, 2160, 16, False, 0)]


class Build:
    """one build of the library: the setters a recorded program needs, vfgs_init_afgs1 and the programmed to-surface calls"""

    def __init__(self, lib, hw, fw):
        self.lib, self.hw = lib, hw
        vp, u, i = C.c_void_p, C.c_uint, C.c_int
        fp, spf, u32p = C.POINTER(hw.FramePtrs), C.POINTER(hw.SpFrame), C.POINTER(C.c_uint32)
        for n, a in (("vfgs_set_luma_pattern", [i, vp]), ("vfgs_set_chroma_pattern", [i, vp]), ("vfgs_set_scale_lut", [i, vp]), ("vfgs_set_pattern_lut", [i, vp]),
                     ("vfgs_set_seed", [u]), ("vfgs_set_scale_shift", [i]), ("vfgs_set_depth", [i]), ("vfgs_set_legal_range", [i]),
                     ("vfgs_set_chroma_subsampling", [i, i]), ("vfgs_hip_init", [i]), ("vfgs_init_afgs1", [C.POINTER(fw.FgsAfgs1)]),
                     ("vfgs_hip_add_grain_frame_list_to_sp_dev", [fp, spf, u32p, u, u, u, u, u, u, u, u, vp]),
                     ("vfgs_hip_add_grain_frame_list_to_sp8_dev", [fp, spf, u32p, u, u, u, u, u, u, u, vp]),
                     ("vfgs_hip_last_launch_info", [C.POINTER(hw.LaunchInfo)])):
            getattr(lib, n).argtypes = a
        lib.vfgs_init_afgs1.restype = None
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

    def program(self, T, rec):
        self.lib.vfgs_hip_reset_state()
        T.replay(self, rec)

    def kernel(self):
        li = self.hw.LaunchInfo()
        return li.kernel.decode() if self.lib.vfgs_hip_last_launch_info(C.byref(li)) == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libvfgs_hip.so of the parent commit: the baseline of `buys` and the `costs` part (left out without it)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "models_to_sp.json"))
    args = ap.parse_args()
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
    this = Build(lib, hw, fw)
    parent = Build(C.CDLL(str(args.parent_lib)), hw, fw) if args.parent_lib else None
    base = parent or this
    out = {"what": "a model per picture from planar pictures onto semi-planar surfaces (tools/models_to_sp_bench.py): legs alternated in one command on one "
                   "MI355X, %d rounds, device-event windows of %d passes after %d warm-up passes, every plane an allocation of its own, content uniform in "
                   "0.3 .. 0.7 of the range" % (args.rounds, args.window, args.warmup), "device": hip.device_info(),
           "baseline_library": "the parent commit's" if parent else "this build's"}

    def planes(n, rows, cols, depth):
        lo, hi = int(0.3 * (1 << depth)), int(0.7 * (1 << depth))
        a = rng.integers(lo, hi, (rows, cols), dtype=np.uint32).astype(np.uint16 if depth > 8 else np.uint8)
        t = torch.from_numpy(a.view(np.int16) if depth > 8 else a).cuda()
        return [t.clone() for _ in range(n)]

    def fill(n, rows, cols, wide):
        return [torch.full((rows, cols), 0x5a5a if wide else 0x5a, dtype=torch.int16 if wide else torch.uint8, device="cuda") for _ in range(n)]

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

    class Pictures:
        """nf planar pictures of w x h at 4:2:0 and their surfaces: the depth's container (shifted up by `shift`) or, narrowed, bytes; pitches = the rows"""

        def __init__(self, w, h, nf, depth, out8, shift):
            self.w, self.h, self.nf, self.out8, self.shift = w, h, nf, out8, shift
            self.src = [planes(nf, h, w, depth), planes(nf, h // 2, w // 2, depth), planes(nf, h // 2, w // 2, depth)]
            wide = depth > 8 and not out8
            self.dst = [fill(nf, h, w, wide), fill(nf, h // 2, w, wide)]
            sp, dp = [tuple(p.data_ptr() for p in f) for f in zip(*self.src)], [tuple(p.data_ptr() for p in f) for f in zip(*self.dst)]
            self.s, self.d = hw.VfgsHip.frame_list(sp), hw.VfgsHip.sp_frame_list(dp)
            self.s1, self.d1 = [hw.VfgsHip.frame_list([p]) for p in sp], [hw.VfgsHip.sp_frame_list([p]) for p in dp]
            self.probe = [p[0] for p in self.dst]
            self.blank = 0x5a5a if wide else 0x5a

        def programmed(self, L, s=None, d=None, n=None):
            s, d, n = s or self.s, d or self.d, n or self.nf
            w, h = self.w, self.h
            if self.out8:
                return L.vfgs_hip_add_grain_frame_list_to_sp8_dev(s, d, None, n, w, h, w, w // 2, w, w, st)
            return L.vfgs_hip_add_grain_frame_list_to_sp_dev(s, d, None, n, w, h, w, w // 2, w, w, self.shift, st)

        def with_models(self, ms, seeds):
            w, h = self.w, self.h
            if self.out8:
                hip.add_grain_frame_list_models_to_sp8_dev(self.s, self.d, ms, seeds, w, h, w, w // 2, w, w, st)
            else:
                hip.add_grain_frame_list_models_to_sp_dev(self.s, self.d, ms, seeds, w, h, w, w // 2, w, w, self.shift, st)

    # ---- what it buys
    w, h, nf = 1920, 1080, 32
    afgs1 = []
    for i in range(nf):
        kind, raw = T.load_fwcfg(AFGS1_10_420[i % 16])[1][-1]
        assert kind == 1
        a = fw.struct_from_bytes(1, raw)
        if i >= 16:     # the second model of a parameter set: another seed, another luma scaling function
            a.grain_seed = (a.grain_seed + 257 * (i - 15)) & 0xffff
            for k in range(a.num_y_points):
                a.point_y_scaling[k] = max(1, a.point_y_scaling[k] - 1 - (i & 3))
        afgs1.append(a)
    assert len({bytes(a) for a in afgs1}) == nf
    seeds = [fw.afgs1_seed(a) for a in afgs1]
    buys = {}
    for name, out8, shift in (("1920x1080 10-bit 4:2:0 planar -> P010 x32", False, 6), ("1920x1080 10-bit 4:2:0 planar -> NV12 x32", True, 0)):
        for b in {id(base): base, id(this): this}.values():
            b.program(T, T.load_trace("fgs_afgs1_test1_10_420"))      # depth, format, range
        pic = Pictures(w, h, nf, 10, out8, shift)
        info = {}

        def leg_new():
            ms = hip.models_from_afgs1(afgs1, st)
            n0 = hip.last_launch_info()["launches"] if hip.last_launch_info() else 0
            pic.with_models(ms, seeds)
            li = hip.last_launch_info()
            info["new"] = {"kernel": li["kernel"], "grain_launches_per_32_pictures": li["launches"] - n0}
            for m in ms:
                hip.model_release(m)

        def leg_old():
            for k in range(nf):
                base.lib.vfgs_init_afgs1(C.byref(afgs1[k]))
                base.set_seed(seeds[k])
                assert pic.programmed(base.lib, pic.s1[k], pic.d1[k], 1) == 0, base.lib.vfgs_hip_last_error_string()
            info["old"] = {"kernel": base.kernel(), "grain_launches_per_32_pictures": nf}

        leg_new()
        stream.synchronize()
        got_new = [p.clone() for p in pic.probe]
        for p in pic.probe:
            p.fill_(pic.blank)
        torch.cuda.synchronize()
        leg_old()
        stream.synchronize()
        same = all(bool(torch.equal(a, b)) for a, b in zip(got_new, pic.probe)) and bool((pic.probe[0] != pic.blank).any())
        us = {"new": [], "old": []}
        for _ in range(args.rounds):
            us["new"].append(timed(leg_new, args.warmup, args.window, nf))
            us["old"].append(timed(leg_old, args.warmup, args.window, nf))
        med = {k: statistics.median(v) for k, v in us.items()}
        e = {"same_picture": same, "models_from": "vfgs_hip_models_from_afgs1", "distinct_parameter_sets": len({bytes(c) for c in afgs1}), "legs": info,
             "us_per_picture_rounds": us, "us_per_picture": {k: round(v, 3) for k, v in med.items()},
             "us_per_picture_min_max": {k: [min(v), max(v)] for k, v in us.items()}, "old_over_new": round(med["old"] / med["new"], 2),
             "old_spread_pct": round(100 * (max(us["old"]) - min(us["old"])) / med["old"], 2),
             "new_rounds_all_below_old_rounds": max(us["new"]) < min(us["old"])}
        buys[name] = e
        print(name, json.dumps(e), flush=True)
        del pic, got_new
        torch.cuda.empty_cache()
    out["buys"] = {"legs": {"new": "vfgs_hip_models_from_afgs1 + the _models_to_sp / _models_to_sp8 call + vfgs_hip_model_release, all inside the window",
                            "old": "per picture vfgs_init_afgs1 + vfgs_set_seed + a one-picture _to_sp / _to_sp8 call, on the baseline library"},
                   "workloads": buys}

    # ---- the same model on every frame
    same_model = {}
    for name, out8, shift in (("1920x1080 10-bit 4:2:0 planar -> P010 x32", False, 6), ("1920x1080 10-bit 4:2:0 planar -> NV12 x32", True, 0)):
        for trace in ("fgs_sei_10_420", "fgs_afgs1_test1_10_420"):
            this.program(T, T.load_trace(trace))
            m = hip.model_capture(st)
            pic = Pictures(w, h, nf, 10, out8, shift)
            ms = (C.c_void_p * nf)(*([m] * nf))

            def leg_models():
                pic.with_models(ms, None)

            def leg_programmed():
                assert pic.programmed(lib) == 0, lib.vfgs_hip_last_error_string()

            us = {"models": [], "programmed": []}
            for _ in range(args.rounds):
                us["models"].append(timed(leg_models, args.warmup, args.window, nf))
                us["programmed"].append(timed(leg_programmed, args.warmup, args.window, nf))
            med = {k: statistics.median(v) for k, v in us.items()}
            e = {"kernel": this.kernel(), "us_per_frame_rounds": us, "us_per_frame": {k: round(v, 3) for k, v in med.items()},
                 "models_over_programmed": round(med["models"] / med["programmed"], 4)}
            same_model["%s, %s" % (name, trace)] = e
            print("same model:", name, trace, json.dumps(e), flush=True)
            hip.model_release(m)
            del pic
            torch.cuda.empty_cache()
    out["same_model"] = {"what": "one captured model on all 32 frames through the new call against the programmed call of the same model, this build", "workloads": same_model}

    # ---- what it must not cost
    if parent:
        builds = {"parent": parent, "this": this}
        cost = {}
        for name, trace, depth, cw, ch, cn, out8, shift in COST:
            rec = T.load_trace(trace)
            for b in builds.values():
                b.program(T, rec)
            pic = Pictures(cw, ch, cn, depth, out8, shift)
            us, kernels = {k: [] for k in builds}, {}
            for _ in range(args.rounds):
                for k, b in builds.items():
                    def fn(b=b):
                        assert pic.programmed(b.lib) == 0, b.lib.vfgs_hip_last_error_string()
                    us[k].append(timed(fn, args.warmup, args.window, cn))
                    kernels[k] = b.kernel()
            med = {k: statistics.median(v) for k, v in us.items()}
            p = us["parent"]
            e = {"kernel": kernels, "frames_per_launch": cn, "us_per_frame_rounds": us, "us_per_frame": {k: round(v, 3) for k, v in med.items()},
                 "this_over_parent": round(med["this"] / med["parent"], 4), "parent_min_max": [min(p), max(p)],
                 "parent_spread_pct": round(100 * (max(p) - min(p)) / med["parent"], 2),
                 "this_median_within_parent_spread": bool(min(p) <= med["this"] <= max(p)), "this_median_not_above_parent_max": bool(med["this"] <= max(p))}
            cost[name] = e
            print(name, json.dumps(e), flush=True)
            del pic
            torch.cuda.empty_cache()
        out["costs"] = {"what": "the programmed _to_sp / _to_sp8 calls, the parent commit's library and this one alternated on the same buffers",
                        "workloads": cost, "every_median_within_parent_spread": all(e["this_median_within_parent_spread"] for e in cost.values()),
                        "no_median_above_parent_max": all(e["this_median_not_above_parent_max"] for e in cost.values())}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
