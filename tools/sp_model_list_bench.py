#!/usr/bin/env python3
"""Developer tool: what a model per picture costs a launch over semi-planar surfaces, and what it saves, on one MI355X, in one command.

Legs, alternated, `--rounds` rounds, HIP-event windows of `--window` launches after a warm-up, in place, every plane an allocation of
its own, one seed sequence:
  a  vfgs_hip_add_grain_sp_frame_list_dev, one programmed model -- from the library given with --parent-lib (the parent commit's build,
     loaded beside this one: the yardstick whose code no change here touches); without the option, this library's
  b  vfgs_hip_add_grain_sp_frame_list_models_dev with that same model on every frame: the price of the mechanism
  c  the models call with two models of one form alternating (the second: the first with halved scale LUTs and the other range)
  e  leg a's call through THIS library (with --parent-lib: what separates the two builds from the two entry points)
  d  the alternative to c without models: vfgs_init_sei / vfgs_init_afgs1 + vfgs_hip_add_grain_sp_frame_list_dev on ONE surface per
     launch, two recorded configurations (tests/golden/fwcfg) alternating -- pattern generation on the device, a table build and an
     upload per picture
Prints one JSON document (profiles/sp_model_list.json holds three: the legs in three orders)."""
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
import vfgs_testlib as T  # noqa: E402
from versatilefilmgrain_amd import fw, hw  # noqa: E402

SHAPES = [  # name, width, height, configuration of legs a-c (and d), second configuration of leg d, frames per launch
    ("1920x1080 P010 fgs_sei x32", 1920, 1080, "fgs_sei_10_420", "fgs_afgs1_test1_10_420", 32),
    ("3840x2160 P010 fgs_afgs1_test1 x16", 3840, 2160, "fgs_afgs1_test1_10_420", "fgs_sei_10_420", 16),
    ("7680x4320 P010 fgs_sei x8", 7680, 4320, "fgs_sei_10_420", "fgs_afgs1_test1_10_420", 8),
    ("3840x2160 NV12 fgs_afgs1_test1 x8", 3840, 2160, "fgs_afgs1_test1_8_420", "fgs_sei_8_420", 8),
]


class ParentLib:
    """the few entry points leg a needs, from another build of the library loaded beside this one (a state of its own)"""

    def __init__(self, path):
        self.lib = C.CDLL(str(path))
        vp, u, i = C.c_void_p, C.c_uint, C.c_int
        for n, a in (("vfgs_set_luma_pattern", [i, vp]), ("vfgs_set_chroma_pattern", [i, vp]), ("vfgs_set_scale_lut", [i, vp]), ("vfgs_set_pattern_lut", [i, vp]),
                     ("vfgs_set_seed", [u]), ("vfgs_set_scale_shift", [i]), ("vfgs_set_depth", [i]), ("vfgs_set_legal_range", [i]),
                     ("vfgs_set_chroma_subsampling", [i, i]), ("vfgs_hip_init", [i]),
                     ("vfgs_hip_add_grain_sp_frame_list_dev", [C.POINTER(hw.SpFrame), C.POINTER(hw.SpFrame), C.POINTER(C.c_uint32), u, u, u, u, u, u, vp]), ("vfgs_hip_last_launch_info", [C.POINTER(hw.LaunchInfo)])):
            getattr(self.lib, n).argtypes = a
        self.lib.vfgs_hip_last_error_string.restype = C.c_char_p
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pool-mb", type=int, default=1600, help="bytes of frames cycled through per shape (beyond the last-level cache)")
    ap.add_argument("--shapes", default="0,1,2,3")
    ap.add_argument("--order", default="abced", help="the legs of a round, in this order (a permutation of abced, or of some of them: a profiler run without leg d)")
    ap.add_argument("--parent-lib", default=None, help="libvfgs_hip.so of the parent commit, for leg a")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert set(args.order) <= set("abced") and len(set(args.order)) == len(args.order), "--order: legs of abced, each once"
    hip = hw.VfgsHip(device=0)
    lib = hip.lib
    parent = ParentLib(args.parent_lib) if args.parent_lib else None
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    out = {"what": "semi-planar surfaces with a model per picture: legs alternated in one command on one MI355X, %d rounds, HIP-event windows of %d launches after "
                   "%d warm-up launches, in place, every plane an allocation of its own, uniform random content, one seed sequence "
                   "(tools/sp_model_list_bench.py), legs in the order %s" % (args.rounds, args.window, args.warmup, args.order),
           "legs": {"a": "vfgs_hip_add_grain_sp_frame_list_dev, one model, " + ("the parent commit's library" if parent else "THIS library (no --parent-lib)"),
                    "b": "vfgs_hip_add_grain_sp_frame_list_models_dev, that model on every frame",
                    "c": "vfgs_hip_add_grain_sp_frame_list_models_dev, two models of one form alternating",
                    "e": "vfgs_hip_add_grain_sp_frame_list_dev, one model, this library",
                    "d": "vfgs_init_sei / vfgs_init_afgs1 + vfgs_hip_add_grain_sp_frame_list_dev on one surface per launch, two configurations alternating"},
           "device": hip.device_info(), "shapes": {}}
    rng = np.random.default_rng(1)
    for si in [int(x) for x in args.shapes.split(",")]:
        name, w, h, cfg_a, cfg_b, nf = SHAPES[si]
        rec = T.load_trace(cfg_a)
        depth, sx, sy = T.trace_geometry(rec)
        lib.vfgs_hip_reset_state()
        T.replay(hip, rec)
        m_a = hip.model_capture(sp)
        for c in range(3):
            hip.set_scale_lut(c, bytes(v >> 1 for v in hip.luts(c)[0]))
        hip.set_legal_range(0 if hip.params()["ymin"] else 1)
        m_b = hip.model_capture(sp)
        ia, ib = hip.model_info(m_a), hip.model_info(m_b)
        assert (ia["one_y"], ia["one_c"]) == (ib["one_y"], ib["one_c"]), (ia, ib)
        lib.vfgs_hip_reset_state()
        T.replay(hip, rec)
        if parent:
            T.replay(parent, rec)
        structs = []
        for n in (cfg_a, cfg_b):
            assert T.trace_geometry(T.load_trace(n)) == (depth, sx, sy)
            kind, raw = T.load_fwcfg(n)[1][-1]
            structs.append(fw.struct_from_bytes(kind, raw))
        assert sx == 2
        sz = 2 if depth > 8 else 1
        shift = 16 - depth if depth > 8 else 0          # P010: the samples sit in the high bits
        frame_bytes = (w * h + w * (h // sy)) * sz
        nsets = max(2, -(-args.pool_mb * (1 << 20) // (frame_bytes * nf)))
        keep, sets, singles = [], [], []
        dt, top = (torch.int16, 1 << 10) if depth > 8 else (torch.uint8, 256)
        for _ in range(nsets):
            ptrs = []
            for _ in range(nf):
                planes = [torch.randint(0, top, (rows, w), dtype=dt, device="cuda") << shift for rows in (h, h // sy)]      # Y, and UV: as many containers a row
                keep.append(planes)
                ptrs.append(tuple(p.data_ptr() for p in planes))
            ptrs = [ptrs[i] for i in rng.permutation(nf)]          # list order is not address order
            sets.append(hip.sp_frame_list(ptrs))
            singles.append(ptrs)
        torch.cuda.synchronize()
        ncalls = args.warmup + args.window
        ones = [[hip.sp_frame_list([p]) for p in ptrs] for ptrs in singles]
        same = (C.c_void_p * nf)(*([m_a] * nf))
        alt = (C.c_void_p * nf)(*[m_b if i & 1 else m_a for i in range(nf)])
        la = parent.lib if parent else lib

        def leg_a(k):
            return la.vfgs_hip_add_grain_sp_frame_list_dev(sets[k % nsets], sets[k % nsets], None, nf, w, h, w, w, shift, sp)

        def leg_b(k):
            return lib.vfgs_hip_add_grain_sp_frame_list_models_dev(sets[k % nsets], sets[k % nsets], same, None, nf, w, h, w, w, shift, sp)

        def leg_c(k):
            return lib.vfgs_hip_add_grain_sp_frame_list_models_dev(sets[k % nsets], sets[k % nsets], alt, None, nf, w, h, w, w, shift, sp)

        def leg_e(k):
            return lib.vfgs_hip_add_grain_sp_frame_list_dev(sets[k % nsets], sets[k % nsets], None, nf, w, h, w, w, shift, sp)

        def leg_d(k):
            rc = 0
            for i, one in enumerate(ones[k % nsets]):
                fw.init(structs[i & 1])
                rc |= lib.vfgs_hip_add_grain_sp_frame_list_dev(one, one, None, 1, w, h, w, w, shift, sp)
            return rc

        def window(leg, n_warm, n_win):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for k in range(n_warm):
                assert leg(k) == 0, (la if leg is leg_a else lib).vfgs_hip_last_error_string()
            stream.synchronize()
            e0.record(stream)
            for k in range(n_warm, n_warm + n_win):
                assert leg(k) == 0, (la if leg is leg_a else lib).vfgs_hip_last_error_string()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / (n_win * nf)

        us = {k: [] for k in args.order}
        kernels = {}
        for _ in range(args.rounds):
            for key, leg in [(k, {"a": leg_a, "b": leg_b, "c": leg_c, "e": leg_e, "d": leg_d}[k]) for k in args.order]:
                # (leg d is a launch per FRAME: a window of as many launches as the others, not of nf times as many)
                nw, nn = (args.warmup, args.window) if key != "d" else (max(1, args.warmup // nf), max(2, args.window // nf))
                us[key].append(round(window(leg, nw, nn), 3))
                kernels[key] = parent.kernel() if (key == "a" and parent) else hip.last_launch_info()["kernel"]
            # leg d leaves this library programmed with a firmware configuration: back to the trace's state for legs that read it
            lib.vfgs_hip_reset_state()
            T.replay(hip, rec)
        med = {k: statistics.median(v) for k, v in us.items()}
        rngs = {k: [min(v), max(v)] for k, v in us.items()}
        traffic = frame_bytes * 2      # every sample read once and written once
        r = {"us_per_frame": us, "kernel": kernels, "median": {k: round(v, 3) for k, v in med.items()}, "min_max": rngs,
             "fraction_of_8TBs_peak_at_median": {k: round(traffic / (med[k] * 1e-6) / 8e12, 3) for k in med},
             "model_device_bytes": ia["device_bytes"], "model_form": [ia["one_y"], ia["one_c"]], "frame_sets_cycled": nsets}
        for x, y in ("ba", "be", "ea", "cb", "dc"):
            if x in med and y in med:
                r[f"{x}_over_{y}_ratio_of_medians"] = round(med[x] / med[y], 4)
        if "c" in med and "d" in med:
            r["c_spread_entirely_below_d_spread"] = rngs["c"][1] < rngs["d"][0]
        out["shapes"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        hip.model_release(m_a)
        hip.model_release(m_b)
        del keep, sets, singles, ones
        torch.cuda.empty_cache()
    lib.vfgs_hip_reset_state()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
