"""Generators of the firmware's parameter space (TEST INFRASTRUCTURE): FGC SEI messages, AFGS1 parameter sets and pattern jobs, seeded with
numpy.random.default_rng, and what each covers, read from the structure alone (facts) -- so the coverage the GPU tests rely on is checked
without a GPU (tests/test_fw_space_cpu.py).  No GPU and no library: only the ctypes structures of versatilefilmgrain_amd.fw.

Every generated set is one the reference firmware accepts (AFGS1 points strictly increasing, lag 1..3, at most 256 intervals).  With
gpu=True (the default) it is also inside what vfgs_init_sei / vfgs_init_afgs1 and the two model builders admit: the stored scale shift
2..7.  gpu=False widens the auto-regressive log2_scale_factor to 2..9, for the recording reference and the host-records program only.

SEI messages: case = index % 25 -- the 20 constructions of tests/sei_model_util.py, then five wide ones:
  20 ar_wide            auto-regressive values over the 10-bit range: v1, v3, v5 -512..511, v4 0..1023 (the int16 storage of the taps wraps)
  21 upper_below_lower  intervals whose upper bound is below the lower one: they fill no table entry but still join the pattern list
  22 zero_intervals     a component present with an interval count of 0 (luma, Cb, Cr in turn: with luma the call makes no luma pattern)
  23 repeated_tails     Cb and Cr repeat luma's parameter sets (values 1..5): equal tails across components
  24 unused_entry       a chroma interval whose values 1..5 are the FIRST five numbers of luma's first interval: the reference's search
                        matches the first unused list entry, the interval joins nothing and its table entries name a slot nothing wrote
AFGS1 sets: case = index % 10 -- eight forced constructions on top of generated_set's draw, then two free ones (see forced_afgs1)."""
import numpy as np

import sei_model_util as G

SEI_CASES = 25
AFGS1_CASES = 10
FORMATS = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "440": (1, 2)}
GEOMETRIES = [(d, *FORMATS[f]) for d in (8, 10, 12) for f in sorted(FORMATS)]


def _fw():
    from versatilefilmgrain_amd import fw
    return fw


# ------------------------------------------------------------------------------------------------------------------------ SEI messages

def _wide_values(rng, s):
    return [int(rng.integers(0, 250)), int(rng.integers(-512, 512)), 0, int(rng.integers(-512, 512)), int(rng.integers(0, 1024)),
            int(rng.integers(-512, 512))]


def space_sei(FgsSei, rng, index, gpu=True):
    """message `index` of a list over the space"""
    case = index % SEI_CASES
    if case < G.CASES:
        return G.generated_sei(FgsSei, rng, case)
    s = FgsSei()
    ar = case == 20 or bool(rng.integers(0, 2))
    s.model_id = 1 if ar else 0
    s.log2_scale_factor = (int(rng.integers(3, 9)) if gpu else int(rng.integers(2, 10))) if ar else int(rng.integers(2, 8))
    if case == 20:
        for c in range(3):
            sets = [_wide_values(rng, s) for _ in range(int(rng.integers(1, 7)))]
            if c == 0:
                sets[0][1:] = [511, 0, -512, 1023, -512]          # the ends of the range, whatever was drawn
            G._put(s, c, G._tiled(rng, sets))
    elif case == 21:
        for c in range(3):
            sets = G._distinct(rng, s, ar, 4)
            a = int(rng.integers(40, 100))
            G._put(s, c, [(0, a, sets[0]), (a + 60, a + 10, sets[1]), (a + 61, 255, sets[2]), (255, 0, sets[3])])
    elif case == 22:
        for c in range(3):
            G._put(s, c, G._tiled(rng, G._distinct(rng, s, ar, 3)))
        s.num_intensity_intervals[(index // SEI_CASES) % 3] = 0
    elif case == 23:
        luma = G._distinct(rng, s, ar, 4)
        G._put(s, 0, G._tiled(rng, luma))
        G._put(s, 1, G._tiled(rng, [[int(rng.integers(0, 250))] + v[1:] for v in luma[:3]]))
        G._put(s, 2, G._tiled(rng, [[int(rng.integers(0, 250))] + v[1:] for v in luma[::-1]]))
    else:
        luma = G._distinct(rng, s, ar, 3)
        G._put(s, 0, G._tiled(rng, luma))
        first = G._read(s, 0, 0)
        for c in (1, 2):
            sets = G._distinct(rng, s, ar, 3)
            sets[c] = [int(rng.integers(0, 250))] + first[:5]
            G._put(s, c, G._tiled(rng, sets))
    return s


def sei_facts(s):
    """sei_model_util.facts and the wide constructions' words"""
    out = G.facts(s)
    first = tuple(G._read(s, 0, 0)[:5])
    tails = {}
    for c in range(3):
        if not s.comp_model_present_flag[c]:
            continue
        n = s.num_intensity_intervals[c]
        if n == 0:
            out.add("zero_intervals")
        vals = [G._read(s, c, k) for k in range(n)]
        tails[c] = {tuple(v[1:]) for v in vals}
        if any(s.intensity_interval_upper_bound[c][k] < s.intensity_interval_lower_bound[c][k] for k in range(n)):
            out.add("upper_below_lower")
        if s.model_id and any(abs(v[j]) > 256 for v in vals for j in (1, 3, 5)) and any(v[4] > 511 for v in vals):
            out.add("ar_wide")
        if c and first in tails[c]:
            out.add("unused_entry")
    if len(tails) == 3 and tails[0] & tails[1] and tails[0] & tails[2]:
        out.add("repeated_tails")
    if no_luma_pattern(s):
        out.add("no_luma_pattern")
    return out


def no_luma_pattern(cfg):
    """the call makes no luma pattern: the reference then hands over chroma payloads whose bytes 1024.. are uninitialised"""
    return not hasattr(cfg, "grain_seed") and (not cfg.comp_model_present_flag[0] or cfg.num_intensity_intervals[0] == 0)


WIDE = {"ar_wide", "upper_below_lower", "zero_intervals", "repeated_tails", "unused_entry"}
SEI_REQUIRED = G.REQUIRED | WIDE | {"no_luma_pattern"}


def sei_list(seed, n, gpu=True, first=0):
    """messages first .. first + n - 1 of the list with this seed"""
    FgsSei = _fw().FgsSei
    rng = np.random.default_rng(seed)
    return [space_sei(FgsSei, rng, first + i, gpu) for i in range(n)]


def sei_init_list(depth, sx, sy):
    """the 20 messages of tests/test_gpu_fw_space.py::test_init_over_the_space: the five wide constructions and 15 of the 20 others, a
    window that moves by five with the depth and with the format, so that the lists of any one depth and the lists of any one format
    together hold every construction"""
    FgsSei = _fw().FgsSei
    rng = np.random.default_rng(7000 + 100 * depth + 10 * sx + sy)
    g = GEOMETRIES.index((depth, sx, sy))
    cases = [(5 * (g // 4 + g % 4) + i) % G.CASES for i in range(15)] + list(range(G.CASES, SEI_CASES))
    return [space_sei(FgsSei, rng, c + SEI_CASES * g) for c in cases]


def sei_build_list(depth, sx, sy):
    """the 40 messages of test_both_builders_against_the_oracle: every construction, two chunks"""
    return sei_list(8000 + 100 * depth + 10 * sx + sy, 40, first=SEI_CASES * GEOMETRIES.index((depth, sx, sy)))


def facts_of_sei_list(msgs):
    return set().union(*[sei_facts(m) for m in msgs])


# -------------------------------------------------------------------------------------------------------------------------- AFGS1 sets

def generated_set(rng):
    """a valid parameter set over the space a bitstream spans: lag 1..3, shifts, 1..14 / 0..10 scaling points, coefficients over 8 bits"""
    a = _fw().FgsAfgs1()
    a.grain_seed = int(rng.integers(0, 65536))
    for pts, vals, scal, lo, mx in (("num_y_points", a.point_y_values, a.point_y_scaling, 1, 14),
                                    ("num_cb_points", a.point_cb_values, a.point_cb_scaling, 0, 10),
                                    ("num_cr_points", a.point_cr_values, a.point_cr_scaling, 0, 10)):
        n = int(rng.integers(lo, mx + 1))
        setattr(a, pts, n)
        xs = np.sort(rng.choice(np.arange(0, 256), size=n, replace=False))
        for k in range(n):
            vals[k] = int(xs[k])
            scal[k] = int(rng.integers(0, 256))
    a.chroma_scaling_from_luma = int(rng.integers(0, 2))
    a.grain_scaling = int(rng.integers(8, 12))
    a.ar_coeff_lag = int(rng.integers(1, 4))
    for arr, n in ((a.ar_coeffs_y, 24), (a.ar_coeffs_cb, 25), (a.ar_coeffs_cr, 25)):
        for k in range(n):
            arr[k] = int(rng.integers(-128, 128))
    a.ar_coeff_shift = int(rng.integers(6, 10))
    a.grain_scale_shift = int(rng.integers(0, 4))
    a.clip_to_restricted_range = int(rng.integers(0, 2))
    # the mix fields are ignored by the call, whatever they hold
    a.cb_mult, a.cb_luma_mult, a.cb_offset = (int(v) for v in rng.integers(0, 256, 3))
    a.cr_mult, a.cr_luma_mult, a.cr_offset = (int(v) for v in rng.integers(0, 256, 3))
    return a


def _points(a, which, xs, ys):
    setattr(a, f"num_{which}_points", len(xs))
    for k, (x, y) in enumerate(zip(xs, ys)):
        getattr(a, f"point_{which}_values")[k] = x
        getattr(a, f"point_{which}_scaling")[k] = y


def _taps(a, v):
    for arr, n in ((a.ar_coeffs_y, 24), (a.ar_coeffs_cb, 25), (a.ar_coeffs_cr, 25)):
        for k in range(n):
            arr[k] = v


def forced_afgs1(a, case, rng):
    """the forced constructions, applied to a drawn set:
      0  lag 1; no points at all; grain_scale_shift 0, ar_coeff_shift 6
      1  lag 2; one point per function
      2  lag 3; two points per function, first at 0 and last at 255, falling over an odd span (255)
      3  the maximum number of points (14 / 10 / 10), first at 0 and last at 255
      4  lag 3, taps all +127; grain_scale_shift 3, ar_coeff_shift 9
      5  lag 3, taps all -128; ar_coeff_shift 6
      6  falling segments of even (8, 234) and odd (13) span, every function used
      7  lag 1, taps all -128; grain_scale_shift 0, ar_coeff_shift 9"""
    if case == 0:
        a.ar_coeff_lag, a.grain_scale_shift, a.ar_coeff_shift = 1, 0, 6
        a.num_y_points = a.num_cb_points = a.num_cr_points = a.chroma_scaling_from_luma = 0
    elif case == 1:
        a.ar_coeff_lag, a.chroma_scaling_from_luma = 2, 0
        for w in ("y", "cb", "cr"):
            _points(a, w, [int(rng.integers(0, 256))], [int(rng.integers(0, 256))])
    elif case == 2:
        a.ar_coeff_lag, a.chroma_scaling_from_luma = 3, 0
        for w in ("y", "cb", "cr"):
            _points(a, w, [0, 255], [int(rng.integers(130, 256)), int(rng.integers(0, 120))])
    elif case == 3:
        a.chroma_scaling_from_luma = 0
        for w, mx in (("y", 14), ("cb", 10), ("cr", 10)):
            xs = [0] + sorted(int(v) for v in rng.choice(np.arange(1, 255), size=mx - 2, replace=False)) + [255]
            _points(a, w, xs, [int(v) for v in rng.integers(0, 256, mx)])
    elif case == 4:
        a.ar_coeff_lag, a.grain_scale_shift, a.ar_coeff_shift = 3, 3, 9
        _taps(a, 127)
    elif case == 5:
        a.ar_coeff_lag, a.ar_coeff_shift = 3, 6
        _taps(a, -128)
    elif case == 6:
        a.chroma_scaling_from_luma = 0
        for w in ("y", "cb", "cr"):
            _points(a, w, [0, 8, 21, 255], [int(rng.integers(200, 256)), int(rng.integers(100, 190)), int(rng.integers(30, 90)), int(rng.integers(0, 25))])
    elif case == 7:
        a.ar_coeff_lag, a.grain_scale_shift, a.ar_coeff_shift = 1, 0, 9
        _taps(a, -128)
    return a


def space_afgs1(rng, index):
    return forced_afgs1(generated_set(rng), index % AFGS1_CASES, rng)


def afgs1_list(seed, n, first=0):
    rng = np.random.default_rng(seed)
    return [space_afgs1(rng, first + i) for i in range(n)]


def afgs1_init_list(depth, sx, sy):
    return afgs1_list(7500 + 100 * depth + 10 * sx + sy, 20)


def afgs1_build_list(depth, sx, sy):
    return afgs1_list(8500 + 100 * depth + 10 * sx + sy, 40)


def afgs1_facts(a):
    out = {f"lag_{a.ar_coeff_lag}", f"grain_scale_shift_{a.grain_scale_shift}", f"ar_coeff_shift_{a.ar_coeff_shift}"}
    funcs = [("y", a.num_y_points, a.point_y_values, a.point_y_scaling)]
    if not a.chroma_scaling_from_luma:
        funcs += [("cb", a.num_cb_points, a.point_cb_values, a.point_cb_scaling), ("cr", a.num_cr_points, a.point_cr_values, a.point_cr_scaling)]
    for w, n, xs, ys in funcs:
        out.add(f"{w}_points_" + ("max" if n == (14 if w == "y" else 10) else str(n) if n < 3 else "some"))
        if n >= 2 and xs[0] == 0 and xs[n - 1] == 255:
            out.add("first_0_last_255")
        for k in range(1, n):
            assert xs[k] > xs[k - 1], "scaling points must increase strictly"
            if ys[k] < ys[k - 1]:
                out.add("falling_odd_span" if (xs[k] - xs[k - 1]) % 2 else "falling_even_span")
    n = 2 * a.ar_coeff_lag * (a.ar_coeff_lag + 1)
    for v, word in ((127, "taps_all_127"), (-128, "taps_all_minus_128")):
        if all(arr[k] == v for arr in (a.ar_coeffs_y, a.ar_coeffs_cb, a.ar_coeffs_cr) for k in range(n)):
            out.add(word)
    return out


AFGS1_REQUIRED = ({"lag_1", "lag_2", "lag_3", "first_0_last_255", "falling_odd_span", "falling_even_span", "taps_all_127", "taps_all_minus_128",
                   "grain_scale_shift_0", "grain_scale_shift_3", "ar_coeff_shift_6", "ar_coeff_shift_9"}
                  | {f"{w}_points_{n}" for w in ("y", "cb", "cr") for n in ("0", "1", "2", "max")})


def facts_of_afgs1_list(sets):
    return set().union(*[afgs1_facts(a) for a in sets])


def admitted(cfg):
    """inside what vfgs_init_* and the two builders admit (include/vfgs_hip_fw.h, refusals 42 and 9)"""
    if hasattr(cfg, "grain_seed"):
        return 1 <= cfg.ar_coeff_lag <= 3 and 8 <= cfg.grain_scaling <= 11 and 1 <= cfg.ar_coeff_shift <= 15 and cfg.grain_scale_shift <= 6 \
            and cfg.num_y_points <= 14 and cfg.num_cb_points <= 10 and cfg.num_cr_points <= 10
    return 2 <= cfg.log2_scale_factor - (1 if cfg.model_id else 0) <= 7 \
        and all(cfg.num_intensity_intervals[c] <= 256 for c in range(3) if cfg.comp_model_present_flag[c])


# ------------------------------------------------------------------------------------------------------------------------ pattern jobs

def _job(kind, chroma, seed_index, fh=0, fv=0, scale=0, shift=0, taps=None):
    j = _fw().PatternJob()
    j.kind, j.chroma, j.seed_index, j.fh, j.fv, j.scale, j.shift = kind, chroma, seed_index, fh, fv, scale, shift
    if taps is not None:
        for k, v in enumerate(np.asarray(taps).reshape(-1)):
            j.coef[k] = int(v)
    return j


def ff_jobs():
    """the frequency-filtered job space: every (fh, fv) of -1..16 squared in the 64x64 form with seed index 0 and in the 32x32 form with
    seed index 1; eight jobs with seed indices 2 and 255; cut-offs at the int16 limits -> [(words, job)], chroma per job"""
    rng = np.random.default_rng(31)
    out = [({"grid"}, _job(0, chroma, chroma, fh, fv)) for chroma in (0, 1) for fh in range(-1, 17) for fv in range(-1, 17)]
    for i in range(8):
        sd = (2, 255)[i % 2]
        out.append(({f"seed_{sd}"}, _job(0, (i // 2) % 2, sd, int(rng.integers(0, 16)), int(rng.integers(0, 16)))))
    for chroma in (0, 1):
        for fh, fv in ((-32768, 5), (7, -32768), (32767, 32767), (32767, 3), (2, 32767), (-32768, -32768)):
            out.append(({"limit"}, _job(0, chroma, chroma, fh, fv)))
    return out


TAP_CLASSES = ["random_128", "random_512", "all_32767", "alternating_limits", "one_corner"]


def _causal(lag):
    return [(j, i) for j in range(-lag, 1) for i in range(-lag, lag + 1) if i < 0 or j < 0]


def ar_jobs():
    """the auto-regressive job space: lag {1, 2, 3} x scale {1, 2, 6, 7, 8, 9, 15} x shift 1..7 in both banks; the tap class rotates per job
    -> [(words, job)]"""
    rng = np.random.default_rng(32)
    out, n, corner = [], 0, 0
    for chroma in (0, 1):
        for lag in (1, 2, 3):
            for scale in (1, 2, 6, 7, 8, 9, 15):
                for shift in range(1, 8):
                    cls = TAP_CLASSES[n % 5]
                    n += 1
                    taps = np.zeros((4, 7), dtype=np.int64)
                    cells = _causal(lag)
                    words = {cls, f"lag_{lag}", f"scale_{scale}", f"shift_{shift}", f"bank_{chroma}"}
                    if cls == "one_corner":
                        # the four corners of the causal neighbourhood: top left, top right, the far end of the sample's own row, and the
                        # right end of the row above it; a gain just under 1 so that the tap's samples carry through the whole pattern
                        j, i = ((-lag, -lag), (-lag, lag), (0, -lag), (-1, lag))[corner % 4]
                        words.add(f"corner_{corner % 4}")
                        corner += 1
                        taps[3 + j, 3 + i] = (1 if corner % 8 < 4 else -1) * min(32767, (1 << scale) - 1)
                    else:
                        for q, (j, i) in enumerate(cells):
                            taps[3 + j, 3 + i] = {"random_128": lambda: int(rng.integers(-128, 129)), "random_512": lambda: int(rng.integers(-512, 513)),
                                                  "all_32767": lambda: 32767, "alternating_limits": lambda: 32767 if q % 2 == 0 else -32768}[cls]()
                    out.append((words, _job(1, chroma, int(rng.integers(0, 3)), scale=scale, shift=shift, taps=taps)))
    return out


AR_REQUIRED = (set(TAP_CLASSES) | {f"lag_{l}" for l in (1, 2, 3)} | {f"scale_{s}" for s in (1, 2, 6, 7, 8, 9, 15)} | {f"shift_{s}" for s in range(1, 8)}
               | {"bank_0", "bank_1"} | {f"corner_{c}" for c in range(4)})


def calls_of(jobs, per_call=16):
    """split a job list into calls of at most 16 jobs, luma jobs first, slots dealt 0..7 per bank -> [[job]]"""
    luma = [j for _, j in jobs if not j.chroma]
    chroma = [j for _, j in jobs if j.chroma]
    calls = []
    while luma or chroma:
        a, luma = luma[:per_call // 2], luma[per_call // 2:]
        b, chroma = chroma[:per_call // 2], chroma[per_call // 2:]
        for bank in (a, b):
            for slot, j in enumerate(bank):
                j.index = slot
        calls.append(a + b)
    return calls
