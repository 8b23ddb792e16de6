"""Helpers of the tests of vfgs_hip_models_from_sei (TEST INFRASTRUCTURE): generated FGC SEI messages over the space a bitstream spans, and
what a message covers, read from the message alone (facts) -- so the coverage the GPU test relies on is checked without a GPU
(tests/test_sei_model_generator_cpu.py).

A message is one of 20 constructions (case = index % 20) with random values inside it: both kinds of model; 1, several, exactly 8 and more
than 8 distinct parameter sets in a list; Cb and Cr sharing patterns and not; Cb uniform on one slot and Cr on another; lower bounds out of
order, overlapping intervals, gaps below the first interval; each component absent; 256 intervals; cut-offs 0..15; scales >= 250.  The
auto-regressive values span the ranges of test_gpu_fw._random_sei: v1 -100..100, v3 -60..60, v4 0..2^log2_scale_factor - 1, v5 -40..40."""
import numpy as np

CASES = 20


def _values(rng, s, ar, scale=None, cut=None):
    """one parameter set: [scale, 5 more values]"""
    v0 = int(rng.integers(0, 250)) if scale is None else scale
    if ar:
        return [v0, int(rng.integers(-100, 101)), 0, int(rng.integers(-60, 61)), int(rng.integers(0, 1 << s.log2_scale_factor)),
                int(rng.integers(-40, 41))]
    fh, fv = (int(rng.integers(0, 16)), int(rng.integers(0, 16))) if cut is None else cut
    return [v0, fh, fv, 0, 0, 0]


def _distinct(rng, s, ar, n, taken=()):
    """n parameter sets whose values 1..5 differ pairwise (and from `taken`)"""
    out, seen = [], {tuple(t[1:]) for t in taken}
    while len(out) < n:
        v = _values(rng, s, ar)
        if tuple(v[1:]) not in seen:
            seen.add(tuple(v[1:]))
            out.append(v)
    return out


def _put(s, c, intervals):
    """intervals: [(lower, upper, values)] in the order the message lists them"""
    s.comp_model_present_flag[c] = 1
    s.num_intensity_intervals[c] = len(intervals)
    s.num_model_values[c] = 6 if s.model_id else 3
    for k, (lo, hi, v) in enumerate(intervals):
        s.intensity_interval_lower_bound[c][k] = lo
        s.intensity_interval_upper_bound[c][k] = hi
        for j in range(6):
            s.comp_model_value[c][k][j] = v[j]


def _tiled(rng, sets, first=0):
    """consecutive intervals from `first` to 255, one per entry of sets"""
    n = len(sets)
    cuts = np.sort(rng.choice(np.arange(first + 1, 255), size=n - 1, replace=False)) if n > 1 else []
    lows = [first] + [int(c) for c in cuts]
    highs = [int(c) - 1 for c in cuts] + [255]
    return [(lo, hi, v) for lo, hi, v in zip(lows, highs, sets)]


def generated_sei(FgsSei, rng, index):
    """message `index` of a generated list"""
    case = index % CASES
    s = FgsSei()
    ar = case in (1, 3, 5, 7) or (case >= 8 and case not in (17, 18) and bool(rng.integers(0, 2)))
    s.model_id = (1 if rng.integers(0, 2) else int(rng.integers(2, 256))) if ar else 0     # (any non-zero model_id is the auto-regressive model)
    s.log2_scale_factor = int(rng.integers(3, 9)) if ar else int(rng.integers(2, 8))       # (the stored shift is log2_scale_factor - ar: 2..7)
    if case in (0, 1):                  # one parameter set per list
        for c in range(3):
            _put(s, c, _tiled(rng, [_values(rng, s, ar)] if c < 2 else [[int(rng.integers(0, 250))] + _read(s, 1, 0)[1:]]))
    elif case in (2, 3):                # several
        _put(s, 0, _tiled(rng, _distinct(rng, s, ar, int(rng.integers(2, 6)))))
        cb = _distinct(rng, s, ar, int(rng.integers(2, 4)))
        _put(s, 1, _tiled(rng, cb))
        _put(s, 2, _tiled(rng, _distinct(rng, s, ar, 2, cb)))
    elif case in (4, 5):                # exactly 8 in each list
        _put(s, 0, _tiled(rng, _distinct(rng, s, ar, 8)))
        cb = _distinct(rng, s, ar, 4)
        _put(s, 1, _tiled(rng, cb))
        _put(s, 2, _tiled(rng, _distinct(rng, s, ar, 4, cb)))
    elif case in (6, 7):                # more than 8: the list is full, the rest finds no entry (or the unused one)
        _put(s, 0, _tiled(rng, _distinct(rng, s, ar, 11)))
        cb = _distinct(rng, s, ar, 6)
        _put(s, 1, _tiled(rng, cb))
        _put(s, 2, _tiled(rng, _distinct(rng, s, ar, 6, cb)))
    elif case == 8:                     # Cr repeats Cb's parameter sets with scales of its own
        _put(s, 0, _tiled(rng, _distinct(rng, s, ar, 3)))
        cb = _distinct(rng, s, ar, 3)
        _put(s, 1, _tiled(rng, cb))
        _put(s, 2, _tiled(rng, [[int(rng.integers(0, 250))] + v[1:] for v in cb[::-1]]))
    elif case == 9:                     # Cb uniform on slot 0, Cr uniform on slot 1, under a luma of two patterns
        _put(s, 0, _tiled(rng, _distinct(rng, s, ar, 2)))
        cb = _distinct(rng, s, ar, 2)
        _put(s, 1, [(0, 255, cb[0])])
        _put(s, 2, [(0, 255, cb[1])])
    elif case == 10:                    # lower bounds out of order
        for c in range(3):
            _put(s, c, _tiled(rng, _distinct(rng, s, ar, 4))[::-1])
    elif case == 11:                    # overlapping intervals
        for c in range(3):
            sets = _distinct(rng, s, ar, 3)
            _put(s, c, [(0, 140, sets[0]), (100, 200, sets[1]), (180, 255, sets[2])])
    elif case == 12:                    # gaps: below the first interval, between intervals, above the last
        for c in range(3):
            sets = _distinct(rng, s, ar, 3)
            a = int(rng.integers(5, 40))
            _put(s, c, [(a, a + 30, sets[0]), (a + 50, a + 90, sets[1]), (a + 100, 250, sets[2])])
    elif case in (13, 14, 15):          # a component absent (its fields hold values all the same: they must not be read)
        for c in range(3):
            _put(s, c, _tiled(rng, _distinct(rng, s, ar, 2)))
        s.comp_model_present_flag[case - 13] = 0
    elif case == 16:                    # 256 intervals in luma, one intensity each, over more than 8 parameter sets
        sets = _distinct(rng, s, ar, 10)
        _put(s, 0, [(k, k, [int(rng.integers(0, 250))] + sets[int(rng.integers(0, 10))][1:]) for k in range(256)])
        _put(s, 1, _tiled(rng, _distinct(rng, s, ar, 2)))
    elif case == 17:                    # uniform components with scales >= 250 at a stored shift of 11+: the packed 16-bit form does not fit at 8 bit
        s.log2_scale_factor = int(rng.integers(5, 8))
        for c in range(3):
            _put(s, c, [(0, 255, _values(rng, s, ar, scale=int(rng.integers(250, 256))))])
    elif case == 18:                    # the ends of the cut-off range
        _put(s, 0, _tiled(rng, [_values(rng, s, ar, cut=c) for c in ((0, 0), (15, 15), (0, 15), (15, 0))]))
        _put(s, 1, _tiled(rng, [_values(rng, s, ar, cut=c) for c in ((15, 15), (0, 0))]))
    else:                               # free: 1..11 intervals per component, any of them absent but luma
        for c in range(3):
            n = int(rng.integers(1, 12))
            _put(s, c, _tiled(rng, [_values(rng, s, ar) for _ in range(n)]))
            if c and not rng.integers(0, 3):
                s.comp_model_present_flag[c] = 0
    return s


def _read(s, c, k):
    return [int(s.comp_model_value[c][k][j]) for j in range(6)]


def facts(s):
    """what the message covers, as a set of words"""
    out = {"ar" if s.model_id else "ff"}
    tails = {}
    for c in range(3):
        if not s.comp_model_present_flag[c]:
            out.add(f"absent_{c}")
            tails[c] = []
            continue
        n = s.num_intensity_intervals[c]
        if n == 0:                      # (present with no interval: nothing to read; none of generated_sei's messages is)
            tails[c] = []
            continue
        lows = [int(s.intensity_interval_lower_bound[c][k]) for k in range(n)]
        highs = [int(s.intensity_interval_upper_bound[c][k]) for k in range(n)]
        vals = [_read(s, c, k) for k in range(n)]
        tails[c] = [tuple(v[1:]) for v in vals]
        if n == 256:
            out.add("intervals_256")
        if any(a > b for a, b in zip(lows, lows[1:])):
            out.add("out_of_order")
        if any(lows[i] <= highs[j] and lows[j] <= highs[i] for i in range(n) for j in range(i)):
            out.add("overlap")
        if min(lows) > 0:
            out.add("gap_below_first")
        if max(v[0] for v in vals) >= 250:
            out.add("scale_250")
        if not s.model_id:
            for v in vals:
                out.update({f"cut_{v[1]}", f"cut_{v[2]}"})
    for name, distinct in (("luma", len(set(tails[0]))), ("chroma", len(set(tails[1]) | set(tails[2])))):
        out.add(f"{name}_" + ("none" if distinct == 0 else "one" if distinct == 1 else "several" if distinct < 8 else "eight" if distinct == 8 else "more"))
    if tails[1] and tails[2]:
        out.add("chroma_shared" if set(tails[1]) & set(tails[2]) else "chroma_apart")
        whole = all(s.num_intensity_intervals[c] == 1 and s.intensity_interval_lower_bound[c][0] == 0 and s.intensity_interval_upper_bound[c][0] == 255
                    for c in (1, 2))
        if whole and tails[1] != tails[2]:
            out.add("chroma_two_uniform_slots")
    return out


REQUIRED = ({"ar", "ff", "intervals_256", "out_of_order", "overlap", "gap_below_first", "scale_250", "absent_0", "absent_1", "absent_2",
             "chroma_shared", "chroma_apart", "chroma_two_uniform_slots"}
            | {f"{l}_{w}" for l in ("luma", "chroma") for w in ("one", "several", "eight", "more")} | {f"cut_{k}" for k in range(16)})


def generated_list(FgsSei, seed, n=40):
    rng = np.random.default_rng(seed)
    return [generated_sei(FgsSei, rng, i) for i in range(n)]


def list_seed(depth, sx, sy):
    """the rng seed of a parametrisation of test_bytes_equal_the_capture_path (checked for coverage on the CPU)"""
    return 1000 * depth + 10 * sx + sy
