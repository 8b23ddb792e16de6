"""Generated hardware-layer programs (TEST INFRASTRUCTURE): the model space the 66 firmware traces do not span.

The traces of tests/golden/traces never program a general luma AND a general chroma pattern LUT together, never select slot 8 (the
reference's never-written ninth bank), never make Cb and Cr uniform on different slots, hold no -128, no scale above 208, no
scale_shift 7 and only two setter orders.  `program(name)` builds a programming sequence in the format `T.replay()` takes for every
such case; `content(name, ...)` builds frames for it; `expected_form(records, wide)` restates, from vfgs_layout.h and the header
comments, which form of the table image (general / one pattern, per luma and chroma) the library has to choose for a program.

Names are `<class>_<depth>_<format>[_<variant>]`, e.g. `general_runs_10_420`, `pk16_split_8_444_s7y`.  Everything random comes from
the integer generator below, seeded from the name: the same name means the same bytes on every machine, whatever numpy it has.
"""
from __future__ import annotations

import re

import numpy as np

import vfgs_testlib as T

SUB = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "440": (1, 2)}
DEPTHS = (8, 10, 12)
FORMATS = ("420", "422", "444", "440")
M64 = (1 << 64) - 1


class Rng:
    """splitmix64 over an FNV-1a hash of the name, in plain Python integers."""

    def __init__(self, name: str):
        h = 0xcbf29ce484222325
        for ch in name.encode():
            h = ((h ^ ch) * 0x100000001b3) & M64
        self.s = h

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def below(self, n: int) -> int:
        return self.next() % n

    def between(self, lo: int, hi: int) -> int:
        """lo..hi, both included"""
        return lo + self.next() % (hi - lo + 1)

    def bytes(self, n: int) -> bytes:
        return b"".join(self.next().to_bytes(8, "little") for _ in range((n + 7) // 8))[:n]

    def shuffle(self, items: list) -> list:
        items = list(items)
        for i in range(len(items) - 1, 0, -1):
            j = self.below(i + 1)
            items[i], items[j] = items[j], items[i]
        return items


def parse(name: str):
    """-> (class, depth, format, variant or '')"""
    m = re.fullmatch(r"(.+?)_(8|10|12)_(420|422|444|440)(?:_(.+))?", name)
    assert m, f"not a program name: {name}"
    return m.group(1), int(m.group(2)), m.group(3), m.group(4) or ""


def fits16_limit(shift: int) -> int:
    """the largest scale an 8-bit one-pattern component may hold at scale_shift `shift` (stored shift + 6):
    max(scale) * 127 + 2^(shift + 5) <= 32767"""
    return (32767 - (1 << (shift + 5))) // 127


def copied_offsets(fmt: str) -> np.ndarray:
    """offsets of the 4096-byte vfgs_set_chroma_pattern payload that the call copies at this format: rows r < 64/csuby,
    bytes (64/csuby)*r + x with x < 64/csubx (the pitch comes from csuby, the length from csubx)"""
    sx, sy = SUB[fmt]
    r, x = np.meshgrid(np.arange(64 // sy), np.arange(64 // sx), indexing="ij")
    return np.unique((64 // sy) * r + x)


# --------------------------------------------------------------------------- pieces of a model

def _pattern(rng: Rng, lowest=-128, extremes=False) -> np.ndarray:
    """4096 int8: the full range down to `lowest`, or mostly +-127"""
    raw = np.frombuffer(rng.bytes(4096), dtype=np.uint8)
    if extremes:
        table = np.array([127, -127, 127, -127, 127, -127, 126, -126, -1, 0, 1, 64, 127, -127, 127, -127], dtype=np.int8)
        return table[raw & 15].copy()
    p = raw.view(np.int8).copy()
    if lowest > -128:
        p[p < lowest] = lowest
    return p


def _with_m128(p: np.ndarray, rng: Rng, offsets=None, count=24) -> np.ndarray:
    """`count` bytes of p (among `offsets`, default anywhere) set to -128"""
    p = p.copy()
    offsets = np.arange(4096) if offsets is None else offsets
    for _ in range(count):
        p[int(offsets[rng.below(len(offsets))])] = -128
    return p


def _without_m128(p: np.ndarray) -> np.ndarray:
    p = p.copy()
    p[p == -128] = -127
    return p


def _plut_uniform(rng: Rng, slot: int) -> bytes:
    """one slot for every intensity, garbage in the low nibbles (the reference reads the high nibble only)"""
    return bytes((slot << 4) | (b & 15) for b in rng.bytes(256))


def _plut_runs(rng: Rng, slots, max_run=40, force=None) -> bytes:
    """piecewise constant over runs of 1..max_run intensities, slots drawn from `slots`; force: a slot every fourth run takes (runs of at most 12)"""
    out, k = [], 0
    while len(out) < 256:
        n = rng.between(1, max_run)
        s = slots[rng.below(len(slots))]
        if force is not None and k % 4 == 1:
            s, n = force, min(n, 12)
        out += [s] * n
        k += 1
    low = rng.bytes(256)
    return bytes((s << 4) | (b & 15) for s, b in zip(out[:256], low))


def _plut_per_intensity(rng: Rng, slots) -> bytes:
    """the slot changes at EVERY intensity"""
    out, prev = [], -1
    for b in rng.bytes(256):
        s = slots[rng.below(len(slots))]
        while s == prev:
            s = slots[rng.below(len(slots))]
        out.append((s << 4) | (b & 15))
        prev = s
    return bytes(out)


def _slut(rng: Rng, top=255, body=None, peaks=0) -> bytes:
    """scale LUT: entries 0..body (default top), `peaks` random entries (at least one if top < 255 matters) set to `top`"""
    body = top if body is None else min(body, top)
    lut = [b % (body + 1) for b in rng.bytes(256)]
    for _ in range(peaks):
        lut[rng.below(256)] = top
    return bytes(lut)


class Spec:
    """the end state of a program; emitted in the firmware's order (depth, subsampling, patterns, LUTs, shift, range, seed)"""

    def __init__(self, depth, fmt):
        self.depth, self.fmt = depth, fmt
        self.luma = [None] * 8
        self.chroma = [None] * 8
        self.plut = [None] * 3
        self.slut = [None] * 3
        self.shift, self.legal, self.seed = 5, 0, 1

    def records(self):
        sx, sy = SUB[self.fmt]
        rec = [(T.OP_DEPTH, self.depth, 0, b""), (T.OP_CHROMA_SUBSAMPLING, sx, sy, b"")]
        rec += [(T.OP_LUMA_PATTERN, k, 0, self.luma[k].tobytes()) for k in range(8)]
        rec += [(T.OP_CHROMA_PATTERN, k, 0, self.chroma[k].tobytes()) for k in range(8)]
        for c in range(3):
            rec += [(T.OP_SCALE_LUT, c, 0, self.slut[c]), (T.OP_PATTERN_LUT, c, 0, self.plut[c])]
        rec += [(T.OP_SCALE_SHIFT, self.shift, 0, b""), (T.OP_LEGAL_RANGE, self.legal, 0, b""), (T.OP_SEED, self.seed, 0, b"")]
        return rec


SHUFFLED_TWINS = {"shuffled_0": "general_runs", "shuffled_1": "one_same_slot", "shuffled_2": "one_cb_cr_differ"}
# scale_shift of the two classes that exist in every format, by format: every value 2..7 occurs at every depth
_SHIFTS = {"general_runs": (2, 7, 4, 5), "general_per_intensity": (3, 6, 7, 2)}


def _spec(name: str) -> Spec:
    cls, depth, fmt, variant = parse(name)
    rng = Rng(name)
    s = Spec(depth, fmt)
    fi, di = FORMATS.index(fmt), DEPTHS.index(depth)
    s.shift = _SHIFTS[cls][fi] if cls in _SHIFTS else rng.between(2, 7)
    s.legal = rng.below(2)
    s.seed = rng.below(1 << 32)
    s.luma = [_pattern(rng) for _ in range(8)]
    s.chroma = [_pattern(rng) for _ in range(8)]
    all9 = list(range(9))
    uniform = [False] * 3          # components meant to take the one-pattern form: their scales respect the 8-bit limit
    cap = lambda: min(255, fits16_limit(s.shift)) if depth == 8 else 255

    def general(c, slots=all9, **kw):
        s.plut[c] = _plut_runs(rng, slots, **kw)

    def one(c, slot, clean=True):
        s.plut[c] = _plut_uniform(rng, slot)
        uniform[c] = True
        if clean and slot < 8:
            bank = s.luma if c == 0 else s.chroma
            bank[slot] = _without_m128(bank[slot])

    if cls == "general_runs":
        for c in range(3):
            general(c)
    elif cls == "general_per_intensity":
        for c in range(3):
            s.plut[c] = _plut_per_intensity(rng, all9)
    elif cls == "one_y_general_c":
        one(0, rng.between(1, 7))
        general(1), general(2)
    elif cls == "general_y_one_c":
        general(0)
        one(1, rng.between(1, 7)), one(2, rng.between(1, 7))
    elif cls == "one_same_slot":
        k = rng.between(1, 7)
        s.luma = [_pattern(rng, lowest=-127) for _ in range(8)]
        s.chroma = [_pattern(rng, lowest=-127) for _ in range(8)]
        for c in range(3):
            one(c, k)
    elif cls == "one_cb_cr_differ":
        a = rng.between(0, 7)
        b = (a + rng.between(1, 7)) % 8
        one(0, rng.between(0, 7)), one(1, a), one(2, b)
    elif cls == "slot8_luma":
        one(0, 8), one(1, rng.between(1, 7)), one(2, rng.between(1, 7))
    elif cls == "slot8_cb":
        one(0, rng.between(1, 7)), one(1, 8), one(2, rng.between(1, 7))
    elif cls == "slot8_chroma":
        one(0, rng.between(1, 7)), one(1, 8), one(2, 8)
    elif cls == "slot8_some":
        s.shift = 2 + s.shift % 4      # (2..5: with a quarter of the intensities on the zero slot, shift 7 would leave too few samples changed)
        for c in range(3):
            general(c, slots=all9[:8], force=8)
    elif cls == "m128_unselected":
        sel = [rng.between(0, 7) for _ in range(3)]
        for c in range(3):
            one(c, sel[c])
        for k in range(8):
            if k != sel[0]:
                s.luma[k] = _with_m128(s.luma[k], rng)
            if k not in sel[1:]:
                s.chroma[k] = _with_m128(s.chroma[k], rng, offsets=copied_offsets(fmt))
    elif cls == "m128_cr_only":
        a = rng.between(0, 7)
        b = (a + rng.between(1, 7)) % 8
        one(0, rng.between(0, 7)), one(1, a), one(2, b, clean=False)
        s.luma = [_without_m128(p) for p in s.luma]
        s.chroma = [_without_m128(p) for p in s.chroma]
        s.chroma[b] = _with_m128(s.chroma[b], rng, offsets=copied_offsets(fmt))
    elif cls == "m128_outside_window":
        assert fmt != "444", "4:4:4 copies the whole payload"
        outside = np.setdiff1d(np.arange(4096), copied_offsets(fmt))
        a = rng.between(0, 7)
        b = (a + rng.between(1, 7)) % 8
        one(0, rng.between(0, 7)), one(1, a), one(2, b)
        for k in (a, b):
            s.chroma[k] = _with_m128(s.chroma[k], rng, offsets=outside, count=200)
    elif cls == "pk16_split":
        assert depth == 8 and variant in ("s2", "s5", "s7", "s2y", "s5y", "s7y")
        s.shift = int(variant[1])
        s.luma = [_pattern(rng, extremes=True) for _ in range(8)]
        s.chroma = [_pattern(rng, extremes=True) for _ in range(8)]
        one(0, rng.between(0, 7)), one(1, rng.between(0, 7)), one(2, rng.between(0, 7))
    elif cls == "zero_scale_one_component":
        for c in range(3):
            general(c)
    else:
        raise ValueError(f"unknown program class {cls}")

    for c in range(3):
        s.slut[c] = _slut(rng, top=cap(), peaks=2) if uniform[c] else _slut(rng, peaks=2)      # (the largest scale allowed is met)
    if cls == "zero_scale_one_component":
        s.slut[(fi + di) % 3] = bytes(256)
    if cls == "pk16_split":
        limit = fits16_limit(s.shift)
        at, over = min(limit, 255), min(limit + 1, 255)
        # (at shift 2 a scale near 255 moves a sample by up to 126: few intensities hold it, so that the clip stays rare)
        body, peaks = (40, 6) if s.shift == 2 else (None, 24)
        tops = (over, at - 3, at - 1) if variant.endswith("y") else (at, at, over)
        for c in range(3):
            s.slut[c] = _slut(rng, top=tops[c], body=body, peaks=peaks)
    return s


def twin_of(name: str) -> str:
    """the unshuffled program a `shuffled_<k>` program has to end in the state of"""
    cls, depth, fmt, _ = parse(name)
    return f"{SHUFFLED_TWINS[cls]}_{depth}_{fmt}"


def _shuffled(name: str):
    """The end state of the twin reached the long way round: set_depth 8 -> 10 -> target with set_scale_shift between the flips; the
    LUTs before the patterns; every setter called twice, the last call winning; half the chroma patterns set while another
    subsampling is in force.  Where that subsampling is 4:4:4 (the whole payload lands in the bank, vfgs_hw.c:320-325) the call that
    WINS for those slots is made there, with a payload laid out so that the region the final format reads holds the twin's bytes
    (and -128 elsewhere); the other half, and every slot of a 4:4:4 program, gets its last call after the switch."""
    cls, depth, fmt, _ = parse(name)
    s = _spec(twin_of(name))
    rng = Rng(name)
    sx, sy = SUB[fmt]
    other = "420" if fmt == "444" else "444"
    junk = lambda: _pattern(rng).tobytes()
    wrong = lambda b: bytes(x ^ 0x5a for x in b)
    early = set(rng.shuffle(range(8))[:4])

    def merge(chains):
        chains, out = [list(c) for c in chains if c], []
        while chains:
            c = chains[rng.below(len(chains))]
            out.append(c.pop(0))
            if not c:
                chains.remove(c)
        return out

    depth_chain = [(T.OP_DEPTH, 8, 0, b""), (T.OP_SCALE_SHIFT, 2 + (s.shift - 1) % 6, 0, b""), (T.OP_DEPTH, 10, 0, b""),
                   (T.OP_SCALE_SHIFT, s.shift, 0, b""), (T.OP_DEPTH, depth, 0, b"")]
    phase1 = [[(T.OP_CHROMA_SUBSAMPLING, *SUB[other], b"")]]
    for c in range(3):
        phase1.append([(T.OP_SCALE_LUT, c, 0, wrong(s.slut[c])), (T.OP_SCALE_LUT, c, 0, s.slut[c])])
        phase1.append([(T.OP_PATTERN_LUT, c, 0, wrong(s.plut[c])), (T.OP_PATTERN_LUT, c, 0, s.plut[c])])
    phase1.append([(T.OP_LEGAL_RANGE, 1 - s.legal, 0, b""), (T.OP_SEED, s.seed ^ 0x1234567, 0, b"")])
    rec = merge(phase1)
    # chroma patterns under the other subsampling (after it is in force: the LUT and range calls above may come before or after it)
    at = max(i for i, r in enumerate(rec) if r[0] == T.OP_CHROMA_SUBSAMPLING)
    under_other, late = [], []
    for k in sorted(early):
        p = s.chroma[k]
        if other == "444":
            laid = np.full(4096, -128, np.int8)         # bank[r][x] = payload[64 r + x] there; the final format reads bank[r][x] = p[(64/sy) r + x]
            for r in range(64 // sy):
                laid[64 * r: 64 * r + 64 // sx] = p[(64 // sy) * r: (64 // sy) * r + 64 // sx]
            under_other.append([(T.OP_CHROMA_PATTERN, k, 0, junk()), (T.OP_CHROMA_PATTERN, k, 0, laid.tobytes())])
        else:
            under_other.append([(T.OP_CHROMA_PATTERN, k, 0, junk())])
            late.append([(T.OP_CHROMA_PATTERN, k, 0, p.tobytes())])
    rec = rec[:at + 1] + merge([rec[at + 1:]] + under_other)
    rec.append((T.OP_CHROMA_SUBSAMPLING, sx, sy, b""))
    phase2 = late + [depth_chain, [(T.OP_LEGAL_RANGE, s.legal, 0, b""), (T.OP_SEED, s.seed, 0, b"")]]
    for k in range(8):
        phase2.append([(T.OP_LUMA_PATTERN, k, 0, junk()), (T.OP_LUMA_PATTERN, k, 0, s.luma[k].tobytes())])
        if k not in early:
            phase2.append([(T.OP_CHROMA_PATTERN, k, 0, junk()), (T.OP_CHROMA_PATTERN, k, 0, s.chroma[k].tobytes())])
    return rec + merge(phase2)


_cache: dict = {}


def program(name: str):
    """-> list of (op, a, b, payload), the format T.replay() takes"""
    if name not in _cache:
        cls = parse(name)[0]
        _cache[name] = _shuffled(name) if cls in SHUFFLED_TWINS else _spec(name).records()
    return _cache[name]


def classes():
    return ["general_runs", "general_per_intensity", "one_y_general_c", "general_y_one_c", "one_same_slot", "one_cb_cr_differ",
            "slot8_luma", "slot8_cb", "slot8_chroma", "slot8_some", "m128_unselected", "m128_cr_only", "m128_outside_window",
            "pk16_split", "zero_scale_one_component", "shuffled_0", "shuffled_1", "shuffled_2"]


def names(cls=None, depth=None, fmt=None) -> list[str]:
    """every program name, or those of one class / depth / format"""
    out = []
    for c in classes():
        for d in DEPTHS:
            for f in FORMATS:
                if c == "m128_outside_window" and f == "444":
                    continue
                if c == "pk16_split":
                    if d == 8:
                        out += [f"{c}_{d}_{f}_{v}" for v in ("s2", "s5", "s7", "s2y", "s5y", "s7y")]
                    continue
                out.append(f"{c}_{d}_{f}")
    return [n for n in out if (cls is None or parse(n)[0] == cls) and (depth is None or parse(n)[1] == depth)
            and (fmt is None or parse(n)[2] == fmt)]


def at_depth(records, depth):
    """the same program with the depth it ENDS in replaced (the last depth record)"""
    last = max(i for i, r in enumerate(records) if r[0] == T.OP_DEPTH)
    return [(op, depth if i == last else a, b, p) for i, (op, a, b, p) in enumerate(records)]


# --------------------------------------------------------------------------- frames

VARIANTS = ("in_range", "garbage")
_POOL = 65521


def content(name: str, width: int, height: int, nframes: int, variant: str = "in_range", pad: int = 0):
    """Frames for a program.  'in_range': picture samples in [64 << bs, 192 << bs), garbage in the stride padding (up to the full
    container width at 10 / 12 bit).  'garbage': anything the container holds in the picture as well -- at 10 / 12 bit that is
    intensity wrap and values >= 0x7000.  pad: samples added to both row pitches (a caller's padded allocation)."""
    assert variant in VARIANTS
    _, depth, fmt, _ = parse(name)
    sx, sy = SUB[fmt]
    bs = depth - 8
    rng = Rng(f"content/{name}/{width}x{height}/{variant}")
    pool = np.frombuffer(rng.bytes(_POOL), dtype=np.uint8)
    out, at = [], 0

    def take(n):            # n bytes: the pool repeated, every repetition changed (integer operations only)
        nonlocal at
        idx = np.arange(at, at + n, dtype=np.int64)
        at += n
        return pool[idx % _POOL] ^ ((idx // _POOL) * 29 + (idx // _POOL >> 3)).astype(np.uint8)

    for _ in range(nframes):
        f = T.Frame(width, height, depth, sx, sy)
        if pad:
            f = T.Frame(width, height, depth, sx, sy, f.stride + pad, f.cstride + pad)
        for p, (w, h) in zip(f.planes(), ((width, height), (f.cwidth, f.cheight), (f.cwidth, f.cheight))):
            raw = take(p.size * p.itemsize).view(p.dtype).reshape(p.shape)
            p[...] = raw
            if variant == "in_range":
                p[:h, :w] = (64 << bs) + raw[:h, :w] % (128 << bs)
        out.append(f)
    return out


# --------------------------------------------------------------------------- the form the library has to choose

class _FullBanks(T.StateModel):
    """StateModel with the chroma bank kept whole: what a call under one subsampling leaves where another one reads"""

    def __init__(self):
        super().__init__()
        self.cbank = np.zeros((8, 64, 64), np.int8)

    def set_chroma_pattern(self, i, P):
        p = np.frombuffer(bytes(P), dtype=np.int8)
        for r in range(64 // self.suby):
            self.cbank[i, r, :64 // self.subx] = p[(64 // self.suby) * r: (64 // self.suby) * r + 64 // self.subx]


def expected_form(records, wide: bool = False):
    """(one_y, one_c) by the documented rule (vfgs_layout.h "one-pattern form", "packed 16-bit form"; vfgs_host.cpp header comment):
    a component takes the one-pattern form when its pattern LUT selects one slot for every intensity, that slot is the all-zero
    slot 8 or holds no -128 in the region the format reads (the form keeps a negated copy), and -- at 8 bit, where pattern and
    scale are multiplied in 16 bits -- max(scale) * 127 + 2^(stored shift - 1) <= 32767.  Chroma needs all of it for Cb and Cr.
    Pictures wider than 8192 samples (`wide`) have one-pattern kernels only where csubx == csuby and chroma is one-pattern."""
    st = _FullBanks()
    T.replay(st, records)

    def one(c):
        slots = {b >> 4 for b in st.plut[c]}
        if len(slots) != 1:
            return False
        k = slots.pop()
        if k < 8:
            region = st.luma.get(k, np.zeros((64, 64), np.int8)) if c == 0 else st.cbank[k, :64 // st.suby, :64 // st.subx]
            if (region == -128).any():
                return False
        if st.bs == 0 and max(st.slut[c]) * 127 + (1 << (st.shift - 1)) > 32767:
            return False
        return True

    one_y, one_c = one(0), one(1) and one(2)
    if wide and not (st.subx == st.suby and one_c):
        return False, False
    return one_y, one_c
