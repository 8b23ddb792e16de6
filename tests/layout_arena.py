"""One allocation per call, the planes back to back (TEST INFRASTRUCTURE; numpy only): the memory a real caller hands over.

Every other GPU test gives each plane a torch allocation of its own -- 256-byte aligned, the pitch rounded up to 64 samples, the height to
16 rows -- which is kinder than include/vfgs_hip.h promises to accept.  An ARENA is one host byte buffer that becomes ONE device (or host)
allocation and holds every plane a call addresses, its sources and its destinations:

Placement   plane group i of case j starts at RESIDUES[(i + j) % 8] mod 256: never 0 mod 256, mostly 16 mod 32.  The frames of a contiguous
            batch follow frame 0 at the tight frame pitch, pitch x rows.
Pitches     the smallest the contract accepts: whole 16-sample blocks of the row, rounded up to 16 bytes (8-bit subsampled chroma with an
            odd block count: 8 pad bytes).
Rows        exactly the rows the call addresses: height, ceil(height / csuby), a part's own lines.
Guards      in front of the first group, between groups and behind the last: random bytes, at least guard_bytes() each (twice the largest
            ring group of any walk of vfgs_layout.h, and no less than 16 KiB), so a store that missed its row by a whole group still lands
            inside the arena and is found by comparing bytes.
Region      region_mask(): the bytes the contract allows the call to write -- the whole blocks of every addressed row of every destination
            plane.  Everything else -- guards, pad bytes, the sources of an out-of-place call -- must come back unchanged.

tests/layout_cases.py builds the arenas of its cases and their expectation with this; compare() is the one whole-arena comparison."""
from __future__ import annotations

import re
from collections import namedtuple

import numpy as np

import vfgs_testlib as T

RESIDUES = (16, 48, 32, 80, 144, 64, 112, 240)
MIN_GUARD = 16 << 10
LAYOUT_H = T.ROOT / "versatilefilmgrain_amd" / "csrc" / "vfgs_layout.h"

# name: "<side>.f<frame>.<role>"; role: Y / U / V / UV; side: "io" (in place), "src", "dst"; off: byte offset of the plane's first row in the
# arena; pitch, rowbytes (the whole blocks of a row) in bytes; rows: the rows the arena holds; row0: the plane's own row number of the first
# of them (a part's part_y, or part_y / csuby); sz: bytes of a container
Plane = namedtuple("Plane", "name role side frame off pitch rows rowbytes sz row0")
# what a layout asks for: the same without the offset
Want = namedtuple("Want", "name role side frame pitch rows rowbytes sz row0")


def ring_group_bytes(text=None):
    """-> (bytes of a planar ring group, bytes of a UV ring group) as vfgs_layout.h has them: a position is kMaxUnits 16-byte units (a UV
    position twice that), a group is the ring depth of positions"""
    text = LAYOUT_H.read_text() if text is None else text
    units = int(re.search(r"constexpr int kMaxUnits = (\d+);", text).group(1))
    rings = [int(v) for v in re.findall(r"#define VFGS_RING\w* (\d+)", text)]
    sp_rings = [int(v) for v in re.findall(r"constexpr int kSp\w*Ring = (\d+);", text)]
    assert rings and sp_rings, "vfgs_layout.h no longer names its ring depths as this parser expects"
    return max(rings) * units * 16, max(sp_rings) * 2 * units * 16


def guard_bytes():
    return max(MIN_GUARD, 2 * max(ring_group_bytes()))


def min_pitch(nblk, sz, csubx=1):
    """the smallest pitch in bytes the contract accepts for a row of nblk blocks: its whole blocks, rounded up to 16 bytes"""
    return (16 * nblk // csubx * sz + 15) // 16 * 16


class Arena:
    """buf: the bytes (uint8); planes: [Plane]; groups: [[index into planes]] -- the planes that lie back to back; guards: [(begin, end)]"""

    def __init__(self, groups, index, seed):
        """groups: [[Want]]; index: the case's number (rotates the residues); seed: of the fill"""
        g = guard_bytes()
        self.planes, self.groups, self.guards = [], [], []
        at = 0
        for i, group in enumerate(groups):
            begin = at
            at += g
            at += (RESIDUES[(i + index) % len(RESIDUES)] - at) % 256
            self.guards.append((begin, at))
            self.groups.append([])
            for w in group:
                assert w.pitch % 16 == 0 and w.pitch >= w.rowbytes and w.rows > 0
                self.groups[-1].append(len(self.planes))
                self.planes.append(Plane(w.name, w.role, w.side, w.frame, at, w.pitch, w.rows, w.rowbytes, w.sz, w.row0))
                at += w.pitch * w.rows
        self.guards.append((at, at + g))
        at += g
        self._by_name = {(p.side, p.frame, p.role): p for p in self.planes}
        self.buf = np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)

    def copy(self):
        a = object.__new__(Arena)
        a.planes, a.groups, a.guards, a._by_name, a.buf = self.planes, self.groups, self.guards, self._by_name, self.buf.copy()
        return a

    def plane(self, side, frame, role) -> Plane:
        return self._by_name[side, frame, role]

    def rows(self, p: Plane, buf=None):
        """the plane as (rows, pitch) bytes: a view"""
        buf = self.buf if buf is None else buf
        return buf[p.off:p.off + p.rows * p.pitch].reshape(p.rows, p.pitch)

    def put(self, p: Plane, a, buf=None):
        """rows row0 .. of the 2-d array `a` (containers), their whole blocks, copied into place, row for row"""
        n = p.rowbytes // p.sz
        assert a.itemsize == p.sz and a.shape[0] >= p.row0 + p.rows and a.shape[1] >= n, (p, a.shape)
        self.rows(p, buf)[:, :p.rowbytes] = np.ascontiguousarray(a[p.row0:p.row0 + p.rows, :n]).view(np.uint8)

    def get(self, p: Plane, a, buf=None):
        """the inverse: the plane's rows copied out of the arena into rows row0 .. of `a`"""
        n = p.rowbytes // p.sz
        assert a.itemsize == p.sz and a.shape[0] >= p.row0 + p.rows and a.shape[1] >= n, (p, a.shape)
        a[p.row0:p.row0 + p.rows, :n] = np.ascontiguousarray(self.rows(p, buf)[:, :p.rowbytes]).view(a.dtype)

    def region_mask(self):
        """True: a byte the call may write"""
        m = np.zeros(self.buf.size, bool)
        for p in self.planes:
            if p.side != "src":
                self.rows(p, m)[:, :p.rowbytes] = True
        return m

    def sample_mask(self, p: Plane, mask2d, out):
        """clear in `out` (bytes of the arena) the containers of plane p that the 2-d boolean mask2d (containers, True: compared) leaves out"""
        n = p.rowbytes // p.sz
        self.rows(p, out)[:, :p.rowbytes] &= np.repeat(mask2d[p.row0:p.row0 + p.rows, :n], p.sz, axis=1)

    def describe(self, o: int) -> str:
        """where byte o of the arena lies: the plane, the row, the byte in the row, and region / pad / guard / source"""
        for p in self.planes:
            if p.off <= o < p.off + p.rows * p.pitch:
                row, byte = divmod(o - p.off, p.pitch)
                kind = "a source" if p.side == "src" else "the region" if byte < p.rowbytes else "the pad"
                return f"plane {p.name}, row {p.row0 + row} (row {row} of the arena's), byte {byte} of the row: in {kind}"
        p = min(self.planes, key=lambda q: min(abs(o - q.off), abs(o - (q.off + q.rows * q.pitch - 1))))
        row, byte = divmod(o - p.off, p.pitch)
        where = "in front of" if o < p.off else "behind"
        return f"plane {p.name}, row {p.row0 + row} (row {row} of the arena's: {where} the plane), byte {byte} of the row: in a guard"


def compare(arena: Arena, got, want, compared=None, what=""):
    """the whole-arena comparison: got, want: bytes of the arena; compared: None, or False where a byte is left out (the mix, inside the region)"""
    assert got.shape == want.shape == arena.buf.shape
    bad = got != want
    if compared is not None:
        bad &= compared
    if bad.any():
        at = np.flatnonzero(bad)
        o = int(at[0])
        raise AssertionError(f"{what}: {len(at)} bytes differ from the expectation, the first at arena offset {o}: {arena.describe(o)}; "
                             f"got {int(got[o])}, want {int(want[o])}; the last at {int(at[-1])}: {arena.describe(int(at[-1]))}")
