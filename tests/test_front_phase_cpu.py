"""CPU: which task a workgroup of a grain launch runs (vfgs_layout.h front_task) and the host's rule for the phase between the two
frame fronts (front_phase), as a pure function.

A stand-alone g++ program (tests/front_phase/front_phase.cpp) decodes every (blockIdx.x, blockIdx.y) of a launch's grid; held here:
 (a) the tasks (f, r) with f < nframes are dealt out exactly once each, every other index decodes to a frame the kernel skips;
 (b) with the phase on, the even front keeps the order of memory and the odd front begins at the first chroma task in every group in front
     of front_plain_from -- and runs the frame's tasks on from there, wrapping once;
 (c) the launch's last group is plain (it drains on chroma workgroups), so a launch of one group is the launch of always;
and with the phase off, or one front (lfronts == 0), the decode is today's.  No GPU needed."""
import shutil
import subprocess
from pathlib import Path

import pytest

PROGRAM = Path(__file__).resolve().parent / "front_phase" / "front_phase.cpp"

WGS = [(1080, 540), (4, 2), (3, 3), (5, 1), (1, 1)]      # (luma, one chroma plane): 4320p 4:2:0; small ones, chroma as many as luma, fewer, one each
NFRAMES = [2, 3, 4, 5, 8]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++"), "needs g++"
    out = tmp_path_factory.mktemp("front_phase") / "front_phase"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", str(PROGRAM), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def decode(exe, wy, wc, nframes, lfronts, on):
    lines = subprocess.run([str(exe), str(wy), str(wc), str(nframes), str(lfronts), str(int(on))], capture_output=True, text=True, check=True).stdout.split("\n")
    shift, plain_from, gx, gy = map(int, lines[0].split())
    tasks = [tuple(map(int, l.split())) for l in lines[1:1 + gx * gy]]
    assert len(tasks) == gx * gy
    return shift, plain_from, gx, gy, tasks


@pytest.mark.parametrize("lfronts", [0, 1])
@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("wy,wc", WGS)
def test_every_task_once_and_the_order_of_the_fronts(exe, wy, wc, on, lfronts):
    per = wy + 2 * wc
    for nframes in NFRAMES:
        shift, plain_from, gx, gy, tasks = decode(exe, wy, wc, nframes, lfronts, on)
        ctx = (wy, wc, nframes, lfronts, on)
        nfr = 1 << lfronts
        assert gx == per * nfr and gy == (nframes + nfr - 1) // nfr, ctx
        # the rule: two fronts with the phase on and more than one group, nothing else
        groups = gy
        if on and lfronts == 1 and groups > 1:
            assert (shift, plain_from) == (wy, groups - 1), ctx
        else:
            assert shift == 0, ctx
        # (a) every task of the launch's frames exactly once; what is left over lies behind the last frame
        real = [t for t in tasks if t[0] < nframes]
        assert sorted(real) == [(f, r) for f in range(nframes) for r in range(per)], ctx
        assert all(0 <= r < per and nframes <= f < gy * nfr for f, r in tasks if f >= nframes), ctx
        for by in range(gy):
            row = tasks[by * gx:(by + 1) * gx]
            for front in range(nfr):
                mine = row[front::nfr]              # this front's workgroups in the order they are dealt out
                assert all(f == by * nfr + front for f, _ in mine), ctx
                order = [r for _, r in mine]
                rotated = shift != 0 and front == 1 and by < plain_from
                if rotated:
                    # (b) Cb, Cr, Y: the first task is the first chroma task, the luma tasks follow the last Cr task
                    assert order[0] == wy and order == list(range(wy, per)) + list(range(wy)), ctx
                else:
                    assert order == list(range(per)), ctx
            # (b) / (c): rotated are the odd fronts of all groups but the last, and no other
            if nfr == 2:
                assert (row[1][1] != 0) == (on and by < gy - 1), ctx
        # (c) the last group is plain
        assert [r for _, r in tasks[(gy - 1) * gx:][0::nfr]] == list(range(per)), ctx
        assert [r for _, r in tasks[(gy - 1) * gx:][nfr - 1::nfr]] == list(range(per)), ctx


def test_headline_launch(exe):
    """7680 x 4320 4:2:0, 8 frames: 1080 luma and 540 + 540 chroma workgroups a frame; while the even front runs its luma tasks the odd front
    runs chroma and the first half of ITS luma tasks follows -- at every moment of a rotated group both plane types are being dealt out"""
    shift, plain_from, gx, gy, tasks = decode(exe, 1080, 540, 8, 1, True)
    assert (shift, plain_from, gx, gy) == (1080, 3, 4320, 4)
    for by in range(3):
        row = tasks[by * gx:(by + 1) * gx]
        for i in range(0, gx, 2):
            (_, r0), (_, r1) = row[i], row[i + 1]
            assert (r0 < 1080) != (r1 < 1080), (by, i)     # one luma, one chroma, all the way through (1080 == 540 + 540)
