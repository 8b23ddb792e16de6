"""CPU: the product's host firmware (versatilefilmgrain_amd/csrc/vfgs_fw_host.cpp) against the firmware oracle, with no reference and no GPU.

tests/fw_host_records/fw_host_records.cpp is a stand-alone program: vfgs_fw_host.cpp linked with stubs that record the nine setters, the
jobs given to vfgs_hip_generate_patterns and the chroma-mix calls (built here with g++, as tests/front_phase is).  For 1000 generated SEI messages and 1000 AFGS1 sets of tests/fw_space.py (the wide lists: log2_scale_factor 2..9):
  * the setter calls equal the oracle's non-pattern records, in order;
  * the jobs come in one call, luma first, one per (bank, slot) the oracle programs, and each job's pattern by the oracle's generator
    (fw_oracle_util.job_pattern) equals the oracle's pattern for that bank and slot;
  * the chroma mix is cleared, and with the switch of vfgs_hip_afgs1_chroma_mix on (the environment variable) set as include/vfgs_hip_fw.h says."""
import ctypes as C
import os
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

import fw_oracle_util as O
import fw_space as S
import vfgs_testlib as T
from versatilefilmgrain_amd import fw

HERE = Path(__file__).resolve().parent
SOURCES = [HERE / "fw_host_records" / "fw_host_records.cpp", T.ROOT / "versatilefilmgrain_amd" / "csrc" / "vfgs_fw_host.cpp"]
N = 1000
OP_JOB, OP_CLEAR_MIX, OP_SET_MIX, OP_END = 100, 101, 102, 199


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++"), "needs g++"
    out = tmp_path_factory.mktemp("fw_host_records") / "fw_host_records"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *map(str, SOURCES), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def host_records(exe, tmp_path, cfgs, mix=False):
    """-> per parameter set, the records the host firmware's calls left"""
    inp, outp = tmp_path / "sets.bin", tmp_path / "records.bin"
    inp.write_bytes(b"".join(struct.pack("<I", 1 if hasattr(c, "grain_seed") else 0) + bytes(c) for c in cfgs))
    env = dict(os.environ, VFGS_HIP_AFGS1_CHROMA_MIX="1" if mix else "0")          # (the switch of vfgs_hip_afgs1_chroma_mix, by the environment)
    r = subprocess.run([str(exe), str(inp), str(outp)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    sets, cur = [], []
    for rec in O.parse_records(outp.read_bytes()):
        if rec[0] == OP_END:
            assert rec[1] == len(sets)
            sets.append(cur)
            cur = []
        else:
            cur.append(rec)
    assert not cur and len(sets) == len(cfgs)
    return sets


def check(cfg, host, i):
    want = O.program(cfg)
    patterns = O.patterns_of(want)
    setters = [r for r in host if r[0] < OP_JOB]
    assert setters == [r for r in want if r[0] not in (T.OP_LUMA_PATTERN, T.OP_CHROMA_PATTERN)], i
    jobs = [(a, b, fw.PatternJob.from_buffer_copy(p)) for op, a, b, p in host if op == OP_JOB]
    assert [a for a, _, _ in jobs] == list(range(len(jobs))) and all(b == len(jobs) for _, b, _ in jobs), i        # one call
    jobs = [j for _, _, j in jobs]
    assert [j.chroma for j in jobs] == sorted(j.chroma for j in jobs), i                                         # luma first
    assert sorted((j.chroma, j.index) for j in jobs) == sorted(patterns), i
    luma = [j for j in jobs if not j.chroma]
    for j in jobs:
        got = O.job_pattern(j)
        assert got == patterns[(j.chroma, j.index)][:len(got)], (i, j.chroma, j.index)
    # the tail of a chroma payload is the LAST luma job's pattern (fw_commit_chroma's last_luma), zeros without one
    for (bank, slot), p in patterns.items():
        if bank:
            assert p[1024:] == (O.job_pattern(luma[-1])[1024:] if luma else bytes(3072)), (i, slot)


def test_sei_messages(exe, tmp_path):
    msgs = S.sei_list(3, N, gpu=False)
    assert not S.SEI_REQUIRED - S.facts_of_sei_list(msgs)
    for i, (m, host) in enumerate(zip(msgs, host_records(exe, tmp_path, msgs))):
        check(m, host, i)
        assert [r[0] for r in host if r[0] > OP_JOB] == [OP_CLEAR_MIX] and host[-1][0] == OP_CLEAR_MIX, i


def test_afgs1_sets(exe, tmp_path):
    sets = S.afgs1_list(4, N)
    assert not S.AFGS1_REQUIRED - S.facts_of_afgs1_list(sets)
    plain = host_records(exe, tmp_path, sets)
    mixed = host_records(exe, tmp_path, sets, mix=True)
    for i, (a, host, hostm) in enumerate(zip(sets, plain, mixed)):
        check(a, host, i)
        assert [r[0] for r in host if r[0] > OP_JOB] == [OP_CLEAR_MIX], i
        assert [r for r in hostm if r[0] <= OP_JOB] == [r for r in host if r[0] <= OP_JOB], i
        cfl = a.chroma_scaling_from_luma != 0
        want = [(OP_CLEAR_MIX, 0, 0, b"")]
        for c, lm, cm, off in ((1, a.cb_luma_mult, a.cb_mult, a.cb_offset), (2, a.cr_luma_mult, a.cr_mult, a.cr_offset)):
            want.append((OP_SET_MIX, c, 0, struct.pack("<3i", *((64, 0, 0) if cfl else (lm - 128, cm - 128, off - 256)))))
        assert [r for r in hostm if r[0] > OP_JOB] == want, i
        assert fw.PatternJob.from_buffer_copy(next(p for op, _, _, p in host if op == OP_JOB)).seed_index == 0
    assert C.sizeof(fw.PatternJob) == 88
