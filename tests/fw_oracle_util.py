"""The firmware oracle's Python face (TEST INFRASTRUCTURE): oracle/vfgs_fw_oracle.c, the CPU restatement of the reference firmware --
vfgs_init_sei, vfgs_init_afgs1 and the two pattern generators -- through ctypes.

  program_sei(cfg) / program_afgs1(cfg) / program(cfg)  -> program records [(op, a, b, payload)], what the reference firmware programs
      for the parameter set, in its order: directly usable by T.replay, T.BankModel, T.OracleHW and model_list_util.expect_seeded.
      A pattern payload is the reference's whole 4096-byte scratch buffer (a chroma pattern: 32x32 in the first 1024 bytes, then the
      tail of the last luma pattern of the same call; zeros where the call made none -- the reference leaves that undefined).
  job_pattern(job)                                      -> n*n bytes for a job with the fields of vfgs_hip_pattern_job
  job_payload(job, last_luma=None)                      -> the 4096-byte buffer a setter would be handed for that job

What pins the oracle: tests/test_fw_oracle_c_cpu.py."""
import ctypes as C

import numpy as np

import vfgs_testlib as T

TABLES = (T.ROOT / "versatilefilmgrain_amd" / "csrc" / "fw_tables.bin").read_bytes()
assert len(TABLES) == 7168
_CAP = 16 * (4096 + 16) + 8 * (256 + 16) + 64       # 16 patterns, 6 tables and the scalars of one call


def parse_records(raw):
    """records in the layout of oracle/trace_shim.c (no file header) -> [(op, a, b, payload)]"""
    pos, out = 0, []
    while pos < len(raw):
        op, a, b, n = np.frombuffer(raw, dtype="<i4", count=4, offset=pos)
        pos += 16
        out.append((int(op), int(a), int(b), bytes(raw[pos:pos + int(n)])))
        pos += int(n)
    return out


def _program(fn, cfg):
    buf = C.create_string_buffer(_CAP)
    n = fn(TABLES, C.addressof(cfg), buf, _CAP)
    if n < 0:
        raise ValueError("the parameter set is one the reference firmware aborts on (or leaves undefined)")
    return parse_records(buf.raw[:n])


def program_sei(cfg):
    return _program(T.oracle_lib().vfgs_fw_oracle_init_sei, cfg)


def program_afgs1(cfg):
    return _program(T.oracle_lib().vfgs_fw_oracle_init_afgs1, cfg)


def program(cfg):
    return program_afgs1(cfg) if hasattr(cfg, "grain_seed") else program_sei(cfg)


def job_pattern(job) -> bytes:
    out = C.create_string_buffer(4096)
    n = T.oracle_lib().vfgs_fw_oracle_pattern(TABLES, C.addressof(job), out)
    if n < 0:
        raise ValueError("a pattern job outside what the generators define")
    return out.raw[:n]


def job_payload(job, last_luma=None) -> bytes:
    """what vfgs_set_luma_pattern / vfgs_set_chroma_pattern receives for the job: a chroma pattern is followed by the tail of
    `last_luma` (the 4096 bytes of the last luma pattern of the same call), zeros if there is none"""
    p = job_pattern(job)
    return p if len(p) == 4096 else p + (last_luma[1024:] if last_luma is not None else bytes(3072))


def patterns_of(records):
    """{(bank, slot): payload} a program leaves, the later record of a slot winning"""
    return {(0 if op == T.OP_LUMA_PATTERN else 1, a): p for op, a, _, p in records if op in (T.OP_LUMA_PATTERN, T.OP_CHROMA_PATTERN)}
