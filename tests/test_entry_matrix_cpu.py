"""CPU: what every device-pointer entry of libvfgs_hip answers -- return code, error text, which of two refusals wins, the launch record,
the seed registers -- over the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp, compared byte for byte with a recording:
tests/sanitize_entries/entry_matrix.cpp, a stand-alone program built the way tests/test_sanitize_sp_models_cpu.py builds its walks, prints
one line per call, and tests/golden/entry_matrix.txt is what it printed when it was written.  The recording is NOT regenerated when the
host layer is reshaped: a reshaped host layer answers every call of the matrix as before, or this test says which line moved."""
import shutil
import subprocess

import pytest

from test_sanitize_cpu import CSRC, HIP_INCLUDE, HOST_SOURCES, ROOT, SAN, run

DRIVER = SAN.parent / "sanitize_entries" / "entry_matrix.cpp"
GOLDEN = ROOT / "tests" / "golden" / "entry_matrix.txt"

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not (HIP_INCLUDE / "hip" / "hip_runtime_api.h").exists(),
                                reason="needs g++ and the HIP headers")


def build(tmp, name, flags):
    exe = tmp / name
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", *flags, "-D__HIP_PLATFORM_AMD__", f"-I{HIP_INCLUDE}",
           f'-DVFGS_FW_TABLES_PATH="{CSRC / "fw_tables.bin"}"', *map(str, HOST_SOURCES), str(SAN / "hip_stub.cpp"), str(DRIVER), "-o", str(exe), "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_every_entry_answers_the_matrix_as_recorded(tmp_path):
    exe = build(tmp_path, "entry_matrix_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    got, want = r.stdout.splitlines(), GOLDEN.read_text().splitlines()
    moved = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not moved, f"line {moved[0] + 1} of {len(moved)} that moved:\n  recorded: {want[moved[0]]}\n  now:      {got[moved[0]]}"
    assert r.stdout == GOLDEN.read_text(), f"{len(got)} lines, recorded {len(want)}"
