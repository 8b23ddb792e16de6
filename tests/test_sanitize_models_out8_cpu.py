"""CPU: a model per picture with the narrowed 8-bit destination (vfgs_hip_add_grain_frame_list_models_copy8_dev,
vfgs_hip_add_grain_sp_frame_list_models_copy8_dev) in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer and under
ThreadSanitizer: tests/sanitize_models_out8/models_out8_walks.cpp, a stand-alone program with its own main, built the way
tests/test_sanitize_sp_models_cpu.py builds its walks, against the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp (host code
on the CPU only; nothing is loaded into Python and nothing is preloaded).  The head of the walks file says what the stub's kernel proves --
every destination byte of every launch -- and what it cannot.  Values are the GPU suite's business (tests/test_gpu_model_list_out8.py,
tests/test_gpu_sp_model_list_out8.py)."""
import shutil
import subprocess

import pytest

from test_sanitize_cpu import CSRC, HIP_INCLUDE, HOST_SOURCES, SAN, no_aslr_prefix, run

WALKS = SAN.parent / "sanitize_models_out8" / "models_out8_walks.cpp"
NWALKS = 3

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not (HIP_INCLUDE / "hip" / "hip_runtime_api.h").exists(),
                                reason="needs g++ and the HIP headers")


def build(tmp, name, flags):
    exe = tmp / name
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", *flags, "-D__HIP_PLATFORM_AMD__", f"-I{HIP_INCLUDE}",
           f'-DVFGS_FW_TABLES_PATH="{CSRC / "fw_tables.bin"}"', *map(str, HOST_SOURCES), str(SAN / "hip_stub.cpp"), str(WALKS), "-o", str(exe), "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_models_out8_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build(tmp_path, "models_out8_walks_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.count(" ok ") == NWALKS and "FAILED" not in r.stdout, r.stdout


def test_models_out8_walks_under_thread_sanitizer(tmp_path):
    exe = build(tmp_path, "models_out8_walks_tsan", ["-fsanitize=thread"])
    r = run(exe, {"TSAN_OPTIONS": "halt_on_error=0:second_deadlock_stack=1"}, prefix=no_aslr_prefix())
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.count(" ok ") == NWALKS and "FAILED" not in r.stdout, r.stdout
