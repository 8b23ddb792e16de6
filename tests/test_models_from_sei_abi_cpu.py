"""CPU: models built from FGC SEI messages (vfgs_hip_models_from_sei) in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer
and under ThreadSanitizer: tests/sanitize_sei_model_build/sei_model_build_walks.cpp, a stand-alone program built the way
tests/test_models_from_afgs1_abi_cpu.py builds its walks -- the host sources, the two entry points' own translation units, the unchanged
model of the HIP runtime tests/sanitize/hip_stub.cpp -- plus the walks' OWN stand-ins for the launchers of fw_sei_build_kernel and
fw_models_kernel, which the stub does not know and the host layer does not name.  Host code on the CPU only; values are the GPU suite's
business (tests/test_gpu_models_from_sei.py)."""
import shutil
import subprocess

import pytest

from test_sanitize_cpu import CSRC, HIP_INCLUDE, HOST_SOURCES, SAN, no_aslr_prefix, run

WALKS = SAN.parent / "sanitize_sei_model_build" / "sei_model_build_walks.cpp"
ENTRY_AFGS1 = CSRC / "vfgs_model_build_host.cpp"
ENTRY_SEI = CSRC / "vfgs_model_build_sei_host.cpp"
NWALKS = 7

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not (HIP_INCLUDE / "hip" / "hip_runtime_api.h").exists(),
                                reason="needs g++ and the HIP headers")


def build(tmp, name, flags, sources=None):
    exe = tmp / name
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", *flags, "-D__HIP_PLATFORM_AMD__", f"-I{HIP_INCLUDE}",
           f'-DVFGS_FW_TABLES_PATH="{CSRC / "fw_tables.bin"}"',
           *map(str, sources or [*HOST_SOURCES, ENTRY_AFGS1, ENTRY_SEI, SAN / "hip_stub.cpp", WALKS]), "-o", str(exe), "-pthread"]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def test_sei_model_build_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe, r = build(tmp_path, "sei_model_build_walks_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert r.returncode == 0, r.stderr[-4000:]
    r = run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.count(" ok ") == NWALKS and "FAILED" not in r.stdout, r.stdout


def test_sei_model_build_walks_under_thread_sanitizer(tmp_path):
    exe, r = build(tmp_path, "sei_model_build_walks_tsan", ["-fsanitize=thread"])
    assert r.returncode == 0, r.stderr[-4000:]
    r = run(exe, {"TSAN_OPTIONS": "halt_on_error=0:second_deadlock_stack=1"}, prefix=no_aslr_prefix())
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.count(" ok ") == NWALKS and "FAILED" not in r.stdout, r.stdout


def test_the_host_layer_does_not_name_the_new_launcher(tmp_path):
    """the link every older sanitizer suite makes -- the three host sources against the unchanged stub, which knows nothing of
    fw_sei_build_kernel -- still succeeds: only the new entry point's translation unit needs the new launcher, and it names no other"""
    main = tmp_path / "main.cpp"
    main.write_text('#include "%s"\nint main() { vfgs_hip_shutdown(); return 0; }\n' % (CSRC.parent.parent / "include" / "vfgs_hip.h"))
    exe, r = build(tmp_path, "host_only", [], [*HOST_SOURCES, SAN / "hip_stub.cpp", main])
    assert r.returncode == 0, r.stderr[-4000:]
    exe, r = build(tmp_path, "entry_without_launcher", [], [*HOST_SOURCES, ENTRY_SEI, SAN / "hip_stub.cpp", main])
    assert r.returncode != 0 and "launch_fw_sei_build" in r.stderr and "launch_fw_models" not in r.stderr, r.stderr[-2000:]
