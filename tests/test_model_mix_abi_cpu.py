"""CPU: models that carry a chroma mix (vfgs_hip_models_from_afgs1_mix, vfgs_hip_model_capture_mix, vfgs_hip_model_chroma_mix and the two list
calls with a model per picture) in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer: tests/sanitize_model_mix/
model_mix_walks.cpp, a stand-alone program built the way tests/test_models_from_afgs1_abi_cpu.py builds its walks -- the host sources, the
entry point's translation unit, the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp, the walks' own stand-in for the launcher
of fw_models_kernel.  It holds the entry points to their C types (static_assert), the record's host side, the splitting into runs with the
kernel family each run is given, what the launcher of the grain kernels is handed for it (the key of a mix family with models_kernel set:
the walks' launcher stands in front of the model's and holds every launch to family_fields()), and the refusal codes.  Values are the GPU suite's business (tests/test_gpu_model_list_mix.py)."""
import ctypes as C
import shutil

import pytest

import versatilefilmgrain_amd.build as B
from test_models_from_afgs1_abi_cpu import build
from test_sanitize_cpu import CSRC, HIP_INCLUDE, HOST_SOURCES, SAN, run

WALKS = SAN.parent / "sanitize_model_mix" / "model_mix_walks.cpp"
ENTRY = CSRC / "vfgs_model_build_host.cpp"
NWALKS = 3

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None or not (HIP_INCLUDE / "hip" / "hip_runtime_api.h").exists(), reason="needs g++ and the HIP headers")


@needs_gxx
def test_model_mix_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe, r = build(tmp_path, "model_mix_walks_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                   [*HOST_SOURCES, ENTRY, WALKS])      # (the walks compile tests/sanitize/hip_stub.cpp into their own translation unit)
    assert r.returncode == 0, r.stderr[-4000:]
    r = run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.count(" ok ") == NWALKS and "FAILED" not in r.stdout, r.stdout


def test_the_library_exports_the_three_entry_points():
    """(no GPU: the symbols of the built library)"""
    lib = C.CDLL(str(B.build()))
    for name in ("vfgs_hip_models_from_afgs1_mix", "vfgs_hip_model_capture_mix", "vfgs_hip_model_chroma_mix"):
        assert getattr(lib, name) is not None
    from versatilefilmgrain_amd import hw
    for name in ("models_from_afgs1_mix", "model_capture_mix", "model_chroma_mix"):
        assert callable(getattr(hw.VfgsHip, name))
