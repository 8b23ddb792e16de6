"""CPU: models that carry a chroma mix (vfgs_hip_models_from_afgs1_mix, vfgs_hip_model_capture_mix, vfgs_hip_model_chroma_mix and the two list
calls with a model per picture) in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer: tests/sanitize_model_mix/
model_mix_walks.cpp, a stand-alone program built by tests/sanitize_build.py -- the host sources, the
entry point's translation unit, the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp, the walks' own stand-in for the launcher
of fw_models_kernel.  It holds the entry points to their C types (static_assert), the record's host side, the splitting into runs with the
kernel family each run is given, what the launcher of the grain kernels is handed for it (the key of a mix family with models_kernel set:
the walks' launcher stands in front of the model's and holds every launch to family_fields()), and the refusal codes.  Values are the GPU suite's business (tests/test_gpu_model_list_mix.py)."""
import ctypes as C

import versatilefilmgrain_amd.build as B
from sanitize_build import ASAN_UBSAN, CSRC, SAN, build, check_asan_ubsan, needs_gxx

WALKS = SAN.parent / "sanitize_model_mix" / "model_mix_walks.cpp"
ENTRY = CSRC / "vfgs_model_build_host.cpp"
NWALKS = 3


@needs_gxx
def test_model_mix_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    # (the walks compile tests/sanitize/hip_stub.cpp into their own translation unit)
    check_asan_ubsan(build(tmp_path, "model_mix_walks_asan", ASAN_UBSAN, [WALKS], extra=(ENTRY,), stub=False), NWALKS)


def test_the_library_exports_the_three_entry_points():
    """(no GPU: the symbols of the built library)"""
    lib = C.CDLL(str(B.build()))
    for name in ("vfgs_hip_models_from_afgs1_mix", "vfgs_hip_model_capture_mix", "vfgs_hip_model_chroma_mix"):
        assert getattr(lib, name) is not None
    from versatilefilmgrain_amd import hw
    for name in ("models_from_afgs1_mix", "model_capture_mix", "model_chroma_mix"):
        assert callable(getattr(hw.VfgsHip, name))
