"""CPU: a model per picture from planar pictures onto semi-planar surfaces (vfgs_hip_add_grain_frame_list_models_to_sp_dev,
vfgs_hip_add_grain_frame_list_models_to_sp8_dev) in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer and under
ThreadSanitizer: tests/sanitize_models_to_sp/models_to_sp_walks.cpp, a stand-alone program with its own main, built by
tests/sanitize_build.py over the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp, which the program compiles into its own
translation unit so that a launcher of its own stands in front of the model's (host code on the CPU only; nothing is loaded into Python and
nothing is preloaded).  The head of the walks file says what the model of the launch proves and what it cannot.  Values are the GPU
suite's business (tests/test_gpu_models_to_sp.py)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_models_to_sp" / "models_to_sp_walks.cpp"
NWALKS = 4

pytestmark = needs_gxx


def test_models_to_sp_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "models_to_sp_walks_asan", ASAN_UBSAN, [WALKS], stub=False), NWALKS)


def test_models_to_sp_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "models_to_sp_walks_tsan", TSAN, [WALKS], stub=False), NWALKS)
