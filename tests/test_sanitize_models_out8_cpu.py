"""CPU: a model per picture with the narrowed 8-bit destination (vfgs_hip_add_grain_frame_list_models_copy8_dev,
vfgs_hip_add_grain_sp_frame_list_models_copy8_dev) in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer and under
ThreadSanitizer: tests/sanitize_models_out8/models_out8_walks.cpp, a stand-alone program with its own main, built by tests/sanitize_build.py, against the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp (host code
on the CPU only; nothing is loaded into Python and nothing is preloaded).  The head of the walks file says what the stub's kernel proves --
every destination byte of every launch -- and what it cannot.  Values are the GPU suite's business (tests/test_gpu_model_list_out8.py,
tests/test_gpu_sp_model_list_out8.py)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_models_out8" / "models_out8_walks.cpp"
NWALKS = 3

pytestmark = needs_gxx


def test_models_out8_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "models_out8_walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_models_out8_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "models_out8_walks_tsan", TSAN, [WALKS]), NWALKS)
