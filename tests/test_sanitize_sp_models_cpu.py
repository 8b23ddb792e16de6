"""CPU: semi-planar frames with a model per picture (vfgs_hip_add_grain_sp_frame_list_models_dev) in the host layer under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer: tests/sanitize_sp_models/sp_model_walks.cpp, a stand-alone program built by tests/sanitize_build.py, against the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp (host code
on the CPU only).  The head of the walks file says what the stub's kernel cannot prove -- it reads the first frame's table image only --
and how the walks cover the other models' bytes.  Values are the GPU suite's business (tests/test_gpu_sp_model_list.py)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_sp_models" / "sp_model_walks.cpp"
NWALKS = 5

pytestmark = needs_gxx


def test_sp_model_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "sp_model_walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_sp_model_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "sp_model_walks_tsan", TSAN, [WALKS]), NWALKS)
