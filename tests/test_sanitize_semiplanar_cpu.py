"""CPU: semi-planar frames (vfgs_hip_add_grain_sp_frame_list_dev) in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer
and under ThreadSanitizer: tests/sanitize_semiplanar/sp_walks.cpp, a stand-alone program built by tests/sanitize_build.py, against the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp (host code on the CPU only).  The planes
are allocated exactly as large as the contract says, and the model's launch touches the bytes the real kernels address: a wrong extent
or pitch of the UV plane is a heap overflow the sanitizer sees.  Values are the GPU suite's business (tests/test_gpu_semiplanar.py)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_semiplanar" / "sp_walks.cpp"
NWALKS = 5

pytestmark = needs_gxx


def test_semiplanar_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "sp_walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_semiplanar_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "sp_walks_tsan", TSAN, [WALKS]), NWALKS)
