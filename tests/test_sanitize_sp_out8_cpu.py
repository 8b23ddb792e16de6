"""CPU: semi-planar frames with the narrowed 8-bit destination (vfgs_hip_add_grain_sp_frame_list_copy8_dev) in the host layer under
AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer: tests/sanitize_sp_out8/sp_out8_walks.cpp, a stand-alone program
built by tests/sanitize_build.py, against the unchanged model of the HIP runtime
tests/sanitize/hip_stub.cpp (host code on the CPU only).  The planes are allocated exactly as large as the contract says -- the destination's
in bytes, at pitches of their own -- and the model's launch touches the bytes the real kernels address: a wrong extent or pitch of either
UV plane is a heap overflow the sanitizer sees.  Values are the GPU suite's business (tests/test_gpu_semiplanar_out8.py)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_sp_out8" / "sp_out8_walks.cpp"
NWALKS = 4

pytestmark = needs_gxx


def test_sp_out8_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "sp_out8_walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_sp_out8_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "sp_out8_walks_tsan", TSAN, [WALKS]), NWALKS)
