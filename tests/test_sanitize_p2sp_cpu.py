"""CPU: planar frames in, semi-planar surfaces out (vfgs_hip_add_grain_frame_list_to_sp_dev / _to_sp8_dev) in the host layer under
AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer: tests/sanitize_p2sp/p2sp_walks.cpp, a stand-alone program built by tests/sanitize_build.py, against the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp
(host code on the CPU only).  The planes are allocated exactly as large as the contract says; the head of the walks file says which
extents the model's row copy proves and which it cannot.  Values are the GPU suite's business (tests/test_gpu_planar_to_sp.py)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_p2sp" / "p2sp_walks.cpp"
NWALKS = 5

pytestmark = needs_gxx


def test_p2sp_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "p2sp_walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_p2sp_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "p2sp_walks_tsan", TSAN, [WALKS]), NWALKS)
