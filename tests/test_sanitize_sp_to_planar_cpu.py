"""CPU: semi-planar surfaces in, planar pictures out (vfgs_hip_add_grain_sp_frame_list_to_planar_dev, _models_to_planar_dev) in the host
layer under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer: tests/sanitize_sp_to_planar/sp_to_planar_walks.cpp, a
stand-alone program with its own main, built by tests/sanitize_build.py over the unchanged model of the HIP runtime
tests/sanitize/hip_stub.cpp, which the program compiles into its own translation unit so that a launcher of its own stands in front of the
model's: it holds KernelArgs::sp_kernel == 3 to the families sp / spml and models such a launch itself, byte-exactly and inside the
destination rows (host code on the CPU only; nothing is loaded into Python and nothing is preloaded).  Values are the GPU suite's business
(tests/test_gpu_sp_to_planar.py)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_sp_to_planar" / "sp_to_planar_walks.cpp"
NWALKS = 6

pytestmark = needs_gxx


def test_sp_to_planar_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "sp_to_planar_walks_asan", ASAN_UBSAN, [WALKS], stub=False), NWALKS)


def test_sp_to_planar_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "sp_to_planar_walks_tsan", TSAN, [WALKS], stub=False), NWALKS)
