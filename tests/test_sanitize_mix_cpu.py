"""CPU: the host layer with a luma / chroma mix active under AddressSanitizer + UndefinedBehaviorSanitizer and under
ThreadSanitizer: tests/sanitize_mix/mix_walks.cpp, built by tests/sanitize_build.py, against the unchanged
model of the HIP runtime tests/sanitize/hip_stub.cpp (host code on the CPU only; values are the GPU suite's business)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_mix" / "mix_walks.cpp"
NWALKS = 5

pytestmark = needs_gxx


def test_mix_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "mix_walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_mix_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "mix_walks_tsan", TSAN, [WALKS]), NWALKS)
