"""CPU: the host layer at sample depth 12 under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer:
tests/sanitize_depth12/depth12_walks.cpp, built by tests/sanitize_build.py, against the unchanged model of
the HIP runtime tests/sanitize/hip_stub.cpp (host code on the CPU only; values are the GPU suite's business, and so are the narrowed
destination and the persistent luma workgroups at depth 12, which that stub only models at depth 10)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_depth12" / "depth12_walks.cpp"
NWALKS = 5

pytestmark = needs_gxx


def test_depth12_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "depth12_walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_depth12_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "depth12_walks_tsan", TSAN, [WALKS]), NWALKS)
