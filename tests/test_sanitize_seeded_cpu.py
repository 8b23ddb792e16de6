"""CPU: the frame lists with a seed per picture in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer and under
ThreadSanitizer: tests/sanitize_seeded/seeded_walks.cpp, built by tests/sanitize_build.py, against the
unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp (host code on the CPU only; that model aborts when a launch addresses
LFSR bits behind the image it was handed, and its deferred queues run a launch long after the call that queued it -- a slot of the
images' ring that is overwritten or freed too early is an access the sanitizer sees).  Values are the GPU suite's business
(tests/test_gpu_seeded_list.py)."""
from sanitize_build import ASAN_UBSAN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx

WALKS = SAN.parent / "sanitize_seeded" / "seeded_walks.cpp"
NWALKS = 7

pytestmark = needs_gxx


def test_seeded_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "seeded_walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_seeded_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "seeded_walks_tsan", TSAN, [WALKS]), NWALKS)
