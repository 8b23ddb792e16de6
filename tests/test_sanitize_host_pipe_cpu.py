"""CPU: pictures in host memory as a stream (vfgs_hip_host_pipe_*, include/vfgs_hip.h) in the host layer of libvfgs_hip under
AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer: the stand-alone program tests/sanitize_host_pipe/host_pipe_walks.cpp
over the model of the HIP runtime tests/sanitize/hip_stub.cpp, built and run by tests/sanitize_build.py.  The program has its own main:
nothing is loaded into Python and nothing is preloaded."""
import sanitize_build as S

# (the program wraps the host layer's event waits, so that a wait can be made to sleep: see its head)
WALKS = [S.ROOT / "tests" / "sanitize_host_pipe" / "host_pipe_walks.cpp", "-Wl,--wrap=hipEventSynchronize"]
NWALKS = 5

pytestmark = S.needs_gxx


def test_host_pipe_walks_asan_ubsan(tmp_path):
    S.check_asan_ubsan(S.build(tmp_path, "host_pipe_walks_asan", S.ASAN_UBSAN, WALKS), NWALKS)


def test_host_pipe_walks_tsan(tmp_path):
    S.check_tsan(S.build(tmp_path, "host_pipe_walks_tsan", S.TSAN, WALKS), NWALKS)
