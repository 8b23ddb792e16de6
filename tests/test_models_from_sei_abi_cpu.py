"""CPU: models built from FGC SEI messages (vfgs_hip_models_from_sei) in the host layer under AddressSanitizer + UndefinedBehaviorSanitizer
and under ThreadSanitizer: tests/sanitize_sei_model_build/sei_model_build_walks.cpp, a stand-alone program built by tests/sanitize_build.py -- the host sources, the two entry points' own translation units, the unchanged
model of the HIP runtime tests/sanitize/hip_stub.cpp -- plus the walks' OWN stand-ins for the launchers of fw_sei_build_kernel and
fw_models_kernel, which the stub does not know and the host layer does not name.  Host code on the CPU only; values are the GPU suite's
business (tests/test_gpu_models_from_sei.py)."""
from sanitize_build import ASAN_UBSAN, CSRC, PLAIN, SAN, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx, try_build

WALKS = SAN.parent / "sanitize_sei_model_build" / "sei_model_build_walks.cpp"
ENTRY_AFGS1 = CSRC / "vfgs_model_build_host.cpp"
ENTRY_SEI = CSRC / "vfgs_model_build_sei_host.cpp"
NWALKS = 7

pytestmark = needs_gxx


def test_sei_model_build_walks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "sei_model_build_walks_asan", ASAN_UBSAN, [WALKS], extra=(ENTRY_AFGS1, ENTRY_SEI)), NWALKS)


def test_sei_model_build_walks_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "sei_model_build_walks_tsan", TSAN, [WALKS], extra=(ENTRY_AFGS1, ENTRY_SEI)), NWALKS)


def test_the_host_layer_does_not_name_the_new_launcher(tmp_path):
    """the link every older sanitizer suite makes -- the three host sources against the unchanged stub, which knows nothing of
    fw_sei_build_kernel -- still succeeds: only the new entry point's translation unit needs the new launcher, and it names no other"""
    main = tmp_path / "main.cpp"
    main.write_text('#include "%s"\nint main() { vfgs_hip_shutdown(); return 0; }\n' % (CSRC.parent.parent / "include" / "vfgs_hip.h"))
    exe, r = try_build(tmp_path, "host_only", PLAIN, [main])
    assert r.returncode == 0, r.stderr[-4000:]
    exe, r = try_build(tmp_path, "entry_without_launcher", PLAIN, [main], extra=(ENTRY_SEI,))
    assert r.returncode != 0 and "launch_fw_sei_build" in r.stderr and "launch_fw_models" not in r.stderr, r.stderr[-2000:]
