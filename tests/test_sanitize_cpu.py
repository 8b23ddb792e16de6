"""CPU: the host layer of libvfgs_hip under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer.

3,300 lines of C++ (vfgs_host.cpp, vfgs_fw_host.cpp, vfgs_cfg_host.cpp) hold stream rings, pinned staging buffers, worker threads
and a look-ahead that reads caller memory ahead of the line it was handed.  GPU sanitizers do not exist on the pool, so the host
sources are compiled with g++ and the sanitizers against tests/sanitize/hip_stub.cpp -- a model of the HIP runtime with deferred
stream execution, in which every copy and every "kernel launch" touches exactly the bytes the real one would -- and driven by
tests/sanitize/host_walks.cpp through the walks of tests/test_gpu_parity.py (lines in order, late edits, repeats, skips, setters
in the middle of a frame, the ring of stripes, promised frame heights over buffers of different pitches), the host stripe / frame
pipelines, replicas on several devices, batches, parts, lists, overlap regions, refusals.  The reference declares such a switch
and never wires it (/root/reference/CMakeLists.txt:25-29).  Values are the GPU suite's business; here the sanitizers check
addresses, lifetimes and threads, and the walks check that what a call hands back is what the (zero-grain) stub kernel made of it.
"""
import pytest

import sanitize_build as S
from sanitize_build import ASAN_UBSAN, CSRC, SAN, STUB, TSAN, build, check_asan_ubsan, check_tsan, needs_gxx, run

WALKS = SAN / "host_walks.cpp"
NWALKS = 10

pytestmark = needs_gxx


def test_host_layer_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    check_asan_ubsan(build(tmp_path, "walks_asan", ASAN_UBSAN, [WALKS]), NWALKS)


def test_host_layer_under_thread_sanitizer(tmp_path):
    check_tsan(build(tmp_path, "walks_tsan", TSAN, [WALKS]), NWALKS)


def overflow_is_seen(tmp_path, walks, walk, allocator=None):
    """a stub kernel that walks one row past every plane, built only with -fsanitize=address, under one walk of one program: reported, and
    (allocator given) the block it ran past is one that this type of tests/sanitize/walks.h allocated"""
    bad = tmp_path / "hip_stub_bad.cpp"
    src = STUB.read_text()
    assert "r < row_first + pd.nrows; r++)" in src
    bad.write_text(src.replace("r < row_first + pd.nrows; r++)", "r < row_first + pd.nrows + 1; r++)")
                   .replace('"../../versatilefilmgrain_amd/csrc/', f'"{CSRC}/'))
    obj = tmp_path / "hip_stub_bad.o"
    r = S.gxx(("-O1", "-fsanitize=address"), "-c", bad, "-o", obj)
    assert r.returncode == 0, r.stderr[-4000:]
    exe = build(tmp_path, "walks_bad", ASAN_UBSAN, [obj, SAN.parent / walks], stub=False)
    r = run(exe, {}, walk)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-3000:]
    if allocator:
        allocated_by = r.stderr.split("allocated by", 1)[1].split("SUMMARY", 1)[0]
        assert f"{allocator}::{allocator}" in allocated_by, allocated_by[:3000]


def test_the_harness_sees_a_kernel_that_touches_one_row_too_many(tmp_path):
    """The check of the checker: the same build with a stub kernel that walks one row past every plane must be reported."""
    overflow_is_seen(tmp_path, "sanitize/host_walks.cpp", "device_entries")


@pytest.mark.parametrize("walks,walk,allocator", [("sanitize/picture_walks.cpp", "sp_pool", "DevSpPic"), ("sanitize_seeded/seeded_walks.cpp", "entries", "DevFrame")],
                         ids=["picture_walks", "seeded_walks"])
def test_the_harness_sees_a_kernel_that_touches_one_row_too_many_in_the_shared_pictures(tmp_path, walks, walk, allocator):
    """... and so through the picture types of tests/sanitize/walks.h, on which "exactly as large as the contract says" rests for every other
    program: the block the kernel ran past was allocated by the shared semi-planar picture's device copy (tests/sanitize/picture_walks.cpp,
    whose first launch runs on an SpPool; the walks of sp_walks.cpp all launch on planar_regs()' scratch planes first, where the sanitizer
    would stop), and by the shared planar device frame (the first launch of seeded_walks' `entries`)."""
    overflow_is_seen(tmp_path, walks, walk, allocator)


def test_the_picture_walk_is_clean_over_the_unchanged_stub(tmp_path):
    check_asan_ubsan(build(tmp_path, "picture_walks_asan", ASAN_UBSAN, [SAN / "picture_walks.cpp"]), 1)
