"""CPU: what every device-pointer entry of libvfgs_hip answers -- return code, error text, which of two refusals wins, the launch record,
the seed registers -- over the unchanged model of the HIP runtime tests/sanitize/hip_stub.cpp, compared byte for byte with a recording:
tests/sanitize_entries/entry_matrix.cpp, a stand-alone program built by tests/sanitize_build.py, prints
one line per call, and tests/golden/entry_matrix.txt is what it printed when it was written.  The recording is NOT regenerated when the
host layer is reshaped: a reshaped host layer answers every call of the matrix as before, or this test says which line moved."""
from sanitize_build import ASAN_UBSAN, ROOT, SAN, build, needs_gxx, run_asan_ubsan

DRIVER = SAN.parent / "sanitize_entries" / "entry_matrix.cpp"
GOLDEN = ROOT / "tests" / "golden" / "entry_matrix.txt"

pytestmark = needs_gxx


def test_every_entry_answers_the_matrix_as_recorded(tmp_path):
    r = run_asan_ubsan(build(tmp_path, "entry_matrix_asan", ASAN_UBSAN, [DRIVER]))
    got, want = r.stdout.splitlines(), GOLDEN.read_text().splitlines()
    moved = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not moved, f"line {moved[0] + 1} of {len(moved)} that moved:\n  recorded: {want[moved[0]]}\n  now:      {got[moved[0]]}"
    assert r.stdout == GOLDEN.read_text(), f"{len(got)} lines, recorded {len(want)}"
