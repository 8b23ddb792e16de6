"""CPU: the generated FGC SEI messages of tests/test_gpu_models_from_sei.py::test_bytes_equal_the_capture_path cover what that test says
they cover, in every one of its parametrisations (tests/sei_model_util.py: facts read from the messages alone).  No GPU, no library."""
import pytest

import sei_model_util as G
from versatilefilmgrain_amd.fw import FgsSei

FORMATS = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "440": (1, 2)}


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_the_generated_list_covers_the_cases(depth, fmt):
    msgs = G.generated_list(FgsSei, G.list_seed(depth, *FORMATS[fmt]))
    assert len(msgs) == 40
    seen = set().union(*[G.facts(m) for m in msgs])
    assert not G.REQUIRED - seen, sorted(G.REQUIRED - seen)
    for m in msgs:      # what the call accepts: the stored shift in range, at most 256 intervals
        assert 2 <= m.log2_scale_factor - (1 if m.model_id else 0) <= 7
        assert all(m.num_intensity_intervals[c] <= 256 for c in range(3))


def test_the_generator_is_deterministic():
    a = G.generated_list(FgsSei, 7)
    b = G.generated_list(FgsSei, 7)
    assert [bytes(x) for x in a] == [bytes(y) for y in b]
