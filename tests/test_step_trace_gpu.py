"""Same kernels, same arguments: every step of tests/native_trace.py's matrix launches exactly the
native ops, with exactly the scalar arguments and tensor shapes / dtypes, that
tests/golden/step_traces.json recorded before the streamed-weight dispatch was folded into one
(``python -m tests.native_trace --record`` regenerates the file; this test never writes it)."""
import json

import pytest

from docqa_amd import ops
from tests import native_trace as nt

pytestmark = pytest.mark.gpu

_MODEL = {}      # one resident model at a time: CASES are grouped by weights


@pytest.fixture(scope="module")
def golden():
    assert ops.load_native(build_if_missing=True)
    g = nt.load_golden()
    assert sorted(g) == sorted(nt.CASES)
    yield g
    _MODEL.clear()


@pytest.mark.parametrize("case", nt.CASES)
def test_step_launches_the_recorded_native_ops(golden, case):
    weights = case.split("-")[0]
    if weights not in _MODEL:
        _MODEL.clear()
        _MODEL[weights] = nt.build_model(weights)
    trace = json.loads(json.dumps(nt.run_case(_MODEL[weights], case)))
    want = golden[case]
    assert [c[0] for c in trace] == [c[0] for c in want]
    for i, (got, exp) in enumerate(zip(trace, want)):
        assert got == exp, (i, got, exp)
