import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle_lib import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def _reference_calls():
    """The recorded answers of the reference (tests/reference_tape.py); rewritten at the end of a
    PCRAMP_RECORD_REFERENCE=1 run."""
    import reference_tape
    tapes = reference_tape.load_tapes()
    yield tapes
    if os.environ.get("PCRAMP_RECORD_REFERENCE") == "1":
        reference_tape.save_tapes(tapes)


@pytest.fixture
def reference(request, oracle, _reference_calls):
    """The real reference behind oracle/ref_harness.cpp where oracle/Makefile built it; elsewhere its recorded answers,
    checked against the oracle's (tests/reference_tape.py)."""
    import reference_tape
    from oracle_lib import Reference
    test_id = "%s::%s" % (request.node.module.__name__, request.node.name)
    if Reference.available():
        if os.environ.get("PCRAMP_RECORD_REFERENCE") == "1":
            _reference_calls[test_id] = {}
            yield reference_tape.RecordingReference(Reference(), oracle, _reference_calls[test_id])
        else:
            yield Reference()
        return
    if test_id not in _reference_calls:
        pytest.fail("no recorded reference answers for %s (tests/golden/reference_calls.json.gz)" % test_id)
    replay = reference_tape.ReplayReference(test_id, oracle, _reference_calls[test_id])
    yield replay
    replay._finish()
