"""pcr_site_tm without a device: the symbol, the refusals that come before the handle, and the oracle held to the reference on
every (expansion, target) duplex the GPU scenarios of tests/test_gpu_site_tm.py melt -- templates with dangling flanks and
several mismatches, which test_heterodimer_random meets only by chance."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import reference_tape

import site_tm_cases as SC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def lib():
    """The library under test; every test of this file is about a call it must export."""
    L = api.load_library()
    assert hasattr(L, "pcr_site_tm"), "libpcramp_hip.so does not export pcr_site_tm"
    return L


# The reference's answers to this file's calls, kept beside the suite's tape (tests/golden/reference_calls.json.gz, which belongs
# to tests/test_oracle_vs_reference.py and stays as it is) in the same format and through the same proxies:
#     PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_site_tm_host.py      # rewrites the file below
SITE_TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "site_tm_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"


@pytest.fixture(scope="module")
def _site_tapes():
    tapes = {}
    if os.path.exists(SITE_TAPE):
        with gzip.open(SITE_TAPE, "rt") as f:
            tapes = json.load(f)
    yield tapes
    if _RECORD:
        with gzip.GzipFile(SITE_TAPE, "wb", mtime=0) as g:
            g.write(reference_tape.canonical(tapes))


@pytest.fixture
def site_reference(request, oracle, _site_tapes):
    """The compiled reference where it was built; elsewhere its recorded answers, checked against the oracle's (as the
    suite's `reference` fixture, on this file's own tape)."""
    from oracle_lib import Reference
    test_id = "%s::%s" % (request.node.module.__name__, request.node.name)
    if Reference.available():
        if _RECORD:
            _site_tapes[test_id] = {}
            yield reference_tape.RecordingReference(Reference(), oracle, _site_tapes[test_id])
        else:
            yield Reference()
        return
    if test_id not in _site_tapes:
        pytest.fail("no recorded reference answers for %s (%s)" % (test_id, SITE_TAPE))
    replay = reference_tape.ReplayReference(test_id, oracle, _site_tapes[test_id])
    yield replay
    replay._finish()


def _call(lib, which, panel, template_strand=0.0, primer_strand=9e-7, salt=0.05, ids=True, out=None, cap=0):
    a = W.pairs_array(panel) if panel else None
    oid = np.zeros(max(2 * len(panel), 1), np.uint32)
    args = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    rc = lib.pcr_site_tm(None, which, a.ctypes.data if a is not None else None, len(panel), 0.9, C.byref(args),
                         float(template_strand), oid.ctypes.data if ids else None, out, cap)
    return rc, api._err(lib)


def test_symbol_is_exported(lib):
    assert "pcr_site_tm" in api.ABI_SYMBOLS
    assert hasattr(lib, "pcr_site_tm")
    assert api.SITE_DTYPE.itemsize == 48 and SC.SITE == api.SITE_DTYPE


def test_refusals_before_the_handle(lib, oracle):
    pair = (oracle.centered_word("ACGTTGCAAGCTTGCATGCA"), oracle.centered_word("TTGACCGTAGGCTAGCTAAC"))
    rc, msg = _call(lib, api.TARGET, [pair])
    assert rc == PCR_ERR_ARG and "null handle" in msg                       # every argument is fine: only the handle is missing
    rc, msg = _call(lib, api.MULTIPLEX, [pair])
    assert rc == PCR_ERR_ARG and "PCR_SET_MULTIPLEX" in msg
    rc, msg = _call(lib, 7, [pair])
    assert rc == PCR_ERR_ARG and "unknown sequence set" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=-1e-9)
    assert rc == PCR_ERR_ARG and "negative" in msg
    rc, msg = _call(lib, api.TARGET, [pair], primer_strand=-9e-7)
    assert rc == PCR_ERR_ARG and "negative" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=0.0, primer_strand=0.0)   # log(0) is no concentration
    assert rc == PCR_ERR_ARG and "zero" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=1e-7, primer_strand=0.0)  # the template alone is one
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, api.TARGET, [pair], ids=False)
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair], cap=4)                          # cap without a buffer
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1))
    assert rc == PCR_ERR_ARG and "PCR_POOL_MAX_PAIRS" in msg
    too = SC.too_degenerate_oligo(oracle)
    assert oracle.word_degeneracy(too) == 512
    rc, msg = _call(lib, api.TARGET, [pair, (pair[0], too)])
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg
    assert api.SITE_MAX_EXPANSIONS == 256
    rc, msg = _call(lib, api.TARGET, [(pair[0], oracle.centered_word("ACGTNNNNACGTACGTACG"))])   # 256 expansions pass
    assert rc == PCR_ERR_ARG and "null handle" in msg


def test_expansion_order_is_word_begin_next(oracle):
    """The expectation spells expansions in oracle.word_expand's order; its first and last are all-lowest / all-highest."""
    w = oracle.centered_word("ACRTNGYA")
    exps = [SC.spell(SC.slots_of(x)) for x in oracle.word_expand(w)]
    assert len(exps) == 16 and len(set(exps)) == 16
    assert exps[0] == "ACATAGCA" and exps[-1] == "ACGTTGTA"
    # three-fold codes: the centred 8-mer lies in slots 12 .. 19, so B (slot 14) turns fastest, then H (slot 18), then R (slot 16)
    w = oracle.centered_word("ACBTRGHA")
    exps = [SC.spell(SC.slots_of(x)) for x in oracle.word_expand(w)]
    assert len(exps) == 18 and len(set(exps)) == 18
    assert exps[0] == "ACCTAGAA" and exps[-1] == "ACTTGGTA"
    assert exps[:4] == ["ACCTAGAA", "ACGTAGAA", "ACTTAGAA", "ACCTAGCA"] and exps[9] == "ACCTGGAA"


@pytest.mark.parametrize("name", SC.SCENARIO_NAMES)
def test_scenario_duplexes_oracle_equals_reference(oracle, site_reference, name):
    """Every duplex of the scenario: reference.heterodimer_full == oracle.heterodimer_full, bit for bit."""
    case = SC.gpu_scenarios(oracle)[name]
    jobs = set()
    SC.expectation(oracle, case, jobs=jobs)
    assert jobs, name
    for q, t, ca, cb in sorted(jobs):
        want = site_reference.heterodimer_full(q, t, SC.SALT, ca, cb)
        got = oracle.heterodimer_full(q, t, SC.SALT, ca, cb)
        assert want.view(np.uint32).tolist() == got.view(np.uint32).tolist(), (q, t, ca, cb)
