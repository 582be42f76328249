"""pcr_site_variants without a device: the symbol and the record, the refusals that come before the handle, the host helpers on
hand-made records, and the oracle held to the reference on every duplex the scenarios of site_variant_cases add to those of
site_tm_cases (whose duplexes tests/test_site_tm_host.py holds)."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import reference_tape

import site_tm_cases as SC
import site_variant_cases as VC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def lib():
    """The library under test; every test of this file is about a call it must export."""
    L = api.load_library()
    assert hasattr(L, "pcr_site_variants"), "libpcramp_hip.so does not export pcr_site_variants"
    return L


# The reference's answers to this file's calls, on a tape of its own in the format of tests/golden/reference_calls.json.gz:
#     PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_site_variants_host.py      # rewrites the file below
VARIANT_TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "site_variants_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"


@pytest.fixture(scope="module")
def _variant_tapes():
    tapes = {}
    if os.path.exists(VARIANT_TAPE):
        with gzip.open(VARIANT_TAPE, "rt") as f:
            tapes = json.load(f)
    yield tapes
    if _RECORD:
        with gzip.GzipFile(VARIANT_TAPE, "wb", mtime=0) as g:
            g.write(reference_tape.canonical(tapes))


@pytest.fixture
def variant_reference(request, oracle, _variant_tapes):
    """The compiled reference where it was built; elsewhere its recorded answers, checked against the oracle's (as the
    suite's `reference` fixture, on this file's own tape)."""
    from oracle_lib import Reference
    test_id = "%s::%s" % (request.node.module.__name__, request.node.name)
    if Reference.available():
        if _RECORD:
            _variant_tapes[test_id] = {}
            yield reference_tape.RecordingReference(Reference(), oracle, _variant_tapes[test_id])
        else:
            yield Reference()
        return
    if test_id not in _variant_tapes:
        pytest.fail("no recorded reference answers for %s (%s)" % (test_id, VARIANT_TAPE))
    replay = reference_tape.ReplayReference(test_id, oracle, _variant_tapes[test_id])
    yield replay
    replay._finish()


def _call(lib, which, panel, template_strand=0.0, primer_strand=9e-7, salt=0.05, ids=True, out=None, cap=0, args=True,
          site_variant=None, site_cap=0):
    a = W.pairs_array(panel) if panel else None
    oid = np.zeros(max(2 * len(panel), 1), np.uint32)
    targs = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    rc = lib.pcr_site_variants(None, which, a.ctypes.data if a is not None else None, len(panel), 0.9,
                               C.byref(targs) if args else None, float(template_strand), oid.ctypes.data if ids else None,
                               out, cap, site_variant, site_cap, None)
    return rc, api._err(lib)


def test_symbol_and_record():
    assert "pcr_site_variants" in api.ABI_SYMBOLS
    assert hasattr(api.load_library(), "pcr_site_variants")
    assert api.SITE_VARIANT_DTYPE.itemsize == 80 and VC.VARIANT == api.SITE_VARIANT_DTYPE
    assert api.SITE_VARIANT_DTYPE.fields["word"][0].shape == (2,)
    assert api.SITE_VARIANT_DTYPE.fields["tm_max"][1] == 64


def test_refusals_before_the_handle(lib, oracle):
    """pcr_site_tm's refusals in its order, with args == NULL legal; then the site map's; then the handle."""
    pair = (oracle.centered_word("ACGTTGCAAGCTTGCATGCA"), oracle.centered_word("TTGACCGTAGGCTAGCTAAC"))
    bad_oligo = (pair[0], SC.too_degenerate_oligo(oracle))
    buf = np.zeros(4, np.uint32)
    rc, msg = _call(lib, api.TARGET, [pair])
    assert rc == PCR_ERR_ARG and "null handle" in msg                       # every argument is fine: only the handle is missing
    rc, msg = _call(lib, api.TARGET, [pair], args=False)
    assert rc == PCR_ERR_ARG and "null handle" in msg                       # ... and so without thermodynamics
    rc, msg = _call(lib, 7, [pair], ids=False, salt=2.0)                    # the set comes first
    assert rc == PCR_ERR_ARG and "unknown sequence set" in msg
    rc, msg = _call(lib, api.MULTIPLEX, [pair], ids=False, salt=2.0)
    assert rc == PCR_ERR_ARG and "PCR_SET_MULTIPLEX" in msg
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), ids=False, salt=2.0)   # null pointers before the size
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair], cap=4, salt=2.0)               # cap without a buffer
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), template_strand=-1e-9)   # the size before the numbers
    assert rc == PCR_ERR_ARG and "PCR_POOL_MAX_PAIRS" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=-1e-9, salt=2.0)   # concentrations before salt
    assert rc == PCR_ERR_ARG and "negative" in msg
    rc, msg = _call(lib, api.TARGET, [pair], primer_strand=-9e-7)
    assert rc == PCR_ERR_ARG and "negative" in msg
    rc, msg = _call(lib, api.TARGET, [pair, bad_oligo], salt=2.0)           # salt before the oligos
    assert rc == PCR_ERR_ARG and "salt" in msg
    rc, msg = _call(lib, api.TARGET, [pair, bad_oligo], site_cap=4)         # the oligos before the site map
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=0.0, primer_strand=0.0, site_cap=4)   # log(0) is no concentration
    assert rc == PCR_ERR_ARG and "zero" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=1e-7, primer_strand=0.0)   # the template alone is one
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, api.TARGET, [pair], site_cap=4)                    # site_cap without a buffer
    assert rc == PCR_ERR_ARG and "site_variant" in msg
    rc, msg = _call(lib, api.TARGET, [pair], site_cap=4, site_variant=buf.ctypes.data)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    # without thermodynamics the numbers are not read; the oligos still are
    rc, msg = _call(lib, api.TARGET, [pair], args=False, template_strand=-1.0)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, api.TARGET, [pair, bad_oligo], args=False)
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg
    rc, msg = _call(lib, api.TARGET, [(pair[0], (0, 0))], args=False)
    assert rc == PCR_ERR_ARG and "empty" in msg
    rc, msg = _call(lib, api.TARGET, [], args=False)                        # an empty panel needs no pointers
    assert rc == PCR_ERR_ARG and "null handle" in msg


# ------------------------------------------------------------------ host helpers, on hand-made records
def _slots(text, start):
    sl = [0] * 32
    for i, ch in enumerate(text):
        sl[start + i] = W._CODE[ch]
    return sl


def _record(word, oligo, sites, sequences, tm_max=0.0, tm_min=0.0, dH=0.0, dS=0.0, flags=0, first=(0, 0, 1), matches=8):
    r = np.zeros(1, api.SITE_VARIANT_DTYPE)
    r["word"], r["oligo"], r["sites"], r["sequences"], r["flags"], r["matches"] = word, oligo, sites, sequences, flags, matches
    r["first_sequence"], r["first_loc5"], r["first_strand"] = first
    r["tm_max"], r["tm_min"], r["dH"], r["dS"] = tm_max, tm_min, dH, dS
    r["n_expansions"], r["clamp3"], r["clamp5"] = 1, 8, 8
    return r


def test_variant_texts():
    rec = np.concatenate([_record(W.word_from_slots(_slots("TACGTACGTC", 11)), 0, 1, 1),
                          _record(W.word_from_slots(_slots("ACRTNCGT", 12)), 0, 1, 1),
                          _record(W.word_from_slots(_slots("GA", 0)), 0, 1, 1),
                          _record(W.word_from_slots(_slots("CC", 30)), 0, 1, 1)])
    assert api.variant_texts(rec) == ["TACGTACGTC", "ACRTNCGT", "GA", "CC"]
    assert api.variant_texts(rec[:0]) == []


def test_merge_variant_flanks():
    oligo = W.centered_word(W.codes_from_text("ACGTACGT"))                   # slots 12 .. 19
    other = W.centered_word(W.codes_from_text("TTGACCGT"))
    word = lambda text: W.word_from_slots(_slots(text, 11))                 # 5' flank, the eight bases, 3' flank
    rec = np.concatenate([
        _record(word("TACGTACGTC"), 0, 10, 7, 50.0, 49.0, -60.0, -0.16, first=(2, 30, 1)),
        _record(word("GACGTACGTC"), 0, 4, 4, 51.5, 51.0, -61.0, -0.17, first=(1, 80, 2)),     # another 5' flank: the warmer one
        _record(word("TACGTACGTA"), 0, 2, 2, 48.0, 47.5, -59.0, -0.15, first=(1, 90, 1)),     # another 3' flank
        _record(word("TACGTACGAC"), 0, 3, 3, 40.0, 39.0, -50.0, -0.14, first=(5, 10, 1), matches=7),   # another base inside: stays
        _record(word("RACGTACGAC"), 0, 1, 1, flags=api.SITE_NO_TM, first=(0, 12, 1), matches=7),      # ... and its unmelted flank variant
        _record(word("TACGTACGTC"), 1, 6, 6, 30.0, 30.0, -40.0, -0.12, first=(0, 5, 2), matches=4),   # the same word under another oligo
        _record(word("NACGTACGTC"), 1, 1, 1, flags=api.SITE_NO_TM, first=(9, 5, 2), matches=4)])
    site_variant = np.repeat(np.arange(7), rec["sites"]).astype(np.uint32)
    #                sequences of the sites, variant by variant: variants 0 and 1 share sequences 1 and 2; 0 and 2 share 1
    sequences = np.array([1, 1, 1, 2, 2, 3, 4, 5, 6, 7] + [1, 2, 8, 9] + [1, 10] + [5, 6, 7] + [0] + [0, 1, 2, 3, 4, 5] + [9])
    for oligos in ([oligo, other], [(oligo, other)], [(oligo, oligo), (oligo, other)]):
        got = api.merge_variant_flanks(rec, oligos, site_variant, sequences)
        assert len(got) == 3
        a, b, c = got
        inner = W.word_from_slots(_slots("ACGTACGT", 12))
        assert (int(a["word"][0]), int(a["word"][1])) == inner and a["oligo"] == 0
        assert (a["sites"], a["sequences"]) == (16, 10)                     # 7 + 4 + 2 counted 13: three are shared
        assert (a["tm_max"], a["dH"], a["dS"], a["tm_min"]) == tuple(np.float32(v) for v in (51.5, -61.0, -0.17, 47.5))
        assert (a["first_sequence"], a["first_loc5"], a["first_strand"]) == (1, 80, 2) and a["flags"] == 0
        assert (int(b["word"][0]), int(b["word"][1])) == W.word_from_slots(_slots("ACGTACGA", 12))
        assert (b["sites"], b["sequences"], b["matches"], b["flags"]) == (4, 4, 7, 0)   # the melted member's numbers
        assert (b["tm_max"], b["tm_min"], b["first_sequence"]) == (np.float32(40.0), np.float32(39.0), 0)
        assert (c["oligo"], c["sites"], c["sequences"], c["flags"]) == (1, 7, 7, 0)
        assert (int(c["word"][0]), int(c["word"][1])) == inner
    # the same sequence column out of site records; and without the map: the largest member's count, a lower bound
    sites = np.zeros(len(sequences), api.SITE_DTYPE)
    sites["sequence"] = sequences
    assert api.merge_variant_flanks(rec, [oligo, other], site_variant, sites).tobytes() == got.tobytes()
    loose = api.merge_variant_flanks(rec, [oligo, other])
    assert loose["sequences"].tolist() == [7, 3, 6] and loose["sites"].tolist() == [16, 4, 7]
    # nothing melted at all: the flag stays
    only = api.merge_variant_flanks(rec[4:5], [oligo, other])
    assert len(only) == 1 and only[0]["flags"] == api.SITE_NO_TM and only[0]["tm_max"] == 0.0
    assert len(api.merge_variant_flanks(rec[:0], [oligo, other])) == 0


# ------------------------------------------------------------------ the expectation itself, and the oracle behind it
def test_conserved_case_by_hand(oracle):
    """The classes of the conserved scenario as its docstring states them, from the expectation alone."""
    case = VC.conserved_case(oracle)
    ids, want, site_map, n_jobs = VC.expectation(oracle, case)
    assert ids == [0, 0]
    n_large = VC.CONSERVED_EXACT + 2
    assert want["sequences"].tolist() == [n_large, VC.CONSERVED_3P, VC.CONSERVED_FLANK, VC.CONSERVED_5P2]
    assert want["sites"].tolist() == [n_large + 1, VC.CONSERVED_3P, VC.CONSERVED_FLANK, VC.CONSERVED_5P2]
    assert want["matches"].tolist() == [20, 19, 20, 18]
    assert want["mismatch_mask"].tolist() == [0, 1 << 19, 0, 3]
    assert want["clamp3"].tolist() == [20, 0, 20, 18] and want["clamp5"].tolist() == [20, 19, 20, 0]
    assert n_jobs == 4 and len(site_map) == int(want["sites"].sum())
    assert np.bincount(site_map).tolist() == want["sites"].tolist()
    text = api.variant_texts(want)
    assert text[0][1:-1] == text[2][1:-1] and text[0][0] != text[2][0] and text[0][-1] == text[2][-1]
    assert want[0]["tm_max"] != want[2]["tm_max"]                           # the flank base is in the duplex (a dangling end)
    assert want[0]["tm_max"] > want[1]["tm_max"] and want[0]["tm_max"] > want[3]["tm_max"]


def test_expectation_agrees_with_the_site_records(oracle):
    """Joined through the site map, a variant carries what site_tm_cases expects for each of its sites, bit for bit."""
    for name in ("ids", "ambiguity", "split", "expansions_1", "zero_tie"):
        case = SC.gpu_scenarios(oracle)[name]
        ids, sites, jobs_sites = SC.expectation(oracle, case)
        vids, want, site_map, n_jobs = VC.expectation(oracle, case)
        assert vids == ids and len(site_map) == len(sites)
        assert n_jobs == int(want["n_expansions"].sum()) <= jobs_sites
        for s, v in zip(sites, site_map):
            r = want[v]
            for f in ("oligo", "matches", "n_expansions", "flags"):
                assert s[f] == r[f], (name, f)
            for f in ("tm_max", "tm_min", "dH", "dS"):
                assert np.float32(s[f]).view(np.uint32) == np.float32(r[f]).view(np.uint32), (name, f)


@pytest.mark.parametrize("name", VC.NEW_SCENARIO_NAMES)
def test_scenario_duplexes_oracle_equals_reference(oracle, variant_reference, name):
    """Every duplex of the scenario: reference.heterodimer_full == oracle.heterodimer_full, bit for bit."""
    case = VC.new_scenarios(oracle)[name]
    jobs = set()
    VC.expectation(oracle, case, jobs=jobs)
    SC.expectation(oracle, case, jobs=jobs)                                  # (the same duplexes: the GPU test joins the two calls)
    assert jobs, name
    for q, t, ca, cb in sorted(jobs):
        want = variant_reference.heterodimer_full(q, t, SC.SALT, ca, cb)
        got = oracle.heterodimer_full(q, t, SC.SALT, ca, cb)
        assert want.view(np.uint32).tolist() == got.view(np.uint32).tolist(), (q, t, ca, cb)
