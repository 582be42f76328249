"""pcr_pool_products_tm without a device: the symbol and the record layout, the refusals that come before the handle, the
properties of the scenarios that tests/test_gpu_products_tm.py relies on (computed with the CPU oracle), and the oracle held to
the reference on every duplex the new scenarios melt."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import reference_tape

import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


# The reference's answers to this file's calls, on a tape of its own (the format and proxies of tests/reference_tape.py):
#     PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_products_tm_host.py      # rewrites the file below
TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "products_tm_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"


@pytest.fixture(scope="module")
def _tapes():
    tapes = {}
    if os.path.exists(TAPE):
        with gzip.open(TAPE, "rt") as f:
            tapes = json.load(f)
    yield tapes
    if _RECORD:
        with gzip.GzipFile(TAPE, "wb", mtime=0) as g:
            g.write(reference_tape.canonical(tapes))


@pytest.fixture
def products_reference(request, oracle, _tapes):
    """The compiled reference where it was built; elsewhere its recorded answers, checked against the oracle's."""
    from oracle_lib import Reference
    test_id = "%s::%s" % (request.node.module.__name__, request.node.name)
    if Reference.available():
        if _RECORD:
            _tapes[test_id] = {}
            yield reference_tape.RecordingReference(Reference(), oracle, _tapes[test_id])
        else:
            yield Reference()
        return
    if test_id not in _tapes:
        pytest.fail("no recorded reference answers for %s (%s)" % (test_id, TAPE))
    replay = reference_tape.ReplayReference(test_id, oracle, _tapes[test_id])
    yield replay
    replay._finish()


def test_symbol_is_exported(lib):
    assert "pcr_pool_products_tm" in api.ABI_SYMBOLS
    assert hasattr(lib, "pcr_pool_products_tm"), "libpcramp_hip.so does not export pcr_pool_products_tm"
    assert api.PRODUCT_TM_DTYPE.itemsize == 48 and PC.PRODUCT_TM == api.PRODUCT_TM_DTYPE
    assert api.PRODUCT_TM_DTYPE.names[:8] == api.PRODUCT_DTYPE.names == PC.FIELDS8
    assert (api.PRODUCT_PLUS_NO_TM, api.PRODUCT_MINUS_NO_TM) == (PC.PLUS_NO_TM, PC.MINUS_NO_TM) == (1, 2)


def _call(lib, which, pool, template_strand=0.0, primer_strand=9e-7, salt=0.05, tm_floor=0.0, ids=True, args=True, out=None, cap=0):
    a = W.pairs_array(pool) if pool else None
    oid = np.zeros(max(2 * len(pool), 1), np.uint32)
    th = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    rc = lib.pcr_pool_products_tm(None, which, a.ctypes.data if a is not None else None, len(pool), 0.9, 80, 200,
                                  C.byref(th) if args else None, float(template_strand), float(tm_floor),
                                  oid.ctypes.data if ids else None, out, cap, None, None)
    return rc, api._err(lib)


def test_refusals_before_the_handle(lib, oracle):
    """pcr_site_tm's checks in its order, then the floor, then the handle: each call below is wrong in one thing and in the
    handle, and the message names the one thing; two things wrong name the earlier."""
    pair = (oracle.centered_word("ACGTTGCAAGCTTGCATGCA"), oracle.centered_word("TTGACCGTAGGCTAGCTAAC"))
    too = SC.too_degenerate_oligo(oracle)
    rc, msg = _call(lib, api.TARGET, [pair])
    assert rc == PCR_ERR_ARG and "null handle" in msg                       # every argument is fine: only the handle is missing
    rc, msg = _call(lib, 7, [pair], ids=False)
    assert rc == PCR_ERR_ARG and "unknown sequence set" in msg
    rc, msg = _call(lib, api.MULTIPLEX, [pair], ids=False)
    assert rc == PCR_ERR_ARG and "PCR_SET_MULTIPLEX" in msg
    rc, msg = _call(lib, api.TARGET, [pair], ids=False)
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair], args=False)
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair], cap=4)                          # cap without a buffer
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), cap=4)
    assert rc == PCR_ERR_ARG and "bad argument" in msg                       # ... comes before the pool's size
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), template_strand=-1e-9)
    assert rc == PCR_ERR_ARG and "PCR_POOL_MAX_PAIRS" in msg                 # ... which comes before the concentrations
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=-1e-9, salt=2.0)
    assert rc == PCR_ERR_ARG and "negative" in msg                           # ... which come before the salt
    rc, msg = _call(lib, api.TARGET, [pair], primer_strand=-9e-7)
    assert rc == PCR_ERR_ARG and "negative" in msg
    rc, msg = _call(lib, api.TARGET, [pair, (pair[0], too)], salt=2.0)
    assert rc == PCR_ERR_ARG and "salt" in msg                               # ... which comes before the oligos
    rc, msg = _call(lib, api.TARGET, [pair], salt=1e-7)
    assert rc == PCR_ERR_ARG and "salt" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=0.0, primer_strand=0.0)   # log(0) is no concentration
    assert rc == PCR_ERR_ARG and "zero" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=1e-7, primer_strand=0.0)  # the template alone is one
    assert rc == PCR_ERR_ARG and "null handle" in msg
    assert oracle.word_degeneracy(too) == 512
    rc, msg = _call(lib, api.TARGET, [pair, (pair[0], too)], tm_floor=float("nan"))
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg            # the oligos come before the floor
    rc, msg = _call(lib, api.TARGET, [(pair[0], (0, 0))])
    assert rc == PCR_ERR_ARG and "empty" in msg
    holed = W.word_from_slots([1 if k in (5, 6, 7, 9, 10, 11) else 0 for k in range(32)])
    rc, msg = _call(lib, api.TARGET, [(pair[0], holed)])
    assert rc == PCR_ERR_ARG and "hole" in msg
    rc, msg = _call(lib, api.TARGET, [(pair[0], oracle.centered_word("ACGTNNNNACGTACGTACG"))])   # 256 expansions pass
    assert rc == PCR_ERR_ARG and "null handle" in msg
    for bad in (float("nan"), float("inf"), float("-inf")):
        rc, msg = _call(lib, api.TARGET, [pair], tm_floor=bad)
        assert rc == PCR_ERR_ARG and "tm_floor" in msg
    rc, msg = _call(lib, api.TARGET, [pair], tm_floor=55.0)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, api.TARGET, [])                                     # n_pool = 0 still needs a handle
    assert rc == PCR_ERR_ARG and "null handle" in msg


# ------------------------------------------------------------------ what the GPU tests rely on, computed with the oracle
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_existing_scenarios_are_what_the_gpu_tests_need(oracle):
    ids, rec, sites, n_jobs = PC.all_products(oracle, "ids")
    assert len(rec) == 6 and rec["intended"].all() and len(np.unique(PC.min_tm(rec))) == 6
    assert ids == [0, 1, 2, 3, 4, 0] and 1 not in rec["sequence"].tolist()   # F of pair 0 is R of pair 2; sequence 1 is inactive
    ids, rec, sites, n_jobs = PC.all_products(oracle, "random")
    assert (len(rec), int(rec["intended"].sum()), len(sites), n_jobs) == (6647, 492, 1970, 3308)
    assert len(np.unique(PC.min_tm(rec))) >= 300 and PC.min_tm(rec).min() == 0.0 and PC.min_tm(rec).max() > 58.0
    assert len(set(zip(rec["plus_oligo"].tolist(), rec["minus_oligo"].tolist()))) > 50      # cross products of most combinations
    _, rec, _, _ = PC.all_products(oracle, "placement")
    assert len(rec) == 16 and not rec["intended"].any() and len(np.unique(PC.min_tm(rec))) == 7
    _, sub, _, _ = PC.all_products(oracle, "placement_words")
    assert len(sub) == 1 and set(map(tuple, PC.as_bits(sub))) <= set(map(tuple, PC.as_bits(rec)))
    _, rec, _, _ = PC.all_products(oracle, "ambiguity")
    assert len(rec) == 1 and rec[0]["intended"] == 1 and rec[0]["flags"] == PC.MINUS_NO_TM
    assert _bits(rec[0]["tm_minus"]) == 0 and rec[0]["tm_plus"] > 50.0
    for k in range(3):
        _, rec, _, n_jobs = PC.all_products(oracle, "expansions_%d" % k)
        assert len(rec) == 2 and rec["intended"].all() and n_jobs == 281
    tms = [PC.min_tm(PC.all_products(oracle, "expansions_%d" % k)[1]) for k in range(3)]
    assert len({tuple(_bits(t).tolist()) for t in tms}) == 3                 # the template concentration moves every Tm
    assert len(PC.all_products(oracle, "split")[1]) == 0                     # 220 bases apart: nothing at 80..200


def test_ladder(oracle):
    case = PC.scenario(oracle, "ladder")
    (f, r), = case["panel"]
    assert f != r and len(case["seqs"]) == 3
    ids, rec, sites, _ = PC.all_products(oracle, "ladder")
    assert ids == [0, 1]
    on0 = rec[rec["sequence"] == 0]
    combos = {(int(p["begin"]), int(p["end"])) for p in on0 if p["plus_oligo"] == 0 and p["minus_oligo"] == 1}
    assert combos >= {(a, b + 21) for a in PC.LADDER_PLUS for b in PC.LADDER_MINUS}            # all 25, R is a 22-mer
    assert len(rec) == 27 and rec["intended"].all() and not rec["flags"].any()
    m = PC.min_tm(rec)
    assert len(np.unique(m)) >= 6 and m.min() > 0
    weak, strong = rec[rec["sequence"] == 1], rec[rec["sequence"] == 2]
    assert len(weak) == 1 and len(strong) == 1
    assert PC.min_tm(weak)[0] == m.min() and PC.min_tm(strong)[0] == m.max() and m.min() < m.max()
    # a floor between them: different bits per sequence; the floors the GPU test uses move the count at every step
    mid = float(np.unique(m)[len(np.unique(m)) // 2])
    _, k, fr, rf = PC.expectation(oracle, "ladder", mid)
    assert fr.tolist() == [[0b101]] and rf.tolist() == [[0]] and 0 < len(k) < len(rec)
    assert PC.expectation(oracle, "ladder", 0.0)[2].tolist() == [[0b111]]
    counts = [len(PC.kept(rec, fl)) for fl in PC.floors_of(rec)]
    assert counts[0] == 27 and counts[1] < 27 and counts[-3] == 27 and counts[-2] == 0 and counts[-1] == 27
    assert all(counts[2 * i] > counts[2 * i + 1] for i in range(3))          # nextafter above a value drops it


def test_words(oracle):
    case = PC.scenario(oracle, "words")
    n = len(case["seqs"])
    assert n == PC.WORDS_N >= 130 and (n + 63) // 64 == 3
    ids, rec, sites, _ = PC.all_products(oracle, "words")
    assert ids == [0, 1, 2, 3, 4, 5] and rec["intended"].all()
    with_product = set(rec["sequence"].tolist())
    quiet = set(PC.WORDS_INACTIVE) | set(PC.WORDS_NO_SITE)
    assert with_product == set(range(n)) - quiet and {63, 64, 127, 128} <= with_product
    block = rec[rec["sequence"] == PC.WORDS_BLOCK]
    assert len(block) >= 64 and set(zip(block["plus_oligo"].tolist(), block["minus_oligo"].tolist())) == {(0, 1)}
    for i in set(range(n - 1)) - quiet:                                      # one product of pair i % 3 each
        mine = rec[rec["sequence"] == i]
        assert len(mine) == 1 and (mine[0]["plus_oligo"], mine[0]["minus_oligo"]) == (2 * (i % 3), 2 * (i % 3) + 1)
    for i in PC.WORDS_MUTATED:                                               # a substitution in the minus site: a lower tm_minus
        assert rec[rec["sequence"] == i][0]["tm_minus"] < rec[rec["sequence"] == i % 3][0]["tm_minus"] - 2
    _, _, fr, rf = PC.expectation(oracle, "words")
    assert not rf.any() and all(fr[i].any() for i in range(3)) and all((fr[:, w] != 0).any() for w in range(3))
    assert int(fr[0, 2]) >> (PC.WORDS_BLOCK - 128) & 1
    # the lowest min-Tm among pair 0's unmutated products as the floor: every one of them stays, the mutated ones go
    pair0 = rec[(rec["plus_oligo"] == 0) & ~np.isin(rec["sequence"], PC.WORDS_MUTATED)]
    floor = float(PC.min_tm(pair0).min())
    _, k, fr_f, _ = PC.expectation(oracle, "words", floor)
    assert 0 < len(k) < len(rec)
    dropped = [i for i in PC.WORDS_MUTATED if i % 3 == 0]
    assert dropped
    for i in dropped:
        assert (int(fr[0, i >> 6]) >> (i & 63)) & 1 and not (int(fr_f[0, i >> 6]) >> (i & 63)) & 1
    assert int(fr[0, 2]) == int(fr_f[0, 2]) and bin(int(fr[0, 0] ^ fr_f[0, 0])).count("1") + bin(int(fr[0, 1] ^ fr_f[0, 1])).count("1") == len(dropped)


def test_pairs(oracle):
    case = PC.scenario(oracle, "pairs")
    ids, rec, _, _ = PC.all_products(oracle, "pairs")
    assert ids == [0, 1, 2, 2, 0, 3, 0, 1, 1, 0]                             # (A, B), (C, C), (A, D), (A, B), (B, A)
    _, _, fr, rf = PC.expectation(oracle, "pairs")
    assert fr[0].tolist() == fr[3].tolist() and rf[0].tolist() == rf[3].tolist()          # the duplicated pair
    assert fr[1].tolist() == rf[1].tolist() and fr[1].any()                               # F = R
    assert fr[4].tolist() == rf[0].tolist() and rf[4].tolist() == fr[0].tolist()          # the exchanged pair
    assert fr[0].any() and rf[0].any() and fr[0].tolist() != rf[0].tolist()
    assert fr[2].any() and not rf[2].any() and fr[2].tolist() != fr[0].tolist()           # (A, D) shares A with (A, B)
    assert not ((fr | rf) >> np.uint64(4)).any()                                          # the last sequence has no product
    assert rec["intended"].all() and len(np.unique(PC.min_tm(rec))) >= 4


def test_split_variants(oracle):
    _, wide, _, _ = PC.all_products(oracle, "split_wide")
    _, inner, _, _ = PC.all_products(oracle, "split_inner")
    assert set(wide["sequence"].tolist()) == {0, 1} and set(inner["sequence"].tolist()) == {1}
    whole = wide[wide["sequence"] == 1]
    assert len(whole) == 1 and PC.as_bits(whole) == PC.as_bits(inner)
    assert (wide[wide["sequence"] == 0]["tm_plus"] < whole[0]["tm_plus"]).all()            # the words over the split: weaker sites


@pytest.mark.parametrize("name", PC.NEW_SCENARIOS)
def test_scenario_duplexes_oracle_equals_reference(oracle, products_reference, name):
    """Every duplex of the new scenarios: reference.heterodimer_full == oracle.heterodimer_full, bit for bit."""
    case = PC.scenario(oracle, name)
    jobs = set()
    SC.expectation(oracle, case, jobs=jobs)
    assert jobs, name
    for q, t, ca, cb in sorted(jobs):
        want = products_reference.heterodimer_full(q, t, SC.SALT, ca, cb)
        got = oracle.heterodimer_full(q, t, SC.SALT, ca, cb)
        assert want.view(np.uint32).tolist() == got.view(np.uint32).tolist(), (q, t, ca, cb)
