"""pcr_pool_dimers without a device: the symbol and its record, every refusal that comes before the handle (in the order the
header lists them), and the oracle held to the reference on every duplex the scenarios of tests/test_gpu_pool_dimers.py
compare cell by cell -- heterodimers in both orders and homodimers, which test_heterodimer_random meets only by chance."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import reference_tape

import pool_dimer_cases as PC
from pcramp_amd import api, words as W

PCR_ERR_ARG, PCR_ERR_CAPACITY = -1, -4


@pytest.fixture(scope="module", autouse=True)
def lib():
    """The library under test; every test of this file is about a call it must export."""
    L = api.load_library()
    assert hasattr(L, "pcr_pool_dimers"), "libpcramp_hip.so does not export pcr_pool_dimers"
    return L


# The reference's answers to this file's calls, on a tape of its own (format and proxies of tests/reference_tape.py, as
# tests/test_site_tm_host.py keeps its tape):
#     PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_pool_dimers_host.py      # rewrites the file below
DIMER_TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_dimers_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"


@pytest.fixture(scope="module")
def _dimer_tapes():
    tapes = {}
    if os.path.exists(DIMER_TAPE):
        with gzip.open(DIMER_TAPE, "rt") as f:
            tapes = json.load(f)
    yield tapes
    if _RECORD:
        with gzip.GzipFile(DIMER_TAPE, "wb", mtime=0) as g:
            g.write(reference_tape.canonical(tapes))


@pytest.fixture
def dimer_reference(request, oracle, _dimer_tapes):
    """The compiled reference where it was built; elsewhere its recorded answers, checked against the oracle's."""
    from oracle_lib import Reference
    test_id = "%s::%s" % (request.node.module.__name__, request.node.name)
    if Reference.available():
        if _RECORD:
            _dimer_tapes[test_id] = {}
            yield reference_tape.RecordingReference(Reference(), oracle, _dimer_tapes[test_id])
        else:
            yield Reference()
        return
    if test_id not in _dimer_tapes:
        pytest.fail("no recorded reference answers for %s (%s)" % (test_id, DIMER_TAPE))
    replay = reference_tape.ReplayReference(test_id, oracle, _dimer_tapes[test_id])
    yield replay
    replay._finish()


def _call(lib, pool, salt=0.05, primer_strand=9e-7, rule=PC.POOL, tm_floor=0.0, args=True, ids=True, pairs=True, out=None, cap=0):
    a = W.pairs_array(pool) if pool else None
    oid = np.zeros(max(2 * len(pool), 1), np.uint32)
    ta = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    rc = lib.pcr_pool_dimers(None, a.ctypes.data if (a is not None and pairs) else None, len(pool), C.byref(ta) if args else None,
                             rule, tm_floor, oid.ctypes.data if ids else None, out, cap)
    return rc, api._err(lib)


def test_symbol_record_and_constants(lib):
    assert "pcr_pool_dimers" in api.ABI_SYMBOLS and hasattr(lib, "pcr_pool_dimers")
    assert api.POOL_DIMER_DTYPE.itemsize == 40 and PC.DIMER == api.POOL_DIMER_DTYPE
    assert (api.DIMER_RULE_POOL, api.DIMER_RULE_ASSAY, api.DIMER_HOMO) == (PC.POOL, PC.ASSAY, PC.HOMO) == (0, 1, 1)
    hdr = open(os.path.join(os.path.dirname(api.library_path()), "..", "include", "pcramp_hip.h")).read()
    assert "#define PCR_DIMER_RULE_POOL  0" in hdr and "#define PCR_DIMER_RULE_ASSAY 1" in hdr and "#define PCR_DIMER_HOMO 1u" in hdr
    inc = open(os.path.join(os.path.dirname(api.library_path()), "csrc", "pcr_pool_dimers.inc")).read()
    assert api.POOL_DIMER_BATCH_JOBS >= 65536
    assert "POOL_DIMER_BATCH_JOBS = 1u << %d;" % (api.POOL_DIMER_BATCH_JOBS.bit_length() - 1) in inc
    assert api.POOL_DIMER_BATCH_JOBS == 1 << (api.POOL_DIMER_BATCH_JOBS.bit_length() - 1)
    assert hasattr(api.Screener, "pool_dimers") and hasattr(api.Screener, "dimer_matrix")


def test_dimer_matrix():
    rec = np.zeros(3, api.POOL_DIMER_DTYPE)
    rec["query_oligo"], rec["target_oligo"] = [0, 2, 1], [1, 2, 0]
    rec["tm_max"], rec["dH"] = [41.5, 12.25, 40.0], [-50.0, -20.0, -49.0]
    m = api.Screener.dimer_matrix(rec, 3)
    assert m.dtype == np.float32 and m.shape == (3, 3)
    assert m.tolist() == [[0.0, 41.5, 0.0], [40.0, 0.0, 0.0], [0.0, 0.0, 12.25]]
    assert api.Screener.dimer_matrix(rec, 3, "dH")[1, 0] == -49.0


def test_refusals_before_the_handle(lib, oracle):
    w = oracle.centered_word
    pair = (w("ACGTTGCAAGCTTGCATGCA"), w("TTGACCGTAGGCTAGCTAAC"))
    buf = np.zeros(4, api.POOL_DIMER_DTYPE)
    for rule in (PC.POOL, PC.ASSAY):
        rc, msg = _call(lib, [pair], rule=rule)
        assert rc == PCR_ERR_ARG and "null handle" in msg                   # every argument is fine: only the handle is missing
    rc, msg = _call(lib, [pair], out=buf.ctypes.data, cap=4, tm_floor=35.0)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    # null pointers; cap without out
    for kw in (dict(args=False), dict(ids=False), dict(pairs=False), dict(cap=4)):
        rc, msg = _call(lib, [pair], **kw)
        assert rc == PCR_ERR_ARG and "bad argument" in msg, kw
    # ... which come before everything else
    rc, msg = _call(lib, [pair] * (api.POOL_MAX_PAIRS + 1), cap=4, rule=9, salt=2.0)
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    # n_pool, then the rule, then primer_strand, then salt, then the oligos, then the capacity
    rc, msg = _call(lib, [pair] * (api.POOL_MAX_PAIRS + 1), rule=9, primer_strand=0.0, salt=2.0)
    assert rc == PCR_ERR_ARG and "PCR_POOL_MAX_PAIRS" in msg
    hole = (int(pair[0][0]) & ~(0xF << 8), int(pair[0][1]))                 # slot 13 emptied: a hole between the ends
    assert oracle.word_size(hole) == 19 and oracle.word_stop(hole) - oracle.word_start(hole) + 1 == 20
    for bad_rule in (2, -1, 9):
        rc, msg = _call(lib, [pair, (hole, pair[1])], rule=bad_rule, primer_strand=0.0, salt=2.0)
        assert rc == PCR_ERR_ARG and "unknown rule" in msg
    for ps in (0.0, -9e-7, float("nan")):
        rc, msg = _call(lib, [pair, (hole, pair[1])], primer_strand=ps, salt=2.0)
        assert rc == PCR_ERR_ARG and "primer_strand" in msg
    for salt in (2.0, 0.0, 9e-7, float("nan")):
        rc, msg = _call(lib, [pair, (hole, pair[1])], salt=salt)
        assert rc == PCR_ERR_ARG and "salt" in msg
    for salt in (1e-6, 1.0):
        rc, msg = _call(lib, [pair], salt=salt)
        assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, [pair, (hole, pair[1])])
    assert rc == PCR_ERR_ARG and "hole" in msg
    rc, msg = _call(lib, [pair, ((0, 0), pair[1])])
    assert rc == PCR_ERR_ARG and "empty" in msg
    too = w("ACGTNNNNRACGTACGTACG")
    assert oracle.word_degeneracy(too) == 512
    rc, msg = _call(lib, [pair, (pair[0], too)])
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg
    most = w("ACGTNNNNACGTACGTACG")
    assert oracle.word_degeneracy(most) == api.SITE_MAX_EXPANSIONS == 256
    rc, msg = _call(lib, [(pair[0], most)])                                 # 256 expansions pass
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, [])                                                # nothing to refuse in an empty pool
    assert rc == PCR_ERR_ARG and "null handle" in msg


def test_capacity_refusal_before_the_handle(lib, oracle):
    """1 024 pairs of distinct 256-expansion oligos: 2 048 * 256 * (2 047 * 256 + 1) duplexes, far past 2^31."""
    base = "ACGTACGTACG"
    digits = "ACGT"
    pool, seen = [], set()
    for k in range(api.POOL_MAX_PAIRS):
        pair = []
        for side in (0, 1):
            v = 2 * k + side
            tail = "".join(digits[(v >> (2 * i)) & 3] for i in range(6))   # 4^6 = 4 096 distinct tails
            s = "NNNN" + base + tail
            assert s not in seen
            seen.add(s)
            pair.append(oracle.centered_word(s))
        pool.append(tuple(pair))
    assert oracle.word_degeneracy(pool[-1][1]) == 256
    assert 2048 * 256 * (2047 * 256 + 1) >= 2 ** 31
    rc, msg = _call(lib, pool)
    assert rc == PCR_ERR_CAPACITY and "2^31" in msg
    rc, msg = _call(lib, pool[:3])                                          # 6 such oligos are fine
    assert rc == PCR_ERR_ARG and "null handle" in msg


def test_batch_rule_of_the_expectation():
    """batch_starts / jobs_before, which the GPU test of the batch boundaries relies on, on a matrix small enough to list."""
    D = [2, 1, 3]
    cells = [2, 2, 6, 2, 1, 3, 6, 3, 3]                                     # row-major, the diagonal cells D(q)
    assert [PC.jobs_before(D, q, t) for q in range(3) for t in range(3)] == [sum(cells[:c]) for c in range(9)]
    assert PC.batch_starts(D, 6) == [0, 2, 3, 6, 7]                         # 2+2 | 6 | 2+1+3 | 6 | 3+3
    assert PC.batch_starts(D, 100) == [0]
    assert PC.batch_starts(D, 1) == list(range(9))                          # a cell larger than the limit is a batch of its own


@pytest.mark.parametrize("name", PC.SCENARIO_NAMES)
def test_scenario_duplexes_oracle_equals_reference(oracle, dimer_reference, name):
    """Every duplex of the scenario's checked cells: the reference's heterodimer (Tm, dH, dS) or homodimer (thermo_full[7:10])
    equals the oracle's, bit for bit."""
    pool, rule, cells = PC.checked_cells(oracle, name)
    P = PC.Pool(oracle, pool)
    jobs = set()
    PC.expected_cells(oracle, P, rule, cells, jobs=jobs)
    assert jobs, name
    kinds = set()
    for job in sorted(jobs):
        kinds.add(job[0])
        if job[0] == "homo":
            _, x, salt, s = job
            want = dimer_reference.thermo_full(x, salt, s)[7:10]
            got = oracle.thermo_full(x, salt, s)[7:10]
        else:
            _, x, y, salt, ca, cb = job
            want = dimer_reference.heterodimer_full(x, y, salt, ca, cb)
            got = oracle.heterodimer_full(x, y, salt, ca, cb)
        assert want.view(np.uint32).tolist() == got.view(np.uint32).tolist(), job
    if cells is None:
        assert kinds == ({"homo", "hetero"} if P.n > 1 else {"homo"})


def test_rules_are_the_references_own_calls(oracle, dimer_reference):
    """The two calls the GPU test pins the strand rules with: reference == oracle on the 30 assays and the 30 assay pairs."""
    pool = PC.rules_pool(oracle)
    P = PC.Pool(oracle, pool)
    for k, pair in enumerate(pool):
        want = dimer_reference.max_dimer_tm(pair, PC.SALT, PC.PRIMER_STRAND)
        assert PC.BITS(want) == PC.BITS(oracle.max_dimer_tm(pair, PC.SALT, PC.PRIMER_STRAND))
        assert PC.BITS(want) == PC.expected_cell(oracle, P, P.ids[2 * k], P.ids[2 * k + 1], PC.ASSAY)[6]      # rule ASSAY
    for a, b in PC.RULES_PAIRS:
        four = [PC.expected_cell(oracle, P, P.ids[2 * a + i], P.ids[2 * b + j], PC.POOL)[6] for i in (0, 1) for j in (0, 1)]
        m = max(np.uint32(v).view(np.float32) for v in four)
        up = np.nextafter(np.float32(m), np.float32(np.inf))
        for lim, ok in ((float(m), 0), (float(up), 1)):                     # rule POOL: incompatible at the maximum, compatible just above
            assert dimer_reference.multiplex_compatible(pool[a], pool[b], PC.SALT, PC.PRIMER_STRAND, lim) == ok
            assert oracle.multiplex_compatible(pool[a], pool[b], PC.SALT, PC.PRIMER_STRAND, lim) == ok


def test_scenarios_are_honest(oracle):
    """What the GPU tests can only show if the scenarios hold it: an order-dependent pair, a homodimer that is not the
    heterodimer of the oligo with itself, and an all-zero degenerate cell whose first and last duplex differ in dH."""
    P = PC.Pool(oracle, PC.order_pool(oracle))
    cell = lambda q, t: PC.expected_cell(oracle, P, q, t, PC.ASSAY)
    swapped = [(q, t) for q in range(P.n) for t in range(q) if cell(q, t)[6:] != cell(t, q)[6:]]
    assert len(swapped) >= 100, len(swapped)                               # (most pairs: the last bits of Tm, dH or dS)
    assert any(cell(q, t)[6] != cell(t, q)[6] for q, t in swapped)         # ... also in Tm itself
    ca = PC.strand_of(PC.ASSAY, PC.PRIMER_STRAND, 1)
    differs = 0
    for q in range(P.n):
        x = P.exps(q)[0]
        hetero = oracle.heterodimer_full(x, x, PC.SALT, ca, ca)
        differs += cell(q, q)[6:] != (PC.BITS(hetero[0]), PC.BITS(hetero[0]), PC.BITS(hetero[1]), PC.BITS(hetero[2]))
    assert differs >= 1
    E = PC.Pool(oracle, PC.expansions_pool(oracle))
    assert [E.degeneracy(k) for k in range(E.n)] == [6, 12, 24, 1]
    res = PC.duplexes_of(oracle, E, 0, 1, PC.ASSAY)                         # (under rule POOL some of them melt above 0 C)
    assert len(res) == 72 and all(PC.BITS(r[0]) == 0 for r in res)
    assert PC.BITS(res[0][1]) != PC.BITS(res[-1][1])                       # the lowest index and the highest give different records
    assert PC.expected_cell(oracle, E, 0, 1, PC.ASSAY)[3:5] == (0, 0)
    best = [PC.expected_cell(oracle, E, q, t, PC.ASSAY)[3:5] for q in range(E.n) for t in range(E.n)]
    assert any(qe > 0 and te > 0 for qe, te in best)                        # a winner that is not expansion (0, 0)
    F = PC.Pool(oracle, PC.floor_pool(oracle))
    tms = sorted(np.uint32(c[6]).view(np.float32) for c in PC.expected_cells(oracle, F, PC.ASSAY))
    assert tms[0] < tms[len(tms) // 2]                                      # a floor at the median drops some cells and keeps some
