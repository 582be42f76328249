"""pcr_pool_dimers_end3 without a device: the oracle held to the reference on every run the scenarios of
tests/test_gpu_dimer_end3.py melt (heterodimers of 3 bases and up, which no other test meets), api.dimer_products on
hand-written placements, the records' sizes, the refusals that come before the handle, and the expectation's own geometry."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import reference_tape

import dimer_end3_cases as DC
import pool_dimer_cases as PC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1

# The reference's answers to this file's calls, on a tape of its own (format and proxies of tests/reference_tape.py, as
# tests/test_pool_dimers_host.py keeps its tape):
#     PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_dimer_end3_host.py      # rewrites the file below
END3_TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dimer_end3_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"


@pytest.fixture(scope="module")
def _end3_tapes():
    tapes = {}
    if os.path.exists(END3_TAPE):
        with gzip.open(END3_TAPE, "rt") as f:
            tapes = json.load(f)
    yield tapes
    if _RECORD:
        with gzip.GzipFile(END3_TAPE, "wb", mtime=0) as g:
            g.write(reference_tape.canonical(tapes))


@pytest.fixture
def end3_reference(request, oracle, _end3_tapes):
    """The compiled reference where it was built; elsewhere its recorded answers, checked against the oracle's."""
    from oracle_lib import Reference
    test_id = "%s::%s" % (request.node.module.__name__, request.node.name)
    if Reference.available():
        if _RECORD:
            _end3_tapes[test_id] = {}
            yield reference_tape.RecordingReference(Reference(), oracle, _end3_tapes[test_id])
        else:
            yield Reference()
        return
    if test_id not in _end3_tapes:
        pytest.fail("no recorded reference answers for %s (%s)" % (test_id, END3_TAPE))
    replay = reference_tape.ReplayReference(test_id, oracle, _end3_tapes[test_id])
    yield replay
    replay._finish()


# ------------------------------------------------------------------ the oracle on every melted run
@pytest.mark.parametrize("name", DC.SCENARIO_NAMES)
def test_scenario_runs_oracle_equals_reference(oracle, end3_reference, name):
    """Every sub-duplex the scenario melts: the reference's heterodimer (Tm, dH, dS) equals the oracle's, bit for bit."""
    pool, rule, min_run, min_extension = DC.checked(oracle, name)
    P = PC.Pool(oracle, pool)
    jobs = set()
    recs, places = DC.expected(oracle, P, rule, min_run, min_extension, jobs=jobs)
    assert jobs and places, name
    for tail, stretch, salt, ca, cb in sorted(jobs):
        assert 3 <= len(tail) == len(stretch) <= 32
        want = end3_reference.heterodimer_full(tail, stretch, salt, ca, cb)
        got = oracle.heterodimer_full(tail, stretch, salt, ca, cb)
        assert want.view(np.uint32).tolist() == got.view(np.uint32).tolist(), (tail, stretch, salt, ca, cb)
    if name == "planted":
        assert {len(j[0]) for j in jobs} >= set(DC.PLANTED_R)               # 3-base strands up to the whole 22-mer


def test_engine_has_no_energy_below_three_bases(oracle):
    """Why min_run starts at 3: perfect duplexes of 1 and 2 bases come back as zeros, 3-mers do not."""
    for s in ("A", "G", "AC", "GC", "TA"):
        assert oracle.heterodimer_full(s, DC.revcomp(s), DC.SALT, DC.PRIMER_STRAND, 0.0).view(np.uint32).tolist() == [0, 0, 0]
    for s in ("ACG", "GCC", "TAT"):
        assert any(oracle.heterodimer_full(s, DC.revcomp(s), DC.SALT, DC.PRIMER_STRAND, 0.0).view(np.uint32).tolist()[1:])


# ------------------------------------------------------------------ the Python surface
def test_record_sizes_and_constants():
    assert api.POOL_DIMER_END3_DTYPE.itemsize == 48 and api.DIMER_PLACEMENT_DTYPE.itemsize == 40
    assert api.POOL_DIMER_END3_DTYPE == DC.CELL and api.DIMER_PLACEMENT_DTYPE == DC.PLACEMENT
    assert (api.DIMER_HOMO, api.DIMER_END3_MUTUAL) == (DC.HOMO, DC.MUTUAL) == (1, 2)
    root = os.path.join(os.path.dirname(api.library_path()), "..")
    hdr = open(os.path.join(root, "include", "pcramp_hip.h")).read()
    assert "#define PCR_DIMER_END3_MUTUAL 2u" in hdr and "pcr_pool_dimers_end3" in api.ABI_SYMBOLS
    inc = open(os.path.join(os.path.dirname(api.library_path()), "csrc", "pcr_pool_dimers_end3.inc")).read()
    for name in ("POOL_DIMER_END3_BATCH_DUPLEXES", "POOL_DIMER_END3_BATCH_JOBS"):
        v = getattr(api, name)
        assert v == 1 << (v.bit_length() - 1) and "%s = 1u << %d;" % (name, v.bit_length() - 1) in inc
    assert api.POOL_DIMER_END3_BATCH_DUPLEXES >= 65536 and api.POOL_DIMER_END3_BATCH_JOBS <= api.POOL_DIMER_END3_BATCH_DUPLEXES
    assert hasattr(api.Screener, "pool_dimers_end3") and hasattr(api.Screener, "dimer_end3_matrix")


def test_dimer_products(oracle):
    w = oracle.centered_word
    x, y, z = "ACGTTGCAAGCTTGCATGCA", "TTGACCGTAGGCTAGCTAAC", "GGATCRTTAGCYAGGCTTAACG"
    pool = [(w(x), w(y)), (w(z), w(x))]
    ids = np.array([0, 1, 2, 0], np.uint32)
    pl = np.zeros(5, api.DIMER_PLACEMENT_DTYPE)
    pl["query_oligo"], pl["target_oligo"] = [0, 0, 1, 0, 2], [1, 1, 0, 2, 2]
    pl["q_expansion"], pl["t_expansion"] = [0, 0, 0, 0, 3], [0, 0, 0, 2, 3]
    pl["extension"] = [0, 5, 20, 7, 4]
    exp_z = [PC.spell(PC.slots_of(e)) for e in oracle.word_expand(w(z))]
    assert len(exp_z) == 4 and len(set(exp_z)) == 4
    want = [x, x + DC.revcomp(y[:5]), y + DC.revcomp(x), x + DC.revcomp(exp_z[2][:7]), exp_z[3] + DC.revcomp(exp_z[3][:4])]
    assert api.dimer_products(pl, pool, ids) == want
    assert api.dimer_products(pl[:0], pool, ids) == []
    for k in range(4):                                                      # the host's expansion order is the oracle's
        assert api._expansion_text(w(z), k) == exp_z[k]
    for s in (PC.EXP_A, PC.EXP_B, PC.EXP_C):
        got = [api._expansion_text(w(s), k) for k in range(int(oracle.word_degeneracy(w(s))))]
        assert got == [PC.spell(PC.slots_of(e)) for e in oracle.word_expand(w(s))]


def test_dimer_end3_matrix():
    rec = np.zeros(2, api.POOL_DIMER_END3_DTYPE)
    rec["query_oligo"], rec["target_oligo"], rec["dG"], rec["run"] = [0, 2], [1, 2], [-3.5, -1.25], [6, 4]
    m = api.Screener.dimer_end3_matrix(rec, 3)
    assert m.dtype == np.float32 and m.shape == (3, 3) and m[0, 1] == -3.5 and m[2, 2] == -1.25
    assert np.isinf(m).sum() == 7
    assert api.Screener.dimer_end3_matrix(rec, 3, "run", fill=0).tolist() == [[0, 6, 0], [0, 0, 0], [0, 0, 4]]


# ------------------------------------------------------------------ refusals before the handle
def _call(lib, pool, salt=0.05, primer_strand=9e-7, rule=PC.POOL, min_run=4, min_extension=1, dg_max=float("inf"), args=True,
          ids=True, pairs=True, out=None, cap=0, pout=None, pcap=0):
    a = W.pairs_array(pool) if pool else None
    oid = np.zeros(max(2 * len(pool), 1), np.uint32)
    ta = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    n_place = C.c_uint64(0)
    rc = lib.pcr_pool_dimers_end3(None, a.ctypes.data if (a is not None and pairs) else None, len(pool), C.byref(ta) if args else None,
                                  rule, min_run, min_extension, dg_max, oid.ctypes.data if ids else None, out, cap, pout, pcap,
                                  C.byref(n_place))
    return rc, api._err(lib)


def test_refusals_before_the_handle(oracle):
    lib = api.load_library()
    w = oracle.centered_word
    pair = (w("ACGTTGCAAGCTTGCATGCA"), w("TTGACCGTAGGCTAGCTAAC"))
    hole = (int(pair[0][0]) & ~(0xF << 8), int(pair[0][1]))
    bad_pool = [pair, (hole, pair[1])]
    rc, msg = _call(lib, [pair])
    assert rc == PCR_ERR_ARG and "null handle" in msg                       # every argument is fine: only the handle is missing
    for kw in (dict(min_run=3, min_extension=0), dict(min_run=32, min_extension=31), dict(dg_max=-2.0), dict(dg_max=float("-inf"))):
        rc, msg = _call(lib, [pair], **kw)
        assert rc == PCR_ERR_ARG and "null handle" in msg, kw
    # null pointers; a cap without its array
    for kw in (dict(args=False), dict(ids=False), dict(pairs=False), dict(cap=4), dict(pcap=4)):
        rc, msg = _call(lib, [pair], **kw)
        assert rc == PCR_ERR_ARG and "bad argument" in msg, kw
    # then, in the header's order: n_pool, rule, primer_strand, salt, min_run, min_extension, dg_max, the oligos
    wrong = dict(rule=9, primer_strand=0.0, salt=2.0, min_run=2, min_extension=32, dg_max=float("nan"))
    order = (("PCR_POOL_MAX_PAIRS", None), ("unknown rule", "rule"), ("primer_strand", "primer_strand"), ("salt", "salt"),
             ("min_run", "min_run"), ("min_extension", "min_extension"), ("dg_max", "dg_max"), ("hole", None))
    rc, msg = _call(lib, [pair] * (api.POOL_MAX_PAIRS + 1), pcap=4, **wrong)
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, [pair] * (api.POOL_MAX_PAIRS + 1), **wrong)
    assert rc == PCR_ERR_ARG and order[0][0] in msg
    for word, fixed in order[1:]:
        rc, msg = _call(lib, bad_pool, **wrong)
        assert rc == PCR_ERR_ARG and word in msg, (word, msg)
        if fixed:
            del wrong[fixed]
    assert not wrong
    for kw in (dict(min_run=2), dict(min_run=33), dict(min_run=0)):
        rc, msg = _call(lib, [pair], **kw)
        assert rc == PCR_ERR_ARG and "min_run" in msg, kw
    rc, msg = _call(lib, [pair], min_extension=32)
    assert rc == PCR_ERR_ARG and "min_extension" in msg
    rc, msg = _call(lib, [pair], dg_max=float("nan"))
    assert rc == PCR_ERR_ARG and "dg_max" in msg
    rc, msg = _call(lib, [])                                                # nothing to refuse in an empty pool
    assert rc == PCR_ERR_ARG and "null handle" in msg


# ------------------------------------------------------------------ the expectation itself
def test_geometry_by_hand():
    x = "GGGGACGT"
    # x's 3' end ...ACGT read backwards is T G C A, which pairs y[2 .. 5] = A C G T; then x's G faces y[6] = A
    assert DC.geometry(x, "TTACGTAA", 3, 0) == [(2, 4, 6, 4, False)]
    assert DC.geometry(x, "TTACGTCC", 3, 0) == [(2, 6, 6, 6, True)]         # ... or C C: the run goes on to the target's end
    assert DC.geometry("ACGT", "ACGT", 3, 0) == [(0, 4, 4, 4, True)]        # a palindrome on itself: the whole of both, MUTUAL
    assert DC.geometry("ACGT", "ACGT", 3, 1) == []                          # ... with nothing to copy
    assert DC.geometry("TTTGCA", "CCTGC", 3, 0) == [(2, 3, 3, 3, True)]     # the run reaches the target's 3' end
    assert DC.geometry("AC", "GTGT", 3, 0) == []                            # shorter than min_run
    assert DC.geometry("AAAA", "TTTTTT", 3, 2) == [(2, 4, 4, 4, True), (3, 3, 3, 3, True)]


def test_scenarios_are_honest(oracle):
    """What the GPU tests can only show if the scenarios hold it."""
    pool, where = DC.planted_pool(oracle)
    P = PC.Pool(oracle, pool)
    query = P.exps(0)[0]
    for (r, e), t in where.items():
        j = 2 if e == "mutual" else e
        got = [g for g in DC.geometry(query, P.exps(t)[0], 3, 0) if g[0] == j]
        assert len(got) == 1 and got[0][1] == r and got[0][4] == (e == "mutual"), (r, e, got)
        assert not [g for g in DC.geometry(query, P.exps(t)[0], r + 1, 0) if g[0] == j]
    L = PC.Pool(oracle, DC.limits_pool(oracle))
    assert not [g for g in DC.geometry(L.exps(0)[0], L.exps(1)[0], 2 + 1, 0) if g[0] == 3]
    assert [g for g in DC.geometry(L.exps(0)[0], L.exps(1)[0], 2, 0) if g[0] == 3][0][1] == 2   # the planted run is 2 and no more
    assert DC.geometry(L.exps(2)[0], L.exps(3)[0], 32, 0) == [(0, 32, 32, 32, True)]
    E = PC.Pool(oracle, DC.expansions_pool(oracle))
    assert [E.degeneracy(k) for k in range(E.n)] == [6, 12, 24, 1, 2, 8]
    nd, pl = DC.cell_placements(oracle, E, 4, 5, PC.ASSAY, 3, 0)
    at5 = sorted((p[2], p[3], p[4]) for p in pl if p[5] == 5)
    assert nd == 16 and len(at5) == 2 and all(r >= 8 for _, _, r in at5)    # R = A with Y = T, R = G with Y = C, and N = A
    assert [qe for qe, _, _ in at5] == [0, 1] and at5[0][1] != at5[1][1]   # one target expansion for each of the query's two
    S = PC.Pool(oracle, DC.self_priming_pool(oracle))
    diag = [p for p in DC.cell_placements(oracle, S, 0, 0, PC.ASSAY, 3, 0)[1] if p[5] == len(S.exps(0)[0]) - 6]
    assert len(diag) == 1 and diag[0][4] >= 6 and diag[0][8] == DC.HOMO | DC.MUTUAL
    T = PC.Pool(oracle, DC.twice_pool(oracle))
    nd, pl = DC.cell_placements(oracle, T, 0, 1, PC.POOL, 3, 1)
    five = [p for p in pl if p[4] == 5]
    assert [p[5] for p in five] == [2, 10] and five[0][9:] == five[1][9:]   # the same floats at two places
    assert DC.best_of(pl)[5] == 2 and DC.two_lowest_equal(pl)               # ... and the lower j wins


def test_random_pool_counts(oracle):
    """The four numbers that keep the random pool exercising the tie rule."""
    assert DC.random_counts(oracle, PC.POOL) == DC.RANDOM_COUNTS
