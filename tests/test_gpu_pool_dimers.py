"""pcr_pool_dimers / Screener.pool_dimers on the GPU: every checked cell against pool_dimer_cases.expected_cell (oracle.word_expand,
oracle.heterodimer_full off the diagonal, oracle.thermo_full's homodimer on it), field for field and every float as bits."""
import ctypes as C
import random

import numpy as np
import pytest

import pool_dimer_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

RULE = {PC.POOL: "pool", PC.ASSAY: "assay"}


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _run(d, pool, rule, **kw):
    return d.pool_dimers(pool, salt=PC.SALT, primer_strand=PC.PRIMER_STRAND, rule=RULE[rule], **kw)


def _check_all(d, oracle, pool, rule):
    """Every cell of the pool -> (Pool, records)."""
    P = PC.Pool(oracle, pool)
    ids, rec = _run(d, pool, rule)
    assert ids.tolist() == P.ids
    got, want = PC.as_bits(rec), PC.expected_cells(oracle, P, rule)
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert len(got) == len(want) == P.n * P.n
    return P, rec


def _check_cells(oracle, P, rec, rule, cells):
    """The listed (q, t) of a full matrix of records (cell order)."""
    for q, t in cells:
        g = PC.as_bits(rec[q * P.n + t:q * P.n + t + 1])[0]
        w = PC.expected_cell(oracle, P, q, t, rule)
        assert g == w, (g, w)


def _in_cell_order(rec, n):
    c = np.arange(n * n, dtype=np.int64)
    return len(rec) == n * n and (rec["query_oligo"] == c // n).all() and (rec["target_oligo"] == c % n).all()


# ------------------------------------------------------------------ 1. lengths
@pytest.mark.parametrize("rule", (PC.ASSAY, PC.POOL))
def test_lengths(dev, oracle, rule):
    P, rec = _check_all(dev, oracle, PC.lengths_pool(oracle), rule)
    assert [len(P.exps(k)[0]) for k in range(P.n)] == list(PC.LENGTHS) and len(rec) == 81
    assert P.ids == [0, 1, 2, 3, 4, 5, 6, 7, 8, 0]
    zero = lambda r: all(PC.BITS(r[f]) == 0 for f in ("tm_max", "tm_min", "dH", "dS"))
    for k in range(9):                                                      # a 1-base strand leaves fewer than 3 columns: zeros
        assert zero(rec[k]) and zero(rec[9 * k])
    assert zero(rec[9 * 1 + 1])                                             # the 2-mer's homodimer
    assert not zero(rec[9 * 1 + 3]) and rec[9 * 8 + 8]["tm_max"] > 0        # the 2-mer on the 4-mer has energies; the 32-mer's homodimer melts above 0 C
    assert (rec["n_duplexes"] == 1).all() and (rec["q_expansion"] == 0).all() and (rec["t_expansion"] == 0).all()
    assert (rec["flags"] == np.where(rec["query_oligo"] == rec["target_oligo"], api.DIMER_HOMO, 0)).all()


def test_one_pair_with_f_equal_r(dev, oracle):
    P, rec = _check_all(dev, oracle, PC.self_pair_pool(oracle), PC.ASSAY)
    assert P.ids == [0, 0] and len(rec) == 1 and rec[0]["flags"] == api.DIMER_HOMO


# ------------------------------------------------------------------ 2. order
def test_order_and_diagonal(dev, oracle):
    P, rec = _check_all(dev, oracle, PC.order_pool(oracle), PC.ASSAY)
    assert P.n == 40 and len(rec) == 1600
    bits = PC.as_bits(rec)
    swapped = sum(bits[q * 40 + t][6:] != bits[t * 40 + q][6:] for q in range(40) for t in range(q))
    assert swapped >= 100                                                   # the matrix is not symmetric in its last bits
    ca = PC.strand_of(PC.ASSAY, PC.PRIMER_STRAND, 1)
    differs = 0
    for q in range(40):
        x = P.exps(q)[0]
        homo = oracle.thermo_full(x, PC.SALT, ca)[7:10]
        assert bits[q * 41][6:] == (PC.BITS(homo[0]), PC.BITS(homo[0]), PC.BITS(homo[1]), PC.BITS(homo[2]))
        hetero = oracle.heterodimer_full(x, x, PC.SALT, ca, ca)
        differs += bits[q * 41][8:] != (PC.BITS(hetero[1]), PC.BITS(hetero[2]))
    assert differs >= 1                                                     # the diagonal is the homodimer, not the heterodimer (a, a)
    m = api.Screener.dimer_matrix(rec, 40)
    assert m.shape == (40, 40) and (m.reshape(-1).view(np.uint32) == rec["tm_max"].view(np.uint32)).all()


# ------------------------------------------------------------------ 3. expansions on both sides
@pytest.mark.parametrize("rule", (PC.ASSAY, PC.POOL))
def test_expansions_on_both_sides(dev, oracle, rule):
    P, rec = _check_all(dev, oracle, PC.expansions_pool(oracle), rule)
    D = [6, 12, 24, 1]
    assert [P.degeneracy(k) for k in range(4)] == D
    assert rec["n_duplexes"].reshape(4, 4).tolist() == [[D[q] if q == t else D[q] * D[t] for t in range(4)] for q in range(4)]
    assert rec[0 * 4 + 1]["n_duplexes"] == 72 and rec[2 * 4 + 3]["n_duplexes"] == 24 and rec[3 * 4 + 2]["n_duplexes"] == 24
    diag = rec[[0, 5, 10]]
    assert (diag["q_expansion"] == diag["t_expansion"]).all() and (diag["flags"] == api.DIMER_HOMO).all()
    assert any(r["q_expansion"] > 0 and r["t_expansion"] > 0 for r in rec if r["query_oligo"] != r["target_oligo"])
    assert (rec["tm_max"] >= rec["tm_min"]).all() and (rec["tm_max"] > rec["tm_min"]).any()
    if rule == PC.ASSAY:
        # every duplex of cell (0, 1) is clamped to Tm 0 with different dH: the record is duplex 0's, not the last one's
        res = PC.duplexes_of(oracle, P, 0, 1, rule)
        assert all(PC.BITS(r[0]) == 0 for r in res) and PC.BITS(res[0][1]) != PC.BITS(res[-1][1])
        r = rec[1]
        assert (int(r["q_expansion"]), int(r["t_expansion"])) == (0, 0) and r["tm_max"] == 0.0 and r["tm_min"] == 0.0
        assert (PC.BITS(r["dH"]), PC.BITS(r["dS"])) == (PC.BITS(res[0][1]), PC.BITS(res[0][2]))
        # the diagonal of a degenerate oligo: D duplexes at primer_strand / D
        homo = [oracle.thermo_full(x, PC.SALT, float(np.float32(float(np.float32(PC.PRIMER_STRAND)) / 24)))[7:10] for x in P.exps(2)]
        assert PC.BITS(rec[10]["tm_max"]) == PC.BITS(max(h[0] for h in homo)) and rec[10]["n_duplexes"] == 24


# ------------------------------------------------------------------ 4. the largest cell
def test_largest_cell(dev, oracle):
    P, rec = _check_all(dev, oracle, PC.largest_pool(oracle), PC.ASSAY)
    assert rec["n_duplexes"].tolist() == [256, 32768, 32768, 128]
    off = rec[[1, 2]]
    assert (off["tm_max"] > off["tm_min"]).all() and int(off["q_expansion"].max()) > 127


# ------------------------------------------------------------------ 5. the rules against the reference's own calls
def test_rule_assay_is_max_dimer_tm(dev, oracle):
    pool = PC.rules_pool(oracle)
    P = PC.Pool(oracle, pool)
    ids, rec = _run(dev, pool, PC.ASSAY)
    assert ids.tolist() == P.ids and _in_cell_order(rec, P.n)
    cells = [(P.ids[2 * k], P.ids[2 * k + 1]) for k in range(30)]
    _check_cells(oracle, P, rec, PC.ASSAY, cells)
    positive = 0
    for k, (q, t) in enumerate(cells):
        want = oracle.max_dimer_tm(pool[k], PC.SALT, PC.PRIMER_STRAND)
        assert PC.BITS(rec[q * P.n + t]["tm_max"]) == PC.BITS(want), k
        positive += want > 0
    assert positive >= 5 and int(rec["n_duplexes"].max()) == 16


def test_rule_pool_is_multiplex_compatible(dev, oracle):
    pool = PC.rules_pool(oracle)
    P = PC.Pool(oracle, pool)
    ids, rec = _run(dev, pool, PC.POOL)
    assert ids.tolist() == P.ids and _in_cell_order(rec, P.n)
    positive = 0
    for a, b in PC.RULES_PAIRS:
        cells = [(P.ids[2 * a + i], P.ids[2 * b + j]) for i in (0, 1) for j in (0, 1)]
        _check_cells(oracle, P, rec, PC.POOL, cells)
        m = np.float32(max(rec[q * P.n + t]["tm_max"] for q, t in cells))
        up = np.nextafter(m, np.float32(np.inf))
        assert oracle.multiplex_compatible(pool[a], pool[b], PC.SALT, PC.PRIMER_STRAND, float(m)) == 0, (a, b)
        assert oracle.multiplex_compatible(pool[a], pool[b], PC.SALT, PC.PRIMER_STRAND, float(up)) == 1, (a, b)
        positive += m > 0
    assert positive >= 5


# ------------------------------------------------------------------ 6. floor, cap, count
def test_floor_cap_count(dev, oracle):
    pool = PC.floor_pool(oracle)
    P = PC.Pool(oracle, pool)
    want = PC.expected_cells(oracle, P, PC.ASSAY)
    tms = np.array([c[6] for c in want], np.uint32).view(np.float32)
    floor = float(np.sort(tms)[len(tms) // 2])
    kept = [c for c, tm in zip(want, tms) if tm >= np.float32(floor)]
    assert floor > 0 and 0 < len(kept) < len(want)                          # some cells are kept, some are dropped
    ids, rec = _run(dev, pool, PC.ASSAY, tm_floor=floor)
    assert PC.as_bits(rec) == kept                                          # the filtered expectation, in cell order
    a = W.pairs_array(pool)
    oid = np.zeros(2 * len(pool), np.uint32)
    args = api.ThermoArgs(PC.SALT, PC.PRIMER_STRAND, 0.0, 0.0, 0.0, 0.0)
    call = lambda fl, out, cap: dev.L.pcr_pool_dimers(dev.h, a.ctypes.data, len(pool), C.byref(args), PC.ASSAY, fl, oid.ctypes.data, out, cap)
    assert call(floor, None, 0) == len(kept)                                # count only
    buf = np.zeros(len(want), api.POOL_DIMER_DTYPE)
    assert call(floor, buf.ctypes.data, len(kept) - 1) == len(kept)         # too small: the count again
    assert call(floor, buf.ctypes.data, len(kept)) == len(kept)
    assert PC.as_bits(buf[:len(kept)]) == kept
    assert call(0.0, None, 0) == len(want) == P.n * P.n                     # tm_floor = 0: every cell
    assert call(-5.0, buf.ctypes.data, len(want)) == len(want)
    assert PC.as_bits(buf) == want
    assert call(1000.0, buf.ctypes.data, len(want)) == 0                    # nothing melts that high
    _, rec = _run(dev, pool, PC.ASSAY, tm_floor=floor, cap=1)               # the wrapper takes the count and retries
    assert PC.as_bits(rec) == kept
    ids0, none = _run(dev, [], PC.ASSAY)
    assert len(ids0) == 0 and len(none) == 0


# ------------------------------------------------------------------ 7. strides and batches
def test_more_duplexes_than_one_grid_stride(dev, oracle):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    P, rec = _check_all(dev, oracle, PC.stride_pool(oracle), PC.ASSAY)
    assert P.n == 64 and len(rec) > 12 * n_cu, "the device holds all duplexes in one stride: give stride_pool more oligos"


def test_batch_boundaries(dev, oracle):
    limit = api.POOL_DIMER_BATCH_JOBS
    pool = PC.batches_pool(oracle, limit)
    P = PC.Pool(oracle, pool)
    D = [P.degeneracy(k) for k in range(P.n)]
    assert min(D) >= 2 and set(D) == {2, 3, 4, 6}                           # every cell is several duplexes
    starts = PC.batch_starts(D, limit)
    assert len(starts) >= 3                                                 # at least two boundaries
    for s in starts[1:]:                                                    # ... which the job counts confirm
        q, t = divmod(s, P.n)
        prev = starts[starts.index(s) - 1]
        first = PC.jobs_before(D, *divmod(prev, P.n))
        here = PC.jobs_before(D, q, t)
        assert here - first <= limit < here + (D[q] if q == t else D[q] * D[t]) - first
    ids, rec = _run(dev, pool, PC.ASSAY)
    assert ids.tolist() == P.ids and _in_cell_order(rec, P.n)
    want_n = np.outer(D, D)
    want_n[np.arange(P.n), np.arange(P.n)] = D
    assert (rec["n_duplexes"].reshape(P.n, P.n) == want_n).all()
    rng = random.Random(7)
    cells = set(rng.randrange(P.n * P.n) for _ in range(500))
    for s in starts[1:]:
        cells.update(range(s - 8, s + 8))
    cells.update((0, P.n * P.n - 1))
    _check_cells(oracle, P, rec, PC.ASSAY, [divmod(c, P.n) for c in sorted(cells)])


# ------------------------------------------------------------------ 8. full size
def test_full_size_pool(dev, oracle):
    pool = PC.full_pool(oracle)
    assert len(pool) == api.POOL_MAX_PAIRS
    P = PC.Pool(oracle, pool)
    ids, rec = _run(dev, pool, PC.ASSAY)
    assert P.n == 2048 and ids.tolist() == P.ids == list(range(2048))
    assert len(rec) == 4194304 and _in_cell_order(rec, P.n)
    assert (rec["n_duplexes"] == 1).all() and (rec["q_expansion"] == 0).all() and (rec["t_expansion"] == 0).all()
    assert (rec["flags"] == (rec["query_oligo"] == rec["target_oligo"])).all()
    assert (rec["tm_max"].view(np.uint32) == rec["tm_min"].view(np.uint32)).all()
    rng = random.Random(8)
    cells = set(rng.randrange(P.n * P.n) for _ in range(2000))
    cells.update(range(2048))
    cells.update(range(2047 * 2048, 2048 * 2048))
    _check_cells(oracle, P, rec, PC.ASSAY, [divmod(c, P.n) for c in sorted(cells)])


# ------------------------------------------------------------------ 9. state
def test_fresh_handle_and_live_resources(oracle):
    before = api.live_resources()
    d = api.Screener(0)
    try:
        pool = PC.expansions_pool(oracle)                                   # nothing loaded, no word DB
        P = PC.Pool(oracle, pool)
        ids, rec = d.pool_dimers(pool, salt=PC.SALT, primer_strand=PC.PRIMER_STRAND, rule="assay")
        assert ids.tolist() == P.ids and PC.as_bits(rec) == PC.expected_cells(oracle, P, PC.ASSAY)
        _, hot = d.pool_dimers(pool, salt=PC.SALT, primer_strand=PC.PRIMER_STRAND, rule="assay", tm_floor=20.0)
        assert 0 < len(hot) < len(rec)
        assert api.live_resources()[0] > before[0]
        with pytest.raises(api.PcrError, match="salt"):
            d.pool_dimers(pool, salt=2.0)
        with pytest.raises(ValueError):
            d.pool_dimers(pool, rule="panel")
    finally:
        d.close()
    assert api.live_resources() == before


def test_loaded_handle_is_left_as_it_was(dev, oracle):
    case = SC.ids_case(oracle)
    dev.load_texts(case["seqs"])
    dev.set_active(case["active"])
    dev.select_sites(case["panel"], SC.SQ(case["thr"]))
    panel = case["panel"]

    def state():
        bits = dev.find_target_match(panel, case["thr"])
        pid, prod = dev.pool_products(panel, case["thr"], select=False)
        sid, site = dev.site_tm(panel, case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
        return bits.tolist(), pid.tolist(), prod.tolist(), sid.tolist(), site.tolist(), dev.entries()

    before = state()
    P = PC.Pool(oracle, panel)
    ids, rec = _run(dev, panel, PC.ASSAY)
    assert state() == before
    assert ids.tolist() == P.ids == [0, 1, 2, 3, 4, 0] == before[1]         # F of pair 0 is R of pair 2: one id, pool_products' numbering
    assert PC.as_bits(rec) == PC.expected_cells(oracle, P, PC.ASSAY) and len(rec) == 25


def test_salt_sequence(dev, oracle):
    pool = PC.order_pool(oracle)[:4]
    runs = [dev.pool_dimers(pool, salt=s, primer_strand=PC.PRIMER_STRAND, rule="pool")[1] for s in (0.05, 0.1, 0.05)]
    assert PC.as_bits(runs[0]) == PC.as_bits(runs[2]) and PC.as_bits(runs[0]) != PC.as_bits(runs[1])
    P = PC.Pool(oracle, pool)
    assert PC.as_bits(runs[1]) == PC.expected_cells(oracle, P, PC.POOL, salt=0.1)
