"""pcr_pool_dimers_end3 / Screener.pool_dimers_end3 on the GPU: every cell record and every placement record against
dimer_end3_cases.expected (plain-Python geometry over oracle.word_expand, oracle.heterodimer_full of the run alone), field for
field and every float as bits."""
import ctypes as C
import random

import numpy as np
import pytest

import dimer_end3_cases as DC
import pool_dimer_cases as PC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

RULE = {PC.POOL: "pool", PC.ASSAY: "assay"}


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _run(d, pool, rule, min_run, min_extension, **kw):
    return d.pool_dimers_end3(pool, min_run=min_run, min_extension=min_extension, salt=PC.SALT, primer_strand=PC.PRIMER_STRAND,
                              rule=RULE[rule], placements=True, **kw)


def _check_all(d, oracle, pool, rule, min_run, min_extension, dg_max=None):
    """Every cell and placement record of the pool -> (Pool, cell records, placement records, the two expectations)."""
    P = PC.Pool(oracle, pool)
    ids, rec, pl = _run(d, pool, rule, min_run, min_extension, dg_max=dg_max)
    assert ids.tolist() == P.ids
    want_c, want_p = DC.expected(oracle, P, rule, min_run, min_extension, dg_max=dg_max)
    got_c, got_p = DC.cells_as_bits(rec), DC.places_as_bits(pl)
    for g, w in zip(got_p, want_p):
        assert g == w, (g, w)
    assert len(got_p) == len(want_p)
    for g, w in zip(got_c, want_c):
        assert g == w, (g, w)
    assert len(got_c) == len(want_c)
    return P, rec, pl, want_c, want_p


# ------------------------------------------------------------------ 1. planted anchors
def test_planted_anchors(dev, oracle):
    pool, where = DC.planted_pool(oracle)
    seen = {}
    for min_extension in (0, 1):
        P, rec, pl, _, _ = _check_all(dev, oracle, pool, PC.POOL, 3, min_extension)
        row = pl[pl["query_oligo"] == 0]
        for (r, e), t in where.items():
            j = 2 if e == "mutual" else e
            hit = row[(row["target_oligo"] == t) & (row["extension"] == j)]
            if j < min_extension:
                assert len(hit) == 0, (r, e)                                # nothing to copy: the e = 0 placements are gone
                continue
            assert len(hit) == 1 and hit[0]["run"] == r and hit[0]["overlap"] == min(22, len(P.exps(t)[0]) - j), (r, e)
            assert bool(hit[0]["flags"] & api.DIMER_END3_MUTUAL) == (e == "mutual") and hit[0]["overlap_matches"] >= r
            seen[(r, e, min_extension)] = float(hit[0]["dG"])
    assert len(seen) == 2 * len(where) - len(DC.PLANTED_R)
    assert seen[(3, 1, 1)] > seen[(8, 1, 1)] > seen[(20, 1, 1)] > seen[(22, 1, 1)]   # longer runs bind harder
    for r in DC.PLANTED_R:                                                  # min_run just above the planted run: it disappears
        P, rec, pl, _, _ = _check_all(dev, oracle, pool, PC.POOL, r + 1, 0)
        row = pl[pl["query_oligo"] == 0]
        for e in DC.PLANTED_E + ("mutual",):
            j = 2 if e == "mutual" else e
            assert not ((row["target_oligo"] == where[(r, e)]) & (row["extension"] == j)).any()
        assert (pl["run"] > r).all()


# ------------------------------------------------------------------ 2. limits
def test_limits(dev, oracle):
    P, rec, pl, _, _ = _check_all(dev, oracle, DC.limits_pool(oracle), PC.POOL, 3, 0)
    assert not ((pl["query_oligo"] == 0) & (pl["target_oligo"] == 1) & (pl["extension"] == 3)).any()   # a run of 2 never qualifies
    P, rec, pl, _, _ = _check_all(dev, oracle, DC.limits_pool(oracle), PC.POOL, 32, 0)
    assert sorted(zip(pl["query_oligo"].tolist(), pl["target_oligo"].tolist())) == [(2, 3), (3, 2)]
    for p in pl:
        assert (p["run"], p["extension"], p["overlap"], p["overlap_matches"]) == (32, 0, 32, 32) and p["flags"] == api.DIMER_END3_MUTUAL
    assert (rec["n_placements"] == 1).all() and len(rec) == 2 and (rec["dG"] < -20).all()
    _, none, nopl = _run(dev, DC.limits_pool(oracle), PC.POOL, 32, 1)       # ... and has nothing to copy
    assert len(none) == 0 and len(nopl) == 0


@pytest.mark.parametrize("min_run", (3, 5, 19))
def test_lengths(dev, oracle, min_run):
    P, rec, pl, _, _ = _check_all(dev, oracle, PC.lengths_pool(oracle), PC.ASSAY, min_run, 0)
    lens = np.array([len(P.exps(k)[0]) for k in range(P.n)])
    assert lens.tolist() == list(PC.LENGTHS)
    assert (lens[pl["query_oligo"]] >= min_run).all() and (lens[pl["target_oligo"]] >= min_run).all()
    assert (lens[rec["query_oligo"]] >= min_run).all() and (lens[rec["target_oligo"]] >= min_run).all()
    if min_run == 3:
        assert len(pl) > 0


# ------------------------------------------------------------------ 3. expansions
@pytest.mark.parametrize("rule", (PC.ASSAY, PC.POOL))
def test_expansions(dev, oracle, rule):
    P, rec, pl, want_c, _ = _check_all(dev, oracle, DC.expansions_pool(oracle), rule, 3, 0)
    D = [6, 12, 24, 1, 2, 8]
    assert [P.degeneracy(k) for k in range(P.n)] == D
    by = {(int(r["query_oligo"]), int(r["target_oligo"])): r for r in rec}
    for (q, t), r in by.items():
        assert r["n_duplexes"] == (D[q] if q == t else D[q] * D[t])
        nd, all_pl = DC.cell_placements(oracle, P, q, t, rule, 3, 0)
        assert r["n_placements"] == len(all_pl) and nd == r["n_duplexes"]   # over all duplexes of the cell
        assert bool(r["flags"] & api.DIMER_HOMO) == (q == t)
        if q == t:
            assert r["q_expansion"] == r["t_expansion"] < D[q]
    assert any(q == t and D[q] > 1 for q, t in by)                          # a degenerate oligo's diagonal: D duplexes
    assert any(r["q_expansion"] > 0 and r["t_expansion"] > 0 for r in rec if r["query_oligo"] != r["target_oligo"])
    r = by[(4, 5)]                                                          # the R at the 3' end on Y ... N
    assert r["extension"] == 5 and r["run"] >= 8 and r["n_duplexes"] == 16
    both = pl[(pl["query_oligo"] == 4) & (pl["target_oligo"] == 5) & (pl["extension"] == 5)]
    assert len(both) == 2 and both["q_expansion"].tolist() == [0, 1]


# ------------------------------------------------------------------ 4. self-priming
def test_self_priming(dev, oracle):
    P, rec, pl, _, _ = _check_all(dev, oracle, DC.self_priming_pool(oracle), PC.ASSAY, 4, 1)
    Lq = len(P.exps(0)[0])
    diag = rec[(rec["query_oligo"] == 0) & (rec["target_oligo"] == 0)]
    assert len(diag) == 1 and diag[0]["flags"] & api.DIMER_HOMO
    hit = pl[(pl["query_oligo"] == 0) & (pl["target_oligo"] == 0) & (pl["extension"] == Lq - 6)]
    assert len(hit) == 1 and hit[0]["run"] >= 6 and hit[0]["flags"] == api.DIMER_HOMO | api.DIMER_END3_MUTUAL
    text = api.dimer_products(hit, DC.self_priming_pool(oracle), [0, 1])
    assert text == [P.exps(0)[0] + DC.revcomp(P.exps(0)[0][:Lq - 6])]


# ------------------------------------------------------------------ 5. ties and order
def test_the_lower_placement_wins_a_tie(dev, oracle):
    P, rec, pl, _, _ = _check_all(dev, oracle, DC.twice_pool(oracle), PC.POOL, 3, 1)
    two = pl[(pl["query_oligo"] == 0) & (pl["target_oligo"] == 1) & (pl["run"] == 5)]
    assert two["extension"].tolist() == [2, 10]
    assert DC.places_as_bits(two[:1])[0][9:] == DC.places_as_bits(two[1:])[0][9:]
    cell = rec[(rec["query_oligo"] == 0) & (rec["target_oligo"] == 1)][0]
    assert cell["extension"] == 2 and cell["run"] == 5 and cell["n_placements"] >= 2


@pytest.mark.parametrize("rule", (PC.POOL, PC.ASSAY))
def test_random_pool(dev, oracle, rule):
    assert DC.random_counts(oracle, rule) == DC.RANDOM_COUNTS               # the case keeps exercising the tie rule
    P, rec, pl, want_c, want_p = _check_all(dev, oracle, DC.random_pool(oracle), rule, 3, 1)
    assert (len(pl), len(rec)) == DC.RANDOM_COUNTS[:2] and P.n == 40
    assert int((pl["flags"] & api.DIMER_END3_MUTUAL != 0).sum()) == DC.RANDOM_COUNTS[3]
    m = api.Screener.dimer_end3_matrix(rec, 40)
    assert np.isinf(m).sum() == 1600 - len(rec) and m[rec[0]["query_oligo"], rec[0]["target_oligo"]] == rec[0]["dG"]


# ------------------------------------------------------------------ 6. filter and caps
def test_filter_and_caps(dev, oracle):
    pool = DC.random_pool(oracle)
    P = PC.Pool(oracle, pool)
    all_c, all_p = DC.expected(oracle, P, PC.POOL, 3, 1)
    best = np.sort(np.array([c[11] for c in all_c], np.uint32).view(np.float32))
    dg_max = float(best[len(best) // 2])
    want_c, want_p = DC.expected(oracle, P, PC.POOL, 3, 1, dg_max=dg_max)
    assert 0 < len(want_c) < len(all_c) and len(want_c) <= len(want_p) < len(all_p)
    assert want_p == [p for p in all_p if DC.f32(p[9]) <= np.float32(dg_max)]   # in float32
    assert want_c == [c for c in all_c if DC.f32(c[11]) <= np.float32(dg_max)]  # n_placements is unchanged
    ids, rec, pl = _run(dev, pool, PC.POOL, 3, 1, dg_max=dg_max)
    assert DC.cells_as_bits(rec) == want_c and DC.places_as_bits(pl) == want_p
    a = W.pairs_array(pool)
    oid = np.zeros(2 * len(pool), np.uint32)
    args = api.ThermoArgs(PC.SALT, PC.PRIMER_STRAND, 0.0, 0.0, 0.0, 0.0)
    n_place = C.c_uint64(0)

    def call(dg, out, cap, pout, pcap):
        n = dev.L.pcr_pool_dimers_end3(dev.h, a.ctypes.data, len(pool), C.byref(args), PC.POOL, 3, 1, dg, oid.ctypes.data, out, cap, pout, pcap,
                                       C.byref(n_place))
        return n, n_place.value

    inf = float("inf")
    assert call(inf, None, 0, None, 0) == (len(all_c), len(all_p))         # cap 0: the counts
    assert call(dg_max, None, 0, None, 0) == (len(want_c), len(want_p))
    cbuf, pbuf = np.zeros(len(all_c), api.POOL_DIMER_END3_DTYPE), np.zeros(len(all_p), api.DIMER_PLACEMENT_DTYPE)
    assert call(dg_max, cbuf.ctypes.data, len(want_c) - 1, pbuf.ctypes.data, len(want_p) - 1) == (len(want_c), len(want_p))   # too small: the counts again
    assert call(inf, cbuf.ctypes.data, len(all_c) - 1, pbuf.ctypes.data, len(all_p)) == (len(all_c), len(all_p))
    assert DC.places_as_bits(pbuf) == all_p                                 # ... the array that was large enough is filled
    assert call(dg_max, cbuf.ctypes.data, len(want_c), None, 0) == (len(want_c), len(want_p))
    assert DC.cells_as_bits(cbuf[:len(want_c)]) == want_c
    assert call(inf, cbuf.ctypes.data, len(all_c), pbuf.ctypes.data, len(all_p)) == (len(all_c), len(all_p))
    assert DC.cells_as_bits(cbuf) == all_c and DC.places_as_bits(pbuf) == all_p
    assert call(-1000.0, cbuf.ctypes.data, len(all_c), pbuf.ctypes.data, len(all_p)) == (0, 0)
    _, rec, pl = _run(dev, pool, PC.POOL, 3, 1, dg_max=dg_max, cap=1)       # the wrapper takes the counts and retries
    assert DC.cells_as_bits(rec) == want_c and DC.places_as_bits(pl) == want_p
    ids2, rec2 = dev.pool_dimers_end3(pool, min_run=3, min_extension=1, salt=PC.SALT, primer_strand=PC.PRIMER_STRAND)
    assert ids2.tolist() == P.ids and DC.cells_as_bits(rec2) == all_c       # without placement records
    ids0, none = dev.pool_dimers_end3([])
    assert len(ids0) == 0 and len(none) == 0


# ------------------------------------------------------------------ 7. batches
def test_batch_boundaries(dev, oracle):
    limit = api.POOL_DIMER_END3_BATCH_DUPLEXES
    assert api.POOL_DIMER_END3_BATCH_JOBS <= limit
    pool = PC.batches_pool(oracle, limit)
    P = PC.Pool(oracle, pool)
    D = [P.degeneracy(k) for k in range(P.n)]
    starts = PC.batch_starts(D, limit)
    assert len(starts) >= 3                                                 # at least two boundaries between batches of cells
    ids, rec, pl = _run(dev, pool, PC.ASSAY, 3, 1)
    assert ids.tolist() == P.ids
    cell_no = rec["query_oligo"].astype(np.int64) * P.n + rec["target_oligo"]
    assert (np.diff(cell_no) > 0).all() and int(rec["n_placements"].sum()) == len(pl)
    pcell = pl["query_oligo"].astype(np.int64) * P.n + pl["target_oligo"]
    assert (np.diff(pcell) >= 0).all()
    # the melt launches split too: the jobs of a batch of cells are numbered from its first one
    csum = np.concatenate([[0], np.cumsum(rec["n_placements"].astype(np.int64))])
    first_of = np.searchsorted(cell_no, starts + [P.n * P.n])
    per_batch = np.diff(csum[first_of])
    assert per_batch.max() > 2 * api.POOL_DIMER_END3_BATCH_JOBS, per_batch
    job_cuts = []                                                           # (cell, the cell after) around every launch boundary
    for b, f in enumerate(first_of[:-1]):
        for cut in range(api.POOL_DIMER_END3_BATCH_JOBS, int(per_batch[b]), api.POOL_DIMER_END3_BATCH_JOBS):
            k = int(np.searchsorted(csum, csum[f] + cut, side="right")) - 1
            job_cuts.extend(int(cell_no[i]) for i in range(max(k - 2, 0), min(k + 3, len(rec))))
    rng = random.Random(7)
    cells = set(rng.randrange(P.n * P.n) for _ in range(200))
    for s in starts[1:]:
        cells.update(range(s - 8, s + 8))
    cells.update(job_cuts)
    cells.update((0, P.n * P.n - 1))
    cells = sorted(cells)
    want_c, want_p = DC.expected(oracle, P, PC.ASSAY, 3, 1, cells=[divmod(c, P.n) for c in cells])
    pick = np.isin(cell_no, cells)
    assert DC.cells_as_bits(rec[pick]) == want_c
    assert DC.places_as_bits(pl[np.isin(pcell, cells)]) == want_p
    assert any(c[3] > 1 for c in want_c) and len(want_c) > 50
    # 20 cells against a call with those two oligos alone
    words = {}
    for s, k in enumerate(P.ids):
        words.setdefault(k, pool[s // 2][s & 1])
    have = [c for c in want_c if c[0] != c[1]]
    for c in rng.sample(have, 20):
        q, t = c[0], c[1]
        _, r2, p2 = _run(dev, [(words[q], words[t])], PC.ASSAY, 3, 1)
        one = r2[(r2["query_oligo"] == 0) & (r2["target_oligo"] == 1)]
        mine = rec[cell_no == q * P.n + t]
        assert len(one) == 1 and DC.cells_as_bits(one)[0][2:] == DC.cells_as_bits(mine)[0][2:]
        p_one = p2[(p2["query_oligo"] == 0) & (p2["target_oligo"] == 1)]
        assert [p[2:] for p in DC.places_as_bits(p_one)] == [p[2:] for p in DC.places_as_bits(pl[pcell == q * P.n + t])]


# ------------------------------------------------------------------ 8. handle
def test_fresh_handle_and_live_resources(oracle):
    before = api.live_resources()
    d = api.Screener(0)
    try:
        pool = DC.expansions_pool(oracle)                                   # nothing loaded, no word DB
        P = PC.Pool(oracle, pool)
        dim0 = d.pool_dimers(pool, salt=PC.SALT, primer_strand=PC.PRIMER_STRAND, rule="assay")[1]
        ids, rec, pl = d.pool_dimers_end3(pool, min_run=3, min_extension=0, salt=0.1, primer_strand=PC.PRIMER_STRAND, rule="assay",
                                          placements=True)
        want_c, want_p = DC.expected(oracle, P, PC.ASSAY, 3, 0, salt=0.1)
        assert ids.tolist() == P.ids and DC.cells_as_bits(rec) == want_c and DC.places_as_bits(pl) == want_p
        dim1 = d.pool_dimers(pool, salt=PC.SALT, primer_strand=PC.PRIMER_STRAND, rule="assay")[1]
        assert dim0.tobytes() == dim1.tobytes() and len(dim0) == P.n * P.n  # pool_dimers before and after, at another salt
        assert api.live_resources()[0] > before[0]
        with pytest.raises(api.PcrError, match="min_run"):
            d.pool_dimers_end3(pool, min_run=2)
        with pytest.raises(ValueError):
            d.pool_dimers_end3(pool, rule="panel")
    finally:
        d.close()
    assert api.live_resources() == before


# ------------------------------------------------------------------ 9. errors
def test_errors_on_a_live_handle(dev, oracle):
    pool = DC.twice_pool(oracle)
    w = oracle.centered_word
    hole = (int(pool[0][0][0]) & ~(0xF << 8), int(pool[0][0][1]))
    cases = (("min_run", dict(min_run=2)), ("min_run", dict(min_run=33)), ("min_extension", dict(min_extension=32)),
             ("dg_max", dict(dg_max=float("nan"))), ("salt", dict(salt=2.0)), ("primer_strand", dict(primer_strand=0.0)))
    for word, kw in cases:
        with pytest.raises(api.PcrError, match=word):
            dev.pool_dimers_end3(pool, **kw)
    with pytest.raises(api.PcrError, match="hole"):
        dev.pool_dimers_end3(pool + [(hole, pool[0][1])])
    with pytest.raises(api.PcrError, match="PCR_SITE_MAX_EXPANSIONS"):
        dev.pool_dimers_end3(pool + [(pool[0][0], w("ACGTNNNNRACGTACGTACG"))])
    with pytest.raises(api.PcrError, match="salt"):                         # the header's order: salt before min_run
        dev.pool_dimers_end3(pool, salt=2.0, min_run=2, min_extension=40)
    with pytest.raises(api.PcrError, match="min_run"):                      # ... min_run before min_extension, dg_max and the oligos
        dev.pool_dimers_end3(pool + [(hole, pool[0][1])], min_run=2, min_extension=40, dg_max=float("nan"))
    with pytest.raises(api.PcrError, match="min_extension"):
        dev.pool_dimers_end3(pool + [(hole, pool[0][1])], min_extension=40, dg_max=float("nan"))
    with pytest.raises(api.PcrError, match="dg_max"):
        dev.pool_dimers_end3(pool + [(hole, pool[0][1])], dg_max=float("nan"))
    ids, rec = dev.pool_dimers_end3(pool, min_run=3, min_extension=0)       # the handle still works
    assert len(rec) > 0
