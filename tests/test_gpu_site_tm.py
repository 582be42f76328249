"""pcr_site_tm / Screener.site_tm on the GPU: every record against site_tm_cases.expected_sites (the oracle's word DB, a Python
restatement of the target rule, oracle.word_expand and oracle.heterodimer_full), entry for entry and every float as bits."""
import ctypes as C

import numpy as np
import pytest

import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

PCR_ERR_ARG, PCR_ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _load(d, oracle, case):
    """The scenario's sequences, flags, splits and word DB on the device; the DB must be the one the oracle expects."""
    d.load_texts(case["seqs"])
    if case.get("active") is not None:
        d.set_active(case["active"])
    for s, p in case.get("splits", ()):
        d.split(s, p)
    thr2 = SC.SQ(case["thr"])
    if case["select"] == "all":
        d.select_sites(case["panel"], thr2)
    else:
        d.select_words(case["panel"], thr2)
    assert d.entries() == SC.db_of(oracle, case)


def _melt(d, case, **kw):
    return d.site_tm(case["panel"], case["thr"], template_strand=case.get("template_strand", 0.0), **SC.conditions_of(case), **kw)


def _check(d, oracle, case):
    _load(d, oracle, case)
    return _compare(d, oracle, case)


def _compare(d, oracle, case):
    ids, rec = _melt(d, case)
    want_ids, want, n_jobs = SC.expectation(oracle, case)
    assert ids.tolist() == want_ids
    got_bits, want_bits = SC.as_bits(rec), SC.as_bits(want)
    for g, w in zip(got_bits, want_bits):
        assert g == w, (g, w)
    assert len(got_bits) == len(want_bits)
    key = [(b[0], b[1], b[2], b[4]) for b in got_bits]                     # (oligo, sequence, loc5, strand)
    assert key == sorted(set(key)), "records are not unique and in key order"
    return ids, rec, n_jobs


def _at(rec, strand, loc5, oligo=0):
    r = rec[(rec["strand"] == strand) & (rec["loc5"] == loc5) & (rec["oligo"] == oligo)]
    assert len(r) == 1, (strand, loc5, oligo)
    return r[0]


# ------------------------------------------------------------------ 1. mismatch placement
def test_mismatch_placement(dev, oracle):
    case = SC.placement_case(oracle)
    _, rec, _ = _check(dev, oracle, case)
    assert len(rec) == 10
    for strand, places in ((1, SC.PLACEMENT_PLUS), (2, SC.PLACEMENT_MINUS)):
        site = [_at(rec, strand, p) for p in places]
        assert [int(s["matches"]) for s in site] == [20, 19, 19, 18, 17]
        assert all(int(s["loc3"]) == int(s["loc5"]) + 19 and s["flags"] == 0 for s in site)
        for s in site[1:]:
            print("strand %d: exact %.3f, variant with %d matches at %d: %.3f" % (strand, site[0]["tm_max"], s["matches"], s["loc5"], s["tm_max"]))
            assert site[0]["tm_max"] > s["tm_max"]
    # select_words on the same input: the arg-max subset of the same records
    _, sub, _ = _check(dev, oracle, SC.placement_case(oracle, "words"))
    assert 0 < len(sub) < len(rec)
    assert set(SC.as_bits(sub)) <= set(SC.as_bits(rec))
    assert set(int(m) for m in sub["matches"]) == {20}


# ------------------------------------------------------------------ 2. flanks and ends
def test_flanks_and_ends(dev, oracle):
    case = SC.ends_case(oracle)
    ids, rec, _ = _check(dev, oracle, case)
    assert ids.tolist() == [0, 1, 2, 3, 4, 5]
    sizes = [18, 25, 30, 31, 32, 32]
    by = {o: rec[rec["oligo"] == o] for o in range(6)}
    assert all(len(by[o]) >= 1 for o in range(6))
    assert all(int(r["loc3"]) - int(r["loc5"]) + 1 == sizes[int(r["oligo"])] for r in rec)
    assert any(r["loc5"] == 0 and r["strand"] == 1 for r in by[0])         # a site at base 0: no 5' template flank
    assert any(r["loc3"] == 77 for r in by[1]) and any(r["loc3"] == 77 for r in by[2])   # tail partial words: loc carries the + 1
    assert any(r["matches"] == 28 for r in by[5])                          # 2 bases past the end (and 2 the centred word lacks)
    assert not rec["flags"].any()


# ------------------------------------------------------------------ 3. template bases that cannot be melted
def test_no_tm_on_ambiguity(dev, oracle):
    case = SC.ambiguity_case(oracle)
    _, rec, _ = _check(dev, oracle, case)
    for strand, loc5, oligo, flagged in ((1, 50, 0, True), (1, 150, 0, False), (2, 300, 1, True), (2, 400, 1, False)):
        r = _at(rec, strand, loc5, oligo)
        assert bool(r["flags"] & api.SITE_NO_TM) == flagged
        zero = [np.float32(r[f]).view(np.uint32) == 0 for f in ("tm_max", "tm_min", "dH", "dS")]
        assert all(zero) if flagged else not any(zero)
    assert len(rec) == 4


def test_site_straddling_a_split(dev, oracle):
    """The words over an EOS join the bases on either side (Word::push_back), so the straddling site has no hole: it is a
    weaker site, melted as its word spells it; the whole copy on the other sequence is unaffected."""
    case = SC.split_case(oracle)
    _, rec, _ = _check(dev, oracle, case)
    whole = _at(rec[rec["sequence"] == 1], 1, 100)
    assert whole["matches"] == 22 and whole["flags"] == 0
    split = rec[(rec["sequence"] == 0) & (rec["oligo"] == 0)]
    assert len(split) >= 1 and int(split["matches"].max()) < 22
    assert all(whole["tm_max"] > r["tm_max"] for r in split)


# ------------------------------------------------------------------ 4. expansions
@pytest.mark.parametrize("k", range(len(SC.TEMPLATE_STRANDS)))
def test_expansions(dev, oracle, k):
    case = SC.expansions_case(oracle, SC.TEMPLATE_STRANDS[k])
    _, rec, n_jobs = _check(dev, oracle, case)
    assert sorted(int(r["n_expansions"]) for r in rec if r["matches"] == 22) == [1, 2, 4, 16, 256]
    assert n_jobs == int(rec["n_expansions"].sum())
    tie = rec[rec["oligo"] == 4]
    assert len(tie) == 1 and tie[0]["n_expansions"] == 2 and tie[0]["matches"] == 20
    # both expansions tie -- in dH and dS too, so this case cannot tell which one wins (test_tie_keeps_the_lowest_expansion can)
    assert np.float32(tie[0]["tm_max"]).view(np.uint32) == np.float32(tie[0]["tm_min"]).view(np.uint32)
    for r in rec[rec["n_expansions"] > 2]:
        assert r["tm_max"] > r["tm_min"]


def test_tie_keeps_the_lowest_expansion(dev, oracle):
    """Both expansions melt below 0 C: their Tm are clamped to 0 and tie, their dH and dS differ; the record carries those of
    expansion 0.  (In test_expansions' tie the two expansions have the same dH and dS as well: it cannot tell the rule.)"""
    case = SC.zero_tie_case(oracle)
    first, second = SC.zero_tie_expansions(oracle, case)
    assert first[0] == 0.0 and second[0] == 0.0
    assert first[1] != second[1] and first[2] != second[2]
    _, rec, _ = _check(dev, oracle, case)
    r = _at(rec, 1, 90)
    assert r["n_expansions"] == 2 and r["flags"] == 0 and r["tm_max"] == 0.0 and r["tm_min"] == 0.0
    bits = lambda x: int(np.float32(x).view(np.uint32))
    assert (bits(r["dH"]), bits(r["dS"])) == (bits(first[1]), bits(first[2]))


def test_512_expansions_are_refused(dev, oracle):
    case = SC.expansions_case(oracle)
    _load(dev, oracle, case)
    panel = list(case["panel"]) + [(case["panel"][0][0], SC.too_degenerate_oligo(oracle))]
    with pytest.raises(api.PcrError, match="PCR_SITE_MAX_EXPANSIONS"):
        dev.site_tm(panel, case["thr"])
    ids, rec = _melt(dev, case)                                            # the handle is as it was
    assert SC.as_bits(rec) == SC.as_bits(SC.expectation(oracle, case)[1])


# ------------------------------------------------------------------ 5. ids and state
def test_ids_inactive_and_state(dev, oracle):
    case = SC.ids_case(oracle)
    _load(dev, oracle, case)
    panel = case["panel"]

    def state():
        bits = dev.find_target_match(panel, case["thr"])
        amps = [dev.collect_amplicons(p, case["thr"]) for p in panel]
        pid, prod = dev.pool_products(panel, case["thr"], select=False)
        return bits.tolist(), amps, pid.tolist(), prod.tolist(), dev.entries()

    before = state()
    ids, rec, _ = _compare(dev, oracle, case)
    assert state() == before
    assert ids.tolist() == [0, 1, 2, 3, 4, 0]                              # F of pair 0 is R of pair 2: one id
    assert int(rec["oligo"].max()) == 4
    shared = rec[rec["oligo"] == 0]
    assert len(shared) == 4 and sorted(shared["strand"].tolist()) == [1, 1, 2, 2]   # ... and one set of records
    assert 1 not in rec["sequence"].tolist()                               # the inactive sequence has none
    assert before[2] == ids.tolist()                                       # pool_products' numbering


def test_state_errors(oracle):
    d = api.Screener(0)
    try:
        case = SC.placement_case(oracle)
        d.load_texts(case["seqs"])
        with pytest.raises(api.PcrError, match="no word DB"):
            d.site_tm(case["panel"], case["thr"])
        d.select_sites(case["panel"], SC.SQ(case["thr"]))
        ids, rec = d.site_tm([], case["thr"])
        assert len(ids) == 0 and len(rec) == 0
        with pytest.raises(api.PcrError, match="salt"):
            d.site_tm(case["panel"], case["thr"], salt=2.0)
    finally:
        d.close()


# ------------------------------------------------------------------ 6. cap
def test_cap(dev, oracle):
    case = SC.placement_case(oracle)
    _load(dev, oracle, case)
    _, want, _ = SC.expectation(oracle, case)
    a = W.pairs_array(case["panel"])
    ids = np.zeros(2, np.uint32)
    args = api.ThermoArgs(SC.SALT, SC.PRIMER_STRAND, 0.0, 0.0, 0.0, 0.0)
    call = lambda out, cap: dev.L.pcr_site_tm(dev.h, api.TARGET, a.ctypes.data, 1, float(case["thr"]), C.byref(args), 0.0,
                                              ids.ctypes.data, out, cap)
    assert call(None, 0) == len(want)                                      # count only
    buf = np.zeros(len(want), api.SITE_DTYPE)
    assert call(buf.ctypes.data, len(want) - 1) == len(want)               # too small: the count again
    assert call(buf.ctypes.data, len(want)) == len(want)
    assert SC.as_bits(buf) == SC.as_bits(want)
    _, rec = _melt(dev, case, cap=1)                                       # the wrapper grows and retries
    assert SC.as_bits(rec) == SC.as_bits(want)


# ------------------------------------------------------------------ 7. grid edges
def test_grid_edges(dev, oracle):
    """602 jobs of one oligo (more than one block of waves, not a multiple of a block's), then a call with a single job."""
    case = SC.grid_case(oracle)
    _, rec, n_jobs = _check(dev, oracle, case)
    many = rec[rec["oligo"] == 0]
    assert len(many) == SC.GRID_SITES and (many["n_expansions"] == 2).all() and n_jobs == 2 * SC.GRID_SITES + 1
    inner = many[1:-1]
    assert len(set(zip(inner["tm_max"].view(np.uint32).tolist(), inner["tm_min"].view(np.uint32).tolist()))) == 1
    _, one, n_jobs = _check(dev, oracle, SC.grid_single(oracle))
    assert len(one) == 1 and n_jobs == 1


def test_more_jobs_than_one_grid_stride(dev, oracle):
    """k_site_tm's grid is capped at one block of 12 waves per CU and its waves stride over the jobs: 4 097 jobs are more than
    the whole grid takes in one stride, so waves come round for a second job."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = SC.stride_case(oracle)
    _, rec, n_jobs = _check(dev, oracle, case)
    assert n_jobs == 256 * SC.STRIDE_SITES + 1
    assert n_jobs > 12 * n_cu, "the device holds all jobs in one stride: give stride_case more sites"
    many = rec[rec["oligo"] == 0]
    assert len(many) == SC.STRIDE_SITES and (many["n_expansions"] == 256).all()
    assert (many["tm_max"] > many["tm_min"]).all()


# ------------------------------------------------------------------ 8. random differential, 9. the join with pool_products
def test_random_differential_and_join(dev, oracle):
    case = SC.random_case(oracle)
    ids, rec, n_jobs = _check(dev, oracle, case)
    assert len(rec) >= 200 and n_jobs <= 4000
    assert len(set(rec["sequence"].tolist())) == 8 and set(rec["strand"].tolist()) == {1, 2}
    assert int(rec["n_expansions"].max()) == 4
    pid, prod = dev.pool_products(case["panel"], case["thr"], select=False)
    assert pid.tolist() == ids.tolist() and len(prod) >= 6
    plus, minus = dev.product_tm(prod, rec)                                # every product finds both of its sites
    for p, tp, tm in zip(prod, plus, minus):
        a = _at(rec[rec["sequence"] == p["sequence"]], 1, p["begin"], p["plus_oligo"])
        b = rec[(rec["sequence"] == p["sequence"]) & (rec["strand"] == 2) & (rec["loc3"] == p["end"]) & (rec["oligo"] == p["minus_oligo"])]
        assert len(b) == 1
        assert np.float32(tp).view(np.uint32) == np.float32(a["tm_max"]).view(np.uint32)
        assert np.float32(tm).view(np.uint32) == np.float32(b[0]["tm_max"]).view(np.uint32)
    with pytest.raises(api.PcrError, match="no .*site record"):
        dev.product_tm(prod, rec[rec["strand"] == 1])
