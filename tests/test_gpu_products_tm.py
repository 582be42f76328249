"""pcr_pool_products_tm / Screener.pool_products_tm on the GPU: records, floors and both bitsets against
products_tm_cases (the oracle's word DB and duplex Tm, the join and the floor restated in Python), every float as bits."""
import ctypes as C

import numpy as np
import pytest

import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

PCR_ERR_ARG, PCR_ERR_STATE = -1, -3
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _load(d, oracle, case, which=api.TARGET):
    """The scenario's sequences, flags, splits and word DB on the device; the DB must be the one the oracle expects."""
    d.load_texts(case["seqs"], which=which)
    if case.get("active") is not None:
        d.set_active(case["active"], which=which)
    for s, p in case.get("splits", ()):
        d.split(s, p, which=which)
    thr2 = SC.SQ(case["thr"])
    if case["select"] == "all":
        d.select_sites(case["panel"], thr2, which=which)
    else:
        d.select_words(case["panel"], thr2, which=which)
    assert d.entries(which=which) == SC.db_of(oracle, case)


def _run(d, case, tm_floor=0.0, which=api.TARGET, **kw):
    lo, hi = PC.amp_of(case)
    return d.pool_products_tm(case["panel"], case["thr"], tm_floor=tm_floor, template_strand=case.get("template_strand", 0.0),
                              amp_min=lo, amp_max=hi, which=which, **SC.conditions_of(case), **kw)


def _equal(got, want):
    g, w = PC.as_bits(got), PC.as_bits(want)
    for a, b in zip(g, w):
        assert a == b, (a, b)
    assert len(g) == len(w)


def _compare(d, oracle, name, tm_floor=0.0, which=api.TARGET):
    case = PC.scenario(oracle, name)
    ids, rec, fr, rf = _run(d, case, tm_floor, which=which, bits=True)
    want_ids, want, want_fr, want_rf = PC.expectation(oracle, name, tm_floor)
    assert ids.tolist() == want_ids
    _equal(rec, want)
    assert fr.tolist() == want_fr.tolist() and rf.tolist() == want_rf.tolist()
    assert not rec["reserved"].any()
    return ids, rec, fr, rf


def _raw(d, case, tm_floor, out, cap, fr, rf, which=api.TARGET):
    a = W.pairs_array(case["panel"])
    ids = np.zeros(2 * len(case["panel"]), np.uint32)
    cond = SC.conditions_of(case)
    args = api.ThermoArgs(cond["salt"], cond["primer_strand"], 0.0, 0.0, 0.0, 0.0)
    lo, hi = PC.amp_of(case)
    ptr = lambda x: None if x is None else x.ctypes.data
    return d.L.pcr_pool_products_tm(d.h, which, a.ctypes.data, len(case["panel"]), float(case["thr"]), lo, hi, C.byref(args),
                                    float(case.get("template_strand", 0.0)), float(tm_floor), ids.ctypes.data, ptr(out), cap, ptr(fr), ptr(rf))


# ------------------------------------------------------------------ 1. every scenario at floor 0
@pytest.mark.parametrize("name", PC.SCENARIO_NAMES)
def test_scenario(dev, oracle, name):
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    ids, rec, fr, rf = _compare(dev, oracle, name)
    lo, hi = PC.amp_of(case)
    pid, prod = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)     # the eight fields: pcr_pool_products' on this DB
    assert pid.tolist() == ids.tolist()
    assert rec[list(PC.FIELDS8)].tolist() == prod.tolist()
    key = [tuple(r) for r in rec[["plus_oligo", "minus_oligo", "sequence", "begin", "end"]].tolist()]
    assert key == sorted(set(key)), "records are not unique and in key order"


# ------------------------------------------------------------------ 2. floors
@pytest.mark.parametrize("name", PC.FLOOR_SCENARIOS)
def test_floors(dev, oracle, name):
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    _, everything, _, _ = PC.all_products(oracle, name)
    seen = set()
    for tm_floor in PC.floors_of(everything):
        _, rec, fr, rf = _compare(dev, oracle, name, tm_floor)
        seen.add(len(rec))
        print("%s: floor %.6f keeps %d of %d" % (name, tm_floor, len(rec), len(everything)))
    assert 0 in seen and len(everything) in seen and len(seen) >= 4


def test_ladder_floor_splits_the_sequences(dev, oracle):
    case = PC.scenario(oracle, "ladder")
    _load(dev, oracle, case)
    m = np.unique(PC.min_tm(PC.all_products(oracle, "ladder")[1]))
    _, rec, fr, rf = _compare(dev, oracle, "ladder", float(m[len(m) // 2]))
    assert fr.tolist() == [[0b101]] and rf.tolist() == [[0]]                 # the weakest combination's sequence is gone


# ------------------------------------------------------------------ 3. bits whatever the cap
@pytest.mark.parametrize("name,tm_floor", [("words", 0.0), ("words", 46.0), ("pairs", 0.0), ("pairs", 55.0), ("split", 0.0)])
def test_bits_whatever_the_cap(dev, oracle, name, tm_floor):
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    _, want, want_fr, want_rf = PC.expectation(oracle, name, tm_floor)
    assert tm_floor == 0.0 or 0 < len(want) < len(PC.all_products(oracle, name)[1])   # a floor that cuts through the scenario
    shape = want_fr.shape
    for cap in sorted({0, max(len(want) - 1, 0), len(want), len(want) + 7}):
        fr, rf = np.full(shape, POISON), np.full(shape, POISON)
        out = np.zeros(max(cap, 1), api.PRODUCT_TM_DTYPE)
        assert _raw(dev, case, tm_floor, out if cap else None, cap, fr, rf) == len(want), cap
        assert fr.tolist() == want_fr.tolist() and rf.tolist() == want_rf.tolist(), cap   # zero rows and words included
        if cap >= len(want):
            _equal(out[:len(want)], want)
    # one bitset alone
    fr = np.full(shape, POISON)
    assert _raw(dev, case, tm_floor, None, 0, fr, None) == len(want) and fr.tolist() == want_fr.tolist()
    rf = np.full(shape, POISON)
    assert _raw(dev, case, tm_floor, None, 0, None, rf) == len(want) and rf.tolist() == want_rf.tolist()
    ids, rec = _run(dev, case, tm_floor, cap=1)[:2]                          # the wrapper grows and retries
    _equal(rec, want)


def test_no_site_at_all(dev, oracle):
    """A DB without a hit of the pool: 0 products, and the rows are still written."""
    case = PC.scenario(oracle, "pairs")
    _load(dev, oracle, case)
    other = dict(case, panel=[(oracle.centered_word("ACGTTGCAAGCTTGCATGCA"), oracle.centered_word("TTGACCGTAGGCTAGCTAAC"))])
    fr, rf = np.full((1, 1), POISON), np.full((1, 1), POISON)
    assert _raw(dev, other, 0.0, None, 0, fr, rf) == 0
    assert fr.tolist() == [[0]] and rf.tolist() == [[0]]


# ------------------------------------------------------------------ 4. pairs, inactive sequences, background, NO_TM
def test_duplicated_equal_and_shared_pairs(dev, oracle):
    case = PC.scenario(oracle, "pairs")
    _load(dev, oracle, case)
    for tm_floor in (0.0, 55.0, 57.0):
        ids, rec, fr, rf = _compare(dev, oracle, "pairs", tm_floor)
        assert fr[0].tolist() == fr[3].tolist() and rf[0].tolist() == rf[3].tolist()
        assert fr[1].tolist() == rf[1].tolist()
        assert fr[4].tolist() == rf[0].tolist() and rf[4].tolist() == fr[0].tolist()


def test_inactive_sequences_and_many_threads_one_bit(dev, oracle):
    case = PC.scenario(oracle, "words")
    _load(dev, oracle, case)
    ids, rec, fr, rf = _compare(dev, oracle, "words")
    both = fr | rf
    for i in PC.WORDS_INACTIVE + PC.WORDS_NO_SITE:
        assert not (int(np.bitwise_or.reduce(both[:, i >> 6])) >> (i & 63)) & 1 and i not in rec["sequence"].tolist()
    assert int((rec["sequence"] == PC.WORDS_BLOCK).sum()) >= 64
    assert bin(int(fr[0, 2])).count("1") == len([i for i in range(128, PC.WORDS_N) if i % 3 == 0 or i == PC.WORDS_BLOCK])


@pytest.mark.parametrize("name", ["ids", "pairs"])
def test_background(oracle, name):
    case = PC.scenario(oracle, name)
    d = api.Screener(0)
    try:
        _load(d, oracle, case, which=api.BACKGROUND)
        _compare(d, oracle, name, which=api.BACKGROUND)
        tm_floor = float(np.median(PC.min_tm(PC.all_products(oracle, name)[1])))
        _compare(d, oracle, name, tm_floor, which=api.BACKGROUND)
        with pytest.raises(api.PcrError, match="no word DB"):
            _run(d, case)                                                   # the target set has none
    finally:
        d.close()


def test_no_tm_flags(dev, oracle):
    case = PC.scenario(oracle, "ambiguity")
    _load(dev, oracle, case)
    ids, rec, fr, rf = _compare(dev, oracle, "ambiguity")
    assert len(rec) == 1 and rec[0]["flags"] == api.PRODUCT_MINUS_NO_TM and rec[0]["intended"] == 1
    assert rec["tm_minus"].view(np.uint32)[0] == 0 and rec[0]["tm_plus"] > 50.0 and fr.tolist() == [[1]]
    ids, rec, fr, rf = _compare(dev, oracle, "ambiguity", 1e-3)             # any floor above 0: the product and its bit are gone
    assert len(rec) == 0 and fr.tolist() == [[0]] and rf.tolist() == [[0]]


# ------------------------------------------------------------------ 5. the plain count
@pytest.mark.parametrize("name", ["random", "words", "split_wide"])
def test_count_only_is_pool_products_count(dev, oracle, name):
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    lo, hi = PC.amp_of(case)
    _, prod = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)
    assert len(prod) == len(PC.all_products(oracle, name)[1])
    for tm_floor in (0.0, -3.0):
        assert _raw(dev, case, tm_floor, None, 0, None, None) == len(prod)


# ------------------------------------------------------------------ 6. state
def test_other_calls_answer_the_same(dev, oracle):
    case = PC.scenario(oracle, "ids")
    _load(dev, oracle, case)
    panel = case["panel"]

    def state():
        bits = dev.find_target_match(panel, case["thr"])
        pid, prod = dev.pool_products(panel, case["thr"], select=False)
        sid, sites = dev.site_tm(panel, case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
        did, dim = dev.pool_dimers(panel, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
        return (bits.tolist(), pid.tolist(), prod.tobytes(), sid.tolist(), sites.tobytes(), did.tolist(), dim.tobytes(), dev.entries())

    before = state()
    ids, rec, fr, rf = _compare(dev, oracle, "ids")
    _compare(dev, oracle, "ids", 58.0)
    assert state() == before
    # the host route gives the same Tm: Screener.product_tm over pool_products and site_tm
    _, prod = dev.pool_products(panel, case["thr"], select=False)
    _, sites = dev.site_tm(panel, case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
    plus, minus = dev.product_tm(prod, sites)
    assert plus.view(np.uint32).tolist() == rec["tm_plus"].view(np.uint32).tolist()
    assert minus.view(np.uint32).tolist() == rec["tm_minus"].view(np.uint32).tolist()


def test_state_errors_and_resources(oracle):
    case = PC.scenario(oracle, "ladder")
    held = api.live_resources()
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        with pytest.raises(api.PcrError, match="no word DB"):
            _run(d, case)
        assert _raw(d, case, 0.0, None, 0, None, None) == PCR_ERR_STATE
        d.select_sites(case["panel"], SC.SQ(case["thr"]))
        out = d.pool_products_tm([], case["thr"], bits=True)
        assert len(out[0]) == 0 and len(out[1]) == 0 and out[2].shape == (0, 1)
        with pytest.raises(api.PcrError, match="salt"):
            d.pool_products_tm(case["panel"], case["thr"], salt=2.0)
        with pytest.raises(api.PcrError, match="tm_floor"):
            d.pool_products_tm(case["panel"], case["thr"], tm_floor=float("nan"))
        with pytest.raises(ValueError):
            d.pool_products_tm(case["panel"], case["thr"], select="some")
        _compare(d, oracle, "ladder", 50.0)                                 # the handle is as it was
        ids, rec = d.pool_products_tm(case["panel"], case["thr"], amp_min=PC.LADDER_AMP[0], amp_max=PC.LADDER_AMP[1], select="all")
        _equal(rec, PC.expectation(oracle, "ladder")[1])                    # select="all" rebuilds the same DB
        assert api.live_resources()[0] > held[0]
    finally:
        d.close()
    assert api.live_resources() == held


# ------------------------------------------------------------------ 7. determinism
def test_determinism(dev, oracle):
    case = PC.scenario(oracle, "random")
    _load(dev, oracle, case)
    a = _run(dev, case, 40.0, bits=True)
    b = _run(dev, case, 40.0, bits=True)
    assert 0 < len(a[1]) < len(PC.all_products(oracle, "random")[1])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
