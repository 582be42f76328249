"""pcr_pool_probe_hits / Screener.probe_hits on the GPU: records, both floors and the detected rows against probe_hit_cases
(the oracle's word DB and duplex Tm; the join, the floors and the rows restated in Python), every record as sixteen u32; and
against the numpy join of the library's own pool_products_tm and site_tm."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import probe_hit_cases as H
import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

PCR_ERR_STATE = -3
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)


def _bench_module():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_probe_hits.py")
    spec = importlib.util.spec_from_file_location("bench_probe_hits", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _load(d, oracle, case, which=api.TARGET):
    """The scenario's sequences, flags, splits and word DB (the pool plus (P, P) per probe) on the device; the DB must be the one
    the oracle expects."""
    d.load_texts(case["seqs"], which=which)
    if case.get("active") is not None:
        d.set_active(case["active"], which=which)
    for s, p in case.get("splits", ()):
        d.split(s, p, which=which)
    panel = H.db_case(case)["panel"]
    (d.select_sites if case["select"] == "all" else d.select_words)(panel, SC.SQ(case["thr"]), which=which)
    assert d.entries(which=which) == H.db_of(oracle, case)


def _kw(case):
    lo, hi = PC.amp_of(case)
    return dict(SC.conditions_of(case), probe_strand=case.get("probe_strand", H.PROBE_STRAND),
                template_strand=case.get("template_strand", 0.0), amp_min=lo, amp_max=hi)


def _run(d, case, tm_floor=0.0, probe_tm_floor=0.0, which=api.TARGET, **kw):
    return d.probe_hits(case["panel"], case["probes"], case["thr"], tm_floor=tm_floor, probe_tm_floor=probe_tm_floor, which=which,
                        **_kw(case), **kw)


def _raw(d, case, tm_floor, probe_tm_floor, out, cap, detected, which=api.TARGET):
    a = W.pairs_array(case["panel"])
    pr = np.array([(0, 0) if p is None else (int(p[0]), int(p[1])) for p in case["probes"]], np.uint64).reshape(-1, 2)
    ids, pid = np.zeros(2 * len(case["panel"]), np.uint32), np.zeros(len(case["panel"]), np.uint32)
    kw = _kw(case)
    args = api.ThermoArgs(kw["salt"], kw["primer_strand"], 0.0, 0.0, 0.0, 0.0)
    ptr = lambda x: None if x is None else x.ctypes.data
    n = d.L.pcr_pool_probe_hits(d.h, which, a.ctypes.data, pr.ctypes.data, len(case["panel"]), float(case["thr"]), kw["amp_min"],
                                kw["amp_max"], C.byref(args), float(kw["probe_strand"]), float(kw["template_strand"]), float(tm_floor),
                                float(probe_tm_floor), ids.ctypes.data, pid.ctypes.data, ptr(out), cap, ptr(detected))
    return n, ids, pid


def _equal(got, want):
    g, w = H.as_bits(got), H.as_bits(want)
    for a, b in zip(g, w):
        assert a == b, (a, b)
    assert len(g) == len(w)


# ------------------------------------------------------------------ 1. every scenario at every floor pair
@pytest.mark.parametrize("name", H.SCENARIO_NAMES)
def test_scenario_at_every_floor_pair(dev, oracle, name):
    case = H.scenario(oracle, name)
    _load(dev, oracle, case)
    lo, hi = PC.amp_of(case)
    pool_ids, _ = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)
    seen = set()
    for tm_floor, probe_tm_floor in H.floor_pairs(oracle, name):
        want_ids, want_pid, want, want_detected = H.expectation(oracle, name, tm_floor, probe_tm_floor)
        ids, pid, rec, detected = _run(dev, case, tm_floor, probe_tm_floor, bits=True)
        print("%s: floors (%.6f, %.6f) keep %d hits" % (name, tm_floor, probe_tm_floor, len(rec)))
        assert ids.tolist() == want_ids == pool_ids.tolist() and pid.tolist() == want_pid
        _equal(rec, want)
        assert detected.tolist() == want_detected.tolist()
        key = [tuple(r) for r in rec[list(H.ORDER)].tolist()]
        assert key == sorted(set(key)), "records are not unique and in key order"
        for cap in sorted({0, max(len(want) - 1, 0)}):                       # the rows whatever the cap: zero rows and words included
            rows = np.full(want_detected.shape, POISON)
            out = np.zeros(max(cap, 1), api.PROBE_HIT_DTYPE)
            n, raw_ids, raw_pid = _raw(dev, case, tm_floor, probe_tm_floor, out if cap else None, cap, rows)
            assert n == len(want) and rows.tolist() == want_detected.tolist(), cap
            assert raw_ids.tolist() == want_ids and raw_pid.tolist() == want_pid
        assert _raw(dev, case, tm_floor, probe_tm_floor, None, 0, None)[0] == len(want)   # no rows asked for
        seen.add(len(rec))
    assert 0 in seen and len(H.everything(oracle, name)[4]) in seen
    rec = _run(dev, case, cap=1)[2]                                          # the wrapper grows and retries
    _equal(rec, H.expectation(oracle, name)[2])


# ------------------------------------------------------------------ 2. the library's own calls, joined in numpy
@pytest.mark.parametrize("name", H.SCENARIO_NAMES)
def test_equals_the_numpy_join_of_products_tm_and_site_tm(dev, oracle, name):
    case = H.scenario(oracle, name)
    _load(dev, oracle, case)
    join = _bench_module().host_join
    kw = _kw(case)
    pairs = H.floor_pairs(oracle, name)
    for tm_floor, probe_tm_floor in (pairs[0], pairs[-2], pairs[-1]):
        ids, pid, rec, detected = _run(dev, case, tm_floor, probe_tm_floor, bits=True)
        pids, prod, fr, rf = dev.pool_products_tm(case["panel"], case["thr"], tm_floor=tm_floor, salt=kw["salt"],
                                                  primer_strand=kw["primer_strand"], template_strand=kw["template_strand"],
                                                  amp_min=kw["amp_min"], amp_max=kw["amp_max"], bits=True)
        _, sites = dev.site_tm([(p, p) for p in H.probe_ids(case["probes"])[1]], case["thr"], salt=kw["salt"],
                               primer_strand=kw["probe_strand"], template_strand=kw["template_strand"])
        assert pids.tolist() == ids.tolist()
        want, want_detected = join(api.PROBE_HIT_DTYPE, prod, fr, rf, sites, ids, pid, probe_tm_floor)
        _equal(rec, want)
        assert detected.tolist() == want_detected.tolist()
        # the product half of every record is a record of pool_products_tm, bit for bit
        fields = list(PC.FIELDS8[:7]) + ["tm_plus", "tm_minus"]
        rows = lambda r: set(zip(*[r[f].view(np.uint32).tolist() for f in fields]))
        assert rows(rec) <= rows(prod)


# ------------------------------------------------------------------ 3. the pool's rows
def test_cross_rows(dev, oracle):
    X = H.CROSS
    case = H.scenario(oracle, "cross")
    _load(dev, oracle, case)
    ids, pid, rec, d = _run(dev, case, bits=True)
    _, _, fr, rf = dev.pool_products_tm(case["panel"], case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, bits=True)
    assert d[X["A"]].tolist() == d[X["A_again"]].tolist() != d[X["A_other_probe"]].tolist()
    assert d[X["C"]].tolist() == (fr | rf)[X["C"]].tolist() and d[X["C"]].any()
    assert d[X["A"]].tolist() != (fr | rf)[X["A"]].tolist()
    foreign = rec[(rec["plus_oligo"] == ids[2]) & (rec["minus_oligo"] == ids[3]) & (rec["probe"] == pid[X["A"]])]
    assert len(foreign) == 1 and foreign[0]["intended"] == api.HIT_PRODUCT_INTENDED
    assert pid[X["C"]] == api.NO_PROBE


def test_many_hits_one_bit(dev, oracle):
    case = H.scenario(oracle, "words")
    _load(dev, oracle, case)
    ids, pid, rec, d = _run(dev, case, bits=True)
    assert int((rec["sequence"] == PC.WORDS_BLOCK).sum()) == 192 and len(rec) > 256
    assert (int(d[0, PC.WORDS_BLOCK >> 6]) >> (PC.WORDS_BLOCK & 63)) & 1
    a = _run(dev, case, 0.0, 50.0, bits=True)
    b = _run(dev, case, 0.0, 50.0, bits=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))             # the same answer twice


def test_background(oracle):
    case = H.scenario(oracle, "cross")
    d = api.Screener(0)
    try:
        _load(d, oracle, case, which=api.BACKGROUND)
        ids, pid, rec, rows = _run(d, case, which=api.BACKGROUND, bits=True)
        _, _, want, want_rows = H.expectation(oracle, "cross")
        _equal(rec, want)
        assert rows.tolist() == want_rows.tolist()
        with pytest.raises(api.PcrError, match="no word DB"):
            _run(d, case)                                                   # the target set has none
    finally:
        d.close()


# ------------------------------------------------------------------ 4. empty inputs, state, resources
def test_empty_pool_empty_db_and_no_site(dev, oracle):
    case = H.scenario(oracle, "edges")
    _load(dev, oracle, case)
    out = dev.probe_hits([], [], case["thr"], bits=True)
    assert [len(x) for x in out[:3]] == [0, 0, 0] and out[3].shape == (0, 1)
    w = oracle.centered_word
    other = dict(case, panel=[(w("ACGTTGCAAGCTTGCATGCA"), w("TTGACCGTAGGCTAGCTAAC"))], probes=[w("GATTACAGGCTTACCGATGCAA")])
    rows = np.full((1, 1), POISON)
    assert _raw(dev, other, 0.0, 0.0, None, 0, rows)[0] == 0 and rows.tolist() == [[0]]   # a DB without a site of this pool
    dev.select_sites(other["panel"], 1.0)                                    # an empty DB
    assert dev.entries() == []
    rows = np.full((1, 1), POISON)
    assert _raw(dev, case, 0.0, 0.0, None, 0, rows)[0] == 0 and rows.tolist() == [[0]]
    ids, pid, rec = _run(dev, case)
    assert len(rec) == 0 and ids.tolist() == [0, 1] and pid.tolist() == [0]


def test_other_calls_answer_the_same(dev, oracle):
    case = H.scenario(oracle, "cross")
    _load(dev, oracle, case)

    def state():
        ids, rec, fr, rf = dev.pool_products_tm(case["panel"], case["thr"], tm_floor=55.0, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, bits=True)
        return (dev.entries(), ids.tolist(), rec.tobytes(), fr.tobytes(), rf.tobytes())

    before = state()
    entries = dev.entries()
    _run(dev, case, 55.0, 50.0, bits=True)
    assert dev.entries() == entries                                          # pcr_get_entries right after the call
    assert state() == before


def test_state_errors_and_resources(oracle):
    case = H.scenario(oracle, "ladder")
    held = api.live_resources()
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        with pytest.raises(api.PcrError, match="no word DB"):
            _run(d, case)
        assert _raw(d, case, 0.0, 0.0, None, 0, None)[0] == PCR_ERR_STATE
        with pytest.raises(api.PcrError, match="probe_tm_floor"):
            _run(d, case, probe_tm_floor=float("nan"))
        with pytest.raises(ValueError):
            _run(d, case, select="some")
        with pytest.raises(ValueError):
            d.probe_hits(case["panel"], [], case["thr"])
        ids, pid, rec, rows = _run(d, case, select="all", bits=True)        # select="all" builds the DB of the pool and its probes
        assert d.entries() == H.db_of(oracle, case)
        _equal(rec, H.expectation(oracle, "ladder")[2])
        assert rows.tolist() == H.expectation(oracle, "ladder")[3].tolist()
        assert api.live_resources()[0] > held[0]
    finally:
        d.close()
    assert api.live_resources() == held


def test_select_true_is_select_words(oracle):
    case = H.scenario(oracle, "words_db")
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        d.set_active(case["active"])
        ids, pid, rec = _run(d, case, select=True)
        assert d.entries() == H.db_of(oracle, case)
        _equal(rec, H.expectation(oracle, "words_db")[2])
    finally:
        d.close()
