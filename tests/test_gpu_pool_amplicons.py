"""pcr_pool_amplicons / Screener.product_amplicons on the GPU against the model of tests/amplicon_seq_cases.py: every info
field, the class tables and the packed bytes of every scenario, region and strand rule; the texts; the oracle's unique
amplicons; the records of the product calls as input; the narrowed hash; caps; splits; refusals; the neighbouring calls."""
import ctypes as C
import os

import numpy as np
import pytest

import amplicon_seq_cases as AC
import probe_hit_cases as H
import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

PCR_ERR_ARG, PCR_ERR_STATE = -1, -3
POISON8, POISON64 = 0xA5, 0xA5A5A5A5A5A5A5A5
SLACK = 8                                        # poisoned entries / bytes behind what a call may write


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _load(d, sc, which=api.TARGET):
    d.load_texts(sc["seqs"], which=which)
    for s, p in sc.get("splits", ()):
        d.split(s, p, which=which)


def _raw(d, rec, region, canonical, want_info=True, class_cap=0, packed_cap=None, which=api.TARGET):
    """One call on poisoned buffers -> (rc, info, class_byte_offset, class_length, packed, packed_bytes); the class arrays have
    class_cap + SLACK entries, packed has packed_cap + SLACK bytes (packed_cap None: no buffer)."""
    rec = np.ascontiguousarray(rec, api.PRODUCT_DTYPE)
    n = len(rec)
    info = np.full(max(n, 1) * 8, 0xA5A5A5A5, np.uint32).view(api.AMPLICON_INFO_DTYPE)
    off = np.full(class_cap + SLACK, POISON64, np.uint64)
    ln = np.full(class_cap + SLACK, POISON64, np.uint64)
    packed = None if packed_cap is None else np.full(packed_cap + SLACK, POISON8, np.uint8)
    need = C.c_uint64(POISON64)
    rc = d.L.pcr_pool_amplicons(d.h, which, rec.ctypes.data if n else None, n, int(region), int(canonical),
                                info.ctypes.data if want_info else None, off.ctypes.data, ln.ctypes.data, class_cap,
                                None if packed is None else packed.ctypes.data, 0 if packed is None else packed_cap, C.byref(need))
    return rc, info[:n], off, ln, packed, int(need.value)


def _same_info(got, want):
    for f in AC.INFO_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (f, int(bad[0]), int(got[f][bad[0]]), int(want[f][bad[0]]))
    assert len(got) == len(want)


def _check(d, rec, m, region, canonical, which=api.TARGET):
    """A sizing call (info only) and a full call against the model m; nothing is written behind the counts."""
    rc, info, off, ln, _, need = _raw(d, rec, region, canonical, which=which)
    assert rc == m["n_classes"], api._err(d.L)
    assert need == m["packed_bytes"]
    _same_info(info, m["info"])
    assert (off == POISON64).all() and (ln == POISON64).all()                 # class_cap = 0: the class arrays are not touched
    nc, nb = m["n_classes"], m["packed_bytes"]
    rc, info, off, ln, packed, need = _raw(d, rec, region, canonical, class_cap=nc, packed_cap=nb, which=which)
    assert rc == nc and need == nb
    _same_info(info, m["info"])
    assert ln[:nc].tolist() == m["class_length"].tolist() and off[:nc].tolist() == m["class_byte_offset"].tolist()
    assert packed[:nb].tolist() == m["packed"].tolist()
    assert (off[nc:] == POISON64).all() and (ln[nc:] == POISON64).all() and (packed[nb:] == POISON8).all()
    return info, off[:nc], ln[:nc], packed[:nb]


# ------------------------------------------------------------------ 1. every scenario, region and strand rule
@pytest.mark.parametrize("name", AC.SCENARIO_NAMES)
def test_scenario(dev, oracle, name):
    sc = AC.scenario(oracle, name)
    _load(dev, sc)
    for region in sc["regions"]:
        for canonical in (0, 1):
            m = AC.expected(oracle, name, region, canonical)
            info, _, _, _ = _check(dev, sc["records"], m, region, canonical)
            print("%s region %d canonical %d: %d records, %d classes, %d bytes, %d reversed" % (
                name, region, canonical, len(info), m["n_classes"], m["packed_bytes"], int((info["flags"] & 1).sum())))


def test_background_set(dev, oracle):
    """The same call on PCR_SET_BACKGROUND, with another set loaded as the target."""
    _load(dev, AC.scenario(oracle, "packing"), which=api.TARGET)
    sc = AC.scenario(oracle, "strands")
    _load(dev, sc, which=api.BACKGROUND)
    _check(dev, sc["records"], AC.expected(oracle, "strands", AC.REGION_INSERT, 1), AC.REGION_INSERT, 1, which=api.BACKGROUND)


# ------------------------------------------------------------------ 2. the texts, and as multiplex keys
@pytest.mark.parametrize("name,region", [("ladder", AC.REGION_PRODUCT), ("words", AC.REGION_INNER), ("strands", AC.REGION_INSERT)])
def test_texts(dev, oracle, name, region):
    sc = AC.scenario(oracle, name)
    _load(dev, sc)
    for canonical in (False, True):
        m = AC.expected(oracle, name, region, canonical)
        info, texts = dev.product_amplicons(sc["records"], region, canonical=canonical, sequences=True)
        _same_info(info, m["info"])
        assert texts == m["texts"]
        _same_info(dev.product_amplicons(sc["records"], region, canonical=canonical), m["info"])
        if name != "strands":                                                # (whole amplicons: what the design loop loads)
            assert dev.multiplex_load(texts) == dev.multiplex_load(m["texts"]) > 0
    info, texts = dev.product_amplicons(sc["records"][:0], region, sequences=True)
    assert len(info) == 0 and texts == []


# ------------------------------------------------------------------ 3. the oracle's unique amplicons
@pytest.mark.parametrize("name", AC.ORACLE_SCENARIOS)
def test_inner_spellings_are_the_oracles_unique_amplicons(dev, oracle, name):
    sc = AC.scenario(oracle, name)
    _load(dev, sc)
    info, texts = dev.product_amplicons(sc["records"], AC.REGION_INNER, sequences=True)
    AC.check_against_oracle(oracle, name, dict(info=info, spellings=[W.codes_from_text(t) for t in texts]))


# ------------------------------------------------------------------ 4. the records of the product calls as they come
def test_records_of_the_product_calls(dev, oracle):
    case = H.scenario(oracle, "ladder")
    dev.load_texts(case["seqs"])
    panel = H.db_case(case)["panel"]
    dev.select_sites(panel, SC.SQ(case["thr"]))
    lo, hi = PC.amp_of(case)
    kw = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, template_strand=case.get("template_strand", 0.0), amp_min=lo, amp_max=hi)
    _, prod = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)
    _, prod_tm = dev.pool_products_tm(case["panel"], case["thr"], **kw)
    _, _, hits = dev.probe_hits(case["panel"], case["probes"], case["thr"], probe_strand=case.get("probe_strand", H.PROBE_STRAND), **kw)
    assert len(prod) and len(prod_tm) == len(prod) and len(hits)
    coords = lambda r: tuple(int(r[f]) for f in ("sequence", "begin", "end", "inner_start", "inner_length"))
    sc = dict(seqs=case["seqs"])
    for region in AC.REGIONS:
        by_coords = {}
        for rec in (prod, prod_tm, hits):
            info = dev.product_amplicons(rec, region, canonical=True)
            m = AC.model(sc, region, True, records=rec)
            _same_info(info, m["info"])
            for r, i in zip(rec, info):                                      # equal coordinates: equal length, gc, other, flags
                assert by_coords.setdefault(coords(r), tuple(int(v) for v in i.tolist()[:4])) == tuple(int(v) for v in i.tolist()[:4])
        both = np.concatenate([prod_tm[list(api.PRODUCT_DTYPE.names)].astype(api.PRODUCT_DTYPE), prod])   # several calls in one
        info = dev.product_amplicons(both, region)
        assert info["amplicon"][:len(prod)].tolist() == info["amplicon"][len(prod):].tolist() and (info["copies"] % 2 == 0).all()


# ------------------------------------------------------------------ 5. the hash narrowed to a few bits: the resolve path
def _with_hash_bits(bits):
    old = os.environ.get("PCRAMP_DEBUG_AMP_HASH_BITS")
    os.environ["PCRAMP_DEBUG_AMP_HASH_BITS"] = str(bits)                      # read by pcr_create
    try:
        return api.Screener(0)
    finally:
        if old is None:
            os.environ.pop("PCRAMP_DEBUG_AMP_HASH_BITS", None)
        else:
            os.environ["PCRAMP_DEBUG_AMP_HASH_BITS"] = old


@pytest.mark.parametrize("bits", [1, 3])
def test_equal_hashes_are_resolved(dev, oracle, bits):
    d = _with_hash_bits(bits)
    try:
        for name in ("classes_same", "classes_distinct", "classes_mixed", "classes_empty", "strands", "random"):
            sc = AC.scenario(oracle, name)
            _load(d, sc)
            _load(dev, sc)
            for region in sc["regions"]:
                for canonical in (0, 1):
                    m = AC.expected(oracle, name, region, canonical)
                    narrow = _check(d, sc["records"], m, region, canonical)
                    full = _check(dev, sc["records"], m, region, canonical)
                    for a, b in zip(narrow, full):
                        assert a.tolist() == b.tolist()
    finally:
        d.close()


# ------------------------------------------------------------------ 6. caps
def test_caps(dev, oracle):
    sc = AC.scenario(oracle, "packing")
    _load(dev, sc)
    m = AC.expected(oracle, "packing", AC.REGION_INNER, 0)
    nc, nb = m["n_classes"], m["packed_bytes"]
    rec = sc["records"]
    # no class arrays, no packed buffer: info and the byte count all the same
    rc, info, off, ln, _, need = _raw(dev, rec, AC.REGION_INNER, 0)
    assert rc == nc and need == nb
    _same_info(info, m["info"])
    # one class short: the count comes back, info is whole, nothing behind class_cap is written
    rc, info, off, ln, packed, need = _raw(dev, rec, AC.REGION_INNER, 0, class_cap=nc - 1, packed_cap=nb)
    assert rc == nc and need == nb
    _same_info(info, m["info"])
    assert (off[nc - 1:] == POISON64).all() and (ln[nc - 1:] == POISON64).all() and (packed[nb:] == POISON8).all()
    # one byte short: the class arrays are whole, nothing behind packed_cap is written
    rc, info, off, ln, packed, need = _raw(dev, rec, AC.REGION_INNER, 0, class_cap=nc, packed_cap=nb - 1)
    assert rc == nc and need == nb
    _same_info(info, m["info"])
    assert (packed[nb - 1:] == POISON8).all() and (off[nc:] == POISON64).all() and (ln[nc:] == POISON64).all()
    # room to spare: exactly nc entries and nb bytes are written
    rc, info, off, ln, packed, need = _raw(dev, rec, AC.REGION_INNER, 0, class_cap=nc + 5, packed_cap=nb + 7)
    assert rc == nc and off[:nc].tolist() == m["class_byte_offset"].tolist() and packed[:nb].tolist() == m["packed"].tolist()
    assert (off[nc:] == POISON64).all() and (ln[nc:] == POISON64).all() and (packed[nb:] == POISON8).all()
    # info = NULL
    rc, _, off, ln, packed, need = _raw(dev, rec, AC.REGION_INNER, 0, want_info=False, class_cap=nc, packed_cap=nb)
    assert rc == nc and need == nb and packed[:nb].tolist() == m["packed"].tolist() and ln[:nc].tolist() == m["class_length"].tolist()
    # n = 0
    rc, _, _, _, _, need = _raw(dev, rec[:0], AC.REGION_INNER, 0)
    assert rc == 0 and need == 0


# ------------------------------------------------------------------ 7. a split inside a record's region
def test_split_moves_a_record_out_of_its_class(dev, oracle):
    sc = dict(AC.scenario(oracle, "classes_same"))
    _load(dev, sc)
    rec = sc["records"]
    before = _check(dev, rec, AC.expected(oracle, "classes_same", AC.REGION_INSERT, 0), AC.REGION_INSERT, 0)[0]
    assert len(set(before["amplicon"].tolist())) == 1
    k = 3                                                                    # a record on sequence 64
    s = int(rec[k]["sequence"])
    start, n = AC.region_of(rec[k], AC.REGION_INSERT)
    p = start + n // 2
    dev.split(s, p)
    sc["splits"] = [(s, p)]
    m = AC.model(sc, AC.REGION_INSERT, 0)
    info, _, _, packed = _check(dev, rec, m, AC.REGION_INSERT, 0)
    assert m["n_classes"] == 2 and info["amplicon"][k] == 1 and info["other"][k] == 1 and info["copies"][0] == len(rec) - 1
    _, texts = dev.product_amplicons(rec, AC.REGION_INSERT, sequences=True)
    assert texts[1][p - start] == "-" and texts[1].replace("-", texts[0][p - start]) == texts[0]
    _check(dev, rec, AC.model(sc, AC.REGION_INSERT, 1), AC.REGION_INSERT, 1)


# ------------------------------------------------------------------ 8. refusals with a handle
def test_refusals_with_a_handle(dev, oracle):
    sc = AC.scenario(oracle, "alignment")
    _load(dev, sc)
    good = np.zeros(6, api.PRODUCT_DTYPE)                                     # valid under every region
    for i in range(6):
        good[i] = (0, 0, 0, 60 + 7 * i, 130 + 9 * i, 75 + 7 * i, 30 + i, 0)
    m = AC.model(sc, AC.REGION_PRODUCT, 0, records=good)
    n_seq, tail = len(sc["seqs"]), AC.ALIGN_TAIL_LEN

    def refused(bad, region, at=2):
        rec = np.array(good, api.PRODUCT_DTYPE)
        rec[at] = bad
        rc, _, _, _, _, _ = _raw(dev, rec, region, 0, class_cap=8, packed_cap=64)
        msg = api._err(dev.L)
        assert rc == PCR_ERR_ARG and "record %d" % at in msg, (rc, msg)
        _check(dev, good, m, AC.REGION_PRODUCT, 0)                            # a good call follows

    refused(AC.record(AC.REGION_PRODUCT, n_seq, 0, 10), AC.REGION_PRODUCT)                  # no such sequence
    refused(AC.record(AC.REGION_PRODUCT, 0xFFFFFFFF, 0, 10), AC.REGION_PRODUCT, at=5)
    refused(AC.record(AC.REGION_PRODUCT, 1, tail - 9, 10), AC.REGION_PRODUCT, at=0)         # end = the sequence's length
    refused(AC.record(AC.REGION_PRODUCT, 1, -1, 10), AC.REGION_PRODUCT)                     # negative begin
    refused(AC.record(AC.REGION_PRODUCT, 1, 20, 0), AC.REGION_PRODUCT)                      # end < begin: only an INSERT may be empty
    refused(AC.record(AC.REGION_INNER, 1, tail - 20, 21), AC.REGION_INNER, at=4)            # an INNER stretch running off the end
    refused(AC.record(AC.REGION_INNER, 1, 5, -3), AC.REGION_INNER)
    refused(AC.record(AC.REGION_INSERT, 1, tail - 4, 5), AC.REGION_INSERT)
    refused(AC.record(AC.REGION_INSERT, 1, 10, -1), AC.REGION_INSERT)                       # m5 < p3 + 1
    rec = np.array(good, api.PRODUCT_DTYPE)                                                 # two bad records: the first is named
    rec[1], rec[3] = AC.record(AC.REGION_PRODUCT, 1, -1, 10), AC.record(AC.REGION_PRODUCT, n_seq, 0, 10)
    rc = _raw(dev, rec, AC.REGION_PRODUCT, 0)[0]
    assert rc == PCR_ERR_ARG and "record 1" in api._err(dev.L)
    # the last base of a sequence is still inside
    ok = np.array([AC.record(AC.REGION_PRODUCT, 1, tail - 10, 10), AC.record(AC.REGION_INNER, 1, tail - 10, 10)], api.PRODUCT_DTYPE)
    assert _raw(dev, ok[:1], AC.REGION_PRODUCT, 0)[0] == 1 and _raw(dev, ok[1:], AC.REGION_INNER, 0)[0] == 1
    # a set that was never loaded
    d = api.Screener(0)
    try:
        rc = _raw(d, good, AC.REGION_PRODUCT, 0)[0]
        assert rc == PCR_ERR_STATE and "not loaded" in api._err(d.L)
        with pytest.raises(api.PcrError):
            d.product_amplicons(good)
        _load(d, sc)
        _check(d, good, m, AC.REGION_PRODUCT, 0)
        rc = _raw(d, good, AC.REGION_PRODUCT, 0, which=api.BACKGROUND)[0]
        assert rc == PCR_ERR_STATE
    finally:
        d.close()


# ------------------------------------------------------------------ 9. the neighbouring calls are unchanged
def test_neighbouring_calls_are_unchanged(dev, oracle):
    case = PC.scenario(oracle, "ladder")
    dev.load_texts(case["seqs"])
    dev.select_sites(case["panel"], SC.SQ(case["thr"]))
    lo, hi = PC.amp_of(case)
    entries = dev.entries()
    ids, prod = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)
    assert len(prod) == 27
    for region in AC.REGIONS:
        for canonical in (False, True):
            info, texts = dev.product_amplicons(prod, region, canonical=canonical, sequences=True)
            assert len(info) == len(prod) and len(texts) == int(info["amplicon"].max()) + 1
    assert dev.entries() == entries
    ids2, prod2 = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)
    assert ids2.tolist() == ids.tolist() and prod2.tolist() == prod.tolist()
