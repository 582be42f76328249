"""pcr_pool_products_end3 without a device: the symbol and the record layout, the refusals that come before the handle, and
whether end3_cases' scenarios can fail a wrong kernel -- every rule of the grid drops and keeps something, the clamps take
every value, the hanging and the degenerate-template sites are what they are meant to be, and the model's TaqMAMA bits are
the oracle session's target_match at the same thresholds."""
import ctypes as C
import gzip
import itertools
import json
import os

import numpy as np
import pytest

import reference_tape

import end3_cases as E
import products_tm_cases as PT
import site_tm_cases as SC
import site_variant_cases as SV
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1
TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "end3_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


@pytest.fixture(scope="module", autouse=True)
def _entry_point(lib):
    """Every test of this file is about pcr_pool_products_end3's cases: without the entry point in the library they say nothing."""
    assert hasattr(lib, "pcr_pool_products_end3"), "libpcramp_hip.so does not export pcr_pool_products_end3"


@pytest.fixture(scope="module")
def ends(oracle):
    return E.scenario_name(oracle, "ends")


# ------------------------------------------------------------------ the ABI
def test_symbol_and_layout(lib):
    assert "pcr_pool_products_end3" in api.ABI_SYMBOLS
    assert hasattr(lib, "pcr_pool_products_end3"), "libpcramp_hip.so does not export pcr_pool_products_end3"
    d = api.PRODUCT_END3_DTYPE
    assert d.itemsize == 64 and d == E.PRODUCT_END3
    assert [d.fields[n][1] for n in api.PRODUCT_TM_DTYPE.names] == [api.PRODUCT_TM_DTYPE.fields[n][1] for n in api.PRODUCT_TM_DTYPE.names]
    assert [d.fields[n][1] for n in ("clamp3_plus", "clamp3_minus", "end_mismatch_plus", "end_mismatch_minus", "id_plus",
                                     "id_minus", "reserved2")] == [48, 49, 50, 51, 52, 56, 60]
    assert C.sizeof(api.End3Rule) == 20


def _refused(lib, oracle, pool=None, which=api.TARGET, thermo=True, salt=0.05, primer_strand=9e-7, template_strand=0.0, tm_floor=0.0,
             n_pool=None, out_cap=0, **rule):
    """The call on a NULL handle -> (return value, message)."""
    w = oracle.centered_word
    pool = [(w("ACGTTGCAAGCTTGCATGCA"), w("TTGACCGTAGGCTAGCTAAC"))] if pool is None else pool
    a = W.pairs_array(pool)
    ids = np.zeros(max(2 * len(pool), 1), np.uint32)
    args = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    r = E.rule_of(**rule)
    rs = api.End3Rule(r["min_clamp3"], r["window"], r["max_end_mismatch"], r["use_taq_mama"], r["ident_threshold"])
    rc = lib.pcr_pool_products_end3(None, which, a.ctypes.data, len(pool) if n_pool is None else n_pool, 0.9, 80, 200,
                                    C.byref(args) if thermo else None, template_strand, tm_floor, C.byref(rs), ids.ctypes.data, None,
                                    out_cap, None, None, None)
    return rc, api._err(lib)


def test_refusals_in_order(lib, oracle):
    """Every PCR_ERR_ARG in the stated order: each case breaks one check and every later one as well (the handle is NULL
    throughout), so the message names the earliest."""
    late = dict(window=33, use_taq_mama=2, ident_threshold=2.0)             # the rule's own refusals, all at once
    steps = [
        (dict(which=7, salt=2.0, tm_floor=float("nan"), **late), "unknown sequence set"),
        (dict(which=api.MULTIPLEX, salt=2.0, tm_floor=float("nan"), **late), "PCR_SET_MULTIPLEX"),
        (dict(out_cap=5, salt=2.0, tm_floor=float("nan"), **late), "bad argument"),
        (dict(n_pool=api.POOL_MAX_PAIRS + 1, salt=2.0, tm_floor=float("nan"), **late), "PCR_POOL_MAX_PAIRS"),
        (dict(primer_strand=-1.0, salt=2.0, tm_floor=float("nan"), **late), "negative strand concentration"),
        (dict(salt=2.0, tm_floor=float("nan"), **late), "salt outside"),
        (dict(primer_strand=0.0, tm_floor=float("nan"), **late), "strand concentration of an oligo's duplex is zero"),
        (dict(tm_floor=float("nan"), **late), "tm_floor is not finite"),
        (dict(window=33, use_taq_mama=2, ident_threshold=2.0), "above 32"),
        (dict(min_clamp3=33, use_taq_mama=2, ident_threshold=2.0), "above 32"),
        (dict(max_end_mismatch=33, use_taq_mama=2, ident_threshold=2.0), "above 32"),
        (dict(use_taq_mama=2, ident_threshold=2.0), "use_taq_mama"),
        (dict(use_taq_mama=-1, ident_threshold=2.0), "use_taq_mama"),
        (dict(ident_threshold=1.5, thermo=False, tm_floor=50.0), "ident_threshold"),
        (dict(ident_threshold=-0.25, thermo=False, tm_floor=50.0), "ident_threshold"),
        (dict(ident_threshold=float("nan"), thermo=False, tm_floor=50.0), "ident_threshold"),
        (dict(ident_threshold=float("inf"), thermo=False, tm_floor=50.0), "ident_threshold"),
        (dict(thermo=False, tm_floor=50.0), "tm_floor > 0 without args"),
        (dict(), "null handle"),
        (dict(thermo=False), "null handle"),
        (dict(thermo=False, salt=2.0, primer_strand=-1.0, template_strand=-1.0), "null handle"),   # without args neither is looked at
        (dict(window=32, min_clamp3=32, max_end_mismatch=32, use_taq_mama=1, ident_threshold=1.0), "null handle"),
    ]
    for kw, what in steps:
        rc, msg = _refused(lib, oracle, **kw)
        assert rc == PCR_ERR_ARG and what in msg and "pcr_pool_products_end3" in msg, (kw, msg)


def test_oligo_refusals_come_before_the_rule(lib, oracle):
    too_many = SC.too_degenerate_oligo(oracle)
    pool = [(too_many, oracle.centered_word("TTGACCGTAGGCTAGCTAAC"))]
    for thermo in (True, False):
        rc, msg = _refused(lib, oracle, pool=pool, thermo=thermo, window=40)
        assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg


# ------------------------------------------------------------------ ends_case can fail a wrong kernel
def test_ends_case_is_as_described(oracle, ends):
    case = PT.scenario(oracle, ends)
    assert [len(s) for s in case["seqs"]] == [1660, 400, 400, 400] and case["active"] == (True, True, True, False)
    ids, words = SC.distinct_oligos(case["panel"])
    assert [oracle.word_size(w) for w in words] == [20, 22, 18, 25, 21, 32]
    assert (oracle.word_start(words[5]), oracle.word_stop(words[5])) == (0, 31)
    assert oracle.word_degeneracy(words[4]) == 2 and SC.slots_of(words[4])[oracle.word_stop(words[4])] in (5, 10)
    site = E.site_ends(oracle, ends)
    for oid, strand in ((0, 1), (2, 1), (4, 1), (1, 2), (3, 2), (5, 2)):
        on0 = [v for k, v in site.items() if k[0] == oid and k[1] == 0 and k[2] == strand]
        length = on0[0]["length"]
        assert sorted(v["clamp3"] for v in on0) == [0, 1, 2, 3, 4, 5, length - 2, length], (oid, strand)
        # equal matches, different clamp3: the six single substitutions; and the 5'-end pair is the only site two short
        assert sorted(v["clamp3"] for v in on0 if v["matches"] == length - 1) == [0, 1, 2, 3, 4, 5]
        assert [v["clamp3"] for v in on0 if v["matches"] == length - 2] == [length - 2]
    # every plus x minus combination on sequence 0 is a product
    _, rec, _ = E.products_before_rule(oracle, ends)
    plus0 = [k for k in site if k[1] == 0 and k[2] == 1 and k[0] in (0, 2, 4)]
    minus0 = [k for k in site if k[1] == 0 and k[2] == 2 and k[0] in (1, 3, 5)]
    assert len(plus0) == len(minus0) == 24
    on0 = rec[rec["sequence"] == 0]
    have = set(zip(on0["plus_oligo"].tolist(), on0["begin"].tolist(), on0["minus_oligo"].tolist(), on0["end"].tolist()))
    for p in plus0:
        for m in minus0:
            assert (p[0], p[3], m[0], m[3] + site[m]["length"] - 1) in have
    # nothing on the inactive sequence, and the split's product is gone while its neighbours stay
    assert 3 not in rec["sequence"].tolist() and not any(k[1] == 3 for k in site)
    everything = PT.all_products(oracle, ends)[1]
    s, p = E.ENDS_SPLIT
    cut = everything[(everything["sequence"] == s) & (everything["inner_start"] <= p) & (p < everything["inner_start"] + everything["inner_length"])]
    assert (2, 3) in set(zip(cut["plus_oligo"].tolist(), cut["minus_oligo"].tolist())) and len(everything) - len(cut) == len(rec)
    assert len(rec[rec["sequence"] == s]) >= 2


def test_split_drops_the_product_in_the_oracle_too(oracle, ends):
    """The product the model cuts for the EOS split is one the oracle stops reporting when the sequence is split there."""
    case = PT.scenario(oracle, ends)
    pair = case["panel"][1]
    lo, hi = PT.amp_of(case)
    found = []
    for split in (False, True):
        so = oracle.session()
        for i, s in enumerate(case["seqs"]):
            so.add_target(s, 1.0, bool(case["active"][i]))
        if split:
            so.split(*E.ENDS_SPLIT)
        so.select(case["panel"], SC.SQ(1.0))                                # the exact sites
        found.append([b for b in so.collect_amplicons(pair, 1.0, lo, hi)[0] if b[0] == E.ENDS_SPLIT[0]])
    assert found[0] == [(2, 250, 384)] and found[1] == []


def test_special_sites(oracle, ends):
    site = E.site_ends(oracle, ends, use_taq=1)
    plain = E.site_ends(oracle, ends, use_taq=0)
    hanging = {k: v for k, v in site.items() if v["hang"]}
    assert sorted((k[0], k[1], k[2]) for k in hanging) == [(1, 1, 2), (4, 1, 1)]   # the 22-mer's minus, the 21-mer's plus site
    assert all(v["clamp3"] == 0 and v["miss"][0] and v["factor"] == 1 for v in hanging.values())
    five = site[(5, 2, 1, -1)]                                              # the 32-mer hanging over the start with its 5' base
    assert five["clamp3"] == 31 and five["matches"] == 31 and five["miss"][31]
    amb = site[(0, 2, 1, 60)]                                               # N under the last base, a two-fold code under the one before
    assert amb["t2"] == 15 and amb["t1"] in (5, 10) and amb["clamp3"] == amb["matches"] == 20 and amb["factor"] == 1
    assert amb["id"] == np.float32(1.0)
    _, rec, sites = E.products_before_rule(oracle, ends)
    on = rec[(rec["sequence"] == 2) & (rec["plus_oligo"] == 0) & (rec["begin"] == 60)]
    assert len(on) >= 1 and (on["flags"] & PT.PLUS_NO_TM).all() and not on["tm_plus"].any()
    # the factor does something somewhere: a plain 3' mismatch is scaled down
    assert any(site[k]["id"] < plain[k]["id"] for k in site) and all(site[k]["id"] <= plain[k]["id"] for k in site)
    # two mismatches inside a window of five
    assert any(E.end_mismatch(v, 5) == 2 for v in site.values())


def test_clamps_agree_with_site_variants(oracle, ends):
    """clamp3 and the mismatches of every site are those of its pcr_site_variants record (site_variant_cases' model)."""
    case = PT.scenario(oracle, ends)
    _, variants, site_map, _ = SV.expectation(oracle, case, thermo=False)
    site = E.site_ends(oracle, ends)
    keys = sorted(site, key=lambda k: (k[0], k[1], k[3], k[2]))             # (oligo, sequence, loc5, strand)
    assert len(keys) == len(site_map)
    for k, v in zip(keys, site_map):
        rec = variants[v]
        assert (int(rec["oligo"]), int(rec["clamp3"]), int(rec["matches"])) == (k[0], site[k]["clamp3"], site[k]["matches"])
        mask = int(rec["mismatch_mask"])
        assert [bool((mask >> (site[k]["length"] - 1 - d)) & 1) for d in range(site[k]["length"])] == site[k]["miss"]


def test_every_rule_drops_and_keeps(oracle, ends):
    zero = E.expected(oracle, ends, E.ZERO_RULE)
    assert len(zero[1]) == zero[4] > 500
    counts = {}
    for rule in E.rule_grid():
        for thermo, tm_floor in ((True, 0.0), (False, 0.0)):
            ids, rec, fr, rf, before = E.expected(oracle, ends, rule, tm_floor, thermo)
            assert before == zero[4]
            if E.is_trivial(rule):
                assert len(rec) == before and E.as_bits(rec) == E.as_bits(E.expected(oracle, ends, E.ZERO_RULE, tm_floor, thermo)[1])
            else:
                assert 0 < len(rec) < before, rule
            counts[(rule["min_clamp3"], rule["window"], rule["max_end_mismatch"])] = len(rec)
            assert not rec["reserved"].any() and not rec["reserved2"].any()
    assert len(set(counts.values())) >= 8                                   # the grid tells many rules apart
    # a floor and a rule together: both cut
    floors = PT.floors_of(E.products_before_rule(oracle, ends)[1])
    mid = floors[2]
    r = E.expected(oracle, ends, E.rule_of(min_clamp3=3), mid)
    assert 0 < len(r[1]) < r[4] < zero[4]


# ------------------------------------------------------------------ taq_case against the oracle's find_target_match
def test_taq_case_is_as_described(oracle):
    case = E.taq_case(oracle)
    assert len(case["panel"]) == len(case["seqs"]) == 16 and all(len(s) == 300 for s in case["seqs"])
    ids, words = SC.distinct_oligos(case["panel"])
    assert len(words) == 17 and ids[1::2] == [1] * 16
    texts = [SC.spell(SC.slots_of(w)) for w in words]
    assert [t[18:] for t in texts[:1] + texts[2:]] == list(E.DINUCS) and len({t[:18] for t in texts[:1] + texts[2:]}) == 1
    for j, s in enumerate(case["seqs"]):
        assert s[E.TAQ_F_AT + 18:E.TAQ_F_AT + 20] == E.DINUCS[j] and E.TAQ_R_AT - E.TAQ_F_AT == 120
        assert min(E.TAQ_F_AT, len(s) - (E.TAQ_R_AT + 21)) >= 16


@pytest.mark.parametrize("use_taq", [0, 1])
def test_taq_model_is_find_target_match(oracle, use_taq):
    seen = set()
    for thr in E.taq_thresholds():
        name = E.taq_name(oracle, thr)
        case = PT.scenario(oracle, name)
        ids, rec, fr, rf, before = E.expected(oracle, name, E.rule_of(use_taq_mama=use_taq, ident_threshold=thr), thermo=False)
        got_fr, got_rf = E.unpack_bits(fr, 16), E.unpack_bits(rf, 16)
        want_fr, want_rf = E.oracle_bits(oracle, case, thr, use_taq)
        assert (got_fr == want_fr).all() and (got_rf == want_rf).all(), thr
        assert not got_rf.any()                                             # only the (F plus, R minus) orientation has products
        seen.add(got_fr.tobytes())
        if thr == 1.0:
            assert (got_fr == np.eye(16, dtype=bool)).all()                 # the exact cells: score exactly 1.0 = the threshold
            assert all(E.score_of(a, b) == np.float32(1.0) for a, b in zip(rec["id_plus"], rec["id_minus"]))
    assert len(seen) >= (4 if use_taq else 3)                               # without the factor: all cells, one mismatch at most, exact


def test_taq_thresholds_cut_and_differ(oracle):
    """0.96: set and clear cells with and without the factor, and cells that differ between the two.  An attainable score keeps
    its cells, the float above drops them."""
    thr = E.taq_thresholds()[0]
    name = E.taq_name(oracle, thr)
    bits = [E.unpack_bits(E.expected(oracle, name, E.rule_of(use_taq_mama=t, ident_threshold=thr), thermo=False)[2], 16) for t in (0, 1)]
    for b in bits:
        assert b.any() and not b.all()
    assert (bits[0] != bits[1]).any() and not (bits[1] & ~bits[0]).any()
    s19 = E.taq_thresholds()[2]
    at = E.unpack_bits(E.expected(oracle, E.taq_name(oracle, s19), E.rule_of(ident_threshold=s19), thermo=False)[2], 16)
    above = float(np.nextafter(np.float32(s19), np.float32(np.inf)))
    over = E.unpack_bits(E.expected(oracle, E.taq_name(oracle, above), E.rule_of(ident_threshold=above), thermo=False)[2], 16)
    assert at.sum() > over.sum() == 16


# ------------------------------------------------------------------ the oracle held to the reference on what the model asks it
# The reference's answers are on this file's own tape, in the format and through the proxies of tests/reference_tape.py:
#     PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_products_end3_host.py      # rewrites tests/golden/end3_reference_calls.json.gz
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
def end3_reference(request, oracle, _tapes):
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


def test_taq_mama_oracle_equals_reference(oracle, end3_reference):
    """The factor at every (primer pair, template pair) of plain bases."""
    for p1, p2, t1, t2 in itertools.product((1, 2, 4, 8), repeat=4):
        want = np.float32(end3_reference.taq_mama(p1, p2, t1, t2))
        assert want.view(np.uint32) == np.float32(oracle.taq_mama(p1, p2, t1, t2)).view(np.uint32), (p1, p2, t1, t2)


@pytest.mark.parametrize("use_taq", [0, 1])
def test_taq_bits_oracle_equals_reference(oracle, end3_reference, use_taq):
    """find_target_match of all 16 pairs of taq_case at every threshold of the tests: the reference's bits are the oracle's
    (both orientations together: the reference reports no orientation)."""
    for thr in E.taq_thresholds():
        case = PT.scenario(oracle, E.taq_name(oracle, thr))
        lo, hi = PT.amp_of(case)
        so = end3_reference.session(target_threshold=float(thr), amp_min=lo, amp_max=hi, use_taq_mama=int(use_taq))
        for s in case["seqs"]:
            so.add_target(s)
        so.select(case["panel"], SC.SQ(case["thr"]))
        fr, rf = E.oracle_bits(oracle, case, thr, use_taq)
        for i, pair in enumerate(case["panel"]):
            assert (np.asarray(so.target_match(pair)) != 0).tolist() == (fr[i] | rf[i]).tolist(), (thr, i)


def test_ends_duplexes_oracle_equals_reference(oracle, end3_reference, ends):
    """Every duplex ends_case melts: reference.heterodimer_full == oracle.heterodimer_full, bit for bit."""
    case = PT.scenario(oracle, ends)
    jobs = set()
    _, _, n_jobs = SC.expectation(oracle, case, jobs=jobs)
    assert 40 <= len(jobs) <= n_jobs
    for q, t, ca, cb in sorted(jobs):
        want = end3_reference.heterodimer_full(q, t, SC.SALT, ca, cb)
        got = oracle.heterodimer_full(q, t, SC.SALT, ca, cb)
        assert want.view(np.uint32).tolist() == got.view(np.uint32).tolist(), (q, t, ca, cb)
