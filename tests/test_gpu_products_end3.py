"""pcr_pool_products_end3 / Screener.pool_products_end3 on the GPU: the zero rule against pcr_pool_products_tm on the same
handle, every rule of end3_cases' grid against its model (every integer and every float as bits), the TaqMAMA factor against
the oracle's find_target_match and pcr_amplify, counting and caps, the refusals, the handle's state, and a dense bucket against
the host route in numpy."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import dense_buckets as DB
import end3_cases as E
import products_tm_cases as PT
import site_tm_cases as SC
from pcramp_amd import api, words as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
import bench_pool_end3 as HOST  # noqa: E402  (host_end3: the host route in numpy)

pytestmark = pytest.mark.gpu

PCR_ERR_ARG, PCR_ERR_STATE = -1, -3
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _load(d, oracle, case):
    """The scenario's sequences, flags, EOS splits and all-sites word DB on the device.  The DB must be the one the oracle packs
    from the unsplit sequences: end3_cases puts its splits where no window over them matches an oligo."""
    d.load_texts(case["seqs"])
    if case.get("active") is not None:
        d.set_active(case["active"])
    for s, p in list(case.get("splits", ())) + list(case.get("eos", ())):
        d.split(s, p)
    if case["select"] == "all":
        d.select_sites(case["panel"], SC.SQ(case["thr"]))
    else:
        d.select_words(case["panel"], SC.SQ(case["thr"]))
    assert d.entries() == SC.db_of(oracle, case)


def _kw(case, thermo=True):
    lo, hi = PT.amp_of(case)
    return dict(template_strand=case.get("template_strand", 0.0), amp_min=lo, amp_max=hi, thermo=thermo, **SC.conditions_of(case))


def _raw(d, case, rule, tm_floor, out, cap, fr, rf, thermo=True, before=True, handle=True, n_pool=None, thr=None):
    """The C call -> (return value, n_before_rule or None).  rule: a dict, or None for a NULL rule."""
    a = W.pairs_array(case["panel"])
    ids = np.zeros(max(2 * len(case["panel"]), 1), np.uint32)
    cond = SC.conditions_of(case)
    args = api.ThermoArgs(cond["salt"], cond["primer_strand"], 0.0, 0.0, 0.0, 0.0)
    rs = None if rule is None else api.End3Rule(rule["min_clamp3"], rule["window"], rule["max_end_mismatch"], rule["use_taq_mama"],
                                                 rule["ident_threshold"])
    lo, hi = PT.amp_of(case)
    nb = C.c_uint64(0xDEAD)
    ptr = lambda x: None if x is None else x.ctypes.data
    n = d.L.pcr_pool_products_end3(d.h if handle else None, api.TARGET, a.ctypes.data, len(case["panel"]) if n_pool is None else n_pool,
                                   float(case["thr"] if thr is None else thr), lo, hi, C.byref(args) if thermo else None,
                                   float(case.get("template_strand", 0.0)), float(tm_floor), None if rs is None else C.byref(rs),
                                   ids.ctypes.data, ptr(out), cap, ptr(fr), ptr(rf), C.byref(nb) if before else None)
    return n, (int(nb.value) if before else None)


def _equal(got, want):
    g, w = E.as_bits(got), E.as_bits(want)
    for a, b in zip(g, w):
        assert a == b, (a, b)
    assert len(g) == len(w)


# ------------------------------------------------------------------ 1. the zero rule is pcr_pool_products_tm
@pytest.mark.parametrize("name", ["ladder", "words", "split_inner", "end3_ends"])
def test_zero_rule(dev, oracle, name):
    if name == "end3_ends":
        name = E.scenario_name(oracle, "ends")
    case = PT.scenario(oracle, name)
    _load(dev, oracle, case)
    _, everything = dev.pool_products_tm(case["panel"], case["thr"], **{k: v for k, v in _kw(case).items() if k != "thermo"})
    v = np.unique(PT.min_tm(everything))
    mid = float(v[v > 0][len(v[v > 0]) // 2]) if (v > 0).any() else 0.0      # an in-range floor: cuts where the scenario has Tm to cut
    kw = {k: v for k, v in _kw(case).items() if k != "thermo"}
    for tm_floor in (0.0, mid):
        ids, want, want_fr, want_rf = dev.pool_products_tm(case["panel"], case["thr"], tm_floor=tm_floor, bits=True, **kw)
        if tm_floor > 0 and name != "split_inner":
            assert 0 < len(want) < len(everything)
        shape = want_fr.shape
        for rule in (None, E.ZERO_RULE):
            out = np.zeros(max(len(want), 1), api.PRODUCT_END3_DTYPE)
            fr, rf = np.full(shape, POISON), np.full(shape, POISON)
            n, before = _raw(dev, case, rule, tm_floor, out, len(out), fr, rf)
            assert n == len(want) == before
            got = out[:n]
            assert got.view(np.uint8).reshape(-1, 64)[:, :48].tobytes() == want.tobytes()                    # the first 48 bytes
            assert all(got[f].tolist() == want[f].tolist() for f in ("plus_oligo", "minus_oligo", "sequence", "begin", "end", "intended"))
            assert fr.tolist() == want_fr.tolist() and rf.tolist() == want_rf.tolist()
            assert not got["reserved2"].any()
        got_ids = dev.pool_products_end3(case["panel"], case["thr"], tm_floor=tm_floor, **_kw(case))[0]
        assert got_ids.tolist() == ids.tolist()


# ------------------------------------------------------------------ 2. the rules of the grid against the model
@pytest.mark.parametrize("thermo", [True, False], ids=["thermo", "no_thermo"])
def test_rules(dev, oracle, thermo):
    name = E.scenario_name(oracle, "ends")
    case = PT.scenario(oracle, name)
    _load(dev, oracle, case)
    floors = [0.0]
    if thermo:
        floors.append(PT.floors_of(E.products_before_rule(oracle, name)[1])[2])   # the middle min-Tm itself: >= keeps it
    kw_tm = {k: v for k, v in _kw(case).items() if k != "thermo"}
    seen = set()
    for tm_floor in floors:
        n_tm = len(dev.pool_products_tm(case["panel"], case["thr"], tm_floor=tm_floor, **kw_tm)[1])
        for rule in E.rule_grid():
            want_ids, want, want_fr, want_rf, want_before = E.expected(oracle, name, rule, tm_floor, thermo)
            r = {k: v for k, v in rule.items()}
            ids, rec, fr, rf, before = dev.pool_products_end3(case["panel"], case["thr"], tm_floor=tm_floor, bits=True, **r, **_kw(case, thermo))
            print("floor %.4f rule %s: %d of %d" % (tm_floor, (rule["min_clamp3"], rule["window"], rule["max_end_mismatch"]), len(rec), before))
            assert ids.tolist() == want_ids
            _equal(rec, want)
            assert fr.tolist() == want_fr.tolist() and rf.tolist() == want_rf.tolist()
            bfr, brf = PT.bits_of(rec, ids.tolist(), len(case["seqs"]))
            assert fr.tolist() == bfr.tolist() and rf.tolist() == brf.tolist()
            assert before == want_before == n_tm
            if not thermo:
                assert not rec["tm_plus"].view(np.uint32).any() and not rec["tm_minus"].view(np.uint32).any() and not rec["flags"].any()
            seen.add(len(rec))
    assert len(seen) >= 8


def test_rules_with_identity_threshold(dev, oracle):
    """min_clamp3, the window and the identity threshold together, with and without the factor, on ends_case."""
    name = E.scenario_name(oracle, "ends")
    case = PT.scenario(oracle, name)
    _load(dev, oracle, case)
    for rule in (E.rule_of(ident_threshold=0.95), E.rule_of(ident_threshold=0.95, use_taq_mama=1), E.rule_of(use_taq_mama=1),
                 E.rule_of(min_clamp3=2, window=5, max_end_mismatch=1, use_taq_mama=1, ident_threshold=0.9)):
        want_ids, want, want_fr, want_rf, want_before = E.expected(oracle, name, rule)
        ids, rec, fr, rf, before = dev.pool_products_end3(case["panel"], case["thr"], bits=True, **rule, **_kw(case))
        _equal(rec, want)
        assert fr.tolist() == want_fr.tolist() and rf.tolist() == want_rf.tolist() and before == want_before
        if rule["ident_threshold"]:
            assert 0 < len(rec) < before


# ------------------------------------------------------------------ 3. the TaqMAMA tie
@pytest.mark.parametrize("use_taq", [0, 1])
def test_taq_mama_tie(dev, oracle, use_taq):
    base = PT.scenario(oracle, E.scenario_name(oracle, "taq"))
    _load(dev, oracle, base)
    lo, hi = PT.amp_of(base)
    n = len(base["seqs"])
    for thr in E.taq_thresholds():
        case = PT.scenario(oracle, E.taq_name(oracle, thr))                  # the same sequences and panel, collected at thr
        rule = E.rule_of(use_taq_mama=use_taq, ident_threshold=thr)
        ids, rec, fr, rf, before = dev.pool_products_end3(case["panel"], thr, bits=True, **rule, **_kw(case, thermo=False))
        want_fr, want_rf = E.oracle_bits(oracle, case, thr, use_taq)
        got_fr, got_rf = E.unpack_bits(fr, n), E.unpack_bits(rf, n)
        assert (got_fr == want_fr).all() and (got_rf == want_rf).all(), thr
        _, amp_fr, amp_rf, _ = dev.amplify(case["panel"], thr, thr, lo, hi, bool(use_taq))
        assert got_fr.tolist() == np.asarray(amp_fr, bool).tolist() and got_rf.tolist() == np.asarray(amp_rf, bool).tolist(), thr   # (amplify unpacks its rows)
        want = E.expected(oracle, E.taq_name(oracle, thr), rule, thermo=False)
        _equal(rec, want[1])
        assert before == want[4]


def test_taq_mama_identity_of_all_cells(dev, oracle):
    """id_plus of the 256 (F_i, sequence j) products: float32(matches) * float32(1 / 20) * factor, as bits."""
    name = E.scenario_name(oracle, "taq")
    case = PT.scenario(oracle, name)
    _load(dev, oracle, case)
    ids, rec, before = dev.pool_products_end3(case["panel"], case["thr"], use_taq_mama=True, **_kw(case, thermo=False))
    cells = rec[(rec["minus_oligo"] == 1) & (rec["begin"] == E.TAQ_F_AT)]
    assert len(cells) == 256 and before == len(rec)
    nib = {"A": 1, "C": 2, "G": 4, "T": 8}
    by_id = {int(ids[2 * i]): i for i in range(16)}
    seen = set()
    for r in cells:
        i, j = by_id[int(r["plus_oligo"])], int(r["sequence"])
        p, t = E.DINUCS[i], E.DINUCS[j]
        matches = 18 + (p[0] == t[0]) + (p[1] == t[1])
        factor = np.float32(oracle.taq_mama(nib[p[0]], nib[p[1]], nib[t[0]], nib[t[1]]))
        want = np.float32(np.float32(np.float32(matches) * np.float32(1.0 / 20)) * factor)
        assert r["id_plus"].view(np.uint32) == want.view(np.uint32), (p, t)
        assert r["id_minus"].view(np.uint32) == np.float32(1.0).view(np.uint32)
        assert (int(r["clamp3_plus"]), int(r["clamp3_minus"])) == (0 if p[1] != t[1] else 1 if p[0] != t[0] else 20, 21)
        seen.add((i, j))
    assert len(seen) == 256


# ------------------------------------------------------------------ 4. counting and caps
def test_counting_and_caps(dev, oracle):
    name = E.scenario_name(oracle, "ends")
    case = PT.scenario(oracle, name)
    _load(dev, oracle, case)
    rule = E.rule_of(min_clamp3=3, window=5, max_end_mismatch=0)
    _, want, want_fr, want_rf, want_before = E.expected(oracle, name, rule)
    assert 1 < len(want) < want_before
    shape = want_fr.shape
    for cap in (0, len(want) - 1, len(want), len(want) + 5):
        out = np.zeros(max(cap, 1), api.PRODUCT_END3_DTYPE)
        out.view(np.uint64)[:] = POISON
        fr, rf = np.full(shape, POISON), np.full(shape, POISON)
        n, before = _raw(dev, case, rule, 0.0, out if cap else None, cap, fr, rf)
        assert (n, before) == (len(want), want_before), cap
        assert fr.tolist() == want_fr.tolist() and rf.tolist() == want_rf.tolist(), cap   # rows in full whatever the cap
        if cap == 0:
            assert (out.view(np.uint64) == POISON).all()                        # out is not touched
        elif cap >= len(want):
            _equal(out[:n], want)
            assert (out[n:].view(np.uint64) == POISON).all()
    # no before-rule counter, one bitset alone, no bitset
    assert _raw(dev, case, rule, 0.0, None, 0, None, None, before=False) == (len(want), None)
    fr = np.full(shape, POISON)
    assert _raw(dev, case, rule, 0.0, None, 0, fr, None)[0] == len(want) and fr.tolist() == want_fr.tolist()
    # an empty pool
    assert _raw(dev, case, rule, 0.0, None, 0, None, None, n_pool=0) == (0, 0)
    out = dev.pool_products_end3([], case["thr"], bits=True, **rule)
    assert len(out[0]) == 0 and len(out[1]) == 0 and out[2].shape == (0, 1) and out[4] == 0
    # the wrapper: a count call first, or a cap that grows
    for cap in (None, 1):
        ids, rec, before = dev.pool_products_end3(case["panel"], case["thr"], cap=cap, **rule, **_kw(case))
        _equal(rec, want)
        assert before == want_before


# ------------------------------------------------------------------ 5. errors
def test_errors(oracle):
    name = E.scenario_name(oracle, "ends")
    case = PT.scenario(oracle, name)
    held = api.live_resources()
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        bad = [(dict(window=33), {}), (dict(min_clamp3=33), {}), (dict(max_end_mismatch=33), {}), (dict(use_taq_mama=2), {}),
               (dict(ident_threshold=1.5), {}), (dict(ident_threshold=float("nan")), {}), (dict(), dict(thermo=False, tm_floor=40.0))]
        for handle in (True, False):                                         # decided before the handle: the same with a NULL one
            for rule_kw, call_kw in bad:
                n, _ = _raw(d, case, E.rule_of(**rule_kw), call_kw.get("tm_floor", 0.0), None, 0, None, None,
                            thermo=call_kw.get("thermo", True), handle=handle)
                assert n == PCR_ERR_ARG and "pcr_pool_products_end3" in api._err(d.L), (rule_kw, call_kw)
            n, _ = _raw(d, case, E.ZERO_RULE, float("inf"), None, 0, None, None, handle=handle)
            assert n == PCR_ERR_ARG and "tm_floor is not finite" in api._err(d.L)
        assert _raw(d, case, E.ZERO_RULE, 0.0, None, 0, None, None, handle=False)[0] == PCR_ERR_ARG and "null handle" in api._err(d.L)
        # the order: tm_floor before the rule, the rule before tm_floor > 0 without args
        _raw(d, case, E.rule_of(window=33), float("nan"), None, 0, None, None)
        assert "tm_floor is not finite" in api._err(d.L)
        _raw(d, case, E.rule_of(window=33, use_taq_mama=2), 40.0, None, 0, None, None, thermo=False)
        assert "above 32" in api._err(d.L)
        _raw(d, case, E.rule_of(use_taq_mama=2, ident_threshold=3.0), 40.0, None, 0, None, None, thermo=False)
        assert "use_taq_mama" in api._err(d.L)
        _raw(d, case, E.rule_of(ident_threshold=3.0), 40.0, None, 0, None, None, thermo=False)
        assert "ident_threshold" in api._err(d.L)
        # no DB yet
        assert _raw(d, case, E.ZERO_RULE, 0.0, None, 0, None, None)[0] == PCR_ERR_STATE
        with pytest.raises(api.PcrError, match="no word DB"):
            d.pool_products_end3(case["panel"], case["thr"])
        with pytest.raises(ValueError):
            d.pool_products_end3(case["panel"], case["thr"], select="some")
        with pytest.raises(api.PcrError, match="without args"):
            d.pool_products_end3(case["panel"], case["thr"], tm_floor=40.0, thermo=False, select="all")
    finally:
        d.close()
    assert api.live_resources() == held


# ------------------------------------------------------------------ 6. state
def test_state(oracle):
    name = E.scenario_name(oracle, "ends")
    case = PT.scenario(oracle, name)
    panel, thr = case["panel"], case["thr"]
    melt = SC.conditions_of(case)
    rule_a = E.rule_of(min_clamp3=3, window=5, max_end_mismatch=1, use_taq_mama=1, ident_threshold=0.9)
    rule_b = E.rule_of(min_clamp3=1, window=1)
    kw_tm = {k: v for k, v in _kw(case).items() if k != "thermo"}
    calls = [
        ("site_tm", lambda d: d.site_tm(panel, thr, **melt)),
        ("end3, rule A", lambda d: d.pool_products_end3(panel, thr, tm_floor=45.0, bits=True, **rule_a, **_kw(case))[:5]),
        ("products_tm", lambda d: d.pool_products_tm(panel, thr, tm_floor=45.0, bits=True, **kw_tm)),
        ("end3, rule B, no thermodynamics", lambda d: d.pool_products_end3(panel[:2], thr, bits=True, **rule_b, **_kw(case, thermo=False))[:5]),
        ("site_variants", lambda d: d.site_variants(panel, thr, site_map=True, **melt)),
        ("end3, rule A again", lambda d: d.pool_products_end3(panel, thr, tm_floor=45.0, bits=True, **rule_a, **_kw(case))[:5]),
    ]
    as_bytes = lambda out: [np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else x for x in out]
    held = api.live_resources()
    one = api.Screener(0)
    try:
        _load(one, oracle, case)
        got = [as_bytes(call(one)) for _, call in calls]
        for (what, call), mine in zip(calls, got):
            fresh = api.Screener(0)
            try:
                _load(fresh, oracle, case)
                out = call(fresh)
            finally:
                fresh.close()
            assert len(out[1]) >= 1, what
            assert mine == as_bytes(out), what
        assert got[1] == got[5]
        assert api.live_resources()[0] > held[0]
    finally:
        one.close()
    assert api.live_resources() == held


# ------------------------------------------------------------------ 7. a dense bucket against the host route
def test_dense_bucket_against_the_host_route(oracle, monkeypatch, capfd):
    """The 4 096-slot class of dense_buckets: sites that several entries share go through site_pick in both routes."""
    dn = DB.build(oracle, "4k")
    sc, o = dn.sc, dn.sc.opts
    pool = [sc.pairs[p] for p in (dn.k["d"], 0, 1, 2)]
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    d = api.Screener(0)
    try:
        d.load_texts(sc.seqs, sc.weights)
        act = np.ones(len(sc.seqs), np.uint8)
        act[list(sc.inactive)] = 0
        d.set_active(act)
        for i, pos in sc.splits:
            d.split(i, pos)
        capfd.readouterr()
        d.select_words(sc.pairs, float(np.float32(o["target_threshold"]) * np.float32(o["search_multiplier"])), o["min_primer"], 0, 0)
        done = [(int(a), int(b)) for a, b in re.findall(r"pass done: (\d+)-slot buckets, largest fill (\d+)", capfd.readouterr().err)]
        cap = DB.CLASSES["4k"].cap
        assert done and done[-1][0] == cap and cap // 2 < done[-1][1] <= cap, done
        # at the threshold the DB was selected at, the near-copy that is its sequence's best site of the decoy oligo is a site: one
        # substitution at least three bases from either end, which a clamp of 18 refuses and the identity threshold admits
        thr = float(np.float32(o["target_threshold"]) * np.float32(o["search_multiplier"]))
        kw = dict(amp_min=0, amp_max=2000)
        rule = dict(min_clamp3=18, window=5, max_end_mismatch=0, ident_threshold=0.97)
        ids, rec, before = d.pool_products_end3(pool, thr, tm_floor=40.0, **rule, **kw)
        _, tm = d.pool_products_tm(pool, thr, tm_floor=40.0, **kw)
        _, variants, site_map = d.site_variants(pool, thr, site_map=True, thermo=False)
        _, sites = d.site_tm(pool, thr)
        want = HOST.host_end3(api.PRODUCT_END3_DTYPE, tm, sites, variants, site_map, HOST.oligo_lengths(pool, ids), **rule)
        print("dense 4k: %d sites, %d products past the floor, %d kept" % (len(sites), before, len(rec)))
        assert before == len(tm) and 0 < len(rec) < before
        assert any(dn.dense[0] == s for s in rec["sequence"].tolist())
        _equal(rec, want)
    finally:
        d.close()
