"""pcr_pool_conflicts / Screener.pool_conflicts on the GPU: every record against pool_conflict_cases (the oracle's products and
dimer cells, the grouping restated with dictionaries and sets), every float as bits; against pcr_pool_products_tm,
pcr_pool_dimers and multiplex_compatible on the same device; the errors in their order; and the wrapper down to tubes."""
import ctypes as C
import random

import numpy as np
import pytest

import pool_conflict_cases as CC
import pool_dimer_cases as DC
import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

PCR_ERR_ARG, PCR_ERR_STATE, PCR_ERR_CAPACITY = -1, -3, -4
GUARD = 8                                        # poisoned records behind the output buffer
POISON_BYTE = 0xA5
RULES = {"pool": DC.POOL, "assay": DC.ASSAY}


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


def _raw(d, case, tm_floor=0.0, rule=CC.NO_DIMERS, dimer_floor=0.0, cap=None, which=api.TARGET, panel=None):
    """The C call with a poisoned, guarded buffer of `cap` records (None: all n(n + 1)/2 cells).
    -> (return value, oligo ids, the cap records, the guard)"""
    panel = case["panel"] if panel is None else panel
    n_pool = len(panel)
    a = W.pairs_array(panel)
    cond = SC.conditions_of(case)
    args = api.ThermoArgs(cond["salt"], cond["primer_strand"], 0.0, 0.0, 0.0, 0.0)
    lo, hi = PC.amp_of(case)
    if cap is None:
        cap = n_pool * (n_pool + 1) // 2
    ids = np.zeros(max(2 * n_pool, 1), np.uint32)
    buf = np.zeros(cap + GUARD, api.POOL_CONFLICT_DTYPE)
    buf.view(np.uint8)[:] = POISON_BYTE
    n = d.L.pcr_pool_conflicts(d.h, which, a.ctypes.data, n_pool, float(case["thr"]), lo, hi, C.byref(args),
                               float(case.get("template_strand", 0.0)), float(tm_floor), int(rule), float(dimer_floor),
                               ids.ctypes.data, buf.ctypes.data if cap else None, cap)
    return n, ids[:2 * n_pool].tolist(), buf[:cap], buf[cap:]


def _clean(guard):
    return bool((guard.view(np.uint8) == POISON_BYTE).all())


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, k, a, b)


def _check(d, oracle, name, tm_floor, rule=CC.NO_DIMERS, dimer_floor=0.0, which=api.TARGET):
    case = CC.scenario(oracle, name)
    want_ids, want = CC.expected(oracle, name, tm_floor, rule, dimer_floor)
    n, ids, rec, guard = _raw(d, case, tm_floor, rule, dimer_floor, which=which)
    assert n == len(want) and ids == want_ids, (name, tm_floor, n, len(want))
    _same(CC.as_bits(rec[:n]), want, (name, tm_floor, rule, dimer_floor))
    assert (rec[n:].view(np.uint8) == POISON_BYTE).all() and _clean(guard)
    return want


# ------------------------------------------------------------------ 1. every scenario against the expectation, at its floors
def _floors(oracle, name):
    rec = PC.all_products(oracle, name)[1]
    floors = CC.floors_of(rec)
    return floors if name != "c_pool40" else [floors[2], floors[3], 0.0]       # (the middle value, above it, none: the model takes a while)


@pytest.mark.parametrize("name", CC.ALL_SCENARIOS)
def test_scenario(dev, oracle, name):
    case = CC.scenario(oracle, name)
    _load(dev, oracle, case)
    sizes = set()
    for f in _floors(oracle, name):
        sizes.add(len(_check(dev, oracle, name, f)))
    # cap at 0, exact and one short: the count either way, nothing written past cap
    want_ids, want = CC.expected(oracle, name, 0.0)
    for cap in sorted({0, len(want), max(len(want) - 1, 0)}):
        n, ids, rec, guard = _raw(dev, case, 0.0, cap=cap)
        assert n == len(want) and ids == want_ids and _clean(guard), cap
        if cap == len(want):
            _same(CC.as_bits(rec), want, (name, "cap", cap))
    if name in ("random", "c_pool40"):
        assert len(sizes) > 1                                                  # the floor empties cells


def test_grouping_scenarios_show_their_case(oracle):
    """What each new scenario is there for, read off the expectation (no device)."""
    for name in CC.GROUPING_SCENARIOS:
        CC.scenario(oracle, name)
    cells = lambda name: {(r[0], r[1]): r for r in CC.expected(oracle, name)[1]}
    c = cells("c_shared")
    assert sorted(c) == [(0, 0), (0, 1), (1, 1)] and [c[k][2] for k in sorted(c)] == [1, 2, 1]
    c = cells("c_roles")
    assert sorted(c) == [(0, 0), (0, 1), (1, 1)] and c[(0, 1)][2] == 2
    c = cells("c_repeat")
    assert sorted(c) == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3)] and all(r[2] == 1 for r in c.values())
    c = cells("c_self_pair")
    assert sorted(c) == [(0, 1), (1, 1)] and c[(0, 1)][2:4] == (2, 2)
    c = cells("c_counts")
    assert list(c) == [(0, 1)] and c[(0, 1)][2:4] == (4, 2)
    c = cells("c_tie")
    assert c[(0, 1)][2:4] == (3, 3) and c[(0, 1)][5] == CC.TIE_SEQS[0]
    rec = PC.all_products(oracle, "c_tie")[1]
    top = [int(r["sequence"]) for r in rec if CC.BITS(CC.melt_value(r)) == c[(0, 1)][4]]
    assert sorted(top) == list(CC.TIE_SEQS)
    c = cells("c_wide")
    assert c[(0, 1)][2:4] == (3, 3) and sorted(int(r["sequence"]) for r in PC.all_products(oracle, "c_wide")[1]) == list(CC.WIDE_PRODUCT)
    assert cells("c_split_wide")[(0, 1)][3] == 2 and cells("c_split_inner")[(0, 1)][3] == 1
    assert cells("c_fanin")[(0, 1)][2:4] == (CC.FANIN_N, CC.FANIN_N)
    ids, rec = PC.all_products(oracle, "c_pool40")[:2]
    assert CC.attributions(ids, rec) > 65536


# ------------------------------------------------------------------ 2. the background set
@pytest.mark.parametrize("name", ["c_shared", "random"])
def test_background(oracle, name):
    case = CC.scenario(oracle, name)
    d = api.Screener(0)
    try:
        _load(d, oracle, case, which=api.BACKGROUND)
        f = CC.floors_of(PC.all_products(oracle, name)[1])[2]
        for floor in (0.0, f):
            _check(d, oracle, name, floor, which=api.BACKGROUND)
        assert _raw(d, case)[0] == PCR_ERR_STATE                                # the target set has no DB
    finally:
        d.close()


# ------------------------------------------------------------------ 3. dimers against the oracle's cells
@pytest.mark.parametrize("rule", ["pool", "assay"])
@pytest.mark.parametrize("name", ["c_repeat", "c_self_pair", "expansions_0", "ids"])
def test_dimers(dev, oracle, name, rule):
    case = CC.scenario(oracle, name)
    _load(dev, oracle, case)
    n_pool = len(case["panel"])
    want = _check(dev, oracle, name, 0.0, RULES[rule], 0.0)
    assert len(want) == n_pool * (n_pool + 1) // 2                              # dimer_floor <= 0: every cell
    assert len(_check(dev, oracle, name, 0.0, RULES[rule], -5.0)) == len(want)
    assert all(r[9] & CC.DIMER for r in want)
    # a floor exactly at a cell's value keeps it, nextafter above drops it (unless it has a product)
    tms = sorted({float(CC.F32(r[6])) for r in want})
    at = np.float32(tms[len(tms) // 2] if tms[len(tms) // 2] > 0 else tms[-1])
    if at > 0:
        above = np.nextafter(at, np.float32(np.inf))
        keep_at = _check(dev, oracle, name, 0.0, RULES[rule], float(at))
        keep_above = _check(dev, oracle, name, 0.0, RULES[rule], float(above))
        hit = lambda rows: {(r[0], r[1]) for r in rows if r[9] & CC.DIMER}
        assert hit(keep_at) - hit(keep_above) == {(r[0], r[1]) for r in want if CC.F32(r[6]) == at} != set()


def test_no_dimers_leaves_the_fields_zero(dev, oracle):
    case = CC.scenario(oracle, "random")
    _load(dev, oracle, case)
    n, ids, rec, guard = _raw(dev, case)
    assert n == 21 and not rec["dimer_tm"].view(np.uint32).any() and not rec["dimer_query"].any() and not rec["dimer_target"].any()
    assert (rec["flags"] == CC.PRODUCT).all() and not rec["reserved"].any()


# ------------------------------------------------------------------ 4. dimers against pcr_pool_dimers and multiplex_compatible on the device
def _dimer_reduction(d, panel, rule):
    """-> (a, b) -> (tm bits, q, t) from the full matrix of pool_dimers, reduced in numpy."""
    ids, cells = d.pool_dimers(panel, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, rule=rule, tm_floor=0.0)
    n_ol = int(ids.max()) + 1
    m = api.Screener.dimer_matrix(cells, n_ol)
    out = {}
    for a in range(len(panel)):
        for b in range(a, len(panel)):
            qt = np.array(CC.dimer_cells_of(ids.tolist(), a, b))
            v = m[qt[:, 0], qt[:, 1]]
            k = int(np.argmax(v))                                               # the first maximum: qt is sorted
            out[(a, b)] = (CC.BITS(v[k]), int(qt[k, 0]), int(qt[k, 1]))
    return out


@pytest.mark.parametrize("rule", ["pool", "assay"])
@pytest.mark.parametrize("pool_name", ["rules", "expansions", "c_pool40"])
def test_dimers_are_pool_dimers_reduced(dev, oracle, pool_name, rule):
    case = CC.scenario(oracle, "c_shared")
    _load(dev, oracle, case)
    panel = {"rules": DC.rules_pool, "expansions": DC.expansions_pool, "c_pool40": lambda o: CC.scenario(o, "c_pool40")["panel"]}[pool_name](oracle)
    want = _dimer_reduction(dev, panel, rule)
    n, ids, rec, guard = _raw(dev, case, rule=RULES[rule], panel=panel)
    assert n == len(want) == len(panel) * (len(panel) + 1) // 2 and _clean(guard)
    got = {(int(r["row_a"]), int(r["row_b"])): (CC.BITS(r["dimer_tm"]), int(r["dimer_query"]), int(r["dimer_target"])) for r in rec}
    assert got == want


def test_dimer_tm_decides_multiplex_compatible(dev, oracle):
    case = CC.scenario(oracle, "c_shared")
    _load(dev, oracle, case)
    panel = DC.rules_pool(oracle)
    n, ids, rec, guard = _raw(dev, case, rule=DC.POOL, panel=panel)
    tm = {(int(r["row_a"]), int(r["row_b"])): np.float32(r["dimer_tm"]) for r in rec}
    pairs = [(min(a, b), max(a, b)) for a, b in DC.RULES_PAIRS]                 # two different assays each
    values = sorted({float(tm[p]) for p in pairs})
    assert values[-1] > 0
    limits = [40.0, values[-1], float(np.nextafter(np.float32(values[-1]), np.float32(np.inf))), values[len(values) // 2],
              float(np.nextafter(np.float32(values[len(values) // 2]), np.float32(np.inf)))]
    A, B = [panel[a] for a, _ in pairs], [panel[b] for _, b in pairs]
    for limit in limits:
        ab = dev.multiplex_compatible(A, B, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, max_dimer=limit)
        ba = dev.multiplex_compatible(B, A, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, max_dimer=limit)
        want = [bool(tm[p] < np.float32(limit)) for p in pairs]
        assert (ab & ba).tolist() == want, limit


def test_no_dimers_runs_where_pool_dimers_refuses_the_size(dev, oracle):
    case = CC.scenario(oracle, "c_shared")
    _load(dev, oracle, case)
    rng = random.Random(6201)
    txt = set()
    while len(txt) < 184:                                                       # 184 oligos x 256 expansions: 47 104 squared > 2^31 duplexes
        txt.add("".join(rng.choice("ACGT") for _ in range(4)) + "NNNN" + "".join(rng.choice("ACGT") for _ in range(11)))
    big = DC._pairs(oracle, sorted(txt))
    with pytest.raises(api.PcrError, match="2\\^31"):
        dev.pool_dimers(big, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
    assert _raw(dev, case, rule=DC.POOL, panel=big)[0] == PCR_ERR_CAPACITY
    n, ids, rec, guard = _raw(dev, case, panel=big)
    assert n >= 0 and len(set(ids)) == 184 and _clean(guard)
    got = CC.as_bits(rec[:n])
    assert all(r[6:9] == (0, 0, 0) and r[9] == CC.PRODUCT for r in got)


# ------------------------------------------------------------------ 5. against pcr_pool_products_tm on the same handle
def _group(ids, rec):
    """pool_products_tm's records -> (a, b) -> (products, sequences, melt bits, melt_sequence), in numpy."""
    n_pool = len(ids) // 2
    sp = rec[rec["intended"] == 0]
    v = np.minimum(sp["tm_plus"], sp["tm_minus"]) + np.float32(0.0)
    has = np.zeros((n_pool, int(ids.max()) + 1), bool)
    has[np.arange(n_pool), ids[0::2]] = True
    has[np.arange(n_pool), ids[1::2]] = True
    out = {}
    for a in range(n_pool):
        xa, ya = has[a][sp["plus_oligo"]], has[a][sp["minus_oligo"]]
        for b in range(a, n_pool):
            sel = (xa & has[b][sp["minus_oligo"]]) | (has[b][sp["plus_oligo"]] & ya)
            if sel.any():
                vs, ss = v[sel], sp["sequence"][sel]
                out[(a, b)] = (int(sel.sum()), len(np.unique(ss)), CC.BITS(vs.max()), int(ss[vs == vs.max()].min()))
    return out


@pytest.mark.parametrize("name", ["random", "c_pool40"])
def test_products_are_pool_products_tm_grouped(dev, oracle, name):
    case = CC.scenario(oracle, name)
    _load(dev, oracle, case)
    lo, hi = PC.amp_of(case)
    v = np.unique(PC.min_tm(PC.all_products(oracle, name)[1]))
    v = v[v > 0]
    for floor in (0.0, float(v[len(v) // 2]), float(v[(3 * len(v)) // 4])):
        ids, rec = dev.pool_products_tm(case["panel"], case["thr"], tm_floor=floor, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND,
                                        amp_min=lo, amp_max=hi, cap=1 << 17)
        want = _group(ids, rec)
        n, got_ids, got, guard = _raw(dev, case, floor)
        assert got_ids == ids.tolist() and n == len(want) and _clean(guard)
        have = {(int(r["row_a"]), int(r["row_b"])): (int(r["products"]), int(r["sequences"]), CC.BITS(r["melt"]), int(r["melt_sequence"]))
                for r in got[:n]}
        assert have == want, floor


# ------------------------------------------------------------------ 6. errors, in their order
def _call(d, h, which, panel, n_pool, args, template_strand, tm_floor, rule, dimer_floor, ids, out, cap, thr=0.95):
    a = W.pairs_array(panel) if panel is not None else None
    return d.L.pcr_pool_conflicts(h, which, a.ctypes.data if a is not None else None, n_pool, thr, 80, 200,
                                  C.byref(args) if args is not None else None, template_strand, tm_floor, rule, dimer_floor,
                                  ids.ctypes.data if ids is not None else None, out.ctypes.data if out is not None else None, cap)


def test_argument_errors_in_order(dev, oracle):
    case = CC.scenario(oracle, "c_shared")
    _load(dev, oracle, case)
    good = case["panel"]
    ids, out = np.zeros(8, np.uint32), np.zeros(8, api.POOL_CONFLICT_DTYPE)
    ok_args = lambda: api.ThermoArgs(SC.SALT, SC.PRIMER_STRAND, 0.0, 0.0, 0.0, 0.0)
    bad_salt = api.ThermoArgs(2.0, SC.PRIMER_STRAND, 0.0, 0.0, 0.0, 0.0)
    bad_salt_neg = api.ThermoArgs(2.0, -1.0, 0.0, 0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")
    degenerate = [(SC.too_degenerate_oligo(oracle), good[0][1])]
    # every call breaks one rule and every later one: the message names the earliest
    steps = [
        ("unknown sequence set", dict(which=7, panel=None, n_pool=1, args=None)),
        ("PCR_SET_MULTIPLEX", dict(which=api.MULTIPLEX, panel=None, n_pool=1, args=None)),
        ("bad argument", dict(panel=None, n_pool=1, args=None)),
        ("bad argument", dict(n_pool=2000, ids=None, args=bad_salt_neg)),
        ("bad argument", dict(n_pool=2, out=None, cap=4, args=bad_salt_neg)),
        ("PCR_POOL_MAX_PAIRS", dict(panel=good * 513, n_pool=1026, ids=np.zeros(4096, np.uint32), args=bad_salt_neg)),
        ("negative strand", dict(args=bad_salt_neg, tm_floor=nan)),
        ("negative strand", dict(template_strand=-1.0, args=bad_salt, tm_floor=nan)),
        ("salt outside", dict(args=bad_salt, panel=degenerate, n_pool=1, tm_floor=nan)),
        ("PCR_SITE_MAX_EXPANSIONS", dict(panel=degenerate, n_pool=1, tm_floor=nan, rule=5)),
        ("strand concentration of an oligo's duplex is zero", dict(args=api.ThermoArgs(SC.SALT, 0.0, 0.0, 0.0, 0.0, 0.0), tm_floor=nan, rule=5)),
        ("tm_floor is not finite", dict(tm_floor=nan, rule=5, dimer_floor=inf)),
        ("tm_floor is not finite", dict(tm_floor=inf, rule=5, dimer_floor=inf)),
        ("unknown dimer_rule", dict(rule=5, dimer_floor=inf, h=None)),
        ("unknown dimer_rule", dict(rule=2, dimer_floor=nan, h=None)),
        ("dimer_floor is not finite", dict(rule=DC.POOL, dimer_floor=inf, h=None)),
        ("dimer_floor is not finite", dict(rule=CC.NO_DIMERS, dimer_floor=nan, h=None)),
        ("primer_strand must be positive", dict(rule=DC.ASSAY, args=api.ThermoArgs(SC.SALT, 0.0, 0.0, 0.0, 0.0, 0.0), template_strand=1e-6, h=None)),
        ("null handle", dict(h=None)),
        ("null handle", dict(h=None, rule=DC.POOL)),
    ]
    for message, change in steps:
        kw = dict(h=dev.h, which=api.TARGET, panel=good, n_pool=2, args=ok_args(), template_strand=0.0, tm_floor=0.0,
                  rule=CC.NO_DIMERS, dimer_floor=0.0, ids=ids, out=out, cap=8)
        kw.update(change)
        rc = _call(dev, **kw)
        assert rc == PCR_ERR_ARG and message in api._err(dev.L), (message, change, rc, api._err(dev.L))
    # an empty oligo (a word with no base) comes with the oligos
    empty = W.pairs_array(good).copy()
    empty.view(np.uint8)[:16] = 0
    args = ok_args()
    rc = dev.L.pcr_pool_conflicts(dev.h, api.TARGET, empty.ctypes.data, 2, 0.95, 80, 200, C.byref(args), 0.0, nan, 5, inf,
                                  ids.ctypes.data, out.ctypes.data, 8)
    assert rc == PCR_ERR_ARG and "empty or has a hole" in api._err(dev.L)
    # the 0-strand case with a template strand is legal without dimers
    args = api.ThermoArgs(SC.SALT, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert _call(dev, dev.h, api.TARGET, good, 2, args, 1e-6, 0.0, CC.NO_DIMERS, 0.0, ids, out, 8) >= 0


def test_state_small_pools_and_an_empty_db(oracle):
    case = CC.scenario(oracle, "c_shared")
    held = api.live_resources()
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        assert _raw(d, case)[0] == PCR_ERR_STATE and "no word DB" in api._err(d.L)
        assert _raw(d, case, rule=DC.POOL)[0] == PCR_ERR_STATE                  # also when only dimers would give records
        with pytest.raises(api.PcrError, match="no word DB"):
            d.pool_conflicts(case["panel"], case["thr"])
        _load(d, oracle, case)
        before = (d.entries(), d.find_target_match(case["panel"], case["thr"]).tolist())
        ids, rec = d.pool_conflicts([], case["thr"])                            # n_pool = 0
        assert len(ids) == 0 and len(rec) == 0 and rec.dtype == api.POOL_CONFLICT_DTYPE
        one = case["panel"][:1]                                                 # n_pool = 1: the A-A product, the row against itself
        ids, rec = d.pool_conflicts(one, case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, dimers=None)
        assert ids.tolist() == [0, 1] and CC.as_bits(rec)[0][:4] == (0, 0, 1, 1) and len(rec) == 1
        ids, rec = d.pool_conflicts(one, case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, dimers="assay")
        _, cells = d.pool_dimers(one, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, rule="assay")
        assert len(rec) == 1 and int(rec[0]["flags"]) == 3 and CC.BITS(rec[0]["dimer_tm"]) == CC.BITS(cells["tm_max"].max())
        a = d.pool_conflicts(case["panel"], case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, dimers="pool")
        b = d.pool_conflicts(case["panel"], case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, dimers="pool")
        assert a[1].tobytes() == b[1].tobytes() and len(a[1]) == 3              # two runs, the same bytes
        assert before == (d.entries(), d.find_target_match(case["panel"], case["thr"]).tolist())
        with pytest.raises(ValueError):
            d.pool_conflicts(case["panel"], dimers="some")
        with pytest.raises(ValueError):
            d.pool_conflicts(case["panel"], select="some")
        # an empty DB: no product anywhere, the dimers still answer
        rng = random.Random(6202)
        other = DC._pairs(oracle, [DC._plain(rng, 21) for _ in range(4)])
        d.select_sites(other, SC.SQ(1.0))
        assert d.entries() == []
        ids, rec = d.pool_conflicts(other, 1.0, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, dimers=None)
        assert len(rec) == 0
        ids, rec = d.pool_conflicts(other, 1.0, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, dimers="pool")
        assert len(rec) == 3 and not rec["products"].any() and (rec["flags"] == CC.DIMER).all()
        assert rec["melt"].view(np.uint32).tolist() == [CC.NO_PRODUCT_BITS] * 3
        assert api.live_resources()[0] > held[0]
    finally:
        d.close()
    assert api.live_resources() == held


def test_determinism(dev, oracle):
    case = CC.scenario(oracle, "c_pool40")
    _load(dev, oracle, case)
    a = _raw(dev, case, rule=DC.POOL)
    b = _raw(dev, case, rule=DC.POOL)
    assert a[0] == b[0] == 820 and a[2].tobytes() == b[2].tobytes()


# ------------------------------------------------------------------ 7. the wrapper, down to tubes
def test_conflicts_to_tubes_end_to_end(oracle):
    case = CC.scenario(oracle, "random")
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        lo, hi = PC.amp_of(case)
        kw = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, amp_min=lo, amp_max=hi)
        ids, rec = d.pool_conflicts(case["panel"], case["thr"], select="all", dimers="pool", **kw)
        assert d.entries() == SC.db_of(oracle, case) and len(rec) == 21
        _same(CC.as_bits(rec), CC.expected(oracle, "random", 0.0, DC.POOL, 0.0)[1], "wrapper")
        melts = np.sort(rec["melt"][rec["row_a"] != rec["row_b"]])
        anneal = float(melts[len(melts) // 2])                                  # half of the off-diagonal cells still conflict
        m = api.conflict_matrix(rec, len(case["panel"]), anneal=anneal, max_dimer=40.0)
        tube, self_conflict = api.assign_tubes(m)
        assert 1 < tube.max() + 1 <= len(case["panel"]) and self_conflict.tolist() == m.diagonal().tolist()
        _, prod = d.pool_products_tm(case["panel"], case["thr"], tm_floor=anneal, cap=1 << 14, **kw)
        rows = CC.rows_of(ids.tolist())
        for r in prod[prod["intended"] == 0]:
            for i, j in CC.cells_of_product(rows, r["plus_oligo"], r["minus_oligo"]):
                assert i == j or tube[i] != tube[j], (i, j)
    finally:
        d.close()
