"""pcr_pool_conflicts_ext / Screener.pool_conflicts(ext_min_run=...) on the GPU: every record against conflict_ext_cases (the
oracle's products, whole-oligo dimers and 3'-anchored cells joined by a plain loop), every field and every float as bits;
against pcr_pool_conflicts_end3 and pcr_pool_dimers_end3 on the same device; caps, order, state and resources; and the wrapper
down to tubes."""
import bisect
import ctypes as C
import random

import numpy as np
import pytest

import conflict_ext_cases as X
import dimer_end3_cases as DE
import pool_conflict_cases as CC
import pool_dimer_cases as DC
import pool_rule_cases as R
import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W
from testdata import rand_seq

pytestmark = pytest.mark.gpu

PCR_ERR_STATE = -3
GUARD = 4                                        # poisoned records behind the output buffer
POISON_BYTE = 0xA5
BASE_NAMES = list(api.POOL_CONFLICT_DTYPE.names)
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _load(d, oracle, case):
    """The scenario's sequences and word DB on the device; the DB must be the one the oracle expects."""
    d.load_texts(case["seqs"])
    if case.get("active") is not None:
        d.set_active(case["active"])
    assert case["select"] == "all" and not case.get("splits")
    d.select_sites(case["panel"], SC.SQ(case["thr"]))
    assert d.entries() == SC.db_of(oracle, case)


def _raw(d, case, tm_floor=0.0, rule=X.NO_DIMERS, dimer_floor=0.0, ext=None, cap=None, end3=None, call="ext"):
    """The C call with a poisoned, guarded buffer of `cap` records (None: all n(n + 1)/2 cells).  ext: None or (rule, min_run,
    min_extension, dg_max or None); end3: None or an End3Rule's five fields; call = "end3": pcr_pool_conflicts_end3 instead.
    -> (return value, oligo ids, the cap records, the guard)"""
    panel = case["panel"]
    n_pool = len(panel)
    a = W.pairs_array(panel)
    cond = SC.conditions_of(case)
    args = api.ThermoArgs(cond["salt"], cond["primer_strand"], 0.0, 0.0, 0.0, 0.0)
    lo, hi = PC.amp_of(case)
    if cap is None:
        cap = n_pool * (n_pool + 1) // 2
    ids = np.zeros(max(2 * n_pool, 1), np.uint32)
    buf = np.zeros(cap + GUARD, api.POOL_CONFLICT_EXT_DTYPE if call == "ext" else api.POOL_CONFLICT_DTYPE)
    buf.view(np.uint8)[:] = POISON_BYTE
    rs = None if end3 is None else api.End3Rule(*end3)
    xs = None if ext is None else api.DimerEnd3Args(ext[0], ext[1], ext[2], INF if ext[3] is None else ext[3])
    head = [d.h, api.TARGET, a.ctypes.data, n_pool, float(case["thr"]), lo, hi, C.byref(args), float(case.get("template_strand", 0.0)),
            float(tm_floor), None if rs is None else C.byref(rs), int(rule), float(dimer_floor)]
    tail = [ids.ctypes.data, buf.ctypes.data if cap else None, cap]
    if call == "ext":
        n = d.L.pcr_pool_conflicts_ext(*head, None if xs is None else C.byref(xs), *tail)
    else:
        n = d.L.pcr_pool_conflicts_end3(*head, *tail)
    return n, ids[:2 * n_pool].tolist(), buf[:cap], buf[cap:]


def _clean(guard):
    return bool((guard.view(np.uint8) == POISON_BYTE).all())


def _same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, k, a, b)
    assert len(got) == len(want), (what, len(got), len(want))


def _check(d, oracle, name, rule=X.NO_DIMERS, dimer_floor=0.0, ext=None, tm_floor=0.0):
    """One call against the expectation -> the device's records."""
    case = X.scenario(oracle, name)
    want_ids, want = X.expected(oracle, name, tm_floor, rule, dimer_floor, ext)
    n, ids, rec, guard = _raw(d, case, tm_floor, rule, dimer_floor, ext)
    assert n == len(want) and ids == want_ids, (name, rule, dimer_floor, ext, n, len(want))
    _same(X.as_bits(rec[:n]), want, (name, rule, dimer_floor, ext))
    assert (rec[n:].view(np.uint8) == POISON_BYTE).all() and _clean(guard)
    return rec[:n]


def _base_of(rec):
    """The first 48 bytes of every 96-byte record as pcr_pool_conflict records."""
    out = np.zeros(len(rec), api.POOL_CONFLICT_DTYPE)
    for f in BASE_NAMES:
        out[f] = rec[f]
    assert out.tobytes() == np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 96)[:, :48].tobytes()
    return out


def _ext_bytes(rec):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 96)[:, 48:]


# ------------------------------------------------------------------ 1. ext = NULL
def test_without_ext_the_call_is_conflicts_end3(dev, oracle):
    name, product_rule = R.triples_of(oracle, "conflicts")[0]
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    r = product_rule
    rules = (None, (0, 0, 0, 0, 0.0), (r["min_clamp3"], r["window"], r["max_end_mismatch"], r["use_taq_mama"], r["ident_threshold"]))
    sizes = set()
    for end3 in rules:
        for rule, floor in ((X.NO_DIMERS, 0.0), (X.POOL, 0.0), (X.POOL, 30.0)):
            n0, ids0, rec0, g0 = _raw(dev, case, 0.0, rule, floor, end3=end3, call="end3")
            n1, ids1, rec1, g1 = _raw(dev, case, 0.0, rule, floor, ext=None, end3=end3)
            assert n0 == n1 >= 0 and ids0 == ids1 and _clean(g0) and _clean(g1), (end3, rule, floor)
            assert _base_of(rec1[:n1]).tobytes() == rec0[:n0].tobytes(), (end3, rule, floor)
            assert not _ext_bytes(rec1[:n1]).any() and (rec1[n1:].view(np.uint8) == POISON_BYTE).all()
            sizes.add((end3 is rules[2], rule, floor, n1))
    assert len({s[3] for s in sizes}) > 1                                       # the rule and the floor change the record set
    _, plain = dev.pool_conflicts(case["panel"], case["thr"], dimers="pool")    # the wrapper without the keyword: as ever
    assert plain.dtype == api.POOL_CONFLICT_DTYPE


# ------------------------------------------------------------------ 2. a pair that only extends
def test_planted_pair_appears_only_through_ext(dev, oracle):
    case = X.scenario(oracle, "x_planted")
    _load(dev, oracle, case)
    ext = X.PLANT_EXT + (None,)
    assert _raw(dev, case)[0] == 0 and _raw(dev, case, rule=X.POOL, dimer_floor=40.0)[0] == 0   # no product, no Tm dimer at 40 C
    for rule, floor in ((X.NO_DIMERS, 0.0), (X.POOL, 40.0)):
        rec = _check(dev, oracle, "x_planted", rule, floor, ext)
        p = rec[(rec["row_a"] == 0) & (rec["row_b"] == 1)]
        assert len(p) == 1 and p[0]["products"] == 0 and p[0]["melt"] == api.ANNEAL_NO_PRODUCT and p[0]["flags"] == api.CONFLICT_EXTENSION
        assert (p[0]["ext_query"], p[0]["ext_target"], p[0]["ext_run"], p[0]["ext_extension"]) == (0, 2, X.PLANT_RUN, X.PLANT_AT)
        assert (rec["flags"] == api.CONFLICT_EXTENSION).all() and (rec["ext_cells"] > 0).all()
    _check(dev, oracle, "x_planted", X.POOL, 0.0, ext)                          # every cell, the dimer fields beside the ext ones
    _check(dev, oracle, "x_planted", X.ASSAY, 20.0, (X.ASSAY, 4, 0, -2.0))


# ------------------------------------------------------------------ 3. repeats in the list of eight
def test_repeated_cells_count_once(dev, oracle):
    case = X.scenario(oracle, "x_repeats")
    _load(dev, oracle, case)
    for rule in (X.NO_DIMERS, X.POOL):
        rec = _check(dev, oracle, "x_repeats", rule, 0.0, X.REPEAT_EXT + (None,))
    ids = X.scenario_ids(oracle, "x_repeats")
    cell_of = X.ext_cells_of(oracle, "x_repeats", *X.REPEAT_EXT)
    seen = set()
    for r in rec:
        a, b = int(r["row_a"]), int(r["row_b"])
        assert (int(r["ext_cells"]), int(r["ext_placements"])) == X.ext_half_brute(ids, a, b, cell_of, None), (a, b)
        seen.add((a, b))
    assert {(0, 0), (1, 1), (0, 1), (0, 2), (0, 3), (0, 4), (3, 4)} <= seen     # a = b, F = R, a shared oligo, a repeated and an exchanged row
    assert all(X.has_repeats(ids, a, b) for a, b in seen)
    same = lambda p, q: X.as_bits(rec[(rec["row_a"] == p[0]) & (rec["row_b"] == p[1])])[0][2:] == \
        X.as_bits(rec[(rec["row_a"] == q[0]) & (rec["row_b"] == q[1])])[0][2:]
    assert same((0, 0), (0, 3)) and same((0, 0), (3, 4)) and same((0, 2), (2, 4))   # rows 3 and 4 are row 0 again


# ------------------------------------------------------------------ 4. a tie across cells
def test_the_lowest_cell_wins_a_tie(dev, oracle):
    case = X.scenario(oracle, "x_tie")
    _load(dev, oracle, case)
    rec = _check(dev, oracle, "x_tie", X.NO_DIMERS, 0.0, X.TIE_EXT + (None,))
    r = rec[(rec["row_a"] == 0) & (rec["row_b"] == 1)][0]
    assert (r["ext_query"], r["ext_target"], r["ext_run"], r["ext_extension"]) == (0, 2, 4, 3) and r["ext_cells"] >= 2
    _, cells = dev.pool_dimers_end3(case["panel"], min_run=4, min_extension=1, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, rule="pool")
    two = cells[(cells["query_oligo"] == 0) & (cells["target_oligo"] >= 2)]
    assert len(two) == 2 and DE.cells_as_bits(two[:1])[0][11:] == DE.cells_as_bits(two[1:])[0][11:]   # the device's two cells tie too
    # exchanging T1 and T2 moves the winner to the other oligo: still the lowest (q, t)
    swapped = dict(case, panel=[case["panel"][0], (case["panel"][1][1], case["panel"][1][0])])
    n, ids, rec2, guard = _raw(dev, swapped, ext=X.TIE_EXT + (None,))
    r2 = rec2[:n][(rec2[:n]["row_a"] == 0) & (rec2[:n]["row_b"] == 1)][0]
    assert (r2["ext_query"], r2["ext_target"], r2["ext_extension"]) == (0, 2, 7) and CC.BITS(r2["ext_dG"]) == CC.BITS(r["ext_dG"])


# ------------------------------------------------------------------ 5. degenerate oligos
@pytest.mark.parametrize("rule", (X.POOL, X.ASSAY))
def test_degenerate_oligos(dev, oracle, rule):
    case = X.scenario(oracle, "x_degenerate")
    _load(dev, oracle, case)
    rec = _check(dev, oracle, "x_degenerate", X.NO_DIMERS, 0.0, X.DEGENERATE_EXT[rule] + (None,))
    assert len(rec) == 6 and rec["ext_placements"].max() > 100 and ((rec["ext_q_expansion"] > 0) & (rec["ext_t_expansion"] > 0)).any()
    other = X.ASSAY if rule == X.POOL else X.POOL
    _check(dev, oracle, "x_degenerate", other, 0.0, X.DEGENERATE_EXT[rule] + (-3.0,))   # dimer_rule and ext->rule are independent


# ------------------------------------------------------------------ 6. the dg_max filter
def test_dg_max_filter(dev, oracle):
    case = X.scenario(oracle, "x_repeats")
    _load(dev, oracle, case)
    ext = X.REPEAT_EXT
    dg = X.filter_dg(oracle, "x_repeats", ext)
    full = _check(dev, oracle, "x_repeats", X.NO_DIMERS, 0.0, ext + (None,))
    cut = _check(dev, oracle, "x_repeats", X.NO_DIMERS, 0.0, ext + (dg,))
    cut_d = _check(dev, oracle, "x_repeats", X.POOL, 0.0, ext + (dg,))
    key = lambda rec: set(zip(rec["row_a"].tolist(), rec["row_b"].tolist()))
    gone = key(full) - key(cut)
    assert gone and key(cut) < key(full) and len(cut_d) == 15
    for a, b in gone:                                                           # placements, none kept: a record only where the dimers keep it
        r = cut_d[(cut_d["row_a"] == a) & (cut_d["row_b"] == b)][0]
        assert r["ext_placements"] > 0 and r["ext_cells"] == 0 and not _ext_bytes(cut_d[(cut_d["row_a"] == a) & (cut_d["row_b"] == b)])[:, 8:].any()
        assert not r["flags"] & api.CONFLICT_EXTENSION
    low = _check(dev, oracle, "x_repeats", X.NO_DIMERS, 0.0, ext + (-30.0,))    # below every dG: the product half alone keeps cells
    assert len(low) and (low["products"] > 0).all() and (low["ext_cells"] == 0).all() and (low["ext_placements"] > 0).any()
    # +inf: every pair with a qualifying placement has a record
    ids = X.scenario_ids(oracle, "x_repeats")
    _, cells = dev.pool_dimers_end3(case["panel"], min_run=ext[1], min_extension=ext[2], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, rule="pool")
    have = set(zip(cells["query_oligo"].tolist(), cells["target_oligo"].tolist()))
    want = {(a, b) for a in range(5) for b in range(a, 5) if any(c in have for c in X.eight_cells(ids, a, b))}
    assert key(full) == want


# ------------------------------------------------------------------ 7. the device's own route
def test_pool40_against_the_two_calls_it_combines(dev, oracle):
    case = CC.scenario(oracle, "c_pool40")
    _load(dev, oracle, case)
    kw = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
    n_pool = len(case["panel"])
    for dimers, floor, xrule, dg in (("pool", 0.0, "pool", None), (None, 0.0, "assay", -2.0), ("assay", 35.0, "pool", -3.0)):
        ids, rec = dev.pool_conflicts(case["panel"], case["thr"], dimers=dimers, dimer_floor=floor, ext_min_run=4, ext_dg_max=dg, ext_rule=xrule, **kw)
        assert rec.dtype == api.POOL_CONFLICT_EXT_DTYPE
        ids0, all_base = dev.pool_conflicts(case["panel"], case["thr"], dimers=dimers if dimers else "pool", dimer_floor=0.0, **kw)
        ids1, base = dev.pool_conflicts(case["panel"], case["thr"], dimers=dimers, dimer_floor=floor, **kw)
        ids2, cells = dev.pool_dimers_end3(case["panel"], min_run=4, min_extension=1, rule=xrule, **kw)   # every cell with a placement
        assert ids.tolist() == ids0.tolist() == ids1.tolist() == ids2.tolist() and len(all_base) == n_pool * (n_pool + 1) // 2
        keeps = set(zip(base["row_a"].tolist(), base["row_b"].tolist()))
        by = {(r[0], r[1]): r for r in CC.as_bits(base)}
        for r in CC.as_bits(all_base):                                          # a cell the base call drops: its fields at floor 0, no dimer flag
            if (r[0], r[1]) not in by:
                by[(r[0], r[1])] = r[:6] + ((r[6], r[7], r[8]) if dimers else (0, 0, 0)) + (r[9] & ~CC.DIMER,) + r[10:]
        want = X.join(ids.tolist(), by, keeps, X.from_cells(cells), dg)
        _same(X.as_bits(rec), want, (dimers, floor, xrule, dg))
        kept_base = rec[[(a, b) in keeps for a, b in zip(rec["row_a"].tolist(), rec["row_b"].tolist())]]
        plain = _base_of(kept_base)
        plain["flags"] &= ~np.uint32(api.CONFLICT_EXTENSION)
        assert plain.tobytes() == base.tobytes()                                # c is Screener.pool_conflicts'
        assert (rec["ext_cells"] > 0).any() and (np.diff(rec["row_a"].astype(np.int64) * n_pool + rec["row_b"]) > 0).all()


# ------------------------------------------------------------------ 8. batches of cells and melt launches
def test_batch_boundaries(dev, oracle):
    limit = api.POOL_DIMER_END3_BATCH_DUPLEXES
    pool = DC.batches_pool(oracle, limit)
    P = DC.Pool(oracle, pool)
    n_pool, n = len(pool), P.n
    assert P.ids == list(range(2 * n_pool))                                     # all distinct: oligo k is in row k // 2
    D = [P.degeneracy(k) for k in range(n)]
    starts = DC.batch_starts(D, limit)
    assert len(starts) >= 3
    rng = random.Random(7301)
    dev.load_texts([rand_seq(rng, 200), rand_seq(rng, 200)])
    dev.select_sites(pool, SC.SQ(1.0))
    assert dev.entries() == []                                                  # no site, no product: the records come from ext alone
    kw = dict(salt=DC.SALT, primer_strand=DC.PRIMER_STRAND)
    ids, rec = dev.pool_conflicts(pool, 1.0, dimers=None, ext_min_run=3, ext_min_extension=1, ext_rule="assay", cap=n_pool * (n_pool + 1) // 2, **kw)
    ids2, cells = dev.pool_dimers_end3(pool, min_run=3, min_extension=1, rule="assay", **kw)
    assert ids.tolist() == ids2.tolist() == P.ids
    assert (rec["products"] == 0).all() and (rec["flags"] == api.CONFLICT_EXTENSION).all()
    # every pair against the device's own cells reduced on the host
    empty = {(a, b): (a, b, 0, 0, CC.NO_PRODUCT_BITS, 0, 0, 0, 0, 0, 0) for a in range(n_pool) for b in range(a, n_pool)}
    got = X.as_bits(rec)
    _same(got, X.join(P.ids, empty, set(), X.from_cells(cells), None), "device cells")
    # a sample against the oracle: pairs whose cells lie in different batches, beside the batch boundaries, around the launch cuts
    cell_no = cells["query_oligo"].astype(np.int64) * n + cells["target_oligo"]
    csum = np.concatenate([[0], np.cumsum(cells["n_placements"].astype(np.int64))])
    first_of = np.searchsorted(cell_no, starts + [n * n])
    per_batch = np.diff(csum[first_of])
    assert per_batch.max() > 2 * api.POOL_DIMER_END3_BATCH_JOBS, per_batch
    near = [s + k for s in starts[1:] for k in (-2, -1, 0, 1)]
    for b, f in enumerate(first_of[:-1]):
        for cut in range(api.POOL_DIMER_END3_BATCH_JOBS, int(per_batch[b]), api.POOL_DIMER_END3_BATCH_JOBS):
            k = int(np.searchsorted(csum, csum[f] + cut, side="right")) - 1
            near.extend(int(cell_no[i]) for i in (k, min(k + 1, len(cells) - 1)))
    pairs = {tuple(sorted((c // n // 2, c % n // 2))) for c in near}
    pairs = set(rng.sample(sorted(pairs), min(len(pairs), 24)))
    batch_of = lambda q, t: bisect.bisect_right(starts, q * n + t) - 1
    spread = lambda a, b: len({batch_of(q, t) for q, t in X.eight_cells(P.ids, a, b)})
    far = [(a, b) for a in range(0, n_pool, 7) for b in range(a, n_pool, 5) if spread(a, b) >= 2]
    assert len(far) >= 8 and max(spread(a, b) for a, b in far) >= 2
    pairs.update(rng.sample(far, 8))
    pairs.update({(0, 0), (0, n_pool - 1), (n_pool - 1, n_pool - 1)})
    need = sorted({c for a, b in pairs for c in X.eight_cells(P.ids, a, b)})
    want_cells, _ = DE.expected(oracle, P, X.ASSAY, 3, 1, cells=need, **kw)
    cell_of = {(r[0], r[1]): r for r in want_cells}
    want = X.join(P.ids, empty, set(), cell_of, None, pairs=pairs)
    mine = [g for g in got if (g[0], g[1]) in pairs]
    _same(mine, want, "oracle sample")
    assert len(want) > 20 and any(w[11] > 1 for w in want) and any(w[15] > 0 or w[16] > 0 for w in want)


# ------------------------------------------------------------------ 9. capacity, order, state
def test_capacity_order_and_state(oracle):
    case = X.scenario(oracle, "x_repeats")
    ext = X.REPEAT_EXT + (None,)
    want_ids, want = X.expected(oracle, "x_repeats", 0.0, X.NO_DIMERS, 0.0, ext)
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        assert _raw(d, case, ext=ext)[0] == PCR_ERR_STATE and "no word DB" in api._err(d.L)
        assert _raw(d, case, ext=None)[0] == PCR_ERR_STATE
        with pytest.raises(api.PcrError, match="pcr_pool_conflicts_ext: no word DB"):
            d.pool_conflicts(case["panel"], case["thr"], ext_min_run=3)
        _load(d, oracle, case)
        for cap in (0, len(want) - 1, len(want)):
            n, ids, rec, guard = _raw(d, case, ext=ext, cap=cap)
            assert n == len(want) and ids == want_ids and _clean(guard), cap
            if cap == len(want):
                _same(X.as_bits(rec), want, "cap")
                order = rec["row_a"].astype(np.int64) * len(case["panel"]) + rec["row_b"]
                assert (np.diff(order) > 0).all() and (rec["row_a"] <= rec["row_b"]).all()
        ids, rec = d.pool_conflicts(case["panel"], case["thr"], dimers=None, ext_min_run=3, cap=1)   # the wrapper takes the count and retries
        _same(X.as_bits(rec), want, "wrapper")
        ids, rec = d.pool_conflicts([], case["thr"], ext_min_run=3)             # n_pool = 0
        assert len(ids) == 0 and len(rec) == 0 and rec.dtype == api.POOL_CONFLICT_EXT_DTYPE
        one = dict(case, panel=case["panel"][:1])                               # n_pool = 1: the row against itself
        n, ids, rec, guard = _raw(d, one, ext=ext)
        assert n == 1 and ids == [0, 1] and X.as_bits(rec[:1])[0][2:] == want[0][2:] and _clean(guard)
        for word, kw in (("ext->min_run", dict(ext_min_run=2)), ("ext->min_extension", dict(ext_min_run=3, ext_min_extension=32)),
                         ("ext->dg_max", dict(ext_min_run=3, ext_dg_max=float("nan")))):
            with pytest.raises(api.PcrError, match=word):
                d.pool_conflicts(case["panel"], case["thr"], **kw)
        with pytest.raises(ValueError, match="ext_rule"):
            d.pool_conflicts(case["panel"], case["thr"], ext_min_run=3, ext_rule="panel")
        assert _raw(d, case, ext=ext)[0] == len(want)                           # the handle still works
    finally:
        d.close()


# ------------------------------------------------------------------ 10. determinism and resources
def test_determinism_resources_and_neighbours(oracle):
    case = CC.scenario(oracle, "c_pool40")
    held = api.live_resources()
    d = api.Screener(0)
    try:
        _load(d, oracle, case)
        kw = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
        others = lambda: (d.pool_conflicts(case["panel"], case["thr"], dimers="pool", **kw)[1].tobytes(),
                          d.pool_dimers_end3(case["panel"], min_run=3, placements=True, **kw)[2].tobytes(),
                          d.pool_dimers_end3(case["panel"], min_run=4, dg_max=-2.0, **kw)[1].tobytes(),
                          d.entries(), d.find_target_match(case["panel"], case["thr"]).tolist())
        before = others()
        a = _raw(d, case, rule=X.POOL, ext=(X.ASSAY, 3, 1, -1.0))
        b = _raw(d, case, rule=X.POOL, ext=(X.ASSAY, 3, 1, -1.0))
        assert a[0] == b[0] == 820 and a[2].tobytes() == b[2].tobytes() and (a[2]["ext_cells"] > 0).any()
        assert others() == before                                               # pool_conflicts, pool_dimers_end3 and a screen pass: unchanged
        c = _raw(d, case, rule=X.POOL, ext=(X.ASSAY, 3, 1, -1.0))
        assert c[2].tobytes() == a[2].tobytes()                                 # ... and the call after them
        assert api.live_resources()[0] > held[0]
    finally:
        d.close()
    assert api.live_resources() == held


# ------------------------------------------------------------------ 11. the wrapper, down to tubes
def test_extension_conflicts_to_tubes_end_to_end(oracle):
    case = X.scenario(oracle, "x_planted")
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        kw = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, select="all")
        ids, rec = d.pool_conflicts(case["panel"], case["thr"], dimers="pool", ext_min_run=X.PLANT_EXT[1], ext_dg_max=-5.0, **kw)
        assert d.entries() == SC.db_of(oracle, case)
        _same(X.as_bits(rec), X.expected(oracle, "x_planted", 0.0, X.POOL, 0.0, X.PLANT_EXT + (-5.0,))[1], "wrapper")
        tube, self_conflict = api.assign_tubes(api.conflict_matrix(rec, 3, max_dimer=40.0, max_extension_dg=-5.0))
        assert tube[0] != tube[1] and tube.max() == 1 and not self_conflict.any()   # A extends on C: rows 0 and 1 are split
        one, _ = api.assign_tubes(api.conflict_matrix(rec, 3, max_dimer=40.0))
        assert one.tolist() == [0, 0, 0]                                        # the whole-oligo Tm alone sees nothing
        _, plain = d.pool_conflicts(case["panel"], case["thr"], dimers="pool", **kw)
        assert api.assign_tubes(api.conflict_matrix(plain, 3, max_dimer=40.0))[0].tolist() == [0, 0, 0]
        with pytest.raises(ValueError, match="max_extension_dg"):
            api.conflict_matrix(plain, 3, max_extension_dg=-5.0)
        ids, only = d.pool_conflicts(case["panel"], case["thr"], dimers=None, ext_min_run=X.PLANT_EXT[1], ext_dg_max=-5.0, **kw)
        assert list(zip(only["row_a"].tolist(), only["row_b"].tolist())) == [(0, 1)]   # dimers=None: the one pair, through ext alone
    finally:
        d.close()
