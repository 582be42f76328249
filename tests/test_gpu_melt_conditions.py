"""Per-site melting on the GPU away from 50 mM, 0.9 uM and two-fold codes: melt_condition_cases' scenarios through pcr_site_tm
and the pool entry points built on the same melt stage, every record against the oracle's expectation at the scenario's own
salt and concentrations with every float as bits, and a sequence of calls on one handle whose salts alternate.  The
comparisons are the entry points' own: the helpers of their test files, which read a scenario's conditions from its keys."""
import numpy as np
import pytest

import anneal_profile_cases as AC
import melt_condition_cases as MC
import pool_conflict_cases as CC
import pool_dimer_cases as DC
import probe_hit_cases as H
import products_tm_cases as PC
import site_tm_cases as SC
import site_variant_cases as VC
import test_gpu_anneal_profile as T_ANNEAL
import test_gpu_pool_conflicts as T_CONFLICTS
import test_gpu_probe_hits as T_HITS
import test_gpu_products_tm as T_PRODUCTS
import test_gpu_site_repair as T_REPAIR
import test_gpu_site_tm as T_SITES
import test_gpu_site_variants as T_VARIANTS
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codes_dev(oracle):
    """A handle holding codes_case and its word DB, selected once."""
    d = api.Screener(0)
    T_SITES._load(d, oracle, MC.codes_case(oracle))
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


# ------------------------------------------------------------------ 1. three-fold codes at every condition
@pytest.mark.parametrize("cond", MC.conditions(), ids=MC.condition_id)
def test_codes_at_every_condition(codes_dev, oracle, cond):
    """One call of pcr_site_tm: every expansion of the 24-, 9-, 27- and 24-fold oligos and 16 of the 243-fold one on a site of its
    own (tests/test_melt_conditions_host.py: a dropped or doubled expansion changes a record), 5 850 jobs."""
    case = MC.at(MC.codes_case(oracle), cond)
    ids, rec, n_jobs = T_SITES._compare(codes_dev, oracle, case)
    assert ids.tolist() == [0, 1, 2, 3, 4, 4]
    assert n_jobs == MC.CODES_JOBS == int(rec["n_expansions"].sum()) and len(rec) == MC.CODES_SITES
    for o, d in enumerate(MC.DEGENERACIES):
        mine = rec[rec["oligo"] == o]
        assert len(mine) == len(case["planted"][o]) and (mine["n_expansions"] == d).all()
    assert not rec["flags"].any() and (rec["tm_min"] > 0).all()


# ------------------------------------------------------------------ 2. the pool entry points at three conditions
def _differs(a, b):
    assert len(a) == len(b) and a != b
    return True


@pytest.mark.parametrize("k", range(len(MC.POOL_NAMES)))
def test_pool_consumers_at_conditions(dev, oracle, k):
    name = MC.register_pool(oracle)[k]
    case, default = PC.scenario(oracle, name), MC.POOL_DEFAULT
    cond = MC.POOL_CONDITIONS[k]
    assert (case["salt"], case["primer_strand"], case["template_strand"]) == cond
    T_PRODUCTS._load(dev, oracle, case)
    # pool_products_tm, with bits: no floor, and a floor from the oracle's records that keeps some products and drops others
    everything = PC.all_products(oracle, name)[1]
    assert _differs(PC.as_bits(everything), PC.as_bits(PC.all_products(oracle, default)[1]))
    floor = PC.floors_of(everything)[2]
    assert 0 < len(PC.kept(everything, floor)) < len(everything)
    _, rec, _, _ = T_PRODUCTS._compare(dev, oracle, name, 0.0)
    assert len(rec) == len(everything)
    _, rec, _, _ = T_PRODUCTS._compare(dev, oracle, name, floor)
    assert len(rec) == len(PC.kept(everything, floor))
    # anneal_profile over temperatures bracketing the expected melt values
    temps = AC.temps_of(everything)
    v = AC.melt_values(everything)
    assert temps[0] < 0 and temps[-1] > v.max() and (temps > 0).sum() >= 3 and temps[temps > 0][0] < v[v > 0].min()
    assert _differs(AC.as_words(AC.expected(oracle, name, temps)[2]), AC.as_words(AC.expected(oracle, default, temps)[2]))
    n, out, guards = T_ANNEAL._raw(dev, case, temps)
    assert n == len(everything)
    T_ANNEAL._check(oracle, name, temps, out["ids"], out["points"], out["pair_seq"], out["fr"], out["rf"], out["spur"])
    assert all((g.view(np.uint8) == T_ANNEAL.POISON_BYTE).all() for g in guards.values())
    # pool_conflicts: with the pool's dimers at the same salt and concentration, and without at the floor
    assert _differs(CC.expected(oracle, name, 0.0, DC.POOL)[1], CC.expected(oracle, default, 0.0, DC.POOL)[1])
    want = T_CONFLICTS._check(dev, oracle, name, 0.0, DC.POOL, 0.0)
    assert len(want) == 21 and any(r[9] & CC.PRODUCT for r in want)
    T_CONFLICTS._check(dev, oracle, name, floor)
    # site_variants (and, in its helper, site_tm on the same handle)
    assert _differs(VC.as_bits(VC.expectation(oracle, case)[1]), VC.as_bits(VC.expectation(oracle, PC.scenario(oracle, default))[1]))
    var, _, sites, _ = T_VARIANTS._compare(dev, oracle, case)
    assert 3 in var["n_expansions"] and 3 in sites["n_expansions"]
    # probe_hits: two pairs, the next pair's F as their probe (one of them three-fold), on the DB that holds the probes' sites
    pcase = H.scenario(oracle, name)
    assert pcase["probe_strand"] == MC.POOL_PROBE_STRAND and (pcase["salt"], pcase["primer_strand"], pcase["template_strand"]) == cond
    T_HITS._load(dev, oracle, pcase)
    hits = H.everything(oracle, name)[4]
    assert _differs(H.as_bits(hits), H.as_bits(H.everything(oracle, default)[4]))
    pairs = H.floor_pairs(oracle, name)
    seen = set()
    for tm_floor, probe_tm_floor in (pairs[0], pairs[-2], pairs[-1]):
        want_ids, want_pid, want, want_detected = H.expectation(oracle, name, tm_floor, probe_tm_floor)
        ids, pid, rec, detected = T_HITS._run(dev, pcase, tm_floor, probe_tm_floor, bits=True)
        assert ids.tolist() == want_ids and pid.tolist() == want_pid
        T_HITS._equal(rec, want)
        assert detected.tolist() == want_detected.tolist()
        seen.add(len(rec))
    assert len(hits) in seen and len(seen) >= 2


# ------------------------------------------------------------------ 3. the salt changes between calls on one handle
def _bytes(out):
    return [np.ascontiguousarray(x).tobytes() for x in out]


def _thermo_array(res):
    return np.array([[float(r[f]) for f in ("valid", "n", "tm", "dH", "dS", "hairpin_tm", "homodimer_tm", "dG")] for r in res], np.float32)


def test_salt_changes_on_one_handle(oracle):
    """The dG table is kept on the handle and keyed by the salt: eight calls whose salts alternate, each answered as the oracle
    expects at its own salt and with the bytes a fresh handle gives for that call alone."""
    names = MC.register_pool(oracle)
    at_default, at_10mm, at_1m = (PC.scenario(oracle, n) for n in (MC.POOL_DEFAULT, names[0], names[1]))
    panel, thr = at_default["panel"], at_default["thr"]
    lo, hi = PC.amp_of(at_default)
    _, words = SC.distinct_oligos(panel)
    plain = [w for w in words if oracle.word_degeneracy(w) == 1]
    ps = SC.PRIMER_STRAND
    tms = sorted(float(oracle.thermo_full(W.word_text(w), 0.01, ps)[0]) for w in plain)
    limits = dict(tm_min=tms[len(tms) // 2], tm_max=75.0, max_hairpin=40.0, max_dimer=40.0)

    def melt_kw(case):
        return dict(SC.conditions_of(case), template_strand=case["template_strand"])

    calls = [
        ("site_tm at 0.05", lambda d: d.site_tm(panel, thr, **melt_kw(at_default))),
        ("pool_dimers at 0.1", lambda d: d.pool_dimers(panel, salt=0.1, primer_strand=ps, rule="pool")),
        ("site_tm at 0.05 again", lambda d: d.site_tm(panel, thr, **melt_kw(at_default))),
        ("is_valid at 0.01", lambda d: (_thermo_array(d.is_valid(words, True, salt=0.01, primer_strand=ps, **limits)),)),
        ("pool_products_tm at 1.0", lambda d: d.pool_products_tm(panel, thr, bits=True, amp_min=lo, amp_max=hi, **melt_kw(at_1m))),
        ("site_variants at 0.01", lambda d: d.site_variants(panel, thr, site_map=True, **melt_kw(at_10mm))),
        ("site_tm at 0.01", lambda d: d.site_tm(panel, thr, **melt_kw(at_10mm))),
        ("pool_conflicts at 0.05", lambda d: d.pool_conflicts(panel, thr, dimers="pool", amp_min=lo, amp_max=hi, **melt_kw(at_default))),
    ]

    def handle():
        d = api.Screener(0)
        T_PRODUCTS._load(d, oracle, at_default)
        return d

    one = handle()
    try:
        got = [call(one) for _, call in calls]
    finally:
        one.close()
    # each answer against the oracle's expectation at its own salt
    def same(a, b, what):
        for x, y in zip(a, b):
            assert tuple(x) == tuple(y), (what, x, y)
        assert len(a) == len(b), what

    for k, case in ((0, at_default), (2, at_default), (6, at_10mm)):
        want_ids, want, _ = SC.expectation(oracle, case)
        assert got[k][0].tolist() == want_ids
        same(SC.as_bits(got[k][1]), SC.as_bits(want), calls[k][0])
    assert SC.as_bits(got[0][1]) != SC.as_bits(got[6][1])
    P = DC.Pool(oracle, panel)
    assert got[1][0].tolist() == P.ids
    same(DC.as_bits(got[1][1]), DC.expected_cells(oracle, P, DC.POOL, salt=0.1, primer_strand=ps), calls[1][0])
    valid = got[3][0][:, 0] != 0
    want_valid = [bool(oracle.is_valid(w, 0.01, ps, limits["tm_min"], limits["tm_max"], limits["max_hairpin"], limits["max_dimer"], True))
                  for w in words]
    assert valid.tolist() == want_valid and 0 < sum(want_valid) < len(words)
    for row, w in zip(got[3][0], words):
        if oracle.word_degeneracy(w) == 1:
            t = oracle.thermo_full(W.word_text(w), 0.01, ps)
            assert row[[2, 3, 4, 5, 6]].view(np.uint32).tolist() == t[[0, 1, 2, 4, 7]].view(np.uint32).tolist(), w
    want_ids, want, want_fr, want_rf = PC.expectation(oracle, names[1], 0.0)
    assert got[4][0].tolist() == want_ids and got[4][2].tolist() == want_fr.tolist() and got[4][3].tolist() == want_rf.tolist()
    same(PC.as_bits(got[4][1]), PC.as_bits(want), calls[4][0])
    want_ids, want, want_map, _ = VC.expectation(oracle, at_10mm)
    assert got[5][0].tolist() == want_ids and got[5][2].tolist() == want_map
    same(VC.as_bits(got[5][1]), VC.as_bits(want), calls[5][0])
    want_ids, want = CC.expected(oracle, MC.POOL_DEFAULT, 0.0, DC.POOL, 0.0)
    assert got[7][0].tolist() == want_ids
    same(CC.as_bits(got[7][1]), want, calls[7][0])
    # and against a fresh handle's answer to the same single call
    for (what, call), mine in zip(calls, got):
        fresh = handle()
        try:
            out = call(fresh)
        finally:
            fresh.close()
        assert _bytes(mine) == _bytes(out), what


# ------------------------------------------------------------------ 4. a three-fold oligo through pcr_site_repair
def test_three_fold_oligo_in_site_repair(dev, oracle):
    """pcr_site_repair reads the same oligo table: pool_case at the default condition against site_repair_cases' model as it is.
    (pcr_pool_probe_candidates takes product records, not oligos: its model needs more than the scenario's keys and is not
    run here.)"""
    MC.register_pool(oracle)
    case = PC.scenario(oracle, MC.POOL_DEFAULT)
    T_REPAIR._load(dev, oracle, case)
    got = T_REPAIR._compare(dev, oracle, case, max_mismatch=1)
    ids, _ = SC.distinct_oligos(case["panel"])
    for pair, side, _ in MC.POOL_WIDENED:
        mine = got[got["oligo"] == ids[2 * pair + side]]
        assert len(mine) >= 1 and int(mine[0]["n_expansions"]) == 3
