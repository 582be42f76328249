"""pcr_pool_anneal_profile_end3, pcr_pool_conflicts_end3 and pcr_pool_probe_hits_end3 without a device: the symbols and their
prototypes, the refusals that come before the handle and their order, the wrappers' keywords, and whether pool_rule_cases'
inputs can fail a wrong join -- for every (call, scenario, rule) the GPU tests run, the models drop and keep something where
that call reports it; under the zero rule the composed models are the base calls' models."""
import ctypes as C
import inspect

import numpy as np
import pytest

import anneal_profile_cases as AP
import end3_cases as E
import pool_conflict_cases as CC
import pool_rule_cases as R
import probe_hit_cases as H
import products_tm_cases as PT
import site_tm_cases as SC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1
CALLS = ("pcr_pool_anneal_profile_end3", "pcr_pool_conflicts_end3", "pcr_pool_probe_hits_end3")
KEYWORDS = dict(min_clamp3=0, window=0, max_end_mismatch=0, use_taq_mama=False, ident_threshold=0.0)


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


# ------------------------------------------------------------------ the ABI
def test_symbols_and_prototypes(lib):
    for name in CALLS:
        assert name in api.ABI_SYMBOLS
        assert hasattr(lib, name), "libpcramp_hip.so does not export " + name
        fn = getattr(lib, name)
        base = getattr(lib, name[:-len("_end3")])
        assert fn.restype is C.c_int64
        rule_at = [i for i, t in enumerate(fn.argtypes) if t == C.POINTER(api.End3Rule)]
        assert len(rule_at) == 1
        assert list(fn.argtypes[:rule_at[0]]) + list(fn.argtypes[rule_at[0] + 1:]) == list(base.argtypes)   # the base call's, plus the rule
    # after template_strand where there is no floor, else after the last floor
    assert lib.pcr_pool_anneal_profile_end3.argtypes.index(C.POINTER(api.End3Rule)) == 9
    assert lib.pcr_pool_conflicts_end3.argtypes.index(C.POINTER(api.End3Rule)) == 10
    assert lib.pcr_pool_probe_hits_end3.argtypes.index(C.POINTER(api.End3Rule)) == 13


def test_wrapper_signatures():
    for name in ("anneal_profile", "pool_conflicts", "probe_hits"):
        par = inspect.signature(getattr(api.Screener, name)).parameters
        for k, default in KEYWORDS.items():
            assert k in par and par[k].default == default and type(par[k].default) is type(default), (name, k)
    want = inspect.signature(api.Screener.pool_products_end3).parameters
    assert all(want[k].default == v for k, v in KEYWORDS.items())           # pool_products_end3's names and defaults


# ------------------------------------------------------------------ the refusals
def _refused(lib, oracle, call, pool=None, probes=None, which=api.TARGET, null_args=False, salt=0.05, primer_strand=9e-7, probe_strand=2.5e-7,
             template_strand=0.0, tm_floor=0.0, probe_tm_floor=0.0, n_pool=None, out_cap=0, temps=(50.0, 60.0), dimer_rule=CC.NO_DIMERS,
             dimer_floor=0.0, null_rule=False, **rule):
    """One of the three calls on a NULL handle -> (return value, message)."""
    w = oracle.centered_word
    pool = [(w("ACGTTGCAAGCTTGCATGCA"), w("TTGACCGTAGGCTAGCTAAC"))] if pool is None else pool
    a = W.pairs_array(pool)
    n = len(pool) if n_pool is None else n_pool
    ids = np.zeros(max(2 * len(pool), 1), np.uint32)
    args = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    pa = None if null_args else C.byref(args)
    r = E.rule_of(**rule)
    rs = api.End3Rule(r["min_clamp3"], r["window"], r["max_end_mismatch"], r["use_taq_mama"], r["ident_threshold"])
    pr = None if null_rule else C.byref(rs)
    if call == "anneal":
        t = np.asarray(temps, np.float32)
        points = np.zeros(max(len(t), 1), api.ANNEAL_POINT_DTYPE)
        rc = lib.pcr_pool_anneal_profile_end3(None, which, a.ctypes.data, n, 0.9, 80, 200, pa, template_strand, pr, t.ctypes.data, len(t),
                                              ids.ctypes.data, points.ctypes.data, None, None, None, None)
    elif call == "conflicts":
        rc = lib.pcr_pool_conflicts_end3(None, which, a.ctypes.data, n, 0.9, 80, 200, pa, template_strand, tm_floor, pr, dimer_rule,
                                         dimer_floor, ids.ctypes.data, None, out_cap)
    else:
        words = np.zeros((max(len(pool), 1), 2), np.uint64)
        for i, p in enumerate(probes or ()):
            words[i] = p
        pid = np.zeros(max(len(pool), 1), np.uint32)
        rc = lib.pcr_pool_probe_hits_end3(None, which, a.ctypes.data, words.ctypes.data, n, 0.9, 80, 200, pa, probe_strand, template_strand,
                                          tm_floor, probe_tm_floor, pr, ids.ctypes.data, pid.ctypes.data, None, out_cap, None)
    return rc, api._err(lib)


LATE = dict(window=33, use_taq_mama=2, ident_threshold=2.0)                 # the rule's own refusals, all at once
RULE_STEPS = [
    (dict(window=33, use_taq_mama=2, ident_threshold=2.0), "window, min_clamp3 or max_end_mismatch above 32"),
    (dict(min_clamp3=33, use_taq_mama=2, ident_threshold=2.0), "window, min_clamp3 or max_end_mismatch above 32"),
    (dict(max_end_mismatch=33, use_taq_mama=2, ident_threshold=2.0), "window, min_clamp3 or max_end_mismatch above 32"),
    (dict(use_taq_mama=2, ident_threshold=2.0), "use_taq_mama is neither 0 nor 1"),
    (dict(use_taq_mama=-1, ident_threshold=2.0), "use_taq_mama is neither 0 nor 1"),
    (dict(ident_threshold=1.5), "ident_threshold is not finite or outside [0, 1]"),
    (dict(ident_threshold=-0.25), "ident_threshold is not finite or outside [0, 1]"),
    (dict(ident_threshold=float("nan")), "ident_threshold is not finite or outside [0, 1]"),
    (dict(ident_threshold=float("inf")), "ident_threshold is not finite or outside [0, 1]"),
    (dict(), "null handle"),
    (dict(null_rule=True), "null handle"),
    (dict(window=32, min_clamp3=32, max_end_mismatch=32, use_taq_mama=1, ident_threshold=1.0), "null handle"),
]
# the base calls' checks in their order; each case breaks one check and every later one as well, the rule's included
BASE_STEPS = {
    "anneal": [
        (dict(which=7, salt=2.0, temps=()), "unknown sequence set"),
        (dict(which=api.MULTIPLEX, salt=2.0, temps=()), "PCR_SET_MULTIPLEX"),
        (dict(null_args=True, temps=()), "bad argument"),
        (dict(n_pool=api.POOL_MAX_PAIRS + 1, salt=2.0, temps=()), "PCR_POOL_MAX_PAIRS"),
        (dict(primer_strand=-1.0, salt=2.0, temps=()), "negative strand concentration"),
        (dict(salt=2.0, temps=()), "salt outside"),
        (dict(primer_strand=0.0, temps=()), "strand concentration of an oligo's duplex is zero"),
        (dict(temps=()), "n_temps is 0"),
        (dict(temps=(50.0, float("nan"))), "a temperature is not finite"),
        (dict(temps=(60.0, 50.0)), "not strictly ascending"),
    ],
    "conflicts": [
        (dict(which=7, salt=2.0, tm_floor=float("nan"), dimer_rule=5), "unknown sequence set"),
        (dict(which=api.MULTIPLEX, salt=2.0, tm_floor=float("nan"), dimer_rule=5), "PCR_SET_MULTIPLEX"),
        (dict(out_cap=5, salt=2.0, tm_floor=float("nan"), dimer_rule=5), "bad argument"),
        (dict(n_pool=api.POOL_MAX_PAIRS + 1, salt=2.0, tm_floor=float("nan"), dimer_rule=5), "PCR_POOL_MAX_PAIRS"),
        (dict(primer_strand=-1.0, salt=2.0, tm_floor=float("nan"), dimer_rule=5), "negative strand concentration"),
        (dict(salt=2.0, tm_floor=float("nan"), dimer_rule=5), "salt outside"),
        (dict(primer_strand=0.0, tm_floor=float("nan"), dimer_rule=5), "strand concentration of an oligo's duplex is zero"),
        (dict(tm_floor=float("nan"), dimer_rule=5), "tm_floor is not finite"),
        (dict(dimer_rule=5, dimer_floor=float("nan")), "unknown dimer_rule"),
        (dict(dimer_rule=api.DIMER_RULE_POOL, dimer_floor=float("nan"), primer_strand=0.0, template_strand=1e-7), "dimer_floor is not finite"),
        (dict(dimer_rule=api.DIMER_RULE_POOL, primer_strand=0.0, template_strand=1e-7), "with a dimer rule primer_strand must be positive"),
    ],
    "probes": [
        (dict(which=7, salt=2.0, tm_floor=float("nan")), "unknown sequence set"),
        (dict(which=api.MULTIPLEX, salt=2.0, tm_floor=float("nan")), "PCR_SET_MULTIPLEX"),
        (dict(out_cap=5, salt=2.0, tm_floor=float("nan")), "bad argument"),
        (dict(n_pool=api.POOL_MAX_PAIRS + 1, salt=2.0, tm_floor=float("nan")), "PCR_POOL_MAX_PAIRS"),
        (dict(probe_strand=-1.0, salt=2.0, tm_floor=float("nan")), "negative strand concentration"),
        (dict(salt=2.0, tm_floor=float("nan")), "salt outside"),
        (dict(primer_strand=0.0, tm_floor=float("nan")), "strand concentration of a primer's duplex is zero"),
        (dict(probe_strand=0.0, tm_floor=float("nan"), probes="one"), "strand concentration of a probe's duplex is zero"),
        (dict(tm_floor=float("nan"), probe_tm_floor=float("nan")), "tm_floor is not finite"),
        (dict(probe_tm_floor=float("inf")), "probe_tm_floor is not finite"),
    ],
}


@pytest.mark.parametrize("call", ["anneal", "conflicts", "probes"])
def test_refusals_in_order(lib, oracle, call):
    """Every PCR_ERR_ARG in the documented order on a NULL handle: the base call's checks, then the rule's, then the handle."""
    name = {"anneal": CALLS[0], "conflicts": CALLS[1], "probes": CALLS[2]}[call]
    probe = oracle.centered_word("GGATCCATTGCAAGTCCGTA")
    for kw, what in [(dict(k, **LATE), w) for k, w in BASE_STEPS[call]] + RULE_STEPS:
        kw = dict(kw)
        if kw.get("probes") == "one":
            kw["probes"] = [probe]
        rc, msg = _refused(lib, oracle, call, **kw)
        assert rc == PCR_ERR_ARG and what in msg and msg.startswith(name + ": "), (kw, msg)


@pytest.mark.parametrize("call", ["anneal", "conflicts", "probes"])
def test_oligo_refusals_come_before_the_rule(lib, oracle, call):
    too_many = SC.too_degenerate_oligo(oracle)
    pool = [(too_many, oracle.centered_word("TTGACCGTAGGCTAGCTAAC"))]
    rc, msg = _refused(lib, oracle, call, pool=pool, window=40)
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg
    if call == "probes":                                                    # a probe is an oligo of the table as well
        rc, msg = _refused(lib, oracle, call, probes=[too_many], window=40)
        assert rc == PCR_ERR_ARG and "a probe has more than PCR_SITE_MAX_EXPANSIONS" in msg


# ------------------------------------------------------------------ the inputs
def test_probe_ends_is_as_described(oracle):
    name = R.probe_ends_name(oracle)
    case, base = H.scenario(oracle, name), PT.scenario(oracle, R.ends_name(oracle))
    assert [len(s) for s in case["seqs"]] == [len(s) for s in base["seqs"]] and case["panel"] == base["panel"]
    assert case["active"] == base["active"] and "eos" not in case and not case.get("splits")
    assert [p is not None for p in case["probes"]] == [True, True, False]
    ids, pid, prod, psites, hits = H.everything(oracle, name)
    assert pid == [0, 1, H.NO_PROBE]
    assert R.keys_of(PT.all_products(oracle, name)[1]) == R.keys_of(prod)   # the pool's products do not depend on the probes in the DB
    # pair 0's probe: one exact site on sequence 0, inside every product of that sequence
    on0 = prod[prod["sequence"] == 0]
    site0 = psites[(psites["oligo"] == 0) & (psites["sequence"] == 0) & (psites["loc5"] == R.PROBE0_AT)]
    assert len(site0) == 1 and int(site0["loc3"][0]) == R.PROBE0_AT + R.PROBE0_LEN - 1 and len(on0) >= 24 * 24
    with0 = hits[(hits["sequence"] == 0) & (hits["probe"] == 0) & (hits["probe_loc5"] == R.PROBE0_AT)]
    assert R.keys_of(with0) == R.keys_of(on0)
    # pair 1's probe: inside the exact product on sequence 2, and inside pair 1's only product on sequence 1
    for s, begin in ((2, 250), (1, 160)):
        mine = hits[(hits["sequence"] == s) & (hits["probe"] == 1) & (hits["intended"] == (H.PRODUCT_INTENDED | H.PROBE_INTENDED))]
        assert len(mine) == 1 and int(mine["begin"][0]) == begin
    ends = E.site_ends(oracle, name)
    weak = ends[(2, 1, 1, 160)]
    assert weak["clamp3"] == 1 and E.end_mismatch(weak, 5) == 2 and ends[(2, 2, 1, 250)]["clamp3"] == 18


def test_arms_is_as_described(oracle):
    name = R.arms_name(oracle)
    ids, rec, _ = E.products_before_rule(oracle, name)
    assert ids == [0, 1, 2, 3, 4, 5] and len(rec) == 7
    ends = E.site_ends(oracle, name)
    spur = rec[rec["intended"] == 0]
    cells = CC.product_cells(ids, rec, 0.0)
    assert {c: v["products"] for c, v in cells.items()} == {(0, 1): 2, (0, 2): 2}
    clamp = lambda r: ends[(int(r["plus_oligo"]), int(r["sequence"]), 1, int(r["begin"]))]["clamp3"]
    assert sorted(clamp(r) for r in spur if {int(r["plus_oligo"]), int(r["minus_oligo"])} <= {0, 1, 2, 3}) == [0, 0]
    assert sorted(clamp(r) for r in spur if int(r["plus_oligo"]) == 4) == [0, 20]
    assert all(clamp(r) == 20 for r in rec[rec["intended"] != 0])


def _shows(oracle, call, name, rule):
    """Whether the models drop and keep something where `call` reports it (at no floor)."""
    before, after = R.ruled(oracle, name, E.ZERO_RULE)[1], R.ruled(oracle, name, rule)[1]
    if not 0 < len(after) < len(before):
        return False
    if call == "anneal":
        temps = R.anneal_temps(oracle, name, rule)
        a, z = R.anneal(oracle, name, rule, temps), R.anneal(oracle, name, E.ZERO_RULE, temps)
        melt = any((a[i].view(np.uint32) != z[i].view(np.uint32)).any() for i in (4, 5, 6))
        return bool((a[3] != z[3]).any()) and melt
    if call == "conflicts":
        a = {(r[0], r[1]): r[2] for r in R.conflicts(oracle, name, rule)[1]}
        z = {(r[0], r[1]): r[2] for r in R.conflicts(oracle, name, E.ZERO_RULE)[1]}
        return any(c not in a for c in z) and any(0 < a[c] < z[c] for c in a)
    a, z = R.probes(oracle, name, name, rule), R.probes(oracle, name, name, E.ZERO_RULE)
    return 0 < len(a[2]) < len(z[2]) and bool((z[3] & ~a[3]).any()) and bool(a[3].any())


def test_input_conditions(oracle):
    """Every triple the GPU tests run shows a dropped and a kept product in its call's output; the candidates left out do not."""
    used = R.triples(oracle)
    key = lambda t: (t[0], t[1], R.rule_id(t[2]))
    assert {key(t) for t in used} <= {key(t) for t in R.candidates(oracle)}
    for call, name, rule in R.candidates(oracle):
        assert _shows(oracle, call, name, rule) == (key((call, name, rule)) in {key(t) for t in used}), key((call, name, rule))
    for call in ("anneal", "conflicts", "probes"):
        mine = R.triples_of(oracle, call)
        assert len(mine) >= 5
        assert any(r["ident_threshold"] and r["use_taq_mama"] for _, r in mine) and any(r["ident_threshold"] and not r["use_taq_mama"] for _, r in mine)
    # ends_case itself serves pcr_pool_anneal_profile_end3; no rule empties one of its conflict cells (every oligo pair has an exact product)
    assert any(n == R.ends_name(oracle) for n, _ in R.triples_of(oracle, "anneal"))
    # the in-range floor cuts, something passes floor and rule together, and for most rules both cut
    both = 0
    for call, name, rule in used:
        f = R.floor_of(oracle, name)
        n_both, n_floor = len(R.ruled(oracle, name, rule, f)[1]), len(R.ruled(oracle, name, E.ZERO_RULE, f)[1])
        assert 0 < n_both <= n_floor < len(R.ruled(oracle, name, E.ZERO_RULE)[1])
        both += n_both < n_floor
    assert both >= len(used) - 3                                             # (window 5, one mismatch: what it drops melts below the floor)


def test_words_rule_crosses_a_word_boundary(oracle):
    """min_clamp3 = 32 on "words" takes the products of the mutated minus sites away: bits go out in u64 words 0 and 1."""
    ids, rec, fr, rf, before = R.ruled(oracle, "words", R.WORDS_RULE)
    _, _, zfr, zrf, _ = R.ruled(oracle, "words", E.ZERO_RULE)
    gone = E.unpack_bits(zfr & ~fr, PT.WORDS_N).any(axis=0)
    assert np.nonzero(gone)[0].tolist() == list(PT.WORDS_MUTATED) and 0 < len(rec) < before
    assert (zfr[:, 0] != fr[:, 0]).any() and (zfr[:, 1] != fr[:, 1]).any() and (zfr[:, 2] == fr[:, 2]).all()
    kept = E.unpack_bits(fr, PT.WORDS_N).any(axis=0)
    assert [bool(kept[s]) for s in R.WORDS_SEQS] == [True, False, False, True]    # 64: mutated, 65: inactive


# ------------------------------------------------------------------ the zero rule
def test_zero_rule_models_are_the_base_models(oracle):
    """Composed under the zero rule, the models are anneal_profile_cases.expected, pool_conflict_cases.expected and
    probe_hit_cases.expectation (on scenarios without an EOS split, which those models do not know)."""
    for name in ("ladder", R.arms_name(oracle), R.probe_ends_name(oracle)):
        temps = AP.temps_of(PT.all_products(oracle, name)[1])
        got, want = R.anneal(oracle, name, E.ZERO_RULE, temps), AP.expected(oracle, name, temps)
        assert got[1] == len(PT.all_products(oracle, name)[1])
        for a, b in zip(got[2:], want):
            assert AP.as_words(a) == AP.as_words(b)
        for tm_floor in (0.0, R.floor_of(oracle, name)):
            for dimer_rule in (CC.NO_DIMERS, api.DIMER_RULE_POOL):
                assert R.conflicts(oracle, name, E.ZERO_RULE, tm_floor, dimer_rule) == CC.expected(oracle, name, tm_floor, dimer_rule)
    name = R.probe_ends_name(oracle)
    for tm_floor in (0.0, R.floor_of(oracle, name)):
        got, want = R.probes(oracle, name, name, E.ZERO_RULE, tm_floor), H.expectation(oracle, name, tm_floor)
        assert got[0] == want[0] and got[1] == want[1] and H.as_bits(got[2]) == H.as_bits(want[2]) and got[3].tolist() == want[3].tolist()
