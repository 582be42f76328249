"""pcr_site_variants / Screener.site_variants on the GPU: every record against site_variant_cases.expected_variants (the oracle's
word DB, site_tm_cases' site and pick rules, a Python restatement of the key, the mask and the clamps, oracle.heterodimer_full),
record for record and every float as bits; and joined, site by site, with site_tm's records on the same handle."""
import ctypes as C

import numpy as np
import pytest

import site_tm_cases as SC
import site_variant_cases as VC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

BITS = lambda x: int(np.float32(x).view(np.uint32))


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


def _kw(case):
    return dict(SC.conditions_of(case), template_strand=case.get("template_strand", 0.0))


def _raw(d, case, cap, site_cap, thermo=True):
    """The C call itself -> (return value, ids, records, site map, counts)."""
    a = W.pairs_array(case["panel"])
    ids = np.zeros(max(2 * len(case["panel"]), 1), np.uint32)
    cond = SC.conditions_of(case)
    args = api.ThermoArgs(cond["salt"], cond["primer_strand"], 0.0, 0.0, 0.0, 0.0)
    out = np.zeros(max(cap, 1), api.SITE_VARIANT_DTYPE)
    smap = np.full(max(site_cap, 1), 0xFFFFFFFF, np.uint32)
    counts = np.full(2, 99, np.uint64)
    n = d.L.pcr_site_variants(d.h, api.TARGET, a.ctypes.data, len(case["panel"]), float(case["thr"]),
                              C.byref(args) if thermo else None, float(case.get("template_strand", 0.0)), ids.ctypes.data,
                              out.ctypes.data if cap else None, cap, smap.ctypes.data if site_cap else None, site_cap,
                              counts.ctypes.data)
    return int(n), ids, out, smap, counts.tolist()


def _compare(d, oracle, case):
    """Variants, site map and counts equal the expectation; the join with site_tm on the same handle.  -> (variants, site map,
    site records, counts)."""
    want_ids, want, want_map, want_jobs = VC.expectation(oracle, case)
    ids, var, smap = d.site_variants(case["panel"], case["thr"], site_map=True, **_kw(case))
    assert ids.tolist() == want_ids
    got_bits, want_bits = VC.as_bits(var), VC.as_bits(want)
    for g, w in zip(got_bits, want_bits):
        assert g == w, (g, w)
    assert len(got_bits) == len(want_bits)
    assert smap.tolist() == want_map
    n, _, _, _, counts = _raw(d, case, len(want), len(want_map))
    assert n == len(want) and counts == [len(want_map), want_jobs]
    assert want_jobs == int(want["n_expansions"].sum())
    # every site of site_tm carries, bit for bit, what its variant says
    sid, sites = d.site_tm(case["panel"], case["thr"], **_kw(case))
    assert sid.tolist() == ids.tolist() and len(sites) == len(smap)
    assert int(var["sites"].sum()) == len(sites)
    assert want_jobs <= int(sites["n_expansions"].sum())
    assert (want_jobs == int(sites["n_expansions"].sum())) == (len(var) == len(sites))
    for s, v in zip(sites, smap.tolist()):
        r = var[v]
        assert (s["oligo"], s["matches"], s["n_expansions"], s["flags"]) == (r["oligo"], r["matches"], r["n_expansions"], r["flags"])
        assert [BITS(s[f]) for f in ("tm_max", "tm_min", "dH", "dS")] == [BITS(r[f]) for f in ("tm_max", "tm_min", "dH", "dS")]
    # first_* is the lowest member, sequences the distinct ones (site_tm's records are sorted by (oligo, sequence, loc5, strand))
    first, seqs = {}, {}
    for s, v in zip(sites, smap.tolist()):
        first.setdefault(v, (int(s["sequence"]), int(s["loc5"]), int(s["strand"])))
        seqs.setdefault(v, set()).add(int(s["sequence"]))
    members = np.bincount(smap, minlength=len(var)).tolist()
    for v, r in enumerate(var):
        assert (int(r["first_sequence"]), int(r["first_loc5"]), int(r["first_strand"])) == first[v]
        assert int(r["sequences"]) == len(seqs[v]) and int(r["sites"]) == members[v]
    return var, smap, sites, counts


def _check(d, oracle, case):
    _load(d, oracle, case)
    return _compare(d, oracle, case)


# ------------------------------------------------------------------ 1. every scenario pcr_site_tm is tested on
@pytest.mark.parametrize("name", SC.SCENARIO_NAMES)
def test_site_tm_scenarios(dev, oracle, name):
    var, smap, sites, counts = _check(dev, oracle, SC.gpu_scenarios(oracle)[name])
    assert len(var) >= 1
    if name == "grid":                                                      # 301 copies of one site: the inner ones are one variant
        assert int(var[0]["sites"]) >= SC.GRID_SITES - 2 and var[0]["sequences"] == 1
        assert counts[1] < counts[0]


# ------------------------------------------------------------------ 2. a conserved target set, and block edges
def test_conserved_classes(dev, oracle):
    case = VC.conserved_case(oracle)
    var, smap, sites, counts = _check(dev, oracle, case)
    n_large = VC.CONSERVED_EXACT + 2                                        # ... + the sequence with two sites + the strand-2 one
    assert n_large + 1 > 2 * 256                                            # the large class spans several POOL_THREADS blocks
    assert var["oligo"].tolist() == [0, 0, 0, 0]
    assert var["sequences"].tolist() == [n_large, 6, 5, 3]
    assert var["sites"].tolist() == [n_large + 1, 6, 5, 3]                  # the double site: sites + 1, sequences + 0
    assert var["matches"].tolist() == [20, 19, 20, 18]
    assert var["mismatch_mask"].tolist() == [0, 1 << 19, 0, 0b11]
    assert var["clamp3"].tolist() == [20, 0, 20, 18]
    assert var["clamp5"].tolist() == [20, 19, 20, 0]
    assert not var["flags"].any() and (var["n_expansions"] == 1).all()
    # the strand-2 site is a member of the large class; the inactive sequence's spelling appears nowhere
    members = sites[np.asarray(smap) == 0]
    assert sorted(set(members["strand"].tolist())) == [1, 2] and int((members["strand"] == 2).sum()) == 1
    assert VC.CONSERVED_N - 1 not in sites["sequence"].tolist()
    text = api.variant_texts(var)
    assert len(set(text)) == 4 and text[0][1:] == text[2][1:] and text[0][0] != text[2][0]
    assert counts == [n_large + 1 + 6 + 5 + 3, 4]                            # 4 duplexes for 600 sites
    merged = api.merge_variant_flanks(var, case["panel"], smap, sites)
    assert merged["sites"].tolist() == [n_large + 1 + 5, 6, 3] and merged["sequences"].tolist() == [n_large + 5, 6, 3]
    assert BITS(merged[0]["tm_max"]) == max(BITS(var[0]["tm_max"]), BITS(var[2]["tm_max"]))


# ------------------------------------------------------------------ 3. oligo identity
def test_oligo_identity_and_expansions(dev, oracle):
    case = VC.identity_case(oracle)
    _load(dev, oracle, case)
    var, smap, sites, counts = _compare(dev, oracle, case)
    ids, _ = dev.site_variants(case["panel"], case["thr"], **_kw(case))
    assert ids.tolist() == [0, 1, 0, 2, 3, 0]                               # q three times in the panel: one oligo
    assert sorted(set(var["oligo"].tolist())) == [0, 1, 2, 3]
    # q and q1 both match q's site in every sequence: a variant of each oligo there, never a shared one
    q, q1 = var[var["oligo"] == 0], var[var["oligo"] == 1]
    assert int(q["sites"].sum()) == 3 and int(q1["sites"].sum()) == 3
    assert set(q["matches"].tolist()) == {22} and set(q1["matches"].tolist()) == {21}
    assert set(map(tuple, q["word"].tolist())) == set(map(tuple, q1["word"].tolist()))
    assert (q1["mismatch_mask"] == 1 << 8).all()
    # 4 and 256 expansions: one job per (variant, expansion)
    d4, d256 = var[var["oligo"] == 2], var[var["oligo"] == 3]
    assert set(d4["n_expansions"].tolist()) == {4} and set(d256["n_expansions"].tolist()) == {256}
    assert counts[1] == int(var["n_expansions"].sum())
    assert (d4["tm_max"] > d4["tm_min"]).all() and (d256["tm_max"] > d256["tm_min"]).all()


# ------------------------------------------------------------------ 4. order ties
def test_ties_come_in_planes_order(dev, oracle):
    case = VC.ties_case(oracle)
    var, _, _, _ = _check(dev, oracle, case)
    one = var[(var["matches"] == 20) & (var["oligo"] == 0)]
    assert len(one) == len(VC.TIE_PLACES)
    assert set(one["sequences"].tolist()) == {1} and set(one["sites"].tolist()) == {1}
    assert sorted(int(m).bit_length() - 1 for m in one["mismatch_mask"]) == sorted(VC.TIE_PLACES)
    planes = [SC.planes_of(SC.slots_of((int(r["word"][0]), int(r["word"][1])))) for r in one]
    assert planes == sorted(planes) and len(set(planes)) == len(planes)
    assert [tuple(r["word"]) for r in one] != sorted(tuple(r["word"]) for r in one) or \
        [int(r["first_sequence"]) for r in one] != sorted(int(r["first_sequence"]) for r in one), \
        "the planes order coincides with the word order and the sequence order: the case cannot tell them apart"


# ------------------------------------------------------------------ 5. template bases that cannot be melted; a split
def test_no_tm_variants_and_the_straddling_site(dev, oracle):
    var, smap, sites, _ = _check(dev, oracle, SC.ambiguity_case(oracle))
    assert len(var) == 4 and sorted(var["flags"].tolist()) == [0, 0, api.SITE_NO_TM, api.SITE_NO_TM]
    for r in var:
        zero = [BITS(r[f]) == 0 for f in ("tm_max", "tm_min", "dH", "dS")]
        assert all(zero) if r["flags"] & api.SITE_NO_TM else not any(zero)
    for r, t in zip(var, api.variant_texts(var)):                           # the flag is there where the spelling has a code
        assert bool(set(t) - set("ACGT")) == bool(r["flags"] & api.SITE_NO_TM), t
    var, smap, sites, _ = _check(dev, oracle, SC.split_case(oracle))
    whole = var[(var["oligo"] == 0) & (var["matches"] == 22)]
    assert len(whole) == 1 and whole[0]["first_sequence"] == 1 and whole[0]["flags"] == 0
    weak = var[(var["oligo"] == 0) & (var["matches"] < 22)]                  # the straddling site: its own, weaker variant(s)
    assert len(weak) >= 1 and set(weak["first_sequence"].tolist()) == {0}
    assert all(whole[0]["tm_max"] > r["tm_max"] for r in weak)


# ------------------------------------------------------------------ 6. without thermodynamics; caps
def test_without_thermodynamics_and_caps(dev, oracle):
    case = VC.conserved_case(oracle)
    _load(dev, oracle, case)
    _, want, want_map, _ = VC.expectation(oracle, case)
    _, cold, cold_map, zero_jobs = VC.expectation(oracle, case, thermo=False)
    ids, var, smap = dev.site_variants(case["panel"], case["thr"], thermo=False, site_map=True, salt=7.0, primer_strand=-1.0,
                                       template_strand=-1.0)                 # ... none of which is read
    assert VC.as_bits(var) == VC.as_bits(cold) and smap.tolist() == cold_map == want_map and zero_jobs == 0
    assert [b[:14] for b in VC.as_bits(var)] == [b[:14] for b in VC.as_bits(want)]
    assert all(b[14:] == (0, 0, 0, 0) for b in VC.as_bits(var))
    n, _, out, m, counts = _raw(dev, case, len(want), len(want_map), thermo=False)
    assert n == len(want) and counts == [len(want_map), 0] and VC.as_bits(out[:n]) == VC.as_bits(cold)
    n, _, _, m, counts = _raw(dev, case, 0, len(want_map))                  # cap = 0: the count, no map, no job
    assert n == len(want) and counts == [len(want_map), 0] and (m == 0xFFFFFFFF).all()
    n, _, _, m, counts = _raw(dev, case, len(want) - 1, len(want_map))      # too small: the count again, no map
    assert n == len(want) and counts[0] == len(want_map) and (m == 0xFFFFFFFF).all()
    n, _, out, m, counts = _raw(dev, case, len(want), len(want_map) - 1)    # the sites do not fit: records, no map
    assert n == len(want) and VC.as_bits(out[:n]) == VC.as_bits(want) and (m == 0xFFFFFFFF).all()
    assert counts == [len(want_map), len(want)]
    n, _, out, m, counts = _raw(dev, case, len(want) + 3, 0)                # no map asked for
    assert n == len(want) and VC.as_bits(out[:n]) == VC.as_bits(want)
    ids, var = dev.site_variants(case["panel"], case["thr"], cap=1, **_kw(case))   # the wrapper grows and retries
    assert VC.as_bits(var) == VC.as_bits(want)
    ids, var, smap = dev.site_variants(case["panel"], case["thr"], cap=1, site_map=True, **_kw(case))
    assert VC.as_bits(var) == VC.as_bits(want) and smap.tolist() == want_map


# ------------------------------------------------------------------ 7. state and resources
def test_state_and_resources(oracle):
    before = api.live_resources()
    d = api.Screener(0)
    try:
        case = SC.ids_case(oracle)
        d.load_texts(case["seqs"])
        with pytest.raises(api.PcrError, match="no word DB"):
            d.site_variants(case["panel"], case["thr"])
        assert d.L.pcr_site_variants(d.h, api.TARGET, None, 0, 0.9, None, 0.0, None, None, 0, None, 0, None) == -3   # PCR_ERR_STATE
        _load(d, oracle, case)
        ids, var, smap = d.site_variants([], case["thr"], site_map=True)
        assert len(ids) == 0 and len(var) == 0 and len(smap) == 0 and var.dtype == api.SITE_VARIANT_DTYPE
        with pytest.raises(api.PcrError, match="salt"):
            d.site_variants(case["panel"], case["thr"], salt=2.0)
        entries = d.entries()
        sid, sites = d.site_tm(case["panel"], case["thr"])
        _compare(d, oracle, case)
        assert d.entries() == entries
        sid2, sites2 = d.site_tm(case["panel"], case["thr"])
        assert sid2.tolist() == sid.tolist() and sites2.tobytes() == sites.tobytes()
        assert 1 not in sites["sequence"].tolist()                          # the inactive sequence: no site, no variant
    finally:
        d.close()
    assert api.live_resources() == before


# ------------------------------------------------------------------ 8. determinism
def test_two_calls_give_identical_bytes(dev, oracle):
    case = SC.random_case(oracle)
    _load(dev, oracle, case)
    a = dev.site_variants(case["panel"], case["thr"], site_map=True, **_kw(case))
    b = dev.site_variants(case["panel"], case["thr"], site_map=True, **_kw(case))
    assert len(a[1]) > 50
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
