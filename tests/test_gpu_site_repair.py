"""pcr_site_repair / Screener.site_repair on the GPU: every field of every record against site_repair_cases.expected_repair (the
oracle's word DB, site_variant_cases' variants and site map, a Python restatement of held / candidates / the greedy step,
oracle.is_valid), on site_variant_cases' and site_tm_cases' small scenarios and on scenarios sized to where the kernels can go
wrong: 64-bit edges of the held bitset, more variants than a workgroup has threads, the candidate cut, ties, degeneracy edges."""
import ctypes as C

import numpy as np
import pytest

import site_repair_cases as RC
import site_tm_cases as SC
import site_variant_cases as VC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu


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
        d.split(s, p)
    thr2 = SC.SQ(case["thr"])
    if case["select"] == "all":
        d.select_sites(case["panel"], thr2, which=which)
    else:
        d.select_words(case["panel"], thr2, which=which)
    assert d.entries(which) == SC.db_of(oracle, case)


def _run(d, case, **kw):
    args = dict(RC.THERMO)
    args.update(case.get("repair", {}))
    args.update(kw)
    return d.site_repair(case["panel"], case["thr"], **args)


def _compare(d, oracle, case, **kw):
    """The records equal the expectation, field for field.  -> the records."""
    want_ids, want = RC.expectation(oracle, case, **{k: v for k, v in kw.items() if k != "which"})
    ids, got = _run(d, case, **kw)
    assert ids.tolist() == want_ids
    for g, w in zip(RC.as_tuples(got), RC.as_tuples(want)):
        assert g == w, (g, w)
    assert len(got) == len(want)
    # what needs no expectation: each oligo's steps are 0 .. its last, one reason on the last alone, gains add up
    for o in set(got["oligo"].tolist()):
        mine = got[got["oligo"] == o]
        assert mine["step"].tolist() == list(range(len(mine)))
        assert not mine["flags"][:-1].any() and int(mine["flags"][-1]) in (1, 2, 4, 8)
        assert (np.diff(mine["sequences_held"].astype(np.int64)) == mine["gain"][1:]).all() and (mine["gain"][1:] > 0).all()
        assert mine[0]["variant"] == api.REPAIR_NO_VARIANT and mine[0]["added_mask"] == 0 and mine[0]["candidates"] == 0
        assert (mine["sequences_held"] <= mine["sequences_total"]).all()
    return got


def _check(d, oracle, case, **kw):
    _load(d, oracle, case)
    return _compare(d, oracle, case, **kw)


# ------------------------------------------------------------------ the small scenarios of the calls underneath
@pytest.mark.parametrize("name", ("placement", "ends", "ambiguity", "split", "ids", "expansions_1", "random"))
def test_site_tm_scenarios(dev, oracle, name):
    case = SC.gpu_scenarios(oracle)[name]
    got = _check(dev, oracle, case, max_mismatch=1 if name == "random" else 0)
    assert len(got) >= len(set(got["oligo"].tolist())) >= 1


@pytest.mark.parametrize("name", VC.NEW_SCENARIO_NAMES)
def test_site_variant_scenarios(dev, oracle, name):
    _check(dev, oracle, VC.new_scenarios(oracle)[name])


# ------------------------------------------------------------------ free coverage
def test_free_coverage(dev, oracle):
    got = _check(dev, oracle, RC.free_coverage_case(oracle))
    mine = got[got["oligo"] == 0]
    _, var = dev.site_variants(RC.free_coverage_case(oracle)["panel"], RC.free_coverage_case(oracle)["thr"], thermo=False)
    assert var["sequences"].tolist() == [5, 4, 2, 1]                        # A, B, the exact spelling, C
    assert mine["variant"].tolist() == [api.REPAIR_NO_VARIANT, 0, 1]        # A, then B; C is never unioned
    assert mine["gain"].tolist() == [0, 5, 5] and mine["sequences_held"].tolist() == [2, 7, 12]
    assert mine["variants_held"].tolist() == [1, 2, 4] and mine["flags"].tolist() == [0, 0, api.REPAIR_COMPLETE]
    assert mine["added_mask"].tolist() == [0, 1 << 3, 1 << 10] and mine["n_expansions"].tolist() == [1, 2, 4]
    # every candidate weighed: C's union holds all three and is taken at once
    wide = _compare(dev, oracle, RC.free_coverage_case(oracle), max_candidates=256)
    assert wide[wide["oligo"] == 0]["variant"].tolist() == [api.REPAIR_NO_VARIANT, 3]
    assert wide[wide["oligo"] == 0]["gain"].tolist() == [0, 10]


# ------------------------------------------------------------------ distinct sequences, at the bitset's word edges
@pytest.mark.parametrize("n", (65, 129))
def test_distinct_sequences(dev, oracle, n):
    got = _check(dev, oracle, RC.distinct_case(oracle, n))
    mine = got[got["oligo"] == 0]
    assert mine["sequences_total"].tolist() == [2 * n, 2 * n]               # the inactive sequence is no part of it
    assert mine["sequences_held"].tolist() == [n + 1, 2 * n]                # the sequence with both spellings is held from the start
    assert mine["gain"].tolist() == [0, n - 1] and mine["sites_held"].tolist() == [n + 1, 2 * n + 1]


# ------------------------------------------------------------------ more variants than threads and than candidates
@pytest.mark.parametrize("max_candidates", (256, 8))
def test_wide_oligo(dev, oracle, max_candidates):
    case = RC.wide_case(oracle, max_candidates)
    got = _check(dev, oracle, case)
    _, var = dev.site_variants(case["panel"], case["thr"], thermo=False)
    assert int((var["oligo"] == 0).sum()) == 300
    mine = got[got["oligo"] == 0]
    assert mine[0]["variants_held"] == 0 and (mine["candidates"][1:] == max_candidates).all()
    assert (mine["variant"][1:] < 300).all()
    if max_candidates == 8:                                                 # the cut is by record order: only the first records are seen
        assert (mine["variant"][1:] < 8 + len(mine)).all()


# ------------------------------------------------------------------ ties
def test_ties(dev, oracle):
    got = _check(dev, oracle, RC.ties_case(oracle))
    mine = got[got["oligo"] == 0]
    assert (mine["gain"][1:] == 1).all() and len(mine) == 5                 # four one-sequence variants: the index decides
    assert mine["variant"][1:].tolist() == sorted(mine["variant"][1:].tolist())
    got = _check(dev, oracle, RC.expansions_tie_case(oracle))
    mine = got[got["oligo"] == 0]
    assert mine["n_expansions"].tolist() == [2, 3, 6]                       # 2 -> 3 at the degenerate slot wins over 2 -> 4
    assert mine["gain"].tolist() == [0, 2, 2] and mine["flags"].tolist() == [0, 0, api.REPAIR_COMPLETE]


# ------------------------------------------------------------------ degeneracy edges
def test_degeneracy_edges(dev, oracle):
    got = _check(dev, oracle, RC.degeneracy_case(oracle))                   # lands exactly on max_degeneracy = 4, then nothing fits
    mine = got[got["oligo"] == 0]
    assert mine["n_expansions"].tolist() == [1, 2, 4] and mine["flags"].tolist() == [0, 0, api.REPAIR_DEGENERACY]
    got = _check(dev, oracle, RC.degeneracy_case(oracle, max_degeneracy=3))   # over the cap by one candidate
    mine = got[got["oligo"] == 0]
    assert mine["n_expansions"].tolist() == [1, 2] and mine["flags"].tolist() == [0, api.REPAIR_DEGENERACY]
    got = _check(dev, oracle, RC.degeneracy_case(oracle, start_codes=((3, "R"), (15, "R")), max_degeneracy=16))
    assert got[got["oligo"] == 0]["n_expansions"].tolist() == [4, 8, 16]
    got = _check(dev, oracle, RC.degeneracy_case(oracle, start_codes=((4, "N"), (9, "N"), (12, "N"), (17, "N")), max_degeneracy=256))
    mine = got[got["oligo"] == 0]
    assert mine["n_expansions"].tolist() == [256] and mine["flags"].tolist() == [api.REPAIR_DEGENERACY]
    _compare(dev, oracle, RC.degeneracy_case(oracle, start_codes=((4, "N"), (9, "N"), (12, "N"), (17, "N")), max_degeneracy=256),
             max_degeneracy=16)                                             # the oligo itself is over the cap: step 0 alone


def test_max_steps(dev, oracle):
    got = _check(dev, oracle, RC.degeneracy_case(oracle, max_steps=0))
    assert got[got["oligo"] == 0]["flags"].tolist() == [api.REPAIR_STEPS]
    got = _check(dev, oracle, RC.degeneracy_case(oracle, max_steps=1))
    assert got[got["oligo"] == 0]["flags"].tolist() == [0, api.REPAIR_STEPS]
    got = _check(dev, oracle, RC.deep_case(oracle))
    mine = got[got["oligo"] == 0]
    assert len(mine) == 13 and mine[-1]["n_expansions"] == 256 and mine[-1]["flags"] == api.REPAIR_COMPLETE
    assert mine["gain"][1:].tolist() == list(range(12, 0, -1))


# ------------------------------------------------------------------ ambiguity codes and sequence ends
def test_ambiguity_and_ends(dev, oracle):
    case = RC.ambiguity_case(oracle)
    got = _check(dev, oracle, case)
    _, var = dev.site_variants(case["panel"], case["thr"], thermo=False)
    mine = got[got["oligo"] == 0]
    assert mine["sequences_held"].tolist() == [4, 8] and mine["candidates"].tolist() == [0, 1]   # the N-carrying double is no candidate
    assert mine["variants_held"].tolist() == [2, 4] and mine["flags"].tolist() == [0, api.REPAIR_COMPLETE]
    taken = var[int(mine[1]["variant"]):int(mine[1]["variant"]) + 1]
    assert set(api.variant_texts(taken)[0]) <= set("ACGT") and taken[0]["sequences"] == 2
    texts = api.variant_texts(var[var["oligo"] == 0])
    assert sum("N" in t for t in texts) == 2                                # held where N intersects: at step 0 one, after the union both
    got = _check(dev, oracle, SC.ends_case(oracle))                         # sites hanging over a sequence end: empty slots never match
    assert len(got) >= 6


# ------------------------------------------------------------------ max_mismatch and clamp3
@pytest.mark.parametrize("max_mismatch,clamp3", ((1, 3), (2, 0)))
def test_mismatch_and_clamp(dev, oracle, max_mismatch, clamp3):
    case = RC.mismatch_case(oracle, max_mismatch, clamp3)
    got = _check(dev, oracle, case)
    _, var = dev.site_variants(case["panel"], case["thr"], thermo=False)
    for o in (0, 1):
        mine, v = got[got["oligo"] == o], var[var["oligo"] == o]
        held = [bin(int(m)).count("1") <= max_mismatch and int(c) >= clamp3 for m, c in zip(v["mismatch_mask"], v["clamp3"])]
        assert mine[0]["variants_held"] == sum(held) and mine[0]["sites_held"] == int(v["sites"][np.array(held, bool)].sum())


# ------------------------------------------------------------------ panel shapes, caps, the other set
def _raw(d, case, cap, poison=False, which=api.TARGET, thermo=True):
    a = W.pairs_array(case["panel"])
    ids = np.zeros(max(2 * len(case["panel"]), 1), np.uint32)
    args = api.ThermoArgs(*(RC.THERMO[k] for k in ("salt", "primer_strand", "tm_min", "tm_max", "max_hairpin", "max_dimer")))
    out = np.zeros(max(cap, 1), api.REPAIR_STEP_DTYPE)
    if poison:
        out.view(np.uint8)[:] = 0xA5
    r = case.get("repair", {})
    n = d.L.pcr_site_repair(d.h, which, a.ctypes.data, len(case["panel"]), float(case["thr"]), r.get("max_degeneracy", 16),
                            r.get("max_mismatch", 0), r.get("clamp3", 0), r.get("max_candidates", 256), r.get("max_steps", 12),
                            C.byref(args) if thermo else None, 1, ids.ctypes.data, out.ctypes.data if cap else None, cap)
    return int(n), out


def test_panel_shapes_and_caps(dev, oracle):
    case = RC.shapes_case(oracle)
    got = _check(dev, oracle, case)
    ids, _ = _run(dev, case)
    assert ids.tolist() == [0, 1, 0, 2, 0, 3]                               # q in three pairs: one oligo, one set of steps
    assert got["oligo"].tolist() == [0, 0, 1, 1, 2, 3]
    sid, sites = dev.site_tm(case["panel"], case["thr"])
    assert set(sites[sites["oligo"] == 1]["strand"].tolist()) == {2}        # r2: strand-2 sites only
    assert got[4]["flags"] == api.REPAIR_COMPLETE and got[4]["sequences_total"] == 0 and got[4]["n_expansions"] == 1   # z: no site
    n, _ = _raw(dev, case, 0)                                               # cap = 0: the count
    assert n == len(got)
    n, out = _raw(dev, case, len(got) - 1, poison=True)                     # one short: the count, nothing written
    assert n == len(got) and (out.view(np.uint8) == 0xA5).all()
    n, out = _raw(dev, case, len(got) + 2, poison=True)
    assert n == len(got) and out[:n].tobytes() == got.tobytes() and (out[n:].view(np.uint8) == 0xA5).all()
    ids, small = dev.site_repair(case["panel"], case["thr"], cap=1, **RC.THERMO)   # the wrapper grows and retries
    assert small.tobytes() == got.tobytes()
    ids, none = dev.site_repair([], case["thr"])
    assert len(ids) == 0 and len(none) == 0 and none.dtype == api.REPAIR_STEP_DTYPE


def test_background_set(oracle):
    d = api.Screener(0)
    try:
        case = RC.free_coverage_case(oracle)
        _load(d, oracle, case, which=api.BACKGROUND)
        with pytest.raises(api.PcrError, match="no word DB"):
            _run(d, case)                                                   # the target set has none
        _compare(d, oracle, case, which=api.BACKGROUND)
    finally:
        d.close()


# ------------------------------------------------------------------ validity
def test_validity(dev, oracle):
    case = VC.ties_case(oracle)
    _load(dev, oracle, case)
    loose = dict(RC.THERMO, tm_min=40.0, max_dimer=25.0)
    for homo in (True, False):
        want = RC.expectation(oracle, case, thermo=loose, check_homo_dimer=homo)[1]
        ids, got = dev.site_repair(case["panel"], case["thr"], check_homo_dimer=homo, **loose)
        assert RC.as_tuples(got) == RC.as_tuples(want)
        words = [(int(r["word"][0]), int(r["word"][1])) for r in got]
        same = dev.is_valid(words, homo, flags=True, **loose)
        assert got["valid"].astype(bool).tolist() == same.tolist()
        assert got["valid"].tolist() == [1 if oracle.is_valid(w, check_homo_dimer=homo, **loose) else 0 for w in words]
    a = dev.site_repair(case["panel"], case["thr"], check_homo_dimer=True, **loose)[1]
    assert 0 < int(a["valid"].sum()) < len(a)                               # the thresholds tell the words apart
    ids, cold = dev.site_repair(case["panel"], case["thr"], thermo=False, salt=7.0, primer_strand=-1.0)   # ... none of which is read
    assert not cold["valid"].any()
    assert [t[:-1] for t in RC.as_tuples(cold)] == [t[:-1] for t in RC.as_tuples(a)]


# ------------------------------------------------------------------ end to end: the repaired panel holds what the steps claimed
def test_repaired_panel_holds_what_was_claimed(dev, oracle):
    case = RC.free_coverage_case(oracle)
    _load(dev, oracle, case)
    ids, steps = _run(dev, case)
    panel = api.repaired_panel(case["panel"], ids, steps, require_valid=False)
    assert panel[0][0] != tuple(case["panel"][0][0]) and panel[0][1] == tuple(int(x) for x in case["panel"][0][1])
    last = steps[steps["oligo"] == 0][-1]
    assert panel[0][0] == (int(last["word"][0]), int(last["word"][1]))
    dev.select_sites(panel, SC.SQ(case["thr"]))
    _, var, smap = dev.site_variants(panel, case["thr"], thermo=False, site_map=True)
    _, sites = dev.site_tm(panel, case["thr"])
    perfect = set(int(s["sequence"]) for s, v in zip(sites, smap.tolist()) if s["oligo"] == 0 and var[v]["mismatch_mask"] == 0)
    assert len(perfect) == int(last["sequences_held"]) == 12                # every sequence claimed has a perfect site of the new oligo
    ids2, again = dev.site_repair(panel, case["thr"], **RC.THERMO)
    assert again[again["oligo"] == 0]["flags"].tolist() == [api.REPAIR_COMPLETE]


# ------------------------------------------------------------------ stability and resources
def test_two_runs_identical_and_nothing_left(oracle):
    before = api.live_resources()
    d = api.Screener(0)
    try:
        case = SC.random_case(oracle)
        _load(d, oracle, case)
        entries = d.entries()
        a = d.site_repair(case["panel"], case["thr"], max_mismatch=1, **RC.THERMO)
        v1 = d.site_variants(case["panel"], case["thr"], site_map=True)
        b = d.site_repair(case["panel"], case["thr"], max_mismatch=1, **RC.THERMO)
        v2 = d.site_variants(case["panel"], case["thr"], site_map=True)
        assert len(a[1]) >= len(set(a[0].tolist()))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(v1, v2)) and d.entries() == entries
    finally:
        d.close()
    assert api.live_resources() == before
