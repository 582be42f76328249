"""pcr_pool_probe_candidates / Screener.probe_candidates on the GPU against the model of tests/probe_candidate_cases.py: the count
and every field of every record for every scenario and argument set, caps, the thermodynamic half against pcr_thermo bit for
bit, the background set, splits, the records of the product calls through the wrapper, the loop closed through probe_hits,
refusals with a handle, and the neighbouring calls."""
import ctypes as C

import numpy as np
import pytest

import probe_candidate_cases as PB
import probe_hit_cases as H
import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

PCR_ERR_ARG, PCR_ERR_STATE, PCR_ERR_CAPACITY = -1, -3, -4
POISON = 0xA5A5A5A5
SLACK = 4                                        # poisoned records behind what a call may write
SALT, PROBE_STRAND = 0.05, 2.5e-7
OPEN_LIMITS = dict(tm_min=-1.0e30, tm_max=1.0e30, max_hairpin=1.0e30, max_dimer=1.0e30)


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _load(d, sc, which=api.TARGET):
    d.load_texts(sc["seqs"], which=which)
    for s, p in sc.get("splits", ()):
        d.split(s, p, which=which)


def _raw(d, rec, grp, a, cap, limits=None, check_homo=False, which=api.TARGET):
    """One call on a poisoned buffer of cap + SLACK records -> (rc, the whole buffer)."""
    rec = np.ascontiguousarray(rec, api.PRODUCT_DTYPE)
    n = len(rec)
    out = np.full((cap + SLACK) * 16, POISON, np.uint32).view(api.PROBE_CANDIDATE_DTYPE)
    g = None if grp is None else np.ascontiguousarray(grp, np.uint32)
    args = api.ThermoArgs(SALT, PROBE_STRAND, limits["tm_min"], limits["tm_max"], limits["max_hairpin"], limits["max_dimer"]) if limits else None
    rc = d.L.pcr_pool_probe_candidates(d.h, which, rec.ctypes.data if n else None, None if g is None else g.ctypes.data, n,
                                       a["len_min"], a["len_max"], a["strands"], a["rules"], a["max_run"], a["gc_min"], a["gc_max"],
                                       a["min_sequences"], C.byref(args) if limits else None, int(check_homo), a["per_group"],
                                       out.ctypes.data if cap else None, cap)
    return rc, out


def _untouched(out, start):
    return (out[start:].view(np.uint32) == POISON).all()


def _same(got, want):
    assert len(got) == len(want)
    g, w = PB.as_bits(got), PB.as_bits(want)
    for i, (x, y) in enumerate(zip(g, w)):
        assert x == y, (i, got[i], want[i])


def _check(d, rec, grp, a, want, limits=None, check_homo=False, which=api.TARGET):
    """A counting call, a call with exactly enough room and one with one record too few, against the expected records."""
    n = len(want)
    rc, out = _raw(d, rec, grp, a, 0, limits, check_homo, which)
    assert rc == n, (rc, n, api._err(d.L))
    assert _untouched(out, 0)
    rc, out = _raw(d, rec, grp, a, n, limits, check_homo, which)
    assert rc == n
    _same(out[:n], want)
    assert _untouched(out, n)
    if n:
        rc, short = _raw(d, rec, grp, a, n - 1, limits, check_homo, which)
        assert rc == n and _untouched(short, n - 1)
    return out[:n]


def _device_melt(d, limits=OPEN_LIMITS, check_homo=False):
    """melt() of the model from Screener.is_valid (pcr_thermo) at the tests' salt and probe concentration."""
    def melt(words):
        return d.is_valid(words, check_homo, salt=SALT, primer_strand=PROBE_STRAND, **limits) if words else []
    return melt


# ------------------------------------------------------------------ 1. every scenario and argument set
@pytest.mark.parametrize("name", PB.SCENARIO_NAMES)
def test_scenario(dev, oracle, name):
    sc = PB.scenario(oracle, name)
    _load(dev, sc)
    for i, a in enumerate(sc["args"]):
        want = PB.expected(oracle, name, i)
        _check(dev, sc["records"], sc.get("group"), a, want)
        print("%s args %d: %d windows, %d candidates, %d records" % (name, i, PB.window_count(sc, a), len(PB.expected_candidates(oracle, name, i)), len(want)))


def test_n_zero_and_nothing_to_find(dev, oracle):
    sc = PB.scenario(oracle, "edges")
    _load(dev, sc)
    assert _raw(dev, sc["records"][:0], None, sc["args"][0], 4)[0] == 0
    assert _raw(dev, sc["records"][:1], None, sc["args"][0], 4)[0] == 0          # 19 bases: no window
    assert _raw(dev, sc["records"][3:4], None, sc["args"][0], 4)[0] == 0         # an empty insert
    assert _raw(dev, sc["records"], None, PB.args_of(gc_min=0.99, gc_max=1.0), 4)[0] == 0   # windows, none passes
    assert _raw(dev, sc["records"], np.full(len(sc["records"]), PB.NO_GROUP, np.uint32), sc["args"][0], 4)[0] == 0


# ------------------------------------------------------------------ 2. the thermodynamic half: pcr_thermo's floats and verdict
@pytest.mark.parametrize("check_homo", [False, True])
@pytest.mark.parametrize("name,i", [("support", 0), ("rules", 0), ("lengths", 2)])
def test_floats_and_verdict_are_pcr_thermos(dev, oracle, name, i, check_homo):
    sc = PB.scenario(oracle, name)
    _load(dev, sc)
    a = sc["args"][i]
    cands = PB.expected_candidates(oracle, name, i)
    words = [PB.word_of(c) for c in cands]
    # every candidate with limits that admit all: the four floats are is_valid's, bit for bit
    everything = PB.finish(cands, a, _device_melt(dev, OPEN_LIMITS, check_homo), OPEN_LIMITS, check_homo)
    got = _check(dev, sc["records"], sc.get("group"), a, everything, OPEN_LIMITS, check_homo)
    ref = dev.is_valid([(int(r["word"][0]), int(r["word"][1])) for r in got], check_homo, salt=SALT, primer_strand=PROBE_STRAND, **OPEN_LIMITS)
    assert len(got) == len(cands) and all(r["valid"] for r in ref)
    for r, t in zip(got, ref):
        for f in ("tm", "hairpin_tm", "homodimer_tm", "dG"):
            assert np.float32(r[f]).view(np.uint32) == np.float32(t[f]).view(np.uint32), (f, r, t)
    assert bool((got["homodimer_tm"] != 0).any()) == check_homo
    # limits through the middle of what the candidates melt at: the kept set is the words is_valid calls valid
    tms, hps = np.sort(got["tm"]), np.sort(got["hairpin_tm"])
    limits = dict(tm_min=float(tms[len(tms) // 4]), tm_max=float(tms[-1 - len(tms) // 8]), max_hairpin=float(hps[-1 - len(hps) // 8]),
                  max_dimer=float(np.sort(got["homodimer_tm"])[len(got) // 2]))
    flags = dev.is_valid(words, check_homo, salt=SALT, primer_strand=PROBE_STRAND, flags=True, **limits)
    assert 0 < int(flags.sum()) < len(words)
    want = PB.finish(cands, a, _device_melt(dev, limits, check_homo), limits, check_homo)
    assert {tuple(int(v) for v in r["word"]) for r in want} == {w for w, ok in zip(words, flags) if ok}
    _check(dev, sc["records"], sc.get("group"), a, want, limits, check_homo)
    # and with the cut taken after the filter
    cut = dict(a, per_group=2)
    _check(dev, sc["records"], sc.get("group"), cut, PB.finish(cands, cut, _device_melt(dev, limits, check_homo), limits, check_homo), limits, check_homo)


def test_floats_are_the_oracles(dev, oracle):
    """The model completed with the oracle's NucCruc instead of the device's own pcr_thermo."""
    sc = PB.scenario(oracle, "support")
    _load(dev, sc)
    a = sc["args"][0]
    limits = dict(tm_min=45.0, tm_max=64.0, max_hairpin=35.0, max_dimer=30.0)
    for check_homo in (False, True):
        want = PB.finish(PB.expected_candidates(oracle, "support", 0), a, PB.oracle_melt(oracle, SALT, PROBE_STRAND), limits, check_homo)
        _check(dev, sc["records"], None, a, want, limits, check_homo)


# ------------------------------------------------------------------ 3. the other set, splits, the product calls' records, pool grouping
def test_background_set(dev, oracle):
    _load(dev, PB.scenario(oracle, "edges"), which=api.TARGET)
    sc = PB.scenario(oracle, "holes")
    _load(dev, sc, which=api.BACKGROUND)
    _check(dev, sc["records"], sc["group"], sc["args"][0], PB.expected(oracle, "holes", 0), which=api.BACKGROUND)


def test_a_split_removes_the_windows_around_it(dev, oracle):
    sc = dict(PB.scenario(oracle, "support"))
    _load(dev, sc)
    a = sc["args"][0]
    before = _check(dev, sc["records"], None, a, PB.expected(oracle, "support", 0))
    assert int(before["sequences"].max()) == PB.SUPPORT_TOP
    start, n = PB.region_of(sc["records"][1], PB.INSERT)
    dev.split(1, start + n // 2)
    sc["splits"] = [(1, start + n // 2)]
    after = _check(dev, sc["records"], None, a, PB.finish(PB.candidates(sc, a), a))
    assert int(after["sequences"].max()) == PB.SUPPORT_TOP - 1 and int(after["sequences"].sum()) < int(before["sequences"].sum())   # sequence 1 holds no window any more


def _wrapper_args(a, **more):
    kw = dict(len_min=a["len_min"], len_max=a["len_max"], strands=a["strands"], no_5g=bool(a["rules"] & PB.NO_5G), c_ge_g=bool(a["rules"] & PB.C_GE_G),
              max_run=a["max_run"], gc_min=a["gc_min"], gc_max=a["gc_max"], min_sequences=a["min_sequences"], per_group=a["per_group"], thermo=False)
    kw.update(more)
    return kw


def test_records_of_the_product_calls_and_pool_grouping(dev, oracle):
    case = H.scenario(oracle, "ladder")
    dev.load_texts(case["seqs"])
    dev.select_sites(H.db_case(case)["panel"], SC.SQ(case["thr"]))
    lo, hi = PC.amp_of(case)
    kw = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, template_strand=case.get("template_strand", 0.0), amp_min=lo, amp_max=hi)
    ids, prod = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)
    _, prod_tm = dev.pool_products_tm(case["panel"], case["thr"], **kw)
    _, _, hits = dev.probe_hits(case["panel"], case["probes"], case["thr"], probe_strand=case.get("probe_strand", H.PROBE_STRAND), **kw)
    assert len(prod) and len(prod_tm) == len(prod) and len(hits)
    sc = dict(seqs=case["seqs"])
    a = PB.args_of(len_max=22, per_group=4, **PB.PROBE_RULES)
    for rec in (prod, prod_tm, hits):
        grp = PB.groups_of(len(case["panel"]), ids, rec)
        want = PB.finish(PB.candidates(sc, a, records=rec, group=grp), a)
        assert len(want)
        _same(dev.probe_candidates(rec, pool=case["panel"], ids=ids, **_wrapper_args(a)), want)
        _same(dev.probe_candidates(rec, group=grp, cap=1, **_wrapper_args(a)), want)                  # the retry on the count
        _same(dev.probe_candidates(rec, **_wrapper_args(a)), PB.finish(PB.candidates(sc, a, records=rec, group=np.zeros(len(rec), np.uint32)), a))
    # a pool in which no pair owns the records: every record is NO_GROUP
    other = [(case["panel"][0][0], case["panel"][0][0])]
    assert len(dev.probe_candidates(prod, pool=other, ids=[ids[0], ids[0]], **_wrapper_args(a))) == 0
    # thermo=True through the wrapper: is_valid's verdict at the wrapper's own limits
    got = dev.probe_candidates(prod, pool=case["panel"], ids=ids, per_group=0, tm_min=55.0, tm_max=70.0)
    a_def = PB.args_of(per_group=0, **PB.PROBE_RULES)
    limits = dict(tm_min=55.0, tm_max=70.0, max_hairpin=40.0, max_dimer=40.0)
    _same(got, PB.finish(PB.candidates(sc, a_def, records=prod, group=PB.groups_of(len(case["panel"]), ids, prod)), a_def, _device_melt(dev, limits), limits))


# ------------------------------------------------------------------ 4. the loop closed: the proposed probe lights up what supports it
def test_best_probes_hit_the_sequences_that_support_them(dev, oracle):
    sc = PB.loop_case(oracle)
    dev.load_texts(sc["seqs"])
    pool = sc["panel"]
    ids, prod = dev.pool_products(pool, 1.0, *PB.LOOP_AMP, select="all")
    assert set(prod["sequence"].tolist()) == set(range(len(sc["seqs"])))
    a = PB.args_of(per_group=1, **PB.PROBE_RULES)
    got = dev.probe_candidates(prod, pool=pool, ids=ids, **_wrapper_args(a))
    cands = PB.candidates(sc, a, records=prod, group=PB.groups_of(len(pool), ids, prod))
    _same(got, PB.finish(cands, a))
    probes = api.best_probes(got, len(pool))
    assert all(p is not None for p in probes)
    _, pid, hits, detected = dev.probe_hits(pool, probes, 1.0, tm_floor=0.0, probe_tm_floor=0.0, amp_min=PB.LOOP_AMP[0], amp_max=PB.LOOP_AMP[1],
                                            select="all", bits=True)
    for g in range(len(pool)):
        top = next(c for c in cands if c["group"] == g)
        assert PB.word_of(top) == probes[g] and len(top["support"]) >= 2
        mine = hits[((hits["intended"] & api.HIT_PROBE_INTENDED) != 0) & (hits["probe"] == pid[g])]
        lit = set(mine["sequence"].tolist())
        assert top["support"] <= lit, (g, sorted(top["support"]), sorted(lit))
        assert top["support"] <= {s for s in range(len(sc["seqs"])) if api.bits_to_bool(detected[g], len(sc["seqs"]))[s]}


# ------------------------------------------------------------------ 5. refusals with a handle
def test_refusals_with_a_handle(dev, oracle):
    sc = PB.scenario(oracle, "groups")
    _load(dev, sc)
    a = sc["args"][0]
    want = PB.expected(oracle, "groups", 0)
    rec, grp = np.array(sc["records"], api.PRODUCT_DTYPE), np.array(sc["group"], np.uint32)
    for bad in (PB.MAX_GROUPS, 0xFFFFFFFE):
        g = grp.copy()
        g[1] = bad
        rc, _ = _raw(dev, rec, g, a, 8)
        assert rc == PCR_ERR_ARG and "record 1" in api._err(dev.L) and "group" in api._err(dev.L)
    # the NO_GROUP record that lies outside its sequence is not looked at; the same record in a group is refused by index
    g = grp.copy()
    g[4] = 0
    rc, _ = _raw(dev, rec, g, a, 8)
    assert rc == PCR_ERR_ARG and "record 4" in api._err(dev.L)
    g[3] = 0                                                                  # 80 .. 109 of 90 bases: the first of the two is named
    rc, _ = _raw(dev, rec, g, a, 8)
    assert rc == PCR_ERR_ARG and "record 3" in api._err(dev.L)
    r = rec.copy()
    r[0] = PB.record(PB.INSERT, 0, 30, -1)                                    # negative in length
    rc, _ = _raw(dev, r, grp, a, 8)
    assert rc == PCR_ERR_ARG and "record 0" in api._err(dev.L)
    rc, _ = _raw(dev, r, None, a, 8)                                          # group = NULL: every record takes part
    assert rc == PCR_ERR_ARG and "record 0" in api._err(dev.L)
    _check(dev, rec, grp, a, want)                                            # a good call follows
    # 2^28 windows from a few long inserts, added up on the host: nothing is allocated
    long_seq = "ACGT" * 150000
    dev.load_texts([long_seq])
    held = api.live_resources()[0]
    many = np.array([PB.record(PB.INSERT, 0, 0, len(long_seq))] * 8, api.PRODUCT_DTYPE)
    wide = PB.args_of(len_min=1, len_max=32)
    assert PB.window_count(dict(records=many), wide) >= 1 << 28 > PB.window_count(dict(records=many[:6]), wide)
    rc, _ = _raw(dev, many, None, wide, 0)
    assert rc == PCR_ERR_CAPACITY and "2^28" in api._err(dev.L)
    assert api.live_resources()[0] == held
    with pytest.raises(api.PcrError) as e:
        dev.probe_candidates(many, len_min=1, len_max=32, thermo=False)
    assert e.value.rc == PCR_ERR_CAPACITY
    # a set that was never loaded
    d = api.Screener(0)
    try:
        rc, _ = _raw(d, rec, grp, a, 8)
        assert rc == PCR_ERR_STATE and "not loaded" in api._err(d.L)
        _load(d, sc)
        _check(d, rec, grp, a, want)
        assert _raw(d, rec, grp, a, 8, which=api.BACKGROUND)[0] == PCR_ERR_STATE
    finally:
        d.close()


# ------------------------------------------------------------------ 6. the neighbouring calls; the handle's resources
def test_neighbouring_calls_are_unchanged(dev, oracle):
    case = PC.scenario(oracle, "ladder")
    dev.load_texts(case["seqs"])
    dev.select_sites(case["panel"], SC.SQ(case["thr"]))
    lo, hi = PC.amp_of(case)
    entries = dev.entries()
    ids, prod = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)
    info, texts = dev.product_amplicons(prod, api.REGION_INSERT, sequences=True)
    assert len(prod) == 27
    for thermo in (False, True):
        for check_homo in (False, True):
            got = dev.probe_candidates(prod, pool=case["panel"], ids=ids, thermo=thermo, check_homo_dimer=check_homo, tm_min=40.0)
            assert len(got)
    assert dev.entries() == entries
    ids2, prod2 = dev.pool_products(case["panel"], case["thr"], lo, hi, select=False)
    assert ids2.tolist() == ids.tolist() and prod2.tobytes() == prod.tobytes()
    info2, texts2 = dev.product_amplicons(prod, api.REGION_INSERT, sequences=True)
    assert info2.tobytes() == info.tobytes() and texts2 == texts


def test_the_handle_gives_everything_back(oracle):
    start = api.live_resources()
    d = api.Screener(0)
    try:
        sc = PB.scenario(oracle, "support")
        _load(d, sc)
        limits = dict(tm_min=40.0, tm_max=80.0, max_hairpin=60.0, max_dimer=60.0)
        assert _raw(d, sc["records"], None, sc["args"][0], 64, limits, True)[0] > 0
        assert api.live_resources()[0] > start[0]
    finally:
        d.close()
    assert api.live_resources() == start
