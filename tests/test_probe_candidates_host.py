"""pcr_pool_probe_candidates without a device: the symbol, the record layout and the Python names, the refusals that come before
the handle in their order, the properties of the scenarios that tests/test_gpu_probe_candidates.py relies on, the model's
thermodynamic verdict held to the oracle's PCR::is_valid, and api.best_probes."""
import ctypes as C

import numpy as np
import pytest

import probe_candidate_cases as PB
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


def test_symbol_is_exported(lib):
    assert "pcr_pool_probe_candidates" in api.ABI_SYMBOLS
    assert hasattr(lib, "pcr_pool_probe_candidates"), "libpcramp_hip.so does not export pcr_pool_probe_candidates"
    assert api.PROBE_CANDIDATE_DTYPE.itemsize == 64 and api.PROBE_CANDIDATE_DTYPE == PB.CANDIDATE
    assert (api.PROBE_NO_5G, api.PROBE_C_GE_G, api.NO_GROUP) == (PB.NO_5G, PB.C_GE_G, PB.NO_GROUP) == (1, 2, 0xFFFFFFFF)
    assert api.POOL_MAX_PAIRS == PB.MAX_GROUPS
    assert callable(api.Screener.probe_candidates) and callable(api.best_probes)


def _call(lib, which=api.TARGET, n=1, products=True, cap=0, out=False, thermo=None, **kw):
    a = PB.args_of(**kw)
    rec = np.zeros(4, api.PRODUCT_DTYPE)                                      # (n may lie: nothing is read before the handle)
    buf = np.zeros(4, api.PROBE_CANDIDATE_DTYPE)
    args = api.ThermoArgs(*thermo) if thermo else None
    rc = lib.pcr_pool_probe_candidates(None, which, rec.ctypes.data if products else None, None, n, a["len_min"], a["len_max"], a["strands"],
                                       a["rules"], a["max_run"], a["gc_min"], a["gc_max"], a["min_sequences"], C.byref(args) if thermo else None,
                                       0, a["per_group"], buf.ctypes.data if out else None, cap)
    return rc, api._err(lib)


GOOD_THERMO = (0.05, 2.5e-7, 65.0, 75.0, 40.0, 40.0)


def test_refusals_before_the_handle(lib):
    """The set, the pointers, the count, the lengths, the strands, the rule bits, the G+C bounds, the thermodynamic arguments, then
    the handle: each call is wrong in one thing and in the handle and the message names the one thing; two things wrong name the
    earlier."""
    def refused(text, **kw):
        rc, msg = _call(lib, **kw)
        assert rc == PCR_ERR_ARG and text in msg, (kw, rc, msg)

    refused("null handle")
    refused("null handle", which=api.BACKGROUND, n=0, products=False)         # n = 0 needs no records, but a handle
    refused("null handle", cap=4, out=True, thermo=GOOD_THERMO, len_min=1, len_max=32, strands=1, rules=3)
    refused("unknown sequence set", which=7, products=False)                  # ... comes before the pointers
    refused("PCR_SET_MULTIPLEX", which=api.MULTIPLEX, n=1 << 31)              # ... and before the count
    refused("bad argument", products=False)
    refused("bad argument", cap=4)                                            # cap without out
    refused("bad argument", cap=4, n=1 << 31)                                 # ... comes before the count
    for n in (1 << 31, 1 << 40):
        refused("2^31", n=n)
    refused("2^31", n=1 << 31, len_min=0)                                     # ... comes before the lengths
    refused("null handle", n=(1 << 31) - 1)
    for lo, hi in ((0, 20), (21, 20), (20, 33), (33, 40), (0, 0)):
        refused("len_min", len_min=lo, len_max=hi)
    refused("len_min", len_min=0, strands=0)                                  # ... come before the strands
    for s in (0, 4, 7):
        refused("strands", strands=s)
    refused("strands", strands=0, rules=4)                                    # ... come before the rule bits
    for r in (4, 8, 0x80000000, 7):
        refused("rule bits", rules=r)
    refused("rule bits", rules=4, gc_min=float("nan"))                        # ... come before the G+C bounds
    for lo, hi in ((float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.5), (0.6, 0.5)):
        refused("gc_min", gc_min=lo, gc_max=hi)
    refused("gc_min", gc_min=0.6, gc_max=0.5, thermo=(0.05, 0.0, 65.0, 75.0, 40.0, 40.0))   # ... come before the concentration
    for strand in (0.0, -1.0e-7, float("nan")):
        refused("primer_strand", thermo=(0.05, strand, 65.0, 75.0, 40.0, 40.0))
    refused("primer_strand", thermo=(2.0, 0.0, 65.0, 75.0, 40.0, 40.0))       # ... comes before the salt
    for salt in (0.0, 1.0e-7, 1.5, float("nan")):
        refused("salt", thermo=(salt, 2.5e-7, 65.0, 75.0, 40.0, 40.0))
    refused("null handle", thermo=(1.0e-6, 2.5e-7, 65.0, 75.0, 40.0, 40.0))
    refused("null handle", gc_min=0.5, gc_max=0.5)


# ------------------------------------------------------------------ what the GPU tests rely on
def _by_text(cands):
    return {(c["group"], W.text_from_codes(np.frombuffer(c["text"], np.uint8))): c for c in cands}


def test_edges_and_lengths():
    sc = PB.scenario(None, "edges")
    a = sc["args"][0]
    per_record = [len(PB.candidates(sc, a, records=sc["records"][k:k + 1])) for k in range(len(sc["records"]))]
    assert per_record[:4] == [0, 2, 6, 0]                                     # 19 bases: nothing; 20: one window; 21: three; empty: nothing
    starts = [PB.region_of(r, PB.INSERT)[0] for r in sc["records"]]
    assert {s & 31 for s in starts} >= {0, 1, 30, 31}
    assert sum(PB.region_of(r, PB.INSERT) == (PB.EDGE_TAIL - 20, 20) and r["sequence"] == 1 for r in sc["records"]) == 1 and PB.EDGE_TAIL % 32
    assert PB.window_count(sc, a) == 172 and PB.window_count(sc, sc["args"][1]) == 86
    sc = PB.scenario(None, "lengths")
    n = [len(PB.expected_candidates(None, "lengths", i)) for i in range(3)]
    assert n[0] == 4 and n[1] == 2 * 9 and n[2] > 1000                        # single bases: A, C, G, T; nine 32-mers on two strands
    assert {c["length"] for c in PB.expected_candidates(None, "lengths", 2)} == set(range(1, 33))
    sc = PB.scenario(None, "long")
    assert sorted(PB.region_of(r, PB.INSERT)[1] for r in sc["records"]) == [65, 2049]
    firsts = {c["first"][2] for c in PB.expected_candidates(None, "long", 0)}
    assert max(firsts) > 120 + 2000 and any(31 + 32 < f < 31 + 65 for f in firsts)   # starts past the 62nd block of an insert, and in a third


def test_holes():
    sc = PB.scenario(None, "holes")
    cands = PB.expected_candidates(None, "holes", 0)
    per_group = [sum(c["group"] == g for c in cands) for g in range(7)]
    whole = per_group[0]
    assert whole == 2 * sum(44 - n + 1 for n in range(20, 25))
    assert per_group[1] == per_group[4] and per_group[2] == per_group[5] and per_group[3] == per_group[6]   # an EOS and an N cost the same
    assert 0 < per_group[2] < per_group[1] == per_group[3] < whole            # a hole in the middle costs more than one at an end
    codes = PB.codes_of(sc)
    assert all(codes[1 + i][p] == 0 and codes[4 + i][p] == 15 for i, p in enumerate(PB.HOLE_AT))
    for g in (1, 4):                                                          # the first base: the windows from the second base on stay
        assert min(c["first"][2] for c in cands if c["group"] == g) == PB.HOLE_AT[0] + 1
    for g in (3, 6):                                                          # the last base: the windows that end before it stay
        assert max(c["first"][2] + c["length"] for c in cands if c["group"] == g) == PB.HOLE_AT[2]
    for g in (2, 5):
        assert all(c["first"][2] + c["length"] <= PB.HOLE_AT[1] or c["first"][2] > PB.HOLE_AT[1] for c in cands if c["group"] == g)


def test_strands_and_counts():
    (c,) = PB.expected_candidates(None, "palindrome", 0)
    assert (c["sequences"], c["records"], c["first"][3]) == (1, 1, 1)         # two occurrences in one record: counted once, strand 1 first
    (c2,) = PB.expected_candidates(None, "palindrome", 2)
    assert c2["text"] == c["text"] and c2["first"][3] == 2
    sc = PB.scenario(None, "twice")
    by = _by_text(PB.expected_candidates(None, "twice", 0))
    w = by[(0, sc["word"])]
    assert (w["sequences"], w["records"], w["first"]) == (1, 2, (0, 0, 30, 1))   # twice in record 0 (30 and 57), once in record 1
    assert sc["seqs"][0].count(sc["word"]) == 2
    both = PB.expected_candidates(None, "both_strands", 0)
    assert len(both) == 2 and all((c["sequences"], c["records"]) == (2, 2) for c in both)   # the insert and its reverse complement, each in both
    assert sorted(c["first"][3] for c in both) == [1, 2] and all(c["first"][0] == 0 for c in both)
    plus = PB.expected_candidates(None, "both_strands", 1)
    assert len(plus) == 2 and all((c["sequences"], c["records"]) == (1, 1) for c in plus)
    assert {c["text"] for c in plus} == {c["text"] for c in both}
    groups = PB.expected_candidates(None, "groups", 0)
    assert {c["group"] for c in groups} == {5, 1023} and len(groups) == 2 * 12
    assert {c["text"] for c in groups if c["group"] == 5} == {c["text"] for c in groups if c["group"] == 1023}
    assert all(c["sequences"] == 1 for c in groups) and PB.expected_candidates(None, "groups", 1) == []
    sc = PB.scenario(None, "groups")
    assert (sc["group"] == PB.NO_GROUP).sum() == 3 and int(sc["records"][4]["sequence"]) >= len(sc["seqs"])


def test_rules_scenario():
    sc = PB.scenario(None, "rules")
    g = {name: i for i, name in enumerate(sc["names"])}
    assert all(len(w) == 20 for w in PB.RULE_WORDS.values())
    strands = lambda i, names: {name: sorted(c["first"][3] for c in PB.expected_candidates(None, "rules", i) if c["group"] == g[name]) for name in names}
    assert all(v == [1, 2] for v in strands(0, sc["names"]).values())         # no rule: every word on both strands
    s = strands(1, ("five_g", "five_g_rc", "c_gt_g"))
    assert s == dict(five_g=[], five_g_rc=[1], c_gt_g=[1, 2])                 # 5' G as oriented
    s = strands(2, ("c_gt_g", "c_eq_g"))
    assert s == dict(c_gt_g=[1], c_eq_g=[1, 2])                               # C >= G picks the strand; a tie passes on both
    s = strands(3, ("run4_first", "run5_first", "run4_last", "run5_last"))
    assert s == dict(run4_first=[1, 2], run5_first=[], run4_last=[1, 2], run5_last=[])
    s = strands(4, ("gc_5", "gc_6", "gc_16", "gc_17"))
    assert s == dict(gc_5=[], gc_6=[1, 2], gc_16=[1, 2], gc_17=[])            # exactly on the bounds, in float
    assert np.float32(6) / np.float32(20) == np.float32(0.3) and np.float32(16) / np.float32(20) == np.float32(0.8)
    assert 0.3 != float(np.float32(0.3))                                      # (in double the lower bound would not be met)
    together = PB.expected_candidates(None, "rules", 5)
    assert 0 < len(together) < len(PB.expected_candidates(None, "rules", 1))
    assert PB.expected_candidates(None, "rules", 6) == [] and len(PB.expected_candidates(None, "rules", 7)) == 24


def test_support_and_the_rest():
    c = PB.expected_candidates(None, "support", 0)
    top = [x for x in c if x["sequences"] == PB.SUPPORT_TOP]
    assert len(top) == 5 and all(x["records"] == 3 and x["length"] == 20 for x in top) and len(c) == 10
    assert [x["text"] for x in top] == sorted(x["text"] for x in top)         # only the text orders them
    assert [len(PB.expected_candidates(None, "support", i)) for i in (1, 2, 3)] == [5, 7, 0]
    cut = PB.expected(None, "support", 4)
    assert len(cut) == 2 and [tuple(r["word"]) for r in cut] == [PB.word_of(x) for x in top[:2]]
    assert len(PB.expected(None, "support", 6)) == 6
    ids = PB.expected(None, "seq_ids", 0)
    assert len(ids) == 70 and (ids["sequences"] == 5).all() and (ids["records"] == 9).all()
    assert {int(s) for s in PB.scenario(None, "seq_ids")["records"]["sequence"]} == {0, 1, 63, 64, 128}
    many = PB.scenario(None, "many")
    assert len(many["records"]) == PB.MANY_RECORDS and PB.window_count(many, many["args"][0]) > 256 * 256 * 8
    starts = PB.MANY_RECORDS * (25 - many["args"][0]["len_min"] + 1)
    assert (starts + 255) // 256 == 2188 > 256 * 8                            # chunks of 256 starts against 8 blocks per CU of an MI355X's 256: the enumeration's grid strides
    m = PB.expected(None, "many", 0)
    assert len(m) == 15 and m["group"].tolist() == [g for g in range(3) for _ in range(5)] and int(m["records"].max()) > 200


def test_panel_scenarios(oracle):
    for name in PB.PANEL_SCENARIOS:
        sc = PB.scenario(oracle, name)
        assert len(sc["records"]) and (sc["group"] != PB.NO_GROUP).any()
        assert len(PB.expected(oracle, name, 0))
    rnd = PB.scenario(oracle, "random")
    assert (rnd["group"] == PB.NO_GROUP).any() and len(set(rnd["group"].tolist())) > 3
    loop = PB.loop_case()
    assert len(loop["seqs"]) == 6 and len(loop["panel"]) == 2


# ------------------------------------------------------------------ the model's verdict against the oracle's is_valid
@pytest.mark.parametrize("name,i", [("support", 0), ("rules", 0)])
@pytest.mark.parametrize("check_homo", [False, True])
def test_model_verdict_is_the_oracles_is_valid(oracle, name, i, check_homo):
    sc = PB.scenario(oracle, name)
    cands = PB.expected_candidates(oracle, name, i)
    salt, strand = 0.05, 2.5e-7
    everything = PB.finish(cands, sc["args"][i], PB.oracle_melt(oracle, salt, strand), dict(tm_min=-1e30, tm_max=1e30, max_hairpin=1e30, max_dimer=1e30), check_homo)
    assert len(everything) == len(cands)
    tms = np.sort(everything["tm"])
    limits = dict(tm_min=float(tms[len(tms) // 4]), tm_max=float(tms[-1 - len(tms) // 8]), max_hairpin=float(np.sort(everything["hairpin_tm"])[-2]),
                  max_dimer=float(np.sort(everything["homodimer_tm"])[len(tms) // 2]))
    kept = PB.finish(cands, sc["args"][i], PB.oracle_melt(oracle, salt, strand), limits, check_homo)
    want = [PB.word_of(c) for c in cands if oracle.is_valid(PB.word_of(c), salt, strand, limits["tm_min"], limits["tm_max"], limits["max_hairpin"],
                                                            limits["max_dimer"], check_homo)]
    assert 0 < len(want) < len(cands)
    assert sorted(tuple(int(v) for v in r["word"]) for r in kept) == sorted(want)


# ------------------------------------------------------------------ best_probes
def test_best_probes():
    rec = np.zeros(5, api.PROBE_CANDIDATE_DTYPE)
    rec["group"] = [0, 0, 2, 2, 5]
    rec["word"] = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10)]
    assert api.best_probes(rec, 4) == [(1, 2), None, (5, 6), None]            # the first of each group; a group beyond the pool is left out
    assert api.best_probes(rec, 6) == [(1, 2), None, (5, 6), None, None, (9, 10)]
    assert api.best_probes(rec[:0], 2) == [None, None] and api.best_probes(rec, 0) == []
    words = api.best_probes(PB.expected(None, "support", 4), 1)
    assert words == [tuple(int(v) for v in PB.expected(None, "support", 4)[0]["word"])] and len(W.word_text(words[0])) == 20
