"""melt_condition_cases without a device: the conditions under which tests/test_gpu_melt_conditions.py means something, asked of
the oracle alone, and the oracle held to the reference on the duplexes those scenarios melt.

The reference's answers are on this file's own tape, in the format and through the proxies of tests/reference_tape.py:
    PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_melt_conditions_host.py      # rewrites the file below
It holds every duplex of codes_case at melt_condition_cases.reference_conditions() -- 6 of the 24 conditions: every salt, both
primer concentrations, all four kinds of template concentration -- and every duplex of the three pool_case registrations.
"""
import gzip
import itertools
import json
import os

import numpy as np
import pytest

import reference_tape

import melt_condition_cases as MC
import probe_hit_cases as H
import products_tm_cases as PC
import site_tm_cases as SC
import site_variant_cases as VC

TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "melt_conditions_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"
MELT = ("tm_max", "tm_min", "dH", "dS")


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
def melt_reference(request, oracle, _tapes):
    """The compiled reference where it was built; elsewhere its recorded answers, checked against the oracle's (as the
    suite's `reference` fixture, on this file's own tape)."""
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


def _melt_bits(rec):
    return [tuple(int(np.float32(r[f]).view(np.uint32)) for f in MELT) for r in rec]


def _one_oligo(oracle, case, o, cond, entries, tamper=None):
    """The records of oligo o of codes_case alone, at a condition."""
    word = SC.distinct_oligos(case["panel"])[1][o]
    _, rec, _ = SC.expected_sites(oracle, entries, [(word, word)], case["thr"], salt=cond[0], primer_strand=cond[1],
                                  template_strand=cond[2], seqs=case["seqs"], cache=SC._CACHE, tamper=tamper)
    return rec


# ------------------------------------------------------------------ the scenario is what it says
def test_codes_case_is_as_described(oracle):
    case = MC.codes_case(oracle)
    ids, words = SC.distinct_oligos(case["panel"])
    assert ids == [0, 1, 2, 3, 4, 4] and len(case["seqs"]) == 1 and len(case["seqs"][0]) <= 16384
    assert [int(oracle.word_degeneracy(w)) for w in words] == list(MC.DEGENERACIES)
    for (n, places), w, text in zip(MC.OLIGOS, words, case["texts"]):
        sl = SC.slots_of(w)
        start, stop = oracle.word_start(w), oracle.word_stop(w)
        assert stop - start + 1 == n == len(text)
        folds = {start + p: fold for p, fold in places}
        assert {k: bin(v).count("1") for k, v in enumerate(sl) if bin(v).count("1") > 1} == folds
        assert all(start + 2 <= k <= stop - 2 for k in folds)                # interior: the flank slots are clipped to the word
    assert set("BYN") <= set(case["texts"][0])
    for k in (3, 4):                                                         # both sides of the seam between the word's halves
        deg = [i for i, v in enumerate(SC.slots_of(words[k])) if bin(v).count("1") > 1]
        assert 15 in deg and 16 in deg and min(deg) < 15
    assert max(i for i, v in enumerate(SC.slots_of(words[4])) if bin(v).count("1") > 1) > 16
    assert [len(p) for p in case["planted"]] == list(MC.DEGENERACIES[:MC.BIG]) + [MC.BIG_PLANTED]
    assert case["planted"][MC.BIG][0] == 0 and case["planted"][MC.BIG][-1] == MC.DEGENERACIES[MC.BIG] - 1
    _, rec, n_jobs = SC.expectation(oracle, MC.at(case, MC.DEFAULT))
    assert len(rec) == MC.CODES_SITES and n_jobs == MC.CODES_JOBS
    assert n_jobs > 12 * 256                                                 # more than one stride of 12-wave blocks on 256 CUs
    assert (rec["matches"] == [MC.OLIGOS[o][0] for o in rec["oligo"]]).all() and not rec["flags"].any()
    assert set(rec["strand"].tolist()) == {1, 2}
    assert [int(r["n_expansions"]) for r in rec] == [MC.DEGENERACIES[o] for o in rec["oligo"]]


def test_conditions_grid():
    grid = MC.conditions()
    assert len(grid) == len(set(grid)) == 24
    assert {c[0] for c in grid} == {0.05, 0.01, 1.0} and {c[1] for c in grid} == {9e-7, 2e-8}
    for salt, ps, ts in grid:
        ca = [np.float32(MC.duplex_strand(ps, d)) for d in MC.DEGENERACIES]
        cb = np.float32(ts)
        assert float(cb) == ts                                               # a float: the call sees the same number
        kind = MC.template_strands(ps).index(ts)
        above = [bool(a > cb) for a in ca]
        assert (kind == 0 and ts == 0.0) or (kind == 1 and all(above) and ts > 0) or (kind == 3 and not any(above)) \
            or (kind == 2 and any(above) and not all(above) and any(a == cb for a in ca))
    assert MC.COUNT_CONDITIONS == ((0.05, 9e-7, 0.0), (0.01, 2e-8, 0.0), (1.0, 9e-7, 5e-8))
    assert MC.POOL_CONDITIONS == ((0.01, 2e-8, 0.0), (1.0, 9e-7, 5e-8), (0.05, 2e-8, 2e-8))
    ref = MC.reference_conditions()
    assert len(ref) == 6 and {c[0] for c in ref} == {0.05, 0.01, 1.0} and {c[1] for c in ref} == {9e-7, 2e-8}
    assert {MC.template_strands(c[1]).index(c[2]) for c in ref} == {0, 1, 2, 3}


# ------------------------------------------------------------------ every expansion counts
@pytest.mark.parametrize("cond", MC.COUNT_CONDITIONS, ids=MC.condition_id)
def test_every_expansion_counts(oracle, cond):
    """Leaving an expansion out, or melting a copy of another one in its place, changes a record: a decode that drops or
    doubles an expansion cannot give the records the GPU test expects.  No exception among the expansions planted."""
    case = MC.codes_case(oracle)
    entries = SC.db_of(oracle, case)
    failed, asked = [], 0
    for o, planted in enumerate(case["planted"]):
        full = _melt_bits(_one_oligo(oracle, case, o, cond, entries))
        assert len(full) == len(planted)
        n = MC.DEGENERACIES[o]
        for e in planted:
            other = (e + 1) % n
            left_out = _melt_bits(_one_oligo(oracle, case, o, cond, entries, lambda _, x: x[:e] + x[e + 1:]))
            doubled = _melt_bits(_one_oligo(oracle, case, o, cond, entries, lambda _, x: x[:e] + [x[other]] + x[e + 1:]))
            asked += 1
            if left_out == full or doubled == full:
                failed.append((o, e))
    assert asked == sum(MC.DEGENERACIES[:MC.BIG]) + MC.BIG_PLANTED
    assert not failed, failed


@pytest.mark.parametrize("cond", MC.COUNT_CONDITIONS, ids=MC.condition_id)
def test_planted_expansion_is_the_unique_best_at_its_site(oracle, cond):
    """At its own site every planted expansion has the highest Tm, alone: tm_max, dH and dS of the site's record are its."""
    case = MC.codes_case(oracle)
    entries = SC.db_of(oracle, case)
    for o, planted in enumerate(case["planted"]):
        full = _one_oligo(oracle, case, o, cond, entries)                    # in sequence order: one oligo, one sequence
        for rec, e in zip(full, planted):
            alone = _one_oligo(oracle, case, o, cond, entries, lambda _, x: [x[e]])
            mine = alone[(alone["loc5"] == rec["loc5"]) & (alone["strand"] == rec["strand"])]
            assert len(mine) == 1
            assert _melt_bits(mine)[0][0] == _melt_bits([rec])[0][0] and _melt_bits(mine)[0][2:] == _melt_bits([rec])[0][2:], (o, e)
            rest = _one_oligo(oracle, case, o, cond, entries, lambda _, x: x[:e] + x[e + 1:])
            rest = rest[(rest["loc5"] == rec["loc5"]) & (rest["strand"] == rec["strand"])]
            assert rest[0]["tm_max"] < rec["tm_max"], (o, e)


# ------------------------------------------------------------------ no clamping, distinct conditions
def test_no_site_is_clamped(oracle):
    """The Tm is clamped at 0 C, which would hide differences: every exact site of codes_case melts above it, its weakest
    expansion included, at every condition."""
    case = MC.codes_case(oracle)
    lowest = {}
    for cond in MC.conditions():
        _, rec, _ = SC.expectation(oracle, MC.at(case, cond))
        lowest[cond] = float(rec["tm_min"].min())
        assert len(rec) == MC.CODES_SITES and (rec["tm_min"] > 0).all(), (cond, lowest[cond])
        assert (rec["tm_max"] > rec["tm_min"]).all()
    cond = min(lowest, key=lowest.get)
    print("the lowest tm_min: %.3f at %s" % (lowest[cond], MC.condition_id(cond)))


def test_conditions_are_distinct(oracle):
    """Any two conditions of the grid differ in some record; an oligo's records may coincide under two conditions (its duplex
    concentration is the same under both rules), never all oligos' at once."""
    case = MC.codes_case(oracle)
    per = {}
    for cond in MC.conditions():
        _, rec, _ = SC.expectation(oracle, MC.at(case, cond))
        per[cond] = [_melt_bits(rec[rec["oligo"] == o]) for o in range(len(MC.DEGENERACIES))]
    for a, b in itertools.combinations(MC.conditions(), 2):
        same = [o for o in range(len(MC.DEGENERACIES)) if per[a][o] == per[b][o]]
        if same:
            print("%s and %s coincide for the oligos %s" % (MC.condition_id(a), MC.condition_id(b), same))
        assert len(same) < len(MC.DEGENERACIES), (a, b)


def test_pool_case_is_as_described(oracle):
    names = MC.register_pool(oracle)
    case = MC.pool_case(oracle)
    base = PC.scenario(oracle, "random")
    assert len(case["seqs"]) == 8 and len(case["panel"]) == 6 and sum(len(s) for s in case["seqs"]) <= 16384
    changed = [(i, k) for i in range(6) for k in (0, 1) if case["panel"][i][k] != base["panel"][i][k]]
    assert changed == [(p, s) for p, s, _ in MC.POOL_WIDENED]
    for (p, s, code) in MC.POOL_WIDENED:
        w = case["panel"][p][s]
        assert MC.NIBBLE[code] in SC.slots_of(w) and oracle.word_degeneracy(w) == 3 * oracle.word_degeneracy(base["panel"][p][s])
    assert [(PC.scenario(oracle, n)["salt"], PC.scenario(oracle, n)["primer_strand"], PC.scenario(oracle, n)["template_strand"])
            for n in names] == list(MC.POOL_CONDITIONS)
    probes = H.scenario(oracle, names[0])
    assert probes["probe_strand"] == MC.POOL_PROBE_STRAND and probes["probes"] == [case["panel"][1][0], case["panel"][2][0]]
    default = PC.all_products(oracle, MC.POOL_DEFAULT)
    assert 3 in default[2]["n_expansions"] and default[3] <= 6000
    for name in names:
        ids, rec, sites, n_jobs = PC.all_products(oracle, name)
        assert n_jobs == default[3] and len(rec) == len(default[1]) >= 6
        assert PC.as_bits(rec) != PC.as_bits(default[1])
        assert len(H.everything(oracle, name)[4]) >= 1


# ------------------------------------------------------------------ the oracle against the reference
def _held(reference, oracle, jobs, salt):
    assert jobs
    for q, t, ca, cb in sorted(jobs):
        want = reference.heterodimer_full(q, t, salt, ca, cb)
        got = oracle.heterodimer_full(q, t, salt, ca, cb)
        assert want.view(np.uint32).tolist() == got.view(np.uint32).tolist(), (q, t, salt, ca, cb)


@pytest.mark.parametrize("cond", MC.reference_conditions(), ids=MC.condition_id)
def test_codes_duplexes_oracle_equals_reference(oracle, melt_reference, cond):
    """Every duplex of codes_case at the condition: reference.heterodimer_full == oracle.heterodimer_full, bit for bit."""
    jobs = set()
    _, _, n_jobs = SC.expectation(oracle, MC.at(MC.codes_case(oracle), cond), jobs=jobs)
    assert len(jobs) == n_jobs == MC.CODES_JOBS                             # every site spells its own target
    _held(melt_reference, oracle, jobs, cond[0])


@pytest.mark.parametrize("k", range(len(MC.POOL_NAMES)))
def test_pool_duplexes_oracle_equals_reference(oracle, melt_reference, k):
    """Every duplex the pool_case registration melts -- primers, probes and variants -- held to the reference."""
    name = MC.register_pool(oracle)[k]
    jobs = set()
    SC.expectation(oracle, PC.scenario(oracle, name), jobs=jobs)
    VC.expectation(oracle, PC.scenario(oracle, name), jobs=jobs)
    jobs |= H.jobs_of(oracle, name)
    _held(melt_reference, oracle, jobs, MC.POOL_CONDITIONS[k][0])
