"""pcr_pool_probe_hits without a device: the symbol and the record layout, the refusals that come before the handle in their
order, the properties of the scenarios that tests/test_gpu_probe_hits.py relies on (computed with the CPU oracle, so that no
GPU assertion is vacuous), and the oracle held to the reference on every duplex the scenarios melt."""
import ctypes as C
import gzip
import json
import os
import random

import numpy as np
import pytest

import reference_tape

import probe_hit_cases as H
import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W
from testdata import rand_seq

PCR_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


# The reference's answers to this file's calls, on a tape of its own (the format and proxies of tests/reference_tape.py):
#     PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_probe_hits_host.py      # rewrites the file below
TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_hits_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"


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
def probe_reference(request, oracle, _tapes):
    """The compiled reference where it was built; elsewhere its recorded answers, checked against the oracle's."""
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


def test_symbol_is_exported(lib):
    assert "pcr_pool_probe_hits" in api.ABI_SYMBOLS
    assert hasattr(lib, "pcr_pool_probe_hits"), "libpcramp_hip.so does not export pcr_pool_probe_hits"
    assert api.PROBE_HIT_DTYPE.itemsize == 64 and H.HIT == api.PROBE_HIT_DTYPE
    assert (api.HIT_PRODUCT_INTENDED, api.HIT_PROBE_INTENDED, api.HIT_PROBE_NO_TM) == (1, 2, 4)
    assert (H.PRODUCT_INTENDED, H.PROBE_INTENDED, H.PROBE_NO_TM) == (1, 2, 4)
    assert api.NO_PROBE == H.NO_PROBE == 0xFFFFFFFF
    assert hasattr(api.Screener, "probe_hits")


def _call(lib, which, pool, probes="same", template_strand=0.0, primer_strand=9e-7, probe_strand=2.5e-7, salt=0.05, tm_floor=0.0,
          probe_tm_floor=0.0, ids=True, pids=True, args=True, has_pool=True, cap=0):
    """A call on the null handle.  probes: a list of words / None per pair, "same" for one fixed probe everywhere, None for a
    null pointer."""
    a = W.pairs_array(pool) if pool else np.zeros((1, 4), np.uint64)
    if probes == "same":
        probes = [PROBE] * len(pool)
    pr = None
    if probes is not None:
        pr = np.zeros((max(len(pool), 1), 2), np.uint64)
        for i, p in enumerate(probes):
            if p is not None:
                pr[i] = (p[0], p[1])
    oid = np.zeros(max(2 * len(pool), 1), np.uint32)
    pid = np.zeros(max(len(pool), 1), np.uint32)
    th = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    rc = lib.pcr_pool_probe_hits(None, which, a.ctypes.data if has_pool else None, pr.ctypes.data if pr is not None else None,
                                 len(pool), 0.9, 80, 200, C.byref(th) if args else None, float(probe_strand), float(template_strand),
                                 float(tm_floor), float(probe_tm_floor), oid.ctypes.data if ids else None,
                                 pid.ctypes.data if pids else None, None, cap, None)
    return rc, api._err(lib)


PROBE = W.centered_word(W.codes_from_text("GATTACAGGCTTACCGATGCAA"))


def test_refusals_before_the_handle(lib, oracle):
    """The order of include/pcramp_hip.h: each call below is wrong in one thing and in the handle, and the message names the
    one thing; two things wrong name the earlier."""
    w = oracle.centered_word
    assert tuple(int(x) for x in PROBE) == tuple(int(x) for x in w("GATTACAGGCTTACCGATGCAA"))
    pair = (w("ACGTTGCAAGCTTGCATGCA"), w("TTGACCGTAGGCTAGCTAAC"))
    too = SC.too_degenerate_oligo(oracle)
    holed = W.word_from_slots([1 if k in (5, 6, 7, 9, 10, 11) else 0 for k in range(32)])
    nan = float("nan")

    def refused(fragment, *a, **kw):
        rc, msg = _call(lib, *a, **kw)
        assert rc == PCR_ERR_ARG and fragment in msg, (fragment, rc, msg)
        return msg

    refused("null handle", api.TARGET, [pair])                               # every argument is fine: only the handle is missing
    refused("null handle", api.TARGET, [pair], probes=[None])                # ... also without a probe
    # 1. the set, before the pointers
    refused("unknown sequence set", 7, [pair], ids=False)
    refused("PCR_SET_MULTIPLEX", api.MULTIPLEX, [pair], ids=False)
    # 2. the pointers, before the pool's size
    for kw in (dict(ids=False), dict(pids=False), dict(args=False), dict(has_pool=False), dict(probes=None), dict(cap=4)):
        refused("bad argument", api.TARGET, [pair], **kw)
    refused("bad argument", api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), cap=4)
    # 3. the pool's size, before the concentrations
    refused("PCR_POOL_MAX_PAIRS", api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), template_strand=-1e-9)
    # 4. the concentrations, before the salt
    refused("negative", api.TARGET, [pair], template_strand=-1e-9, salt=2.0)
    refused("negative", api.TARGET, [pair], primer_strand=-9e-7, salt=2.0)
    refused("negative", api.TARGET, [pair], probe_strand=-2.5e-7, salt=2.0)
    # 5. the salt, before the oligos
    refused("salt", api.TARGET, [pair, (pair[0], too)], salt=2.0)
    refused("salt", api.TARGET, [pair], salt=1e-7)
    # 6. the primers, before the probes
    refused("empty", api.TARGET, [(pair[0], (0, 0))], probes=[holed])
    assert "a primer" in refused("hole", api.TARGET, [(pair[0], holed)], probes=[too])
    assert "a primer" in refused("PCR_SITE_MAX_EXPANSIONS", api.TARGET, [pair, (pair[0], too)], probes=[holed, holed])
    assert "a primer" in refused("zero", api.TARGET, [pair], primer_strand=0.0, probes=[holed])
    refused("null handle", api.TARGET, [pair], primer_strand=0.0, template_strand=1e-7)       # the template alone is a concentration
    refused("null handle", api.TARGET, [(pair[0], w("ACGTNNNNACGTACGTACG"))])                # 256 expansions pass
    # 7. the probes, before the number of oligos
    many = [(w(rand_seq(rng, 20)), w(rand_seq(rng, 20))) for rng in [random.Random(6201)] for _ in range(api.POOL_MAX_PAIRS)]
    assert len({x for p in many for x in p}) == 2 * api.POOL_MAX_PAIRS
    assert "a probe" in refused("hole", api.TARGET, many, probes=[holed] + [None] * (len(many) - 1))
    assert "a probe" in refused("PCR_SITE_MAX_EXPANSIONS", api.TARGET, [pair], probes=[too], tm_floor=nan)
    assert oracle.word_degeneracy(too) == 512
    assert "a probe" in refused("zero", api.TARGET, [pair], probe_strand=0.0, tm_floor=nan)
    refused("null handle", api.TARGET, [pair], probe_strand=0.0, template_strand=1e-7)
    refused("null handle", api.TARGET, [pair], probe_strand=0.0, probes=[None])               # no probe: its concentration is not used
    # 8. the number of distinct oligos, before the floors
    refused("too many distinct oligos", api.TARGET, many, probes=[PROBE] + [None] * (len(many) - 1), tm_floor=nan)
    refused("null handle", api.TARGET, many, probes=[None] * len(many))                       # 2 048 primers alone pass
    refused("too many distinct oligos", api.TARGET, many, probes=[many[3][1]] + [None] * (len(many) - 1))   # a probe equal to a primer is one more oligo
    # 9. / 10. the floors, tm_floor first
    for bad in (nan, float("inf"), float("-inf")):
        refused("pcr_pool_probe_hits: tm_floor", api.TARGET, [pair], tm_floor=bad, probe_tm_floor=nan)
        refused("probe_tm_floor", api.TARGET, [pair], probe_tm_floor=bad)
    refused("null handle", api.TARGET, [pair], tm_floor=55.0, probe_tm_floor=60.0)
    # 11. the handle: n_pool = 0 still needs one
    refused("null handle", api.TARGET, [])


# ------------------------------------------------------------------ what the GPU tests rely on, computed with the oracle
def _bit(rows, i, s):
    return (int(rows[i, s >> 6]) >> (s & 63)) & 1


@pytest.mark.parametrize("name", H.SCENARIO_NAMES)
def test_every_scenario_has_hits_misses_and_floors_that_cut(oracle, name):
    ids, pid, prod, psites, hits = H.everything(oracle, name)
    assert len(hits) >= 1 and len(psites) >= 1
    with_hit = {tuple(r) for r in hits[list(PC.FIELDS8[:5])].tolist()}
    assert any(tuple(r) not in with_hit for r in prod[list(PC.FIELDS8[:5])].tolist()), "every product has a hit"
    key = [tuple(r) for r in hits[list(H.ORDER)].tolist()]
    assert key == sorted(set(key))
    _, _, _, detected = H.expectation(oracle, name)
    assert detected.any() and (detected != H.products_bits(oracle, name)).any()
    pairs = H.floor_pairs(oracle, name)
    counts = [len(H.kept(hits, a, b)) for a, b in pairs]
    assert counts[0] == len(hits) and 0 in counts and len(set(counts)) >= min(3, len(hits) + 1), counts
    moved_by = lambda k: {c for (a, b), c in zip(pairs, counts) if (a, b)[1 - k] == 0.0 and (a, b)[k] > 0}
    assert len(moved_by(0)) >= 2 and len(moved_by(1)) >= 2                   # either floor alone moves the count
    rows = {H.expectation(oracle, name, a, b)[3].tobytes() for a, b in pairs}
    assert len(rows) >= 2                                                    # ... and the rows


@pytest.mark.parametrize("name", ["edges", "words_db"])
def test_edges_fall_on_the_stated_side(oracle, name):
    case = H.scenario(oracle, name)
    ids, pid, prod, psites, hits = H.everything(oracle, name)
    assert ids == [0, 1] and pid == [0]
    E = H.EDGES
    at = lambda what: psites[psites["sequence"] == E[what]]
    inside = set(hits["sequence"].tolist())
    assert inside == {E["plus"], E["minus"], E["in_plus_side"], E["in_minus_side"]}
    assert set(prod["sequence"].tolist()) == set(range(len(E))) - {E["no_product"], E["inactive"]}
    assert (prod["inner_start"] + 3 == H.EDGE_P3).all() and (prod["inner_start"] + prod["inner_length"] - 8 == H.EDGE_M5).all()
    assert at("plus")["strand"].tolist() == [1] and at("minus")["strand"].tolist() == [2]
    assert at("minus")["loc5"].tolist() == at("plus")["loc5"].tolist() and (at("minus")["loc5"] <= at("minus")["loc3"]).all()
    assert at("in_plus_side")["loc5"].tolist() == [H.EDGE_P3 + 1] and at("out_plus_side")["loc5"].tolist() == [H.EDGE_P3]
    assert at("in_minus_side")["loc3"].tolist() == [H.EDGE_M5 - 1] and at("out_minus_side")["loc3"].tolist() == [H.EDGE_M5]
    assert at("upstream")["loc3"][0] < prod[0]["begin"]
    assert len(at("no_probe")) == 0 and len(at("no_product")) == 1 and len(at("inactive")) == 0
    assert not case["active"][E["inactive"]] and all(case["active"][i] for i in range(len(E)) if i != E["inactive"])
    assert (hits["intended"] == 3).all() and not hits["flags"].any()
    _, _, _, detected = H.expectation(oracle, name)
    assert [s for s in range(len(E)) if _bit(detected, 0, s)] == sorted(inside)


def test_ladder(oracle):
    ids, pid, prod, psites, hits = H.everything(oracle, "ladder")
    assert len(prod) == 2 and hits["probe_loc5"].tolist() == list(H.LADDER_PROBE_AT) and (hits["sequence"] == 0).all()
    assert hits["probe_strand"].tolist() == [1, 2, 1, 2, 1]
    assert len(np.unique(hits["tm_probe"])) == 5 and hits["tm_probe"].min() > 0
    floors = H.probe_floors_of(hits)
    counts = [len(H.kept(hits, 0.0, f)) for f in floors]
    assert counts[0] == 5 and counts[-3] == 5 and counts[-2] == 0 and counts[-1] == 5
    assert all(counts[2 * i] == counts[2 * i + 1] + 1 for i in range(3))     # nextafter above a value drops exactly it
    assert H.expectation(oracle, "ladder", 0.0, floors[-2])[3].tolist() == [[0]]
    assert H.expectation(oracle, "ladder", 0.0, floors[4])[3].tolist() == [[1]]


def test_cross(oracle):
    X = H.CROSS
    ids, pid, prod, psites, hits = H.everything(oracle, "cross")
    assert ids[:2] == ids[6:8] == ids[8:10] and ids[12] == ids[13]            # A three times; F = R
    assert pid == [0, 1, H.NO_PROBE, 1, 0, 0, 2, 3]
    a, b = (ids[0], ids[1]), (ids[2], ids[3])
    of = lambda pair, probe: hits[(hits["plus_oligo"] == pair[0]) & (hits["minus_oligo"] == pair[1]) & (hits["probe"] == probe)]
    foreign = of(b, pid[X["A"]])                                             # A's probe inside B's product
    assert len(foreign) == 1 and foreign[0]["intended"] == H.PRODUCT_INTENDED and foreign[0]["sequence"] == 1
    assert len(of(b, pid[X["B"]])) == 1 and of(b, pid[X["B"]])[0]["intended"] == 3
    _, _, _, d = H.expectation(oracle, "cross")
    assert d[X["B"]].tolist() == [1 << 1]                                    # row B: its own probe's hit alone
    assert d[X["A"]].tolist() == d[X["A_again"]].tolist() == [1 << 0]        # the duplicated triple
    assert d[X["A_other_probe"]].tolist() == [1 << 2]                        # the same pair with B's probe: another row
    assert d[X["E_shares_Pa"]].tolist() == [1 << 3] and of((ids[10], ids[11]), 0)[0]["probe_strand"] == 2
    assert d[X["G_equal"]].tolist() == [1 << 3] and len(of((ids[12], ids[12]), pid[X["G_equal"]])) == 1
    assert d[X["C"]].tolist() == H.products_bits(oracle, "cross")[X["C"]].tolist() == [1 << 2]   # no probe: the product's bit
    # the probe that is a primer word: a table entry of its own, sites wherever Fa binds, its hit inside D's product
    fa_probe = pid[X["D_primer_probe"]]
    assert set(psites[psites["oligo"] == fa_probe]["sequence"].tolist()) == {0, 2, 4, 6}
    assert d[X["D_primer_probe"]].tolist() == [1 << 4]
    assert H.products_bits(oracle, "cross")[X["A"]].tolist() == [0b1000101]  # products_tm sees A on 0, 2 and 6
    assert not (prod["intended"] == 1).all()                                 # (Fa, Rd) on sequence 4: a cross product


def test_words(oracle):
    case = H.scenario(oracle, "words")
    ids, pid, prod, psites, hits = H.everything(oracle, "words")
    assert len(case["seqs"]) == PC.WORDS_N and pid == [0, 1, 2]
    block = hits[hits["sequence"] == PC.WORDS_BLOCK]
    assert len(block) == 64 * 3 and len(hits) > 256 and set(block["probe"].tolist()) == {0}
    _, _, _, d = H.expectation(oracle, "words")
    bits = H.products_bits(oracle, "words")
    for s in (63, 64, 127, 128, PC.WORDS_BLOCK):
        assert _bit(d, s % 3 if s != PC.WORDS_BLOCK else 0, s)
    for s in H.WORDS_NO_PROBE_SITE:
        if s not in PC.WORDS_INACTIVE + PC.WORDS_NO_SITE:
            assert _bit(bits, s % 3, s) and not _bit(d, s % 3, s)
    for s in PC.WORDS_INACTIVE + PC.WORDS_NO_SITE:
        assert not any(_bit(d, i, s) for i in range(3))
    assert all((d[:, w] != 0).any() for w in range(3)) and set(hits["probe_strand"].tolist()) == {1, 2}


def test_degenerate_ambiguity_split(oracle):
    ids, pid, prod, psites, hits = H.everything(oracle, "degenerate")
    assert psites["n_expansions"].tolist() == [4] and psites[0]["tm_max"] > psites[0]["tm_min"] > 0
    assert hits["tm_probe"].view(np.uint32).tolist() == psites["tm_max"].view(np.uint32).tolist()
    ids, pid, prod, psites, hits = H.everything(oracle, "ambiguity")
    assert hits["flags"].tolist() == [H.PROBE_NO_TM, 0, H.PROBE_NO_TM] and hits["tm_probe"].view(np.uint32).tolist()[0] == 0
    assert H.expectation(oracle, "ambiguity", 0.0, 1e-3)[3].tolist() == [[0b001]]   # any probe floor drops the unmelted site
    assert H.expectation(oracle, "ambiguity")[3].tolist() == [[0b011]]
    ids, pid, prod, psites, hits = H.everything(oracle, "split")
    assert set(prod["sequence"].tolist()) == {1, 2} and hits["sequence"].tolist() == [1]
    assert H.SPLIT_PROBE_AT in psites[psites["sequence"] == 0]["loc5"].tolist()     # the site is there: the product is not
    assert len(psites[psites["sequence"] == 2]) >= 1                                 # weak sites outside the product


def test_offset_probe_sites_share_the_primers_entries(oracle):
    """Words that are not centred: the probe's site is read from the very DB entry of the plus primer (sequence 0) or of the
    minus primer (sequence 1) -- an implementation that looks only at entries strictly between the two would find no hit."""
    case = H.scenario(oracle, "offset")
    ids, pid, prod, psites, hits = H.everything(oracle, "offset")
    starts = [oracle.word_start(w) for w in (case["panel"][0][0], case["panel"][0][1], case["probes"][0])]
    stops = [oracle.word_stop(w) for w in (case["panel"][0][0], case["panel"][0][1], case["probes"][0])]
    assert starts == [0, 0, 18] and stops == [17, 17, 31]
    locs = {(e[3], e[4]): e[2] for e in H.db_of(oracle, case)}               # (sequence, strand) -> the one entry's loc
    assert len(locs) == len(H.db_of(oracle, case)) == 6
    assert hits["sequence"].tolist() == [0, 1] and hits["probe_strand"].tolist() == [1, 2]
    assert hits[0]["probe_loc5"] - starts[2] == locs[(0, 1)] == hits[0]["begin"] - starts[0]        # the plus primer's entry
    assert hits[1]["probe_loc3"] + starts[2] == locs[(1, 2)] == hits[1]["end"] + starts[1]          # the minus primer's entry
    assert hits[0]["probe_loc5"] == hits[0]["inner_start"] + 3 + 1                                   # p3 + 1
    assert hits[1]["probe_loc3"] == hits[1]["inner_start"] + hits[1]["inner_length"] - 8 - 1         # m5 - 1


@pytest.mark.parametrize("name", H.SCENARIO_NAMES)
def test_numpy_join_is_the_definition(oracle, name):
    """host_join of profiles/bench_probe_hits.py -- the second cross-check of the GPU tests and the composition the bench script
    times -- on the oracle's products and probe sites gives the expectation, at every floor pair."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_probe_hits.py")
    spec = importlib.util.spec_from_file_location("bench_probe_hits", path)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    ids, pid, prod, psites, _ = H.everything(oracle, name)
    n_seq = len(H.scenario(oracle, name)["seqs"])
    for tm_floor, probe_tm_floor in H.floor_pairs(oracle, name):
        k = PC.kept(prod, tm_floor)
        fr, rf = PC.bits_of(k, ids, n_seq)
        got, rows = bench.host_join(H.HIT, k, fr, rf, psites, ids, pid, probe_tm_floor)
        _, _, want, want_rows = H.expectation(oracle, name, tm_floor, probe_tm_floor)
        assert H.as_bits(got) == H.as_bits(want) and rows.tolist() == want_rows.tolist()


@pytest.mark.parametrize("name", H.SCENARIO_NAMES)
def test_scenario_duplexes_oracle_equals_reference(oracle, probe_reference, name):
    """Every duplex the scenarios melt: reference.heterodimer_full == oracle.heterodimer_full, bit for bit."""
    jobs = H.jobs_of(oracle, name)
    assert jobs, name
    for q, t, ca, cb in sorted(jobs):
        want = probe_reference.heterodimer_full(q, t, SC.SALT, ca, cb)
        got = oracle.heterodimer_full(q, t, SC.SALT, ca, cb)
        assert want.view(np.uint32).tolist() == got.view(np.uint32).tolist(), (q, t, ca, cb)
