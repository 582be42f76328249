"""The dense scenarios of tests/dense_buckets.py are what they claim, for every size class: the oracle's word DB,
orientation bits, coverage and collect_amplicons equal the labels computed from the planted geometry; the dense
sequence's bucket lies in the class's entry band, with labelled amplicons at both of its ends and across the
low-complexity stretch; the decoy pair has amplicons inside and one base outside the window; the near-copies are
not in the DB.  The expected values of tests/test_gpu_dense_buckets.py therefore do not come from the code under test.

The largest class (a dense sequence of 572 000 bases, 23 500 entries) takes the oracle 0.35 s to select and 0.1 s to match
its eight pairs on one CPU core; building the scenario and its labels takes about 1 s of Python, this whole file 30 s."""
import numpy as np
import pytest

import amplicon_edges as AE
import dense_buckets as DB

CASES = [(c, False) for c in ("4k", "8k", "32k", "64k")] + [("8k", True), ("32k", True), ("64k", True)]


def session(oracle, sc):
    """Splits before the selection, as on the device (its split() drops the word DB); the dense scenarios' splits lie far
    from every primer's word, so the labels hold in this order too."""
    so = oracle.session(**sc.opts)
    for s, w in zip(sc.seqs, sc.weights):
        so.add_target(s, w)
    for i in sc.inactive:
        so.set_active(i, False)
    for i, pos in sc.splits:
        so.split(i, pos)
    so.select(sc.pairs)
    return so


@pytest.fixture(scope="module", params=CASES, ids=lambda c: c[0] + ("-two" if c[1] else ""))
def case(request, oracle):
    d = DB.build(oracle, *request.param)
    return d, session(oracle, d.sc)


def _site_entries(lib, sc, i):
    """(loc, strand) of the DB entry of every planted site of sequence i."""
    return {(s.loc, 1 if s.role == "P" else 2) for s in sc.sites[i]}


def test_db_is_the_planted_sites(oracle, case):
    d, so = case
    sc = d.sc
    ent = so.db_entries()
    lo, hi = DB.CLASSES[d.cls].entries
    assert lo <= AE.largest_bucket(ent) <= hi
    n_sites = DB.CLASSES[d.cls].n_sites
    for i in d.dense:
        b = DB.bucket(ent, i)
        assert lo <= len(b) <= hi
        # exactly the planted sites: no near-copy (it ties below the maximum of its scan), no chance match
        assert {(e[2], e[4]) for e in b} == _site_entries(oracle, sc, i) and len(b) == len(sc.sites[i])
        assert sum(1 for s in sc.sites[i] if s.oligo == (d.k["d"], "F") and s.role == "P") == n_sites + 5
        assert d.n_near >= n_sites // 8 - 2
        # labelled entries at both ends of the bucket, and the low-complexity entries between the two sites of pair 1
        first, last = sc.sites[i][0], [s for s in sc.sites[i] if s.oligo[0] == 2]
        assert first.oligo == (0, "F") and (b[0][2], b[1][2]) == (first.loc, sc.sites[i][1].loc)
        assert sorted(e[2] for e in b[-2:]) == sorted(s.loc for s in last) and len(last) == 2
        assert len(b) - 2 >= lo
        p1 = [s for s in sc.sites[i] if s.oligo[0] == 1]
        between = [e for e in b if p1[0].loc < e[2] < p1[1].loc]
        assert len(p1) == 2 and len(between) >= 2 * (DB.CLASSES[d.cls].lc_len - 19 - 32) > 1024
    # the ordinary sequences: few entries or none, one inactive without any
    per = [len(DB.bucket(ent, i)) for i in range(len(sc.seqs))]
    assert all(per[i] <= 8 for i in range(len(sc.seqs)) if i not in d.dense)
    assert sum(1 for n in per if n == 0) >= 3 and all(per[i] == 0 for i in sc.inactive) and sc.inactive


def test_oracle_answers_equal_the_labels(oracle, case):
    d, so = case
    for sc in (d.sc, DB.wide(d.sc)):
        so.set_options(amp_min=sc.opts["amp_min"], amp_max=sc.opts["amp_max"])
        fr, rf = AE.expected(sc)
        for p, pair in enumerate(sc.pairs):
            _, ori = so.target_match(pair, orient=True)
            assert np.array_equal((ori & 1) != 0, fr[p]) and np.array_equal((ori & 2) != 0, rf[p]), (sc.name, p)
            for l in sc.labels:
                if l.pair == p:
                    assert bool(ori[l.seq] & (1 if l.orient == "FR" else 2)) == l.admitted, (sc.name, l)
            want = np.float32(sum(np.float32(w) for i, w in enumerate(sc.weights) if fr[p, i] or rf[p, i]))
            assert abs(so.target_coverage(pair) - want) <= 1e-4 * max(1.0, want)
            if p != d.k["lc"]:                          # (the low-complexity pair forms ~10^5 amplicons: bits only)
                bounds, _ = so.collect_amplicons(pair, sc.opts["target_threshold"], sc.opts["amp_min"], sc.opts["amp_max"])
                assert sorted(set(bounds)) == AE.expected_bounds(sc, p), (sc.name, p)
    so.set_options(**DB.NARROW)


def test_the_edges_are_there(oracle, case):
    d, _ = case
    narrow, wide = d.sc, DB.wide(d.sc)
    k = d.k
    for i in d.dense:
        at = lambda sc, pair, orient: [l for l in sc.labels if l.seq == i and l.pair == pair and l.orient == orient]
        for sc in (narrow, wide):
            assert at(sc, 0, "FR")[0].admitted and at(sc, 2, "RF")[0].admitted          # both ends of the bucket
            assert not any(l.admitted for l in sc.labels if l.seq == i and l.pair == k["cut"])      # EOS and split
        assert not at(narrow, 1, "FR")[0].admitted and at(wide, 1, "FR")[0].admitted   # across the low-complexity stretch
        assert not any(l.admitted for l in narrow.labels if l.seq == i and l.pair == k["out"])      # one base outside only
        # the decoy pair: amplicons inside the window and one base outside it, both orientations
        got = {(e - b + 1) for s, b, e in AE.expected_bounds(narrow, k["d"]) if s == i}
        assert got == {80, 140, 200}
        lens = {l.amp_len for l in narrow.labels if l.seq == i and l.pair == k["d"]}
        assert {79, 80, 200, 201} <= lens
        fr, rf = AE.expected(narrow)
        assert fr[k["d"], i] and rf[k["d"], i] and fr[k["lc"], i] and not rf[k["lc"], i]
    # a sequence whose best d1 site is a near-copy holds it in the DB and is refused by the identity test
    near = [l for l in narrow.labels if l.what == "near-copy is the best site"]
    assert len(near) == 1 and not near[0].admitted
    assert any(l.admitted for l in narrow.labels if l.what == "decoy pair in an ordinary sequence")
    assert not any(l.admitted for l in narrow.labels if l.what == "inactive")


@pytest.mark.parametrize("cls", ["s4k", "s8k"])
def test_shift_classes(oracle, cls):
    """The classes that are selected with optimize_5 = optimize_3 = 1 (several words per site): the dense bucket lies in
    the class's band, and the answers are the labels' all the same."""
    d = DB.build(oracle, cls)
    sc = d.sc._replace(opts=dict(d.sc.opts, optimize_5=1, optimize_3=1))
    so = session(oracle, sc)
    ent = so.db_entries()
    lo, hi = DB.CLASSES[cls].entries
    assert lo <= AE.largest_bucket(ent) <= hi and all(lo <= len(DB.bucket(ent, i)) for i in d.dense)
    fr, rf = AE.expected(sc)
    for p, pair in enumerate(sc.pairs):
        _, ori = so.target_match(pair, orient=True)
        assert np.array_equal((ori & 1) != 0, fr[p]) and np.array_equal((ori & 2) != 0, rf[p]), (sc.name, p)
