"""The scenarios of tests/background_lists.py held to what they promise, from the oracle alone (no GPU): the bucket band of every
case, the planted candidate counts, bits both set and clear, the two index modes told apart, and the record totals of the
overflow cases on either side of the capacities they are aimed at."""
import numpy as np
import pytest

import background_lists as BL


@pytest.fixture(scope="module")
def cases(oracle):
    return BL.cases(oracle)


NAMES = (["class64", "class128", "class256", "ballast128", "ballast256", "limit", "wide128", "wide129", "wide200"]
         + ["spill_%d_%d" % (nr, p) for nr in BL.SPILL_NR for p in range(1, 6)] + ["spill_24_128", "natural"]
         + ["hook16", "hook256", "hook_n-1", "hook_n", "hook_16n-1", "hook_16n", "hist8192", "hist8193"])


def test_every_case_is_listed(cases):
    assert sorted(cases) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_case(oracle, cases, name):
    c = cases[name]
    a = BL.oracle_answers(oracle, c)
    lo, hi = BL.band(c.slots)
    assert lo <= BL.largest_bucket(a.entries) <= hi, (name, BL.largest_bucket(a.entries), c.slots)
    assert {e[3] for e in a.entries} == set(c.racks.values()) and len(c.racks) <= 4     # four sequences with entries at most: one workgroup, one sub-list
    # the planted candidates, and nothing else
    for k, want in enumerate(c.per_pair):
        if want is not None:
            assert a.counts[k] == want, (name, k)
    nf, nr = c.n_f, c.n_r
    assert c.per_pair[0] == nf * nr + BL.MF * BL.MR + (nf - 1) * nr       # rack, mutated rack, the cut copy without its first F site
    assert all(w == 2 * nf * nr + BL.MF * BL.MR for w in c.per_pair[1:c.n_distinct])
    assert a.records == BL.expected_records(c, a.counts[c.n_distinct:])
    assert len(c.batch) == len(c.origin) and all(c.batch[i] == c.unique[o] for i, o in enumerate(c.origin))
    # bits set and clear, in every mode; nothing on the inactive copy, which holds every site of the rack
    for key, rows in a.bits.items():
        assert rows.any() and not rows.all(), (name, key)
        assert rows[:, c.racks["rack"]].all() or len(c.unique) > c.n_distinct, (name, key)
        assert not rows[:, list(c.inactive)].any(), (name, key)
    # the form the library must choose
    wide = (2 * len(c.batch) + 31) // 32 > 8
    assert c.form == ("emit<0>" if wide or c.slots > 128 else "emit<%d>" % c.slots)


def test_index_modes_differ(oracle, cases):
    """The mutated rack's one good candidate has an odd index past the sequence count: the reference's rule drops it."""
    n = 0
    for name in ("class64", "class128", "class256", "natural", "spill_13_1"):
        c = cases[name]
        a = BL.oracle_answers(oracle, c)
        for k in range(c.n_distinct):
            if a.bits[(True, 0)][k, c.racks["mutated"]] and not a.bits[(False, 0)][k, c.racks["mutated"]]:
                n += 1
        assert a.counts[0] > len(c.seqs)                                   # more candidates than sequences: the ordered path
    assert n >= 5


def test_classes_and_widths(cases):
    assert [cases["class%d" % s].form for s in (64, 128, 256)] == ["emit<64>", "emit<128>", "emit<0>"]
    assert [cases["class%d" % s].slots for s in (64, 128, 256)] == [64, 128, 256]
    assert cases["wide128"].form == "emit<64>" and cases["wide129"].form == cases["wide200"].form == "emit<0>"
    assert cases["wide129"].slots == cases["wide200"].slots == 64
    for s in (128, 256):                                                   # the same sequences and batch as class64, larger buckets
        c = cases["ballast%d" % s]
        assert c.slots == s and c.seqs[:-1] == cases["class64"].seqs and c.batch == cases["class64"].batch
    assert cases["ballast128"].form == "emit<128>" and cases["ballast256"].form == "emit<0>"
    assert cases["wide200"].batch[:128] == cases["wide128"].batch and cases["wide129"].seqs == cases["wide128"].seqs


def test_spill_sweep(cases):
    """Records per F site and chunk of partners: P * nR, on both sides of the wave list's flush (64) and capacity (128)."""
    per_site = {len(cases[n].batch) * cases[n].n_r for n in cases if n.startswith("spill_")}
    assert {63, 64, 65, 126, 128, 129, 24 * 128} <= per_site
    assert any(64 < x < 128 for x in per_site) and any(128 < x < 256 for x in per_site) and any(x >= 256 for x in per_site)
    assert all(cases[n].form == "emit<128>" for n in cases if n.startswith("spill_"))


def test_overflow_totals(oracle, cases):
    c = cases["natural"]
    n = BL.oracle_answers(oracle, c).records
    assert c.hook is None and n > BL.DEFAULT_CAP // BL.SUB_LISTS == 65536 and n <= BL.DEFAULT_CAP     # a sub-list overflows, the sum fits
    assert len(BL.attempts(BL.DEFAULT_CAP, n)) == 2
    assert 4 * n <= 4e5                                                    # Smith-Waterman lanes of one pass
    n = BL.oracle_answers(oracle, cases["class64"]).records
    hooks = {"hook16": 16, "hook256": 256, "hook_n-1": n - 1, "hook_n": n, "hook_16n-1": 16 * n - 1, "hook_16n": 16 * n}
    for name, hook in hooks.items():
        c = cases[name]
        assert c.hook == hook and BL.oracle_answers(oracle, c).records == n and c.form == "emit<64>"
        caps = BL.attempts(hook, n)
        assert len(caps) < 6 and caps[-1] // BL.SUB_LISTS >= n
    assert 256 // 16 < n < 256                                             # a sub-list overflows while the sum fits
    assert len(BL.attempts(n - 1, n)) > 1 and len(BL.attempts(n, n)) > 1   # the sum overflows by one; fits exactly, the sub-list does not
    assert len(BL.attempts(16, n)) >= 4                                    # several doublings in one call
    assert len(BL.attempts(16 * n - 1, n)) == 2 and len(BL.attempts(16 * n, n)) == 1   # the exact-fit edge of the sub-list


def test_histogram_cases(oracle, cases):
    for p, name in ((8192, "hist8192"), (8193, "hist8193"), (BL.LIMIT_PAIRS, "limit")):
        c = cases[name]
        a = BL.oracle_answers(oracle, c)
        assert len(c.batch) == p and len(c.unique) > c.n_distinct
        assert sum(1 for k in range(c.n_distinct, len(c.unique)) if a.counts[k] == 0) > 7000     # pairs that match nothing
        assert a.records < 65536                                           # one pass
