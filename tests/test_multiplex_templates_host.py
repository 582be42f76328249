"""The scenarios of tests/multiplex_templates.py against the compiled reference: find_multiplex_background_match of the
reference (behind the `reference` fixture: live where oracle/Makefile built it, else its recorded answers) gives the
bits the oracle gave when the scenario was built -- at every threshold and both TaqMAMA settings, for templates of 1 to
32 766 bases and sets of 1 to 70 001 sequences.  The expected values of tests/test_gpu_multiplex_match.py are these
oracle bits, so they do not come from the code under test.

32 766 is the longest template the reference can take: SeqOverlap's column loops count in SO_Score, a 16-bit integer
(`for(SO_Score j = 0;j <= max_target_len;j++)`, seq_overlap.cpp:383,427), and with max_target_len = 32 767 the condition
can never fail.  The compiled reference given one 32 767-base sequence and a short one did not return within 60 s (a
32 766-base one takes it 0.02 s).  No test here may hand it such a template; pcr_multiplex_match refuses them.

Building all scenarios takes the oracle about a minute on one core (the five ladders 4 to 7 s each, the 70 001-sequence
set 12 s, the four oracle rows of the 300-pair batch 13 s)."""
import numpy as np
import pytest

import multiplex_templates as MT

SMALL = [n for n in MT.NAMES if n not in ("big", "batches")]


def ref_session(reference, sc):
    sr = reference.session()
    for s, w in zip(sc.seqs, sc.weights):
        sr.add_target(s, w)
    return sr


@pytest.mark.parametrize("name", SMALL + ["batches"])
def test_reference_gives_the_oracle_bits(oracle, reference, name):
    sc = MT.scenario(oracle, name)
    sr = ref_session(reference, sc)
    n_set = 0
    for p in sc.cpu_pairs:
        for thr in sc.thresholds:
            for taq in sc.taq:
                got = sr.multiplex_match(sc.pairs[p], thr, taq).astype(bool)
                want = sc.want[(p, thr, taq)]
                assert np.array_equal(got, want), (name, p, thr, taq, np.nonzero(got != want)[0][:10])
                n_set += int(want.sum())
    assert n_set > 0


@pytest.mark.parametrize("n", MT.SMALL_SIZES)
def test_reference_small_sets(oracle, reference, n):
    """Sets of 1 .. 129 sequences (an odd count leaves the reference's last call with one sequence)."""
    sc = MT.prefix(MT.scenario(oracle, "sizes"), n)
    sr = ref_session(reference, sc)
    for p in sc.cpu_pairs:
        for thr in sc.thresholds:
            for taq in sc.taq:
                assert np.array_equal(sr.multiplex_match(sc.pairs[p], thr, taq).astype(bool), sc.want[(p, thr, taq)]), (n, p, thr, taq)


@pytest.mark.parametrize("n", MT.BIG_SIZES)
def test_reference_big_sets(oracle, reference, n):
    """65 535, 65 536 and 70 001 sequences go to the reference once each, at the threshold where a quarter of the bits is set."""
    sc = MT.prefix(MT.scenario(oracle, "big"), n)
    sr = ref_session(reference, sc)
    got = sr.multiplex_match(sc.pairs[0], 0.6, 0).astype(bool)
    want = sc.want[(0, 0.6, 0)]
    assert got.shape == (n,) and np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert want[n - 1] and want[0]                                            # the last index of every size is a marked hit


def test_prefix_is_what_the_oracle_says(oracle):
    """prefix() cuts the full set's bits: the oracle run on the shorter set itself gives the same."""
    for name, n in (("big", 65535), ("sizes", 63), ("ladder 12", 101)):
        sc = MT.prefix(MT.scenario(oracle, name), n)
        so = oracle.session()
        for s, w in zip(sc.seqs, sc.weights):
            so.add_target(s, w)
        thr, taq = sc.thresholds[0], 1
        assert np.array_equal(so.multiplex_match(sc.pairs[0], thr, taq).astype(bool), sc.want[(0, thr, taq)]), name


def test_scenarios_cover_what_they_claim(oracle):
    scs = [MT.scenario(oracle, n) for n in MT.NAMES]
    whats = {l.what for sc in scs for l in set(sc.labels)}
    for w in ("unplanted", "begin at column 0", "end at the last column", "interior edge", "last edge", "end at column 0",
              "end at column 1", "same row tie", "row tie", "lane tie", "suffix 0", "suffix 7", "IUPAC holding the base",
              "IUPAC without the base", "IUPAC at the 3' end", "EOS inside the site", "only N", "only EOS", "hit at a word edge",
              "hit at a marked index"):
        assert w in whats, w
    ladders = [sc for sc in scs if sc.name.startswith("ladder")]
    assert sorted(len(sc.pairs_txt[0][0]) for sc in ladders) == list(MT.PRIMER_LENGTHS)
    assert {len(sc.seqs) % 2 for sc in ladders} == {0, 1}                       # an odd and an even sequence count
    # the long templates carry every lane and every kind of copy between them
    long = [l for sc in ladders for s, l in zip(sc.seqs, sc.labels) if len(s) >= 16384 and l.lane is not None]
    assert {l.lane for l in long} == {0, 1, 2, 3} and {l.kind for l in long} == set(MT.KINDS)
    assert {l.what for l in long} >= {"begin at column 0", "end at the last column", "interior edge", "last edge"}
    big = MT.scenario(oracle, "big")
    marked = [i for i, l in enumerate(big.labels) if l.what == "hit at a marked index"]
    assert set(marked) >= {0, 63, 64, 65534, 65535, 65536, 70000} and len(big.seqs) == 70001
    assert len(MT.scenario(oracle, "batches").pairs) == 300
