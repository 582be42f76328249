"""The planted amplicon edges of tests/amplicon_edges.py answer as labelled: the oracle's target_match (per orientation),
coverage and collect_amplicons equal what the reference's rule gives on the planted geometry.  A case that drifts off
its edge (a spurious background match, a site that no longer matches) fails here, not silently in the GPU tests."""
import numpy as np
import pytest

import amplicon_edges as AE


@pytest.fixture(scope="module")
def cases(oracle):
    return AE.scenarios(oracle)


def session(oracle, sc, splits_first=False):
    so = oracle.session(**sc.opts)
    for s, w in zip(sc.seqs, sc.weights):
        so.add_target(s, w)
    for i in sc.inactive:
        so.set_active(i, False)
    if splits_first:
        for i, pos in sc.splits:
            so.split(i, pos)
    so.select(sc.pairs)
    if not splits_first:
        for i, pos in sc.splits:                      # after the selection: the words stay, has_split sees the EOS
            so.split(i, pos)
    return so


def test_cases_cover_the_edges(cases):
    labels = [l for sc in cases for l in sc.labels]
    assert len(labels) > 300
    for orient in ("FR", "RF"):
        mine = [l for l in labels if l.orient == orient]
        assert any(l.admitted for l in mine) and any(not l.admitted for l in mine)
    whats = " ".join(l.what for l in labels)
    for w in ("length", "overlap", "5' hang", "3' hang", "EOS (text)", "EOS (split)", "inactive", "same position",
              "identity at", "identity above", "identity below", "decoy"):
        assert w in whats, w
    # every length edge of every window is there, admitted inside the window and refused outside it
    for sc in cases:
        o = sc.opts
        for l in sc.labels:
            if l.what.startswith("length"):
                assert l.admitted == (o["amp_min"] <= l.amp_len <= o["amp_max"]), (sc.name, l)


@pytest.mark.parametrize("k", range(AE.N_SCENARIOS))
def test_oracle_answers_equal_the_labels(oracle, cases, k):
    assert len(cases) == AE.N_SCENARIOS
    sc = cases[k]
    so = session(oracle, sc)
    fr, rf = AE.expected(sc)
    for p, pair in enumerate(sc.pairs):
        bits, ori = so.target_match(pair, orient=True)
        got_fr, got_rf = (ori & 1) != 0, (ori & 2) != 0
        for l in sc.labels:
            if l.pair == p:
                got = (got_fr if l.orient == "FR" else got_rf)[l.seq]
                assert got == l.admitted, (sc.name, l)
        assert np.array_equal(got_fr, fr[p]), (sc.name, p, np.nonzero(got_fr != fr[p]))
        assert np.array_equal(got_rf, rf[p]), (sc.name, p, np.nonzero(got_rf != rf[p]))
        want_cov = np.float32(sum(np.float32(w) for i, w in enumerate(sc.weights) if fr[p, i] or rf[p, i]))
        assert abs(so.target_coverage(pair) - want_cov) <= 1e-4 * max(1.0, want_cov)
        bounds, _ = so.collect_amplicons(pair, sc.opts["target_threshold"], sc.opts["amp_min"], sc.opts["amp_max"])
        assert sorted(set(bounds)) == AE.expected_bounds(sc, p), (sc.name, p)


def test_split_first_answers(oracle, cases):
    """With the splits made before the word selection (the only order the device allows: its split() drops the word DB),
    every labelled case answers split_first_answer(label): the EOS edges keep their meaning there too."""
    n = n_cut = 0
    for sc in cases:
        if not sc.splits:
            continue
        so = session(oracle, sc, splits_first=True)
        for p, pair in enumerate(sc.pairs):
            _, ori = so.target_match(pair, orient=True)
            for l in sc.labels:
                if l.pair == p:
                    got = bool(ori[l.seq] & (1 if l.orient == "FR" else 2))
                    assert got == AE.split_first_answer(l), (sc.name, l)
                    n += 1
                    n_cut += l.split_first_cut
    assert n > 100 and 0 < n_cut < n
