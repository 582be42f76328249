"""pcr_background_match on the VALUE: the scenarios of tests/background_score_cases.py, in which one sequence holds one candidate
amplicon whose score v = sqrt(max(s0 s3, s1 s2) / (2|F| 2|R|) [x TaqMAMA]) the helper has composed from the oracle's single
alignments and found again by bisecting the oracle's own background_match.  The threshold is put ON every such v, on the float
below and on the float above: the case's bit must be set, set and clear, and the whole bit matrix the oracle's -- a lane
score of k_sw_bg (sw_word_score, the column-parallel Smith-Waterman of the default path) that is off by one, or a tie that
takes the last two aligned bases from the wrong cell, moves a step by at least one float and shows.

The other Smith-Waterman form (k_bg_jobs -> k_sw, the ordered path) is held to the oracle on stacked sets -- several cases on
one sequence, whose bit is an OR over their amplicons: a step on the largest value per sequence, not per case -- and the same
per-case expectations hold the reference-identical index mode, a batch of many rounds of the persistent grid, and a handle that alternates between sets.
The "[pcramp] background_match:" line of every call says which path produced the scores."""
import collections

import numpy as np
import pytest
import torch

import background_score_cases as S
from background_lists import debug_lines as _lines
from pcramp_amd import api

pytestmark = pytest.mark.gpu
f32 = np.float32
MAX_VALUES = 350


def _open(monkeypatch):
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    monkeypatch.delenv("PCRAMP_DEBUG_AMP_CAP", raising=False)
    return api.Screener(0)


def _load(d, sc, oracle):
    """The set as BACKGROUND with its splits, the word DB selected once with the scenario's distinct pairs at 0.72 and a minimum
    oligo length of 16, and equal to the oracle's."""
    d.load_texts(sc.seqs, which=api.BACKGROUND)
    for i, pos in sc.splits:
        d.split(i, pos, which=api.BACKGROUND)
    n = d.select_words(sc.pairs, S.CT, S.MIN_LEN, which=api.BACKGROUND)
    want = S.session(oracle, sc).db_entries()
    assert n == len(want) and d.entries(which=api.BACKGROUND) == want


def _call(d, batch, T, taq, evaluate_all, capfd, path="default path"):
    """One call at score threshold T with the collect threshold kept at 0.72 -> (bits, the last debug line); the call must have
    ended on `path` in one attempt."""
    capfd.readouterr()
    bits = d.find_background_match(batch, T, S.multiplier(T), S.AMP[0], S.AMP[1], bool(taq), evaluate_all=evaluate_all)
    ls = _lines(capfd.readouterr().err)
    assert ls and ls[-1]["end"] == path and ls[-1]["overflow"] == 0 and ls[-1]["kept"] == ls[-1]["emitted"], (T, taq, ls)
    return bits, ls[-1]


def _thinned(sc, vals):
    """At most MAX_VALUES of a scenario's values: every value of a gap, tie, short-key-word or IUPAC case, and of the
    substitution ladder an even spread."""
    keep = {float(v.v) for c, v in zip(sc.cases, vals) if c.cls != "ladder" and not (c.cls == "duplicate" and sc.name == "substitutions")}
    rest = sorted({float(v.v) for v in vals} - keep)
    room = max(0, MAX_VALUES - len(keep))
    if len(rest) > room:
        rest = [rest[int(i)] for i in np.linspace(0, len(rest) - 1, room)] if room else []
    return sorted(keep | set(rest))


def _class(oracle, c, own_value, plain):
    """What a stepped case exercised, for the counts the test prints."""
    if c.cls == "boundary":
        return "gap over columns 15|16"
    if c.cls == "tie":
        return "tie decided by TaqMAMA" if own_value.v < plain.v else "tie"
    if c.cls == "short" and min(oracle.word_size(w) for w in own_value.keys) < 32:
        return "short key word"
    return c.cls


@pytest.mark.parametrize("name", S.NAMES)
def test_on_the_value(oracle, capfd, monkeypatch, name):
    """The threshold on every case's own value, the float below and the float above, TaqMAMA off and on, every candidate
    evaluated: the whole bit matrix is the oracle's, every case's bit is set at its value and clear at the next float, and
    k_sw_bg produced the scores."""
    sc = S.scenario(oracle, name)
    counts = S.candidate_counts(oracle, sc)
    d = _open(monkeypatch)
    try:
        _load(d, sc, oracle)
        compared = stepped = calls = 0
        classes = collections.Counter()
        for taq in (0, 1):
            V = S.step_matrix(oracle, sc, taq)                                 # the oracle's bit of (pair, sequence) at T is V >= T
            vals = S.values(oracle, sc, taq)
            own = {}
            for c, v in zip(sc.cases, vals):
                assert V[c.pair, c.seq] == v.v
                own.setdefault(float(v.v), []).append(c)
            kept, before = _thinned(sc, vals), stepped
            for v in kept:
                got = {}
                for T in (S.below(v), v, S.above(v)):
                    bits, line = _call(d, sc.pairs, T, taq, True, capfd)
                    assert line["emitted"] == sum(counts) and line["pairs"] == len(sc.pairs)
                    want = V >= f32(T)
                    assert np.array_equal(bits, want), (name, taq, T, np.argwhere(bits != want)[:8].tolist())
                    compared += bits.size
                    calls += 1
                    got[T] = bits
                for c in own[v]:
                    assert got[v][c.pair, c.seq] and got[S.below(v)][c.pair, c.seq] and not got[S.above(v)][c.pair, c.seq], (name, taq, c.kind, v)
                    stepped += 1
                    classes[_class(oracle, c, own_value=vals[c.seq], plain=S.value(oracle, sc, c.pair, c.seq, 0))] += 1
            # every case steps on its own value unless the ladder was thinned; then every kept value has its case
            assert stepped - before == len(sc.cases) if len(kept) == len(own) else stepped - before >= len(kept) == MAX_VALUES
        print("%s: %d calls on the default path, %d verdicts compared with the oracle, %d of %d cases (x 2 TaqMAMA settings) stepped "
              "exactly on their value: %s" % (name, calls, compared, stepped, len(sc.cases), dict(classes)))
    finally:
        d.close()


def _some(vs, n):
    vs = sorted(vs)
    return sorted({vs[int(i)] for i in np.linspace(0, len(vs) - 1, n)})


@pytest.mark.parametrize("name", S.NAMES)
def test_reference_identical_mode(oracle, capfd, monkeypatch, name):
    """evaluate_all = False against the oracle with the reference's index rule, at a handful of the cases' values and the floats
    above them: no pair has more candidates than the (filler-padded) set has sequences, so the call stays on the default path."""
    sc = S.scenario(oracle, name)
    sc = S.with_fillers(sc, max(0, max(S.candidate_counts(oracle, sc)) - len(sc.seqs)) + 3)
    assert max(S.candidate_counts(oracle, sc)) <= len(sc.seqs)
    so = S.session(oracle, sc)
    d = _open(monkeypatch)
    try:
        _load(d, sc, oracle)
        for taq in (0, 1):
            for v in _some({float(x.v) for x in S.values(oracle, S.scenario(oracle, name), taq)}, 4) + [0.8]:
                for T in (v, S.above(v)):
                    bits, _ = _call(d, sc.pairs, T, taq, False, capfd)
                    want = S.oracle_bits(oracle, sc, T, taq, 1, so)
                    assert np.array_equal(bits, want), (name, taq, T)
                    assert not bits[:, -3:].any()
    finally:
        d.close()


@pytest.mark.parametrize("name", ["gaps", "ties"])
def test_ordered_path_on_the_same_alignments(oracle, capfd, monkeypatch, name):
    """Several cases on one sequence (stacked()): a pair has more candidates than the set has sequences, the reference mode takes
    the ordered path and k_sw -- the anti-diagonal form -- scores the same key words; evaluate_all stays with k_sw_bg.  A stacked
    sequence's bit is an OR over its amplicons, so this is no step per case: the thresholds are the stacked set's OWN step values
    (the largest value on each sequence, bisected from the oracle) and the floats above them.  With every candidate evaluated
    the bit matrix is V >= T and every sequence steps on its value; the ordered path is held to the oracle with the
    reference's index rule at the same thresholds, where the dropped candidates make some verdicts differ."""
    base = S.scenario(oracle, name)
    sc = S.stacked(oracle, base)
    counts = S.candidate_counts(oracle, sc)
    assert max(counts) > len(sc.seqs)
    so = S.session(oracle, sc)
    d = _open(monkeypatch)
    try:
        _load(d, sc, oracle)
        differ = stepped = 0
        for taq in (0, 1):
            V = S.step_matrix(oracle, sc, taq)
            for v in _some({float(x) for x in V[V > 0]}, 40):
                at = {}
                for T in (v, S.above(v)):
                    bits, line = _call(d, sc.pairs, T, taq, False, capfd, path="ordered path")
                    want = S.oracle_bits(oracle, sc, T, taq, 1, so)
                    assert np.array_equal(bits, want), (name, taq, T, "ordered path")
                    assert line["emitted"] == sum(counts)
                    at[T], _ = _call(d, sc.pairs, T, taq, True, capfd)
                    assert np.array_equal(at[T], V >= f32(T)), (name, taq, T, "default path")
                    differ += int((want != at[T]).sum())
                stepped += int((at[v] & ~at[S.above(v)]).sum())
                assert (at[v] & ~at[S.above(v)]).any()
        print("%s, stacked: %d sequences, candidates per pair %s, %d (pair, sequence) steps on the largest value of the sequence, "
              "%d verdicts differ between the two modes" % (name, len(sc.seqs), counts, stepped, differ))
    finally:
        d.close()


def test_many_rounds(oracle, capfd, monkeypatch):
    """The pairs of the substitution ladder repeated in one batch until the persistent grid of k_sw_bg (8 n_cu workgroups, 16 n_cu
    records a round) goes round more than twice: every repeat's row is its original's and the oracle's."""
    sc = S.scenario(oracle, "substitutions")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    batch, origin, records = S.many_rounds(oracle, sc, n_cu)
    assert records > 32 * n_cu
    d = _open(monkeypatch)
    try:
        _load(d, sc, oracle)
        for taq in (0, 1):
            V = S.step_matrix(oracle, sc, taq)
            vs = _some({float(x.v) for x in S.values(oracle, sc, taq)}, 3)
            for T in (vs[0], vs[1], S.above(vs[1])):
                bits, line = _call(d, batch, T, taq, True, capfd)
                assert line["emitted"] == records and line["pairs"] == len(batch), line
                want = V >= f32(T)
                for i, o in enumerate(origin):
                    assert np.array_equal(bits[i], want[o]), (taq, T, i, o)
                assert want.any() and not want.all()
        print("many rounds: %d pairs, %d records in one call; one round of k_sw_bg takes %d (n_cu = %d)" % (len(batch), records, 16 * n_cu, n_cu))
    finally:
        d.close()


def test_poisoning_between_calls(oracle, capfd, monkeypatch):
    """One handle alternating between two scenarios with different pair counts and key-word lengths: what a call leaves behind
    (sw_out, the counters, the staged queries) must not reach the next -- every result equals that of a fresh handle."""
    plan = []
    for name in ("short", "ties", "short", "alphabet", "ties"):
        sc = S.scenario(oracle, name)
        vs = _some({float(x.v) for x in S.values(oracle, sc, 1)}, 3)
        plan.append((sc, [(T, taq) for taq in (1, 0) for v in vs for T in (v, S.above(v))]))
    fresh = {}
    for sc, calls in plan:
        if sc.name in fresh:
            continue
        d = _open(monkeypatch)
        try:
            _load(d, sc, oracle)
            fresh[sc.name] = [_call(d, sc.pairs, T, taq, True, capfd)[0] for T, taq in calls]
        finally:
            d.close()
    d = _open(monkeypatch)
    try:
        for sc, calls in plan:
            _load(d, sc, oracle)
            for k, (T, taq) in enumerate(calls):
                bits, _ = _call(d, sc.pairs, T, taq, True, capfd)
                assert np.array_equal(bits, fresh[sc.name][k]), (sc.name, T, taq)
                assert np.array_equal(bits, S.step_matrix(oracle, sc, taq) >= f32(T)), (sc.name, T, taq)
    finally:
        d.close()
