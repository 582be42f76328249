"""The scenarios of tests/background_score_cases.py held to what they promise, from the oracle and the reference alone (no GPU):
the value composed from single alignments IS the float at which the oracle's background_match steps, one sequence holds one
case, every class of alignment the device kernel can get wrong is there and decides a value, a score that is off by one moves
the value by at least one float, and the oracle's answers on these very inputs are the compiled reference's."""
import collections
import gzip
import json
import os

import numpy as np
import pytest

import background_score_cases as S
import reference_tape
from testdata import revcomp

TAPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "background_score_reference_calls.json.gz")
_RECORD = os.environ.get("PCRAMP_RECORD_REFERENCE") == "1"
f32 = np.float32


def _bits(x):
    return f32(x).view(np.uint32)


def _deciding(v):
    return [v.lanes[l] for l in v.deciding]


def _horizontal(lane):                                                      # template columns skipped: a gap in the query
    return lane[4] - lane[3] > lane[2] - lane[1]


def _vertical(lane):
    return lane[4] - lane[3] < lane[2] - lane[1]


# ------------------------------------------------------------------ the scenarios are what they say
def test_sizes(oracle):
    total = 0
    for name in S.NAMES:
        sc = S.scenario(oracle, name)
        total += len(sc.seqs)
        assert max(len(q) for q in sc.seqs) <= 260 and len(sc.cases) == len(sc.seqs), name      # one sequence, one case
        assert [c.seq for c in sc.cases] == list(range(len(sc.seqs)))
        assert all(n % 2 == 0 and n > 0 for n in S.candidate_counts(oracle, sc)), name          # (the reference needs an even count)
        assert max(S.candidate_counts(oracle, sc)) <= len(sc.seqs), name                       # the default path in either mode
    assert total < 1000
    kinds = {name: {"F same on both strands": 0, "ordinary": 0} for name in S.NAMES}
    for name in S.NAMES:
        for f, _ in S.scenario(oracle, name).pairs_txt:
            kinds[name]["F same on both strands" if revcomp(f) == f else "ordinary"] += 1
    assert all(k["ordinary"] for k in kinds.values())
    assert all(kinds[n]["F same on both strands"] for n in ("substitutions", "gaps", "short", "alphabet"))


def test_multiplier_keeps_the_collect_threshold():
    """float32(T) * float32(multiplier(T)) is 0.72 to within a float, and unsigned(size * ct * ct) is what it is at 0.72."""
    for T in [2.0 ** -7, 0.031, 0.25, 0.5, 0.72, 0.8, 0.99, 1.0, 1.5] + [float(x) for x in np.linspace(0.1, 1.2, 57)]:
        ct = f32(T) * f32(S.multiplier(T))
        assert abs(float(ct) - S.CT) <= 2 * float(np.spacing(f32(S.CT))), T
        for n in range(16, 33):
            assert int(f32(n) * f32(ct * ct)) == int(f32(n) * f32(f32(S.CT) * f32(S.CT))), (T, n)


@pytest.mark.parametrize("name", S.NAMES)
def test_step_values_agree(oracle, name):
    """For every case the value composed in float32 from oracle.sw_align_words on the four (query, key word) lanes equals, bit
    for bit, the float at which the oracle's own background_match steps; the oracle sets the bit AT v and clears it at the next
    float, with TaqMAMA off and on."""
    sc = S.scenario(oracle, name)
    for taq in (0, 1):
        for c, v in zip(sc.cases, S.values(oracle, sc, taq)):
            assert v is not None and v.v > 0, (name, c)
            assert _bits(v.v) == _bits(S.bisected(oracle, sc, c.pair, c.seq, taq)), (name, taq, c.kind, v.v)
            so, p = S.one(oracle, sc, c.seq), sc.pairs[c.pair]
            for T, want in ((float(v.v), 1), (S.above(v.v), 0), (S.below(v.v), 1)):
                assert so.background_match(p, T, S.multiplier(T), S.AMP[0], S.AMP[1], taq)[0][0] == want, (name, taq, c.kind, T)


@pytest.mark.parametrize("name", S.NAMES)
def test_whole_set_is_the_sum_of_its_sequences(oracle, name):
    """The oracle's bit matrix on the whole set, at thresholds on and beside the cases' values, is step_matrix >= T: every bit
    depends on its own sequence alone (the word DB is selected per sequence), and no pair has more candidates than sequences."""
    sc = S.scenario(oracle, name)
    so = S.session(oracle, sc)
    for taq in (0, 1):
        V = S.step_matrix(oracle, sc, taq)
        vs = sorted({float(v.v) for v in S.values(oracle, sc, taq)})
        for v in [vs[0], vs[len(vs) // 3], vs[len(vs) // 2], vs[-1], 0.8]:
            for T in (S.below(v), v, S.above(v)):
                for bug in (0, 1):
                    got = S.oracle_bits(oracle, sc, T, taq, bug, so)
                    assert np.array_equal(got, V >= f32(T)), (name, taq, T, bug)
        # pairs meet the sequences of other pairs' cases too: a few of those form candidates by chance, and they are in V
        assert (V > 0).sum() >= len(sc.cases)


def _window(sc, c, lib, side):
    """The planted key word of an interior site from the module's own text: the 32 bases around it, the oligo's first base in the
    slot a centred word of its length begins at."""
    f, r = sc.pairs_txt[c.pair]
    q, pl = sc.seqs[c.seq], c.planted
    if side == "F":
        a = pl["f_at"] - S.start_slot(len(f))
        return [lib.word(q[a + d:a + d + 32]) for d in (0, len(pl["f_site"]) - len(f))]
    a = S.start_slot(len(r)) - 32 + pl["r_at"] + len(pl["r_site"])
    return [lib.word(revcomp(q[a - d:a - d + 32])) for d in (0, len(pl["r_site"]) - len(r))]


def _end_words(sc, c, lib):
    """The planted key words of a site at a sequence's end, from the module's own text: the first (F) or last (R, read on the
    other strand) c bases as a centred word, for every length c that short_words() says the site selects."""
    f, r = sc.pairs_txt[c.pair]
    q, side = sc.seqs[c.seq], c.planted["side"]
    lens = S.short_words(len(f if side == "F" else r), c.planted["hang"], at_end=side == "R")
    if lens == [32]:
        return lens, _window(sc, c, lib, side)[:1]
    return lens, [lib.centered_word(q[:n] if side == "F" else revcomp(q[-n:])) for n in lens]


@pytest.mark.parametrize("name", S.NAMES)
def test_one_candidate_per_sequence(oracle, name):
    """At least 90 % of the case sequences hold exactly one candidate amplicon at 0.72, the module's own enumeration of them is
    the oracle's count, and the winning amplicon lies on the planted key words.  In the short-key-word scenario the count is
    what the construction gives (short_words()): exactly one candidate for every site that hangs over a sequence's end, for an
    odd-length site lying flush and for a site with a full word, exactly two -- on the words of 2j and 2j + 1 bases -- for a
    site set in by fewer bases than a full word needs.  Those set-in sites are what puts the even word lengths into the DB; they
    stand outside the 90 %, and every other sequence of that scenario holds exactly one."""
    sc = S.scenario(oracle, name)
    n_one = n_two = 0
    for c, v in zip(sc.cases, S.values(oracle, sc, 0)):
        so = S.one(oracle, sc, c.seq)
        assert so.background_candidates(sc.pairs[c.pair], S.CT, *S.AMP) == v.n_cand >= 1, (name, c.kind)
        n_one += v.n_cand == 1
        if "hang" in c.planted:
            lens, words = _end_words(sc, c, oracle)
            side = "FR".index(c.planted["side"])
            amps = S.amplicons(oracle, so.db_entries(), sc.pairs[c.pair], len(sc.seqs[c.seq]))
            assert v.n_cand == len(lens) == len(amps), (c.kind, lens, v.n_cand)
            assert sorted(a[side] for a in amps) == sorted(words), (c.kind, lens)                  # the planted words, all of them
            assert {a[1 - side] for a in amps} == {_window(sc, c, oracle, "RF"[side])[0]}, c.kind   # ... and the other site's one window
            n_two += v.n_cand == 2
        elif c.cls == "split":
            assert v.n_cand == 1
        else:
            # an indel leaves two readings of the site: the window that holds the bases before it, or the one that holds those behind
            assert v.keys[0] in _window(sc, c, oracle, "F") and v.keys[1] in _window(sc, c, oracle, "R"), (name, c.kind)
    print("%s: %d of %d case sequences hold exactly one candidate amplicon, %d hold the two of a set-in site" % (name, n_one, len(sc.cases), n_two))
    assert n_one + n_two == len(sc.cases) if name == "short" else n_one >= 0.9 * len(sc.cases), (name, n_one, len(sc.cases))
    if name == "short":
        assert (n_one, n_two) == (69, 57)


# ------------------------------------------------------------------ class coverage, read from the oracle's alignments
def test_substitution_ladder(oracle):
    sc = S.scenario(oracle, "substitutions")
    assert [len(f) for f, _ in sc.pairs_txt] == list(S.LADDER_LENGTHS)              # 18 .. 25 and the shortest and longest
    for p, (f, r) in enumerate(sc.pairs_txt):
        mine = [c for c in sc.cases if c.pair == p and c.cls == "ladder"]
        k = S.most_mismatches(len(f))
        assert {c.planted["m"] for c in mine if c.planted["side"] == "F"} == set(range(k + 1)), p    # 0 ... what 0.72 admits
        for where in ("5", "mid", "last", "pen"):                                # every count at every position
            assert sorted(c.planted["m"] for c in mine if c.planted["side"] == "F" and c.planted["where"] == where) == list(range(1, k + 1)), (p, where)
            assert any(c.planted["side"] == "R" and c.planted["where"] == where for c in mine), (p, where)
        assert len(f) - k >= int(f32(len(f)) * f32(S.CT)) > len(f) - k - 1
    # the 5' mismatches are clipped (the alignment starts behind them), the 3' ones end it early: TaqMAMA reads other bases
    v0 = S.values(oracle, sc, 0)
    clipped = sum(1 for c, v in zip(sc.cases, v0) if c.planted.get("where") == "5" and c.planted["side"] == "F" and v.lanes[0][1] >= c.planted["m"])
    early = sum(1 for c, v in zip(sc.cases, v0) if c.planted.get("where") in ("last", "pen") and c.planted["side"] == "F"
                and v.lanes[0][2] < len(sc.pairs_txt[c.pair][0]) - 1)
    assert clipped >= 20 and early >= 20, (clipped, early)
    # values on both sides of the reference's working threshold
    vs = [float(v.v) for v in v0]
    assert min(vs) < 0.5 and sum(1 for x in vs if x >= 0.8) >= 10 and sum(1 for x in vs if 0.6 <= x < 0.8) >= 10


def test_gap_classes(oracle):
    sc = S.scenario(oracle, "gaps")
    v0 = S.values(oracle, sc, 0)
    assert {len(f) for f, _ in sc.pairs_txt[:4]} == {18, 21, 22, 25}
    # insertions and deletions of 1, 2 and 3 bases were planted at EVERY offset of the four sites; an offset is a case unless the
    # pair forms no candidate on its sequence (an indel near the middle leaves neither half enough matches for the word DB at 0.72)
    covered = {}
    for p in range(4):
        n = len(sc.pairs_txt[p][0])
        for gap in ("ins", "del"):
            for d in (1, 2, 3):
                want = set(S.gap_offsets(n, gap, d))
                assert want == set(range(1, n - d)) if gap == "del" else want == set(range(1, n))
                def mine(pl):
                    return pl.get("side") == "F" and pl.get("gap") == gap and pl.get("d") == d
                have = sorted(c.planted["k"] for c in sc.cases if c.cls == "gap" and c.pair == p and mine(c.planted))
                gone = sorted(pl["k"] for cls, _, pair, pl in sc.dropped if cls == "gap" and pair == p and mine(pl))
                assert len(set(have)) == len(have) and not set(have) & set(gone) and set(have) | set(gone) == want, (p, gap, d)
                assert have[0] == 1 and have[-1] == max(want) and 2 * len(have) >= len(want), (p, gap, d, have)
                assert all(3 <= k <= n - 3 for k in gone), (p, gap, d, gone)       # what is missing lies inside the site
                covered[(n, gap, d)] = len(have), len(want)
    print("gaps: offsets that are cases, of those planted, by (primer, kind, bases): %s" % covered)
    horizontal = [(c, v) for c, v in zip(sc.cases, v0) if any(_horizontal(l) for l in _deciding(v))]
    vertical = [(c, v) for c, v in zip(sc.cases, v0) if any(_vertical(l) for l in _deciding(v))]
    print("gaps: %d winning alignments with a horizontal gap, %d with a vertical one" % (len(horizontal), len(vertical)))
    assert len(horizontal) >= 20 and len(vertical) >= 20
    # the 16-lane boundary: lane F+f decides, aligns the whole primer (rows 0 .. n-1) over n + d columns at the cost of ONE gap of
    # d, and the inserted bases continue the site on neither side -- the skipped columns are the inserted ones
    runs = []
    for c, v in zip(sc.cases, v0):
        if c.cls != "boundary":
            continue
        n, d, l0 = len(sc.pairs_txt[c.pair][0]), c.planted["d"], v.lanes[0]
        assert v.deciding == (0, 3) and v.n_cand == 1 and _horizontal(l0)
        assert l0[0] == 2 * n - S.GAP_COST[d] and (l0[1], l0[2]) == (0, n - 1) and (l0[3], l0[4]) == (S.start_slot(n), S.start_slot(n) + n - 1 + d)
        site, f, k = c.planted["f_site"], sc.pairs_txt[c.pair][0], c.planted["k"]
        assert site[:k] == f[:k] and site[k + d:] == f[k:] and site[k] != f[k] and site[k + d - 1] != f[k - 1]
        assert c.planted["cols"] == list(range(S.start_slot(n) + k, S.start_slot(n) + k + d))
        assert oracle.word_start(v.keys[0]) == 0 and oracle.word_size(v.keys[0]) == 32       # key-word column = slot
        runs.append(set(c.planted["cols"]))
    left = sum(1 for r in runs if 15 in r and 16 not in r)
    right = sum(1 for r in runs if 16 in r and 15 not in r)
    both = sum(1 for r in runs if {15, 16} <= r)
    print("gaps: %d gaps over columns 15|16 (%d end at 15, %d begin at 16, %d cover both)" % (len(runs), left, right, both))
    assert len(runs) >= 6 and left >= 1 and right >= 1 and both >= 1


def test_tie_classes(oracle):
    sc = S.scenario(oracle, "ties")
    v0, v1 = S.values(oracle, sc, 0), S.values(oracle, sc, 1)
    by = collections.defaultdict(list)
    differ = 0
    for c, a, b in zip(sc.cases, v0, v1):
        l1 = a.lanes[1]
        assert a.deciding == (1, 2) and l1[0] == 2 * S.TIE_M and l1[4] == S.tie_stop(c.kind), c
        # both copies hold the maximum of lane 1: each alone scores what the two score together
        F = oracle.centered_word(revcomp(sc.pairs_txt[c.pair][0]))
        text = sc.seqs[c.seq][c.planted["f_at"] - 7:c.planted["f_at"] + 25]
        for cut in (text[:25] + "-" * 7, "-" * 7 + text[7:]):
            assert oracle.sw_align_codes(S.W.codes_from_text(revcomp(sc.pairs_txt[c.pair][0])), S.W.codes_from_text(cut)).score == 2 * S.TIE_M, c
        assert oracle.sw_align_words(F, oracle.word(text)).tup() == l1
        winner = S.tie_winner(c.kind)
        assert (b.v < a.v) == (winner == "P"), (c.kind, a.v, b.v)              # which occurrence supplied the last two aligned bases
        differ += b.v < a.v
        by[(c.pair, c.kind)].append((a.v, b.v))
    for p in range(len(sc.pairs)):
        for x, y in (("PD", "DP"), ("EP", "PE"), ("PP", "DD")):
            assert {a for a, _ in by[(p, x)]} == {a for a, _ in by[(p, y)]}   # equal without TaqMAMA ...
        assert {b for _, b in by[(p, "PD")]} != {b for _, b in by[(p, "DP")]}  # ... told apart by the order of the copies with it
        assert {b for _, b in by[(p, "EP")]} == {b for _, b in by[(p, "PE")]}  # the larger row wins wherever it lies
    print("ties: %d cases whose verdict at v differs between TaqMAMA on and off" % differ)
    assert differ >= 10


def test_short_key_words(oracle):
    sc = S.scenario(oracle, "short")
    sizes, starts, over_cut = collections.Counter(), set(), 0
    for c in sc.cases:
        so = S.one(oracle, sc, c.seq)
        for fk, rk in S.amplicons(oracle, so.db_entries(), sc.pairs[c.pair], len(sc.seqs[c.seq])):
            for w in (fk, rk):
                n = oracle.word_size(w)
                sizes[n] += 1
                starts.add(oracle.word_start(w))
                assert oracle.word_start(w) == S.start_slot(n) and oracle.word_stop(w) - oracle.word_start(w) + 1 == n, (c.kind, n)
            if c.cls == "split":                                             # the F key word is read ACROSS the cut: the cut base is skipped
                q, cut = sc.seqs[c.seq], dict(sc.splits)[c.seq]
                text = S.W.word_text(fk)
                over_cut += text not in q and text in q[:cut] + q[cut + 1:] and 0 < c.planted["f_at"] - cut <= 6
    print("short: key words by length %s" % sorted(sizes.items()))
    assert set(sizes) == set(range(S.MIN_LEN, 33))                           # every length the DB forms
    assert sum(n for k, n in sizes.items() if k < 32) >= 60 and starts >= set(range(0, 9))
    assert over_cut == 2 == len(sc.splits)
    hang = {(c.planted["side"], c.planted["hang"]) for c in sc.cases if c.cls == "short"}
    assert {("F", -2), ("F", -1), ("F", 0), ("F", 1), ("R", -1), ("R", 0), ("R", 1)} <= hang


def test_alphabet(oracle):
    sc = S.scenario(oracle, "alphabet")
    assert any(set(f + r) - set("ACGT") for f, r in sc.pairs_txt) and any(not set(f + r) - set("ACGT") for f, r in sc.pairs_txt)
    letters = set("".join(f + r for f, r in sc.pairs_txt))
    assert letters & set("MRWSYK") and letters & set("VHDB") and "N" in letters
    seen = collections.Counter()
    for c, v in zip(sc.cases, S.values(oracle, sc, 0)):
        if c.cls != "alphabet":
            continue
        seen[c.planted["codes"]] += 1
        site = c.planted["f_site"] if c.planted["side"] == "F" else c.planted["r_site"]
        key = v.keys[0 if c.planted["side"] == "F" else 1]
        if c.planted["codes"] in ("holds", "three", "N", "lacks", "end", "pen"):
            assert set(site) - set("ACGT") and oracle.word_degeneracy(key) > 1, c.kind
        if c.planted["codes"] == "flank":
            assert not set(site) - set("ACGT") and oracle.word_degeneracy(key) > 1, c.kind    # codes beside the site, inside the key word
    assert set(seen) == set(S.ALPHABET_KINDS) and all(n >= 4 for n in seen.values()), seen
    # match means "the sets intersect": a code that holds the base costs nothing, one that does not costs a mismatch
    by = {(c.pair, c.planted["side"], c.planted["codes"]): v for c, v in zip(sc.cases, S.values(oracle, sc, 0)) if c.cls == "alphabet"}
    for p in range(len(sc.pairs)):
        for side, lane in (("F", 0), ("R", 2)):
            plain = by[(p, "F", "plain")].lanes[lane][0]
            assert by[(p, side, "holds")].lanes[lane][0] == plain and by[(p, side, "N")].lanes[lane][0] == plain, (p, side)
            assert by[(p, side, "lacks")].lanes[lane][0] <= plain, (p, side)
            if not set("".join(sc.pairs_txt[p])) - set("ACGT"):                # (a degenerate primer may meet the other code all the same)
                assert by[(p, side, "lacks")].lanes[lane][0] < plain, (p, side)


def test_a_wrong_score_would_show(oracle):
    """For every pair of the scenarios and every product two lanes of those lengths can form, distinct products give distinct
    float32 values, with every TaqMAMA factor product that occurs in the cases (and without): a lane score that is off by one
    moves the step by at least one float."""
    for name in S.NAMES:
        sc = S.scenario(oracle, name)
        factors = collections.defaultdict(lambda: {f32(1.0)})
        for c, a, b in zip(sc.cases, S.values(oracle, sc, 0), S.values(oracle, sc, 1)):
            for which in ((0, 3), (1, 2)):                                     # the float32 factor products as compose() forms them
                factors[c.pair].add(S.taq_product(oracle, sc.pairs_txt[c.pair], b.lanes, which))
        for p, (f, r) in enumerate(sc.pairs_txt):
            prods = np.arange(0, 4 * len(f) * len(r) + 1, dtype=np.float32)
            base = (prods * (f32(1.0) / f32(2.0 * len(f)))).astype(np.float32) * (f32(1.0) / f32(2.0 * len(r)))
            for t in factors[p]:
                v = np.sqrt((base * t).astype(np.float32).astype(np.float64)).astype(np.float32)
                assert (np.diff(v) > 0).all(), (name, p, t)


def test_many_rounds_batch(oracle):
    sc = S.scenario(oracle, "substitutions")
    counts = S.candidate_counts(oracle, sc)
    for n_cu in (1, 64, 256, 304):
        batch, origin, records = S.many_rounds(oracle, sc, n_cu)
        assert records > 32 * n_cu and records == sum(counts[o] for o in origin)
        assert len(batch) == len(origin) <= 16384 and all(batch[i] == sc.pairs[o] for i, o in enumerate(origin))
        assert origin[:len(sc.pairs)] == list(range(len(sc.pairs))) and len(origin) % len(sc.pairs) == 0


@pytest.mark.parametrize("name", ["gaps", "ties"])
def test_stacked_sets_take_the_ordered_path(oracle, name):
    """Several cases on one sequence: a pair has more candidates than the set has sequences, and the reference's index rule then
    drops some -- the two modes of the oracle differ at some threshold of the cases."""
    sc = S.scenario(oracle, name)
    st = S.stacked(oracle, sc)
    counts = S.candidate_counts(oracle, st)
    assert max(counts) > len(st.seqs) >= 8, (counts, len(st.seqs))
    so = S.session(oracle, st)
    keys = {e[:2] for e in S.session(oracle, sc).db_entries()}
    assert len({e[:2] for e in so.db_entries()} & keys) >= 2 * len(st.seqs)  # the same key words as in the one-case sequences
    vs = sorted({float(v.v) for v in S.values(oracle, sc, 0)})
    sets = [S.oracle_bits(oracle, st, v, 0, bug, so) for v in vs[::max(1, len(vs) // 12)] for bug in (0, 1)]
    assert any(b.any() and not b.all() for b in sets)


# ------------------------------------------------------------------ the oracle held to the compiled reference on these inputs
# The reference's answers are on this file's own tape, in the format and through the proxies of tests/reference_tape.py:
#     PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_background_scores_host.py   # rewrites tests/golden/background_score_reference_calls.json.gz
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
def score_reference(request, oracle, _tapes):
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


@pytest.mark.parametrize("name", S.NAMES)
def test_lanes_oracle_equals_reference(oracle, score_reference, name):
    """reference.sw_align_words8 on the (query, key word) lanes of every candidate amplicon of every case, eight per call as
    background_match.cpp drives them: score, coordinates and the last two aligned bases are the oracle's."""
    sc = S.scenario(oracle, name)
    jobs = []
    for c in sc.cases:
        so = S.one(oracle, sc, c.seq)
        for fk, rk in S.amplicons(oracle, so.db_entries(), sc.pairs[c.pair], len(sc.seqs[c.seq])):
            for k, o in enumerate(S.oligo_texts(sc.pairs_txt[c.pair])):
                jobs.append((oracle.centered_word(o), fk if k < 2 else rk))
    jobs = sorted(set(jobs))
    assert len(jobs) >= 4 * len({c.planted["f_site"] + c.planted["r_site"] for c in sc.cases}) // 2
    compared = 0
    for i in range(0, len(jobs), 8):
        chunk = jobs[i:i + 8]
        chunk = chunk + [chunk[-1]] * (8 - len(chunk))
        want = score_reference.sw_align_words8([q for q, _ in chunk], [t for _, t in chunk])
        for (q, t), w in zip(chunk, want):
            got = oracle.sw_align_words(q, t)
            assert got.score == w[0], (name, q, t)
            if got.score > 0:
                assert got.tup() == tuple(w), (name, q, t)
                compared += 1
    assert compared >= len(jobs) - 8


@pytest.mark.parametrize("name", S.NAMES)
def test_background_match_oracle_equals_reference(oracle, score_reference, name):
    """find_background_match of the compiled reference on the whole scenario, at thresholds on and beside the cases' values:
    its bits are the oracle's, and its candidate count -- even for every pair, or the reference reads out of bounds -- too."""
    sc = S.scenario(oracle, name)
    so, sr = S.session(oracle, sc), S.session(score_reference, sc)
    assert so.db_entries() == sr.db_entries()
    counts = S.candidate_counts(oracle, sc, so)
    for taq in (0, 1):
        vs = sorted({float(v.v) for v in S.values(oracle, sc, taq)})
        for v in (vs[0], vs[len(vs) // 2], vs[-1], 0.8):
            for T in (v, S.above(v)):
                for k, p in enumerate(sc.pairs):
                    rb, n_amp = sr.background_match(p, T, S.multiplier(T), S.AMP[0], S.AMP[1], taq)
                    assert rb is not None and n_amp == counts[k] and n_amp % 2 == 0, (name, k, n_amp)
                    ob = so.background_match(p, T, S.multiplier(T), S.AMP[0], S.AMP[1], taq, emulate_index_bug=1)[0]
                    assert (np.asarray(rb) == ob).all(), (name, taq, T, k)
