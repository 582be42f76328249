"""Whole-template primer alignment at real amplicon and set sizes (TEST INFRASTRUCTURE, plain helper module, no GPU).

PCR::find_multiplex_background_match (background_match.cpp:168-295) aligns F, (F), R and (R) of a pair -- (X) is
Word::complement() of X, which reverses as it complements (word.h:140-183): the reverse complement -- against every
whole sequence of a set and sets the sequence's bit when any of the four normalised, optionally TaqMAMA-corrected scores reaches the threshold.  The device does this with the
streaming form of its alignment kernel: one half-wave per alignment, the template fed through a 32-column chunk.  The
scenarios built here put templates where that can go wrong and carry per-sequence labels saying what was planted and why:

    scenario(lib, name)        # lib: the oracle; name: one of NAMES.  Seeded, cached per name.
    sc.seqs, sc.weights, sc.pairs, sc.thresholds, sc.taq, sc.labels
    sc.want[(pair index, threshold, taq)]   # the oracle's bits, bool[n], for every pair in sc.cpu_pairs
    prefix(sc, n)              # the first n sequences as a scenario of their own (bits are per sequence)

* ``ladder q``  (q = 12, 18, 22, 31, 32, the length of F; R has another of these lengths): templates of every length of
  LADDER with a near-copy (exact, one mismatch, one inserted base, one deleted base, a wrong base before the 3' end) of the site of one of the four
  lanes beginning at column 0, ending at the last column, beginning at each offset 32k-|o|+1 .. 32k around an interior
  32-column edge and around the last one (a sample of the offsets above 2 kb), or ending at column 0 / column 1 (the rest
  of the template EOS, so that the last two aligned bases are undefined / half defined); one unplanted template per
  length.  The two sequences the reference aligns in one call (2i, 2i+1) always differ in length, mostly by far.
* ``repeated q``: templates of 300 .. 3 000 bases with two or three occurrences of a site at EQUAL score that differ in
  what TaqMAMA sees -- see _repeated().  The threshold sits on that score, so the bit says which occurrence won the tie.
* ``equality``: thresholds float32(s) * float32(1 / (2|o|)) for attainable s, and the floats next to them.
* ``alphabet``: IUPAC codes, N and '-' in the templates, a primer of degeneracy 64, a degenerate 3' end.
* ``sizes``: 129 short sequences with hits around the 64-bit word edges (use prefix() for 1 .. 129), and ``big``:
  70 001 sequences of 20 .. 40 bases drawn from a few hundred texts (prefix() for 65 535 and 65 536).
* ``batches``: 300 pairs over the ladder set of q = 22; the oracle answers the pairs of sc.cpu_pairs.

Every scenario asserts its own discriminating power when it is built (_check): a set and a clear bit at every threshold
(except where a threshold is MEANT to be reached by all or by none), every label class present, and for the repeated
sites and the equalities that the neighbouring answer differs.  A seed for which an assertion fails is changed here.
"""
import functools
import random
from collections import namedtuple

import numpy as np

from pcramp_amd import words as W
from testdata import rand_seq, revcomp

Scenario = namedtuple("Scenario", "name seqs weights pairs_txt pairs thresholds taq labels want cpu_pairs uniform")
# one label per sequence: what = the class of the case, lane = whose site (0..3 = F, (F), R, (R); None = unplanted),
# place / kind = where and how it was written
Label = namedtuple("Label", "what lane place kind")

LANES = ("F", "(F)", "R", "(R)")
PRIMER_LENGTHS = (12, 18, 22, 31, 32)
LADDER = (1, 2, "q-1", "q", 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 2047, 2048, 4095, 16384, 32766)
KINDS = ("exact", "mismatch", "insert", "delete", "wrong base before the 3' end")
BIG_SIZES = (65535, 65536, 70001)
SMALL_SIZES = (1, 63, 64, 65, 127, 128, 129)
BATCHES = (1, 2, 65, 300)
NAMES = tuple("ladder %d" % q for q in PRIMER_LENGTHS) + ("repeated 22", "repeated 32", "equality", "alphabet", "sizes",
                                                          "big", "batches")
SEED = 20261017


def f32(x):
    return np.float32(x)


def oligos(pair_txt):
    """The four query texts in lane order (background_match.cpp:216-220)."""
    f, r = pair_txt
    return [f, revcomp(f), r, revcomp(r)]


def weights_for(n):
    return [1.0 + 0.25 * (i % 7) for i in range(n)]


def lane_results(lib, pair_txt, seq):
    """The oracle's alignment of each lane's oligo against the template -> 4 x (score, t_stop, q_stop, last1, last2)."""
    t = W.codes_from_text(seq)
    out = []
    for o in oligos(pair_txt):
        r = lib.sw_align_codes(W.codes_from_text(o), t)
        out.append((r.score, r.t_stop, r.q_stop, r.last1, r.last2) if r.valid else (0, 0, 0, 15, 15))
    return out


def lane_scores(lib, pair_txt, seq, taq):
    """background_match.cpp:238-251 in float32 from the oracle's single alignments: the four scores the threshold meets."""
    out = []
    for o, (score, _, _, l1, l2) in zip(oligos(pair_txt), lane_results(lib, pair_txt, seq)):
        sc = f32(f32(score) * (f32(1.0) / f32(2.0 * len(o))))
        if taq:
            c = W.codes_from_text(o)
            sc = f32(sc * f32(lib.taq_mama(int(c[-2]) if len(c) > 1 else 0, int(c[-1]), l1, l2)))
        out.append(sc)
    return out


def equality_threshold(score, oligo_len):
    return float(f32(f32(score) * (f32(1.0) / f32(2.0 * oligo_len))))


def _after(x):
    return float(np.nextafter(f32(x), f32(2.0)))


def _before(x):
    return float(np.nextafter(f32(x), f32(-1.0)))


def _primer(rng, n):
    """A non-degenerate primer whose last two bases differ from each other and from the two before them: an alignment
    that ends one row early, or with the two bytes of the primer's 3' end swapped, meets another TaqMAMA entry."""
    while True:
        s = rand_seq(rng, n)
        if len(set(s[-3:])) == 3 and s[-4] != s[-2] and all(s[i:i + 4] != s[i] * 4 for i in range(n - 3)):
            return s


def _other(rng, *not_these):
    return rng.choice([c for c in "ACGT" if c not in not_these])


def _copy(rng, o, kind):
    k = rng.randrange(4, len(o) - 4)
    if kind == "mismatch":
        return o[:k] + _other(rng, o[k]) + o[k + 1:]
    if kind == "insert":
        return o[:k] + _other(rng, o[k - 1], o[k]) + o[k:]
    if kind == "delete":
        return o[:k] + o[k + 1:]
    if kind.startswith("wrong base"):                                          # the alignment ends two rows early: TaqMAMA sees another pair of bases
        return o[:-2] + _other(rng, o[-2]) + o[-1]
    return o


def _write(rng, L, start, text):
    s = rand_seq(rng, L)
    assert 0 <= start and start + len(text) <= L
    return s[:start] + text + s[start + len(text):]


def _interleave(rng, seqs, labels, odd, far=4):
    """Order the set so that the couple (2i, 2i+1) the reference aligns in one call holds a short and a long template, the
    long one first in every other couple; the count is made odd / even as asked by dropping into place one more random
    template."""
    if (len(seqs) % 2 == 1) != odd:
        seqs = seqs + [rand_seq(rng, 40)]
        labels = labels + [Label("unplanted", None, None, None)]
    order = sorted(range(len(seqs)), key=lambda i: (len(seqs[i]), i))
    half = len(order) // 2
    out = []
    for i in range(half):
        a, b = order[i], order[i + half + (len(order) % 2)]
        out += [b, a] if i % 2 else [a, b]
    if len(order) % 2:
        out.append(order[half])
    assert sorted(out) == list(range(len(seqs)))
    seqs, labels = [seqs[i] for i in out], [labels[i] for i in out]
    lens = [len(s) for s in seqs]
    couples = [(min(lens[i], lens[i + 1]), max(lens[i], lens[i + 1])) for i in range(0, len(lens) - 1, 2)]
    assert all(a < b for a, b in couples)
    assert sum(1 for a, b in couples if b >= far * a) * 2 >= len(couples)
    assert any(lens[i] > lens[i + 1] for i in range(0, len(lens) - 1, 2)) and any(lens[i] < lens[i + 1] for i in range(0, len(lens) - 1, 2))
    return seqs, labels


def _ladder_set(rng, pair_txt, odd):
    ol = oligos(pair_txt)
    q = len(pair_txt[0])
    seqs, labels = [], []

    def add(s, *label):
        seqs.append(s)
        labels.append(Label(*label))

    for L in LADDER:
        L = {"q-1": q - 1, "q": q}.get(L, L)
        add(rand_seq(rng, L), "unplanted", None, None, None)
        if L == 1:
            for c in "ACGT":
                add(c, "end at column 0", None, "one base", "exact")
            continue
        if L == 2:
            for lane, o in enumerate(ol):
                add(o[-2:], "end at column 1", lane, "two bases", "exact")
                add(_other(rng, o[-2]) + o[-1], "end at column 1", lane, "two bases", "mismatch")
            continue
        if L <= 257 or L == 4095:
            # the site's last base, last two bases, or last base behind a wrong one, then EOS: the maximum ends at column 0 or 1
            for lane, o in enumerate(ol):
                add(o[-1] + "-" * (L - 1), "end at column 0", lane, "EOS tail", "exact")
                add(o[-2:] + "-" * (L - 2), "end at column 1", lane, "EOS tail", "exact")
                add(_other(rng, o[-2]) + o[-1] + "-" * (L - 2), "end at column 1", lane, "EOS tail", "mismatch")
        n_off = None if L <= 257 else (4 if L <= 4095 else 2)

        def planted(what, start_of):
            lane, kind = rng.randrange(4), rng.choice(KINDS)
            c = _copy(rng, ol[lane], kind)
            start = start_of(len(ol[lane]), len(c))
            if start is None or start < 0 or start + len(c) > L:
                return
            add(_write(rng, L, start, c), what, lane, "start %d" % start, kind)

        for rep in range(2 if L <= 257 else 1):
            planted("begin at column 0", lambda n, m: 0)
            planted("end at the last column", lambda n, m: L - m)
        # around the edges of the 32-column chunk: the site begins at 32k - |o| + 1 .. 32k (d = 0 .. |o| - 1)
        for edge in ("interior edge", "last edge"):
            for d in (range(32) if n_off is None else [None] * n_off):
                def start_of(n, m, d=d):
                    k_last = (L - m) // 32
                    k = k_last if edge == "last edge" else max(1, k_last // 2)
                    d = rng.randrange(n) if d is None else d
                    if k < 1 or d >= n or (edge == "interior edge" and k == k_last):
                        return None
                    return 32 * k - n + 1 + d
                planted(edge, start_of)
    return _interleave(rng, seqs, labels, odd)


def _session(lib, seqs, weights):
    so = lib.session()
    for s, w in zip(seqs, weights):
        so.add_target(s, w)
    return so


def _finish(lib, name, seqs, labels, pairs_txt, thresholds, taq, cpu_pairs=None, uniform=()):
    pairs = [(lib.centered_word(f), lib.centered_word(r)) for f, r in pairs_txt]
    weights = weights_for(len(seqs))
    cpu_pairs = tuple(range(len(pairs))) if cpu_pairs is None else tuple(cpu_pairs)
    so = _session(lib, seqs, weights)
    want = {}
    for p in cpu_pairs:
        for thr in thresholds:
            for t in taq:
                want[(p, thr, t)] = so.multiplex_match(pairs[p], thr, t).astype(bool)
    sc = Scenario(name, seqs, weights, pairs_txt, pairs, tuple(thresholds), tuple(taq), labels, want, cpu_pairs, tuple(uniform))
    _check(sc)
    return sc


def _check(sc):
    """A set and a clear bit at every threshold and TaqMAMA setting (over the pairs the oracle answered), except at the
    thresholds listed as uniform: reached by every sequence, or by none."""
    assert len(sc.seqs) == len(sc.labels) == len(sc.weights)
    for thr in sc.thresholds:
        for t in sc.taq:
            rows = np.stack([sc.want[(p, thr, t)] for p in sc.cpu_pairs])
            if thr in sc.uniform:
                assert rows.all() or not rows.any(), (sc.name, thr, t)
            else:
                assert rows.any() and not rows.all(), (sc.name, thr, t)


def _ladder(lib, q):
    rng = random.Random("%d ladder %d" % (SEED, q))
    k = PRIMER_LENGTHS.index(q)
    pair_txt = (_primer(rng, q), _primer(rng, PRIMER_LENGTHS[(k + 2) % len(PRIMER_LENGTHS)]))
    seqs, labels = _ladder_set(rng, pair_txt, odd=bool(k % 2))
    sc = _finish(lib, "ladder %d" % q, seqs, labels, [pair_txt], (0.5, 0.8, 0.9), (0, 1))
    # every class is there, for every lane and every kind of copy, and the long templates are planted too
    for what in ("unplanted", "begin at column 0", "end at the last column", "interior edge", "last edge", "end at column 0",
                 "end at column 1"):
        mine = [l for l in labels if l.what == what]
        assert mine, what
        if what not in ("unplanted", "end at column 0", "end at column 1"):
            assert {l.lane for l in mine} == {0, 1, 2, 3} and {l.kind for l in mine} == set(KINDS), what
    lens = {len(s) for s in seqs}
    assert lens >= {1, 2, q - 1, q, 16384, 32766} and max(lens) == 32766
    for L in (2047, 2048, 4095, 16384, 32766):
        assert sum(1 for s, l in zip(seqs, labels) if len(s) == L and l.lane is not None and l.kind is not None) >= 6, L
    # an exact copy is a perfect match wherever it lies (TaqMAMA off: 1.0 >= 0.9), and (X) is the reverse complement: its sites are met too
    w = sc.want[(0, 0.9, 0)]
    for i, l in enumerate(labels):
        if l.kind == "exact" and l.what not in ("end at column 0", "end at column 1"):
            assert w[i], (q, i, l)
    assert any(l.lane == 1 for l in labels) and any(l.lane == 3 for l in labels)
    return sc


# ---- repeated sites
def _repeated(lib, q):
    """Occurrences of the site of oligo o (|o| = q) that all score 2(q - 1) and differ in what TaqMAMA sees:
      P  o[:q-1] and a wrong base: ends in row q-2 on plain bases -- the primer's 3' end meets o[q-3], o[q-2]: factor < 1;
      D  the same with the last matched base written as a two-fold IUPAC code that holds it: same row, same score, and
         a degenerate base switches the correction off: factor 1;
      E  a wrong base and o[1:]: ends in row q-1 on the primer's own last two bases: factor 1.
    With the threshold ON that score and TaqMAMA on, the bit is set iff the occurrence that supplies the last two aligned
    bases is a D or an E.  P and D end in the same row: the LAST one in the template wins (the larger column).  E against
    P is a tie between rows: E wins wherever it lies (the larger row).  `cut` = the template cut before its last
    occurrence; the builder asserts with the oracle that the answer changes for every template whose occurrences are P / D
    and stays for the E ones, and that without TaqMAMA every template reaches the threshold."""
    for attempt in range(50):
        rng = random.Random("%d repeated %d %d" % (SEED, q, attempt))
        pair_txt = (_primer(rng, q), _primer(rng, q))
        ol = oligos(pair_txt)
        ok = True
        for o in ol:
            c = [int(x) for x in W.codes_from_text(o)]
            ok = ok and lib.taq_mama(c[-2], c[-1], c[-3], c[-2]) < 1.0 and lib.taq_mama(c[-2], c[-1], c[-2], c[-1]) == 1.0
        if ok:
            break
    assert ok
    degen = {"A": "MRW", "C": "MSY", "G": "RSK", "T": "WYK"}

    def occ(o, kind):
        if kind == "P":
            return o[:q - 1] + _other(rng, o[q - 1])
        if kind == "D":
            return o[:q - 2] + rng.choice(degen[o[q - 2]]) + _other(rng, o[q - 1])
        return _other(rng, o[0]) + o[1:]

    seqs, labels, cuts, flips = [], [], [], []

    def template(parts, what, place):
        """parts: [(lane, kind)] in template order, at random positions with at least 40 bases between them."""
        L = rng.randint(300, 3000)
        texts = [occ(ol[lane], kind) for lane, kind in parts]
        while True:
            starts = sorted(rng.sample(range(8, L - 40), len(parts)))
            if all(b - a >= q + 40 for a, b in zip(starts, starts[1:])):
                break
        s = rand_seq(rng, L)
        for st, t in zip(starts, texts):
            s = s[:st] + t + s[st + len(t):]
        seqs.append(s)
        cuts.append(s[:starts[-1] - 4])
        labels.append(Label(what, parts[-1][0], place, "".join(k for _, k in parts)))

    for lane in range(4):
        for kinds in ("PD", "DP", "PDP", "DPD", "PPD", "DDP"):
            template([(lane, k) for k in kinds], "same row tie", "%d occurrences" % len(kinds))
            flips.append(True)
        for kinds in ("EP", "PE"):
            template([(lane, k) for k in kinds], "row tie", "2 occurrences")
            flips.append(kinds == "PE")                                        # (cut: P alone; EP cut leaves the E that won anyway)
    # F against (F) (and R against (R)): the two lanes' occurrences end within a chunk of each other; the lanes keep their own
    # last two bases
    for a, b in ((0, 1), (1, 0), (2, 3), (3, 2)):
        for ka, kb in (("P", "D"), ("D", "P"), ("P", "P")):
            template([(a, ka), (b, kb)], "lane tie", "two lanes")
            flips.append((ka, kb) == ("P", "D"))
    for _ in range(3):
        seqs.append(rand_seq(rng, rng.randint(300, 3000)))
        cuts.append(seqs[-1][:200])
        labels.append(Label("unplanted", None, None, None))
        flips.append(False)
    T = equality_threshold(2 * (q - 1), q)
    sc = _finish(lib, "repeated %d" % q, seqs, labels, [pair_txt], (T, 0.8), (1, 0))
    cut = _session(lib, cuts, sc.weights).multiplex_match(sc.pairs[0], T, 1).astype(bool)
    full, plain = sc.want[(0, T, 1)], sc.want[(0, T, 0)]
    for i, l in enumerate(labels):
        if l.what == "unplanted":
            assert not full[i] and not plain[i]
            continue
        assert plain[i], (i, l)                                                # without the correction every occurrence reaches T
        assert (full[i] != cut[i]) == flips[i], (i, l)
        last_kind = l.kind[-1]
        if l.what == "same row tie":
            assert full[i] == (last_kind == "D"), (i, l)
        if l.what == "row tie":
            assert full[i], (i, l)
        # the python restatement of the four lanes agrees, and the winning lane ends where the label says
        ls = lane_scores(lib, pair_txt, seqs[i], 1)
        assert any(x >= f32(T) for x in ls) == bool(full[i])
        r = lane_results(lib, pair_txt, seqs[i])[l.lane]
        assert r[0] == 2 * (q - 1) and r[2] == (q - 1 if "E" in l.kind and l.what == "row tie" else q - 2), (i, l, r)
    assert sum(flips) * 2 >= len(flips)
    assert {len(s) > 1500 for s in seqs} == {True, False}
    return sc


# ---- thresholds at equality
def _equality(lib):
    rng = random.Random("%d equality" % SEED)
    pair_txt = (_primer(rng, 18), _primer(rng, 25))
    ol = oligos(pair_txt)
    seqs, labels = [], []
    # suffixes o[k:] behind a wrong base: score 2(|o| - k), ending in the last row on the primer's own 3' end (TaqMAMA factor 1)
    for lane, o in enumerate(ol):
        for k in (0, 1, 2, 4, 7):
            for L in (40, 77, 130):
                st = rng.randrange(1, L - len(o) - 1)
                text = (_other(rng, o[k - 1]) if k else "") + o[k:]
                seqs.append(_write(rng, L, st, text))
                labels.append(Label("suffix %d" % k, lane, "start %d" % st, "exact"))
    for L in (1, 5, 20, 40, 77, 130, 300):
        seqs.append(rand_seq(rng, L))
        labels.append(Label("unplanted", None, None, None))
    thresholds, uniform, attained = [], [], []
    for lane, k in ((0, 0), (0, 1), (2, 1), (2, 2), (1, 4), (3, 7)):
        n = len(ol[lane])
        t = equality_threshold(2 * (n - k), n)
        attained.append(t)
        thresholds += [_before(t), t, _after(t)]
    low = equality_threshold(2, 25)                                            # one matching base of R: every sequence holds one
    none = _after(1.0)
    thresholds += [low, none]
    uniform += [low, none]
    thresholds = sorted(set(thresholds))
    sc = _finish(lib, "equality", seqs, labels, [pair_txt], thresholds, (0, 1), uniform=uniform)
    for taq in (0, 1):
        for t in attained:
            below, at, above = (sc.want[(0, x, taq)] for x in (_before(t), t, _after(t)))
            assert np.array_equal(below, at) and (at & ~above).any() and not (above & ~at).any(), (t, taq)
            # the sequences that leave at the next float are those whose best lane sits exactly on the threshold
            for i in np.nonzero(at & ~above)[0]:
                assert max(lane_scores(lib, pair_txt, seqs[i], taq)) == f32(t)
        assert sc.want[(0, low, taq)].all() and not sc.want[(0, none, taq)].any()
    assert len({float(t) for t in attained}) == len(attained)
    return sc


# ---- alphabet
def _alphabet(lib):
    rng = random.Random("%d alphabet" % SEED)
    contains = {"A": "MRWVHDN", "C": "MSYVHBN", "G": "RSKVDBN", "T": "WYKHDBN"}
    f = list(_primer(rng, 20))
    for k in (3, 6, 9, 11, 13, 15):                                           # six two-fold positions: degeneracy 64
        f[k] = rng.choice([c for c in "MRWSYK" if f[k] in contains and c in contains[f[k]]])
    r = _primer(rng, 22)
    r = r[:-1] + rng.choice([c for c in "MRWSYK" if c in contains[r[-1]]])      # a degenerate 3' end
    plain = (_primer(rng, 18), _primer(rng, 24))
    n3 = _primer(rng, 19)
    n3 = n3[:5] + "N" + n3[6:9] + "N" + n3[10:13] + "N" + n3[14:]              # three N: degeneracy 64
    pairs_txt = [("".join(f), r), plain, (n3, _primer(rng, 21))]
    seqs, labels = [], []

    def add(s, what, lane=None, place=None, kind=None):
        seqs.append(s)
        labels.append(Label(what, lane, place, kind))

    def concrete(o):
        """One plain text the (possibly degenerate) oligo matches everywhere."""
        return "".join(c if c in "ACGT" else rng.choice([b for b in "ACGT" if c in contains[b]]) for c in o)

    for pi, pt in enumerate(pairs_txt):
        for lane, o in enumerate(oligos(pt)):
            site = concrete(o)
            n = len(site)
            for L in (45, 150, 300):
                st = rng.randrange(2, L - n - 2)
                add(_write(rng, L, st, site), "plain site", lane, "pair %d" % pi, "exact")
                ks = rng.sample(range(2, n - 2), 3)
                t = list(site)
                for k in ks:
                    t[k] = rng.choice(contains[site[k]])
                add(_write(rng, L, st, "".join(t)), "IUPAC holding the base", lane, "pair %d" % pi, "exact")
                t = list(site)
                for k in ks[:2]:
                    t[k] = rng.choice([c for c in "MRWSYKVHDB" if c not in contains[site[k]]])
                add(_write(rng, L, st, "".join(t)), "IUPAC without the base", lane, "pair %d" % pi, "mismatch")
                t = list(site)
                t[-1] = rng.choice(contains[site[-1]][:3])
                add(_write(rng, L, st, "".join(t)), "IUPAC at the 3' end", lane, "pair %d" % pi, "exact")
                t = list(site)
                t[-2] = _other(rng, site[-2])
                add(_write(rng, L, st, "".join(t)), "wrong base before the 3' end", lane, "pair %d" % pi, "mismatch")
                k = rng.randrange(3, n - 3)
                add(_write(rng, L, st, site[:k] + "-" + site[k + 1:]), "EOS inside the site", lane, "pair %d" % pi, "mismatch")
                add(_write(rng, L, st, site[:k] + "-" + site[k:])[:L], "EOS inserted in the site", lane, "pair %d" % pi, "insert")
                s = _write(rng, L, st, site)
                add(s[:st - 1] + "-" + s[st:st + n] + "-" + s[st + n + 1:], "EOS on both sides of the site", lane, "pair %d" % pi, "exact")
                add(s[:st] + "N" * n + s[st + n:], "N for the whole site", lane, "pair %d" % pi, "exact")
    add("N" * 40, "only N")
    add("N" * 11, "only N")
    add("-" * 30, "only EOS")
    add("-" + rand_seq(rng, 50) + "-", "EOS at both ends")
    add("-", "only EOS")
    for L in (33, 64, 200, 700):
        add(rand_seq(rng, L, p_degen=0.1, p_n=0.05), "unplanted")
    seqs, labels = _interleave(rng, seqs, labels, odd=True, far=2)
    sc = _finish(lib, "alphabet", seqs, labels, pairs_txt, (0.5, 0.8, 0.9, 1.0), (0, 1))
    assert [W.word_degeneracy(p[0]) for p in sc.pairs] == [64.0, 1.0, 64.0]
    for i, l in enumerate(labels):
        hit = [sc.want[(p, 1.0, 0)][i] for p in range(3)]
        if l.what in ("plain site", "IUPAC holding the base", "IUPAC at the 3' end", "EOS on both sides of the site", "N for the whole site"):
            assert hit[int(l.place[-1])], (i, l)
        if l.what == "only N" and len(seqs[i]) == 40:
            assert all(hit) and sc.want[(0, 1.0, 1)][i]
        if l.what == "only EOS":
            assert not any(sc.want[(p, 0.5, t)][i] for p in range(3) for t in (0, 1))
        if l.what in ("EOS inside the site", "IUPAC without the base"):
            assert not sc.want[(1, 1.0, 0)][i] or l.place != "pair 1", (i, l)
    # TaqMAMA decides somewhere (the wrong base before the 3' end), and never where the template's end is degenerate
    assert any((sc.want[(1, t, 0)] != sc.want[(1, t, 1)]).any() for t in sc.thresholds)
    for i, l in enumerate(labels):
        if l.what == "IUPAC at the 3' end":
            p = int(l.place[-1])
            assert sc.want[(p, 1.0, 1)][i], (i, l)
    return sc


# ---- set sizes
def _hit_text(rng, o, L):
    return _write(rng, L, rng.randrange(0, L - len(o) + 1), o)


def _sizes(lib):
    rng = random.Random("%d sizes" % SEED)
    pairs_txt = [(_primer(rng, 18), _primer(rng, 20)), (_primer(rng, 19), _primer(rng, 18))]
    ol = oligos(pairs_txt[0])
    planted = {0: 0, 31: 1, 62: 2, 63: 3, 64: 0, 65: 1, 100: 2, 126: 3, 127: 0, 128: 1}
    seqs, labels = [], []
    for i in range(129):
        L = rng.randint(20, 40)
        if i in planted:
            seqs.append(_hit_text(rng, ol[planted[i]], L))
            labels.append(Label("hit at a word edge", planted[i], "index %d" % i, "exact"))
        elif i % 4 in (1, 3):                                                  # two wrong bases: above the low threshold only
            t = list(oligos(pairs_txt[i % 4 // 2])[i // 4 % 4])
            for j in rng.sample(range(2, len(t) - 2), 2):
                t[j] = _other(rng, t[j])
            seqs.append(_hit_text(rng, "".join(t), max(L, 24)))
            labels.append(Label("near-copy", i // 4 % 4, "pair %d" % (i % 4 // 2), "mismatch"))
        else:
            seqs.append(rand_seq(rng, L))
            labels.append(Label("unplanted", None, None, None))
    sc = _finish(lib, "sizes", seqs, labels, pairs_txt, (0.6, 0.95), (0, 1))
    assert sorted(np.nonzero(sc.want[(0, 0.95, 0)])[0]) == sorted(planted)
    assert not sc.want[(1, 0.95, 0)].any()                                    # the clear bits of the 1-sequence set
    for p in (0, 1):
        assert 15 < sc.want[(p, 0.6, 0)].sum() < 80
    return sc


def _big(lib):
    """70 001 sequences of 20 .. 40 bases drawn from 320 texts: random ones, near-copies of a site (two or three wrong bases:
    above the low threshold, below the high one) and, at the labelled indices only, exact copies.  Which text an index
    gets is random, so the bits of a block of 64 indices repeat nowhere: an index that wraps, or a block that lands in
    another word, shows."""
    rng = random.Random("%d big" % SEED)
    pairs_txt = [(_primer(rng, 18), _primer(rng, 20))]
    ol = oligos(pairs_txt[0])
    texts = [rand_seq(rng, rng.randint(20, 40)) for _ in range(220)]
    for k in range(100):
        t = list(ol[k % 4])
        for j in rng.sample(range(2, len(t) - 2), 2 + k % 2):
            t[j] = _other(rng, t[j])
        texts.append(_hit_text(rng, "".join(t), rng.randint(24, 40)))
    exact = [_hit_text(rng, ol[k % 4], rng.randint(20, 40)) for k in range(12)]
    n = BIG_SIZES[-1]
    marked = sorted({0, 63, 64, 65534, 65535, 65536, n - 1} | set(rng.sample(range(n), 40)))
    seqs = [texts[rng.randrange(len(texts))] for _ in range(n)]
    labels = [Label("drawn", None, None, None)] * n
    for k, i in enumerate(marked):
        seqs[i] = exact[k % len(exact)]
        labels[i] = Label("hit at a marked index", k % len(exact) % 4, "index %d" % i, "exact")
    sc = _finish(lib, "big", seqs, labels, pairs_txt, (0.6, 0.95), (0, 1))
    assert list(np.nonzero(sc.want[(0, 0.95, 0)])[0]) == marked
    lo = sc.want[(0, 0.6, 0)]
    assert 0.05 < lo.mean() < 0.6
    # the blocks of 64 bits are all different from their neighbours one and 1 024 blocks (65 536 indices) on
    words = np.packbits(lo[:n - n % 64].reshape(-1, 64), axis=1)
    assert (words[:-1] != words[1:]).any(axis=1).all() and (words[:-1024] != words[1024:]).any(axis=1).all()
    assert len(set(seqs)) > 300
    return sc


def _batches(lib):
    """300 pairs over the ladder set of q = 22: the ladder's own pair, damaged copies of it and random primers of every
    length.  The oracle answers pairs 0, 1, 64 and 299 (the rows a 1-, 2-, 65- and 300-pair call end with)."""
    base = scenario(lib, "ladder 22")
    rng = random.Random("%d batches" % SEED)
    f, r = base.pairs_txt[0]
    pairs_txt = [(f, r)]
    while len(pairs_txt) < BATCHES[-1]:
        k = len(pairs_txt)
        if k % 3 == 1:
            g = list(f if k % 2 else r)
            for j in rng.sample(range(len(g)), rng.randint(1, 4)):
                g[j] = _other(rng, g[j])
            pairs_txt.append(("".join(g), _primer(rng, rng.randint(12, 32))))
        else:
            pairs_txt.append((_primer(rng, rng.randint(12, 32)), _primer(rng, rng.randint(12, 32))))
    pairs_txt[299] = (pairs_txt[299][0], r)
    return _finish(lib, "batches", base.seqs, base.labels, pairs_txt, (0.8,), (0, 1), cpu_pairs=[b - 1 for b in BATCHES])


@functools.lru_cache(maxsize=None)
def scenario(lib, name):
    if name.startswith("ladder "):
        return _ladder(lib, int(name.split()[1]))
    if name.startswith("repeated "):
        return _repeated(lib, int(name.split()[1]))
    return {"equality": _equality, "alphabet": _alphabet, "sizes": _sizes, "big": _big, "batches": _batches}[name](lib)


def prefix(sc, n):
    """The first n sequences of a scenario: every bit depends on its own sequence alone, so the oracle's answers are the
    first n of the full set's (tests/test_multiplex_templates_host.py checks that on the oracle itself)."""
    assert 0 < n <= len(sc.seqs)
    return sc._replace(name="%s, first %d" % (sc.name, n), seqs=sc.seqs[:n], weights=sc.weights[:n], labels=sc.labels[:n],
                       want={k: v[:n] for k, v in sc.want.items()})
