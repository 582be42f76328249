"""Background sets that pin the VALUE pcr_background_match compares with its threshold (TEST INFRASTRUCTURE, plain helper
module, no GPU).

The default path of pcr_background_match scores a candidate amplicon with k_sw_bg -> sw_word_score, a column-parallel
Smith-Waterman of its own (pcramp_amd/csrc/pcr_sw.inc), and k_bg_score folds the four lane scores F+f, (F)+f, R+r, (R)+r
(background_match.cpp:46-62) into one float32 v = sqrt(max(s0 s3, s1 s2) / (2|F| 2|R|) [x TaqMAMA]) that meets the
threshold.  Only the bit comes back.  A scenario here is a background set in which ONE SEQUENCE HOLDS ONE CASE -- one planted
F site and, further on, the reverse complement of one planted R site -- so that the bit of (pair, sequence) is the verdict on
one amplicon, and the threshold at which it steps is v itself.

Two kinds of pairs (the reference multiplies the score of an oligo on its own strand with one on the OPPOSITE strand,
background_match.cpp:82-83):
  * ordinary pairs: v = sqrt(good alignment x poor alignment): the poor lanes are near-random alignments of 16 .. 32 rows
    against 32 columns, where ties and gaps arise by themselves;
  * pairs whose F reads the same on either strand ("palindromic", as in tests/background_lists.py): both factors are good
    alignments and v sits around the reference's working threshold of 0.8.

Every call keeps the collect threshold at the reference's float32(0.8) * float32(0.9) = 0.72 by passing
search_multiplier = multiplier(T): the candidate set of a scenario is the same at every score threshold T.

    sc = scenario(lib, name)            # lib: the oracle.  name: one of NAMES.  Seeded, cached.
    sc.pairs_txt, sc.pairs              # the distinct pairs (the word DB is selected with them at 0.72, min length 16)
    sc.seqs, sc.splits                  # the background set; splits = [(sequence, position)]
    sc.cases                            # Case(cls, kind, pair, seq, planted): what was written where, and why
    sc.dropped                          # (cls, kind, pair, planted) of the proposals that formed no candidate at 0.72: not cases
    values(lib, sc, taq)                # per case: Value(v, lanes, deciding, n_cand, keys): v COMPOSED from oracle.sw_align_words
    bisected(lib, sc, pair, seq, taq)   # the float32 at which the oracle's own background_match steps (0.0: no candidate)
    step_matrix(lib, sc, taq)           # bisected() for every (pair, sequence): the oracle's whole bit matrix at any T is V >= T

Classes (one scenario each): "substitutions", "gaps", "ties", "short", "alphabet"; many_rounds() repeats the pairs of
"substitutions" in a batch; stacked() puts several cases with tying sites on one sequence (more candidates than sequences:
the ordered path; such a sequence's bit is an OR over its amplicons and steps on the largest of their values).  tests/test_background_scores_host.py holds every scenario to what it promises;
tests/test_gpu_background_scores.py runs them on the device.
"""
import functools
import random
from collections import namedtuple

import numpy as np

from pcramp_amd import words as W
from testdata import rand_seq, revcomp
from multiplex_templates import _other, _primer, f32

NAMES = ("substitutions", "gaps", "ties", "short", "alphabet")
SEED = 20261021
BT, MULT = 0.8, 0.9
AMP = (0, 2000)
MIN_LEN = 16
PLUS, MINUS = 1, 2
LADDER_LENGTHS = (16, 18, 19, 20, 21, 22, 23, 24, 25, 32)
GAP_COST = {1: 5, 2: 7, 3: 9}           # SW_GAP_OPEN = -5 for the first skipped base, SW_GAP_EXT = -2 for every further one
TIE_M = 6                               # bases of a tie scenario's planted copies

Case = namedtuple("Case", "cls kind pair seq planted")
Scenario = namedtuple("Scenario", "name pairs_txt pairs seqs splits cases dropped", defaults=[()])
# lanes: 4 x (score, q_start, q_stop, t_start, t_stop, last1, last2); deciding: the two lanes of the larger product;
# keys: (f key word, r key word) of the winning amplicon
Value = namedtuple("Value", "v lanes deciding n_cand keys")


def collect_threshold():
    """bg_threshold * bg_multiplier of the reference's defaults, as the callers form it: a float32 product."""
    return float(f32(BT) * f32(MULT))


CT = collect_threshold()


def multiplier(T):
    """The search multiplier that keeps float32(T) * float32(multiplier) at 0.72 (within one float of it: the collect
    threshold only enters as unsigned(size * ct * ct), and no size of 16 .. 32 puts that product near an integer)."""
    m = f32(CT) / f32(T)
    best = min((m, np.nextafter(m, f32(0)), np.nextafter(m, f32(np.inf))), key=lambda x: abs(float(f32(T) * x) - CT))
    return float(best)


def below(x):
    return float(np.nextafter(f32(x), f32(-1.0)))


def above(x):
    return float(np.nextafter(f32(x), f32(4.0)))


def start_slot(n):
    """The slot of the first base of a centred word of n bases (Word::center)."""
    return (33 - n) // 2


def palindrome(rng, n):
    """A primer of even length that is its own reverse complement, its last three bases distinct."""
    assert n % 2 == 0
    while True:
        h = rand_seq(rng, n // 2)
        s = h + revcomp(h)
        if len(set(s[-3:])) == 3 and s[-4] != s[-2] and all(s[i:i + 4] != s[i] * 4 for i in range(n - 3)):
            return s


# ------------------------------------------------------------------ the oracle's view of one sequence
def session(lib, sc, only=None):
    """An oracle session holding the scenario's set (or its one sequence `only`) as the device holds it, the DB selected."""
    so = lib.session()
    for i, q in enumerate(sc.seqs):
        if only is None or i == only:
            so.add_target(q)
    for i, pos in sc.splits:
        if only is None or i == only:
            so.split(0 if only is not None else i, pos)
    so.select(sc.pairs, threshold=CT, min_len_override=MIN_LEN)
    return so


_ONE = {}


def one(lib, sc, i):
    key = (sc.name, i)
    if key not in _ONE:
        _ONE[key] = session(lib, sc, only=i)
    return _ONE[key]


def _need(lib, w):
    return int(f32(lib.word_size(w)) * f32(f32(CT) * f32(CT)))                # match_words: unsigned(size * thr), thr = ct * ct


def amplicons(lib, entries, pair, length):
    """PCR::collect_candidates on the entries of ONE sequence (pcr_assay.cpp:12-69, 338-441; no split inside an amplicon)
    -> [(f key, r key)], one per candidate amplicon."""
    F, R = pair
    out = []
    for plus_w, minus_w, f_is_plus in ((F, R, True), (R, F, False)):
        ps, pe = lib.word_start(plus_w), lib.word_stop(plus_w)
        ms, me = lib.word_start(minus_w), lib.word_stop(minus_w)
        P = [e for e in entries if e[4] == PLUS and lib.word_and(plus_w, e[:2]) >= _need(lib, plus_w)]
        M = [e for e in entries if e[4] == MINUS and lib.word_and(minus_w, e[:2]) >= _need(lib, minus_w)]
        for p in P:
            for q in M:
                if p[2] + pe >= q[2] - me:
                    continue
                n = min(q[2] - ms, length - 1) - (p[2] + ps) + 1
                if AMP[0] <= n <= AMP[1]:
                    out.append((p[:2], q[:2]) if f_is_plus else (q[:2], p[:2]))
    return out


def oligo_texts(pair_txt):
    f, r = pair_txt
    return [f, revcomp(f), r, revcomp(r)]


def lanes_of(lib, pair_txt, fk, rk):
    """oracle.sw_align_words of the four lanes (background_match.cpp:46-62)."""
    out = []
    for k, o in enumerate(oligo_texts(pair_txt)):
        r = lib.sw_align_words(lib.centered_word(o), fk if k < 2 else rk)
        out.append(r.tup())
    return out


def taq_product(lib, pair_txt, lanes, which):
    """The float32 product of the two TaqMAMA factors of a lane couple, (0, 3) or (1, 2), as background_match.cpp:85-93 forms
    it: each oligo's last two bases against the last two aligned bases of its lane."""
    t = []
    for k in (which if which[0] == 0 else which[::-1]):                        # Fp, Rm and Rp, Fm: the order of the product
        c = W.codes_from_text(oligo_texts(pair_txt)[k])
        t.append(f32(lib.taq_mama(int(c[-2]), int(c[-1]), lanes[k][5], lanes[k][6])))
    return f32(t[0] * t[1])


def compose(lib, pair_txt, lanes, taq):
    """orc_session_background_match's arithmetic in float32 (pcr_oracle.cpp: int product, two float multiplies, the TaqMAMA
    product, a double sqrt stored as float) -> (v, the two deciding lanes)."""
    f, r = pair_txt
    f_norm, r_norm = f32(1.0) / f32(2.0 * len(f)), f32(1.0) / f32(2.0 * len(r))
    prod = []
    for a, b in ((0, 3), (1, 2)):
        x = f32(f32(f32(lanes[a][0] * lanes[b][0]) * f_norm) * r_norm)
        if taq:
            x = f32(x * taq_product(lib, pair_txt, lanes, (a, b)))
        prod.append(x)
    win = 0 if prod[0] > prod[1] else 1
    return f32(np.sqrt(np.float64(prod[win]))), ((0, 3), (1, 2))[win]


_VALUES = {}


def value(lib, sc, pair, seq, taq):
    """The composed value of (pair, sequence): the largest over the sequence's candidate amplicons; None without one."""
    key = (sc.name, pair, seq, taq)
    if key not in _VALUES:
        _VALUES[key] = value_on(lib, one(lib, sc, seq), sc.pairs_txt[pair], sc.pairs[pair], len(sc.seqs[seq]), taq)
    return _VALUES[key]


def value_on(lib, so, pair_txt, pair, length, taq):
    """value() on a one-sequence session."""
    best = None
    amps = amplicons(lib, so.db_entries(), pair, length)
    for fk, rk in amps:
        lanes = lanes_of(lib, pair_txt, fk, rk)
        v, dec = compose(lib, pair_txt, lanes, taq)
        if best is None or v > best.v:
            best = Value(v, lanes, dec, len(amps), (fk, rk))
    return best


def values(lib, sc, taq):
    return [value(lib, sc, c.pair, c.seq, taq) for c in sc.cases]


_LO, _HI = 2.0 ** -7, 2.0


def bisected(lib, sc, pair, seq, taq):
    """The largest float32 T at which the oracle's background_match sets the sequence's bit (emulate_index_bug = 0), found by
    bisection over the float32 bit patterns; 0.0 where the pair has no candidate amplicon on the sequence."""
    so, p = one(lib, sc, seq), sc.pairs[pair]
    if so.background_candidates(p, CT, *AMP) == 0:
        return f32(0.0)

    def bit(T):
        return bool(so.background_match(p, T, multiplier(T), AMP[0], AMP[1], taq, emulate_index_bug=0)[0][0])
    lo, hi = int(f32(_LO).view(np.uint32)), int(f32(_HI).view(np.uint32))
    assert bit(_LO) and not bit(_HI)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bit(float(np.uint32(mid).view(np.float32))):
            lo = mid
        else:
            hi = mid
    return np.uint32(lo).view(np.float32)


_STEPS = {}


def step_matrix(lib, sc, taq):
    """bisected() of every (pair, sequence) -> float32[n_pairs, n_seqs]: the oracle's bit of (pair, sequence) at T is V >= T."""
    key = (sc.name, taq)
    if key not in _STEPS:
        V = np.zeros((len(sc.pairs), len(sc.seqs)), np.float32)
        for s in range(len(sc.seqs)):
            for p in range(len(sc.pairs)):
                V[p, s] = bisected(lib, sc, p, s, taq)
        _STEPS[key] = V
    return _STEPS[key]


def oracle_bits(lib, sc, T, taq, emulate_index_bug=0, so=None):
    """background_match of every pair on the whole set in one session -> bool[n_pairs, n_seqs]."""
    so = session(lib, sc) if so is None else so
    return np.stack([so.background_match(p, T, multiplier(T), AMP[0], AMP[1], taq, emulate_index_bug=emulate_index_bug)[0].astype(bool)
                     for p in sc.pairs])


def candidate_counts(lib, sc, so=None):
    so = session(lib, sc) if so is None else so
    return [so.background_candidates(p, CT, *AMP) for p in sc.pairs]


# ------------------------------------------------------------------ building
class _Builder:
    def __init__(self, lib, name, pairs_txt):
        self.lib, self.name, self.pairs_txt = lib, name, list(pairs_txt)
        self.pairs = [(lib.centered_word(f), lib.centered_word(r)) for f, r in pairs_txt]
        self.rng = random.Random("%d %s" % (SEED, name))
        self.seqs, self.splits, self.cases = [], [], []
        self.dropped = []

    def _probe(self, text, split=None):
        """A session of the one sequence, for the builder's own questions: not kept."""
        return session(self.lib, Scenario(self.name, self.pairs_txt, self.pairs, [text], [] if split is None else [(0, split)], []), only=0)

    def add(self, cls, kind, pair, f_site, r_site, lead=None, tail=None, after_f="", split_before=None, accept=None, **planted):
        """One sequence: lead, the F site, after_f and 40 .. 70 random bases, the reverse complement of the R site, tail.  A sequence on
        which the pair forms no candidate amplicon at 0.72 is not a case and is left out (the site was eroded past what the
        word DB keeps); accept(value) may refuse a draw, which is then repeated with other flanks."""
        rng = self.rng
        for draw in range(40):
            a = rand_seq(rng, rng.randint(36, 50)) if lead is None else lead
            mid = after_f + rand_seq(rng, rng.randint(40, 70))
            b = rand_seq(rng, rng.randint(36, 50)) if tail is None else tail
            text = a + f_site + mid + revcomp(r_site) + b
            assert len(text) <= 260
            split = None if split_before is None else len(a) - split_before
            so = self._probe(text, split)
            if so.background_candidates(self.pairs[pair], CT, *AMP) == 0:
                self.dropped.append((cls, kind, pair, planted))
                return False
            if accept is None or accept(*[value_on(self.lib, so, self.pairs_txt[pair], self.pairs[pair], len(text), t) for t in (0, 1)]):
                break
        else:
            raise AssertionError("%s: no acceptable draw for %s %s" % (self.name, cls, kind))
        if split is not None:
            self.splits.append((len(self.seqs), split))
        planted.update(f_at=len(a), r_at=len(a) + len(f_site) + len(mid), f_site=f_site, r_site=r_site)
        self.cases.append(Case(cls, kind, pair, len(self.seqs), planted))
        self.seqs.append(text)
        return True

    def finish(self):
        """Every pair gets an even number of candidate amplicons on the whole set (the compiled reference reads out of bounds
        on an odd one): a case sequence on which that pair alone forms one candidate is written a second time."""
        sc = Scenario(self.name, self.pairs_txt, self.pairs, self.seqs, self.splits, self.cases, tuple(self.dropped))
        for p in range(len(self.pairs)):
            if candidate_counts(self.lib, sc)[p] % 2 == 0:
                continue
            for c in sc.cases:
                if c.pair != p:
                    continue
                so = self._probe(sc.seqs[c.seq])
                if c.pair == p and not any(s == c.seq for s, _ in sc.splits) \
                        and [so.background_candidates(q, CT, *AMP) for q in self.pairs] == [int(k == p) for k in range(len(self.pairs))]:
                    sc.cases.append(Case("duplicate", c.kind, p, len(sc.seqs), dict(c.planted, of=c.seq)))
                    sc.seqs.append(sc.seqs[c.seq])
                    break
            else:
                raise AssertionError("%s: no sequence to double for pair %d" % (self.name, p))
        assert all(n % 2 == 0 for n in candidate_counts(self.lib, sc))
        return sc


def _substituted(rng, o, where, m):
    """o with m wrong bases: '5' = its first m bases (the local alignment clips them), 'mid', 'last' / 'pen' = the last /
    the penultimate base (what TaqMAMA reads) and m - 1 in the middle."""
    n = len(o)
    middle = list(range(n // 3, n - 4))
    js = {"5": list(range(m)), "mid": rng.sample(middle, m), "last": [n - 1] + rng.sample(middle, m - 1),
          "pen": [n - 2] + rng.sample(middle, m - 1)}[where]
    t = list(o)
    for j in js:
        t[j] = _other(rng, o[j])
    return "".join(t), sorted(js)


def most_mismatches(n):
    """The most wrong bases a site of n may hold and still be selected at 0.72: unsigned(n * 0.72) must match."""
    return n - int(f32(n) * f32(CT))


def _substitutions(lib):
    rng = random.Random("%d substitution primers" % SEED)
    L = LADDER_LENGTHS
    pairs_txt = []
    for i, n in enumerate(L):
        f = palindrome(rng, n) if n % 2 == 0 else _primer(rng, n)
        pairs_txt.append((f, _primer(rng, L[(i + 3) % len(L)])))
    b = _Builder(lib, "substitutions", pairs_txt)
    for p, (f, r) in enumerate(pairs_txt):
        b.add("ladder", "exact", p, f, r, m=0, where=None, side="F")
        k = most_mismatches(len(f))
        for where in ("5", "mid", "last", "pen"):
            for m in range(1, k + 1):
                site, js = _substituted(b.rng, f, where, m)
                b.add("ladder", "%d wrong, %s" % (m, where), p, site, r, m=m, where=where, side="F", at=js)
        for where in ("5", "mid", "last", "pen"):
            site, js = _substituted(b.rng, r, where, 1)
            b.add("ladder", "1 wrong in R, %s" % where, p, f, site, m=1, where=where, side="R", at=js)
    return b.finish()


def _gapped(rng, o, kind, k, d):
    """An insertion of d bases before base k of o (none of them continues the site on either side), or the deletion of
    o[k:k+d]."""
    if kind == "ins":
        ins = [_other(rng, o[k])]
        while len(ins) < d:
            ins.append(rng.choice("ACGT"))
        ins[-1] = _other(rng, o[k - 1], o[k]) if d == 1 else _other(rng, o[k - 1])
        return o[:k] + "".join(ins) + o[k:]
    return o[:k] + o[k + d:]


def periodic_primer(rng, n, period, head=8):
    """`head` random bases and then a unit of `period` distinct bases over and over: an insertion of `period` bases into the
    periodic part leaves every later base of the site facing an equal base, so the site is still selected at 0.72 WITHOUT a
    gap, wherever the insertion lies -- also in the middle of the primer, under key-word columns 15 and 16."""
    unit = "".join(rng.sample("ACGT", period))
    while True:
        h = rand_seq(rng, head)
        if h[-1] != unit[-1] and all(h[i:i + 4] != h[i] * 4 for i in range(head - 3)):
            return (h + unit * n)[:n]


def boundary_runs(n, period):
    """(offset k, inserted key-word columns) of the insertions of `period` bases into a site of n whose skipped columns
    touch the 16-lane boundary 15|16."""
    s0 = start_slot(n)
    out = []
    for k in range(9, n - 3):
        cols = list(range(s0 + k, s0 + k + period))
        if 15 in cols or 16 in cols:
            out.append((k, cols))
    return out


def gap_offsets(n, kind, d):
    """Every offset of a site of n at which d bases are inserted before base k, or bases k .. k+d-1 deleted, with at least one
    base of the site left on either side."""
    return range(1, n - (d if kind == "del" else 0))


def _gaps(lib):
    rng = random.Random("%d gap primers" % SEED)
    pairs_txt = [(_primer(rng, 18), _primer(rng, 21)), (_primer(rng, 21), _primer(rng, 25)), (_primer(rng, 25), _primer(rng, 18)),
                 (palindrome(rng, 22), _primer(rng, 20)),
                 (periodic_primer(rng, 25, 2), _primer(rng, 19)), (periodic_primer(rng, 25, 3), _primer(rng, 20))]
    b = _Builder(lib, "gaps", pairs_txt)
    for p, (f, r) in enumerate(pairs_txt[:4]):
        for kind in ("ins", "del"):
            for d in (1, 2, 3):
                for k in gap_offsets(len(f), kind, d):
                    b.add("gap", "%s %d at %d" % (kind, d, k), p, _gapped(b.rng, f, kind, k, d), r, side="F", gap=kind, d=d, k=k)
        if p == 1:                                                           # ... and in the R site: the lanes of the other key word
            for kind in ("ins", "del"):
                for k in range(2, len(r) - 2, 2):
                    b.add("gap", "%s 1 at %d of R" % (kind, k), p, f, _gapped(b.rng, r, kind, k, 1), side="R", gap=kind, d=1, k=k)
    # insertions under the 16-lane boundary: accepted when the gapped lane F+f decides the value
    for p in (4, 5):
        f, r = pairs_txt[p]
        d = p - 2
        for k, cols in boundary_runs(len(f), d):
            site = _gapped(b.rng, f, "ins", k, d)
            r_site = _substituted(b.rng, r, "mid", most_mismatches(len(r)) - 1)[0]   # a weak R + r: F+f x (R)+r is the larger product

            def accept(v0, v1, d=d, n=len(f)):
                l0 = v0.lanes[0]
                return v0.n_cand == 1 and v0.deciding == (0, 3) and v1.deciding == (0, 3) and l0[0] == 2 * n - GAP_COST[d] \
                    and (l0[1], l0[2]) == (0, n - 1) and l0[4] - l0[3] == n - 1 + d
            b.add("boundary", "ins %d under columns %s" % (d, cols), p, site, r_site, accept=accept, side="F", gap="ins", d=d, k=k, cols=cols)
    return b.finish()


def _tie_primer(rng, lib, n):
    """A primer F whose reverse complement (F) meets the two bases before its own 3' end with a TaqMAMA factor below 1."""
    while True:
        f = _primer(rng, n)
        c = [int(x) for x in W.codes_from_text(revcomp(f))]
        if not (lib.taq_mama(c[-2], c[-1], c[-3], c[-2]) < 1.0 and lib.taq_mama(c[-2], c[-1], c[-2], c[-1]) == 1.0
                and len(set(revcomp(f)[-4:])) >= 3):
            continue
        # ... and finds nothing on F's own site that a copy beside it could extend into: between two copies it scores 2 TIE_M
        fc = revcomp(f)
        key = lib.word(tie_copy(rng, fc, "P") + f + tie_copy(rng, fc, "P"))
        if lib.sw_align_words(lib.centered_word(fc), key).score == 2 * TIE_M \
                and lib.sw_align_words(lib.centered_word(fc), lib.centered_word(f)).score <= 6:
            return f


_DEGEN = {"A": "MRW", "C": "MSY", "G": "RSK", "T": "WYK"}


def tie_copy(rng, o, kind):
    """TIE_M + 1 bases that o (the oligo of the poor lane) meets with score 2 TIE_M -- _repeated() of multiplex_templates.py
    moved into the flank of a key word:
      P  o[-M-1:-1] and a wrong base: ends one row early, the 3' end of o meets o[-3], o[-2]: TaqMAMA factor < 1;
      D  the same with its last matched base written as a two-fold code that holds it: a degenerate base, factor 1;
      E  a wrong base and o[-M:]: ends in the last row on o's own last two bases: factor 1."""
    m = TIE_M
    if kind == "E":
        return _other(rng, o[-m - 1]) + o[-m:]
    seg = o[-m - 1:-1]
    if kind == "D":
        seg = seg[:-1] + rng.choice(_DEGEN[seg[-1]])
    return seg + _other(rng, o[-1])


TIE_KINDS = ("PD", "DP", "PP", "DD", "EP", "PE")


def tie_winner(kinds):
    """Which of the two copies (left of the site, right of it) supplies the last two aligned bases: E wherever it lies (the
    larger row), otherwise the right one (the larger column)."""
    return "E" if "E" in kinds else kinds[1]


def tie_stop(kinds):
    """The key-word column the winning copy's alignment ends in: the left copy lies in columns 0 .. 6, the right one in 25 .. 31."""
    return 6 if kinds == "EP" else (31 if kinds == "PE" else 30)


def _ties(lib):
    """F of 18 at key-word columns 7 .. 24: the seven columns on either side hold a copy each for (F), the poor lane of the
    product (F)+f x R+r, which a long exact R site makes the larger one.  Both copies score 12: two cells hold the maximum
    of lane 1.  Same row (P / D): the LARGER COLUMN supplies the last two aligned bases; E against P: the larger ROW, wherever
    it lies (seq_overlap.cpp:583: the last cell in row-major order)."""
    rng = random.Random("%d tie primers" % SEED)
    def quiet(n):
        """An R whose reverse complement finds little on R's own site: the product F+f x (R)+r stays the smaller one."""
        while True:
            r = _primer(rng, n)
            if lib.sw_align_words(lib.centered_word(revcomp(r)), lib.centered_word(r)).score <= 8:
                return r
    pairs_txt = [(_tie_primer(rng, lib, 18), quiet(25)), (_tie_primer(rng, lib, 18), quiet(24)), (_tie_primer(rng, lib, 18), quiet(25))]
    b = _Builder(lib, "ties", pairs_txt)
    for p, (f, r) in enumerate(pairs_txt):
        fc = revcomp(f)
        for kinds in TIE_KINDS:
            for rep in range(2):
                def accept(v0, v1, kinds=kinds):
                    l1 = v0.lanes[1]
                    if not (v0.n_cand == 1 and v0.deciding == (1, 2) and l1[0] == 2 * TIE_M and l1[4] == tie_stop(kinds)):
                        return False
                    # the occurrence that wins the tie shows under TaqMAMA: a P lowers the value, a D or an E leaves it
                    return v1.v < v0.v if tie_winner(kinds) == "P" else (v1.v == v0.v and v1.deciding == (1, 2))
                lead = rand_seq(b.rng, 40) + tie_copy(b.rng, fc, kinds[0])
                b.add("tie", kinds, p, f, r, lead=lead, after_f=tie_copy(b.rng, fc, kinds[1]), accept=accept, side="F")
    return b.finish()


def short_words(n, hang, at_end=False):
    """The lengths of the DB words an exact site of a primer of n bases selects when it begins `hang` bases behind a sequence's
    start (hang < 0: the sequence begins inside the site; the same at a sequence's end, mirrored).  The partial words of 2j and
    2j + 1 bases are centred on the same slot; the longer one reaches one slot further.  A site that hangs over, or an odd one
    that lies flush, has a base in that slot: the longer word alone is selected.  A site set further in lies inside both: they
    tie, both are kept, and the sequence holds two candidate amplicons.  From start_slot(n) bases on, the site has a full word.
    Sequence::pack forms the words of 16 .. 31 bases at a sequence's start and those of 17 .. 31 at its end (the trailing loop
    counts one base less than the word holds, sequence.cpp:198-263)."""
    s0 = start_slot(n)
    if hang >= s0:
        return [32]
    j = 16 - s0 + hang
    lens = [2 * j, 2 * j + 1] if hang >= 2 * s0 + n - 32 else [2 * j + 1]
    return [c for c in lens if c >= (17 if at_end else MIN_LEN)]


def _short(lib):
    """Sites at the very start (F) and the very end (R) of a sequence, hanging over by 0, 1, 2 ... bases or set in by a few:
    the DB entry is a centred partial word (tlen < 32, tstart > 0).  A site hanging over selects ONE word; a site set in by a few
    bases selects two, of 2j and 2j + 1 bases -- they are centred on the same slot and hold the site alike -- so such a sequence
    holds two candidate amplicons whose key words differ by one base at the far end, and the value is the larger of the two.
    And one sequence cut by split() two bases before its
    F site: the words over the cut skip the cut base and read on behind it."""
    rng = random.Random("%d short primers" % SEED)
    pairs_txt = [(_primer(rng, 16), _primer(rng, 18)), (palindrome(rng, 18), _primer(rng, 21)), (_primer(rng, 21), _primer(rng, 25)),
                 (_primer(rng, 25), _primer(rng, 16)), (palindrome(rng, 20), _primer(rng, 19)), (_primer(rng, 32), _primer(rng, 31))]
    b = _Builder(lib, "short", pairs_txt)
    for p, (f, r) in enumerate(pairs_txt):
        for h in range(-4, 8):                                                # h < 0: the sequence begins |h| bases into the site
            lead = rand_seq(b.rng, h) if h > 0 else ""
            b.add("short", "F site at %d" % h, p, f[max(0, -h):], r, lead=lead, side="F", hang=h)
            tail = rand_seq(b.rng, h) if h > 0 else ""
            b.add("short", "R site %d before the end" % h, p, f, r[max(0, -h):], tail=tail, side="R", hang=h)
    f, r = pairs_txt[2]
    b.add("split", "cut two bases before the F site", 2, f, r, split_before=2, side="F")
    b.add("split", "cut five bases before the F site", 2, f, r, split_before=5, side="F")
    return b.finish()


_HOLDS = {"A": "MRWVHDN", "C": "MSYVHBN", "G": "RSKVDBN", "T": "WYKHDBN"}


def _coded(rng, site, kind):
    """A plain site with IUPAC codes written over some of its bases."""
    n, t = len(site), list(site)
    ks = rng.sample(range(3, n - 3), 3)
    if kind == "holds":                                                       # two-fold codes that hold the base: matches
        for k in ks[:2]:
            t[k] = rng.choice(_HOLDS[site[k]][:3])
    elif kind == "three":                                                     # a three-fold code that holds it and one that does not
        t[ks[0]] = rng.choice(_HOLDS[site[ks[0]]][3:6])
        t[ks[1]] = [c for c in "VHDB" if c not in _HOLDS[site[ks[1]]]][0]
    elif kind == "N":
        t[ks[0]] = "N"
        t[ks[1]] = rng.choice(_HOLDS[site[ks[1]]][:3])
    elif kind == "lacks":                                                     # two-fold codes without the base: mismatches
        for k in ks[:2]:
            t[k] = rng.choice([c for c in "MRWSYK" if c not in _HOLDS[site[k]]])
    elif kind == "end":                                                       # a code under the primer's 3' end: TaqMAMA switched off
        t[-1] = rng.choice(_HOLDS[site[-1]][:3])
        t[ks[0]] = _other(rng, site[ks[0]])
    elif kind == "pen":
        t[-2] = rng.choice([c for c in "MRWSYK" if c not in _HOLDS[site[-2]]])
    return "".join(t)


ALPHABET_KINDS = ("plain", "holds", "three", "N", "lacks", "end", "pen", "flank")


def _alphabet(lib):
    rng = random.Random("%d alphabet primers" % SEED)

    def concrete(o):
        return "".join(c if c in "ACGT" else rng.choice([x for x in "ACGT" if c in _HOLDS[x]]) for c in o)
    f = list(_primer(rng, 20))
    for k in (4, 9, 14):
        f[k] = rng.choice(_HOLDS[f[k]][:3])
    r = list(_primer(rng, 22))
    r[6], r[12], r[-1] = rng.choice(_HOLDS[r[6]][3:6]), "N", rng.choice(_HOLDS[r[-1]][:3])     # three-fold, N, a degenerate 3' end
    g = list(palindrome(rng, 22))
    g[5], g[16] = {"A": ("W", "W"), "T": ("W", "W"), "C": ("S", "S"), "G": ("S", "S")}[g[5]]   # (still its own reverse complement)
    pairs_txt = [("".join(f), "".join(r)), (_primer(rng, 19), _primer(rng, 24)), ("".join(g), _primer(rng, 18)),
                 (palindrome(rng, 24), _primer(rng, 21))]
    b = _Builder(lib, "alphabet", pairs_txt)
    for p, (f, r) in enumerate(pairs_txt):
        for kind in ALPHABET_KINDS:
            for side in "FR":
                fs, rs = concrete(f), concrete(r)
                lead = tail = None
                if kind == "flank":                                           # codes in the key word beside the site
                    lead = rand_seq(b.rng, 40) + b.rng.choice("MRWSYK") + b.rng.choice("ACGT") + b.rng.choice("VHDB")
                    tail = b.rng.choice("N") + b.rng.choice("ACGT") + b.rng.choice("MRWSYK") + rand_seq(b.rng, 40)
                elif side == "F":
                    fs = _coded(b.rng, fs, kind)
                else:
                    rs = _coded(b.rng, rs, kind)
                if kind == "plain" and side == "R":
                    continue
                b.add("alphabet", "%s, %s site" % (kind, side), p, fs, rs, lead=lead if side == "F" else None,
                      tail=tail if side == "R" else None, side=side, codes=kind)
    return b.finish()


@functools.lru_cache(maxsize=None)
def scenario(lib, name):
    return {"substitutions": _substitutions, "gaps": _gaps, "ties": _ties, "short": _short, "alphabet": _alphabet}[name](lib)


# ------------------------------------------------------------------ derived scenarios
def many_rounds(lib, sc, n_cu):
    """-> (batch, origin, records): the scenario's pairs repeated cyclically until one call emits more than 32 n_cu records -- k_sw_bg
    is a persistent grid of 8 n_cu workgroups of 8 half-waves, one round of it takes 64 n_cu jobs = 16 n_cu records."""
    per_cycle = sum(candidate_counts(lib, sc))
    assert per_cycle > 0
    cycles = (32 * n_cu) // per_cycle + 1
    origin = [i for _ in range(cycles) for i in range(len(sc.pairs))]
    return [sc.pairs[i] for i in origin], origin, cycles * per_cycle


def with_fillers(sc, n):
    """The scenario with n entry-free sequences behind it (40 bases of one letter: no primer of these scenarios reaches 0.72 on
    a homopolymer)."""
    return sc._replace(name="%s + %d fillers" % (sc.name, n), seqs=sc.seqs + ["ACGT"[i % 4] * 40 for i in range(n)])


def stacked(lib, sc, group=4):
    """Several cases on ONE sequence: the case sequences of a pair whose F sites tie in the word DB and whose R sites tie (equal
    ungapped match counts: select_words keeps the best words of a sequence WITH TIES) written one behind the other, `group`
    at a time.  Every F site forms a candidate with every R site behind it, so a pair has more candidates than the set has
    sequences and pcr_background_match takes the ordered path (k_bg_jobs -> k_sw, the anti-diagonal form) over the same key
    words."""
    buckets = {}
    for c in sc.cases:
        if c.cls == "duplicate" or any(s == c.seq for s, _ in sc.splits):
            continue
        v = value(lib, sc, c.pair, c.seq, 0)
        if v is None or v.n_cand != 1:
            continue
        F, R = sc.pairs[c.pair]
        buckets.setdefault((c.pair, lib.word_and(F, v.keys[0]), lib.word_and(R, v.keys[1])), []).append(c.seq)
    seqs = []
    for key in sorted(buckets):
        b = buckets[key]
        for i in range(0, len(b) - 1, group):
            if len(b[i:i + group]) >= 2:
                seqs.append("".join(sc.seqs[s] for s in b[i:i + group]))
    return Scenario(sc.name + ", stacked", sc.pairs_txt, sc.pairs, seqs, [], [])
