"""Inputs at the edges of the thermodynamics kernel's input space, shared by tests/test_thermo_cases_host.py (oracle against the
reference) and tests/test_gpu_thermo_edges.py (kernel against the oracle): oligos of every length from 1 and at the full 32,
dimers of full and lopsided sizes, and degenerate words at either end of the 32-slot word.

Everything is a pure function of fixed seeds (the reference tape replays the host tests call by call).  Nothing here touches
the library under test or the oracle; the coverage conditions on what these inputs reach are asserted by the host tests.
"""
import functools
import itertools
import random

from pcramp_amd import words as W
from testdata import mutate, rand_seq, revcomp

SHORT_LENGTHS = tuple(range(1, 12))          # below anything the rest of the suite runs
FULL_LENGTHS = (31, 32)
PER_LENGTH = 150
# (len(a), len(b)) of dimer_pairs()
DIMER_LENGTHS = ((1, 1), (1, 32), (32, 1), (2, 32), (3, 31), (4, 32), (8, 32), (32, 8), (32, 32), (31, 32), (32, 31), (12, 32),
                 (5, 5), (6, 7))
PER_DIMER = 40
DEGENERATE_LENGTHS = (5, 8, 12, 20, 31, 32)
# salts and strand concentrations the host tests rotate through
SALTS = (0.05, 0.01, 1.0)
STRANDS = (9e-7, 2e-8)
_EXPANSION = {1: "A", 2: "C", 4: "G", 8: "T"}


def _mixed(rng, n, k):
    """The k-th oligo of the mix at length n: homopolymers, (GC)n, (AT)n, a half with its reverse complement (back to back:
    self-complementary; around a short loop: a hairpin), random."""
    if k < 4:
        return "ACGT"[k] * n
    if k < 8:
        return (("GC", "CG", "AT", "TA")[k - 4] * n)[:n]
    if k < 40:
        if k % 2 == 0 or n < 8:                                          # self-complementary, the middle base free at odd n
            half = rand_seq(rng, n // 2)
            return half + rand_seq(rng, n % 2) + revcomp(half)
        loop = min(3 + k % 3, n - 4)                                     # stem + loop + stem', the rest random at the 3' end
        stem = rand_seq(rng, max(2, min((n - loop) // 2, 3 + k % 5)))
        s = stem + rand_seq(rng, loop) + mutate(rng, revcomp(stem), 0.05)
        return (s + rand_seq(rng, n))[:n]
    if k < 60:                                                           # GC-rich random: a Tm above zero at the short lengths
        return "".join(rng.choice("GGCCAT") for _ in range(n))
    return rand_seq(rng, n)


@functools.lru_cache(maxsize=None)
def short_oligos():
    """-> tuple of oligo texts: every oligo of 1..4 nt, PER_LENGTH each at 5..11 nt and at 31 and 32 nt."""
    out = []
    for n in range(1, 5):
        out.extend("".join(p) for p in itertools.product("ACGT", repeat=n))
    rng = random.Random(7101)
    for n in tuple(range(5, 12)) + FULL_LENGTHS:
        seen = set()
        k = 0
        while len(seen) < PER_LENGTH:
            s = _mixed(rng, n, k)
            k += 1
            if s not in seen:
                seen.add(s)
                out.append(s)
    return tuple(out)


def _fit(rng, core, n, where):
    """core trimmed or extended to n bases; where = 0 / 1 / 2: the core (or the window kept of it) sits at the 5' end, in the
    middle, at the 3' end -- the partner dangles on the other side(s)."""
    if len(core) >= n:
        off = (0, (len(core) - n) // 2, len(core) - n)[where]
        return core[off:off + n]
    pad = n - len(core)
    left = (0, pad // 2, pad)[where]
    return rand_seq(rng, left) + core + rand_seq(rng, pad - left)


@functools.lru_cache(maxsize=None)
def dimer_pairs():
    """-> tuple of (a, b) texts, PER_DIMER per entry of DIMER_LENGTHS: random partners, and partners built from the (mutated)
    reverse complement of the other oligo, trimmed or extended to the stated length with the complementary stretch at either
    end or in the middle.  At (32, 32) also exact reverse complements and self-complementary 32-mers."""
    out = []
    rng = random.Random(7102)
    for la, lb in DIMER_LENGTHS:
        for k in range(PER_DIMER):
            gc = k % 4 == 1
            a = "".join(rng.choice("GGCCAT") for _ in range(la)) if gc else rand_seq(rng, la)
            if (la, lb) == (32, 32) and k < 6:
                if k < 3:
                    b = revcomp(a)                                       # the full 32 x 32 duplex: every column, every row
                else:
                    half = rand_seq(rng, 16)
                    a = half + revcomp(half)
                    b = a if k < 5 else mutate(rng, a, 0.06)
            elif k % 5 == 4:
                b = rand_seq(rng, lb)
            else:
                rate = (0.0, 0.04, 0.08, 0.15)[k % 4]
                rc = mutate(rng, revcomp(a), rate)
                if len(rc) > 12 and k % 7 == 3:                          # frayed: a wrong base next to the end of the stretch
                    rc = mutate(rng, rc[:2], 1.0) + rc[2:]
                b = _fit(rng, rc, lb, k % 3)
            assert len(a) == la and len(b) == lb
            out.append((a, b))
    return tuple(out)


def word_at(text, first):
    """The oligo's IUPAC text as a word whose first base sits in slot `first`."""
    codes = W.codes_from_text(text)
    assert 0 <= first and first + len(codes) <= 32
    slots = [0] * 32
    slots[first:first + len(codes)] = [int(c) for c in codes]
    return W.word_from_slots(slots)


def positions(n):
    """Where the tests put an n-base oligo in the 32 slots: centred (as assays are stored), lowest slots, highest slots."""
    out = []
    for first in ((33 - n) // 2, 0, 32 - n):
        if first not in out:
            out.append(first)
    return out


def _plant(s, where):
    s = list(s)
    for k, c in where:
        s[k] = c
    return "".join(s)


@functools.lru_cache(maxsize=None)
def degenerate_texts():
    """-> tuple of IUPAC texts: per length of DEGENERATE_LENGTHS two random oligos, each with codes planted in the first slot
    only, the last only, first and last, two adjacent middle slots (3-fold beside 2-fold) and N at first, middle and last;
    and one 24-mer with six N (4 096 expansions)."""
    rng = random.Random(7103)
    out = []
    for n in DEGENERATE_LENGTHS:
        for rep in range(2):
            s = rand_seq(rng, n)
            m = n // 2
            out.append(_plant(s, [(0, "RYKM"[(n + rep) % 4])]))
            out.append(_plant(s, [(n - 1, "HDVB"[(n + rep) % 4])]))
            out.append(_plant(s, [(0, "S"), (n - 1, "N")]))
            out.append(_plant(s, [(m - 1, "B"), (m, "W")]))
            out.append(_plant(s, [(0, "N"), (m, "N"), (n - 1, "N")]))
    s = rand_seq(rng, 24)
    out.append(_plant(s, [(k, "N") for k in (0, 1, 11, 12, 22, 23)]))
    return tuple(out)


BIG_TEXT_DEGENERACY = 4096


@functools.lru_cache(maxsize=None)
def degenerate_words():
    """-> tuple of (w0, w1): every text of degenerate_texts() at every slot position of positions()."""
    out = []
    for s in degenerate_texts():
        for first in positions(len(s)):
            out.append(word_at(s, first))
    return tuple(out)


def degeneracy(text):
    d = 1
    for c in W.codes_from_text(text):
        d *= bin(int(c)).count("1")
    return d


def expand(text):
    """Every expansion of an IUPAC text, the textbook way: leftmost position slowest, A < C < G < T.  (Independent of the
    order in which the kernel, the host library or the reference walk them.)"""
    sets = [[_EXPANSION[b] for b in (1, 2, 4, 8) if int(c) & b] for c in W.codes_from_text(text)]
    return ["".join(p) for p in itertools.product(*sets)]


@functools.lru_cache(maxsize=None)
def unequal_pairs():
    """-> tuple of (F word, R word) whose degeneracies differ (1 x 4, 4 x 1, 2 x 3, 3 x 2): the dimer's strand term is
    ca > cb ? ca - cb/2 : cb - ca/2.  R is built from F's reverse complement so that most pairs melt above zero."""
    rng = random.Random(7104)
    out = []
    plans = (("", "N"), ("N", ""), ("R", "H"), ("B", "Y"), ("", "KM"), ("SW", ""))
    for k in range(48):
        cf, cr = plans[k % len(plans)]
        f = rand_seq(rng, rng.randint(18, 25))
        r = _fit(rng, mutate(rng, revcomp(f[2:16]), 0.05), rng.randint(18, 25), k % 3)
        for c in cf:
            f = _plant(f, [(rng.randrange(len(f)), c)])
        for c in cr:
            r = _plant(r, [(rng.randrange(len(r)), c)])
        if len(cf) == 2 and degeneracy(f) != 4 or len(cr) == 2 and degeneracy(r) != 4:   # both codes on one slot
            continue
        out.append((word_at(f, (33 - len(f)) // 2), word_at(r, (33 - len(r)) // 2)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def threshold_candidates():
    """-> tuple of 18..25 nt oligo texts likely to have a duplex, a hairpin and a homodimer Tm above zero at once (the tests
    keep those that do): a stem, a loop, the stem's reverse complement and a self-complementary tail."""
    rng = random.Random(7105)
    out = []
    for k in range(1500):
        n = rng.randint(18, 25)
        stem = "".join(rng.choice("GGCCAT") for _ in range(rng.randint(4, 6)))
        tail = "".join(rng.choice("GCGCAT") for _ in range(3))
        s = stem + rand_seq(rng, rng.randint(3, 5)) + revcomp(stem) + tail + revcomp(tail) + rand_seq(rng, 8)
        out.append(s[:n])
    return tuple(out)
