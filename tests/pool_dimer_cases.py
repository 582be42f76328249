"""The independent expectation for pcr_pool_dimers, and the inputs its tests share.

expected_cell() restates the call's definition (include/pcramp_hip.h) from oracle.word_expand, oracle.heterodimer_full (off
the diagonal; it applies NucCruc's two-concentration rule itself) and oracle.thermo_full (the homodimer, on the diagonal).
Nothing here touches the library under test.
"""
import functools
import random

import numpy as np

from site_tm_cases import distinct_oligos, slots_of, spell
from testdata import rand_seq, revcomp

DIMER = np.dtype([("query_oligo", np.uint32), ("target_oligo", np.uint32), ("n_duplexes", np.uint32),
                  ("q_expansion", np.uint32), ("t_expansion", np.uint32), ("flags", np.uint32),
                  ("tm_max", np.float32), ("tm_min", np.float32), ("dH", np.float32), ("dS", np.float32)])
HOMO = 1
POOL, ASSAY = 0, 1
SALT, PRIMER_STRAND = 0.05, 9e-7
BITS = lambda x: int(np.float32(x).view(np.uint32))


class Pool:
    """A pool's distinct oligos as the expectation needs them: ids, words, expansions in oracle.word_expand order."""

    def __init__(self, oracle, pool):
        self.pool = list(pool)
        self.ids, self.words = distinct_oligos(self.pool)
        self.n = len(self.words)
        self._oracle, self._exps = oracle, {}

    def exps(self, k):
        if k not in self._exps:
            e = [spell(slots_of(x)) for x in self._oracle.word_expand(self.words[k])]
            assert len(e) == int(self._oracle.word_degeneracy(self.words[k]))
            self._exps[k] = e
        return self._exps[k]

    def degeneracy(self, k):
        return len(self.exps(k))


def strand_of(rule, primer_strand, dq, dt=None):
    """-> (strand_a, strand_b) for oracle.heterodimer_full, or the one strand of the homodimer where dt is None."""
    ps = float(np.float32(primer_strand))
    if rule == POOL:                                                     # pcr_assay.cpp:819-821: no degeneracy correction
        return ps if dt is None else (ps, 0.0)
    ca = float(np.float32(ps / dq))                                      # pcr_assay.cpp:244, valid_pcr.cpp:13
    return ca if dt is None else (ca, float(np.float32(ps / dt)))


_CACHE = {}


def duplexes_of(oracle, P, q, t, rule, salt=SALT, primer_strand=PRIMER_STRAND, jobs=None):
    """The (tm, dH, dS) of every duplex of cell (q, t) in job order (query expansion outer)."""
    out = []
    if q == t:
        s = strand_of(rule, primer_strand, P.degeneracy(q))
        for x in P.exps(q):
            key = ("homo", x, salt, s)
            if key not in _CACHE:
                _CACHE[key] = oracle.thermo_full(x, salt, s)[7:10].copy()
            if jobs is not None:
                jobs.add(key)
            out.append(_CACHE[key])
        return out
    ca, cb = strand_of(rule, primer_strand, P.degeneracy(q), P.degeneracy(t))
    for x in P.exps(q):
        for y in P.exps(t):
            key = ("hetero", x, y, salt, ca, cb)
            if key not in _CACHE:
                _CACHE[key] = oracle.heterodimer_full(x, y, salt, ca, cb)
            if jobs is not None:
                jobs.add(key)
            out.append(_CACHE[key])
    return out


def expected_cell(oracle, P, q, t, rule, **kw):
    """One cell as a tuple with every float as its bit pattern (as_bits' form)."""
    res = duplexes_of(oracle, P, q, t, rule, **kw)
    tms = [r[0] for r in res]
    best = max(range(len(res)), key=lambda k: (tms[k], -k))             # the highest Tm, the lowest index on a tie
    dt = P.degeneracy(t)
    qe, te = (best, best) if q == t else (best // dt, best % dt)
    return (q, t, len(res), qe, te, HOMO if q == t else 0, BITS(tms[best]), BITS(min(tms)), BITS(res[best][1]), BITS(res[best][2]))


def expected_cells(oracle, P, rule, cells=None, **kw):
    """All cells in row-major order (or the listed (q, t)) -> list of bit tuples."""
    if cells is None:
        cells = [(q, t) for q in range(P.n) for t in range(P.n)]
    return [expected_cell(oracle, P, q, t, rule, **kw) for q, t in cells]


def as_bits(rec):
    return [(int(r["query_oligo"]), int(r["target_oligo"]), int(r["n_duplexes"]), int(r["q_expansion"]), int(r["t_expansion"]),
             int(r["flags"]), BITS(r["tm_max"]), BITS(r["tm_min"]), BITS(r["dH"]), BITS(r["dS"])) for r in rec]


def jobs_before(D, q, t):
    """Duplexes before cell (q, t) in the whole matrix: D = the degeneracies."""
    S = sum(D)
    row = sum(D[r] * (S - D[r]) + D[r] for r in range(q))
    return row + sum((D[q] if u == q else D[q] * D[u]) for u in range(t))


def batch_starts(D, limit):
    """The first cell of every batch: a batch is a run of consecutive whole cells and closes before the cell that would take
    it past `limit` duplexes (include/pcramp_hip.h has no word on batches: they are the implementation's)."""
    n = len(D)
    starts, count = [0], 0
    for c in range(n * n):
        q, t = divmod(c, n)
        jobs = D[q] if q == t else D[q] * D[t]
        if count and count + jobs > limit:
            starts.append(c)
            count = 0
        count += jobs
    return starts


# ---------------------------------------------------------------------------------------------------------------- scenarios
def _plain(rng, n):
    while True:
        s = rand_seq(rng, n)
        if n < 4 or all(s[j:j + 4] != s[j] * 4 for j in range(n - 3)):
            return s


def _pairs(oracle, texts):
    """Oligo texts -> pool pairs (F, R), (F, R), ...; an odd one out is paired with the first oligo again."""
    w = [oracle.centered_word(s) for s in texts]
    if len(w) % 2:
        w.append(w[0])
    return [(w[i], w[i + 1]) for i in range(0, len(w), 2)]


LENGTHS = (1, 2, 3, 4, 5, 18, 25, 31, 32)


@functools.lru_cache(None)
def lengths_pool(oracle):
    """1. Plain oligos of every length class; 9 distinct oligos (the tenth slot repeats the first)."""
    rng = random.Random(5101)
    return _pairs(oracle, [_plain(rng, n) for n in LENGTHS])


@functools.lru_cache(None)
def self_pair_pool(oracle):
    rng = random.Random(5102)
    w = oracle.centered_word(_plain(rng, 21))
    return [(w, w)]


@functools.lru_cache(None)
def order_pool(oracle):
    """2. 40 random plain oligos of 18 .. 25 bases; three of them carry the reverse complement of a stretch of another, so
    that some cells melt above 0 C."""
    rng = random.Random(5103)
    txt = [_plain(rng, rng.randint(18, 25)) for _ in range(40)]
    for a, b in ((3, 17), (8, 30), (21, 22)):
        txt[b] = revcomp(txt[a][2:16]) + txt[b][14:]
    return _pairs(oracle, txt)


EXP_A = "ACRTGCATGGCTAGCHTAGC"          # D = 6: a two-fold slot below slot 16, a three-fold slot above
EXP_B = "TGCNATCGGATCCGTAABCG"          # D = 12: four-fold below, three-fold above
EXP_C = "GRTCAGTCANGGCTTAGCDA"          # D = 24: 2 x 4 x 3
EXP_P = "CAGGTTCAGCATCGATTACG"          # plain


@functools.lru_cache(None)
def expansions_pool(oracle):
    """3. Degenerate slots on both sides of slot 16 (the centred 20-mers occupy slots 6 .. 25), radices 2, 3 and 4 mixed:
    D = 6 against D = 12 (every one of its 72 duplexes melts below 0 C and is clamped to Tm 0, with dH that differ), 24 x 1
    and 1 x 24, and the diagonals of degenerate oligos."""
    return _pairs(oracle, [EXP_A, EXP_B, EXP_C, EXP_P])


@functools.lru_cache(None)
def largest_pool(oracle):
    """4. A 256-expansion oligo against a 128-expansion oligo: two cells of 32 768 duplexes and two diagonals."""
    return _pairs(oracle, ["ACGTNNNNACGTACGTACG", "TGCANNNRTGACTGACTGA"])


def _widen2(rng, s):
    """Up to 2 two-fold degenerate bases."""
    out = list(s)
    for p in rng.sample(range(len(s)), rng.randint(0, 2)):
        out[p] = "R" if out[p] in "AG" else "Y"
    return "".join(out)


@functools.lru_cache(None)
def rules_pool(oracle):
    """5. 30 random assays, up to 2 degenerate bases per oligo; every third reverse oligo carries the reverse complement of
    a stretch of its forward oligo, so that max_dimer_tm is above 0 C for some."""
    rng = random.Random(5105)
    pool = []
    for k in range(30):
        f, r = _plain(rng, rng.randint(18, 25)), _plain(rng, rng.randint(18, 25))
        if k % 3 == 0:
            r = revcomp(f[3:3 + rng.randint(8, 14)]) + r[12:]
        pool.append((oracle.centered_word(_widen2(rng, f)), oracle.centered_word(_widen2(rng, r))))
    return pool


RULES_PAIRS = [(a, (7 * a + 3) % 30) for a in range(30)]    # 30 assay pairs (a, b), a != b


@functools.lru_cache(None)
def floor_pool(oracle):
    """6. 12 oligos cut from both strands of one GC-rich 30-mer: most cells melt above 0 C, so the median tm_max is positive."""
    rng = random.Random(5106)
    s = "GCGGCCATGGCGCGCCATGGCCGCTAGCGC"
    txt = []
    while len(txt) < 12:
        n = rng.randint(18, 24)
        at = rng.randint(0, len(s) - n)
        cut = s[at:at + n]
        cut = revcomp(cut) if len(txt) % 2 else cut
        if cut not in txt:
            txt.append(cut)
    return _pairs(oracle, txt)


@functools.lru_cache(None)
def stride_pool(oracle):
    """7a. 64 plain oligos: 4 096 cells, more duplexes than a grid of one 12-wave block per CU takes in one stride."""
    rng = random.Random(5107)
    txt = set()
    while len(txt) < 64:
        txt.add(_plain(rng, rng.randint(18, 25)))
    return _pairs(oracle, sorted(txt))


@functools.lru_cache(None)
def batches_pool(oracle, limit):
    """7b. Oligos of 2, 3, 4 and 6 expansions, as many as it takes for the matrix to hold more than 2.3 x limit duplexes:
    at least two batch boundaries, every cell of several duplexes."""
    rng = random.Random(5108)
    codes = {2: ("R",), 3: ("H",), 4: ("R", "Y"), 6: ("R", "B")}
    txt, D = [], []
    while sum(D) ** 2 <= 2.3 * limit or len(txt) % 2:
        s = list(_plain(rng, rng.randint(18, 22)))
        d = (2, 3, 4, 6)[len(txt) % 4]
        for p, code in zip(rng.sample(range(len(s)), len(codes[d])), codes[d]):
            s[p] = {"R": "R" if s[p] in "AG" else "Y", "Y": "Y" if s[p] in "CT" else "R", "H": "H" if s[p] != "G" else "B",
                    "B": "B" if s[p] != "A" else "H"}[code]
        s = "".join(s)
        if s not in txt:
            txt.append(s)
            D.append(d)
    return _pairs(oracle, txt)


@functools.lru_cache(None)
def full_pool(oracle):
    """8. 1 024 pairs of distinct plain oligos."""
    rng = random.Random(5109)
    txt, seen = [], set()
    while len(txt) < 2048:
        s = rand_seq(rng, rng.randint(18, 25))
        if s not in seen:
            seen.add(s)
            txt.append(s)
    return _pairs(oracle, txt)


def checked_cells(oracle, name):
    """(pool, rule, the cells the GPU test of that name compares with the oracle duplex by duplex; None: all)."""
    if name in ("lengths_assay", "lengths_pool"):
        return lengths_pool(oracle), ASSAY if name.endswith("assay") else POOL, None
    if name == "self_pair":
        return self_pair_pool(oracle), ASSAY, None
    if name == "order":
        return order_pool(oracle), ASSAY, None
    if name in ("expansions_assay", "expansions_pool"):
        return expansions_pool(oracle), ASSAY if name.endswith("assay") else POOL, None
    if name == "rules_assay":
        P = Pool(oracle, rules_pool(oracle))
        return rules_pool(oracle), ASSAY, [(P.ids[2 * k], P.ids[2 * k + 1]) for k in range(30)]
    if name == "rules_pool":
        P = Pool(oracle, rules_pool(oracle))
        cells = [(P.ids[2 * a + i], P.ids[2 * b + j]) for a, b in RULES_PAIRS for i in (0, 1) for j in (0, 1)]
        return rules_pool(oracle), POOL, cells
    if name == "floor":
        return floor_pool(oracle), ASSAY, None
    raise KeyError(name)


# the scenarios whose every checked duplex tests/test_pool_dimers_host.py holds to the reference (a few thousand duplexes)
SCENARIO_NAMES = ("lengths_assay", "lengths_pool", "self_pair", "order", "expansions_assay", "expansions_pool", "rules_assay",
                  "rules_pool", "floor")
