"""The independent expectation for pcr_pool_dimers_end3, and the inputs its tests share.

The geometry (placements, runs, overlaps, flags, the order of the records and the best placement of a cell) is plain Python
over the texts of oracle.word_expand; the floats are oracle.heterodimer_full(tail, stretch, salt, ca, cb) of the run alone,
with pool_dimer_cases.strand_of for the two concentrations (the off-diagonal rule, on the diagonal too) and dG in np.float32.
Every float is held as its bit pattern.  Nothing here touches the library under test.
"""
import functools
import random

import numpy as np

import pool_dimer_cases as PC
from pool_dimer_cases import ASSAY, BITS, HOMO, POOL, PRIMER_STRAND, SALT, Pool, _pairs, _plain
from testdata import rand_seq, revcomp

MUTUAL = 2
PAIRS = {("A", "T"), ("T", "A"), ("C", "G"), ("G", "C")}
T37 = np.float32(310.15)

CELL = np.dtype([("query_oligo", np.uint32), ("target_oligo", np.uint32), ("n_duplexes", np.uint32), ("n_placements", np.uint32),
                 ("q_expansion", np.uint32), ("t_expansion", np.uint32), ("run", np.uint8), ("extension", np.uint8),
                 ("overlap", np.uint8), ("overlap_matches", np.uint8), ("flags", np.uint32), ("dG", np.float32),
                 ("tm", np.float32), ("dH", np.float32), ("dS", np.float32)])
PLACEMENT = np.dtype([("query_oligo", np.uint32), ("target_oligo", np.uint32), ("q_expansion", np.uint32), ("t_expansion", np.uint32),
                      ("run", np.uint8), ("extension", np.uint8), ("overlap", np.uint8), ("overlap_matches", np.uint8),
                      ("flags", np.uint32), ("dG", np.float32), ("tm", np.float32), ("dH", np.float32), ("dS", np.float32)])


def geometry(x, y, min_run, min_extension):
    """The qualifying placements of x on y, j ascending -> [(j, run, overlap, overlap_matches, mutual)]."""
    out = []
    for j in range(len(y)):
        overlap = min(len(x), len(y) - j)
        wc = [(x[len(x) - 1 - k], y[j + k]) in PAIRS for k in range(overlap)]
        run = wc.index(False) if False in wc else overlap
        if run >= min_run and j >= min_extension:
            out.append((j, run, overlap, sum(wc), j + run == len(y)))
    return out


_CACHE = {}


def melt(oracle, x, y, j, run, salt, ca, cb, jobs=None):
    """(dG, tm, dH, dS) bits of the run alone: x's last `run` bases on y[j : j + run]."""
    key = (x[len(x) - run:], y[j:j + run], float(salt), ca, cb)
    if key not in _CACHE:
        _CACHE[key] = np.array(oracle.heterodimer_full(key[0], key[1], salt, ca, cb), np.float32).copy()
    if jobs is not None:
        jobs.add(key)
    tm, dH, dS = (np.float32(v) for v in _CACHE[key][:3])
    dG = np.float32(dH - np.float32(T37 * dS))
    return BITS(dG), BITS(tm), BITS(dH), BITS(dS)


def f32(bits):
    return np.uint32(bits).view(np.float32)


def cell_placements(oracle, P, q, t, rule, min_run, min_extension, salt=SALT, primer_strand=PRIMER_STRAND, jobs=None):
    """Every qualifying placement of cell (q, t) in record order -> (n_duplexes, [placement tuples]), before the dG filter."""
    ca, cb = PC.strand_of(rule, primer_strand, P.degeneracy(q), P.degeneracy(t))
    if q == t:
        duplexes = [(i, i) for i in range(P.degeneracy(q))]
    else:
        duplexes = [(i, k) for i in range(P.degeneracy(q)) for k in range(P.degeneracy(t))]
    out = []
    for qe, te in duplexes:
        x, y = P.exps(q)[qe], P.exps(t)[te]
        for j, run, overlap, matches, mutual in geometry(x, y, min_run, min_extension):
            flags = (HOMO if q == t else 0) | (MUTUAL if mutual else 0)
            out.append((q, t, qe, te, run, j, overlap, matches, flags) + melt(oracle, x, y, j, run, salt, ca, cb, jobs))
    return len(duplexes), out


def best_of(placements):
    """The lowest dG; on a tie the longer run, then the earlier record (the lower duplex, then the lower j)."""
    best = None
    for p in placements:
        dg = f32(p[9])
        if best is None or dg < f32(best[9]) or (dg == f32(best[9]) and p[4] > best[4]):
            best = p
    return best


def expected(oracle, P, rule, min_run, min_extension, dg_max=None, cells=None, **kw):
    """-> (cell records, placement records) as bit tuples, in record order; `cells`: only the listed (q, t), in that order."""
    if cells is None:
        cells = [(q, t) for q in range(P.n) for t in range(P.n)]
    recs, places = [], []
    for q, t in cells:
        nd, pl = cell_placements(oracle, P, q, t, rule, min_run, min_extension, **kw)
        kept = [p for p in pl if dg_max is None or f32(p[9]) <= np.float32(dg_max)]
        if not kept:
            continue
        b = best_of(pl)
        recs.append((q, t, nd, len(pl)) + b[2:])
        places.extend(kept)
    return recs, places


def cells_as_bits(rec):
    return [(int(r["query_oligo"]), int(r["target_oligo"]), int(r["n_duplexes"]), int(r["n_placements"]), int(r["q_expansion"]),
             int(r["t_expansion"]), int(r["run"]), int(r["extension"]), int(r["overlap"]), int(r["overlap_matches"]), int(r["flags"]),
             BITS(r["dG"]), BITS(r["tm"]), BITS(r["dH"]), BITS(r["dS"])) for r in rec]


def places_as_bits(rec):
    return [(int(r["query_oligo"]), int(r["target_oligo"]), int(r["q_expansion"]), int(r["t_expansion"]), int(r["run"]),
             int(r["extension"]), int(r["overlap"]), int(r["overlap_matches"]), int(r["flags"]),
             BITS(r["dG"]), BITS(r["tm"]), BITS(r["dH"]), BITS(r["dS"])) for r in rec]


def two_lowest_equal(placements):
    dgs = sorted(float(f32(p[9])) for p in placements)
    return len(dgs) >= 2 and dgs[0] == dgs[1]


# ---------------------------------------------------------------------------------------------------------------- scenarios
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
PLANTED_R = (3, 4, 5, 8, 12, 20, 22)
PLANTED_E = (0, 1, 5)


def _breaker(rng, query, r):
    """A base that does not pair with the query base next to the planted run (any base where the run is the whole query)."""
    if r >= len(query):
        return rng.choice("ACGT")
    return rng.choice([b for b in "ACGT" if b != COMP[query[len(query) - 1 - r]]])


def _planted_texts():
    rng = random.Random(5301)
    query = _plain(rng, 22)
    texts, where = [query], {}
    for r in PLANTED_R:
        stretch = revcomp(query[len(query) - r:])
        for e in PLANTED_E:
            tail = rand_seq(rng, max(2, min(8, 31 - e - r - 1))) if e + r + 1 < 32 else ""
            where[(r, e)] = len(texts)
            texts.append(rand_seq(rng, e) + stretch + _breaker(rng, query, r) + tail)
        where[(r, "mutual")] = len(texts)
        texts.append(rand_seq(rng, 2) + stretch)                            # the run ends the target
    assert len(set(texts)) == len(texts) and all(len(s) <= 32 for s in texts)
    return texts, where


@functools.lru_cache(None)
def planted_pool(oracle):
    """1. A 22-mer query (oligo 0) and, per run length r, targets with the reverse complement of its last r bases at offset
    e = 0, 1, 5, a base that breaks the run and a random tail, and one target that ends with the stretch.
    -> (pool, {(r, e) or (r, "mutual"): oligo id})."""
    texts, where = _planted_texts()
    return _pairs(oracle, texts), where


@functools.lru_cache(None)
def limits_pool(oracle):
    """2. Oligo 0 with a target (oligo 1) that carries the reverse complement of its last 2 bases only at offset 3, and two
    32-mers (oligos 2, 3) that are each other's reverse complement."""
    rng = random.Random(5302)
    query = "GATCTGACTTCAGGCATTCAAC"
    short = "TCA" + revcomp(query[-2:]) + "C" + "CCATACAT"                   # ..GT T | G: the third pair fails
    long = _plain(rng, 32)
    return _pairs(oracle, [query, short, long, revcomp(long)])


EXP_Q3 = "CAGTTGACCATGCTAGGTCR"          # D = 2: the 3' base itself is degenerate
EXP_TN = "TTAGCYGNCCTAGCAAGT"            # D = 8: Y faces the R at offset 5, then GNCCTAG, where only N = A goes on pairing


@functools.lru_cache(None)
def expansions_pool(oracle):
    """3. pool_dimer_cases' degenerate 20-mers, a query whose 3' base is R and a target with Y opposite it and N inside the
    stretch: some duplexes of the cell have the run, some break at once, some after two pairs."""
    return _pairs(oracle, [PC.EXP_A, PC.EXP_B, PC.EXP_C, PC.EXP_P, EXP_Q3, EXP_TN])


@functools.lru_cache(None)
def self_priming_pool(oracle):
    """4. An oligo that ends in the palindrome GAATTC, and a plain partner."""
    return _pairs(oracle, ["ACTGACCTGATCAGGAATTC", "CAGGTTCAGCATCGATTACG"])


@functools.lru_cache(None)
def twice_pool(oracle):
    """5a. A target with the query's anchored 5-base stretch at two places, each followed by a base that breaks the run."""
    query = "GATCTGACTTCAGGCATTCAAC"
    stretch = revcomp(query[-5:])                                          # GTTGA; the next query base is T: anything but A breaks
    return _pairs(oracle, [query, "CC" + stretch + "CTC" + stretch + "GCA"])


@functools.lru_cache(None)
def random_pool(oracle):
    """5b. The 40 random oligos of 18 .. 25 bases the tie rule is pinned on."""
    rng = random.Random(5201)
    return _pairs(oracle, ["".join(rng.choice("ACGT") for _ in range(rng.randint(18, 25))) for _ in range(40)])


RANDOM_COUNTS = (488, 406, 39, 21)       # placements, cells, cells whose two lowest dG are equal, MUTUAL placements


def random_counts(oracle, rule=POOL):
    P = Pool(oracle, random_pool(oracle))
    recs, places = expected(oracle, P, rule, 3, 1)
    ties = 0
    for r in recs:
        ties += two_lowest_equal(cell_placements(oracle, P, r[0], r[1], rule, 3, 1)[1])
    return len(places), len(recs), ties, sum(1 for p in places if p[8] & MUTUAL)


def checked(oracle, name):
    """(pool, rule, min_run, min_extension) of the scenarios whose every melted run tests/test_dimer_end3_host.py holds to
    the reference."""
    return {
        "planted": (planted_pool(oracle)[0], POOL, 3, 0),
        "limits": (limits_pool(oracle), POOL, 3, 0),
        "lengths": (PC.lengths_pool(oracle), ASSAY, 3, 0),
        "expansions_assay": (expansions_pool(oracle), ASSAY, 3, 0),
        "expansions_pool": (expansions_pool(oracle), POOL, 3, 0),
        "self_priming": (self_priming_pool(oracle), ASSAY, 3, 0),
        "twice": (twice_pool(oracle), POOL, 3, 1),
        "random_pool": (random_pool(oracle), POOL, 3, 1),
        "random_assay": (random_pool(oracle), ASSAY, 3, 1),
    }[name]


SCENARIO_NAMES = ("planted", "limits", "lengths", "expansions_assay", "expansions_pool", "self_priming", "twice", "random_pool",
                  "random_assay")
