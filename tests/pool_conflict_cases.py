"""The independent expectation for pcr_pool_conflicts, and the inputs its tests share.

The product records are products_tm_cases.all_products (the oracle's products with the oracle's Tm), the dimer cells
pool_dimer_cases.expected_cells (the oracle's duplexes).  The reduction to unordered pairs of pool rows is the definition of
include/pcramp_hip.h restated with dictionaries and sets.  Nothing here touches the library under test.
"""
import functools
import random

import numpy as np

import pool_dimer_cases as DC
import products_tm_cases as PC
import site_tm_cases as SC
from select_sites_cases import plant
from site_tm_cases import _primer, _sub
from testdata import family_targets, rand_seq, revcomp, sample_pair

NO_PRODUCT_BITS = int(np.float32(-1.0).view(np.uint32))
PRODUCT, DIMER = 1, 2
NO_DIMERS = -1
BITS = DC.BITS
F32 = lambda bits: np.array([bits], np.uint32).view(np.float32)[0]


def rows_of(ids):
    """oligo id -> the sorted pool rows it is an oligo of (a row with F = R once)."""
    out = {}
    for i in range(len(ids) // 2):
        for o in {ids[2 * i], ids[2 * i + 1]}:
            out.setdefault(int(o), []).append(i)
    return out


def melt_value(r):
    """v = min(tm_plus, tm_minus) + 0.0f, as float32."""
    return np.float32(min(np.float32(r["tm_plus"]), np.float32(r["tm_minus"])) + np.float32(0.0))


def spurious_kept(rec, tm_floor):
    """The records that take part: intended = 0 and kept at the floor (!(tm_floor > 0) || v >= tm_floor)."""
    f = np.float32(tm_floor)
    return [r for r in rec if not r["intended"] and (not (f > 0) or melt_value(r) >= f)]


def cells_of_product(rows, x, y):
    """The set of unordered row pairs a product of (plus x, minus y) belongs to."""
    return {(min(i, j), max(i, j)) for i in rows.get(int(x), ()) for j in rows.get(int(y), ())}


def product_cells(ids, rec, tm_floor):
    """(a, b) -> dict(products, sequences, melt_bits, melt_sequence) over the cells that have a product."""
    rows = rows_of(ids)
    acc = {}
    for r in spurious_kept(rec, tm_floor):
        v, s = melt_value(r), int(r["sequence"])
        for cell in cells_of_product(rows, r["plus_oligo"], r["minus_oligo"]):
            c = acc.setdefault(cell, dict(products=0, seqs=set(), best=None))
            c["products"] += 1
            c["seqs"].add(s)
            if c["best"] is None or v > c["best"][0] or (v == c["best"][0] and s < c["best"][1]):
                c["best"] = (v, s)
    return {cell: dict(products=c["products"], sequences=len(c["seqs"]), melt_bits=BITS(c["best"][0]), melt_sequence=c["best"][1])
            for cell, c in acc.items()}


def product_cells_brute(ids, rec, tm_floor):
    """The same by the definition read literally: every (product, row, row) triple is asked the membership question."""
    n_pool = len(ids) // 2
    O = [{int(ids[2 * i]), int(ids[2 * i + 1])} for i in range(n_pool)]
    acc = {}
    for r in spurious_kept(rec, tm_floor):
        x, y, s, v = int(r["plus_oligo"]), int(r["minus_oligo"]), int(r["sequence"]), melt_value(r)
        near = [i for i in range(n_pool) if x in O[i] or y in O[i]]         # (a row with neither oligo is in no pair that holds)
        for i in near:
            for j in near:
                if i <= j and ((x in O[i] and y in O[j]) or (x in O[j] and y in O[i])):
                    acc.setdefault((i, j), []).append((v, s))
    out = {}
    for cell, items in acc.items():
        top = max(v for v, _ in items)
        out[cell] = dict(products=len(items), sequences=len({s for _, s in items}), melt_bits=BITS(top),
                         melt_sequence=min(s for v, s in items if v == top))
    return out


def dimer_cells_of(ids, a, b):
    """The ordered pcr_pool_dimers cells (q, t) of the row pair {a, b}, sorted."""
    Oa, Ob = {int(ids[2 * a]), int(ids[2 * a + 1])}, {int(ids[2 * b]), int(ids[2 * b + 1])}
    return sorted({(q, t) for q in Oa for t in Ob} | {(q, t) for q in Ob for t in Oa})


def best_dimer(cells, tm_of):
    """(tm bits, q, t): the highest tm_max over the sorted cells, the lowest (q, t) on a tie.  tm_of(q, t) -> bits."""
    best = None
    for q, t in cells:
        bits = tm_of(q, t)
        if best is None or F32(bits) > F32(best[0]):
            best = (bits, q, t)
    return best


@functools.lru_cache(None)
def _dimer_matrix(oracle, pool, rule, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND):
    P = DC.Pool(oracle, list(pool))
    cells = DC.expected_cells(oracle, P, rule, salt=salt, primer_strand=primer_strand)
    return P.ids, {(c[0], c[1]): c[6] for c in cells}


def expected(oracle, name, tm_floor=0.0, rule=NO_DIMERS, dimer_floor=0.0, pool=None, rec=None, ids=None):
    """-> (oligo_id list, the records as tuples of eleven integers: every field, the floats as their bit patterns)."""
    cond = SC.conditions_of({})
    if rec is None:
        ids, rec, _, _ = PC.all_products(oracle, name)
        pool = PC.scenario(oracle, name)["panel"]
        cond = SC.conditions_of(PC.scenario(oracle, name))
    n_pool = len(ids) // 2
    prod = product_cells(ids, rec, tm_floor)
    dimers = rule != NO_DIMERS
    tm = None
    if dimers:
        d_ids, tm = _dimer_matrix(oracle, tuple(pool), rule, cond["salt"], cond["primer_strand"])
        assert list(d_ids) == list(ids)
    out = []
    fl = np.float32(dimer_floor)
    for a in range(n_pool):
        for b in range(a, n_pool):
            p = prod.get((a, b))
            row = [a, b, 0, 0, NO_PRODUCT_BITS, 0, 0, 0, 0, 0, 0]
            keep = False
            if p:
                row[2:6] = [p["products"], p["sequences"], p["melt_bits"], p["melt_sequence"]]
                row[9] |= PRODUCT
                keep = True
            if dimers:
                bits, q, t = best_dimer(dimer_cells_of(ids, a, b), lambda q, t: tm[(q, t)])
                row[6:9] = [bits, q, t]
                if F32(bits) >= fl:
                    row[9] |= DIMER
                if not (fl > 0) or F32(bits) >= fl:
                    keep = True
            if keep:
                out.append(tuple(row))
    return list(ids), out


FIELDS = ("row_a", "row_b", "products", "sequences", "melt", "melt_sequence", "dimer_tm", "dimer_query", "dimer_target", "flags",
          "reserved")


def as_bits(rec):
    """Device records -> the tuples expected() gives."""
    out = []
    for r in rec:
        out.append((int(r["row_a"]), int(r["row_b"]), int(r["products"]), int(r["sequences"]), BITS(r["melt"]), int(r["melt_sequence"]),
                    BITS(r["dimer_tm"]), int(r["dimer_query"]), int(r["dimer_target"]), int(r["flags"]), int(r["reserved"])))
    return out


def floors_of(rec):
    """products_tm_cases.floors_of; for a scenario without a product above 0 C the floors anneal_profile_cases takes then."""
    if not (PC.min_tm(rec) > 0).any():
        return [-10.0, 0.0, 1e-3, 55.0]
    return PC.floors_of(rec)


def attributions(ids, rec, tm_floor=0.0):
    rows = rows_of(ids)
    return sum(len(cells_of_product(rows, r["plus_oligo"], r["minus_oligo"])) for r in spurious_kept(rec, tm_floor))


# ---------------------------------------------------------------------------------------------------------------- scenarios
# products_tm_cases' format.  a .. d are four plain primers; a product of (plus p, minus m) is p planted at `at` and the reverse
# complement of m planted 120 bases on.

def _seq(rng, n, products):
    """A random sequence of n bases with the listed (at, plus text, minus text) products planted."""
    s = rand_seq(rng, n)
    for at, p, m in products:
        s = plant(s, at, p)
        s = plant(s, at + 120, revcomp(m))
    return s


def _four(seed):
    rng = random.Random(seed)
    return (rng,) + tuple(_primer(rng, n) for n in (20, 21, 22, 20))


@functools.lru_cache(None)
def shared_case(oracle):
    """Rows (A, B), (A, C).  An A-A product (cells {0,0}, {0,1}, {1,1}, once each), a B-plus / C-minus product (cell {0,1}),
    and A-plus / C-minus, which is row 1's own product and takes no part."""
    rng, a, b, c, d = _four(6101)
    seqs = [_seq(rng, 400, [(40, a, a)]), _seq(rng, 400, [(60, b, c)]), _seq(rng, 400, [(50, a, c)])]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(a), w(b)), (w(a), w(c))], thr=0.95, select="all")


@functools.lru_cache(None)
def roles_case(oracle):
    """Rows (A, B), (C, A): A is F in one row and R in the other.  An A-A product and a B-plus / C-minus product."""
    rng, a, b, c, d = _four(6102)
    seqs = [_seq(rng, 400, [(40, a, a)]), _seq(rng, 400, [(60, b, c)])]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(a), w(b)), (w(c), w(a))], thr=0.95, select="all")


@functools.lru_cache(None)
def repeat_case(oracle):
    """Rows (A, B), (A, B) again, (B, A), (C, D): an A-plus / C-minus product belongs to {0,3}, {1,3}, {2,3}; an A-A product to
    all six pairs of rows 0 .. 2; A-plus / B-minus is every one of these rows' own."""
    rng, a, b, c, d = _four(6103)
    seqs = [_seq(rng, 400, [(40, a, c)]), _seq(rng, 400, [(60, a, a)]), _seq(rng, 400, [(50, a, b)])]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(a), w(b)), (w(a), w(b)), (w(b), w(a)), (w(c), w(d))], thr=0.95, select="all")


@functools.lru_cache(None)
def self_pair_case(oracle):
    """Rows (C, C), (A, B): a C-C product is row 0's own; A-plus / C-minus and C-plus / B-minus share cell {0,1}; A-A is {1,1}."""
    rng, a, b, c, d = _four(6104)
    seqs = [_seq(rng, 400, [(40, c, c)]), _seq(rng, 400, [(60, a, c)]), _seq(rng, 400, [(50, c, b)]), _seq(rng, 400, [(70, a, a)])]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(c), w(c)), (w(a), w(b))], thr=0.95, select="all")


@functools.lru_cache(None)
def counts_case(oracle):
    """Rows (A, B), (C, D).  Sequence 0: two A-plus / C-minus products (two minus sites) and, further on, a B-plus / D-minus
    product -- another oligo pair of the same cell on the same sequence; sequence 1: one A-plus / C-minus product.  Cell {0,1}:
    4 products on 2 sequences."""
    rng, a, b, c, d = _four(6105)
    s0 = _seq(rng, 700, [(40, a, c), (400, b, d)])
    s0 = plant(s0, 40 + 150, revcomp(c))
    seqs = [s0, _seq(rng, 400, [(60, a, c)])]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(a), w(b)), (w(c), w(d))], thr=0.95, select="all")


TIE_SEQS = (1, 3)


@functools.lru_cache(None)
def tie_case(oracle):
    """Rows (A, B), (C, D).  Sequence 0 holds an A-plus / C-minus product with a substitution in the plus site (at 0.8: a weaker
    site), sequences 1 and 3 are the same text with the exact product, sequence 2 has none: melt is attained on 1 and 3, the
    lower is reported."""
    rng, a, b, c, d = _four(6106)
    exact = _seq(rng, 400, [(60, a, c)])
    seqs = [_seq(rng, 400, [(40, _sub(a, (9,)), c)]), exact, rand_seq(rng, 400), exact]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(a), w(b)), (w(c), w(d))], thr=float(np.sqrt(np.float32(0.8))), select="all")


WIDE_N = 130
WIDE_PRODUCT = (63, 64, 128)
WIDE_INACTIVE = 65


@functools.lru_cache(None)
def wide_case(oracle):
    """130 sequences; A-plus / C-minus products on sequences 63, 64 and 128 (three u64 words of a bitset, were there one), and
    on the inactive sequence 65, which takes no part."""
    rng, a, b, c, d = _four(6107)
    seqs = [_seq(rng, 300, [(50, a, c)]) if i in WIDE_PRODUCT + (WIDE_INACTIVE,) else rand_seq(rng, 300) for i in range(WIDE_N)]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(a), w(b)), (w(c), w(d))], thr=0.95, select="all",
                active=tuple(i != WIDE_INACTIVE for i in range(WIDE_N)))


def _cross_split(oracle, splits):
    """site_tm_cases.split_case with its two oligos in different rows: (Q, X), (Y, R).  The Q-plus / R-minus products are
    spurious and lie in cell {0,1}."""
    base = SC.split_case(oracle)
    rng = random.Random(6108)
    w = oracle.centered_word
    q, r = base["panel"][0]
    return dict(base, panel=[(q, w(_primer(rng, 21))), (w(_primer(rng, 20)), r)], splits=splits, amp=PC.SPLIT_AMP)


def cross_split_wide_case(oracle):
    """The split at 110 is outside the inner stretch: both sequences carry a product."""
    return _cross_split(oracle, [(0, 110)])


def cross_split_inner_case(oracle):
    """The split at 200 is inside the inner stretch of sequence 0: only sequence 1 carries a product."""
    return _cross_split(oracle, [(0, 200)])


FANIN_N = 300


@functools.lru_cache(None)
def fanin_case(oracle):
    """300 identical sequences with one A-plus / C-minus product each: one cell, fed by the threads of several workgroups."""
    rng, a, b, c, d = _four(6109)
    s = _seq(rng, 300, [(50, a, c)])
    w = oracle.centered_word
    return dict(seqs=[s] * FANIN_N, panel=[(w(a), w(b)), (w(c), w(d))], thr=0.95, select="all")


POOL40_ROWS = 40
POOL40_THR = 0.76


@functools.lru_cache(None)
def pool40_case(oracle):
    """40 rows sampled from 8 sequences x 1.2 kb in two families, every site at float32(0.76) squared; rows 5 and 20 share
    their forward primer with row 0, row 30 is row 1 exchanged."""
    rng = random.Random(6110)
    seqs = family_targets(rng, 2, 4, 1200, div=0.04)
    txt = []
    while len(txt) < POOL40_ROWS:
        p = sample_pair(rng, rng.choice(seqs))
        if p:
            txt.append(p)
    txt[5] = (txt[0][0], txt[5][1])
    txt[20] = (txt[0][0], txt[20][1])
    txt[30] = (txt[1][1], txt[1][0])
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(f), w(r)) for f, r in txt], thr=POOL40_THR, select="all")


_BUILDERS = {"c_shared": shared_case, "c_roles": roles_case, "c_repeat": repeat_case, "c_self_pair": self_pair_case,
             "c_counts": counts_case, "c_tie": tie_case, "c_wide": wide_case, "c_split_wide": cross_split_wide_case,
             "c_split_inner": cross_split_inner_case, "c_fanin": fanin_case, "c_pool40": pool40_case}
GROUPING_SCENARIOS = tuple(_BUILDERS)
SMALL_SCENARIOS = tuple(n for n in GROUPING_SCENARIOS if n != "c_pool40")


def scenario(oracle, name):
    """name -> scenario, registered with products_tm_cases (its scenarios pass through)."""
    if name in _BUILDERS and name not in PC._CASES:
        PC.register(name, _BUILDERS[name](oracle))
    return PC.scenario(oracle, name)


ALL_SCENARIOS = PC.SCENARIO_NAMES + GROUPING_SCENARIOS
